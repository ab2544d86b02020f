"""Numpy restatement of the two rules of DESIGN.md §18, for the tests: CTC prefix beam search (``beam_search``) and the forced Viterbi
alignment of a labelling (``align``), in a selectable dtype (float64: the reference; float32: the arithmetic of csrc/ctc_beam.hip up to the
hardware exp2 / log2), a brute-force scorer (``ctc_log_likelihood``, the CTC forward in float64; ``best_labellings`` over every labelling)
and the input generators of tests/test_beam_gpu.py, so that the host tests assert the skipped-share caps for exactly those inputs.

The rule.  Per sample, over steps t < min(in_len, T); class 0 is the blank; W prefixes.  A beam entry is a prefix node (parent node, label,
step of creation) with lb / lnb, the log-masses of its alignments ending in blank / in its last label e; total = logaddexp(lb, lnb).  The
beam starts as the empty prefix with lb = 0, lnb = -inf.  At step t entry p of slot i produces, in this order:
  stay      lb' = total + lp[t,0]; lnb' = lnb + lp[t,e] (-inf for the empty prefix), to which the entry q with q + e = p, if it is in the
            beam, adds (q.lb if q.last == e else q.total) + lp[t,e] by logaddexp
  extend c  for c = 1..C-1 ascending unless p + c is itself in the beam: lnb' = (lb if c == e else total) + lp[t,c]; lb' = -inf
Candidates with total -inf do not exist.  The W largest totals survive in descending order; equal totals in candidate order (slot, stay
before extend, label).  The answer is slot 0 after the last step: labelling and total (in_len 0: empty, 0.0; nothing survived: empty, -inf).
"""
from __future__ import annotations

import itertools

import numpy as np

NEG = -np.inf


def beam_search(lp, in_len, W, dtype=np.float64):
    """lp (T, C) log-probs of one sample -> dict ``labels``, ``score``, ``gap`` (total of slot 0 minus total of slot 1 after the last step;
    inf with one entry) and ``prune_gap`` (the smallest, over the steps that pruned, of: best surviving total among the prefixes of the
    answer minus the first pruned total; inf if nothing was pruned), all arithmetic in ``dtype``.  The candidates of a step are laid out as
    a (slots, C) matrix in candidate order -- column 0 the stay, column c the extension by c -- and ranked by a stable sort."""
    lp = np.asarray(lp, dtype=dtype)
    T, C = lp.shape
    Ti = max(0, min(int(in_len), T))
    nodes = [(-1, 0, -1)]  # (parent node, label, step of creation)
    node, par, last = [0], [-1], np.zeros(1, dtype=np.int64)
    lb, lnb = np.zeros(1, dtype=dtype), np.full(1, NEG, dtype=dtype)
    history = []  # per step: (survivors' nodes, their totals, first pruned total or None)
    for t in range(Ti):
        row, nb = lp[t], len(node)
        tot = np.logaddexp(lb, lnb)
        slot_of = {x: i for i, x in enumerate(node)}
        qs = [slot_of.get(x) for x in par]
        cand = np.where(np.arange(C)[None, :] == last[:, None], lb[:, None], tot[:, None]) + row[None, :]  # the extensions
        st_lb = tot + row[0]
        st_lnb = np.where(last == 0, np.asarray(NEG, dtype=dtype), lnb + row[last])
        for i, q in enumerate(qs):
            if q is not None:  # the merge: q + e = p, so q's extension by e is p's mass and no candidate of its own
                e = last[i]
                st_lnb[i] = np.logaddexp(st_lnb[i], (lb[q] if last[q] == e else tot[q]) + row[e])
                cand[q, e] = NEG
        cand[:, 0] = np.logaddexp(st_lb, st_lnb)
        flat = cand.reshape(-1)
        order = np.argsort(-flat, kind="stable")  # ties in candidate order
        order = order[:int((flat > NEG).sum())]
        keep = order[:W]
        n_node, n_par, n_last, n_lb, n_lnb = [], [], [], [], []
        for k in keep.tolist():
            i, c = divmod(k, C)
            if c == 0:
                n_node.append(node[i]), n_par.append(par[i]), n_last.append(last[i]), n_lb.append(st_lb[i]), n_lnb.append(st_lnb[i])
            else:
                n_node.append(len(nodes)), n_par.append(node[i]), n_last.append(c), n_lb.append(NEG), n_lnb.append(flat[k])
                nodes.append((node[i], c, t))
        history.append((n_node, flat[keep], flat[order[W]] if len(order) > W else None))
        node, par, last = n_node, n_par, np.asarray(n_last, dtype=np.int64)
        lb, lnb = np.asarray(n_lb, dtype=dtype), np.asarray(n_lnb, dtype=dtype)
    if not node:
        return dict(labels=[], score=float(NEG), gap=float("inf"), prune_gap=float("inf"))
    labels, x, chain = [], node[0], {0}
    while x > 0:
        chain.add(x)
        labels.append(nodes[x][1])
        x = nodes[x][0]
    totals = np.logaddexp(lb, lnb)
    prune_gap = float("inf")
    for surv, vals, pruned in history:
        anc = [float(v) for nd, v in zip(surv, vals) if nd in chain]
        if pruned is not None and anc:
            prune_gap = min(prune_gap, max(anc) - float(pruned))
    return dict(labels=labels[::-1], score=float(totals[0]), gap=float(totals[0] - totals[1]) if len(node) > 1 else float("inf"), prune_gap=prune_gap)


def align(lp, in_len, labels, dtype=np.float64):
    """Forced alignment of ``labels`` on lp (T, C): over ext = [0, l1, 0, ..., lL, 0], d[0][0] = lp[0,0], d[0][1] = lp[0,l1], d[t][s] = lp[t,
    ext[s]] + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2]) -- the last only if ext[s] != 0 and ext[s] != ext[s-2] -- ties in that order; the
    path ends in the better of states 2L and 2L-1, 2L on a tie.  -> dict ``lens`` (-1: no alignment of finite score, nothing else), ``t0``,
    ``t1``, ``peak`` (the input's own values), ``states`` (the path) and ``score``."""
    dt = np.dtype(dtype).type
    src = np.asarray(lp)
    lp = src.astype(dtype)
    T, C = lp.shape
    Ti, L = max(0, min(int(in_len), T)), len(labels)
    if L == 0 and Ti == 0:
        return dict(lens=0, t0=[], t1=[], peak=[], states=[], score=0.0)
    if L > Ti or any(not 1 <= l < C for l in labels):
        return dict(lens=-1)
    ext = [0]
    for l in labels:
        ext += [int(l), 0]
    S = len(ext)
    d = np.full(S, NEG, dtype=dtype)
    d[0] = lp[0, 0]
    if S > 1:
        d[1] = lp[0, ext[1]]
    back = np.zeros((Ti, S), dtype=np.int8)
    for t in range(1, Ti):
        nd = np.full(S, NEG, dtype=dtype)
        for s in range(S):
            v, b = d[s], 0
            if s >= 1 and d[s - 1] > v:
                v, b = d[s - 1], 1
            if s >= 2 and ext[s] != 0 and ext[s] != ext[s - 2] and d[s - 2] > v:
                v, b = d[s - 2], 2
            nd[s], back[t, s] = dt(lp[t, ext[s]] + v), b
        d = nd
    e2, e1 = d[S - 1], d[S - 2] if L > 0 else dt(NEG)
    s = S - 2 if e1 > e2 else S - 1
    if not max(e1, e2) > NEG:
        return dict(lens=-1)
    score, states = float(max(e1, e2)), []
    for t in range(Ti - 1, -1, -1):
        states.append(s)
        s -= int(back[t, s])
    states = states[::-1]
    t0, t1, peak = [None] * L, [None] * L, [None] * L
    for t, s in enumerate(states):
        if s & 1:
            k = s >> 1
            if t0[k] is None:
                t0[k], peak[k] = t, src[t, ext[s]]
            t1[k], peak[k] = t, max(peak[k], src[t, ext[s]])
    return dict(lens=L, t0=t0, t1=t1, peak=peak, states=states, score=score)


def path_score(lp, labels, t0, t1):
    """float64 sum of lp along the state sequence that spans t0 / t1 describe (blank wherever no character is)"""
    lp = np.asarray(lp, dtype=np.float64)
    cls = np.zeros(lp.shape[0], dtype=np.int64)
    for l, a, b in zip(labels, t0, t1):
        cls[a:b + 1] = l
    return float(lp[np.arange(len(cls)), cls].sum()), cls


# ---- brute force ---------------------------------------------------------------------------------------------------------------------------
def ctc_log_likelihood(lp, labels):
    """log p(labels | lp) by the CTC forward recursion in float64 (all T steps)"""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext = [0]
    for l in labels:
        ext += [int(l), 0]
    S = len(ext)
    a = np.full(S, NEG)
    a[0] = lp[0, 0]
    if S > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, T):
        n = np.full(S, NEG)
        for s in range(S):
            terms = [a[s]]
            if s >= 1:
                terms.append(a[s - 1])
            if s >= 2 and ext[s] != 0 and ext[s] != ext[s - 2]:
                terms.append(a[s - 2])
            m = max(terms)
            n[s] = NEG if m == NEG else m + np.log(sum(np.exp(x - m) for x in terms)) + lp[t, ext[s]]
        a = n
    tail = [a[S - 1]] + ([a[S - 2]] if S > 1 else [])
    m = max(tail)
    return float(NEG) if m == NEG else float(m + np.log(sum(np.exp(x - m) for x in tail)))


def all_labellings(C, T):
    """every labelling of at most T labels from 1..C-1 (feasible or not)"""
    out = [()]
    for n in range(1, T + 1):
        out += list(itertools.product(range(1, C), repeat=n))
    return out


def best_labellings(lp):
    """(best labelling, its float64 log-likelihood, gap to the second best) over every labelling"""
    T, C = np.asarray(lp).shape
    scored = sorted(((ctc_log_likelihood(lp, l), l) for l in all_labellings(C, T)), key=lambda x: -x[0])
    return list(scored[0][1]), scored[0][0], scored[0][0] - scored[1][0]


def best_path(lp, labels):
    """the best alignment score of ``labels`` over every path of T states (exhaustive; small T only), -inf if none"""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    best = NEG
    for path in itertools.product(range(C), repeat=T):
        out, last = [], None
        for c in path:
            if c != last and c != 0:
                out.append(c)
            last = c
        if out == list(labels):
            best = max(best, float(lp[np.arange(T), list(path)].sum()))
    return best


# ---- the inputs of tests/test_beam_gpu.py ----------------------------------------------------------------------------------------------------
def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


EXHAUSTIVE_SHAPES = ((3, 5, 64), (2, 7, 8), (3, 4, 32), (4, 3, 64))  # (C, T, W): W >= the number of prefixes
EXHAUSTIVE_CASES, EXHAUSTIVE_MIN_GAP, EXHAUSTIVE_MAX_SKIP = 50, 1e-4, 0.05
PRUNED_SHAPES = ((12, 24, 8, 12.0), (97, 40, 16, 14.0), (97, 70, 32, 14.0), (5, 33, 4, 10.0))  # (C, T, W, J)
PRUNED_CASES, PRUNED_MIN_MARGIN, PRUNED_MAX_SKIP = 40, 1e-3, 0.10


def exhaustive_inputs(C, T, seed=0):
    """(N, T, C) float32 log-probs: log_softmax(2 N(0,1))"""
    rng = np.random.default_rng([seed, C, T])
    return log_softmax(2.0 * rng.standard_normal((EXHAUSTIVE_CASES, T, C))).astype(np.float32)


def peaky_inputs(C, T, J, seed=0, cases=PRUNED_CASES):
    """(N, T, C) float32 log-probs shaped like a trained recogniser's, and mixed input lengths (N,): every logit -J + N(0,1), a random
    run-length path (runs of 1 to 3 steps) at 0, with probability 0.35 per step one random class at U(-1.5, 0.5); then log_softmax"""
    rng = np.random.default_rng([seed, C, T, 1])
    x = -J + rng.standard_normal((cases, T, C))
    for n in range(cases):
        t = 0
        while t < T:
            c, run = int(rng.integers(0, C)), int(rng.integers(1, 4))
            x[n, t:t + run, c] = 0.0
            t += run
        for t in range(T):
            if rng.random() < 0.35:
                x[n, t, int(rng.integers(0, C))] = rng.uniform(-1.5, 0.5)
    in_len = rng.integers(T // 2, T + 1, size=cases)
    in_len[:2] = T
    return log_softmax(x).astype(np.float32), in_len.astype(np.int64)


def score_bound(T, score64):
    """|score - score64| allowed to an fp32 beam of T steps: three roundings at the running magnitude and one logaddexp per step"""
    return T * (3.0 * 2.0 ** -24 * max(1.0, abs(score64)) + 1e-6)


def greedy(lp, in_len):
    lp = np.asarray(lp)
    out, last = [], None
    for c in lp[:max(0, min(int(in_len), lp.shape[0]))].argmax(axis=1).tolist():
        if c != last and c != 0:
            out.append(c)
        last = c
    return out

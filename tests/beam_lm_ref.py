"""Numpy restatement of DESIGN.md §19 for the tests: CTC prefix beam search with a character n-gram gain table fused into the ranking
(``beam_search_lm``), in a selectable dtype (float64: the reference; float32: the arithmetic of csrc/ctc_beam.hip's LM form up to the hardware
exp2 / log2), the brute-force arg-max of log-likelihood + gains over every labelling (``best_labellings_lm``) and the tables and cases of
tests/test_beam_lm_gpu.py, so that the host tests assert the skipped-share caps for exactly those inputs.

The rule.  Everything of tests/beam_ref.py's rule holds for the CTC numbers lb / lnb / total, the suppression and the merges.  A gain table G
is a float32 array of shape (C,) * order, order 1..3: G[ctx..., c] is the credit for appending label c after the last order - 1 labels of the
prefix, padded on the left with 0.  Every beam entry also has lm (the sum of its labels' gains, in ``dtype``, added in the labels' order)
and last2, the label before its last (0 if none).  The empty prefix has lm = 0.
  stay      lm' = lm; rank = stay total + lm
  extend c  lm' = lm + G[ctx, c]; rank = lnb' + lm'
A candidate exists iff its CTC total and its rank are both > -inf.  The W largest ranks survive in descending order; equal ranks in candidate
order.  The answer is slot 0 after the last step: labelling, its CTC total (``score``) and its lm (``lm_score``); in_len 0: empty, 0.0, 0.0;
nothing survived: empty, -inf, 0.0.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import beam_ref as B

NEG = -np.inf


def context_rows(G, last, last2):
    """(slots, C) rows of G for the slots' contexts"""
    if G.ndim == 1:
        return np.broadcast_to(G, (len(last), G.shape[0]))
    return G[last] if G.ndim == 2 else G[last2, last]


def beam_search_lm(lp, in_len, W, gain, dtype=np.float64):
    """lp (T, C) log-probs of one sample, gain the float32 table -> dict ``labels``, ``score``, ``lm_score``, ``gap`` (rank of slot 0 minus
    rank of slot 1 after the last step; inf with one entry) and ``prune_gap`` (the smallest, over the steps that pruned, of: best surviving
    rank among the prefixes of the answer minus the first pruned rank; inf if nothing was pruned), all arithmetic in ``dtype``."""
    lp = np.asarray(lp, dtype=dtype)
    G = np.asarray(gain, dtype=np.float32).astype(dtype)
    T, C = lp.shape
    assert G.shape == (C,) * G.ndim and 1 <= G.ndim <= 3
    Ti = max(0, min(int(in_len), T))
    nodes = [(-1, 0, -1)]  # (parent node, label, step of creation)
    node, par, last, last2 = [0], [-1], np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    lb, lnb, lm = np.zeros(1, dtype=dtype), np.full(1, NEG, dtype=dtype), np.zeros(1, dtype=dtype)
    history = []  # per step: (survivors' nodes, their ranks, first pruned rank or None)
    for t in range(Ti):
        row = lp[t]
        tot = np.logaddexp(lb, lnb)
        slot_of = {x: i for i, x in enumerate(node)}
        qs = [slot_of.get(x) for x in par]
        cand = np.where(np.arange(C)[None, :] == last[:, None], lb[:, None], tot[:, None]) + row[None, :]  # the extensions' CTC totals
        st_lb = tot + row[0]
        st_lnb = np.where(last == 0, np.asarray(NEG, dtype=dtype), lnb + row[last])
        for i, q in enumerate(qs):
            if q is not None:  # the merge: q + e = p, so q's extension by e is p's mass and no candidate of its own
                e = last[i]
                st_lnb[i] = np.logaddexp(st_lnb[i], (lb[q] if last[q] == e else tot[q]) + row[e])
                cand[q, e] = NEG
        cand[:, 0] = np.logaddexp(st_lb, st_lnb)
        with np.errstate(invalid="ignore"):
            lm_new = lm[:, None] + context_rows(G, last, last2)  # one add per extension
            lm_new[:, 0] = lm                                    # column 0 of the table is never read: the stay keeps lm
            rank = cand + lm_new                                 # one add
        exists = (cand > NEG) & (rank > NEG)
        flat = np.where(exists, rank, np.asarray(NEG, dtype=dtype)).reshape(-1)
        order = np.argsort(-flat, kind="stable")  # ties in candidate order
        order = order[:int(exists.sum())]
        keep = order[:W]
        n_node, n_par, n_last, n_last2, n_lb, n_lnb, n_lm = [], [], [], [], [], [], []
        for k in keep.tolist():
            i, c = divmod(k, C)
            n_lm.append(lm_new[i, c])
            if c == 0:
                n_node.append(node[i]), n_par.append(par[i]), n_last.append(last[i]), n_last2.append(last2[i])
                n_lb.append(st_lb[i]), n_lnb.append(st_lnb[i])
            else:
                n_node.append(len(nodes)), n_par.append(node[i]), n_last.append(c), n_last2.append(last[i])
                n_lb.append(NEG), n_lnb.append(cand[i, c])
                nodes.append((node[i], c, t))
        history.append((n_node, flat[keep], flat[order[W]] if len(order) > W else None))
        node, par = n_node, n_par
        last, last2 = np.asarray(n_last, dtype=np.int64), np.asarray(n_last2, dtype=np.int64)
        lb, lnb, lm = np.asarray(n_lb, dtype=dtype), np.asarray(n_lnb, dtype=dtype), np.asarray(n_lm, dtype=dtype)
    if not node:
        return dict(labels=[], score=float(NEG), lm_score=0.0, gap=float("inf"), prune_gap=float("inf"))
    labels, x, chain = [], node[0], {0}
    while x > 0:
        chain.add(x)
        labels.append(nodes[x][1])
        x = nodes[x][0]
    totals = np.logaddexp(lb, lnb)
    ranks = totals + lm
    prune_gap = float("inf")
    for surv, vals, pruned in history:
        anc = [float(v) for nd, v in zip(surv, vals) if nd in chain]
        if pruned is not None and anc:
            prune_gap = min(prune_gap, max(anc) - float(pruned))
    return dict(labels=labels[::-1], score=float(totals[0]), lm_score=float(lm[0]),
                gap=float(ranks[0] - ranks[1]) if len(node) > 1 else float("inf"), prune_gap=prune_gap)


def gains_of(labels, gain):
    """the float32 table entries a labelling collects, in the labels' order"""
    G = np.asarray(gain, dtype=np.float32)
    ctx, out = [0] * (G.ndim - 1), []
    for c in labels:
        out.append(G[tuple(ctx) + (int(c),)])
        ctx = (ctx + [int(c)])[1:] if G.ndim > 1 else ctx
    return out


def lm_sum(labels, gain):
    """float64 sum of ``gains_of``"""
    return float(np.sum(np.asarray(gains_of(labels, gain), dtype=np.float64))) if len(labels) else 0.0


def lm_bound(labels, gain):
    """|lm_score - lm64| allowed to an fp32 sum: L adds at a running magnitude of at most sum |g_k|"""
    g = np.asarray(gains_of(labels, gain), dtype=np.float64)
    return len(g) * 2.0 ** -24 * max(1.0, float(np.abs(g).sum()))


# ---- brute force ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exhaustive_likelihoods(C, T):
    """(labellings, (cases, labellings) float64 CTC log-likelihoods) of ``B.exhaustive_inputs(C, T)``: shared by the orders and the tests"""
    lp = B.exhaustive_inputs(C, T)
    labellings = B.all_labellings(C, T)
    return labellings, np.asarray([[B.ctc_log_likelihood(x, l) for l in labellings] for x in lp])


def best_labellings_lm(C, T, gain):
    """per case of ``B.exhaustive_inputs(C, T)``: (best labelling, its log-likelihood + gains in float64, gap to the second best, its
    log-likelihood alone)"""
    labellings, ll = exhaustive_likelihoods(C, T)
    total = ll + np.asarray([lm_sum(l, gain) for l in labellings])[None, :]
    out = []
    for row in total:
        k = np.argsort(-row, kind="stable")
        out.append((list(labellings[k[0]]), float(row[k[0]]), float(row[k[0]] - row[k[1]]), float(ll[len(out), k[0]])))
    return out


# ---- the tables and cases of tests/test_beam_lm_gpu.py ---------------------------------------------------------------------------------------
ORDERS = (1, 2, 3)
GAIN_SEED, GAIN_WEIGHT, GAIN_BONUS = 0, 0.7, 0.5


def random_gain(C, order, seed=GAIN_SEED):
    """float32 (C,) * order: logits 1.5 N(0,1), log-softmax over c >= 1 (column 0: -inf before the scaling), 0.7 logP + 0.5"""
    rng = np.random.default_rng([seed, C, order, 2])
    x = 1.5 * rng.standard_normal((C,) * order)
    logp = np.full(x.shape, NEG)
    logp[..., 1:] = B.log_softmax(x[..., 1:])
    return (GAIN_WEIGHT * logp + GAIN_BONUS).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pruned_reference(k, order, dtype_name="float64"):
    """pruned shape k with ``random_gain``: (lp, in_len, gain, [beam_search_lm per case]); computed once per process and not to be changed"""
    C, T, W, J = B.PRUNED_SHAPES[k]
    lp, in_len = B.peaky_inputs(C, T, J)
    gain = random_gain(C, order)
    return lp, in_len, gain, [beam_search_lm(x, il, W, gain, np.dtype(dtype_name).type) for x, il in zip(lp, in_len)]


@functools.lru_cache(maxsize=None)
def plain_reference(k):
    """the plain beam of tests/beam_ref.py on pruned shape k"""
    C, T, W, J = B.PRUNED_SHAPES[k]
    lp, in_len = B.peaky_inputs(C, T, J)
    return [B.beam_search(x, il, W) for x, il in zip(lp, in_len)]

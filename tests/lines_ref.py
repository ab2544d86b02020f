"""CPU restatement of the text-line rule in plain numpy, for the tests of csrc/text_lines.hip.  Written once with a dtype
parameter: in float32 every operation is the kernel's, in the kernel's order, with one rounding each; in float64 it is the comparand for
inputs whose comparisons are away from their thresholds.  Nothing here calls the package's kernels.

The rule.  Input: word quads (N,4,2) float32, pixel-centre coordinates.

* Word frame (the axes ``crop_frame`` chooses).  u = unit vector of the longer of the sides c0->c1 and c1->c2; on a tie the side with the
  larger |x| component (the first if that ties too); signed so that u.x > 0, or u.x == 0 and u.y > 0; a point gets (1, 0).  v = (-u.y, u.x).
  lng, sht = the two side lengths.  Centre c = 0.25 * ((x0 + x1) + (x2 + x3)), likewise y.
* Candidate successor j of i, with d = c_j - c_i, s = d.u_i, t = d.v_i: s > 0; |t| <= 0.5 * min(sht_i, sht_j);
  (s - 0.5 * lng_i) - 0.5 * lng_j <= max_gap * max(sht_i, sht_j); u_i.u_j >= min_cos; d.x > 0, or d.x == 0 and d.y > 0.
* Choice.  next(i) = the candidate with the smallest s, ties: the smallest j.
* Acceptance.  j accepts, among the k with next(k) == j, the one with the smallest s_kj, ties: the smallest k.  A link is chosen AND accepted.
* Lines = maximal chains, words in chain order; lines sorted by their head's (c.y, c.x, word index).
* Line quad.  One word: that quad.  Otherwise u_L = normalise(sum of lng_i * u_i in chain order), v_L = (-u_L.y, u_L.x); all corners are
  projected on u_L, v_L; the corners are (minU,minV), (maxU,minV), (maxU,maxV), (minU,maxV) mapped back to the page.
"""
from __future__ import annotations

import numpy as np

MAX_GAP, MIN_COS = 2.0, 0.9


def ulp32(x: float) -> float:
    """spacing of fp32 numbers at |x|"""
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------------------ the rule -------------------------------------------------------------
def word_frames(quads, dtype=np.float32) -> dict:
    """cx, cy, ux, uy, lng, sht, each (N,) in ``dtype``"""
    T = dtype
    q = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2).astype(T)
    x, y = q[:, :, 0], q[:, :, 1]
    e1x, e1y, e2x, e2y = x[:, 1] - x[:, 0], y[:, 1] - y[:, 0], x[:, 2] - x[:, 1], y[:, 2] - y[:, 1]
    l1, l2 = np.sqrt(e1x * e1x + e1y * e1y), np.sqrt(e2x * e2x + e2y * e2y)
    first = (l1 > l2) | ((l1 == l2) & (np.abs(e1x) >= np.abs(e2x)))
    lng, sht = np.where(first, l1, l2), np.where(first, l2, l1)
    ex, ey = np.where(first, e1x, e2x), np.where(first, e1y, e2y)
    pos = lng > 0
    safe = np.where(pos, lng, T(1))
    ux, uy = np.where(pos, ex / safe, T(1)), np.where(pos, ey / safe, T(0))
    flip = (ux < 0) | ((ux == 0) & (uy < 0))
    ux, uy = np.where(flip, -ux, ux), np.where(flip, -uy, uy)
    cx = T(0.25) * ((x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3]))
    cy = T(0.25) * ((y[:, 0] + y[:, 1]) + (y[:, 2] + y[:, 3]))
    return {k: v.astype(T) for k, v in dict(cx=cx, cy=cy, ux=ux, uy=uy, lng=lng, sht=sht).items()}


def pair_terms(f: dict, i: int, max_gap, min_cos, T) -> dict:
    """the five comparisons of word i against every word j, as (left side, right side) pairs the way the kernel forms them"""
    dx, dy = f["cx"] - f["cx"][i], f["cy"] - f["cy"][i]
    uxi, uyi = f["ux"][i], f["uy"][i]
    s = dx * uxi + dy * uyi
    t = dx * (-uyi) + dy * uxi
    gap = (s - T(0.5) * f["lng"][i]) - T(0.5) * f["lng"]
    cs = uxi * f["ux"] + uyi * f["uy"]
    return dict(s=s, t=t, gap=gap, cs=cs, dx=dx, dy=dy, half=T(0.5) * np.minimum(f["sht"][i], f["sht"]), reach=T(max_gap) * np.maximum(f["sht"][i], f["sht"]),
                min_cos=T(min_cos))


def candidates(p: dict) -> np.ndarray:
    return (p["s"] > 0) & (np.abs(p["t"]) <= p["half"]) & (p["gap"] <= p["reach"]) & (p["cs"] >= p["min_cos"]) & ((p["dx"] > 0) | ((p["dx"] == 0) & (p["dy"] > 0)))


def find_links(f: dict, max_gap=MAX_GAP, min_cos=MIN_COS, dtype=np.float32) -> np.ndarray:
    """next_word (N,) int: the linked successor of every word, or -1"""
    T = dtype
    n = len(f["cx"])
    chosen, s_of = np.full(n, -1), np.zeros(n, dtype=T)
    for i in range(n):
        p = pair_terms(f, i, max_gap, min_cos, T)
        cand = candidates(p)
        if cand.any():
            j = int(np.argmin(np.where(cand, p["s"], T(np.inf))))  # the first of equal minima: the smallest j
            chosen[i], s_of[i] = j, p["s"][j]
    nxt = np.full(n, -1)
    for j in range(n):
        ks = np.nonzero(chosen == j)[0]
        if len(ks):
            k = min(ks.tolist(), key=lambda k: (s_of[k], k))
            nxt[k] = j
    return nxt


def find_lines(quads, max_gap=MAX_GAP, min_cos=MIN_COS, dtype=np.float32) -> dict:
    """next_word, line_of_word, word_order (N,), line_offsets (L+1,), n_lines, quads (L,4,2) in ``dtype``, lines (list of index lists)"""
    T = dtype
    q32 = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    n = len(q32)
    f = word_frames(q32, T)
    nxt = find_links(f, max_gap, min_cos, T) if n else np.zeros(0, dtype=int)
    has_pred = np.zeros(n, dtype=bool)
    has_pred[nxt[nxt >= 0]] = True
    heads = sorted((i for i in range(n) if not has_pred[i]), key=lambda h: (f["cy"][h], f["cx"][h], h))
    lines = []
    for h in heads:
        chain = [h]
        while nxt[chain[-1]] >= 0:
            chain.append(int(nxt[chain[-1]]))
        lines.append(chain)
    line_of_word = np.full(n, -1)
    for l, chain in enumerate(lines):
        line_of_word[chain] = l
    offsets = np.cumsum([0] + [len(c) for c in lines])
    out = np.zeros((len(lines), 4, 2), dtype=T)
    for l, chain in enumerate(lines):
        out[l] = line_quad(q32, f, chain, T)
    return {"next_word": nxt, "line_of_word": line_of_word, "word_order": np.array([i for c in lines for i in c], dtype=int), "line_offsets": offsets,
            "n_lines": len(lines), "quads": out, "lines": lines}


def line_quad(q32, f, chain, T):
    if len(chain) == 1:
        return q32[chain[0]].astype(T)
    sx, sy = T(0), T(0)
    for w in chain:
        sx, sy = sx + f["lng"][w] * f["ux"][w], sy + f["lng"][w] * f["uy"][w]
    norm = np.sqrt(sx * sx + sy * sy)
    ux, uy = (sx / norm, sy / norm) if norm > 0 else (T(1), T(0))
    vx, vy = -uy, ux
    pts = q32[chain].astype(T).reshape(-1, 2)
    pu, pv = pts[:, 0] * ux + pts[:, 1] * uy, pts[:, 0] * vx + pts[:, 1] * vy
    lo_u, hi_u, lo_v, hi_v = pu.min(), pu.max(), pv.min(), pv.max()
    return np.array([[a * ux + b * vx, a * uy + b * vy] for a, b in ((lo_u, lo_v), (hi_u, lo_v), (hi_u, hi_v), (lo_u, hi_v))], dtype=T)


def decision_margin(quads, max_gap=MAX_GAP, min_cos=MIN_COS) -> float:
    """How far (in pixels, float64) the input keeps every decision of the rule from flipping: for each ordered pair the candidate test must
    hold in all five comparisons, or fail in at least one, by the margin; the two nearest candidates of a word, the two nearest choosers of a
    word, and the sort keys c.y of two line heads must differ by it.  The cosine's margin is scaled by 100 to be comparable."""
    T = np.float64
    f = word_frames(quads, T)
    n = len(f["cx"])
    worst = np.inf
    chosen, s_of = np.full(n, -1), np.zeros(n)
    for i in range(n):
        p = pair_terms(f, i, max_gap, min_cos, T)
        m = np.minimum.reduce([p["s"], p["half"] - np.abs(p["t"]), p["reach"] - p["gap"], 100 * (p["cs"] - p["min_cos"]),
                               np.where(p["dx"] != 0, p["dx"], p["dy"])])
        m[i] = -np.inf  # (a word is no candidate of itself: s == 0 exactly)
        worst = min(worst, np.abs(m).min())
        ss = np.sort(p["s"][m > 0])
        if len(ss):
            chosen[i], s_of[i] = int(np.argmin(np.where(m > 0, p["s"], np.inf))), ss[0]
        if len(ss) > 1:
            worst = min(worst, ss[1] - ss[0])
    for j in range(n):
        ss = np.sort(s_of[chosen == j])
        if len(ss) > 1:
            worst = min(worst, ss[1] - ss[0])
    r = find_lines(quads, max_gap, min_cos, T)
    ys = np.sort([f["cy"][c[0]] for c in r["lines"]])
    if len(ys) > 1:
        worst = min(worst, np.diff(ys).min())
    return float(worst)


# ------------------------------------------------------------------ cases ----------------------------------------------------------------
def box(x, y, w, h) -> np.ndarray:
    """axis-aligned word, corners clockwise from the top left"""
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float32)


def rotated_rect(cx, cy, long, short, deg) -> np.ndarray:
    t = np.deg2rad(deg)
    u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
    c = np.array([cx, cy], dtype=np.float64)
    return np.array([c - long / 2 * u - short / 2 * v, c + long / 2 * u - short / 2 * v, c + long / 2 * u + short / 2 * v, c - long / 2 * u + short / 2 * v]).astype(np.float32)


def row_of_words(x, y, n, w=60, h=20, gap=20) -> list:
    return [box(x + k * (w + gap), y, w, h) for k in range(n)]


def case_row_gap_row():
    """three words on a row, a gap of 4 h, two more: lines [0, 1, 2] and [3, 4]"""
    return np.stack(row_of_words(0, 0, 3) + row_of_words(2 * 80 + 60 + 80, 0, 2)), [[0, 1, 2], [3, 4]]


def case_competing():
    """words 0 and 1 both choose word 2; 1 is nearer (s = 70 against 90) and wins, 0 stays alone"""
    return np.stack([box(0, 0, 60, 20), box(20, 16, 60, 20), box(90, 8, 60, 20)]), [[0], [1, 2]]


def case_accept_tie():
    """words 0 and 1 both choose word 2 at s = 90: the smaller index wins"""
    return np.stack([box(0, 0, 60, 20), box(0, 16, 60, 20), box(90, 8, 60, 20)]), [[0, 2], [1]]


def case_choice_tie(swap=False):
    """word 2 (c.y = 20) has two candidates at s = 90, one 6 above and one 6 below its baseline: it chooses index 0, whichever of the two
    that is; the other one is a line of its own, sorted by its c.y (14 or 26) against 20"""
    above, below = box(90, 4, 60, 20), box(90, 16, 60, 20)
    if swap:
        return np.stack([below, above, box(0, 10, 60, 20)]), [[1], [2, 0]]
    return np.stack([above, below, box(0, 10, 60, 20)]), [[2, 0], [1]]


def grid_case(rows, cols, seed=None, w=40, h=14, gap=10, pitch=40):
    """``rows`` lines of ``cols`` axis-aligned integer words; ``seed`` shuffles the word order.  All corners stay below 4096 for
    rows * pitch + h < 4096 and cols * (w + gap) < 4096."""
    q = np.stack([box(c * (w + gap), r * pitch, w, h) for r in range(rows) for c in range(cols)])
    assert q.max() < 4096
    if seed is not None:
        q = q[np.random.RandomState(seed).permutation(len(q))]
    return q


def rotated_case():
    """Lines at +-5, +-20 and 40 degrees with mixed word heights, built so that every comparison is away from its threshold: gaps between
    neighbours of 1 h (linked) or 4 h (a break) with h the taller of the two, baseline offsets of at most 0.2 h of the smaller, one word per
    line turned by a further 45 degrees (never linked), and a stray word 1 h of the taller off the baseline.  Returns float32 quads (shuffled)."""
    r = np.random.RandomState(11)
    quads = []
    for li, deg in enumerate([5, -5, 20, -20, 40]):
        t = np.deg2rad(deg)
        u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
        pos = np.array([150.0, 200.0 + 420.0 * li]) if deg >= 0 else np.array([150.0, 420.0 + 420.0 * li])
        along, prev_h, prev_l = 0.0, None, None
        for k in range(12):
            h = float(r.choice([18.0, 24.0, 30.0]))
            lng = float(r.uniform(70, 140))
            if prev_h is not None:
                along += prev_l / 2 + (4.0 if k == 5 else 1.0) * max(h, prev_h) + lng / 2
            off = float(r.uniform(-0.2, 0.2)) * min(h, prev_h or h)
            turn = 45.0 if k == 2 else 0.0
            c = pos + along * u + off * v
            quads.append(rotated_rect(c[0], c[1], lng, h, deg + turn))
            if k == 7:  # a stray word beside word 7, one (taller) height off the baseline
                c2 = c + 1.0 * 30.0 * v + 0.25 * lng * u
                quads.append(rotated_rect(c2[0], c2[1], 0.4 * lng, 18.0, deg))
            prev_h, prev_l = h, lng
    q = np.stack(quads)
    return q[r.permutation(len(q))]

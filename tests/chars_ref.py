"""CPU restatement of the character rule in plain numpy, for the tests of csrc/char_spans.hip.  Written once with a dtype
parameter, as tests/lines_ref.py: in float32 every operation is the kernel's, in the kernel's order, with one rounding each; in float64 it is
the comparand for inputs whose comparisons are away from their thresholds.  Nothing here calls the package's kernels.

The rule.

(a) Spans.  For sample n of log-probs lp (T,N,C) with ``Ti = min(in_len[n], T)``: ``a[t]`` = the arg-max class at step t, first maximum on
    ties.  Every maximal run of one class ``c != 0`` inside ``[0, Ti)`` is one character: label c, ``t0`` / ``t1`` its first / last step,
    ``peak`` the largest ``lp[t][n][c]`` over the run (one of the input values, untouched).
(b) Extent.  Step t is centred on edge coordinate 4 t of the ``ow`` wide resized crop.  A character covers ``a0 = clamp(4 t0 - 2, 0, ow)`` to
    ``a1 = clamp(4 t1 + 2, 0, ow)``; with the crop frame f of its quad, ``s = a / ow * f.long`` (a and ow converted first, divided, then
    multiplied), the quad is P(s0,0), P(s1,0), P(s1,short), P(s0,short) with ``P(s, r) = origin + s u + r v`` and the centre
    ``c = 0.5 * (s0 + s1)``.
(c) Words.  With f the frame of the LINE quad, word j of the chain projects its corners with ``p = (x - ox) ux + (y - oy) uy``:
    ``lo_j = min p``, ``hi_j = max p``; ``b_j = 0.5 * (hi_j + lo_{j+1})``, ``B_j = max(b_0..b_j)``; character k belongs to word
    ``#{j : B_j <= c_k}``.  Every word's range then gives up the space label at its start, then at its end; an empty range is (e, e).
"""
from __future__ import annotations

import numpy as np

from tests.ocr_ref import crop_frame
from tests.lines_ref import ulp32  # noqa: F401  (the tests take it from here)


def space_label(alphabet) -> int:
    alphabet = list(alphabet)
    return alphabet.index(" ") + 1 if " " in alphabet else -1


# ------------------------------------------------------------------ (a) spans ------------------------------------------------------------
def decode_spans(lp, in_len) -> list[dict]:
    """lp (T,N,C) float32, in_len (N,) -> per sample ``labels``, ``t0``, ``t1`` (int lists) and ``peak`` (float32 array)"""
    lp = np.asarray(lp, dtype=np.float32)
    T, N, _ = lp.shape
    out = []
    for n in range(N):
        Ti = int(min(max(int(in_len[n]), 0), T))
        a = [int(np.argmax(lp[t, n])) for t in range(Ti)]  # np.argmax: the first maximum
        labels, t0, t1, peak = [], [], [], []
        t = 0
        while t < Ti:
            e = t
            while e + 1 < Ti and a[e + 1] == a[t]:
                e += 1
            if a[t] != 0:
                labels.append(a[t]), t0.append(t), t1.append(e)
                peak.append(lp[t:e + 1, n, a[t]].max())
            t = e + 1
        out.append({"labels": labels, "t0": t0, "t1": t1, "peak": np.array(peak, dtype=np.float32)})
    return out


def collapse(a) -> list[int]:
    """ctc_greedy_decode_text's collapse of an arg-max row: the labels ``decode_spans`` must agree with"""
    out, last = [], None
    for c in a:
        if c != last and c != 0:
            out.append(int(c))
        last = c
    return out


# ------------------------------------------------------------------ (b) extent -----------------------------------------------------------
def char_extent(t0, t1, ow: int):
    t0, t1 = np.asarray(t0, dtype=np.int64), np.asarray(t1, dtype=np.int64)
    return np.clip(4 * t0 - 2, 0, ow), np.clip(4 * t1 + 2, 0, ow)


def char_boxes(quad, ow: int, t0, t1, dtype=np.float32) -> dict:
    """``s0``, ``s1``, ``centre`` (K,) and ``quads`` (K,4,2) in ``dtype`` for the characters of the crop of ``quad``"""
    T = dtype
    f = crop_frame(quad, T)
    a0, a1 = char_extent(t0, t1, ow)
    lng, sht = T(f["long"]), T(f["short"])
    s0, s1 = a0.astype(T) / T(ow) * lng, a1.astype(T) / T(ow) * lng
    (ox, oy), (ux, uy), (vx, vy) = f["origin"].astype(T), f["u"].astype(T), f["v"].astype(T)

    def P(s, r):
        return np.stack([ox + s * ux + r * vx, oy + s * uy + r * vy], axis=-1)

    zero = np.zeros_like(s0)
    quads = np.stack([P(s0, zero), P(s1, zero), P(s1, zero + sht), P(s0, zero + sht)], axis=1).astype(T).reshape(-1, 4, 2)
    return {"s0": s0.astype(T), "s1": s1.astype(T), "centre": (T(0.5) * (s0 + s1)).astype(T), "quads": quads}


# ------------------------------------------------------------------ (c) words ------------------------------------------------------------
def word_bounds(line_quad, word_quads, dtype=np.float32) -> dict:
    """``lo``, ``hi`` (m,), ``b``, ``B`` (m-1,) of the chain's words along the line's axis"""
    T = dtype
    f = crop_frame(line_quad, T)
    (ox, oy), (ux, uy) = f["origin"].astype(T), f["u"].astype(T)
    q = np.asarray(word_quads, dtype=np.float32).reshape(-1, 4, 2).astype(T)
    p = (q[:, :, 0] - ox) * ux + (q[:, :, 1] - oy) * uy
    lo, hi = p.min(1), p.max(1)
    b = (T(0.5) * (hi[:-1] + lo[1:])).astype(T)
    return {"lo": lo, "hi": hi, "b": b, "B": np.maximum.accumulate(b) if len(b) else b}


def word_ranges(B, centre, labels, space: int) -> np.ndarray:
    """(m,2) int: the (first, end) of every word of the chain in the line's characters; ``B`` (m-1,) the boundaries' running maximum"""
    B, centre = np.asarray(B), np.asarray(centre)
    m, K = len(B) + 1, len(centre)
    g = np.array([int((B <= c).sum()) for c in centre], dtype=int)
    assert (np.diff(g) >= 0).all()  # the centres do not decrease, so every word's characters are one range
    out = np.zeros((m, 2), dtype=int)
    for j in range(m):
        first, end = int((g < j).sum()), int((g <= j).sum())
        while first < end and labels[first] == space:
            first += 1
        while end > first and labels[end - 1] == space:
            end -= 1
        out[j] = first, end
    assert K == 0 or out.max() <= K
    return out


def line_words(line_quad, word_quads, ow: int, t0, t1, labels, space: int, dtype=np.float32) -> dict:
    """(b) for the line's crop and (c) for its chain: ``ranges`` (m,2), ``margin`` = the smallest |centre - boundary| (inf without either)"""
    box = char_boxes(line_quad, ow, t0, t1, dtype)
    wb = word_bounds(line_quad, word_quads, dtype)
    d = np.abs(box["centre"][:, None].astype(np.float64) - wb["B"][None, :].astype(np.float64))
    return {"ranges": word_ranges(wb["B"], box["centre"], labels, space), "margin": float(d.min()) if d.size else float("inf"), **box, **wb}

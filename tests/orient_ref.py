"""CPU restatement of the orientation rules (ocrs_models_amd/inference/orient.py) in plain numpy, for the tests of
csrc/page_orient.hip.  Nothing here calls the package's kernels.

Convention.  ``orientation = k``, k in 0..3: the upright page is ``np.rot90(page, k)``, k quarter turns counter-clockwise.  For a page of H rows
and W columns ``turn_shape(H, W, k)`` is (H, W) for even k and (W, H) for odd k, and the point (x, y) of the TURNED page lies on the original
page at

    k = 0: (x, y)    k = 1: ((W-1) - y, x)    k = 2: ((W-1) - x, (H-1) - y)    k = 3: (y, (H-1) - x)

Coordinates are pixel centres.  These are proper rotations: corner j of a quad maps to corner j and the winding is kept.

Precision.  Everything is float64, except where a function says that it follows the device bit by bit: ``turn_quads`` with ``dtype=np.float32``
(one operation per coordinate) and the side lengths of ``votes`` (float32: sqrt(x * x + y * y), one rounding per operation, as
csrc/page_orient.hip computes them; the vote's two sums are float64 sums of those float32 lengths)."""
from __future__ import annotations

import numpy as np

COORD_KEYS = ("quad", "words", "char_quads", "spine")


def turn_shape(H: int, W: int, k: int):
    return (H, W) if k % 2 == 0 else (W, H)


def _turn(x, y, k: int, hm, wm, inverse: bool):
    """hm = H - 1, wm = W - 1"""
    if k == 0:
        return x, y
    if k == 2:
        return wm - x, hm - y
    if k == 1:
        return (y, wm - x) if inverse else (wm - y, x)
    if k == 3:
        return (hm - y, x) if inverse else (y, hm - x)
    raise ValueError(k)


def turn_point(x, y, k: int, H: int, W: int, inverse: bool = False):
    """turned-page point -> original-page point of an (H, W) page (``inverse``: the other way), on Python floats or float64 arrays"""
    return _turn(x, y, k, H - 1, W - 1, inverse)


def turn_quads(quads, k: int, H: int, W: int, inverse: bool = False, dtype=np.float64) -> np.ndarray:
    """(..., 2) points in ``dtype``; with float32 this is the device's arithmetic: W - 1 and H - 1 are exact, one subtraction per coordinate"""
    q = np.asarray(quads, dtype=dtype)
    x, y = _turn(q[..., 0], q[..., 1], k, dtype(H - 1), dtype(W - 1), inverse)
    out = np.stack([x, y], axis=-1)
    assert out.dtype == dtype
    return out


def turn_nested(v, k: int, H: int, W: int):
    """the table on nested lists of ``[x, y]`` Python floats, as the drivers map their results"""
    if len(v) == 2 and not isinstance(v[0], (list, tuple)):
        x, y = turn_point(v[0], v[1], k, H, W)
        return [x, y]
    return [turn_nested(e, k, H, W) for e in v]


def turn_results(results, k: int, H: int, W: int):
    """what a driver returns for ``orientation=k`` from what it returns on ``turn_page(page, k)``; (H, W) is the page that was passed"""
    return [{**{key: (turn_nested(val, k, H, W) if key in COORD_KEYS else val) for key, val in d.items()}, "turns": k} for d in results]


def long_sides(quads):
    """per quad: (length of the long side, of the short side, long side runs along x) by the crop-frame rule -- the longer of c0->c1 and
    c1->c2, on a tie the one with the larger |x| -- in float32, operation by operation as the device"""
    q = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 1]
    l1 = np.sqrt(e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1])
    l2 = np.sqrt(e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1])
    assert l1.dtype == np.float32
    first = (l1 > l2) | ((l1 == l2) & (np.abs(e1[:, 0]) >= np.abs(e2[:, 0])))
    lng, sht = np.where(first, l1, l2), np.where(first, l2, l1)
    e = np.where(first[:, None], e1, e2)
    return lng, sht, np.abs(e[:, 0]) >= np.abs(e[:, 1])


def votes(quads, min_aspect: float = 1.5, sample: int = 64) -> dict:
    """``H``, ``V`` (float64 sums of the voters' float32 lengths, in index order), ``voters``, ``K`` and ``picks`` (the K voters with the largest
    length, ties by the smaller index, then -1 up to ``sample``)"""
    lng, sht, horiz = long_sides(quads)
    voter = (sht > 0) & (lng >= np.float32(min_aspect) * sht)
    idx = np.flatnonzero(voter)
    h = float(np.sum(lng[idx][horiz[idx]].astype(np.float64))) if len(idx) else 0.0
    v = float(np.sum(lng[idx][~horiz[idx]].astype(np.float64))) if len(idx) else 0.0
    K = min(sample, len(idx))
    ranked = sorted(idx.tolist(), key=lambda i: (-float(lng[i]), i))[:K]
    return {"H": h, "V": v, "voters": len(idx), "K": K, "picks": ranked + [-1] * (sample - K), "voter": voter, "lengths": lng}


def path_confidence(log_probs, steps) -> np.ndarray:
    """(T, B, C) log-probs, (B,) steps -> (B,) float64: the mean over t < steps[b] of max_c log_probs[t, b, c]"""
    lp = np.asarray(log_probs, dtype=np.float64)
    return np.array([lp[:int(n), b].max(axis=1).mean() for b, n in enumerate(steps)], dtype=np.float64)


def decide(H: float, V: float, score_of) -> dict:
    """the rule of ``page_orientation`` once there are voters: a = 1 if V > H else 0; ``score_of(k)`` is the mean score of the picks on the page
    turned by k; turns = a + 2 if S_a2 > S_a else a"""
    a = 1 if V > H else 0
    s_a, s_a2 = score_of(a), score_of(a + 2)
    return {"a": a, "scores": (s_a, s_a2), "turns": a + 2 if s_a2 > s_a else a}


def mean_in_order(values) -> float:
    s = 0.0
    for v in values:
        s = s + float(v)
    return s / len(values)

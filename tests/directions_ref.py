"""CPU restatement of the mixed-directions rule (ocrs_models_amd/inference/directions.py) in plain numpy, for the tests of
csrc/line_dirs.hip.  Nothing here calls the package's kernels.

The rule.  A word quad is SIDEWAYS if none of its eight coordinates is a NaN and the long side L of the quad -- the crop-frame rule: the longer
of c0->c1 and c1->c2, on a tie the one with the larger |x| (the first if that ties too); lengths in float32 as sqrt(x * x + y * y), one
rounding per operation -- has |L.y| > |L.x|, strictly.  The upright words form virtual page 0 as they are, the sideways words virtual page 1
on the page turned by one quarter turn, (x, y) -> (y, (W-1) - x) in float32 (tests/orient_ref.py's table, k = 1, inverse), each page in input
order.  A crop is flipped iff it is probed and S_flip > S_plain (float64, strictly; a NaN on either side: no flip)."""
from __future__ import annotations

import numpy as np

from tests import orient_ref as O


def sideways(quads) -> np.ndarray:
    """(N,) bool by the rule above, float32 operation by operation as the device"""
    q = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 1]
        l1 = np.sqrt(e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1])
        l2 = np.sqrt(e2[:, 0] * e2[:, 0] + e2[:, 1] * e2[:, 1])
        assert l1.dtype == np.float32
        first = (l1 > l2) | ((l1 == l2) & (np.abs(e1[:, 0]) >= np.abs(e2[:, 0])))
        e = np.where(first[:, None], e1, e2)
        return ~np.isnan(q).any(axis=(1, 2)) & (np.abs(e[:, 1]) > np.abs(e[:, 0]))


def axis_split(quads, H: int, W: int, count=None) -> dict:
    """quads (m,4,2) float32 (page 0 first), page_of_word, word_offs [0, U, m], source_index -- for the first min(count, N) rows"""
    q = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    m = len(q) if count is None else max(0, min(int(count), len(q)))
    q = q[:m]
    s = sideways(q)
    up, side = np.flatnonzero(~s), np.flatnonzero(s)
    out = np.concatenate([q[up], O.turn_quads(q[side], 1, H, W, True, np.float32)]).astype(np.float32)
    return {"quads": out, "page_of_word": np.concatenate([np.zeros(len(up), np.int32), np.ones(len(side), np.int32)]),
            "word_offs": np.array([0, len(up), m], np.int32), "source_index": np.concatenate([up, side]).astype(np.int32)}


def flip_crops(batch, widths, flags=None) -> np.ndarray:
    """(n,1,OH,Wpad) batch -> the flagged crops (None: all) turned by 180 degrees within their valid widths: np.flip of the valid span over
    both axes; the pad columns and the other crops untouched"""
    out = np.array(batch, copy=True)
    for i, w in enumerate(widths):
        w = max(0, min(int(w), out.shape[-1]))
        if flags is None or flags[i]:
            out[i, 0, :, :w] = np.flip(batch[i, 0, :, :w], axis=(0, 1))
    return out


def flip_flags(s_plain, s_flip, probe) -> np.ndarray:
    a, b = np.asarray(s_plain, dtype=np.float64), np.asarray(s_flip, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((np.asarray(probe) != 0) & (b > a)).astype(np.int32)


def direction(sideways_line: bool, flipped: bool) -> int:
    """the quarter turns counter-clockwise that make the line upright"""
    return 0 if not sideways_line else (3 if flipped else 1)

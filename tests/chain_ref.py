"""CPU restatement of the chain-crop rule in plain numpy, for the tests of csrc/line_chain.hip.  Written once with a dtype
parameter, as tests/lines_ref.py: in float32 every operation is the kernel's, in the kernel's order, with one rounding each; in float64 it is
the comparand.  Nothing here calls the package's kernels.

The rule.  A line's words W_0..W_{n-1} in chain order, each with its crop frame f_k (tests/ocr_ref.py::crop_frame: origin o, axis u,
v = (-u.y, u.x), long, short).

* Knots.  L_k = o_k + (0.5 short_k) v_k, R_k = L_k + long_k u_k.
* Segments, 2n - 1 in order: word k (A = L_k, dir = u_k, len = long_k), then for k < n - 1 the gap behind it: d = L_{k+1} - R_k,
  g = sqrt(d.x^2 + d.y^2); with g > 0 and d.(u_k + u_{k+1}) > 0 the gap is (A = R_k, dir = d / g, len = g), else (A = R_k, dir = 0, len = 0).
  start = the running sum of the lengths before, S = the sum of all, H = max short_k.
* Crop.  w = clamp(rint(S), 1, 32768), h = clamp(rint(H), 1, 32768).
* Sample (y, x).  s = ((x + 0.5) / w) S, t = ((y + 0.5) / h - 0.5) H; the segment is the LAST with start <= s; e = s - start;
  normal = v_k on a word; on a gap m / |m| with f = e / len (0 where len == 0) and m = (1 - f) v_k + f v_{k+1} (v_k where |m| = 0);
  P(s, t) = (A + e dir) + t normal; clamp to the page; the four-tap blend of transform_image values.
* Characters.  Edge coordinates a0, a1 (tests/chars_ref.py::char_extent) -> s0 = (a0 / ow) S, s1 likewise; quad P(s0, -H/2), P(s1, -H/2),
  P(s1, +H/2), P(s0, +H/2); centre 0.5 (s0 + s1).
* Words.  b_j = start(word j + 1) - 0.5 len(gap j); character k belongs to word #{j : b_j <= c_k}; spaces trimmed as chars_ref.word_ranges.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.chars_ref import char_extent, word_ranges  # noqa: F401  (word_ranges: the tests take it from here)
from tests.lines_ref import rotated_rect
from tests.ocr_ref import crop_frame, line_output_width, ulp32  # noqa: F401

K_TABLE = 2  # ulp32(max(S, largest |coordinate|)) the float32 spine table and character quads need against float64 (test_chain_host.py pins it)
K_CROP = 3   # ulp32(largest page coordinate) the float32 crop values need against float64, next to the blend's roundings (likewise)


# ------------------------------------------------------------------ the rule -------------------------------------------------------------
def line_spine(words, dtype=np.float64) -> dict:
    """``words`` (n,4,2) in chain order -> ``rows`` (2n,8) = start, len, A.x, A.y, dir.x, dir.y, 0, 0 (the last row all zero), ``S``, ``H``,
    ``knots`` (n,2,2) = L_k, R_k; every operation in ``dtype``"""
    T = dtype
    q = np.asarray(words, dtype=np.float32).reshape(-1, 4, 2)
    n = len(q)
    fr = [crop_frame(x, T) for x in q]
    L, R = [], []
    for f in fr:
        hs = T(0.5) * f["short"]
        left = np.array([f["origin"][0] + hs * f["v"][0], f["origin"][1] + hs * f["v"][1]], dtype=T)
        L.append(left)
        R.append(np.array([left[0] + f["long"] * f["u"][0], left[1] + f["long"] * f["u"][1]], dtype=T))
    rows = np.zeros((2 * n, 8), dtype=T)
    run = T(0)
    for k, f in enumerate(fr):
        rows[2 * k, :6] = [run, f["long"], L[k][0], L[k][1], f["u"][0], f["u"][1]]
        run = T(run + f["long"])
        if k == n - 1:
            break
        un = fr[k + 1]["u"]
        dx, dy = T(L[k + 1][0] - R[k][0]), T(L[k + 1][1] - R[k][1])
        g = T(np.sqrt(T(T(dx * dx) + T(dy * dy))))
        dot = T(T(dx * T(f["u"][0] + un[0])) + T(dy * T(f["u"][1] + un[1])))
        if g > 0 and dot > 0:
            rows[2 * k + 1, :6] = [run, g, R[k][0], R[k][1], T(dx / g), T(dy / g)]
            run = T(run + g)
        else:
            rows[2 * k + 1, :4] = [run, 0, R[k][0], R[k][1]]
    H = max(T(f["short"]) for f in fr)
    return {"rows": rows, "S": T(run), "H": T(H), "knots": np.stack([np.stack(L), np.stack(R)], axis=1).astype(T), "n": n}


def crop_len(v) -> int:
    return int(min(max(np.rint(v), 1), 32768))


def crop_size(sp: dict) -> tuple[int, int]:
    """(h, w) of the line's crop"""
    return crop_len(sp["H"]), crop_len(sp["S"])


def plan_row(sp: dict, output_height: int = 64) -> tuple[int, int, int]:
    h, w = crop_size(sp)
    return h, w, line_output_width(h, w, output_height)


def segment_of(sp: dict, s) -> np.ndarray:
    """index of the last of the 2n - 1 segments with start <= s (0 where there is none)"""
    starts = sp["rows"][:2 * sp["n"] - 1, 0]
    return np.maximum(np.searchsorted(starts, s, side="right") - 1, 0)


def point(sp: dict, s, t, dtype=np.float64):
    """page position (px, py) of P(s, t), arrays of the broadcast shape of s and t, every operation in ``dtype``"""
    T = dtype
    rows = sp["rows"]
    s, t = np.broadcast_arrays(np.asarray(s, dtype=T), np.asarray(t, dtype=T))
    seg = segment_of(sp, s)
    a = rows[seg]
    e = s - a[..., 0]
    p, q = rows[np.maximum(seg - 1, 0)], rows[np.minimum(seg + 1, len(rows) - 1)]
    ln = a[..., 1]
    f = np.where(ln == 0, T(0), e / np.where(ln == 0, T(1), ln))
    g = T(1) - f
    mx, my = g * -p[..., 5] + f * -q[..., 5], g * p[..., 4] + f * q[..., 4]
    nm = np.sqrt(mx * mx + my * my)
    safe = np.where(nm > 0, nm, T(1))
    gap = (seg & 1) == 1
    nx = np.where(gap, np.where(nm > 0, mx / safe, -p[..., 5]), -a[..., 5])
    ny = np.where(gap, np.where(nm > 0, my / safe, p[..., 4]), a[..., 4])
    px, py = (a[..., 2] + e * a[..., 4]) + t * nx, (a[..., 3] + e * a[..., 5]) + t * ny
    assert px.dtype == T and py.dtype == T
    return px, py


def sample_coords(sp: dict, dtype=np.float64):
    """``s`` (w,) and ``t`` (h,) of the crop's columns and rows"""
    T = dtype
    h, w = crop_size(sp)
    s = (np.arange(w, dtype=T) + T(0.5)) / T(w) * T(sp["S"])
    t = ((np.arange(h, dtype=T) + T(0.5)) / T(h) - T(0.5)) * T(sp["H"])
    return s, t


def sample_positions(sp: dict, dtype=np.float64):
    """page coordinates (px, py), each (h, w), of the crop's samples"""
    s, t = sample_coords(sp, dtype)
    return point(sp, s[None, :], t[:, None], dtype)


def blend_f64(page_u8: torch.Tensor, px, py) -> np.ndarray:
    """F.grid_sample(align_corners=True, padding_mode="border") in float64 at float64 positions, as ocr_ref.rectify_f64"""
    page = page_u8.reshape(page_u8.shape[-2:]).double() / 255.0 - 0.5
    H, W = page.shape
    gx = 2.0 * np.clip(px, 0, W - 1) / (W - 1) - 1.0
    gy = 2.0 * np.clip(py, 0, H - 1) / (H - 1) - 1.0
    grid = torch.from_numpy(np.stack([gx, gy], -1))[None]
    return F.grid_sample(page[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0].numpy()


def blend_f32(page_u8: torch.Tensor, px, py) -> np.ndarray:
    """the four-tap blend with every operation in float32, as ocr_ref.rectify_f32"""
    f = np.float32
    page = (page_u8.reshape(page_u8.shape[-2:]).numpy().astype(f) / f(255.0) - f(0.5)).astype(f)
    H, W = page.shape
    px, py = np.clip(px, f(0), f(W - 1)).astype(f), np.clip(py, f(0), f(H - 1)).astype(f)
    x0, y0 = px.astype(np.int64), py.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (px - x0.astype(f)).astype(f), (py - y0.astype(f)).astype(f)
    a, b, c, d = page[y0, x0], page[y0, x1], page[y1, x0], page[y1, x1]
    top, bot = a + (b - a) * fx, c + (d - c) * fx
    return (top + (bot - top) * fy).astype(f)


def rectify(page_u8: torch.Tensor, sp: dict, dtype=np.float64) -> np.ndarray:
    """the (h, w) crop of the line; ``sp`` must be the spine in the same ``dtype``"""
    px, py = sample_positions(sp, dtype)
    return blend_f64(page_u8, px, py) if dtype == np.float64 else blend_f32(page_u8, px, py)


def char_boxes(sp: dict, ow: int, t0, t1, dtype=np.float64) -> dict:
    """``s0``, ``s1``, ``centre`` (K,) and ``quads`` (K,4,2) of the characters of the line's crop"""
    T = dtype
    a0, a1 = char_extent(t0, t1, ow)
    s0, s1 = a0.astype(T) / T(ow) * T(sp["S"]), a1.astype(T) / T(ow) * T(sp["S"])
    hh = T(0.5) * T(sp["H"])
    corners = [point(sp, s, t, T) for s, t in ((s0, -hh), (s1, -hh), (s1, hh), (s0, hh))]
    quads = np.stack([np.stack(c, axis=-1) for c in corners], axis=1).astype(T).reshape(-1, 4, 2)
    return {"s0": s0.astype(T), "s1": s1.astype(T), "centre": (T(0.5) * (s0 + s1)).astype(T), "quads": quads}


def word_bounds(sp: dict) -> np.ndarray:
    """b (n-1,): b_j = start(word j + 1) - 0.5 len(gap j)"""
    rows, n = sp["rows"], sp["n"]
    T = rows.dtype.type
    return np.array([rows[2 * (j + 1), 0] - T(0.5) * rows[2 * j + 1, 1] for j in range(n - 1)], dtype=T)


def table(words, lines, dtype=np.float32):
    """the whole spine table of ``lines`` (index lists into ``words`` (N,4,2), in line order): ``spine`` (2 * words in lines, 8), ``dims`` (L,2)
    and the per-line spines"""
    sps = [line_spine(np.asarray(words)[c], dtype) for c in lines]
    spine = np.concatenate([sp["rows"] for sp in sps]) if sps else np.zeros((0, 8), dtype)
    dims = np.array([[sp["S"], sp["H"]] for sp in sps], dtype=dtype).reshape(-1, 2)
    return spine, dims, sps


# ------------------------------------------------------------------ cases ----------------------------------------------------------------
def arc_line(cx, cy, radius, deg0, deg1, lengths, heights):
    """words whose centres lie on the circle about (cx, cy), evenly spread in angle from deg0 to deg1 (degrees, measured from the top of the
    circle, clockwise: the text runs left to right over the top), each tangent to it -> (n,4,2) float32 in chain order"""
    quads = []
    for a, lng, h in zip(np.linspace(deg0, deg1, len(lengths)), lengths, heights):
        t = np.deg2rad(a)
        quads.append(rotated_rect(cx + radius * np.sin(t), cy - radius * np.cos(t), lng, h, a))
    return np.stack(quads)


def straight_line(x, y, deg, lengths, heights, gaps, offsets=None):
    """words one after the other along a direction of ``deg`` degrees from (x, y): ``gaps[k]`` pixels behind word k, word k's centre
    ``offsets[k]`` pixels off the baseline (down the page for positive values) -> (n,4,2) float32 in chain order"""
    t = np.deg2rad(deg)
    u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
    quads, along = [], 0.0
    for k, (lng, h) in enumerate(zip(lengths, heights)):
        c = np.array([x, y]) + (along + lng / 2) * u + (0.0 if offsets is None else offsets[k]) * v
        quads.append(rotated_rect(c[0], c[1], lng, h, deg))
        along += lng + (gaps[k] if k < len(gaps) else 0.0)
    return np.stack(quads)


ARC_600 = dict(cx=384.0, cy=760.0, radius=600.0, deg0=-22.0, deg1=22.0, lengths=[62.0, 55.0, 70.0, 48.0, 66.0, 58.0, 64.0],
               heights=[24.0, 30.0, 34.0, 26.0, 33.0, 28.0, 31.0])
ARC_300 = dict(cx=400.0, cy=640.0, radius=300.0, deg0=-35.0, deg1=35.0, lengths=[38.0, 44.0, 35.0, 47.0, 40.0, 36.0, 45.0, 39.0],
               heights=[18.0, 22.0, 26.0, 20.0, 24.0, 19.0, 25.0, 21.0])


def curved_cases() -> dict:
    """name -> (n,4,2) float32 words in chain order, every line of at most 16 words on the 1024 x 768 page of ``ocr_ref.rectify_case``: arcs
    of radius 300 and 600, a staircase of words each 0.3 heights lower than the one before, and straight lines at +-20 degrees, with mixed
    word heights; every gap is > 0"""
    stairs_h = [22.0, 28.0, 24.0, 30.0, 26.0, 22.0]
    return {
        "arc 600": arc_line(**ARC_600),
        "arc 300": arc_line(**ARC_300),
        "staircase": straight_line(60.0, 300.0, 0.0, [70.0, 64.0, 80.0, 58.0, 74.0, 66.0], stairs_h, [12.0] * 5,
                                   offsets=list(np.cumsum([0.0] + [0.3 * h for h in stairs_h[1:]]))),
        "plus 20": straight_line(90.0, 120.0, 20.0, [80.0, 66.0, 92.0, 70.0, 85.0], [24.0, 32.0, 20.0, 28.0, 30.0], [14.0, 9.0, 17.0, 11.0]),
        "minus 20": straight_line(120.0, 560.0, -20.0, [60.0, 75.0, 52.0, 88.0, 64.0, 71.0], [26.0, 21.0, 33.0, 24.0, 29.0, 22.0], [10.0, 15.0, 8.0, 13.0, 12.0]),
    }


def long_arc_case():
    """200 words 4 px long and 2.4 to 3.6 px high along the page's diagonal, on an arc of radius 3300 from 41 to 59 degrees: gaps of about
    1.2 px and a crop about 1040 wide, so most lanes' four samples cross a knot"""
    r = np.random.RandomState(5)
    a = np.deg2rad(50.0)
    return arc_line(384.0 - 3300.0 * np.sin(a), 512.0 + 3300.0 * np.cos(a), 3300.0, 41.0, 59.0, [4.0] * 200, list(r.choice([2.4, 3.0, 3.6], 200)))


def overlap_case():
    """three words on one baseline whose expanded boxes overlap by 6 px: both gaps have length 0 and the spine jumps"""
    return np.stack([rotated_rect(200.0, 400.0, 90.0, 26.0, 0), rotated_rect(284.0, 400.0, 90.0, 30.0, 0), rotated_rect(368.0, 401.0, 90.0, 24.0, 0)])

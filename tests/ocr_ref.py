"""CPU restatement of the page-inference rules (ocrs_models_amd/inference/__init__.py's docstring) in plain numpy / torch, for the tests of
csrc/ocr_infer.hip.  Nothing here calls the package's kernels."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def ulp32(x: float) -> float:
    """spacing of fp32 numbers at |x|"""
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------------------ expansion ------------------------------------------------------------
def expand_quad(quad, dist: float) -> np.ndarray:
    q = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    e1, e2 = q[1] - q[0], q[2] - q[1]
    l1, l2 = float(np.hypot(*e1)), float(np.hypot(*e2))
    if l1 == 0.0 and l2 == 0.0:
        return q.copy()
    u = e1 / l1 if l1 > 0 else None
    v = e2 / l2 if l2 > 0 else None
    if u is None:
        u = np.array([v[1], -v[0]])
    if v is None:
        v = np.array([-u[1], u[0]])
    c = q.mean(0)
    a, b = (0.5 * l1 + dist) * u, (0.5 * l2 + dist) * v
    return np.array([c - a - b, c + a - b, c + a + b, c - a + b])


def expand_quads(quads, dist: float) -> torch.Tensor:
    """(..., 4, 2) -> the same shape, float64"""
    q = np.asarray(quads.detach().cpu().numpy() if isinstance(quads, torch.Tensor) else quads, dtype=np.float64)
    out = np.array([expand_quad(x, dist) for x in q.reshape(-1, 4, 2)]).reshape(q.shape)
    return torch.from_numpy(out)


# ------------------------------------------------------------------ crop frame -----------------------------------------------------------
def crop_frame(quad, dtype=np.float64) -> dict:
    """origin, u, v, long, short, h, w of one quad, every operation in ``dtype``"""
    T = dtype
    q = np.asarray(quad, dtype=np.float32).reshape(4, 2).astype(T)
    e1, e2 = q[1] - q[0], q[2] - q[1]
    l1 = np.sqrt(e1[0] * e1[0] + e1[1] * e1[1])
    l2 = np.sqrt(e2[0] * e2[0] + e2[1] * e2[1])
    first = l1 > l2 or (l1 == l2 and abs(e1[0]) >= abs(e2[0]))
    lng, sht, e = (l1, l2, e1) if first else (l2, l1, e2)
    u = e / lng if lng > 0 else np.array([1, 0], dtype=T)
    if u[0] < 0 or (u[0] == 0 and u[1] < 0):
        u = -u
    v = np.array([-u[1], u[0]], dtype=T)
    proj = q[:, 0] * (u[0] + v[0]) + q[:, 1] * (u[1] + v[1])
    origin = q[int(np.argmin(proj))]
    w = max(1, int(np.rint(lng)))
    h = max(1, int(np.rint(sht)))
    return {"origin": origin, "u": u, "v": v, "long": T(lng), "short": T(sht), "h": h, "w": w}


def line_output_width(h: int, w: int, output_height: int = 64) -> int:
    return min(800, max(10, int(output_height * (w / h))))


def sample_positions(fr: dict, dtype=np.float64):
    """page coordinates (px, py), each (h, w), of the crop's samples, every operation in ``dtype``"""
    T = dtype
    h, w = fr["h"], fr["w"]
    su = (np.arange(w, dtype=T) + T(0.5)) / T(w) * T(fr["long"])
    sv = (np.arange(h, dtype=T) + T(0.5)) / T(h) * T(fr["short"])
    u, v, o = fr["u"].astype(T), fr["v"].astype(T), fr["origin"].astype(T)
    px = o[0] + su[None, :] * u[0] + sv[:, None] * v[0]
    py = o[1] + su[None, :] * u[1] + sv[:, None] * v[1]
    return px, py


def rectify_f64(page_u8: torch.Tensor, quad) -> torch.Tensor:
    """the comparand: F.grid_sample(align_corners=True, padding_mode="border") in float64 at float64 sample positions -> (h, w) float64"""
    page = page_u8.reshape(page_u8.shape[-2:]).double() / 255.0 - 0.5
    H, W = page.shape
    px, py = sample_positions(crop_frame(quad, np.float64), np.float64)
    gx = 2.0 * np.clip(px, 0, W - 1) / (W - 1) - 1.0
    gy = 2.0 * np.clip(py, 0, H - 1) / (H - 1) - 1.0
    grid = torch.from_numpy(np.stack([gx, gy], -1))[None]
    return F.grid_sample(page[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0]


def rectify_f32(page_u8: torch.Tensor, quad) -> np.ndarray:
    """the same rule with every operation in float32 (what the kernel's arithmetic is) -> (h, w) float32"""
    f = np.float32
    page = (page_u8.reshape(page_u8.shape[-2:]).numpy().astype(f) / f(255.0) - f(0.5)).astype(f)
    H, W = page.shape
    px, py = sample_positions(crop_frame(quad, np.float32), np.float32)
    px = np.clip(px, f(0), f(W - 1)).astype(f)
    py = np.clip(py, f(0), f(H - 1)).astype(f)
    x0, y0 = px.astype(np.int64), py.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (px - x0.astype(f)).astype(f), (py - y0.astype(f)).astype(f)
    a, b, c, d = page[y0, x0], page[y0, x1], page[y1, x0], page[y1, x1]
    top, bot = a + (b - a) * fx, c + (d - c) * fx
    return (top + (bot - top) * fy).astype(f)


# ------------------------------------------------------------------ batching -------------------------------------------------------------
def batching(hw: list[tuple[int, int]], max_batch: int, width_unit: int, output_height: int = 64):
    """crops (h_i, w_i) -> (order, chunks): the quad indices sorted by (output width, index), and per chunk (first position, count, Wpad)"""
    ows = [line_output_width(h, w, output_height) for h, w in hw]
    order = sorted(range(len(hw)), key=lambda i: (ows[i], i))
    chunks = []
    for p in range(0, len(order), max_batch):
        idx = order[p:p + max_batch]
        widest = max(ows[i] for i in idx)
        chunks.append((p, len(idx), (widest // width_unit + 1) * width_unit))  # train_rec.py's round_up: an exact multiple gets a whole unit more
    return order, chunks, ows


def binarize_resize(prob: torch.Tensor, size, threshold: float = 0.5) -> torch.Tensor:
    """binarize_mask then nearest resize, as eval_detection.py:54-57 -> uint8"""
    p = prob.reshape(-1, 1, *prob.shape[-2:]) if prob.dim() != 4 else prob
    out = F.interpolate((p > threshold).float(), size=tuple(size), mode="nearest").to(torch.uint8)
    return out if prob.dim() == 4 else out[0, 0]


# ------------------------------------------------------------------ the rectification case ---------------------------------------------
def rotated_rect(cx, cy, long, short, deg, flip=False):
    """corners of a rectangle of the given side lengths about (cx, cy), first side along ``deg`` degrees; ``flip`` reverses the orientation"""
    t = np.deg2rad(deg)
    u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
    c = np.array([cx, cy], dtype=np.float64)
    q = np.array([c - long / 2 * u - short / 2 * v, c + long / 2 * u - short / 2 * v, c + long / 2 * u + short / 2 * v, c - long / 2 * u + short / 2 * v])
    return (q[::-1] if flip else q).astype(np.float32)


def rectify_case():
    """(page (1, 1024, 768) uint8, quads (12, 4, 2) float32): smooth gradients with one-pixel checker regions (a full value range per pixel,
    the steepest content a page can hold), and quads that are axis-aligned, turned by +-7, +-35 and 90 degrees, hanging over the page edge,
    one pixel high, and a single pixel"""
    H, W = 1024, 768
    y, x = np.mgrid[0:H, 0:W]
    page = (127.5 + 80 * np.sin(x / 37.0) + 47 * np.cos(y / 53.0 + x / 91.0))
    checker = ((x + y) & 1) * 255
    for (y0, y1, x0, x1) in [(100, 260, 80, 400), (600, 700, 300, 760), (900, 1024, 0, 200)]:
        page[y0:y1, x0:x1] = checker[y0:y1, x0:x1]
    page = torch.from_numpy(np.clip(np.rint(page), 0, 255).astype(np.uint8))[None]
    quads = np.stack([
        rotated_rect(240.3, 180.2, 200.6, 40.3, 0),
        rotated_rect(400.0, 500.0, 150.2, 31.7, 7),
        rotated_rect(300.5, 640.25, 180.4, 45.2, -7, flip=True),
        rotated_rect(500.0, 650.0, 220.3, 50.4, 35),
        rotated_rect(200.0, 820.0, 170.7, 28.3, -35),
        rotated_rect(600.0, 300.0, 210.4, 36.2, 90),
        rotated_rect(740.0, 655.0, 120.3, 40.4, 3),          # hangs over the right edge
        rotated_rect(60.0, 1010.0, 160.2, 44.3, -12),        # hangs over the bottom-left corner
        rotated_rect(350.0, 150.0, 90.3, 1.0, 0),            # one pixel high, inside a checker region
        np.array([[120, 950], [180, 950], [180, 950], [120, 950]], dtype=np.float32),  # a segment, as the hull code returns it
        np.array([[33, 44]] * 4, dtype=np.float32),          # a single pixel
        rotated_rect(500.0, 200.0, 64.0, 64.0, 0),           # a tie
    ])
    return page, torch.from_numpy(quads)


RECTIFY_BLEND_ROUNDINGS = 24  # fp32 roundings of magnitude <= ulp32(0.5) / 2 on the way from four bytes to a blended value, both sides together
RECTIFY_K_CPU = 2             # ulp32(largest page coordinate) the float32 restatement needs against the float64 one (test_ocr_host.py pins it)

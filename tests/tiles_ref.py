"""Tiled detection restated in numpy for the tests: the tile plan of one axis, the owner rule and the composed mask.  Written
from the rule, not from the kernel: a pixel's owner is found by searching the cuts, its source pixel by the float32 expression of the rule.

Per axis, page length L, tile length T >= 1, overlap 0 <= V < T:
* L <= T: one tile, start 0, length L.
* otherwise n = ceil((L - V) / (T - V)) tiles of length T with starts s_i = (i (L - T)) // (n - 1);
* cuts c_i = (s_i + s_{i+1} + T - 1) // 2 for i < n - 1 and c_{n-1} = L - 1; tile i owns c_{i-1} + 1 .. c_i (c_{-1} = -1).
A page's tiles are the product of its row tiles and column tiles, numbered row-major.

Composed mask: the byte of page pixel (y, x) is probs[t][ys][xs] > threshold for the owner tile t with window (y0, x0, th, tw), where
ys = min(int(floorf((float)(y - y0) * ((float)h / (float)th))), h - 1) and xs alike, all in float32."""
import numpy as np


def axis_plan(L, T, V):
    """-> (starts, lengths, cuts) as lists of ints"""
    assert L >= 1 and T >= 1 and 0 <= V < T
    if L <= T:
        return [0], [L], [L - 1]
    n = -((V - L) // (T - V))  # ceil((L - V) / (T - V))
    starts = [(i * (L - T)) // (n - 1) for i in range(n)]
    cuts = [(starts[i] + starts[i + 1] + T - 1) // 2 for i in range(n - 1)] + [L - 1]
    return starts, [T] * n, cuts


def check_axis(L, T, V, starts, lengths, cuts):
    """the properties the rule promises for one axis"""
    n = len(starts)
    assert len(lengths) == len(cuts) == n
    assert starts[0] == 0 and starts[-1] + lengths[-1] == L
    if L <= T:
        assert n == 1 and lengths == [L]
    else:
        assert n >= 2 and lengths == [T] * n
        assert all(1 <= b - a <= T - V for a, b in zip(starts, starts[1:]))  # strides
    assert all(a < b for a, b in zip(cuts, cuts[1:])) and cuts[-1] == L - 1
    prev = -1
    for s, ln, c in zip(starts, lengths, cuts):
        assert prev + 1 <= c and s <= prev + 1 and c <= s + ln - 1  # a non-empty owned range inside its tile
        prev = c


def owner(cuts, v):
    """the tile that owns coordinate v: the first one whose cut is not before v"""
    return int(np.searchsorted(np.asarray(cuts), v, side="left"))


def windows(H, W, tile, overlap):
    """-> (row plan, column plan, [(y0, x0, th, tw)] row-major)"""
    rows, cols = axis_plan(H, tile[0], overlap[0]), axis_plan(W, tile[1], overlap[1])
    return rows, cols, [(y0, x0, th, tw) for y0, th in zip(rows[0], rows[1]) for x0, tw in zip(cols[0], cols[1])]


def _src_index(d, n_src, n_win):
    """min(int(floorf((float)d * ((float)n_src / (float)n_win))), n_src - 1) for an array of offsets d, in float32"""
    scale = np.float32(n_src) / np.float32(n_win)
    return np.minimum(np.floor(d.astype(np.float32) * scale).astype(np.int64), n_src - 1)


def compose_page(probs, H, W, tile, overlap, threshold=0.5):
    """probs (T,h,w) float32, the tiles of ONE H x W page in row-major order -> its (H,W) uint8 mask"""
    probs = np.asarray(probs, dtype=np.float32)
    rows, cols, wins = windows(H, W, tile, overlap)
    assert probs.shape[0] == len(wins)
    _, h, w = probs.shape
    nx = len(cols[0])
    out = np.zeros((H, W), np.uint8)
    oy = np.array([owner(rows[2], y) for y in range(H)])
    ox = np.array([owner(cols[2], x) for x in range(W)])
    for iy in range(len(rows[0])):
        ys_page = np.nonzero(oy == iy)[0]
        for ix in range(nx):
            xs_page = np.nonzero(ox == ix)[0]
            t = iy * nx + ix
            y0, x0, th, tw = wins[t]
            ys, xs = _src_index(ys_page - y0, h, th), _src_index(xs_page - x0, w, tw)
            out[np.ix_(ys_page, xs_page)] = probs[t][np.ix_(ys, xs)] > np.float32(threshold)
    return out


def compose_pages(probs, sizes, tile, overlap, canvas, threshold=0.5):
    """probs (T,h,w) for the tiles of all pages back to back, sizes [(H, W)] -> the (B,Hmax,Wmax) uint8 canvas, 0 outside the pages"""
    out = np.zeros((len(sizes), *canvas), np.uint8)
    t = 0
    for p, (H, W) in enumerate(sizes):
        n = len(windows(H, W, tile, overlap)[2])
        out[p, :H, :W] = compose_page(probs[t:t + n], H, W, tile, overlap, threshold)
        t += n
    assert t == len(probs)
    return out

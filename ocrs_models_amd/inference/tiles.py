"""Tiled detection: tile plans, their device tables, the tile batch and the composed page mask."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from .args import _need_store, _to_device_async

TILES_AXIS_MAX = 64  # OCRS_TILES_AXIS_MAX of include/ocrs_hip.h: the most tiles a page may have along one axis


@dataclass
class AxisPlan:
    """The tiles of one axis of a page: tile i covers ``starts[i] .. starts[i] + lengths[i] - 1`` and owns the coordinates
    ``cuts[i - 1] + 1 .. cuts[i]`` (``cuts[-1]`` read as -1); the last cut is the axis' last coordinate."""
    starts: list[int]
    lengths: list[int]
    cuts: list[int]


@dataclass
class TilePlan:
    """What ``tile_plan`` returns, all on the host: the page's size, its tile rows and tile columns, and ``windows``, the ``(y0, x0, th, tw)``
    of its ``len(rows.starts) * len(cols.starts)`` tiles numbered row-major."""
    H: int
    W: int
    rows: AxisPlan
    cols: AxisPlan
    windows: list[tuple[int, int, int, int]]


def _need_int_pair(value, who: str, name: str) -> tuple[int, int]:
    """an int (both axes) or a pair of ints, bools excluded -> (rows, columns)"""
    pair = (value, value) if isinstance(value, int) else value
    if (not isinstance(pair, (tuple, list)) or len(pair) != 2 or any(not isinstance(v, int) or isinstance(v, bool) for v in pair)):
        raise RuntimeError(f"{who}: {name} must be an int or a pair of ints (rows, columns) in page pixels")
    return int(pair[0]), int(pair[1])


def _axis_plan(L: int, T: int, V: int) -> AxisPlan:
    if L <= T:
        return AxisPlan([0], [L], [L - 1])
    n = -(-(L - V) // (T - V))
    starts = [(i * (L - T)) // (n - 1) for i in range(n)]
    cuts = [(starts[i] + starts[i + 1] + T - 1) // 2 for i in range(n - 1)] + [L - 1]
    return AxisPlan(starts, [T] * n, cuts)


def tile_plan(H: int, W: int, tile, overlap=None) -> TilePlan:
    """The overlapping tiles of an H x W page by the rule of DESIGN.md §20, host integer arithmetic only.  ``tile = (Th, Tw)`` and
    ``overlap = (Vh, Vw)`` in page pixels (an int stands for both axes), ``0 <= V < T`` per axis.  An axis no longer than the tile has one
    tile of its own length; otherwise ``ceil((L - V) / (T - V))`` tiles of length T spread evenly from 0 to L - T, each owning the
    coordinates up to the middle of its overlap with the next.  ``overlap=None`` means ``(Th // 8, Tw // 8)``: a stated default, not a
    measured one -- no trained detector was at hand to tune it with."""
    who = "tile_plan"
    H, W = _need_int_pair((H, W), who, "the page size")
    Th, Tw = _need_int_pair(tile, who, "tile")
    if H < 1 or W < 1 or Th < 1 or Tw < 1:
        raise RuntimeError(f"{who}: the page and the tile must have at least one pixel per axis")
    Vh, Vw = (Th // 8, Tw // 8) if overlap is None else _need_int_pair(overlap, who, "overlap")
    if not (0 <= Vh < Th and 0 <= Vw < Tw):
        raise RuntimeError(f"{who}: overlap must be in 0 .. tile - 1 per axis, got {(Vh, Vw)} for tile {(Th, Tw)}")
    rows, cols = _axis_plan(H, Th, Vh), _axis_plan(W, Tw, Vw)
    windows = [(y0, x0, th, tw) for y0, th in zip(rows.starts, rows.lengths) for x0, tw in zip(cols.starts, cols.lengths)]
    return TilePlan(H, W, rows, cols, windows)


@dataclass
class TileTables:
    """The plans of B pages as the device tables of the C ABI section "tiles", all int32 views of one buffer (one host-to-device copy):
    ``tiles`` (T,5) = page, y0, x0, th, tw; ``tile_offs`` (B+1,); ``page_sizes`` (B,2); ``grids`` (B,2) = tile rows, tile columns;
    ``row_cuts`` / ``col_cuts`` (B,max_axis).  ``max_axis`` (the cut tables' pitch) and ``max_th`` (the tallest window) are host ints."""
    tiles: torch.Tensor
    tile_offs: torch.Tensor
    page_sizes: torch.Tensor
    grids: torch.Tensor
    row_cuts: torch.Tensor
    col_cuts: torch.Tensor
    max_axis: int
    max_th: int


def tile_tables(plans, device) -> TileTables:
    """A list of ``TilePlan``, one per page of a batch -> their ``TileTables`` on ``device``.  No synchronisation.  More than
    ``TILES_AXIS_MAX`` tiles along an axis of a page is an argument error."""
    plans = list(plans)
    if not plans or any(not isinstance(p, TilePlan) for p in plans):
        raise RuntimeError("tile_tables: expected a list of at least one TilePlan")
    B = len(plans)
    K = max(max(len(p.rows.starts), len(p.cols.starts)) for p in plans)
    if K > TILES_AXIS_MAX:
        raise RuntimeError(f"tile_tables: {K} tiles along one axis of a page; at most {TILES_AXIS_MAX} are supported (use a larger tile)")
    tiles, offs, sizes, grids, rc, cc = [], [0], [], [], [], []
    for b, p in enumerate(plans):
        tiles += [v for y0, x0, th, tw in p.windows for v in (b, y0, x0, th, tw)]
        offs.append(offs[-1] + len(p.windows))
        sizes += [p.H, p.W]
        grids += [len(p.rows.starts), len(p.cols.starts)]
        rc += p.rows.cuts + [p.H - 1] * (K - len(p.rows.cuts))
        cc += p.cols.cuts + [p.W - 1] * (K - len(p.cols.cuts))
    T = offs[-1]
    if T > 65535:
        raise RuntimeError(f"tile_tables: {T} tiles in one batch; at most 65535 are supported")
    buf = _to_device_async(tiles + offs + sizes + grids + rc + cc, torch.int32, device)
    parts = torch.split(buf, [5 * T, B + 1, 2 * B, 2 * B, B * K, B * K])
    return TileTables(parts[0].view(T, 5), parts[1], parts[2].view(B, 2), parts[3].view(B, 2), parts[4].view(B, K), parts[5].view(B, K), K,
                      max(th for p in plans for _, _, th, _ in p.windows))


def tile_batch(pages_packed: torch.Tensor, page_offs: torch.Tensor, page_sizes: torch.Tensor, tiles: torch.Tensor, max_th: int, size) -> torch.Tensor:
    """Every tile window of every page as the detector sees it (``ocrs_tile_batch``): the page store of ``pack_pages`` and a (T,5) int32
    device table of tiles ``(page, y0, x0, th, tw)`` -> (T,1,oh,ow) fp32, tile t being ``resize(transform_image(page[:, y0:y0+th, x0:x0+tw]),
    size)`` to the bit.  The windows are read from the uint8 store directly; ``max_th`` is at least the tallest window (it sizes the workspace).
    Two launches for any T, no synchronisation."""
    who = "tile_batch"
    B = _need_store(pages_packed, page_offs, page_sizes, who)
    _need_cuda(tiles, who)
    if tiles.dtype != torch.int32 or tiles.dim() != 2 or tiles.shape[1] != 5:
        raise RuntimeError(f"{who}: tiles must be (T,5) int32 on the device")
    oh, ow = int(size[0]), int(size[1])
    T, max_th = tiles.shape[0], int(max_th)
    if oh < 1 or ow < 1 or max_th < 1:
        raise RuntimeError(f"{who}: size and max_th must be at least 1")
    out = torch.empty(T, 1, oh, ow, dtype=torch.float32, device=tiles.device)
    if T:
        L = lib()
        ws_floats = L.tile_batch_ws_floats(T, max_th, ow)
        ws = torch.empty(ws_floats, dtype=torch.float32, device=tiles.device)
        L.tile_batch(ptr(pages_packed.contiguous()), pages_packed.numel(), ptr(page_offs.contiguous()), ptr(page_sizes.contiguous()), B, ptr(tiles.contiguous()), T,
                     max_th, ptr(ws), ws_floats, ptr(out), oh, ow)
    return out


def binarize_resize_tiles(probs: torch.Tensor, tables: TileTables, canvas, threshold: float = 0.5) -> torch.Tensor:
    """(T,h,w) fp32 tile probabilities and the ``TileTables`` of their B pages -> the uint8 canvas (B,Hmax,Wmax) of ``binarize_resize_pages``:
    every page pixel takes ``probs[t] > threshold`` at the nearest source pixel of the tile t that owns it (``ocrs_binarize_resize_tiles``,
    DESIGN.md §20), 0 outside the pages, in one launch.  A page with one tile gets the bytes of ``binarize_resize_pages``."""
    who = "binarize_resize_tiles"
    _need_cuda(probs, who)
    if not isinstance(tables, TileTables):
        raise RuntimeError(f"{who}: expected the TileTables of tile_tables")
    T, B = tables.tiles.shape[0], tables.page_sizes.shape[0]
    if probs.dtype != torch.float32 or probs.dim() != 3 or probs.shape[0] != T:
        raise RuntimeError(f"{who}: expected (T,h,w) float32 probabilities, one map per tile")
    _, h, w = probs.shape
    Hmax, Wmax = int(canvas[0]), int(canvas[1])
    out = torch.empty(B, Hmax, Wmax, dtype=torch.uint8, device=probs.device)
    lib().binarize_resize_tiles(ptr(probs.contiguous()), T, h, w, ptr(tables.tiles), ptr(tables.tile_offs), ptr(tables.page_sizes), ptr(tables.grids),
                                ptr(tables.row_cuts), ptr(tables.col_cuts), tables.max_axis, ptr(out), B, Hmax, Wmax, float(threshold))
    return out


def _check_tile_args(who: str, tile, chunk):
    if tile is not None and (not isinstance(chunk, int) or isinstance(chunk, bool) or chunk < 1):
        raise RuntimeError(f"{who}: tile_batch must be an int >= 1 (the most tiles per eval forward)")


def _detect_tiles(model, store, sizes, canvas, size, threshold: float, tile, overlap, chunk: int, who: str):
    """The tiled front half of detection for the pages of ``store`` (``sizes``: their host ``(H, W)``): plans, one ``ocrs_tile_batch``, the
    eval forward over the tiles in chunks of at most ``chunk``, the composed canvas.  -> ``(probs (T,h,w), masks (B,*canvas), TileTables)``.
    No host synchronisation."""
    try:
        plans = [tile_plan(H, W, tile, overlap) for H, W in sizes]
    except RuntimeError as e:
        raise RuntimeError(f"{who}: {e}") from None
    tables = tile_tables(plans, store[0].device)
    imgs = tile_batch(*store,tables.tiles, tables.max_th, size)
    with torch.inference_mode():
        parts = [model(imgs[a:a + chunk])[:, 0] for a in range(0, imgs.shape[0], chunk)]
        probs = parts[0] if len(parts) == 1 else torch.cat(parts)
    return probs, binarize_resize_tiles(probs, tables, canvas, threshold), tables

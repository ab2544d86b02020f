"""Crops: the crop plan, the rectified crops of one page or of a page store, and the width-sorted recognition batches."""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from ..text import round_up
from .args import _need_counts, _need_page, _need_quads, _need_store, _to_host_async

_OW_BINS = 801         # line_output_width() is in [10, 800]


@dataclass
class CropPlan:
    """Per-quad crop geometry on the device.  ``table`` (N,8) int32: h, w, output width, packed element offset, horizontal-pass element
    offset, first sampler tile, position in (output width, index) order, the quad at that position.  ``totals`` (805,) int64: N, packed
    elements, horizontal-pass elements, sampler tiles, then the histogram of output widths 0..800."""
    table: torch.Tensor
    totals: torch.Tensor
    output_height: int
    _host: list | None = field(default=None, repr=False)
    _host_table: torch.Tensor | None = field(default=None, repr=False)

    def host(self) -> list:
        """``totals`` on the host: the one synchronisation between the plan and the crops (cached).  The table comes along in the same
        wait, so the order (``host_perm``) costs no second one."""
        if self._host is None:
            tot, tab = _to_host_async(self.totals), _to_host_async(self.table)
            torch.cuda.current_stream(self.totals.device).synchronize()
            self._host, self._host_table = tot.tolist(), tab
            if max(self._host[1:4]) >= 2 ** 31:
                raise RuntimeError("crop_plan: the crops of this page do not fit 32-bit offsets")
        return self._host

    def host_perm(self) -> list[int]:
        """Position of quad i in output-width order as a host list (from the copy ``host()`` made): ``sorted_results[perm[i]]`` is quad i's"""
        n = self.host()[0]
        return self._host_table[:n, 6].tolist()


def crop_plan(quads: torch.Tensor, output_height: int = 64, count: torch.Tensor | None = None) -> CropPlan:
    """Geometry of the crop of every quad (N,4,2) by the module's crop-frame rule, offsets into the packed buffers and the order by output
    width.  One kernel, no synchronisation.  ``count`` (1,) int32 on the device: only the first ``min(count, N)`` quads are planned (the
    table's other rows are left as allocated); the later stages take that number from ``plan.host()[0]``."""
    q = _need_quads(quads, "crop_plan")
    if count is not None:
        count = _need_counts(count, "crop_plan")
    n = q.shape[0]
    table = torch.empty(n, 8, dtype=torch.int32, device=q.device)
    totals = torch.empty(4 + _OW_BINS, dtype=torch.int64, device=q.device)
    lib().crop_plan(ptr(q), ptr(count), n, int(output_height), ptr(table), ptr(totals))
    return CropPlan(table, totals, int(output_height))


def rectify_crops(page_u8: torch.Tensor, quads: torch.Tensor, plan: CropPlan) -> torch.Tensor:
    """Cut every rotated rectangle out of the (1,H,W) / (H,W) uint8 page into one packed fp32 buffer: crop i is (h_i, w_i) row-major at
    ``plan.table[i, 3]``.  ``transform_image`` fused, bilinear, one launch for all crops."""
    page, q = _need_page(page_u8, "rectify_crops"), _need_quads(quads, "rectify_crops", plan=plan)
    H, W = page.shape[-2:]
    _, packed_floats, _, tiles = plan.host()[:4]
    packed = torch.empty(packed_floats, dtype=torch.float32, device=q.device)
    lib().rectify_crops(ptr(page), H, W, ptr(q), ptr(plan.table), ptr(plan.totals), tiles, ptr(packed), packed_floats)
    return packed


def plan_chunks(hist, max_batch: int, width_unit: int) -> list[tuple[int, int, int]]:
    """Host side of the batching rule: from the histogram of output widths, the chunks of the width-sorted crops as
    (first position, crop count, Wpad = round_up(widest crop of the chunk, width_unit))."""
    chunks, pos, total = [], 0, sum(hist)
    edges = []  # cumulative counts per width, ascending
    run = 0
    for wd, c in enumerate(hist):
        if c:
            run += c
            edges.append((run, wd))
    k = 0
    while pos < total:
        cnt = min(max_batch, total - pos)
        while edges[k][0] < pos + cnt:
            k += 1
        chunks.append((pos, cnt, round_up(edges[k][1], width_unit)))
        pos += cnt
    return chunks


def crops_to_batches(packed: torch.Tensor, plan: CropPlan, max_batch: int = 256, width_unit: int = 64):
    """Antialiased resize of every packed crop to ``output_height`` rows and ``line_output_width(h_i, w_i)`` columns, written straight into
    right-padded (n,1,output_height,Wpad) batches (pad value 0.0, as ``collate_samples`` pads).  Crops are ordered by output width (ties by
    quad index), a chunk holds at most ``max_batch`` crops and ``Wpad = round_up(widest crop of the chunk, width_unit)`` with ``text.round_up``,
    the reference's, which gives an exact multiple a whole unit more (train_rec.py:220-225).

    Returns ``(batches, image_widths, perm)``: the batch tensors, the (n,) int64 device widths of their crops, and the permutation back to
    quad order as a host list (``plan.host_perm()``: ``sorted_results[perm[i]]`` belongs to quad i; it came with the totals, no wait of its own)."""
    _need_cuda(packed, "crops_to_batches")
    if packed.dtype != torch.float32 or max_batch < 1 or width_unit < 1:
        raise RuntimeError("crops_to_batches: expected the float32 buffer of rectify_crops, max_batch >= 1 and width_unit >= 1")
    tot = plan.host()
    n, packed_floats, hpass = tot[0], tot[1], tot[2]
    if packed.numel() < packed_floats:
        raise RuntimeError("crops_to_batches: the packed buffer is smaller than the plan says")
    OH = plan.output_height
    dev = packed.device
    chunks = plan_chunks(tot[4:], max_batch, width_unit)
    offs, off = [], 0
    for _, cnt, wpad in chunks:
        offs += [off, wpad]
        off += cnt * OH * wpad
    out = torch.empty(off, dtype=torch.float32, device=dev)
    batches = [out[o:o + cnt * OH * wpad].view(cnt, 1, OH, wpad) for (_, cnt, wpad), o in zip(chunks, offs[::2])]
    if n:
        L = lib()
        chunks_d = torch.tensor(offs, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        ws_floats = L.resize_aa_packed_ws_floats(hpass)
        ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
        L.resize_aa_packed(ptr(packed), ptr(plan.table), None, n, ptr(chunks_d), len(chunks), int(max_batch), ptr(ws), ws_floats, ptr(out), off, OH)
    widths_sorted = plan.table[:n, 2][plan.table[:n, 7].long()].long() if n else torch.empty(0, dtype=torch.int64, device=dev)
    image_widths = [widths_sorted[p:p + cnt] for p, cnt, _ in chunks]
    return batches, image_widths, plan.host_perm()


def rectify_crops_pages(pages_packed: torch.Tensor, page_offs: torch.Tensor, page_sizes: torch.Tensor, quads: torch.Tensor, page_of_quad: torch.Tensor,
                        plan: CropPlan) -> torch.Tensor:
    """``rectify_crops`` from a page store (``pack_pages``): crop i is cut out of page ``page_of_quad[i]`` -- ``page_of_line`` for line crops,
    ``page_of_word`` for word crops.  One launch for the crops of all pages; a crop's values are those ``rectify_crops`` gives it on its own page."""
    _need_cuda(page_of_quad, "rectify_crops_pages")
    B = _need_store(pages_packed, page_offs, page_sizes, "rectify_crops_pages")
    q = _need_quads(quads, "rectify_crops_pages", plan=plan)
    if page_of_quad.dtype != torch.int32 or tuple(page_of_quad.shape) != (q.shape[0],):
        raise RuntimeError("rectify_crops_pages: page_of_quad must be (N,) int32")
    _, packed_floats, _, tiles = plan.host()[:4]
    packed = torch.empty(packed_floats, dtype=torch.float32, device=q.device)
    lib().rectify_crops_pages(ptr(pages_packed.contiguous()), pages_packed.numel(), ptr(page_offs.contiguous()), ptr(page_sizes.contiguous()), B, ptr(q),
                              ptr(page_of_quad.contiguous()), ptr(plan.table), ptr(plan.totals), tiles, ptr(packed), packed_floats)
    return packed

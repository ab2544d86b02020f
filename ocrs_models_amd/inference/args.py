"""Argument checks and asynchronous copy helpers shared by the stages of page inference."""
from __future__ import annotations

import torch

from ..input_pipeline import _need_cuda


# Argument checks shared by the public functions; ``who`` is the caller's name, so every message starts with the function the user called.
def _need_quads(quads: torch.Tensor, who: str, shape: str = "(N,4,2)", plan=None) -> torch.Tensor:
    """fp32 quads of that shape on the device (``plan``, a ``crops.CropPlan``: as many as the plan has rows) -> contiguous"""
    _need_cuda(quads, who)
    if quads.dtype != torch.float32 or quads.dim() != shape.count(",") + 1 or tuple(quads.shape[-2:]) != (4, 2):
        raise RuntimeError(f"{who}: expected {shape} float32 quads")
    if plan is not None and quads.shape[0] != plan.table.shape[0]:
        raise RuntimeError(f"{who}: quads must be the quads the plan was made from")
    return quads.contiguous()


def _need_counts(counts: torch.Tensor, who: str, entries: int = 1) -> torch.Tensor:
    """int32 device counts, ``entries`` of them (one per batch row or page; a single count by default) -> contiguous"""
    _need_cuda(counts, who)
    if counts.dtype != torch.int32 or counts.numel() != entries:
        raise RuntimeError(f"{who}: expected {entries} int32 count(s) on the device")
    return counts.contiguous()


def _need_page(page_u8: torch.Tensor, who: str) -> torch.Tensor:
    """a (1,H,W) or (H,W) uint8 page on the device -> contiguous"""
    _need_cuda(page_u8, who)
    if page_u8.dtype != torch.uint8 or not (page_u8.dim() == 2 or (page_u8.dim() == 3 and page_u8.shape[0] == 1)):
        raise RuntimeError(f"{who}: expected a (1,H,W) or (H,W) uint8 page")
    return page_u8.contiguous()


def _to_host_async(t: torch.Tensor) -> torch.Tensor:
    """a pinned host copy of ``t`` queued on the current stream: valid after the next wait for that stream"""
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


def _to_device_async(values, dtype, device) -> torch.Tensor:
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def _check_pages(pages, who: str):
    """the pages of a batch: (1,H,W) uint8 tensors on one device"""
    pages = list(pages)
    for p in pages:
        if not isinstance(p, torch.Tensor):
            raise RuntimeError(f"{who}: expected a list of (1,H,W) uint8 device pages")
        _need_cuda(p, who)
        if p.dtype != torch.uint8 or p.dim() != 3 or p.shape[0] != 1 or p.shape[1] < 1 or p.shape[2] < 1:
            raise RuntimeError(f"{who}: expected (1,H,W) uint8 pages")
        if p.device != pages[0].device:
            raise RuntimeError(f"{who}: the pages of a batch must be on one device")
    return pages


def _need_store(pages_packed, page_offs, page_sizes, who: str) -> int:
    """the page store of ``pack_pages`` -> B"""
    for t in (pages_packed, page_offs, page_sizes):
        _need_cuda(t, who)
    if pages_packed.dtype != torch.uint8 or pages_packed.dim() != 1:
        raise RuntimeError(f"{who}: expected the flat uint8 buffer of pack_pages")
    B = page_offs.numel()
    if page_offs.dtype != torch.int64 or page_sizes.dtype != torch.int32 or tuple(page_sizes.shape) != (B, 2):
        raise RuntimeError(f"{who}: page_offs must be (B,) int64 and page_sizes (B,2) int32")
    return B

"""Mixed directions (csrc/line_dirs.hip, C ABI section "directions"; restated for the tests in tests/directions_ref.py): sideways
text on an otherwise upright page -- a table's row headers, the label of a y axis, a margin note, a book spine.  ``directions="mixed"`` of
``read_lines`` / ``ocr_lines`` reads one page as a batch of two virtual pages through the page-batch path: page 0 holds the upright words as they
are, page 1 the sideways words on ``turn_page(page, 1)``.  ``split_by_axis`` is that split, ``line_directions`` the recogniser probe that decides
per sideways line which way up it reads (``flip_crops``: a crop turned by 180 degrees within its valid width; ``flip_flags``: the strict
comparison of the two scores), ``mixed_results`` the way back to the page that was passed.

``"direction"`` of a result dict is the number of quarter turns counter-clockwise that make the line upright: 0 for an upright line, 1 for a
sideways line that reads downwards, 3 for one that reads upwards."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from .args import _need_counts, _need_quads
from .orient import _turn_nested, _turn_point, path_confidence

TURNED_KEYS = ("quad", "words", "spine")  # the keys of a line dict that hold page coordinates (``chars`` is refused with directions)


@dataclass
class AxisSplit:
    """What ``split_by_axis`` returns, all on the device.  With U = ``word_offs[1]`` and m = ``word_offs[2]``: ``quads[:U]`` are the upright
    words as they came, ``quads[U:m]`` the sideways words on the page turned by one quarter turn, both in input order; ``page_of_word`` is 0
    and 1 for them; row r was input row ``source_index[r]``.  Rows from m on are not written."""
    quads: torch.Tensor         # (N,4,2) fp32
    page_of_word: torch.Tensor  # (N,) int32
    word_offs: torch.Tensor     # (3,) int32: 0, U, m
    source_index: torch.Tensor  # (N,) int32


def _check_directions(who: str, directions, chars: bool = False):
    """the ``directions`` keyword of ``read_lines`` / ``ocr_lines``: None or "mixed"; "mixed" does not go with ``chars``"""
    if directions is None:
        return None
    if not (isinstance(directions, str) and directions == "mixed"):
        raise RuntimeError(f'{who}: directions must be None or "mixed" (sideways words are read as lines of their own, DESIGN.md §24)')
    if chars:
        raise RuntimeError(f'{who}: directions="mixed" does not go with chars=True (the character boxes of a crop turned by 180 degrees need mirrored spans)')
    return directions


def split_by_axis(quads: torch.Tensor, H: int, W: int, count: torch.Tensor | None = None) -> AxisSplit:
    """Word quads (N,4,2) of a page of H rows and W columns -> the words of two virtual pages (``AxisSplit``).  A word is sideways if the long
    side L of its quad (the crop-frame rule: the longer of c0->c1 and c1->c2, on a tie the one with the larger |x|) has |L.y| > |L.x|
    (strictly: exactly 45 degrees is upright, and so is a quad with a NaN coordinate).  Sideways words are mapped to ``turn_page(page, 1)``,
    the bits ``turn_quads(.., 1, H, W, inverse=True)`` gives.  The order within each page is the input's (a scan: equal input gives equal
    bytes).  ``count`` (1,) int32 on the device: only the first ``min(count, N)`` rows are words.  One launch, no synchronisation; N == 0
    launches nothing."""
    q = _need_quads(quads, "split_by_axis")
    if count is not None:
        count = _need_counts(count, "split_by_axis")
    H, W = int(H), int(W)
    if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
        raise RuntimeError("split_by_axis: H and W must be in 1 .. 2^24")
    n = q.shape[0]
    if n > 1 << 16:
        raise RuntimeError("split_by_axis: at most 65536 quads (the split is sized for the words of one page)")
    i32 = dict(dtype=torch.int32, device=q.device)
    out = AxisSplit(torch.empty_like(q), torch.empty(n, **i32), (torch.empty if n else torch.zeros)(3, **i32), torch.empty(n, **i32))
    lib().axis_split(ptr(q), n, ptr(count), H, W, ptr(out.quads), ptr(out.page_of_word), ptr(out.word_offs), ptr(out.source_index))
    return out


def flip_crops(batch: torch.Tensor, widths: torch.Tensor, flags: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """A recognition batch (n,1,OH,Wpad) fp32 of ``crops_to_batches`` and the (n,) int64 widths of its crops -> the batch with every crop i
    whose ``flags[i] != 0`` ((n,) int32 on the device; None: every crop) turned by 180 degrees within its valid width:
    ``out[i, 0, y, x] = batch[i, 0, OH-1-y, w_i-1-x]`` for ``x < w_i``; the pad columns and the other crops are copied.  An exact permutation
    of the elements.  ``out``: write into this tensor (same shape, contiguous, not the input).  One launch, no synchronisation."""
    who = "flip_crops"
    _need_cuda(batch, who)
    _need_cuda(widths, who)
    if batch.dtype != torch.float32 or batch.dim() != 4 or batch.shape[1] != 1 or min(batch.shape[2:]) < 1 or not batch.is_contiguous():
        raise RuntimeError(f"{who}: expected a contiguous (n,1,OH,Wpad) float32 batch")
    n, _, OH, Wpad = batch.shape
    if widths.dtype != torch.int64 or tuple(widths.shape) != (n,):
        raise RuntimeError(f"{who}: widths must be (n,) int64 on the device")
    if flags is not None:
        _need_cuda(flags, who)
        if flags.dtype != torch.int32 or tuple(flags.shape) != (n,):
            raise RuntimeError(f"{who}: flags must be (n,) int32 on the device")
        flags = flags.contiguous()
    if out is None:
        out = torch.empty_like(batch)
    else:
        _need_cuda(out, who)
        if out.dtype != torch.float32 or out.shape != batch.shape or not out.is_contiguous() or out.data_ptr() == batch.data_ptr():
            raise RuntimeError(f"{who}: out must be a contiguous float32 tensor of the batch's shape, and not the batch")
    lib().flip_crops(ptr(batch), ptr(out), n, OH, Wpad, ptr(widths.contiguous()), ptr(flags))
    return out


def flip_flags(s_plain: torch.Tensor, s_flip: torch.Tensor, probe: torch.Tensor) -> torch.Tensor:
    """(n,) fp64 scores of the crops as they are and turned by 180 degrees, and ``probe`` (n,) int32 (the page of every crop's line, or any
    mask) -> (n,) int32 on the device: 1 where ``probe != 0`` and ``s_flip > s_plain`` -- strictly and in fp64, so equal scores and a NaN on
    either side give 0.  One launch, no synchronisation."""
    who = "flip_flags"
    for t in (s_plain, s_flip, probe):
        _need_cuda(t, who)
    n = s_plain.numel()
    if s_plain.dtype != torch.float64 or s_flip.dtype != torch.float64 or s_plain.dim() != 1 or tuple(s_flip.shape) != (n,):
        raise RuntimeError(f"{who}: the scores must be two (n,) float64 tensors")
    if probe.dtype != torch.int32 or tuple(probe.shape) != (n,):
        raise RuntimeError(f"{who}: probe must be (n,) int32 on the device")
    flags = torch.empty(n, dtype=torch.int32, device=s_plain.device)
    lib().flip_flags(ptr(s_plain.contiguous()), ptr(s_flip.contiguous()), ptr(probe.contiguous()), n, ptr(flags))
    return flags


def line_directions(rec_model, batches, image_widths, probe: torch.Tensor):
    """Which way up every probed crop reads -> ``(flags, scores)`` on the device, rows in the batches' (width-sorted) order: for every chunk
    of ``crops_to_batches`` a second batch with every crop turned (``flip_crops``), the recogniser's eval forward on both and
    ``path_confidence`` over each crop's ``width // 4`` steps; ``scores`` (n,2) fp64 = ``[S_plain, S_flip]`` and ``flags = flip_flags(S_plain,
    S_flip, probe)``.  ``probe`` (n,) int32: the page of every crop's line, in the same order.  Two forwards per chunk, no synchronisation."""
    who = "line_directions"
    if rec_model.training:
        raise RuntimeError(f"{who}: the model must be in eval mode (model.eval())")
    _need_cuda(probe, who)
    plain, turned = [], []
    with torch.inference_mode():
        for img, iw in zip(batches, image_widths):
            steps = iw.div(4, rounding_mode="floor").int()
            plain.append(path_confidence(rec_model(img), steps))
            turned.append(path_confidence(rec_model(flip_crops(img, iw)), steps))
    if not plain:
        return torch.empty(0, dtype=torch.int32, device=probe.device), torch.empty(0, 2, dtype=torch.float64, device=probe.device)
    s_plain, s_flip = torch.cat(plain), torch.cat(turned)
    return flip_flags(s_plain, s_flip, probe), torch.stack([s_plain, s_flip], dim=1)


def turn_flagged(batches, image_widths, flags: torch.Tensor):
    """the batches that are finally read: the plain ones with the flagged crops turned -- ``flip_crops`` again, now with the flags as its mask"""
    out, row = [], 0
    for img, iw in zip(batches, image_widths):
        out.append(flip_crops(img, iw, flags[row:row + img.shape[0]]))
        row += img.shape[0]
    return out


def mixed_results(flat: list, line_page_offs: list, line_at: list, flags: list, scores: list, H: int, W: int) -> list:
    """The flat result list of the two virtual pages -> the result of ``directions="mixed"`` on the page that was passed, H rows by W columns.
    ``flat``: what ``_read_crops`` returned, page 0's lines at the positions ``line_page_offs[0]:line_page_offs[1]`` and page 1's behind them;
    position k holds line ``line_at[k]`` (line order: k itself); ``flags[l]`` and ``scores[l]`` are the probe's flag and ``[S_plain, S_flip]``
    of LINE l.  Every dict gains ``"direction"`` (0 for page 0; 1, or 3 where the line was flipped, for page 1) and ``"direction_scores"``
    (None for page 0) in front of ``"block"``.  Page 1's dicts go through the k = 1 row of ``turn_results``' table (``"quad"``, ``"words"``,
    ``"spine"``); for direction 3 ``"words"`` and the knots of ``"spine"`` are reversed, so both still run in reading direction; their
    ``"block"`` counts on from page 0's last block.  Host work only."""
    first_sideways = line_page_offs[1]
    blocks_upright = flat[first_sideways - 1]["block"] + 1 if first_sideways > 0 and "block" in flat[first_sideways - 1] else 0
    to_page = _turn_point(1, int(H), int(W))
    out = []
    for k, d in enumerate(flat):
        line = line_at[k]
        sideways = k >= first_sideways
        direction = 0 if not sideways else (3 if flags[line] else 1)
        new = {key: val for key, val in d.items() if key != "block"}
        if sideways:
            for key in TURNED_KEYS:
                if key in new:
                    turned = _turn_nested(new[key], to_page)
                    new[key] = turned[::-1] if direction == 3 and key != "quad" else turned
        new["direction"] = direction
        new["direction_scores"] = list(scores[line]) if sideways else None
        if "block" in d:
            new["block"] = d["block"] + (blocks_upright if sideways else 0)
        out.append(new)
    return out

"""Chain crops (csrc/line_chain.hip, C ABI section "chain crops"; restated for the tests in tests/chain_ref.py): a line's crop cut
along the polyline of its words at one constant height, in the place of the rectangle around them, and the character boxes and word ranges of
such crops.  Every function here queues kernels and returns; the only wait is ``plan.host()``."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from ..text import DEFAULT_ALPHABET
from .args import _need_counts, _need_page, _need_quads, _need_store
from .crops import _OW_BINS, CropPlan
from .decode import CharBoxes, CharSpans, space_label
from .lines import TextLines


@dataclass
class LineSpines:
    """What ``line_spines`` returns, on the device.  ``spine`` (2N,8) fp32: row 2p is the word at chain position p (the positions
    ``line_offsets[l]:line_offsets[l + 1]`` are line l's), row 2p+1 the gap behind it, each ``start, len, A.x, A.y, dir.x, dir.y, 0, 0``; the
    last word of a line has an all-zero gap row.  ``line_dims`` (N,2) fp32: the spine's length S and the crop height H of every line.
    ``lines``: the ``TextLines`` they were made from.  Rows of lines from ``lines.n_lines`` on are not written."""
    spine: torch.Tensor
    line_dims: torch.Tensor
    lines: TextLines

    def knots(self) -> torch.Tensor:
        """(N,2,2) fp32 on the device: the two knots L, R of the word at every chain position (L = A of its row, R = L + len * dir, the
        kernel's operations), so line l's spine is ``knots[line_offsets[l]:line_offsets[l + 1]]`` flattened to 2n points"""
        word = self.spine[0::2]
        left = word[:, 2:4]
        return torch.stack([left, left + word[:, 1:2] * word[:, 4:6]], dim=1)


def _need_spines(spines, who: str, plan: CropPlan | None = None) -> int:
    """a ``LineSpines`` whose tensors have the shapes of its lines (``plan``: one table row per line) -> N"""
    if not isinstance(spines, LineSpines) or not isinstance(spines.lines, TextLines):
        raise RuntimeError(f"{who}: expected the LineSpines of line_spines")
    n = spines.lines.word_order.shape[0]
    for t, shape in ((spines.spine, (2 * n, 8)), (spines.line_dims, (n, 2))):
        _need_cuda(t, who)
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{who}: expected the LineSpines of line_spines")
    if plan is not None and plan.table.shape[0] != n:
        raise RuntimeError(f"{who}: the plan must be the crop_plan_chain of these spines")
    return n


def line_spines(lines: TextLines, out: LineSpines | None = None) -> LineSpines:
    """The spine of every line of ``find_lines`` / ``find_lines_pages`` by the rule of DESIGN.md §21 (``ocrs_line_spines``): per word the
    mid-points of its left and right edges in its crop frame, per pair of neighbours the gap between them, and the running length along the
    chain.  ``out``: write into these tensors instead of new ones.  One launch, no host synchronisation; ``N == 0`` launches nothing."""
    who = "line_spines"
    if not isinstance(lines, TextLines) or lines.words is None:
        raise RuntimeError(f"{who}: expected the TextLines of find_lines or find_lines_pages")
    words = _need_quads(lines.words, who)
    n = words.shape[0]
    n_lines = _need_counts(lines.n_lines, who)
    for t, shape in ((lines.line_offsets, (n + 1,)), (lines.word_order, (n,))):
        _need_cuda(t, who)
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{who}: the line table must be that of {n} words")
    if out is None:
        out = LineSpines(torch.empty(2 * n, 8, dtype=torch.float32, device=words.device), torch.empty(n, 2, dtype=torch.float32, device=words.device), lines)
    else:
        out.lines = lines
        _need_spines(out, who)
    if n:
        lib().line_spines(ptr(words), n, ptr(n_lines), n, ptr(lines.line_offsets), ptr(lines.word_order), ptr(out.spine), ptr(out.line_dims))
    return out


def crop_plan_chain(spines: LineSpines, output_height: int = 64) -> CropPlan:
    """``crop_plan`` for chain crops: the same table and totals with ``(h, w)`` of line l from ``(H, S)`` of its spine, for the first
    ``lines.n_lines`` lines (the count stays on the device).  One kernel, no synchronisation."""
    n = _need_spines(spines, "crop_plan_chain")
    dev = spines.line_dims.device
    table = torch.empty(n, 8, dtype=torch.int32, device=dev)
    totals = torch.empty(4 + _OW_BINS, dtype=torch.int64, device=dev)
    lib().crop_plan_dims(ptr(spines.line_dims), ptr(_need_counts(spines.lines.n_lines, "crop_plan_chain")), n, int(output_height), ptr(table), ptr(totals))
    return CropPlan(table, totals, int(output_height))


def rectify_chain(page_u8: torch.Tensor, spines: LineSpines, plan: CropPlan) -> torch.Tensor:
    """``rectify_crops`` along the spines: line l's crop, (h_l, w_l) row-major at ``plan.table[l, 3]`` of one packed fp32 buffer, follows the
    polyline of its words at the constant height H_l.  ``transform_image`` fused, bilinear, one launch for all crops."""
    page = _need_page(page_u8, "rectify_chain")
    n = _need_spines(spines, "rectify_chain", plan)
    H, W = page.shape[-2:]
    _, packed_floats, _, tiles = plan.host()[:4]
    packed = torch.empty(packed_floats, dtype=torch.float32, device=spines.spine.device)
    lib().rectify_chain(ptr(page), H, W, ptr(spines.spine), ptr(spines.line_dims), ptr(spines.lines.line_offsets), n, ptr(plan.table), ptr(plan.totals), tiles,
                        ptr(packed), packed_floats)
    return packed


def rectify_chain_pages(pages_packed: torch.Tensor, page_offs: torch.Tensor, page_sizes: torch.Tensor, spines: LineSpines, page_of_line: torch.Tensor,
                        plan: CropPlan) -> torch.Tensor:
    """``rectify_chain`` from a page store (``pack_pages``): line l is cut out of page ``page_of_line[l]``.  One launch for the lines of all
    pages; a crop's values are those ``rectify_chain`` gives it on its own page."""
    who = "rectify_chain_pages"
    _need_cuda(page_of_line, who)
    B = _need_store(pages_packed, page_offs, page_sizes, who)
    n = _need_spines(spines, who, plan)
    if page_of_line.dtype != torch.int32 or tuple(page_of_line.shape) != (n,):
        raise RuntimeError(f"{who}: page_of_line must be (N,) int32")
    _, packed_floats, _, tiles = plan.host()[:4]
    packed = torch.empty(packed_floats, dtype=torch.float32, device=spines.spine.device)
    lib().rectify_chain_pages(ptr(pages_packed.contiguous()), pages_packed.numel(), ptr(page_offs.contiguous()), ptr(page_sizes.contiguous()), B, ptr(spines.spine),
                              ptr(spines.line_dims), ptr(spines.lines.line_offsets), n, ptr(page_of_line.contiguous()), ptr(plan.table), ptr(plan.totals), tiles,
                              ptr(packed), packed_floats)
    return packed


def char_boxes_chain(spines: LineSpines, plan: CropPlan, spans: CharSpans) -> CharBoxes:
    """``char_boxes`` for chain crops (``ocrs_char_boxes_chain``): a character's stretch of the crop's width is a stretch of the
    spine, and its quad the four points half the crop height to either side of the spine at its two ends -- a quadrilateral that follows the
    line.  ``s0`` / ``s1`` are positions along the spine.  One launch, no synchronisation."""
    n = _need_spines(spines, "char_boxes_chain", plan)
    rows, ld = spans.labels.shape
    if rows > n:
        raise RuntimeError("char_boxes_chain: more span rows than lines")
    f32 = dict(dtype=torch.float32, device=spines.spine.device)
    out = CharBoxes(torch.empty(rows, ld, **f32), torch.empty(rows, ld, **f32), torch.empty(rows, ld, 4, 2, **f32))
    lib().char_boxes_chain(ptr(spines.spine), ptr(spines.line_dims), ptr(spines.lines.line_offsets), n, ptr(plan.table), n, rows, ld, ptr(spans.lens), ptr(spans.t0),
                           ptr(spans.t1), ptr(out.s0), ptr(out.s1), ptr(out.quads))
    return out


def word_chars_chain(spines: LineSpines, plan: CropPlan, spans: CharSpans, boxes: CharBoxes, alphabet=DEFAULT_ALPHABET) -> torch.Tensor:
    """``word_chars`` for chain crops (``ocrs_word_chars_chain``): neighbouring words split the line in the middle of the gap between them,
    measured along the spine; spaces at either end of a range are dropped.  -> (N,2) int32 on the device, indexed by the flat word index.
    One launch, no synchronisation."""
    who = "word_chars_chain"
    n = _need_spines(spines, who, plan)
    rows, ld = spans.labels.shape
    if rows > n or tuple(boxes.s0.shape) != (rows, ld):
        raise RuntimeError(f"{who}: spans and boxes must be those of the lines' crops")
    lines = spines.lines
    out = torch.empty(n, 2, dtype=torch.int32, device=spines.spine.device)
    lib().word_chars_chain(ptr(spines.spine), n, ptr(lines.n_lines), n, ptr(lines.line_offsets), ptr(lines.word_order), ptr(plan.table), rows, ld, ptr(spans.labels),
                           ptr(spans.lens), ptr(boxes.s0), ptr(boxes.s1), space_label(alphabet), ptr(out))
    return out

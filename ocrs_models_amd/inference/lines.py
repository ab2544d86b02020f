"""Words -> text lines and the lines' reading order, for one page or the flat words of a page batch."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from .args import _need_counts, _need_quads


@dataclass
class TextLines:
    """What ``find_lines`` returns, all on the device.  With L = ``n_lines[0]`` and n the number of words: ``quads[:L]`` are the line quads in
    line order; line l holds the words ``word_order[line_offsets[l]:line_offsets[l + 1]]`` in chain (reading) order; ``line_of_word[i]`` is the
    line of word i and ``next_word[i]`` the word linked after it, or -1.  Rows of ``quads`` from L on, entries of ``line_offsets`` after L and
    entries of the per-word tensors from n on are not written."""
    quads: torch.Tensor         # (N,4,2) fp32
    n_lines: torch.Tensor       # (1,) int32
    line_of_word: torch.Tensor  # (N,) int32
    word_order: torch.Tensor    # (N,) int32
    line_offsets: torch.Tensor  # (N+1,) int32
    next_word: torch.Tensor     # (N,) int32
    line_page_offs: torch.Tensor | None = None  # (B+1,) int32, find_lines_pages only: the lines of page p are line_page_offs[p]:line_page_offs[p+1]
    page_of_line: torch.Tensor | None = None    # (N,) int32, find_lines_pages only: rows up to L
    words: torch.Tensor | None = None           # (N,4,2) fp32: the word quads the lines were found in (what ``word_chars`` projects on a line's axis)


def _empty_lines(n: int, device, pages: int | None = None) -> TextLines:
    """the output tensors of ``find_lines`` for n words, or of ``find_lines_pages`` for n words on ``pages`` pages"""
    i32 = dict(dtype=torch.int32, device=device)
    counts = torch.empty if n else torch.zeros  # (with words, the scan kernels write them)
    out = TextLines(torch.empty(n, 4, 2, dtype=torch.float32, device=device), counts(1, **i32), torch.empty(n, **i32), torch.empty(n, **i32),
                    torch.empty(n + 1, **i32), torch.empty(n, **i32))
    if pages is not None:
        out.line_page_offs, out.page_of_line = counts(pages + 1, **i32), torch.empty(n, **i32)
    return out


def find_lines(quads: torch.Tensor, count: torch.Tensor | None = None, max_gap: float = 2.0, min_cos: float = 0.9,
               out: TextLines | None = None) -> TextLines:
    """Group word quads (N,4,2) into text lines in reading order by the geometric rule of DESIGN.md §14 (csrc/text_lines.hip): every word
    links to the nearest word that follows it along its own long axis within ``max_gap`` times the taller of the two heights, on the same
    baseline and with ``min_cos`` between the axes; a word accepts its nearest chooser; lines are the chains, sorted by their first word's
    (centre y, centre x, index).  ``count`` (1,) int32 on the device: only the first ``min(count, N)`` rows are words.  ``out``: write into
    these tensors instead of new ones.  Four stages of kernels, no host synchronisation; ``N == 0`` launches nothing."""
    q = _need_quads(quads, "find_lines")
    if count is not None:
        count = _need_counts(count, "find_lines")
    n = q.shape[0]
    if out is None:
        out = _empty_lines(n, q.device)
    else:
        for name, shape in (("quads", (n, 4, 2)), ("n_lines", (1,)), ("line_of_word", (n,)), ("word_order", (n,)), ("line_offsets", (n + 1,)), ("next_word", (n,))):
            t, dtype = getattr(out, name), torch.float32 if name == "quads" else torch.int32
            _need_cuda(t, "find_lines")
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise RuntimeError(f"find_lines: out.{name} must be a contiguous {shape} {dtype} tensor")
    out.words = q
    if n == 0:
        return out
    L = lib()
    ws_bytes = L.text_lines_ws_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    L.line_links(ptr(q), ptr(count), n, float(max_gap), float(min_cos), ptr(out.next_word), ptr(ws), ws_bytes)
    L.line_rank(ptr(count), n, ptr(out.next_word), ptr(ws), ws_bytes)
    L.line_order(ptr(count), n, ptr(out.n_lines), ptr(out.line_of_word), ptr(out.word_order), ptr(out.line_offsets), ptr(ws), ws_bytes)
    L.line_quads(ptr(q), ptr(count), n, ptr(out.n_lines), ptr(out.line_offsets), ptr(out.word_order), ptr(out.quads), ptr(ws), ws_bytes)
    return out


@dataclass
class ReadingOrder:
    """What ``reading_order`` returns, all on the device.  With L lines: ``line_order[k]`` is the line read at position k and ``new_block[k]``
    is 1 where that line starts a block; the positions ``line_page_offs[p]:line_page_offs[p + 1]`` hold the lines of page p (``0:L`` for a single
    page).  ``before`` is the relation the order was peeled from: bit ``b & 31`` of ``before[a, b >> 5]`` (read as uint32) says that line a comes
    before line b; bits between lines of different pages and rows and columns from L on are 0.  Entries of ``line_order`` and ``new_block`` from
    L on are not written."""
    line_order: torch.Tensor  # (N,) int32
    new_block: torch.Tensor   # (N,) int32, 0 / 1 by position
    before: torch.Tensor      # (N, ceil(N / 32)) int32 holding uint32 bit words


def reading_order(lines: TextLines, block_gap: float = 1.0, out: ReadingOrder | None = None) -> ReadingOrder:
    """The lines of ``find_lines`` / ``find_lines_pages`` in the order they are read, by the geometric rule of DESIGN.md §16
    (csrc/reading_order.hip): all lines are projected on the page's mean text direction; a line comes before every line it overlaps
    horizontally and lies above, and before every line entirely to its right unless a line between the two in height spans both (Breuel's two
    rules); the order emits, again and again, the smallest line index with no unemitted line before it, or the smallest unemitted one where
    the relation has a cycle.  A line starts a new block unless it overlaps the line read before it, lies below it and is at most ``block_gap``
    times the taller of the two heights away.  Lines of different pages are never related.  ``out``: write into these tensors instead of new
    ones.  Three stages of kernels, no host synchronisation; ``N == 0`` launches nothing."""
    who = "reading_order"
    if not isinstance(lines, TextLines):
        raise RuntimeError(f"{who}: expected the TextLines of find_lines or find_lines_pages")
    q = _need_quads(lines.quads, who)
    n = q.shape[0]
    n_lines = _need_counts(lines.n_lines, who)
    offs, B = None, 1
    if lines.line_page_offs is not None:
        _need_cuda(lines.line_page_offs, who)
        if lines.line_page_offs.dtype != torch.int32 or lines.line_page_offs.dim() != 1 or lines.line_page_offs.numel() < 2:
            raise RuntimeError(f"{who}: line_page_offs must be (B+1,) int32 with B >= 1")
        offs, B = lines.line_page_offs.contiguous(), lines.line_page_offs.numel() - 1
    i32 = dict(dtype=torch.int32, device=q.device)
    if out is None:
        out = ReadingOrder(torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, (n + 31) // 32, **i32))
    else:
        for name, shape in (("line_order", (n,)), ("new_block", (n,)), ("before", (n, (n + 31) // 32))):
            t = getattr(out, name)
            _need_cuda(t, who)
            if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous():
                raise RuntimeError(f"{who}: out.{name} must be a contiguous {shape} int32 tensor")
    if n == 0:
        return out
    L = lib()
    ws_bytes = L.reading_order_ws_bytes(n, B)
    if ws_bytes <= 0:
        raise RuntimeError(f"{who}: {n} lines on {B} pages are not supported")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    L.reading_relation(ptr(q), ptr(n_lines), ptr(offs), B, n, ptr(out.before), ptr(ws), ws_bytes)
    L.reading_peel(ptr(n_lines), ptr(offs), B, n, ptr(out.before), ptr(out.line_order), ptr(ws), ws_bytes)
    L.reading_blocks(ptr(n_lines), ptr(offs), B, n, float(block_gap), ptr(out.line_order), ptr(out.new_block), ptr(ws), ws_bytes)
    return out


def page_text(result: list[dict]) -> str:
    """One page's result list of ``ocr_lines`` / ``read_lines`` / ``ocr_pages`` with ``reading_order=True`` -> its text: the lines of a block
    joined with a newline, blocks with a blank line.  A list without ``"block"`` (line order) is one block."""
    blocks, last = [], None
    for line in result:
        block = line.get("block", 0)
        if not blocks or block != last:
            blocks.append([])
        blocks[-1].append(line["text"])
        last = block
    return "\n\n".join("\n".join(b) for b in blocks)


def find_lines_pages(quads: torch.Tensor, page_of_word: torch.Tensor, word_offs: torch.Tensor, max_gap: float = 2.0, min_cos: float = 0.9) -> TextLines:
    """``find_lines`` over the flat words of B pages (``detect_words_batch``'s ``quads``, ``page_of_word`` and ``word_offs``): the rule of
    DESIGN.md §14 with two additions -- a word links only to words of its own page, and lines are ordered by (page, centre y, centre x, word
    index) of their first word.  Indices in the result count through the flat arrays; ``line_page_offs`` (B+1,) and ``page_of_line`` say which
    lines are which page's.  The kernels stage only the words of a workgroup's own page, so the work is the sum of n_p^2.  No host
    synchronisation; N == 0 launches nothing."""
    q = _need_quads(quads, "find_lines_pages")
    n = q.shape[0]
    for t in (page_of_word, word_offs):
        _need_cuda(t, "find_lines_pages")
    if page_of_word.dtype != torch.int32 or tuple(page_of_word.shape) != (n,):
        raise RuntimeError("find_lines_pages: page_of_word must be (N,) int32")
    if word_offs.dtype != torch.int32 or word_offs.dim() != 1 or word_offs.numel() < 2:
        raise RuntimeError("find_lines_pages: word_offs must be (B+1,) int32 with B >= 1")
    B = word_offs.numel() - 1
    offs = word_offs.contiguous()
    out = _empty_lines(n, q.device, B)
    out.words = q
    if n == 0:
        return out
    L = lib()
    ws_bytes = L.text_lines_pages_ws_bytes(n, B)
    if ws_bytes <= 0:
        raise RuntimeError(f"find_lines_pages: {n} words on {B} pages are not supported")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    L.line_links_pages(ptr(q), ptr(offs), B, n, float(max_gap), float(min_cos), ptr(out.next_word), ptr(ws), ws_bytes)
    L.line_rank_pages(ptr(offs), B, n, ptr(out.next_word), ptr(ws), ws_bytes)
    L.line_order_pages(ptr(offs), B, n, ptr(out.n_lines), ptr(out.line_of_word), ptr(out.word_order), ptr(out.line_offsets), ptr(out.line_page_offs),
                       ptr(out.page_of_line), ptr(ws), ws_bytes)
    L.line_quads_pages(ptr(q), ptr(offs), B, n, ptr(out.n_lines), ptr(out.line_offsets), ptr(out.word_order), ptr(out.quads), ptr(ws), ws_bytes)
    return out


def split_by_page(items: list, offs: list) -> list[list]:
    """flat results grouped by page -> one list per page: ``items[offs[p]:offs[p + 1]]`` (``offs``: B + 1 ascending host offsets)"""
    if any(b < a for a, b in zip(offs, offs[1:])) or (offs and (offs[0] != 0 or offs[-1] != len(items))):
        raise RuntimeError("split_by_page: the offsets must ascend from 0 to the number of items")
    return [items[a:b] for a, b in zip(offs, offs[1:])]

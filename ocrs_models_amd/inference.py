"""Page OCR on the GPU: from a page image to word quads, rectified word crops and recognised text.

The detection half is the reference's evaluation script (ocrs_models/eval_detection.py:19-69): resize the page to ``MASK_SIZE``, eval
forward, binarise, nearest-resize the mask back to the page, ``extract_cc_quads``, ``expand_quads(dist=SHRINK_DISTANCE)``.  The
recognition half prepares every word rectangle the way the reference prepares line crops (datasets/hiertext.py:271-294: crop,
``transform_image``, antialiased resize to 64 rows, width by aspect ratio) and pads them into batches as ``collate_samples`` does
(train_rec.py:285-299), then runs the recogniser's eval forward and the greedy CTC decode of ``train_rec.test``.

Every function takes and returns device tensors and has no CPU path; the pixel work is in csrc/ocr_infer.hip (C ABI section "page
inference" of include/ocrs_hip.h).

Host synchronisations per page (``ocr_page``), and there are no others:

1. the component count (``extract_cc_quads_device`` reads N to slice the quads);
2. the crop plan's totals (``CropPlan.host``: they size the packed crop buffer, the resize workspace and the batches);
3. the decoded labels (every chunk's forward and decode are queued first, then the label copies are waited for).

Geometry rules (restated for the tests in tests/ocr_ref.py).  Quad coordinates are pixel-centre indices: coordinate k is the centre of
pixel k, as ``extract_cc_quads`` produces them.

* Expansion.  For a rectangle with corners c0..c3: the centre (mean of the corners) and the unit axes along c0->c1 and c1->c2; ``dist`` is
  added to each half-extent; corner k of the output corresponds to corner k of the input.  For any non-degenerate rectangle this is
  shapely's mitred ``parallel_offset`` followed by ``minimum_rotated_rectangle`` (postprocess.py:39-65).  A zero-length ring (all four
  corners equal) is returned unchanged, as in the reference.  A zero-area ring of non-zero length -- what the hull code returns as
  ``[a, b, b, a]`` -- becomes the rectangle around the segment, ``2 * dist`` thick and ``dist`` longer at each end (the missing axis is the
  normal of the other one; a quad whose first two sides are both empty is returned unchanged).  shapely is not installed where this is
  built, so the vertex ORDER of the result and this degenerate case are UNPINNED in the sense of postprocess.py's docstring.
* Crop frame.  The width axis u is the longer of the sides c0->c1 and c1->c2; on a tie the side with the larger |x| component (the first
  one if that ties too).  The sign of u is chosen so that u.x > 0, or u.x == 0 and u.y > 0 (a point gets u = (1, 0)).  v = (-u.y, u.x) points
  down the page and is never mirrored.  The origin is the corner with the smallest projections on u and v (the smallest sum of the two).
  ``w_i = max(1, round(long))``, ``h_i = max(1, round(short))`` (round half to even).  Sample (y, x) sits at
  ``origin + (x + 0.5) / w_i * long * u + (y + 0.5) / h_i * short * v``; sampling is bilinear on the ``transform_image`` values of the page,
  with coordinates clamped to the page (border padding).  All of this is fp32 arithmetic.
* Output width.  ``line_output_width(h_i, w_i, output_height)``, unchanged.

Lines.  ``find_lines`` groups the word quads into text lines in reading order (csrc/text_lines.hip, C ABI section "text lines"; the rule is
stated once in DESIGN.md §14 and restated for the tests in tests/lines_ref.py) without a host synchronisation, and ``ocr_lines`` is
``ocr_page`` with that stage in between: one crop and one string per line, the recogniser's training unit, with the same three waits.

Reading order (csrc/reading_order.hip, C ABI section "reading order"; restated for the tests in tests/reading_ref.py).  Line
order is top to bottom, so the columns of a page interleave.  ``reading_order`` puts the lines of every page into the order they are read,
column by column, and marks where a new block starts, again without a host synchronisation; ``read_lines``, ``ocr_lines`` and ``ocr_pages`` take
``reading_order=True`` to return their lines that way, with the same three waits; ``page_text`` joins such a result into one string.

Characters (csrc/char_spans.hip, C ABI section "characters"; restated for the tests in tests/chars_ref.py).  With ``chars=True``
``recognize_crops``, ``ocr_page``, ``read_lines``, ``ocr_lines`` and ``ocr_pages`` keep what the greedy decode otherwise drops -- the time steps every
character was collapsed from and its log-prob -- and return, next to the keys they always return, every character's quad on the page
(``char_boxes``: time steps to crop columns to the page through the crop frame) and, for lines, the characters and the text of every word
(``word_chars``: neighbouring words split the line half way between them; spaces at the ends of a range are dropped); the same three waits.

Beam search (csrc/ctc_beam.hip, C ABI section "beam search"; restated for the tests in tests/beam_ref.py).  With ``beam_width=W``
the same functions decode every crop by CTC prefix beam search -- the most probable labelling among the W prefixes kept per step, where the
greedy decode returns the labelling of the single most probable alignment -- and add ``"log_prob"``, the labelling's log-mass, to every
dict; the spans that ``chars=True`` needs come from a forced alignment of the chosen labelling.  None, the default, is the greedy path
unchanged; the same three waits either way.

Language model (``text.CharLM`` / ``LMGain``; restated for the tests in tests/beam_lm_ref.py).  With ``lm=model.gain(...)`` next to
``beam_width`` the beam ranks every prefix by its log-mass + the gains of a character n-gram table and every dict gains ``"lm_score"`` next to
``"log_prob"``, which keeps its meaning.  None, the default, is the plain beam unchanged; ``lm`` without ``beam_width`` is an argument error; the
same waits.

Tiles (csrc/ocr_tiles.hip, C ABI section "tiles"; restated for the tests in tests/tiles_ref.py).  With ``tile=(Th, Tw)`` the detection
drivers cut the page into overlapping windows at (near) native resolution, run the detector on every window and compose ONE page mask from
the tiles before the components are labelled; None, the default, is the whole-page path unchanged; the same waits.

Page batches (C ABI section "page batches").  ``ocr_pages`` reads a list of pages of any sizes with ONE detection forward, one
zero-padded mask canvas, one line stage that keeps to each word's own page, one pooled crop plan and one set of width-sorted recognition chunks
for the crops of all pages: three host synchronisations for the whole batch (the word offsets, the plan's totals, the labels) instead of three
per page.  The single-page functions above are what its tests compare it with.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

from ._lib import lib, ptr
from .input_pipeline import _need_cuda, resize, transform_image
from .text import (DEFAULT_ALPHABET, LMGain, _check_beam_width, _check_lm, beam_decode_spans_async, decode_text, greedy_decode_batch_async, greedy_decode_spans_async, round_up,
                   span_arrays)

MASK_SIZE = (800, 600)   # train_detection.py's mask_size: the size the detection model is trained and evaluated at
SHRINK_DISTANCE = 3.0    # datasets/util.py: how far text polygons are shrunk when training masks are made
_OW_BINS = 801           # line_output_width() is in [10, 800]


# Argument checks shared by the public functions; ``who`` is the caller's name, so every message starts with the function the user called.
def _need_quads(quads: torch.Tensor, who: str, shape: str = "(N,4,2)", plan: CropPlan | None = None) -> torch.Tensor:
    """fp32 quads of that shape on the device (``plan``: as many as the plan has rows) -> contiguous"""
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


def binarize_resize(prob: torch.Tensor, size, threshold: float = 0.5) -> torch.Tensor:
    """(B,1,h,w) or (h,w) fp32 probabilities -> uint8 0/1 mask (B,1,H,W) or (H,W): ``binarize_mask`` followed by
    ``resize(.., size, InterpolationMode.NEAREST)`` (eval_detection.py:54-57) in one launch."""
    _need_cuda(prob, "binarize_resize")
    if prob.dtype != torch.float32 or not (prob.dim() == 2 or (prob.dim() == 4 and prob.shape[1] == 1)):
        raise RuntimeError("binarize_resize: expected (B,1,h,w) or (h,w) float32 probabilities")
    H, W = int(size[0]), int(size[1])
    h, w = prob.shape[-2:]
    B = prob.shape[0] if prob.dim() == 4 else 1
    src = prob.contiguous()
    out = torch.empty((B, 1, H, W) if prob.dim() == 4 else (H, W), dtype=torch.uint8, device=prob.device)
    lib().binarize_resize_nearest(ptr(src), ptr(out), B, h, w, H, W, float(threshold))
    return out


def expand_quads(quads: torch.Tensor, dist: float, counts: torch.Tensor | None = None) -> torch.Tensor:
    """``expand_quads`` (postprocess.py:68-76) on the device: (N,4,2) or (B,cap,4,2) fp32 -> the same shape, every rectangle's edges moved
    outward by ``dist``.  ``counts`` (B,) int32 on the device: rows past ``counts[b]`` are returned as they came."""
    q = _need_quads(quads, "expand_quads", "(B,cap,4,2)" if quads.dim() == 4 else "(N,4,2)")
    B, cap = (1, q.shape[0]) if q.dim() == 3 else (q.shape[0], q.shape[1])
    if counts is None:
        out = torch.empty_like(q)
    else:
        counts = _need_counts(counts, "expand_quads", B)
        out = q.clone()
    lib().expand_quads(ptr(q), ptr(out), ptr(counts), B, cap, float(dist))
    return out


def detect_words(model, page_u8: torch.Tensor, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE, tile=None, overlap=None,
                 tile_batch: int = 16) -> dict:
    """eval_detection.py:32-67 for one (1,H,W) uint8 page on the device -> ``probs`` (h,w), ``text_mask`` (H,W) uint8, ``quads`` (N,4,2) in
    page coordinates and ``n``.  The model must be in eval mode.  One host synchronisation (the component count).
    ``tile = (Th, Tw)``: detect in overlapping tiles of that many page pixels instead of squeezing the whole page to ``size``:
    every window of ``tile_plan(H, W, tile, overlap)`` is resized to ``size`` on its own, the eval forward runs over the tiles in chunks of
    at most ``tile_batch``, and the tile probabilities are composed into ONE page mask -- every pixel from the tile that owns it -- before the
    components are labelled, so a word across a seam stays one word.  ``probs`` becomes (T,h,w) and the dict gains ``tiles``, the (T,5) int32
    device table ``(page, y0, x0, th, tw)``.  ``overlap=None``: an eighth of the tile.  ``tile=None``, the default, is the path above unchanged;
    the same one synchronisation either way."""
    from .postprocess import extract_cc_quads_device

    _need_cuda(page_u8, "detect_words")
    if page_u8.dtype != torch.uint8 or page_u8.dim() != 3 or page_u8.shape[0] != 1:
        raise RuntimeError("detect_words: expected a (1,H,W) uint8 page")
    if model.training:
        raise RuntimeError("detect_words: the model must be in eval mode (model.eval())")
    _check_tile_args("detect_words", tile, tile_batch)
    H, W = (int(v) for v in page_u8.shape[-2:])
    extra = {}
    if tile is None:
        img = resize(transform_image(page_u8), size)
        with torch.inference_mode():
            probs = model(img.unsqueeze(0))[0, 0]
        text_mask = binarize_resize(probs, (H, W), threshold)
    else:
        if H < 1 or W < 1:
            raise RuntimeError("detect_words: a tiled page needs at least one pixel")
        dev = page_u8.device
        store = (page_u8.contiguous().view(-1), _to_device_async([0], torch.int64, dev), _to_device_async([[H, W]], torch.int32, dev))  # the page is its own store
        probs, masks, tables = _detect_tiles(model, store, [(H, W)], (H, W), size, threshold, tile, overlap, tile_batch, "detect_words")
        text_mask, extra = masks[0], {"tiles": tables.tiles}
    quads = expand_quads(extract_cc_quads_device(text_mask), expand)
    return {"probs": probs, "text_mask": text_mask, "quads": quads, "n": quads.shape[0], **extra}


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


@dataclass
class CharSpans:
    """What the recogniser's greedy decode keeps per character, on the device: one row per crop at a pitch of ``ld``
    entries, rows in the crop plan's width-sorted order (row p is the crop of quad ``plan.table[p, 7]``).  Character k of row p has label
    ``labels[p, k]``, was collapsed from the time steps ``t0[p, k] .. t1[p, k]`` and has the log-prob ``peak[p, k]``, the largest of its class
    over those steps; ``lens[p]`` characters.  Entries of a row from ``lens[p]`` on are not written.  ``buf`` is the one int32 buffer all five
    are views of (``text.span_arrays``): one copy brings them to the host.  ``scores`` (R,) fp32, beam decodes only: the
    log-mass of every row's labelling; None for the greedy decode.  ``lm_scores`` (R,) fp32, beam decodes with a language model only
    (DESIGN.md §19): the gains of every row's labelling; None otherwise."""
    buf: torch.Tensor
    labels: torch.Tensor  # (R,ld) int32
    t0: torch.Tensor      # (R,ld) int32
    t1: torch.Tensor      # (R,ld) int32
    peak: torch.Tensor    # (R,ld) fp32
    lens: torch.Tensor    # (R,) int32
    scores: torch.Tensor | None = None  # (R,) fp32
    lm_scores: torch.Tensor | None = None  # (R,) fp32

    def arrays(self):
        return self.buf, self.labels, self.t0, self.t1, self.peak, self.lens


@dataclass
class CharBoxes:
    """What ``char_boxes`` returns, on the device, rows and pitch as in ``CharSpans``: ``s0`` / ``s1`` (R,ld) fp32, where the character starts
    and ends along its crop's width axis in page pixels, and ``quads`` (R,ld,4,2) fp32, its rectangle on the page."""
    s0: torch.Tensor
    s1: torch.Tensor
    quads: torch.Tensor


def _check_batches(rec_model, batches, who: str):
    for b in batches[0]:
        _need_cuda(b, who)
    if rec_model.training:
        raise RuntimeError(f"{who}: the model must be in eval mode (model.eval())")


def _check_lm_args(who: str, beam_width, lm):
    """``lm`` is a keyword of the beam decode: without ``beam_width`` it is an argument error"""
    if lm is not None:
        if beam_width is None:
            raise RuntimeError(f"{who}: lm needs beam_width (the greedy decode has no hypotheses to choose among)")
        _check_lm(who, lm)


def decode_crop_spans(rec_model, batches, beam_width: int | None = None, lm: LMGain | None = None) -> CharSpans:
    """Eval forward of the recogniser per batch, as ``recognize_crops``, with the decode that keeps the spans: the chunks write their rows
    into one set of arrays whose pitch is the longest chunk's number of time steps.  Every forward is queued before the first decode (the
    pitch is known once the last forward has its shape); no synchronisation, nothing is copied.  ``beam_width``: None = the greedy decode;
    a width = prefix beam search and forced alignment (``text.beam_decode_spans_async``) into the same arrays, with
    ``scores`` set.  ``lm`` (with a width): the gain table of a language model fused into the beam's ranking, with
    ``lm_scores`` set."""
    _check_lm_args("decode_crop_spans", beam_width, lm)
    _check_batches(rec_model, batches, "decode_crop_spans")
    if beam_width is not None:
        _check_beam_width("decode_crop_spans", beam_width)
    imgs, image_widths, _ = batches
    with torch.inference_mode():
        lps = [rec_model(img) for img in imgs]
    rows = sum(lp.shape[1] for lp in lps)
    dev = lps[0].device if lps else torch.device("cuda", torch.cuda.current_device())
    spans = CharSpans(*span_arrays(rows, max([lp.shape[0] for lp in lps], default=1), dev))
    if beam_width is not None:
        spans.scores = torch.empty(rows, dtype=torch.float32, device=dev)
    if lm is not None:
        spans.lm_scores = torch.empty(rows, dtype=torch.float32, device=dev)
    row = 0
    for lp, iw in zip(lps, image_widths):
        if beam_width is None:
            greedy_decode_spans_async(lp, iw.div(4, rounding_mode="floor"), spans.arrays(), row)
        else:
            beam_decode_spans_async(lp, iw.div(4, rounding_mode="floor"), beam_width, spans.arrays(), row, spans.scores, lm, spans.lm_scores)
        row += lp.shape[1]
    return spans


def char_boxes(quads: torch.Tensor, plan: CropPlan, spans: CharSpans) -> CharBoxes:
    """Where every character of every crop sits on the page (``ocrs_char_boxes``): ``quads`` (N,4,2) and ``plan`` are what
    the crops were cut with, ``spans`` what ``decode_crop_spans`` wrote for them.  Time step t is centred on column 4 t of the resized crop; a
    character reaches from two columns before its first step to two after its last, clamped to the crop, and that stretch of the crop's
    width axis, over the crop's full height, is mapped to the page through the crop frame.  One launch, no synchronisation."""
    q = _need_quads(quads, "char_boxes", plan=plan)
    rows, ld = spans.labels.shape
    if rows > q.shape[0]:
        raise RuntimeError("char_boxes: more span rows than quads")
    f32 = dict(dtype=torch.float32, device=q.device)
    out = CharBoxes(torch.empty(rows, ld, **f32), torch.empty(rows, ld, **f32), torch.empty(rows, ld, 4, 2, **f32))
    lib().char_boxes(ptr(q), ptr(plan.table), q.shape[0], rows, ld, ptr(spans.lens), ptr(spans.t0), ptr(spans.t1), ptr(out.s0), ptr(out.s1), ptr(out.quads))
    return out


def space_label(alphabet) -> int:
    """the label of the space character (``alphabet.index(" ") + 1``), or -1 if the alphabet has none"""
    alphabet = list(alphabet)
    return alphabet.index(" ") + 1 if " " in alphabet else -1


def word_chars(lines: TextLines, plan: CropPlan, spans: CharSpans, boxes: CharBoxes, alphabet=DEFAULT_ALPHABET) -> torch.Tensor:
    """Which characters of its line every word lies over (``ocrs_word_chars``): ``lines`` from ``find_lines`` /
    ``find_lines_pages``, ``plan`` made from ``lines.quads``, ``spans`` and ``boxes`` of those line crops -> (N,2) int32 on the device, indexed by
    the flat word index: ``(first, end)`` into the characters of the word's line.  Neighbouring words split the line half way between the end
    of one and the start of the next along the line's axis; spaces at either end of a range are dropped.  One launch, no synchronisation."""
    who = "word_chars"
    if not isinstance(lines, TextLines) or lines.words is None:
        raise RuntimeError(f"{who}: expected the TextLines of find_lines or find_lines_pages")
    words = _need_quads(lines.words, who)
    _need_quads(lines.quads, who, plan=plan)
    n = words.shape[0]
    rows, ld = spans.labels.shape
    if rows > n or tuple(boxes.s0.shape) != (rows, ld):
        raise RuntimeError(f"{who}: spans and boxes must be those of the lines' crops")
    out = torch.empty(n, 2, dtype=torch.int32, device=words.device)
    lib().word_chars(ptr(words), n, ptr(lines.quads), ptr(lines.n_lines), n, ptr(lines.line_offsets), ptr(lines.word_order), ptr(plan.table), rows, ld,
                     ptr(spans.labels), ptr(spans.lens), ptr(boxes.s0), ptr(boxes.s1), space_label(alphabet), ptr(out))
    return out


def chars_to_host(spans: CharSpans, boxes: CharBoxes, alphabet=DEFAULT_ALPHABET, ranges: torch.Tensor | None = None):
    """The characters on the host, in the rows' (width-sorted) order: ``(texts, chars, ranges)`` with ``chars[p] = {"char_quads": [4x2 lists],
    "char_log_probs": [floats]}``, one entry per character of ``texts[p]``, and ``ranges`` the (N,2) result of ``word_chars`` as a list (None
    without it).  Spans of a beam decode (``spans.scores``) add ``"log_prob"`` to every ``chars[p]``, those of one with a language model
    (``spans.lm_scores``) ``"lm_score"`` too.  The copies are queued on the current
    stream and there is ONE wait for all of them."""
    alphabet = list(alphabet)
    sp_h, cq_h = _to_host_async(spans.buf), _to_host_async(boxes.quads)
    rg_h = None if ranges is None else _to_host_async(ranges)
    sc_h = None if spans.scores is None else _to_host_async(spans.scores)
    lm_h = None if spans.lm_scores is None else _to_host_async(spans.lm_scores)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(spans.buf.device))
    done.synchronize()
    rows, ld = spans.labels.shape
    labels, peak = sp_h[:rows * ld].view(rows, ld), sp_h[3 * rows * ld:4 * rows * ld].view(rows, ld).view(torch.float32)
    lens = [max(n, 0) for n in sp_h[4 * rows * ld:].tolist()]  # (-1: a beam row without any labelling of finite mass)
    texts = [decode_text(labels[p, :n], alphabet) for p, n in enumerate(lens)]
    chars = [{"char_quads": cq_h[p, :n].tolist(), "char_log_probs": peak[p, :n].tolist()} for p, n in enumerate(lens)]
    if sc_h is not None:  # a beam decode: the labelling's log-mass travels with the characters
        for d, sc in zip(chars, sc_h.tolist()):
            d["log_prob"] = sc
    if lm_h is not None:
        for d, sc in zip(chars, lm_h.tolist()):
            d["lm_score"] = sc
    return texts, chars, None if rg_h is None else rg_h.tolist()


def _beam_texts_to_host(spans: CharSpans, alphabet):
    """texts, scores and language-model scores (None without a model) of a beam decode's span rows on the host, in the rows' order: two or
    three copies and ONE wait, for the event behind them"""
    sp_h, sc_h = _to_host_async(spans.buf), _to_host_async(spans.scores)
    lm_h = None if spans.lm_scores is None else _to_host_async(spans.lm_scores)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(spans.buf.device))
    done.synchronize()
    rows, ld = spans.labels.shape
    lens, alphabet = [max(n, 0) for n in sp_h[4 * rows * ld:].tolist()], list(alphabet)  # (-1: a row without any labelling of finite mass)
    texts = [decode_text(row[:n], alphabet) for row, n in zip(sp_h[:rows * ld].view(rows, ld), lens)]
    return texts, sc_h.tolist(), None if lm_h is None else lm_h.tolist()


def recognize_crops(rec_model, batches, alphabet=DEFAULT_ALPHABET, chars: bool = False, beam_width: int | None = None, lm: LMGain | None = None):
    """Eval forward of the recogniser per batch with ``input_lengths = image_width // 4`` (as ``train_rec.test``) and the device greedy
    decode.  ``batches`` is what ``crops_to_batches`` returned: ``(batch tensors, image widths, perm)``.  Returns the strings in quad order.
    Every chunk's forward and decode are queued before the first label copy is waited for.  ``chars=True``: ``(strings in quad order,
    CharSpans)`` -- the same strings from the decode that keeps every character's time steps and log-prob (``decode_crop_spans``), whose
    device arrays ``char_boxes`` and ``word_chars`` take; one wait, for the one copy of the span buffer.  ``beam_width``: the
    strings of prefix beam search instead -- ``(strings, log-probs of the strings)``, with ``chars=True`` ``(strings, CharSpans, log-probs)``;
    both forms decode into one span buffer and wait once.  ``lm`` (with ``beam_width``): the beam ranks by log-prob + the
    language model's gains, and the gains of the strings are appended to either tuple; the same one wait."""
    _check_lm_args("recognize_crops", beam_width, lm)
    if beam_width is not None:
        spans = decode_crop_spans(rec_model, batches, beam_width, lm)
        texts, scores, lm_sc = _beam_texts_to_host(spans, alphabet)
        texts, scores = [texts[p] for p in batches[2]], [scores[p] for p in batches[2]]
        tail = () if lm_sc is None else ([lm_sc[p] for p in batches[2]],)
        return ((texts, spans, scores) if chars else (texts, scores)) + tail
    if chars:
        spans = decode_crop_spans(rec_model, batches)
        sp_h = _to_host_async(spans.buf)
        torch.cuda.current_stream(spans.buf.device).synchronize()
        rows, ld = spans.labels.shape
        lens, alphabet = sp_h[4 * rows * ld:].tolist(), list(alphabet)
        texts = [decode_text(row[:n], alphabet) for row, n in zip(sp_h[:rows * ld].view(rows, ld), lens)]
        return [texts[p] for p in batches[2]], spans
    batches, image_widths, perm = batches
    for b in batches:
        _need_cuda(b, "recognize_crops")
    if rec_model.training:
        raise RuntimeError("recognize_crops: the model must be in eval mode (model.eval())")
    alphabet = list(alphabet)
    handles = []
    with torch.inference_mode():
        for img, iw in zip(batches, image_widths):
            handles.append(greedy_decode_batch_async(rec_model(img), iw.div(4, rounding_mode="floor")))
    texts = [decode_text(row, alphabet) for h in handles for row in h.result()]
    return [texts[p] for p in perm]


def _read_crops(rec_model, batches, alphabet, words: torch.Tensor, lines: TextLines | None = None, n_lines: int = 0, order: ReadingOrder | None = None,
                line_page_offs: list | None = None, chars_plan: CropPlan | None = None, beam_width: int | None = None, lm: LMGain | None = None) -> list[dict]:
    """The tail of ``ocr_page``, ``read_lines`` and ``ocr_pages``: ``recognize_crops`` on ``batches``, then the flat result list -- one
    ``{"quad", "text"}`` per word, or with ``lines`` one ``{"quad", "text", "words"}`` per line for its first ``n_lines`` lines.  With ``order``
    the list is in reading order -- position k holds line ``order.line_order[k]`` -- and every dict has ``"block"``, counted from 0 on every
    page (``line_page_offs``: the host offsets of the pages' lines; None: one page).  The word quads, the line tables and the reading order
    travel to the host ahead of the recogniser on the same stream: they have arrived when the labels have (no wait of their own).
    ``chars_plan`` (the plan the crops were cut with; ``chars=True`` of the callers): every dict also has ``"char_quads"`` and
    ``"char_log_probs"``, line dicts ``"word_chars"`` and ``"word_texts"`` too.  The boxes and word ranges are queued behind the
    decodes and copied with the labels: still one wait here.  ``beam_width``: the texts of prefix beam search and
    ``"log_prob"`` in every dict; still one wait.  ``lm``: the beam's ranking includes the language model's gains and
    every dict has ``"lm_score"`` next to ``"log_prob"``; its copy joins the same wait."""
    words_h = _to_host_async(words)
    if lines is not None:
        lq_h, order_h, offs_h = (_to_host_async(t) for t in (lines.quads, lines.word_order, lines.line_offsets))
    if order is not None:
        ro_h, nb_h = _to_host_async(order.line_order), _to_host_async(order.new_block)
    scores = lm_sc = None
    if chars_plan is None and beam_width is not None and lm is not None:
        texts, scores, lm_sc = recognize_crops(rec_model, batches, alphabet, beam_width=beam_width, lm=lm)
    elif chars_plan is None and beam_width is not None:
        texts, scores = recognize_crops(rec_model, batches, alphabet, beam_width=beam_width)
    elif chars_plan is None:
        texts = recognize_crops(rec_model, batches, alphabet)
    else:
        spans = decode_crop_spans(rec_model, batches, beam_width, lm)
        boxes = char_boxes(words if lines is None else lines.quads, chars_plan, spans)
        ranges = None if lines is None else word_chars(lines, chars_plan, spans, boxes, alphabet)
        texts, chars, ranges = chars_to_host(spans, boxes, alphabet, ranges)
        perm = batches[2]
        texts, chars = [texts[p] for p in perm], [chars[p] for p in perm]
    wl = words_h.tolist()
    if lines is None:
        if chars_plan is not None:
            return [{"quad": q, "text": t, **c} for q, t, c in zip(wl, texts, chars)]
        if lm_sc is not None:
            return [{"quad": q, "text": t, "log_prob": sc, "lm_score": ls} for q, t, sc, ls in zip(wl, texts, scores, lm_sc)]
        if scores is not None:
            return [{"quad": q, "text": t, "log_prob": sc} for q, t, sc in zip(wl, texts, scores)]
        return [{"quad": q, "text": t} for q, t in zip(wl, texts)]
    word_order, offs, lq = order_h.tolist(), offs_h[:n_lines + 1].tolist(), lq_h[:n_lines].tolist()
    out = [{"quad": lq[l], "text": texts[l], "words": [wl[i] for i in word_order[offs[l]:offs[l + 1]]]} for l in range(n_lines)]
    if scores is not None:
        for l, d in enumerate(out):
            d["log_prob"] = scores[l]
    if lm_sc is not None:
        for l, d in enumerate(out):
            d["lm_score"] = lm_sc[l]
    if chars_plan is not None:
        for l, d in enumerate(out):
            rg = [ranges[i] for i in word_order[offs[l]:offs[l + 1]]]
            d.update(chars[l], word_chars=rg, word_texts=[d["text"][a:b] for a, b in rg])
    if order is None:
        return out
    ro, nb, read = ro_h[:n_lines].tolist(), nb_h[:n_lines].tolist(), []
    pages = [0, n_lines] if line_page_offs is None else line_page_offs
    for a, b in zip(pages, pages[1:]):
        block = -1
        for k in range(a, b):
            block += 1 if (nb[k] or k == a) else 0
            read.append({**out[ro[k]], "block": block})
    return read


def ocr_page(det_model, rec_model, page_u8: torch.Tensor, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE,
             output_height: int = 64, max_batch: int = 256, width_unit: int = 64, alphabet=DEFAULT_ALPHABET, chars: bool = False,
             beam_width: int | None = None, lm: LMGain | None = None, tile=None, overlap=None, tile_batch: int = 16) -> list[dict]:
    """Page (1,H,W) uint8 on the device -> ``[{"quad": (4,2) list, "text": str}, ...]`` in the raster order of ``extract_cc_quads_device``.
    A page without components returns ``[]`` without launching the recogniser.  ``chars=True``: every dict also has ``"char_quads"``, the
    rectangle of every character of ``"text"`` on the page, and ``"char_log_probs"``, the recogniser's log-prob of each; the
    same three waits.
    ``beam_width``: decode by CTC prefix beam search with that many prefixes instead of greedily; every dict gains
    ``"log_prob"``, the log-mass of its text; None = the greedy decode, unchanged; the same waits.
    ``lm`` (with ``beam_width``): the ``LMGain`` of a character language model (``text.CharLM.gain``); the beam ranks by
    log-prob + gains and every dict also gains ``"lm_score"``, the gains of its text; None = the plain beam, unchanged; the same waits.
    ``tile``, ``overlap``, ``tile_batch``: detect in overlapping tiles, as ``detect_words`` describes; the same waits."""
    _check_lm_args("ocr_page", beam_width, lm)
    det = detect_words(det_model, page_u8, size, threshold, expand, tile, overlap, tile_batch)
    if det["n"] == 0:
        return []
    quads = det["quads"]
    plan = crop_plan(quads, output_height)
    packed = rectify_crops(page_u8, quads, plan)
    return _read_crops(rec_model, crops_to_batches(packed, plan, max_batch, width_unit), alphabet, quads, chars_plan=plan if chars else None,
                       beam_width=beam_width, lm=lm)


# ------------------------------------------------------------------ words -> lines -------------------------------------------------------
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


_order_lines = reading_order  # (the drivers below take a keyword of the stage's name)


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


def read_lines(rec_model, page_u8: torch.Tensor, quads: torch.Tensor, output_height: int = 64, max_batch: int = 256, width_unit: int = 64,
               alphabet=DEFAULT_ALPHABET, max_gap: float = 2.0, min_cos: float = 0.9, reading_order: bool = False, block_gap: float = 1.0,
               chars: bool = False, beam_width: int | None = None, lm: LMGain | None = None) -> list[dict]:
    """The half of ``ocr_lines`` after detection: word quads (N,4,2), N > 0, on the device -> the list ``ocr_lines`` returns.  Two host
    synchronisations: the plan's totals (which bring the line count) and the labels; the line table and the quads are copied to the host
    ahead of the recogniser on the same stream, so they have arrived when the labels have -- and so has the reading order, which with
    ``reading_order=True`` is queued behind the line stage and changes nothing about the crops (lines are cropped in line order).
    ``chars=True``: the characters' quads, log-probs and word ranges as ``ocr_lines`` describes them, queued behind the decodes; the same waits.
    ``beam_width``: decode by CTC prefix beam search with that many prefixes instead of greedily; every dict gains
    ``"log_prob"``, the log-mass of its text; None = the greedy decode, unchanged; the same waits.
    ``lm`` (with ``beam_width``): the ``LMGain`` of a character language model (``text.CharLM.gain``); the beam ranks by
    log-prob + gains and every dict also gains ``"lm_score"``, the gains of its text; None = the plain beam, unchanged; the same waits."""
    _check_lm_args("read_lines", beam_width, lm)
    lines = find_lines(quads, None, max_gap, min_cos)
    order = _order_lines(lines, block_gap) if reading_order else None
    plan = crop_plan(lines.quads, output_height, lines.n_lines)
    packed = rectify_crops(page_u8, lines.quads, plan)
    batches = crops_to_batches(packed, plan, max_batch, width_unit)
    return _read_crops(rec_model, batches, alphabet, quads, lines, plan.host()[0], order, chars_plan=plan if chars else None, beam_width=beam_width,
                       lm=lm)


def ocr_lines(det_model, rec_model, page_u8: torch.Tensor, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE,
              output_height: int = 64, max_batch: int = 256, width_unit: int = 64, alphabet=DEFAULT_ALPHABET, max_gap: float = 2.0,
              min_cos: float = 0.9, reading_order: bool = False, block_gap: float = 1.0, chars: bool = False,
              beam_width: int | None = None, lm: LMGain | None = None, tile=None, overlap=None, tile_batch: int = 16) -> list[dict]:
    """Page (1,H,W) uint8 on the device -> ``[{"quad": line quad, "text": str, "words": [word quads in chain order]}, ...]`` in line order:
    ``detect_words``, ``find_lines``, then one crop per LINE through the stages ``ocr_page`` runs per word.  The same three host
    synchronisations as ``ocr_page``: the component count, the plan's totals and the labels (``read_lines``).  A page without components
    returns ``[]`` without launching the recogniser.  ``reading_order=True``: the same dicts in reading order (column by column
    where line order interleaves the columns), each with ``"block"``, the number of its text block counted from 0; still three waits.
    ``chars=True``: every dict keeps those keys and gains ``"char_quads"`` (one 4x2 list per character of ``"text"``: where it
    sits on the page), ``"char_log_probs"`` (the recogniser's log-prob of each), ``"word_chars"`` (parallel to ``"words"``: the ``[first, end]``
    of each word in ``"text"``) and ``"word_texts"`` (``text[first:end]``); still three waits.  ``beam_width``: as in
    ``read_lines``; ``lm``: as in ``read_lines``.  ``tile``, ``overlap``, ``tile_batch``: detect in overlapping
    tiles, as ``detect_words`` describes; still three waits."""
    _check_lm_args("ocr_lines", beam_width, lm)
    det = detect_words(det_model, page_u8, size, threshold, expand, tile, overlap, tile_batch)
    if det["n"] == 0:
        return []
    return read_lines(rec_model, page_u8, det["quads"], output_height, max_batch, width_unit, alphabet, max_gap, min_cos, reading_order, block_gap, chars,
                      beam_width, lm)


# ------------------------------------------------------------------ page batches ---------------------------------------------------------
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


def pack_pages(pages):
    """A list of (1,H_p,W_p) uint8 device pages -> ``(pages_packed, page_offs, page_sizes)``: the pages back to back in one uint8 buffer
    (one device-to-device copy each), their byte offsets (B,) int64 and their ``(h, w)`` (B,2) int32 on the device -- the layout of the page
    stores of ``datasets.py``.  No synchronisation."""
    pages = _check_pages(pages, "pack_pages")
    if not pages:
        raise RuntimeError("pack_pages: expected at least one page")
    dev = pages[0].device
    sizes = [(int(p.shape[1]), int(p.shape[2])) for p in pages]
    offs, off = [], 0
    for h, w in sizes:
        offs.append(off)
        off += h * w
    packed = torch.empty(off, dtype=torch.uint8, device=dev)
    for p, o, (h, w) in zip(pages, offs, sizes):
        packed[o:o + h * w].view(1, h, w).copy_(p)
    return packed, _to_device_async(offs, torch.int64, dev), _to_device_async(sizes, torch.int32, dev)


def binarize_resize_pages(probs: torch.Tensor, page_sizes: torch.Tensor, canvas, threshold: float = 0.5) -> torch.Tensor:
    """(B,h,w) fp32 probabilities and (B,2) int32 device page sizes ``(H_p, W_p)`` -> the uint8 canvas (B,Hmax,Wmax), ``canvas = (Hmax, Wmax)``
    at least as large as every page: ``binarize_resize(probs[p], (H_p, W_p))`` in the top left corner of plane p and 0 elsewhere, in one
    launch that writes the padding too."""
    _need_cuda(probs, "binarize_resize_pages")
    _need_cuda(page_sizes, "binarize_resize_pages")
    if probs.dtype != torch.float32 or probs.dim() != 3:
        raise RuntimeError("binarize_resize_pages: expected (B,h,w) float32 probabilities")
    B, h, w = probs.shape
    if page_sizes.dtype != torch.int32 or tuple(page_sizes.shape) != (B, 2):
        raise RuntimeError("binarize_resize_pages: page_sizes must be (B,2) int32 on the device")
    Hmax, Wmax = int(canvas[0]), int(canvas[1])
    out = torch.empty(B, Hmax, Wmax, dtype=torch.uint8, device=probs.device)
    lib().binarize_resize_pages(ptr(probs.contiguous()), ptr(page_sizes.contiguous()), ptr(out), B, h, w, Hmax, Wmax, float(threshold))
    return out


def gather_page_quads(quads: torch.Tensor, counts: torch.Tensor):
    """Quads (B,cap,4,2) fp32 with device counts (B,) int32, as ``ocrs_cc_quads`` writes them -> ``(flat quads (N_total,4,2), page_of_word
    (N_total,) int32, word_offs (B+1,) int32, counts as a host list)``: the rows of every page back to back in their own (raster) order.
    Reading ``word_offs`` to size the flat rows is the one host synchronisation; it stands for the B waits for component counts."""
    q = _need_quads(quads, "gather_page_quads", "(B,cap,4,2)")
    B, cap = q.shape[:2]
    counts = _need_counts(counts, "gather_page_quads", B)
    L = lib()
    word_offs = torch.empty(B + 1, dtype=torch.int32, device=q.device)
    L.gather_page_quads(ptr(q), ptr(counts), B, cap, None, None, ptr(word_offs), 0)
    offs_h = _to_host_async(word_offs)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(q.device))
    done.synchronize()  # (waits for the copy only, not for whatever else the stream holds)
    offs = offs_h.tolist()
    n = offs[B]
    flat = torch.empty(n, 4, 2, dtype=torch.float32, device=q.device)
    page_of_word = torch.empty(n, dtype=torch.int32, device=q.device)
    if n:
        L.gather_page_quads(ptr(q), ptr(counts), B, cap, ptr(flat), ptr(page_of_word), ptr(word_offs), n)
    return flat, page_of_word, word_offs, [b - a for a, b in zip(offs, offs[1:])]


def _cc_quads_pages_sizes(B: int, H: int, W: int):
    L = lib()
    ws_bytes, cap = L.cc_quads_ws_bytes(B, H, W), L.cc_quads_capacity(H, W)
    if ws_bytes <= 0 or B > 65535 or B * cap >= 2 ** 31:
        raise ValueError(f"a batch of {B} masks of {H}x{W} is not supported")
    return ws_bytes, cap


def cc_quads_pages(text_masks: torch.Tensor):
    """``extract_cc_quads_device`` for the (B,Hmax,Wmax) uint8 canvas of ``binarize_resize_pages``: ``ocrs_cc_quads`` on the whole canvas, then
    ``gather_page_quads`` -> ``(quads (N_total,4,2), page_of_word, word_offs, counts)``.  The padding is background, so page p's rows are the
    quads of its own mask in their own order.  One host synchronisation."""
    _need_cuda(text_masks, "cc_quads_pages")
    if text_masks.dtype != torch.uint8 or text_masks.dim() != 3:
        raise RuntimeError("cc_quads_pages: expected a (B,Hmax,Wmax) uint8 canvas")
    B, H, W = text_masks.shape
    ws_bytes, cap = _cc_quads_pages_sizes(B, H, W)
    m = text_masks.contiguous()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=m.device)
    ncomp = torch.empty(B, dtype=torch.int32, device=m.device)
    raw = torch.empty(B, cap, 4, 2, dtype=torch.float32, device=m.device)
    lib().cc_quads(ptr(m), 1, 0.5, B, H, W, ptr(ncomp), ptr(raw), None, ptr(ws))
    return gather_page_quads(raw, ncomp)


# ------------------------------------------------------------------ tiled detection ------------------------------------------------------
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


_tile_images = tile_batch  # (the drivers below take a keyword of this name: the size of the forward chunks)


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
    imgs = _tile_images(*store, tables.tiles, tables.max_th, size)
    with torch.inference_mode():
        parts = [model(imgs[a:a + chunk])[:, 0] for a in range(0, imgs.shape[0], chunk)]
        probs = parts[0] if len(parts) == 1 else torch.cat(parts)
    return probs, binarize_resize_tiles(probs, tables, canvas, threshold), tables


def detect_words_batch(model, pages, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE, tile=None, overlap=None,
                       tile_batch: int = 16, _store=None) -> dict:
    """``detect_words`` for a list of (1,H_p,W_p) uint8 device pages of any sizes: one eval forward of the (B,1,h,w) batch of
    ``resize(transform_image(page), size)``, the masks of all pages in one zero-padded canvas, ``ocrs_cc_quads`` on the canvas, the quads
    compacted and expanded.  -> ``probs`` (B,h,w), ``text_masks`` (B,Hmax,Wmax) uint8, ``quads`` (N_total,4,2) grouped by page in raster order,
    ``page_of_word`` (N_total,) int32, ``word_offs`` (B+1,) int32 and ``counts``, the words per page as a host list.  One host synchronisation
    (the word offsets).  A canvas ``ocrs_cc_quads`` cannot take raises ValueError, as ``extract_cc_quads_device`` does.
    ``tile``: detect every page in overlapping tiles of that many page pixels, as ``detect_words`` describes; the tiles of all
    pages are cut in one call and pooled into the forward chunks; ``probs`` becomes (T,h,w) and the dict gains ``tiles`` (T,5) int32 and
    ``tile_offs`` (B+1,) int32 (page p's tiles are ``tile_offs[p]:tile_offs[p + 1]``).  None, the default, is the path above unchanged; the
    same one synchronisation either way."""
    pages = _check_pages(pages, "detect_words_batch")
    if not pages:
        raise RuntimeError("detect_words_batch: expected at least one page")
    if model.training:
        raise RuntimeError("detect_words_batch: the model must be in eval mode (model.eval())")
    _check_tile_args("detect_words_batch", tile, tile_batch)
    dev = pages[0].device
    sizes = [(int(p.shape[1]), int(p.shape[2])) for p in pages]
    canvas = (max(h for h, _ in sizes), max(w for _, w in sizes))
    _cc_quads_pages_sizes(len(pages), *canvas)  # (refuses the batch before anything is launched)
    extra = {}
    if tile is None:
        img = torch.stack([resize(transform_image(p), size) for p in pages])
        with torch.inference_mode():
            probs = model(img)[:, 0]
        text_masks = binarize_resize_pages(probs, _to_device_async(sizes, torch.int32, dev), canvas, threshold)
    else:
        store = pack_pages(pages) if _store is None else _store
        probs, text_masks, tables = _detect_tiles(model, store, sizes, canvas, size, threshold, tile, overlap, tile_batch, "detect_words_batch")
        extra = {"tiles": tables.tiles, "tile_offs": tables.tile_offs}
    flat, page_of_word, word_offs, counts = cc_quads_pages(text_masks)
    quads = expand_quads(flat, expand) if flat.shape[0] else flat
    return {"probs": probs, "text_masks": text_masks, "quads": quads, "page_of_word": page_of_word, "word_offs": word_offs, "counts": counts, **extra}


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


def rectify_crops_pages(pages_packed: torch.Tensor, page_offs: torch.Tensor, page_sizes: torch.Tensor, quads: torch.Tensor, page_of_quad: torch.Tensor,
                        plan: CropPlan) -> torch.Tensor:
    """``rectify_crops`` from a page store (``pack_pages``): crop i is cut out of page ``page_of_quad[i]`` -- ``page_of_line`` for line crops,
    ``page_of_word`` for word crops.  One launch for the crops of all pages; a crop's values are those ``rectify_crops`` gives it on its own page."""
    for t in (pages_packed, page_offs, page_sizes, page_of_quad):
        _need_cuda(t, "rectify_crops_pages")
    if pages_packed.dtype != torch.uint8 or pages_packed.dim() != 1:
        raise RuntimeError("rectify_crops_pages: expected the flat uint8 buffer of pack_pages")
    B = page_offs.numel()
    if page_offs.dtype != torch.int64 or page_sizes.dtype != torch.int32 or tuple(page_sizes.shape) != (B, 2):
        raise RuntimeError("rectify_crops_pages: page_offs must be (B,) int64 and page_sizes (B,2) int32")
    q = _need_quads(quads, "rectify_crops_pages", plan=plan)
    if page_of_quad.dtype != torch.int32 or tuple(page_of_quad.shape) != (q.shape[0],):
        raise RuntimeError("rectify_crops_pages: page_of_quad must be (N,) int32")
    _, packed_floats, _, tiles = plan.host()[:4]
    packed = torch.empty(packed_floats, dtype=torch.float32, device=q.device)
    lib().rectify_crops_pages(ptr(pages_packed.contiguous()), pages_packed.numel(), ptr(page_offs.contiguous()), ptr(page_sizes.contiguous()), B, ptr(q),
                              ptr(page_of_quad.contiguous()), ptr(plan.table), ptr(plan.totals), tiles, ptr(packed), packed_floats)
    return packed


def split_by_page(items: list, offs: list) -> list[list]:
    """flat results grouped by page -> one list per page: ``items[offs[p]:offs[p + 1]]`` (``offs``: B + 1 ascending host offsets)"""
    if any(b < a for a, b in zip(offs, offs[1:])) or (offs and (offs[0] != 0 or offs[-1] != len(items))):
        raise RuntimeError("split_by_page: the offsets must ascend from 0 to the number of items")
    return [items[a:b] for a, b in zip(offs, offs[1:])]


def ocr_pages(det_model, rec_model, pages, lines: bool = True, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE,
              output_height: int = 64, max_batch: int = 256, width_unit: int = 64, alphabet=DEFAULT_ALPHABET, max_gap: float = 2.0,
              min_cos: float = 0.9, reading_order: bool = False, block_gap: float = 1.0, chars: bool = False,
              beam_width: int | None = None, lm: LMGain | None = None, tile=None, overlap=None, tile_batch: int = 16) -> list[list[dict]]:
    """A list of (1,H_p,W_p) uint8 device pages of any sizes -> one result list per page, in page order: what ``ocr_lines`` returns for a page
    (``lines=True``: ``quad``, ``text``, ``words`` in chain order, lines in line order) or what ``ocr_page`` returns (``lines=False``: ``quad``,
    ``text`` in raster order).  One detection forward; the crops of ALL pages go through one plan and one set of width-sorted chunks, so a
    crop's chunk, and with it the padded width the recogniser sees, depends on the whole batch.  Three host synchronisations
    for the batch: the word offsets, the plan's totals (the line count and ``line_page_offs`` travel with them) and the labels.  A page
    without words yields ``[]``; a batch without words returns without launching the recogniser; ``pages == []`` launches nothing.
    ``reading_order=True`` (with ``lines``): every page's list in reading order with ``"block"``, as ``ocr_lines`` returns it; the same waits.
    ``chars=True``: the character keys of ``ocr_lines`` / ``ocr_page`` in every dict; the same waits.
    ``beam_width``: decode by CTC prefix beam search with that many prefixes instead of greedily; every dict gains
    ``"log_prob"``, the log-mass of its text; None = the greedy decode, unchanged; the same waits.
    ``lm`` (with ``beam_width``): the ``LMGain`` of a character language model (``text.CharLM.gain``); the beam ranks by
    log-prob + gains and every dict also gains ``"lm_score"``, the gains of its text; None = the plain beam, unchanged; the same waits.
    ``tile``, ``overlap``, ``tile_batch``: detect every page in overlapping tiles, as ``detect_words`` describes; the tiles of all
    pages are pooled into the same forward chunks and cut from the page store the crops are cut from; the same waits."""
    _check_lm_args("ocr_pages", beam_width, lm)
    pages = _check_pages(pages, "ocr_pages")
    if not pages:
        return []
    B = len(pages)
    store = None if tile is None else pack_pages(pages)
    det = detect_words_batch(det_model, pages, size, threshold, expand, tile, overlap, tile_batch, store)
    words = det["quads"]
    if words.shape[0] == 0:
        return [[] for _ in range(B)]
    packed_pages, page_offs, page_sizes = pack_pages(pages) if store is None else store
    word_offs_h = [0]
    for c in det["counts"]:
        word_offs_h.append(word_offs_h[-1] + c)
    if lines:
        tl = find_lines_pages(words, det["page_of_word"], det["word_offs"], max_gap, min_cos)
        order = _order_lines(tl, block_gap) if reading_order else None
        plan = crop_plan(tl.quads, output_height, tl.n_lines)
        lpo_h = _to_host_async(tl.line_page_offs)  # queued ahead of the plan's totals: it has arrived when they have
        packed = rectify_crops_pages(packed_pages, page_offs, page_sizes, tl.quads, tl.page_of_line, plan)
    else:
        plan = crop_plan(words, output_height)
        packed = rectify_crops_pages(packed_pages, page_offs, page_sizes, words, det["page_of_word"], plan)
    batches = crops_to_batches(packed, plan, max_batch, width_unit)
    if not lines:
        return split_by_page(_read_crops(rec_model, batches, alphabet, words, chars_plan=plan if chars else None, beam_width=beam_width, lm=lm),
                             word_offs_h)
    n_lines, lpo = plan.host()[0], lpo_h.tolist()
    return split_by_page(_read_crops(rec_model, batches, alphabet, words, tl, n_lines, order, lpo, plan if chars else None, beam_width, lm), lpo)

"""Decode: the recogniser over the crop batches, the characters' spans, boxes and word ranges, and the one reader that brings a decode to
the host as a ``Decoded`` record."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from ..text import (DEFAULT_ALPHABET, LMGain, _check_beam_width, _check_lm, beam_decode_spans_async, decode_text, greedy_decode_batch_async,
                    greedy_decode_spans_async, span_arrays, span_lengths, span_views)
from .args import _need_quads, _to_host_async
from .crops import CropPlan
from .lines import TextLines


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


def _spans_to_host(spans: CharSpans, alphabet, boxes: CharBoxes | None = None, ranges: torch.Tensor | None = None):
    """The one reader of a span decode, in the rows' (width-sorted) order: ``(texts, log-probs, language-model scores, chars, ranges)`` as
    host lists, each None where the decode or the caller has nothing for it (``spans.scores``, ``spans.lm_scores``, ``boxes``, ``ranges``);
    ``chars[p] = {"char_quads": [4x2 lists], "char_log_probs": [floats]}``.  Every copy is queued on the current stream, then ONE event is
    recorded and waited for."""
    alphabet = list(alphabet)
    sp_h = _to_host_async(spans.buf)
    cq_h, rg_h, sc_h, lm_h = (None if t is None else _to_host_async(t)
                              for t in (None if boxes is None else boxes.quads, ranges, spans.scores, spans.lm_scores))
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(spans.buf.device))
    done.synchronize()
    labels, _, _, peak, lens = span_views(sp_h, *spans.labels.shape)
    lens = span_lengths(lens)
    texts = [decode_text(labels[p, :n], alphabet) for p, n in enumerate(lens)]
    chars = None if cq_h is None else [{"char_quads": cq_h[p, :n].tolist(), "char_log_probs": peak[p, :n].tolist()} for p, n in enumerate(lens)]
    return (texts, *(None if h is None else h.tolist() for h in (sc_h, lm_h)), chars, None if rg_h is None else rg_h.tolist())


def chars_to_host(spans: CharSpans, boxes: CharBoxes, alphabet=DEFAULT_ALPHABET, ranges: torch.Tensor | None = None):
    """The characters on the host, in the rows' (width-sorted) order: ``(texts, chars, ranges)`` with ``chars[p] = {"char_quads": [4x2 lists],
    "char_log_probs": [floats]}``, one entry per character of ``texts[p]``, and ``ranges`` the (N,2) result of ``word_chars`` as a list (None
    without it).  Spans of a beam decode (``spans.scores``) add ``"log_prob"`` to every ``chars[p]``, those of one with a language model
    (``spans.lm_scores``) ``"lm_score"`` too.  The copies are queued on the current
    stream and there is ONE wait for all of them."""
    texts, scores, lm_scores, chars, ranges = _spans_to_host(spans, alphabet, boxes, ranges)
    for key, values in (("log_prob", scores), ("lm_score", lm_scores)):
        if values is not None:  # a beam decode: the labelling's log-mass (and gains) travel with the characters
            for d, v in zip(chars, values):
                d[key] = v
    return texts, chars, ranges


@dataclass
class Decoded:
    """What the recogniser returned for the crops of one call, on the host and in QUAD order (the batches' permutation is already applied):
    ``texts``; ``log_probs`` and ``lm_scores`` of the texts (beam decodes / beam decodes with a language model; None otherwise); ``chars``, per
    crop ``{"char_quads", "char_log_probs"}`` (None unless the crops' geometry was given); ``word_ranges``, the result of ``word_chars`` by flat
    word index (None unless that geometry had lines); ``spans``, the device ``CharSpans`` (None for the greedy decode without characters)."""
    texts: list
    log_probs: list | None = None
    lm_scores: list | None = None
    chars: list | None = None
    word_ranges: list | None = None
    spans: CharSpans | None = None

    @classmethod
    def in_quad_order(cls, perm: list, texts: list, log_probs=None, lm_scores=None, chars=None, word_ranges=None, spans=None) -> Decoded:
        """the record of per-crop lists in the batches' width-sorted order: ``sorted[perm[i]]`` is quad i's (``word_ranges`` and ``spans``
        are not per crop and stay as they are)"""
        return cls(*(None if rows is None else [rows[p] for p in perm] for rows in (texts, log_probs, lm_scores, chars)), word_ranges, spans)


def _decode_crops(rec_model, batches, alphabet=DEFAULT_ALPHABET, chars: bool = False, beam_width: int | None = None, lm: LMGain | None = None,
                  geometry=None) -> Decoded:
    """The recogniser over ``batches`` (what ``crops_to_batches`` returned) -> the ``Decoded`` record every public form is a view of; the one
    place the batches' permutation is applied.  Greedy without characters: every chunk's forward and ``greedy_decode_batch_async`` are queued
    (the decodes on their side stream), then the label copies are waited for.  Anything else: ``decode_crop_spans`` and ONE wait, in
    ``_spans_to_host``.  ``geometry`` = ``(boxes_of, ranges_of)``, the character stages of what the crops were cut with:
    ``boxes_of(spans)`` (``char_boxes`` or ``char_boxes_chain`` on that geometry) and, for lines, ``ranges_of(spans, boxes, alphabet)``
    (``word_chars`` / ``word_chars_chain``; None for word crops) are queued behind the decodes and copied in the same wait."""
    _check_lm_args("recognize_crops", beam_width, lm)
    perm = batches[2]
    if not chars and beam_width is None:
        _check_batches(rec_model, batches, "recognize_crops")
        alphabet = list(alphabet)
        with torch.inference_mode():
            handles = [greedy_decode_batch_async(rec_model(img), iw.div(4, rounding_mode="floor")) for img, iw in zip(*batches[:2])]
        texts = [decode_text(row, alphabet) for h in handles for row in h.result()]
        return Decoded.in_quad_order(perm, texts)
    spans = decode_crop_spans(rec_model, batches, beam_width, lm)
    boxes = ranges = None
    if geometry is not None:
        boxes_of, ranges_of = geometry
        boxes = boxes_of(spans)
        ranges = None if ranges_of is None else ranges_of(spans, boxes, alphabet)
    return Decoded.in_quad_order(perm, *_spans_to_host(spans, alphabet, boxes, ranges), spans)


def recognize_crops(rec_model, batches, alphabet=DEFAULT_ALPHABET, chars: bool = False, beam_width: int | None = None, lm: LMGain | None = None):
    """Eval forward of the recogniser per batch with ``input_lengths = image_width // 4`` (as ``train_rec.test``) and the device greedy
    decode.  ``batches`` is what ``crops_to_batches`` returned: ``(batch tensors, image widths, perm)``.  Returns the strings in quad order.
    Every chunk's forward and decode are queued before the first label copy is waited for.  ``chars=True``: ``(strings in quad order,
    CharSpans)`` -- the same strings from the decode that keeps every character's time steps and log-prob (``decode_crop_spans``), whose
    device arrays ``char_boxes`` and ``word_chars`` take; one wait, for the one copy of the span buffer.  ``beam_width``: the
    strings of prefix beam search instead -- ``(strings, log-probs of the strings)``, with ``chars=True`` ``(strings, CharSpans, log-probs)``;
    both forms decode into one span buffer and wait once.  ``lm`` (with ``beam_width``): the beam ranks by log-prob + the
    language model's gains, and the gains of the strings are appended to either tuple; the same one wait."""
    rec = _decode_crops(rec_model, batches, alphabet, chars, beam_width, lm)
    extras = [v for v in (rec.spans if chars else None, rec.log_probs, rec.lm_scores) if v is not None]
    return (rec.texts, *extras) if extras else rec.texts

"""Drivers: detection, the line stage and the shared tail (plan, cut, batch, read) composed into ``ocr_page``, ``ocr_lines`` and ``ocr_pages``.
Their keywords ``reading_order``, ``lines`` and ``tile_batch`` carry the names of stage functions, so the stages are called through their
modules here."""
from __future__ import annotations

from functools import partial
from itertools import accumulate

import torch

from ..text import DEFAULT_ALPHABET, LMGain
from . import chain, crops, decode, detect, directions as dirs, orient
from . import lines as line_stage
from .args import _check_pages, _to_host_async
from .assemble import assemble_results


def _read_crops(rec_model, batches, alphabet, words: torch.Tensor, lines: line_stage.TextLines | None = None, n_lines: int = 0,
                order: line_stage.ReadingOrder | None = None, line_page_offs: list | None = None, chars_plan: crops.CropPlan | None = None,
                beam_width: int | None = None, lm: LMGain | None = None, spines: chain.LineSpines | None = None) -> list[dict]:
    """The tail of ``ocr_page``, ``read_lines`` and ``ocr_pages``: the device half -- the early host copies, then ``decode._decode_crops`` on
    ``batches`` -- and ``assemble_results`` on what arrived: the flat result list -- one ``{"quad", "text"}`` per word, or with ``lines``
    one ``{"quad", "text", "words"}`` per line for its first ``n_lines`` lines.  With ``order`` the list is in reading order -- position k holds line ``order.line_order[k]`` -- and every dict has ``"block"``, counted from 0 on every
    page (``line_page_offs``: the host offsets of the pages' lines; None: one page).  The word quads, the line tables and the reading order
    travel to the host ahead of the recogniser on the same stream: they have arrived when the labels have (no wait of their own).
    ``chars_plan`` (the plan the crops were cut with; ``chars=True`` of the callers): every dict also has ``"char_quads"`` and
    ``"char_log_probs"``, line dicts ``"word_chars"`` and ``"word_texts"`` too.  The boxes and word ranges are queued behind the
    decodes and copied with the labels: still one wait here.  ``beam_width``: the texts of prefix beam search and
    ``"log_prob"`` in every dict; still one wait.  ``lm``: the beam's ranking includes the language model's gains and
    every dict has ``"lm_score"`` next to ``"log_prob"``; its copy joins the same wait.  ``spines`` (with ``lines``): the
    crops are chain crops cut along these spines; every line dict gains ``"spine"`` and ``"height"``, whose tables travel with the line
    tables, and the characters' boxes and word ranges follow the spines (``char_boxes_chain`` / ``word_chars_chain``); the same waits."""
    words_h = _to_host_async(words)
    if lines is not None:
        lq_h, wo_h, offs_h = (_to_host_async(t) for t in (lines.quads, lines.word_order, lines.line_offsets))
    if spines is not None:
        kn_h, dims_h = _to_host_async(spines.knots()), _to_host_async(spines.line_dims)
    if order is not None:
        ro_h, nb_h = _to_host_async(order.line_order), _to_host_async(order.new_block)
    geometry = None
    if chars_plan is not None and spines is not None:
        geometry = (partial(chain.char_boxes_chain, spines, chars_plan), partial(chain.word_chars_chain, spines, chars_plan))
    elif chars_plan is not None:
        geometry = (partial(decode.char_boxes, words if lines is None else lines.quads, chars_plan),
                    None if lines is None else partial(decode.word_chars, lines, chars_plan))
    rec = decode._decode_crops(rec_model, batches, alphabet, chars_plan is not None, beam_width, lm, geometry)
    if lines is None:
        return assemble_results(rec, words_h.tolist())
    reading = None
    if order is not None:
        reading = (ro_h[:n_lines].tolist(), nb_h[:n_lines].tolist(), [0, n_lines] if line_page_offs is None else line_page_offs)
    offs = offs_h[:n_lines + 1].tolist()
    knots = None if spines is None else (kn_h[:offs[-1]].tolist(), dims_h[:n_lines].tolist())
    return assemble_results(rec, words_h.tolist(), (lq_h[:n_lines].tolist(), wo_h.tolist(), offs), reading, knots)


def _check_rectify(who: str, rectify, lines: bool = True):
    """``rectify`` names how line crops are cut: "quad" (the line quad's rectangle) or "chain" (along the words' spine)"""
    if rectify not in ("quad", "chain"):
        raise RuntimeError(f'{who}: rectify must be "quad" or "chain"')
    if rectify == "chain" and not lines:
        raise RuntimeError(f'{who}: rectify="chain" cuts line crops: it needs lines=True')


def _check_upright_turns(who: str, orientation):
    """``orientation`` of ``read_words`` / ``read_lines``: None or the int the caller turned the page by (there is no detector here to probe with)"""
    if orientation is not None:
        orient._check_turns(who, orientation)


def _turned_back(results: list, upright_u8: torch.Tensor, orientation) -> list:
    """results read on the upright page -> on the page it was turned from by ``orientation`` quarter turns (None: as they are)"""
    if orientation is None:
        return results
    H, W = orient.turn_shape(int(upright_u8.shape[-2]), int(upright_u8.shape[-1]), orientation)
    return orient.turn_results(results, orientation, H, W)


def _crop_stages(rectify: str, words: torch.Tensor, lines, output_height: int, cut_quads, cut_chain):
    """How the crops of ``words`` -- or, with ``lines`` (a ``TextLines``), of its lines -- are planned and cut -> ``(plan_of, cut, spines)``
    for ``_read_quads``.  "quad": ``crop_plan`` of the quads and ``cut_quads(quads, plan)`` (one page: ``rectify_crops``; a page store:
    ``rectify_crops_pages``).  "chain" (lines only): ``line_spines``, then ``crop_plan_chain`` and ``cut_chain(spines, plan)``
    (``rectify_chain`` / ``rectify_chain_pages``)."""
    if rectify == "chain":
        spines = chain.line_spines(lines)
        return partial(chain.crop_plan_chain, spines, output_height), partial(cut_chain, spines), spines
    quads, count = (words, None) if lines is None else (lines.quads, lines.n_lines)
    return partial(crops.crop_plan, quads, output_height, count), partial(cut_quads, quads), None


def _read_quads(rec_model, plan_of, cut, spines, words: torch.Tensor, lines, order, max_batch: int, width_unit: int, alphabet, chars: bool, beam_width, lm,
                before_read=None):
    """The tail after detection, once: plan the crops (``plan_of()``), cut them (``cut(plan)``), batch them, read them (``_read_crops``);
    the three first arguments are what ``_crop_stages`` returned.
    -> ``(flat result list, line_page_offs as a host list or None)``: the lines' page offsets are copied ahead of the plan's totals, so they
    have arrived when those have.  Two host synchronisations: the plan's totals and the labels.  ``before_read(plan, batches) -> batches``
    (``directions="mixed"``): device work on the batches between the batching and the read; what it copies to the host is queued ahead of
    the read on the same stream, so it has arrived when the labels have."""
    plan = plan_of()
    lpo_h = None if lines is None or lines.line_page_offs is None else _to_host_async(lines.line_page_offs)
    batches = crops.crops_to_batches(cut(plan), plan, max_batch, width_unit)
    lpo = None if lpo_h is None else lpo_h.tolist()
    if before_read is not None:
        batches = before_read(plan, batches)
    return _read_crops(rec_model, batches, alphabet, words, lines, plan.host()[0], order, lpo, plan if chars else None, beam_width, lm, spines), lpo


def read_words(rec_model, page_u8: torch.Tensor, quads: torch.Tensor, output_height: int = 64, max_batch: int = 256, width_unit: int = 64,
               alphabet=DEFAULT_ALPHABET, chars: bool = False, beam_width: int | None = None, lm: LMGain | None = None, orientation: int | None = None) -> list[dict]:
    """The half of ``ocr_page`` after detection, the word counterpart of ``read_lines``: word quads (N,4,2), N > 0, on the device -> the list
    ``ocr_page`` returns, one crop and one dict per word.  Two host synchronisations: the plan's totals and the labels.  ``chars``,
    ``beam_width`` and ``lm`` as ``ocr_page`` describes them.  ``orientation``: ``page_u8`` and ``quads`` are always the
    UPRIGHT page's; an int k says that this page is ``turn_page(original, k)``, and the results come back on the original page with
    ``"turns": k`` (``turn_results``); None, the default, changes nothing; the same waits."""
    decode._check_lm_args("read_words", beam_width, lm)
    _check_upright_turns("read_words", orientation)
    stages = _crop_stages("quad", quads, None, output_height, partial(crops.rectify_crops, page_u8), None)
    return _turned_back(_read_quads(rec_model, *stages, quads, None, None, max_batch, width_unit, alphabet, chars, beam_width, lm)[0], page_u8, orientation)


def ocr_page(det_model, rec_model, page_u8: torch.Tensor, size=detect.MASK_SIZE, threshold: float = 0.5, expand: float = detect.SHRINK_DISTANCE,
             output_height: int = 64, max_batch: int = 256, width_unit: int = 64, alphabet=DEFAULT_ALPHABET, chars: bool = False,
             beam_width: int | None = None, lm: LMGain | None = None, tile=None, overlap=None, tile_batch: int = 16, orientation=None) -> list[dict]:
    """Page (1,H,W) uint8 on the device -> ``[{"quad": (4,2) list, "text": str}, ...]`` in the raster order of ``extract_cc_quads_device``.
    A page without components returns ``[]`` without launching the recogniser.  ``chars=True``: every dict also has ``"char_quads"``, the
    rectangle of every character of ``"text"`` on the page, and ``"char_log_probs"``, the recogniser's log-prob of each; the
    same three waits.
    ``beam_width``: decode by CTC prefix beam search with that many prefixes instead of greedily; every dict gains
    ``"log_prob"``, the log-mass of its text; None = the greedy decode, unchanged; the same waits.
    ``lm`` (with ``beam_width``): the ``LMGain`` of a character language model (``text.CharLM.gain``); the beam ranks by
    log-prob + gains and every dict also gains ``"lm_score"``, the gains of its text; None = the plain beam, unchanged; the same waits.
    ``tile``, ``overlap``, ``tile_batch``: detect in overlapping tiles, as ``detect_words`` describes; the same waits.
    ``orientation``: None, the default, reads the page as it is, unchanged.  An int k in 0..3 -- the quarter turns
    counter-clockwise that make the page upright -- reads ``turn_page(page, k)`` (``size`` is applied to the turned page as given) and maps
    every coordinate of the result back to the page that was passed; every dict gains ``"turns": k``; the same three waits.  ``"auto"`` lets
    ``page_orientation`` decide first (at most three more waits; where it finds 0 its detection is reused, otherwise the turned page is
    detected again, so the result is what the explicit k gives).  Anything else is an argument error."""
    decode._check_lm_args("ocr_page", beam_width, lm)
    det = None
    if orient._check_orientation("ocr_page", orientation) is not None:
        probe = dict(size=size, threshold=threshold, expand=expand, output_height=output_height, max_batch=max_batch, width_unit=width_unit, tile=tile,
                     overlap=overlap, tile_batch=tile_batch)
        page_u8, orientation, det = orient._upright("ocr_page", det_model, rec_model, page_u8, orientation, probe)
    if det is None:
        det = detect.detect_words(det_model, page_u8, size, threshold, expand, tile, overlap, tile_batch)
    if det["n"] == 0:
        return []
    return read_words(rec_model, page_u8, det["quads"], output_height, max_batch, width_unit, alphabet, chars, beam_width, lm, orientation)


def _read_lines_mixed(rec_model, page_u8: torch.Tensor, quads: torch.Tensor, output_height: int, max_batch: int, width_unit: int, alphabet, max_gap: float,
                      min_cos: float, reading_order: bool, block_gap: float, beam_width, lm, rectify: str) -> list[dict]:
    """``read_lines(directions="mixed")``: the page as a batch of two virtual pages -- the upright words on the page, the
    sideways words on ``turn_page(page, 1)`` (``split_by_axis``) -- through ``find_lines_pages``, ``reading_order``, one page store, one plan
    and one set of chunks, as ``ocr_pages`` runs them (``_read_quads``); between the batching and the read the probe of page 1's crops
    (``line_directions``) and the flagged crops turned (``turn_flagged``); then ``mixed_results``.  The flags, the scores and the reading
    order are copied to the host ahead of the final read on the same stream: the two waits of ``read_lines`` (the plan's totals and the
    labels)."""
    orient._check_turn_page(page_u8, "read_lines")
    page = page_u8 if page_u8.dim() == 3 else page_u8[None]  # (the page store takes (1,H,W) pages)
    H, W = (int(v) for v in page.shape[-2:])
    split = dirs.split_by_axis(quads, H, W)
    found = line_stage.find_lines_pages(split.quads, split.page_of_word, split.word_offs, max_gap, min_cos)
    order = line_stage.reading_order(found, block_gap) if reading_order else None
    store = detect.pack_pages([page, orient.turn_page(page, 1)])
    stages = _crop_stages(rectify, split.quads, found, output_height, lambda q, plan: crops.rectify_crops_pages(*store, q, found.page_of_line, plan),
                          lambda sp, plan: chain.rectify_chain_pages(*store, sp, found.page_of_line, plan))
    probed = {}

    def probe_and_turn(plan, batches):
        imgs, image_widths, perm = batches
        n_lines = plan.host()[0]
        probe = found.page_of_line.index_select(0, plan.table[:n_lines, 7].long())  # the page of every crop's line, in the batches' order
        flags, scores = dirs.line_directions(rec_model, imgs, image_widths, probe)
        final = dirs.turn_flagged(imgs, image_widths, flags)
        probed.update(flags=_to_host_async(flags), scores=_to_host_async(scores), perm=perm, n=n_lines,
                      line_at=None if order is None else _to_host_async(order.line_order))
        return final, image_widths, perm

    flat, lpo = _read_quads(rec_model, *stages, split.quads, found, order, max_batch, width_unit, alphabet, False, beam_width, lm, probe_and_turn)
    flags, scores, perm, n_lines = probed["flags"].tolist(), probed["scores"].tolist(), probed["perm"], probed["n"]
    line_at = list(range(n_lines)) if probed["line_at"] is None else probed["line_at"][:n_lines].tolist()
    return dirs.mixed_results(flat, lpo, line_at, [flags[p] for p in perm], [scores[p] for p in perm], H, W)


def read_lines(rec_model, page_u8: torch.Tensor, quads: torch.Tensor, output_height: int = 64, max_batch: int = 256, width_unit: int = 64,
               alphabet=DEFAULT_ALPHABET, max_gap: float = 2.0, min_cos: float = 0.9, reading_order: bool = False, block_gap: float = 1.0,
               chars: bool = False, beam_width: int | None = None, lm: LMGain | None = None, rectify: str = "quad",
               orientation: int | None = None, directions: str | None = None) -> list[dict]:
    """The half of ``ocr_lines`` after detection: word quads (N,4,2), N > 0, on the device -> the list ``ocr_lines`` returns.  Two host
    synchronisations: the plan's totals (which bring the line count) and the labels; the line table and the quads are copied to the host
    ahead of the recogniser on the same stream, so they have arrived when the labels have -- and so has the reading order, which with
    ``reading_order=True`` is queued behind the line stage and changes nothing about the crops (lines are cropped in line order).
    ``chars=True``: the characters' quads, log-probs and word ranges as ``ocr_lines`` describes them, queued behind the decodes; the same waits.
    ``beam_width``: decode by CTC prefix beam search with that many prefixes instead of greedily; every dict gains
    ``"log_prob"``, the log-mass of its text; None = the greedy decode, unchanged; the same waits.
    ``lm`` (with ``beam_width``): the ``LMGain`` of a character language model (``text.CharLM.gain``); the beam ranks by
    log-prob + gains and every dict also gains ``"lm_score"``, the gains of its text; None = the plain beam, unchanged; the same waits.
    ``rectify``: ``"quad"``, the default, cuts every line as the rectangle of its line quad; ``"chain"`` cuts it along the
    polyline of its words at one constant height, so the words of a curved line sit upright and at full height in the crop.  With
    ``"chain"`` every dict keeps ``"quad"`` (still the line quad), ``"text"`` and ``"words"`` and gains ``"spine"`` (the 2n knots of its n
    words as ``[x, y]`` lists: the mid-points of each word's left and right edge, in chain order) and ``"height"`` (the crop's height on the
    page); with ``chars`` the character quads follow the spine; the same waits.  Any other value is an argument error.
    ``orientation``: as in ``read_words`` -- the page and the quads are the upright page's, an int k maps the results back to
    the page that ``turn_page(.., k)`` made it from; the mapped keys are ``"quad"``, ``"words"``, ``"char_quads"`` and ``"spine"``.
    ``directions``: None, the default, is the path above unchanged.  ``"mixed"`` also reads sideways text: the words whose
    long side is steeper than 45 degrees are grouped and read on ``turn_page(page, 1)``, a recogniser probe decides per sideways line which
    way up it reads, and the result is one flat list -- the upright lines, then the sideways ones, each group in its line (or reading)
    order -- on the page that was passed.  Every dict gains ``"direction"`` (the quarter turns counter-clockwise that make the line upright:
    0, or 1 / 3 for a sideways line that reads downwards / upwards) and ``"direction_scores"`` (``[S_plain, S_flip]`` of the probe, None for
    upright lines) in front of ``"block"``; three recogniser forwards instead of one; the same two waits.  With ``chars=True`` it is an
    argument error, and so is any other value.  ``orientation`` composes from outside: the directions are those of the upright page."""
    decode._check_lm_args("read_lines", beam_width, lm)
    _check_rectify("read_lines", rectify)
    _check_upright_turns("read_lines", orientation)
    if dirs._check_directions("read_lines", directions, chars) is not None:
        return _turned_back(_read_lines_mixed(rec_model, page_u8, quads, output_height, max_batch, width_unit, alphabet, max_gap, min_cos, reading_order,
                                              block_gap, beam_width, lm, rectify), page_u8, orientation)
    found = line_stage.find_lines(quads, None, max_gap, min_cos)
    order = line_stage.reading_order(found, block_gap) if reading_order else None
    stages = _crop_stages(rectify, quads, found, output_height, partial(crops.rectify_crops, page_u8), partial(chain.rectify_chain, page_u8))
    return _turned_back(_read_quads(rec_model, *stages, quads, found, order, max_batch, width_unit, alphabet, chars, beam_width, lm)[0], page_u8, orientation)


def ocr_lines(det_model, rec_model, page_u8: torch.Tensor, size=detect.MASK_SIZE, threshold: float = 0.5, expand: float = detect.SHRINK_DISTANCE,
              output_height: int = 64, max_batch: int = 256, width_unit: int = 64, alphabet=DEFAULT_ALPHABET, max_gap: float = 2.0,
              min_cos: float = 0.9, reading_order: bool = False, block_gap: float = 1.0, chars: bool = False,
              beam_width: int | None = None, lm: LMGain | None = None, tile=None, overlap=None, tile_batch: int = 16,
              rectify: str = "quad", orientation=None, directions: str | None = None) -> list[dict]:
    """Page (1,H,W) uint8 on the device -> ``[{"quad": line quad, "text": str, "words": [word quads in chain order]}, ...]`` in line order:
    ``detect_words``, ``find_lines``, then one crop per LINE through the stages ``ocr_page`` runs per word.  The same three host
    synchronisations as ``ocr_page``: the component count, the plan's totals and the labels (``read_lines``).  A page without components
    returns ``[]`` without launching the recogniser.  ``reading_order=True``: the same dicts in reading order (column by column
    where line order interleaves the columns), each with ``"block"``, the number of its text block counted from 0; still three waits.
    ``chars=True``: every dict keeps those keys and gains ``"char_quads"`` (one 4x2 list per character of ``"text"``: where it
    sits on the page), ``"char_log_probs"`` (the recogniser's log-prob of each), ``"word_chars"`` (parallel to ``"words"``: the ``[first, end]``
    of each word in ``"text"``) and ``"word_texts"`` (``text[first:end]``); still three waits.  ``beam_width``: as in
    ``read_lines``; ``lm``: as in ``read_lines``.  ``tile``, ``overlap``, ``tile_batch``: detect in overlapping
    tiles, as ``detect_words`` describes; still three waits.  ``rectify``: ``"quad"`` or ``"chain"``, as in ``read_lines``;
    still three waits.  ``orientation``: None, an int 0..3 or ``"auto"``, as in ``ocr_page``: the page is turned upright, read as
    it always is, and ``"quad"``, ``"words"``, ``"char_quads"`` and ``"spine"`` are mapped back to the page that was passed; every dict gains
    ``"turns"``; still three waits for an int, at most three more (and the second detection's) for ``"auto"``.  ``directions`` (DESIGN.md
    §24): None or ``"mixed"``, as in ``read_lines``: sideways words become lines of their own, read the right way up, every dict gains
    ``"direction"`` and ``"direction_scores"``; still three waits; not with ``chars=True``."""
    decode._check_lm_args("ocr_lines", beam_width, lm)
    _check_rectify("ocr_lines", rectify)
    dirs._check_directions("ocr_lines", directions, chars)
    det = None
    if orient._check_orientation("ocr_lines", orientation) is not None:
        probe = dict(size=size, threshold=threshold, expand=expand, output_height=output_height, max_batch=max_batch, width_unit=width_unit, tile=tile,
                     overlap=overlap, tile_batch=tile_batch)
        page_u8, orientation, det = orient._upright("ocr_lines", det_model, rec_model, page_u8, orientation, probe)
    if det is None:
        det = detect.detect_words(det_model, page_u8, size, threshold, expand, tile, overlap, tile_batch)
    if det["n"] == 0:
        return []
    return read_lines(rec_model, page_u8, det["quads"], output_height, max_batch, width_unit, alphabet, max_gap, min_cos, reading_order, block_gap, chars,
                      beam_width, lm, rectify, orientation, directions)


def ocr_pages(det_model, rec_model, pages, lines: bool = True, size=detect.MASK_SIZE, threshold: float = 0.5, expand: float = detect.SHRINK_DISTANCE,
              output_height: int = 64, max_batch: int = 256, width_unit: int = 64, alphabet=DEFAULT_ALPHABET, max_gap: float = 2.0,
              min_cos: float = 0.9, reading_order: bool = False, block_gap: float = 1.0, chars: bool = False,
              beam_width: int | None = None, lm: LMGain | None = None, tile=None, overlap=None, tile_batch: int = 16,
              rectify: str = "quad", orientation=None) -> list[list[dict]]:
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
    pages are pooled into the same forward chunks and cut from the page store the crops are cut from; the same waits.
    ``rectify`` (with ``lines``): ``"quad"`` or ``"chain"``, as in ``read_lines``; ``"chain"`` with ``lines=False`` is an
    argument error; the same waits.
    ``orientation``: None, an int 0..3 or ``"auto"`` for all pages, or a list with one such entry per page.  Every page is turned
    upright (``turn_page``), the turned pages go through the one batched path above, and each page's results are mapped back to the page
    that was passed, every dict with ``"turns"``.  Ints add no wait; ``"auto"`` probes page by page (``page_orientation``), so ITS waits -- one
    detection's and at most three more -- are per probed page, ahead of the batch's three."""
    decode._check_lm_args("ocr_pages", beam_width, lm)
    _check_rectify("ocr_pages", rectify, lines)
    pages = list(pages)
    orientation = orient._check_orientation("ocr_pages", orientation, len(pages))
    pages = _check_pages(pages, "ocr_pages")
    if not pages:
        return []
    if orientation is not None:
        turns = orientation if isinstance(orientation, list) else [orientation] * len(pages)
        for p in pages:
            orient._check_turn_page(p, "ocr_pages")
        probe = dict(size=size, threshold=threshold, expand=expand, output_height=output_height, max_batch=max_batch, width_unit=width_unit, tile=tile,
                     overlap=overlap, tile_batch=tile_batch)
        turns = [orient.page_orientation(det_model, rec_model, p, **probe)["turns"] if k == "auto" else k for p, k in zip(pages, turns)]
        read = ocr_pages(det_model, rec_model, [orient.turn_page(p, k) for p, k in zip(pages, turns)], lines, size, threshold, expand, output_height, max_batch,
                         width_unit, alphabet, max_gap, min_cos, reading_order, block_gap, chars, beam_width, lm, tile, overlap, tile_batch, rectify)
        return [orient.turn_results(res, k, p.shape[1], p.shape[2]) for res, k, p in zip(read, turns, pages)]
    B = len(pages)
    store = None if tile is None else detect.pack_pages(pages)
    det = detect.detect_words_batch(det_model, pages, size, threshold, expand, tile, overlap, tile_batch, store)
    words = det["quads"]
    if words.shape[0] == 0:
        return [[] for _ in range(B)]
    if store is None:
        store = detect.pack_pages(pages)
    found = order = None
    if lines:
        found = line_stage.find_lines_pages(words, det["page_of_word"], det["word_offs"], max_gap, min_cos)
        order = line_stage.reading_order(found, block_gap) if reading_order else None
    page_of_quad = found.page_of_line if lines else det["page_of_word"]
    stages = _crop_stages(rectify, words, found, output_height, lambda q, plan: crops.rectify_crops_pages(*store, q, page_of_quad, plan),
                          lambda sp, plan: chain.rectify_chain_pages(*store, sp, page_of_quad, plan))
    flat, offs = _read_quads(rec_model, *stages, words, found, order, max_batch, width_unit, alphabet, chars, beam_width, lm)
    return line_stage.split_by_page(flat, offs if lines else [0, *accumulate(det["counts"])])

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

Chain crops (csrc/line_chain.hip, C ABI section "chain crops"; restated for the tests in tests/chain_ref.py).  The line quad is one
rotated rectangle around all words of a line, so a curved line -- page curl, an arc, a sagging end -- is cut far higher than its text and runs
diagonally through its crop.  With ``rectify="chain"`` ``read_lines``, ``ocr_lines`` and ``ocr_pages`` cut every line along the polyline of its words
(``line_spines``: the mid-points of each word's left and right edge, joined across the gaps) at one constant height (``crop_plan_chain``,
``rectify_chain`` / ``rectify_chain_pages``), every word upright and at full height; line dicts gain ``"spine"`` and ``"height"``, and with
``chars=True`` the character quads follow the spine (``char_boxes_chain``, ``word_chars_chain``).  ``"quad"``, the default, is the rectangle path
unchanged; the same waits.

Orientation (csrc/page_orient.hip, C ABI section "orientation"; restated for the tests in tests/orient_ref.py).  Every stage above
assumes an upright page: the line stage never chains steep text, and the crop frame's ``u.x > 0`` hands an upside-down page to the recogniser
upside down.  ``orientation=k`` of ``ocr_page``, ``ocr_lines`` and ``ocr_pages`` -- k quarter turns counter-clockwise make the page upright --
reads ``turn_page(page, k)``, an exact permutation of the page's bytes, and maps ``"quad"``, ``"words"``, ``"char_quads"`` and ``"spine"`` back to the
page that was passed (``turn_results``); every dict gains ``"turns"``; the same three waits.  ``orientation="auto"`` decides first
(``page_orientation``: a vote over the word quads for the axis, ``orientation_votes``, and a recogniser probe of the longest words both ways
up for the sign, ``path_confidence``; at most three more waits).  None, the default, is today's path unchanged.

Mixed directions (csrc/line_dirs.hip, C ABI section "directions"; restated for the tests in tests/directions_ref.py).  ``orientation``
turns the whole page; sideways text on an upright page -- row headers, the label of a y axis, a margin note -- is what ``directions="mixed"`` of
``read_lines`` and ``ocr_lines`` reads: ``split_by_axis`` sends the words whose long side is steeper than 45 degrees to a second, virtual page,
``turn_page(page, 1)``, both pages go through the page-batch path below, ``line_directions`` probes every sideways line both ways up
(``flip_crops``, ``path_confidence``, ``flip_flags``) and ``mixed_results`` maps the sideways lines back; every dict gains ``"direction"`` and
``"direction_scores"``; the same three waits.  None, the default, is today's path unchanged.

Page batches (C ABI section "page batches").  ``ocr_pages`` reads a list of pages of any sizes with ONE detection forward, one
zero-padded mask canvas, one line stage that keeps to each word's own page, one pooled crop plan and one set of width-sorted recognition chunks
for the crops of all pages: three host synchronisations for the whole batch (the word offsets, the plan's totals, the labels) instead of three
per page.  The single-page functions above are what its tests compare it with.

Accuracy (csrc/ocr_eval.hip, C ABI section "end-to-end accuracy"; restated for the tests in tests/eval_ref.py).  ``evaluate_pages``
runs ``ocr_pages`` over annotated pages and says how many words were found and how many were read correctly: ``match_words`` assigns predicted
to annotated words one to one on the device, ``OcrAccuracyStats`` keeps integer counters there across ``update`` calls (no wait) and
``result()`` is the one wait.  It consumes the drivers' results and changes none of them.

The package, by stage: ``evaluate`` (the accuracy above), ``args`` (argument checks, asynchronous copies), ``detect``, ``tiles``, ``crops``, ``lines`` (lines and reading order), ``chain`` (chain crops), ``orient`` (page turns and their detection), ``directions`` (sideways lines on an upright page),
``decode`` (the recogniser, characters, and the ``Decoded`` record every decode is read into), ``assemble`` (record + host lists -> result
dicts, no GPU) and ``drivers`` (``ocr_page``, ``read_words``, ``read_lines``, ``ocr_lines``, ``ocr_pages``).  Everything is re-exported here.
"""
from ..input_pipeline import resize, transform_image  # noqa: F401
from ..text import DEFAULT_ALPHABET, decode_text  # noqa: F401
from .assemble import assemble_results  # noqa: F401
from .chain import LineSpines, char_boxes_chain, crop_plan_chain, line_spines, rectify_chain, rectify_chain_pages, word_chars_chain  # noqa: F401
from .crops import CropPlan, crop_plan, crops_to_batches, plan_chunks, rectify_crops, rectify_crops_pages  # noqa: F401
from .decode import CharBoxes, CharSpans, Decoded, char_boxes, chars_to_host, decode_crop_spans, recognize_crops, space_label, word_chars  # noqa: F401
from .detect import (MASK_SIZE, SHRINK_DISTANCE, _cc_quads_pages_sizes, binarize_resize, binarize_resize_pages, cc_quads_pages, detect_words,  # noqa: F401
                     detect_words_batch, expand_quads, gather_page_quads, pack_pages)
from .directions import AxisSplit, flip_crops, flip_flags, line_directions, mixed_results, split_by_axis, turn_flagged  # noqa: F401
from .drivers import _read_crops, ocr_lines, ocr_page, ocr_pages, read_lines, read_words  # noqa: F401
from .evaluate import Matches, OcrAccuracyStats, evaluate_pages, match_words  # noqa: F401
from .lines import ReadingOrder, TextLines, find_lines, find_lines_pages, page_text, reading_order, split_by_page  # noqa: F401
from .orient import orientation_votes, page_orientation, path_confidence, probe_batches, turn_page, turn_quads, turn_results, turn_shape  # noqa: F401
from .tiles import TILES_AXIS_MAX, AxisPlan, TilePlan, TileTables, binarize_resize_tiles, tile_batch, tile_plan, tile_tables  # noqa: F401

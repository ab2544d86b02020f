"""The reference's evaluation entry point (ocrs_models/eval_detection.py:19-69) on the GPU:

    python -m ocrs_models_amd.eval_detection MODEL IMAGE OUT_BASENAME [--rec-model CKPT] [--lines [--reading-order] [--rectify {quad,chain}]] [--chars] [--beam-width N]
        [--lm FILE [--lm-weight A] [--lm-bonus B]] [--tile TH TW [--tile-overlap VH VW]] [--orientation {auto,0,1,2,3}] [--directions mixed]

loads a detection checkpoint, runs ``inference.detect_words`` on the image and writes the same four files: ``-input.png`` (the page as the
model sees it), ``-text-regions.png`` (the page under the text mask), ``-text-probs.png`` and ``-text-words.png`` (the word quads drawn
on the page).  With ``--rec-model`` the words are recognised too (``inference.read_words``) and printed, one JSON object per line.
With ``--lines`` the words are grouped into text lines first (``inference.find_lines``): ``-text-lines.png`` shows the line quads, and with
``--rec-model`` every LINE is recognised (``inference.read_lines``) and printed as one JSON object with its quad, its text and its words' quads
in reading order, instead of the words.  ``--lines --reading-order`` prints those objects in the page's reading order (column by column,
``inference.reading_order``), each with ``"block"``, the number of its text block.  ``--lines --rectify chain`` cuts every line's crop along the
polyline of its words instead of as the rectangle of its line quad (``read_lines(rectify="chain")``); every line object gains
``"spine"`` and ``"height"``.  ``--chars`` (with ``--rec-model``) adds to every object where each
character of its text sits on the page and the recogniser's log-prob of it (``"char_quads"``, ``"char_log_probs"``), and to every line object the text and
character range of each of its words (``"word_texts"``, ``"word_chars"``): ``inference.char_boxes`` / ``word_chars``.  ``--beam-width N`` (with
``--rec-model``) decodes by CTC prefix beam search with N prefixes instead of greedily and adds ``"log_prob"``, the log-mass of the text, to every
object.  ``--lm FILE`` (with ``--beam-width``) loads a character language model written by ``python -m ocrs_models_amd.char_lm``
and fuses ``A log P + B`` per character into the beam's ranking (``--lm-weight A``, default 1; ``--lm-bonus B``, default 0); every object
gains ``"lm_score"``.  ``--tile TH TW`` detects the page in overlapping tiles of TH x TW page pixels instead of squeezing it to the
model's size whole (``detect_words(tile=...)``; ``--tile-overlap VH VW``, default an eighth of the tile); ``-text-probs.png`` then
shows the tiles' probability maps side by side in their grid.  ``--orientation K`` reads a page scanned sideways or upside down: K
quarter turns counter-clockwise make it upright, ``auto`` (with ``--rec-model``) lets ``inference.page_orientation`` find K.  The page is turned
(``inference.turn_page``), detected and read upright -- the pictures show the upright page -- and the JSON objects come back on the page as it
was given, each with ``"turns"``; the turns are printed to stderr and written to ``-orientation.json`` with the vote and the probe's scores.
``--directions mixed`` (with ``--lines`` and ``--rec-model``) also reads sideways text on the upright page
(``read_lines(directions="mixed")``): the JSON objects gain ``"direction"`` and ``"direction_scores"``.
The image is read and the pictures are written with PIL on the host; that is not a hot path.
"""
from __future__ import annotations

import json
import sys
import time
from argparse import ArgumentParser

import numpy as np
import torch
from PIL import Image, ImageDraw

from . import inference
from .checkpoint import load_model_state
from .models import DetectionModel
from .recognition import RecognitionModel
from .text import DEFAULT_ALPHABET, CharLM


def _to_pil(img: torch.Tensor) -> Image.Image:
    """float (H,W) in [0,1] -> 8-bit greyscale, as torchvision's to_pil_image does (mul(255), truncate)"""
    return Image.fromarray(img.detach().mul(255).to(torch.uint8).cpu().numpy())


def draw_quads(img_u8: np.ndarray, quads) -> Image.Image:
    """postprocess.py:190-211: the quads' outlines in red, two pixels wide, on an RGB copy of the page"""
    out = Image.fromarray(img_u8).convert("RGB")
    draw = ImageDraw.Draw(out)
    for quad in quads:
        verts = [(float(x), float(y)) for x, y in quad]
        for i, start in enumerate(verts):
            draw.line((start, verts[(i + 1) % len(verts)]), fill="red", width=2)
    return out


def _load_rec(path: str, device) -> RecognitionModel:
    rec = RecognitionModel(DEFAULT_ALPHABET).to(device)
    load_model_state(path, rec, device)
    return rec.eval()


def main(argv=None):
    parser = ArgumentParser()
    parser.add_argument("model")
    parser.add_argument("image")
    parser.add_argument("out_basename")
    parser.add_argument("--rec-model", help="recognition checkpoint: also recognise the words and print them as JSON lines")
    parser.add_argument("--lines", action="store_true", help="group the words into text lines: write -text-lines.png and, with --rec-model, "
                        "recognise and print one JSON object per line instead of per word")
    parser.add_argument("--reading-order", action="store_true", help="with --lines and --rec-model: print the lines in reading order, column by "
                        "column, each with the number of its block")
    parser.add_argument("--rectify", choices=("quad", "chain"), default="quad", help="with --lines and --rec-model: cut every line's crop as the rectangle "
                        "of its line quad (quad, the default) or along the polyline of its words (chain); chain adds the spine and its height to "
                        "the JSON objects")
    parser.add_argument("--chars", action="store_true", help="with --rec-model: add every character's quad and log-prob to the JSON objects and, with "
                        "--lines, every word's text and character range")
    parser.add_argument("--beam-width", type=int, default=None, metavar="N", help="with --rec-model: decode by CTC prefix beam search with N prefixes "
                        "(1..64) instead of greedily and add the text's log-prob to the JSON objects")
    parser.add_argument("--lm", metavar="FILE", help="with --beam-width: a character language model (.npz of ocrs_models_amd.char_lm) fused into the "
                        "beam's ranking; adds the text's language-model score to the JSON objects")
    parser.add_argument("--lm-weight", type=float, default=1.0, metavar="A", help="with --lm: the gain per character is A log P + B (default 1)")
    parser.add_argument("--lm-bonus", type=float, default=0.0, metavar="B", help="with --lm: see --lm-weight (default 0)")
    parser.add_argument("--tile", type=int, nargs=2, default=None, metavar=("TH", "TW"), help="detect in overlapping tiles of TH x TW page pixels and "
                        "compose one page mask from them, for pages much larger than the model's 800 x 600")
    parser.add_argument("--tile-overlap", type=int, nargs=2, default=None, metavar=("VH", "VW"), help="with --tile: the overlap of neighbouring tiles "
                        "in page pixels (default: an eighth of the tile)")
    parser.add_argument("--orientation", choices=("auto", "0", "1", "2", "3"), default=None, metavar="K", help="the page is scanned sideways or upside "
                        "down: K in 0..3 quarter turns counter-clockwise make it upright; auto (with --rec-model) finds K from the word quads and "
                        "a recogniser probe.  The JSON objects are on the page as given and gain the turns")
    parser.add_argument("--directions", choices=("mixed",), default=None, help="with --lines and --rec-model: also read sideways text on the upright "
                        "page (row headers, axis labels, margin notes); every JSON object gains the line's direction and the probe's two scores")
    args = parser.parse_args(argv)
    if args.directions is not None and not (args.lines and args.rec_model):
        parser.error("--directions needs --lines and --rec-model (sideways words are grouped into lines and a recogniser probe decides which way up they read)")
    if args.directions is not None and args.chars:
        parser.error("--directions does not go with --chars")
    if args.orientation == "auto" and not args.rec_model:
        parser.error("--orientation auto needs --rec-model (the probe reads the longest words both ways up)")
    if args.reading_order and not args.lines:
        parser.error("--reading-order needs --lines")
    if args.rectify == "chain" and not args.lines:
        parser.error("--rectify chain needs --lines")
    if args.beam_width is not None and not args.rec_model:
        parser.error("--beam-width needs --rec-model")
    if args.beam_width is not None and not 1 <= args.beam_width <= 64:
        parser.error("--beam-width must be in 1..64")
    if args.lm is not None and args.beam_width is None:
        parser.error("--lm needs --beam-width")
    if args.tile_overlap is not None and args.tile is None:
        parser.error("--tile-overlap needs --tile")
    if args.tile is not None and (min(args.tile) < 1 or any(not 0 <= v < t for v, t in zip(args.tile_overlap or (0, 0), args.tile))):
        parser.error("--tile must be at least 1 x 1 and --tile-overlap in 0 .. tile - 1 per axis")

    device = torch.device("cuda:0")
    model = DetectionModel().to(device)
    load_model_state(args.model, model, device)
    model.eval()

    page_h = np.asarray(Image.open(args.image).convert("L"), dtype=np.uint8)
    page = torch.from_numpy(page_h.copy())[None].to(device)
    tile = None if args.tile is None else tuple(args.tile)
    overlap = None if args.tile_overlap is None else tuple(args.tile_overlap)

    rec = turns = det = None
    if args.orientation is not None:
        found = {"turns": int(args.orientation)} if args.orientation != "auto" else None
        if found is None:
            rec = _load_rec(args.rec_model, device)
            found = inference.page_orientation(model, rec, page, tile=tile, overlap=overlap)
            det = found.pop("det") if found["turns"] == 0 else None  # an upright page is detected once
            found.pop("det", None)
        turns = found["turns"]
        print(f"Orientation: {turns} quarter turn(s) counter-clockwise make the page upright", file=sys.stderr)
        with open(f"{args.out_basename}-orientation.json", "w") as f:
            json.dump(found, f)
        page = inference.turn_page(page, turns)  # from here on the upright page; the JSON objects are mapped back at the end
        page_h = np.ascontiguousarray(np.rot90(page_h, turns))

    img = inference.resize(inference.transform_image(page), inference.MASK_SIZE)
    _to_pil((img[0] + 0.5).clamp(0, 1)).save(f"{args.out_basename}-input.png")

    torch.cuda.synchronize()
    start = time.time()
    if det is None:
        det = inference.detect_words(model, page, tile=tile, overlap=overlap)
    torch.cuda.synchronize()
    print(f"Predicted text in {time.time() - start:.2f}s", file=sys.stderr)

    text_regions = page[0].float() / 255.0 * det["text_mask"].float()
    _to_pil(text_regions).save(f"{args.out_basename}-text-regions.png")
    probs = det["probs"]
    if tile is not None:  # (T,h,w) in row-major tile order -> the maps side by side in their grid
        plan = inference.tile_plan(page.shape[1], page.shape[2], tile, overlap)
        ny, nx = len(plan.rows.starts), len(plan.cols.starts)
        probs = probs.view(ny, nx, *probs.shape[-2:]).permute(0, 2, 1, 3).reshape(ny * probs.shape[-2], nx * probs.shape[-1])
    _to_pil(probs).save(f"{args.out_basename}-text-probs.png")
    quads = det["quads"].tolist()
    draw_quads(page_h, quads).save(f"{args.out_basename}-text-words.png")

    if args.rec_model and det["n"] and rec is None:
        rec = _load_rec(args.rec_model, device)
    if not det["n"]:
        rec = None
    lm = None
    if args.lm is not None and rec is not None:
        model_lm = CharLM.load(args.lm)
        if model_lm.alphabet is not None and model_lm.alphabet != DEFAULT_ALPHABET:
            parser.error("--lm: the language model was built for another alphabet")
        lm = model_lm.gain(args.lm_weight, args.lm_bonus, device)
    if args.lines:
        if rec is not None:
            lines = inference.read_lines(rec, page, det["quads"], reading_order=args.reading_order, chars=args.chars, beam_width=args.beam_width, lm=lm,
                                         rectify=args.rectify, directions=args.directions)
            for line in lines if turns is None else inference.turn_results(lines, turns, *inference.turn_shape(*page_h.shape, turns)):
                print(json.dumps(line))
            line_quads = [line["quad"] for line in lines]
        else:
            found = inference.find_lines(det["quads"])
            line_quads = found.quads[:int(found.n_lines)].tolist()
        draw_quads(page_h, line_quads).save(f"{args.out_basename}-text-lines.png")
    elif rec is not None:
        for word in inference.read_words(rec, page, det["quads"], chars=args.chars, beam_width=args.beam_width, lm=lm, orientation=turns):
            print(json.dumps(word))


if __name__ == "__main__":
    main()

"""End-to-end accuracy of page OCR on an annotated dataset (no reference counterpart):

    python -m ocrs_models_amd.eval_ocr hiertext DATA_DIR --det-model CKPT --rec-model CKPT [--train] [--max-images N] [--level {word,line}]
        [--ignore-vertical] [--min-iou X] [--batch-pages N] [--rectify {quad,chain}] [--beam-width N] [--lm FILE [--lm-weight A] [--lm-bonus B]]
        [--tile TH TW [--tile-overlap VH VW]] [--orientation {auto,0,1,2,3}]

reads the split's annotated words (``datasets.hiertext_word_truth``; ``--level line``: ``hiertext_line_truth``) and pages, runs
``inference.evaluate_pages`` -- ``ocr_pages`` in batches of ``--batch-pages``, matched and scored on the device -- and prints ONE JSON line:
the options used and the result dict (detection precision / recall / f1, the end-to-end ones that also ask for the right text, the two
character error rates and the raw counters).  The option flags have the names and meanings of ``eval_detection``'s.  Pages are decoded on the
host (``datasets.read_gray``); that is not a hot path.
"""
from __future__ import annotations

import contextlib
import json
import sys
from argparse import ArgumentParser

import torch

from . import inference
from .checkpoint import load_model_state
from .datasets import decode_pages, hiertext_line_truth, hiertext_word_truth, read_gray
from .models import DetectionModel
from .recognition import RecognitionModel
from .text import DEFAULT_ALPHABET, CharLM


def main(argv=None):
    parser = ArgumentParser()
    parser.add_argument("dataset", choices=("hiertext",))
    parser.add_argument("data_dir")
    parser.add_argument("--det-model", required=True, help="detection checkpoint")
    parser.add_argument("--rec-model", required=True, help="recognition checkpoint")
    parser.add_argument("--train", action="store_true", help="score the training split instead of the validation split")
    parser.add_argument("--max-images", type=int, default=None, metavar="N")
    parser.add_argument("--level", choices=("word", "line"), default="word", help="score words against annotated words (default) or lines against "
                        "annotated lines")
    parser.add_argument("--ignore-vertical", action="store_true", help="treat vertical annotations as \"do not care\" regions")
    parser.add_argument("--min-iou", type=float, default=0.5, metavar="X", help="a pair is a candidate match when IoU > X (default 0.5)")
    parser.add_argument("--batch-pages", type=int, default=8, metavar="N", help="pages per ocr_pages call (default 8)")
    parser.add_argument("--rectify", choices=("quad", "chain"), default="quad", help="cut every line's crop as the rectangle of its line quad (quad, "
                        "the default) or along the polyline of its words (chain)")
    parser.add_argument("--beam-width", type=int, default=None, metavar="N", help="decode by CTC prefix beam search with N prefixes (1..64) instead of "
                        "greedily")
    parser.add_argument("--lm", metavar="FILE", help="with --beam-width: a character language model (.npz of ocrs_models_amd.char_lm) fused into the "
                        "beam's ranking")
    parser.add_argument("--lm-weight", type=float, default=1.0, metavar="A", help="with --lm: the gain per character is A log P + B (default 1)")
    parser.add_argument("--lm-bonus", type=float, default=0.0, metavar="B", help="with --lm: see --lm-weight (default 0)")
    parser.add_argument("--tile", type=int, nargs=2, default=None, metavar=("TH", "TW"), help="detect in overlapping tiles of TH x TW page pixels")
    parser.add_argument("--tile-overlap", type=int, nargs=2, default=None, metavar=("VH", "VW"), help="with --tile: the overlap of neighbouring tiles "
                        "in page pixels (default: an eighth of the tile)")
    parser.add_argument("--orientation", choices=("auto", "0", "1", "2", "3"), default=None, metavar="K", help="the pages are scanned sideways or "
                        "upside down: K in 0..3 quarter turns counter-clockwise make them upright; auto finds K page by page")
    args = parser.parse_args(argv)
    if args.beam_width is not None and not 1 <= args.beam_width <= 64:
        parser.error("--beam-width must be in 1..64")
    if args.lm is not None and args.beam_width is None:
        parser.error("--lm needs --beam-width")
    if args.tile_overlap is not None and args.tile is None:
        parser.error("--tile-overlap needs --tile")
    if args.tile is not None and (min(args.tile) < 1 or any(not 0 <= v < t for v, t in zip(args.tile_overlap or (0, 0), args.tile))):
        parser.error("--tile must be at least 1 x 1 and --tile-overlap in 0 .. tile - 1 per axis")
    if args.batch_pages < 1:
        parser.error("--batch-pages must be at least 1")
    if not torch.cuda.is_available():
        raise RuntimeError("eval_ocr needs a GPU (page OCR and its evaluation have no CPU path)")

    device = torch.device("cuda:0")
    read = hiertext_word_truth if args.level == "word" else hiertext_line_truth
    with contextlib.redirect_stdout(sys.stderr):  # (the JSON-lines conversion reports itself on stdout, which here carries the one result line)
        truth = read(args.data_dir, train=args.train, max_images=args.max_images, ignore_vertical=args.ignore_vertical)
    split = "train" if args.train else "validation"
    pages_h = decode_pages([f"{args.data_dir}/{split}/{t.image_id}.jpg" for t in truth], read_gray)

    det = DetectionModel().to(device)
    load_model_state(args.det_model, det, device)
    det.eval()
    rec = RecognitionModel(DEFAULT_ALPHABET).to(device)
    load_model_state(args.rec_model, rec, device)
    rec.eval()

    options = {"rectify": args.rectify}
    if args.beam_width is not None:
        options["beam_width"] = args.beam_width
    if args.lm is not None:
        model_lm = CharLM.load(args.lm)
        if model_lm.alphabet is not None and model_lm.alphabet != DEFAULT_ALPHABET:
            parser.error("--lm: the language model was built for another alphabet")
        options["lm"] = model_lm.gain(args.lm_weight, args.lm_bonus, device)
    if args.tile is not None:
        options["tile"] = tuple(args.tile)
        if args.tile_overlap is not None:
            options["overlap"] = tuple(args.tile_overlap)
    if args.orientation is not None:
        options["orientation"] = args.orientation if args.orientation == "auto" else int(args.orientation)

    pages = [torch.from_numpy(p)[None].to(device) for p in pages_h]
    result = inference.evaluate_pages(det, rec, pages, truth, level=args.level, batch_pages=args.batch_pages, min_iou=args.min_iou, **options)
    used = {"dataset": args.dataset, "split": split, "images": len(pages), "level": args.level, "ignore_vertical": args.ignore_vertical,
            "min_iou": args.min_iou, "batch_pages": args.batch_pages, "rectify": args.rectify, "beam_width": args.beam_width, "lm": args.lm,
            "lm_weight": args.lm_weight if args.lm else None, "lm_bonus": args.lm_bonus if args.lm else None, "tile": args.tile,
            "tile_overlap": args.tile_overlap, "orientation": args.orientation}
    print(json.dumps({"options": used, **result}))
    return result


if __name__ == "__main__":
    main()

"""What reading sideways text on an upright page costs on the GPU (csrc/line_dirs.hip: inference.split_by_axis, flip_crops, line_directions and
``directions="mixed"``).

    python tools/directions_time.py [--reps 30] [--det-model CKPT --rec-model CKPT --image FILE]

One JSON line each, medians of ``--reps`` runs:

* ``axis_split``: ms of ``ocrs_axis_split`` between stream events at 300 and at 4096 words (random rectangles at any angle).
* ``flip_crops``: ms of ``ocrs_flip_crops`` on a (256,1,64,832) batch (widths 10 .. 832, every crop flagged) between stream events, next to a
  ``torch`` device copy of the same bytes -- the yardstick of a pass that can at best run at copy speed -- and the ratio of the two.
* ``mixed``: on a 2048 x 1536 page of 300 painted bars of which 10 % stand sideways, read with the painted stand-in detector of
  tests/test_lines_gpu.py and the golden recognition weights: wall-clock ms of ``ocr_lines`` plain and with ``directions="mixed"``, and of the
  stages of the mixed call on their own -- the split, the probe (``line_directions``: the turned batches, two forwards, the scores, the flags),
  the flip of the flagged crops and the final read (``_read_crops``: the third forward, the decode, the labels' wait).

With ``--det-model``, ``--rec-model`` (checkpoints of train_detection / train_rec) and ``--image`` the tool prints instead one JSON line per
line of ``ocr_lines(directions="mixed")`` on that image with its direction and both scores: how far S_plain and S_flip lie apart on trained
weights, which nobody has measured.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ocrs_models_amd as oa  # noqa: E402
from ocrs_models_amd import inference as inf  # noqa: E402
from ocrs_models_amd._lib import lib  # noqa: E402


def _event_ms(fn, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def _entry_ms(name, fn, reps):
    """median ms between events around the entry point ``ocrs_<name>`` over ``reps`` calls of ``fn``"""
    L = lib()
    fn()
    L.timing = {name: []}
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    timing, L.timing = L.timing, None
    return statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing[name])


def _wall_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), out


def split_times(dev, reps):
    from tests import lines_ref as LR

    out = {}
    for n in (300, 4096):
        r = np.random.RandomState(n)
        q = np.stack([LR.rotated_rect(r.uniform(0, 1536), r.uniform(0, 2048), r.uniform(5, 300), r.uniform(2, 40), r.uniform(0, 360)) for _ in range(n)])
        q_d = torch.from_numpy(q).to(dev)
        ms = _entry_ms("axis_split", lambda: inf.split_by_axis(q_d, 2048, 1536), reps)
        out[str(n)] = {"ms": round(ms, 4), "sideways": int(inf.split_by_axis(q_d, 2048, 1536).page_of_word.sum())}
    return out


def flip_times(dev, reps):
    batch = torch.randn(256, 1, 64, 832, device=dev)
    widths = torch.linspace(10, 832, 256, device=dev).long()
    dst = torch.empty_like(batch)
    dst.copy_(batch)
    copy_ms = _event_ms(lambda: dst.copy_(batch), reps)
    flip_ms = _entry_ms("flip_crops", lambda: inf.flip_crops(batch, widths, out=dst), reps)
    nbytes = 2 * batch.numel() * 4
    return {"shape": list(batch.shape), "flip_ms": round(flip_ms, 4), "copy_ms": round(copy_ms, 4), "flip_over_copy": round(flip_ms / copy_ms, 3),
            "GBps": {"flip": round(nbytes / (1e6 * flip_ms), 1), "copy": round(nbytes / (1e6 * copy_ms), 1)}}


def painted_page(dev):
    """2048 x 1536, 270 horizontal bars in 30 rows of 9 and 30 vertical bars in 3 columns of 10, each column leaning 2 px to the left per word"""
    from tests import test_lines_gpu as TL

    bars = [(40 + 120 * c, 40 + 64 * r, 100, 24) for r in range(30) for c in range(9)]
    bars += [(1200 + 110 * j - 2 * k, 60 + 130 * k, 24, 100) for j in range(3) for k in range(10)]
    return TL.bar_page(2048, 1536, bars, dev)


def mixed_times(dev, rec_model, reps):
    from ocrs_models_amd.inference import crops, detect, directions, drivers, lines, orient
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    page, det_model = painted_page(dev)
    kw = dict(size=(2048, 1536))
    for _ in range(2):
        inf.ocr_lines(det_model, rec_model, page, **kw), inf.ocr_lines(det_model, rec_model, page, directions="mixed", **kw)
    plain_ms, plain = _wall_ms(lambda: inf.ocr_lines(det_model, rec_model, page, **kw), reps)
    mixed_ms, mixed = _wall_ms(lambda: inf.ocr_lines(det_model, rec_model, page, directions="mixed", **kw), reps)
    det = inf.detect_words(det_model, page, **kw)
    H, W = page.shape[-2:]
    split_ms = _entry_ms("axis_split", lambda: inf.split_by_axis(det["quads"], H, W), reps)
    split = inf.split_by_axis(det["quads"], H, W)
    found = lines.find_lines_pages(split.quads, split.page_of_word, split.word_offs)
    store = detect.pack_pages([page, orient.turn_page(page, 1)])
    plan = crops.crop_plan(found.quads, 64, found.n_lines)
    batches, widths, perm = crops.crops_to_batches(crops.rectify_crops_pages(*store, found.quads, found.page_of_line, plan), plan)
    n = plan.host()[0]
    probe = found.page_of_line.index_select(0, plan.table[:n, 7].long())
    probe_ms, (flags, _) = _wall_ms(lambda: directions.line_directions(rec_model, batches, widths, probe), reps)
    flip_ms, final = _wall_ms(lambda: directions.turn_flagged(batches, widths, flags), reps)
    lpo = found.line_page_offs.tolist()
    read_ms, _ = _wall_ms(lambda: drivers._read_crops(rec_model, (final, widths, perm), DEFAULT_ALPHABET, split.quads, found, n, None, lpo), reps)
    return {"page": [H, W], "words": det["n"], "sideways_words": det["n"] - split.word_offs.tolist()[1], "plain_ms": round(plain_ms, 2), "plain_lines": len(plain),
            "mixed_ms": round(mixed_ms, 2), "mixed_lines": len(mixed), "directions": [g["direction"] for g in mixed if g["direction"]],
            "stages_ms": {"split": round(split_ms, 4), "probe_two_forwards": round(probe_ms, 2), "flip": round(flip_ms, 3), "final_read": round(read_ms, 2)},
            "chunks": [tuple(b.shape) for b in batches]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--det-model")
    ap.add_argument("--rec-model")
    ap.add_argument("--image", help="with the two checkpoints: print the direction and both scores of every line of this image")
    args = ap.parse_args()
    if len({bool(args.det_model), bool(args.rec_model), bool(args.image)}) != 1:
        ap.error("--det-model, --rec-model and --image go together")
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    if args.image:
        from PIL import Image

        from ocrs_models_amd.checkpoint import load_model_state

        det, rec = oa.DetectionModel().to(dev), oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
        load_model_state(args.det_model, det, dev)
        load_model_state(args.rec_model, rec, dev)
        img = torch.from_numpy(np.asarray(Image.open(args.image).convert("L"), dtype=np.uint8).copy())[None].to(dev)
        for g in inf.ocr_lines(det.eval(), rec.eval(), img, directions="mixed"):
            print(json.dumps({"text": g["text"], "direction": g["direction"], "direction_scores": g["direction_scores"], "quad": g["quad"]}), flush=True)
        return
    print(json.dumps({"axis_split": split_times(dev, args.reps), "gpu": gpu}), flush=True)
    print(json.dumps({"flip_crops": flip_times(dev, args.reps), "gpu": gpu}), flush=True)
    from tests import test_lines_gpu as TL

    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
    rec.load_state_dict(TL._golden_state("rec"))
    print(json.dumps({"mixed": mixed_times(dev, rec.eval(), max(args.reps // 3, 5)), "weights": "golden test weights", "gpu": gpu}), flush=True)


if __name__ == "__main__":
    main()

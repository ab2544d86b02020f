"""What reading a turned page costs on the GPU (csrc/page_orient.hip: inference.turn_page, orientation_votes, page_orientation).

    python tools/orient_time.py [--reps 50] [--det-model CKPT --rec-model CKPT [--image FILE]]

One JSON line each:

* ``turn``: the median ms of ``turn_page`` between stream events at 1024 x 1024 and at a 300 dpi A4 scan (3508 x 2480) for k = 1, 2, 3, next to
  a ``torch`` device copy of the same bytes -- the yardstick of a pass that can at best run at copy speed -- and both as GB/s (read + write).
* ``probe``: on a page of dots read with the golden test weights (tests/golden), or with the given checkpoints: the ms of the vote
  (``orientation_votes``), of the probe's crops (two turns, the quad table, plan, cut, batches; one host wait inside) and of the recogniser's
  forward with ``path_confidence``, wall-clock between device synchronisations.
* ``auto``: ``ocr_lines`` plain and with ``orientation="auto"`` on that page as it is and turned by a quarter, wall-clock, next to the detection
  alone and to ``page_orientation`` on a detection it is handed (the vote and the probe alone).

With ``--det-model/--rec-model`` (checkpoints of train_detection / train_rec) and ``--image`` the tool also prints the vote and both scores of
``page_orientation`` for all four turns of the image: how well the rule separates on trained weights.
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
from ocrs_models_amd.inference import orient  # noqa: E402

SIZES = {"1024x1024": (1024, 1024), "a4_300dpi": (3508, 2480)}


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


def _wall_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), out


def turn_times(dev, reps):
    L = lib()
    out = {}
    for name, (H, W) in SIZES.items():
        page = torch.randint(0, 256, (1, H, W), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(page)
        for k in (1, 2, 3):
            inf.turn_page(page, k)
        dst.copy_(page)
        row = {"copy_ms": round(_event_ms(lambda: dst.copy_(page), reps), 4)}
        for k in (1, 2, 3):
            L.timing = {"turn_page_u8": []}
            for _ in range(reps):
                inf.turn_page(page, k)
            torch.cuda.synchronize()
            timing, L.timing = L.timing, None
            row[f"k{k}_ms"] = round(statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing["turn_page_u8"]), 4)
        row["GBps"] = {key[:-3]: round(2 * H * W / (1e6 * ms), 1) for key, ms in row.items() if key.endswith("_ms")}
        out[name] = row
    return out


def load_models(args, dev):
    det, rec = oa.DetectionModel().to(dev), oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
    if args.det_model:
        from ocrs_models_amd.checkpoint import load_model_state

        load_model_state(args.det_model, det, dev)
        load_model_state(args.rec_model, rec, dev)
        return det.eval(), rec.eval(), "checkpoints"
    from tests import test_lines_gpu as TL

    det.load_state_dict(TL._golden_state("det"))
    rec.load_state_dict(TL._golden_state("rec"))
    return det.eval(), rec.eval(), "golden test weights"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--det-model")
    ap.add_argument("--rec-model")
    ap.add_argument("--image", help="with the two checkpoints: print the vote and both scores for all four turns of this image")
    args = ap.parse_args()
    if bool(args.det_model) != bool(args.rec_model) or (args.image and not args.det_model):
        ap.error("--det-model and --rec-model go together, and --image needs both")
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    print(json.dumps({"turn": turn_times(dev, args.reps), "gpu": gpu}), flush=True)

    det_model, rec_model, weights = load_models(args, dev)
    from tests import test_lines_gpu as TL

    page = TL.dot_page(1280, 960).to(dev)
    det = inf.detect_words(det_model, page)
    H, W = page.shape[-2:]
    found = inf.page_orientation(det_model, rec_model, page, det=det)
    if found["scores"] is not None:
        a, K = found["turns"] % 2, found["sampled"]
        _, _, picks = inf.orientation_votes(det["quads"])
        picked = det["quads"].index_select(0, picks[:K].long())

        def forward(batches):
            with torch.inference_mode():
                return [orient.path_confidence(rec_model(img), iw.div(4, rounding_mode="floor").int()) for img, iw in zip(*batches[:2])]

        votes_ms, _ = _wall_ms(lambda: inf.orientation_votes(det["quads"]), args.reps)
        probe_ms, batches = _wall_ms(lambda: orient.probe_batches(page, picked, a), args.reps)
        forward_ms, _ = _wall_ms(lambda: forward(batches), args.reps)
        print(json.dumps({"probe": {"words": det["n"], "voters": found["voters"], "sampled": K, "votes_ms": round(votes_ms, 3), "crops_ms": round(probe_ms, 3),
                                    "forward_ms": round(forward_ms, 3), "chunks": [tuple(b.shape) for b in batches[0]]}, "page": [H, W], "weights": weights,
                          "gpu": gpu}), flush=True)
    rows = {}
    for name, p in (("as_it_is", page), ("turned_by_1", inf.turn_page(page, 1))):
        for _ in range(2):
            inf.ocr_lines(det_model, rec_model, p), inf.ocr_lines(det_model, rec_model, p, orientation="auto")
        reps = max(args.reps // 3, 5)
        plain_ms, plain = _wall_ms(lambda: inf.ocr_lines(det_model, rec_model, p), reps)
        auto_ms, auto = _wall_ms(lambda: inf.ocr_lines(det_model, rec_model, p, orientation="auto"), reps)
        detect_ms, det_p = _wall_ms(lambda: inf.detect_words(det_model, p), reps)
        decide_ms, _ = _wall_ms(lambda: inf.page_orientation(det_model, rec_model, p, det=det_p), reps)  # the vote and the probe alone
        rows[name] = {"plain_ms": round(plain_ms, 2), "auto_ms": round(auto_ms, 2), "detect_ms": round(detect_ms, 2), "decide_ms": round(decide_ms, 2),
                      "lines": len(plain), "auto_lines": len(auto), "found": auto[0]["turns"] if auto else None}
    print(json.dumps({"auto": rows, "page": [H, W], "weights": weights, "gpu": gpu}), flush=True)

    if args.image:
        from PIL import Image

        img = torch.from_numpy(np.asarray(Image.open(args.image).convert("L"), dtype=np.uint8).copy())[None].to(dev)
        for k in range(4):  # the image turned by -k: the rule should find k
            fed = inf.turn_page(img, (4 - k) % 4)
            f = inf.page_orientation(det_model, rec_model, fed)
            print(json.dumps({"fed_turned_by": -k, "found": f["turns"], "votes": f["votes"], "voters": f["voters"], "sampled": f["sampled"], "scores": f["scores"]}),
                  flush=True)


if __name__ == "__main__":
    main()

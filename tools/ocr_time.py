"""What the page-inference stages cost on the GPU, next to the same stages done the reference's way on the host.

    python tools/ocr_time.py [--reps 20] [--words 300]

A synthetic 2048x1536 page with about ``--words`` dark word-sized bars (slightly rotated); the detection model has its default initialisation,
so the mask the later stages work on is painted from the bars instead of predicted (the forward is still timed).  One JSON line per stage:
median ms over ``--reps`` runs between device synchronisations, and for the stages the reference does on the host (numpy
``extract_cc_quads``, per-crop torch ``resize`` on the CPU) the host's ms, for orientation only.
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ocrs_models_amd as oa  # noqa: E402
from ocrs_models_amd import inference as inf  # noqa: E402
from ocrs_models_amd import input_pipeline as ip  # noqa: E402
from ocrs_models_amd import postprocess as pp  # noqa: E402

H, W = 2048, 1536


def make_page(words, seed=0):
    """(page (1,H,W) uint8, mask (H,W) uint8 of the word bars)"""
    r = np.random.RandomState(seed)
    cols = 10
    rows = -(-words // cols)
    y, x = np.mgrid[0:H, 0:W]
    page = np.full((H, W), 235, np.float32) + r.uniform(-10, 10, (H, W)).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    for i in range(words):
        cy, cx = (i // cols + 0.5) * H / rows, (i % cols + 0.5) * W / cols
        lng, sht, t = r.uniform(60, 130), r.uniform(18, 34), np.deg2rad(r.uniform(-4, 4))
        ys, xs = slice(max(int(cy) - 80, 0), int(cy) + 80), slice(max(int(cx) - 80, 0), int(cx) + 80)
        pu = (x[ys, xs] - cx) * np.cos(t) + (y[ys, xs] - cy) * np.sin(t)
        pv = -(x[ys, xs] - cx) * np.sin(t) + (y[ys, xs] - cy) * np.cos(t)
        inside = (np.abs(pu) <= lng / 2) & (np.abs(pv) <= sht / 2)
        mask[ys, xs][inside] = 1
        page[ys, xs][inside & ((x[ys, xs] // 3 + y[ys, xs] // 5) % 2 == 0)] = 30
    return torch.from_numpy(np.clip(page, 0, 255).astype(np.uint8))[None], torch.from_numpy(mask)


def gpu_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3)


def host_ms(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--words", type=int, default=300)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    torch.manual_seed(1234)
    det = oa.DetectionModel().to(dev).eval()
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev).eval()
    page_h, mask_h = make_page(args.words)
    page, mask_small = page_h.to(dev), F.interpolate(mask_h[None, None].float(), size=inf.MASK_SIZE, mode="nearest")[0, 0].to(dev) * 0.9

    def emit(stage, ms, host=None, **kw):
        print(json.dumps({"stage": stage, "gpu_ms": ms, "host_ms": host, **kw, "page": [H, W], "gpu": gpu}), flush=True)

    def forward():
        with torch.inference_mode():
            return det(ip.resize(ip.transform_image(page), inf.MASK_SIZE).unsqueeze(0))

    emit("transform + resize + detection forward", gpu_ms(forward, args.reps))
    probs_h = mask_small.cpu()
    emit("binarize_resize", gpu_ms(lambda: inf.binarize_resize(mask_small, (H, W)), args.reps),
         host_ms(lambda: F.interpolate((probs_h > 0.5).float()[None, None], size=(H, W), mode="nearest")))
    mask = inf.binarize_resize(mask_small, (H, W))
    mask_cpu = mask.cpu()
    emit("extract_cc_quads", gpu_ms(lambda: pp.extract_cc_quads_device(mask), args.reps), host_ms(lambda: pp.extract_cc_quads(mask_cpu), 1))
    quads0 = pp.extract_cc_quads_device(mask)
    emit("expand_quads", gpu_ms(lambda: inf.expand_quads(quads0, inf.SHRINK_DISTANCE), args.reps), n=quads0.shape[0])
    quads = inf.expand_quads(quads0, inf.SHRINK_DISTANCE)
    emit("crop_plan (+ totals to the host)", gpu_ms(lambda: inf.crop_plan(quads).host(), args.reps))
    plan = inf.crop_plan(quads)
    emit("rectify_crops", gpu_ms(lambda: inf.rectify_crops(page, quads, plan), args.reps), packed_floats=plan.host()[1])
    packed = inf.rectify_crops(page, quads, plan)
    tab = plan.table.cpu().tolist()
    crops_h = [packed[o:o + h * w].view(1, h, w).cpu() for h, w, _, o, *_ in tab]

    def host_resize():
        return [F.interpolate(c[None], size=(64, ip.line_output_width(c.shape[1], c.shape[2])), mode="bilinear", antialias=True, align_corners=False)
                for c in crops_h]

    emit("crops_to_batches", gpu_ms(lambda: inf.crops_to_batches(packed, plan), args.reps), host_ms(host_resize), crops=len(crops_h))
    batches = inf.crops_to_batches(packed, plan)
    emit("recognize_crops", gpu_ms(lambda: inf.recognize_crops(rec, batches), args.reps), batches=[list(b.shape) for b in batches[0]])

    def whole():
        # the page's own pipeline from the painted mask on (the untrained detector's mask is not the page's words)
        q = inf.expand_quads(pp.extract_cc_quads_device(inf.binarize_resize(mask_small, (H, W))), inf.SHRINK_DISTANCE)
        p = inf.crop_plan(q)
        return inf.recognize_crops(rec, inf.crops_to_batches(inf.rectify_crops(page, q, p), p))

    emit("mask -> text, all stages", gpu_ms(whole, args.reps))


if __name__ == "__main__":
    main()

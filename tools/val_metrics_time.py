"""Time the detection validation metrics on one batch: the device path (postprocess.batch_mask_metrics, B x 1024^2 fp32 masks on the GPU)
against the host path (postprocess.mask_metrics per image, what train_detection.test() runs by default) over the same images, plus the
eval-mode forward of the same batch for scale.  Synthetic word masks (rotated boxes, 10-80 x 6-20 px, +-0.3 rad); the prediction is the
target shifted by a pixel with a few words merged.  Prints one JSON line; checks that both paths give the same numbers.

    python tools/val_metrics_time.py [--batch 32] [--size 1024] [--words 240] [--reps 20] [--host-images N | --no-host]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def word_mask(H, W, n, r):
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        cx, cy, w, h, t = r.uniform(0, W), r.uniform(0, H), r.uniform(10, 80), r.uniform(6, 20), r.uniform(-0.3, 0.3)
        R = int(math.ceil(math.hypot(w, h) / 2)) + 1
        x0, x1, y0, y1 = max(0, int(cx) - R), min(W, int(cx) + R + 1), max(0, int(cy) - R), min(H, int(cy) + R + 1)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
        v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
        m[y0:y1, x0:x1] |= ((np.abs(u) <= w / 2) & (np.abs(v) <= h / 2)).astype(np.uint8)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--words", type=int, default=240)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=None, help="time the host path on the first N images only (default: all)")
    ap.add_argument("--no-host", action="store_true", help="device path only (for a profiler run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path")
    import ocrs_models_amd as oa
    from ocrs_models_amd import postprocess as pp

    dev = torch.device("cuda:0")
    r = np.random.RandomState(0)
    B, S = a.batch, a.size
    tg = np.stack([word_mask(S, S, a.words, r) for _ in range(B)])
    pr = np.roll(tg, (1, 1), axis=(1, 2)).copy()
    for i in range(B):
        for _ in range(5):
            y, x = r.randint(0, S - 40), r.randint(0, S - 260)
            pr[i, y:y + 40, x:x + 260] = 1
    target = torch.from_numpy(tg[:, None].astype(np.float32)).to(dev)
    pred = torch.from_numpy(pr[:, None].astype(np.float32)).to(dev)

    for _ in range(3):
        out = pp.batch_mask_metrics(pred, target)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out = pp.batch_mask_metrics(pred, target)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.reps
    res = {"tool": "val_metrics_time", "batch": B, "size": S, "device_ms": round(dev_ms, 4),
           "ws_bytes": oa._lib.lib().mask_metrics_ws_bytes(B, S, S)}

    model = oa.DetectionModel().to(dev).eval()
    img = (target - 0.5).contiguous()
    with torch.inference_mode():
        for _ in range(2):
            model(img)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(5):
            model(img)
        e1.record()
        torch.cuda.synchronize()
    res["eval_forward_ms"] = round(e0.elapsed_time(e1) / 5, 4)

    if not a.no_host:
        n = B if a.host_images is None else min(B, a.host_images)
        pc, tc = pred.cpu(), target.cpu()
        pp.mask_metrics(pc[0], tc[0])  # cold call (imports) outside the timed loop
        t0 = time.perf_counter()
        host = [pp.mask_metrics(pc[i], tc[i]) for i in range(n)]
        host_ms = (time.perf_counter() - t0) * 1e3 * B / n
        got = out.cpu()
        same = all(tuple(got[i].tolist()) == tuple(host[i][k] for k in pp.METRIC_KEYS) for i in range(n))
        res.update({"host_ms": round(host_ms, 1), "host_images_timed": n, "speedup": round(host_ms / dev_ms, 1), "identical": same})
        if not same:
            print(json.dumps(res))
            raise SystemExit("device and host metrics differ")
    res["components_per_image"] = round(float(np.mean([pp.extract_cc_quads(torch.from_numpy(tg[i])).shape[0] for i in range(min(B, 2))])), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

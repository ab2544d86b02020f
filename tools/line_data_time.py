"""Time per batch of the recognition training data with the device-resident line store, against the host-fed route and the CRNN step.

    python tools/line_data_time.py [--lines 4096] [--batch 256] [--iters 20] [--warmup 5] [--no-augment]

A synthetic store: line widths (at height 64) from ``sampler.config5_population``, crop heights uniform in 16 .. 96, each crop's polygon an
x-monotone band of 4-12 vertices on its bounding box, texts of the population's lengths.
  (a) device   datasets.DeviceLineLoader: index plan, augmentation draws, one pinned upload, ocrs_line_batch + ocrs_augment_lines
  (b) host     the route that existed before: host crops, PIL masks (generate_mask), augment.collate_lines (packs and uploads both)
Per route one JSON line: median / min / max ms per batch between hipEvents recorded on the stream before and after the batch is produced
(the host produces it, so this is the batch's wall time as the device sees it), the host's own median, and, from hipEvents placed directly
around the entry points, the device time of ocrs_line_batch and of ocrs_augment_lines.  Then the ratio to the 4.45 ms CRNN train step
(DESIGN.md section 8).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrs_models_amd._lib import lib  # noqa: E402
from ocrs_models_amd.augment import collate_lines  # noqa: E402
from ocrs_models_amd.datasets import DeviceLineLoader, HierTextRecognition  # noqa: E402
from ocrs_models_amd.sampler import config5_population, config5_sample  # noqa: E402

CRNN_STEP_MS = 4.45


def band_on_box(r, w, h, n):
    """An x-monotone band of n vertices whose bounding box is the (h, w) crop: a top chain from x = 0 to x = w in the upper half, a bottom
    chain back in the lower half (simple by construction)."""
    k = n // 2
    xs = [0] + sorted(r.sample(range(1, w), k - 2)) + [w]
    xs2 = sorted(r.sample(range(1, w), n - k), reverse=True)
    top = [(x, r.randint(0, h // 2 - 1)) for x in xs]
    bot = [(x, r.randint(h // 2 + 1, h)) for x in xs2]
    i, j = r.randrange(len(top)), r.randrange(len(bot))
    top[i], bot[j] = (top[i][0], 0), (bot[j][0], h)  # the box is touched above and below
    return top + bot


def make_lines(n, seed=0):
    widths, lengths = config5_population(n, seed)
    r, rs = random.Random(seed), np.random.RandomState(seed)
    crops, polys, texts = [], [], []
    for w64, L in zip(widths.tolist(), lengths.tolist()):
        h = r.randint(16, 96)
        w = max(h, int(round(w64 * h / 64)))
        crops.append(rs.randint(0, 256, (h, w), dtype=np.uint8))
        polys.append(band_on_box(r, w, h, r.randint(4, 12)))
        texts.append(config5_sample(max(w64, 10), L, rs)["text_seq"])
    return crops, polys, texts


def pil_mask(w, h, poly):
    """generate_mask(w, h, [poly], shrink_dist=0.0) of the reference (datasets/util.py:78-110) as a (h, w) uint8 array"""
    from PIL import Image, ImageDraw

    im = Image.new("1", (w, h), 0)
    ImageDraw.Draw(im).polygon(poly, fill="white", outline=None)
    return np.array(im, dtype=np.uint8)


class HostFed:
    """(b) with the same index plan: PIL masks per batch, then collate_lines from host tensors"""

    def __init__(self, crops, polys, texts, plan, dev, augment):
        self.crops, self.polys, self.texts, self.plan, self.dev, self.augment = [torch.from_numpy(c)[None] for c in crops], polys, texts, plan, dev, augment

    def __iter__(self):
        for idx in self.plan:
            samples = [{"image": self.crops[i], "mask": torch.from_numpy(pil_mask(self.crops[i].shape[2], self.crops[i].shape[1], self.polys[i]))[None],
                        "text_seq": self.texts[i]} for i in idx]
            yield collate_lines(samples, self.dev, augment=self.augment)


def time_batches(loader, iters, warmup):
    it = iter(loader)
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    lib().timing = {"line_batch": [], "augment_lines": []}
    ev, host = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        next(it)
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append((e0, e1))
    torch.cuda.synchronize()
    timing, lib().timing = lib().timing, None
    med = lambda v: round(sorted(v)[len(v) // 2], 3) if v else None  # noqa: E731
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": med(ms), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "host_median_ms": med(host),
            "line_batch_device_ms": med([a.elapsed_time(b) for a, b, _ in timing["line_batch"]]),
            "augment_lines_device_ms": med([a.elapsed_time(b) for a, b, _ in timing["augment_lines"]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--augment", default=True, action=argparse.BooleanOptionalAction)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    crops, polys, texts = make_lines(args.lines)
    t0 = time.perf_counter()
    ds = HierTextRecognition.from_lines(crops, polys, texts, augment=args.augment, device=dev)
    torch.cuda.synchronize()
    made = time.perf_counter() - t0
    store = sum(c.size for c in crops) + 8 * sum(len(p) for p in polys) + 28 * len(crops)
    plan = [[int(i) for i in np.random.RandomState(k).randint(0, len(ds), args.batch)] for k in range(args.iters + args.warmup)]
    routes = {"device": DeviceLineLoader(ds, batch_sampler=plan), "host": HostFed(crops, polys, texts, plan, dev, args.augment)}
    res = {}
    for name, loader in routes.items():
        torch.manual_seed(1234)
        random.seed(1234)
        res[name] = time_batches(loader, args.iters, args.warmup)
        print(json.dumps({"what": "batch", "route": name, "B": args.batch, "lines": len(ds), "augment": args.augment, "iters": args.iters,
                          **res[name], "gpu": torch.cuda.get_device_name(0)}), flush=True)
    d = res["device"]
    print(json.dumps({"what": "summary", "store_bytes": store, "construct_s": round(made, 3), "crnn_step_ms": CRNN_STEP_MS,
                      "device_route_of_step": round(d["median_ms"] / CRNN_STEP_MS, 3),
                      "device_kernels_of_step": round((d["line_batch_device_ms"] + d["augment_lines_device_ms"]) / CRNN_STEP_MS, 3),
                      "host_route_over_device_route": round(res["host"]["median_ms"] / d["median_ms"], 2)}), flush=True)


if __name__ == "__main__":
    main()

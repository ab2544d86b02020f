"""Time per batch of the detection training data with the device-resident page store, against the host-fed route and the detection step.

    python tools/page_data_time.py [--pages 64] [--batch 32] [--width 1600] [--height 1200] [--boxes 100] [--iters 20] [--warmup 3] [--no-augment]

A synthetic store: ``--pages`` grey pages of one size, each with ``--boxes`` word quads (jittered rectangles of text-like sizes laid out in
rows, some reaching over the page's edge).
  (a) device   datasets.DevicePageLoader: index plan, augmentation draws, one pinned upload, ocrs_page_batch + ocrs_augment_det
  (b) host     the route that existed before: host pages, PIL masks of the shrunk polygons (generate_mask; the polygons are shrunk once,
               outside the timing, which flatters this route: the reference shrinks them per item with shapely), augment.detection_batch
               (packs and uploads both)
Per route one JSON line: median / min / max ms per batch between hipEvents recorded on the stream before and after the batch is produced
(the host produces it, so this is the batch's wall time as the device sees it), the host's own median, and, from hipEvents placed directly
around the entry points, the device time of ocrs_page_batch and of ocrs_augment_det.  Then the ratio to the detection train step at this
batch size (README: 2648 images/s bf16, 1061 images/s fp32).
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

from ocrs_models_amd._lib import lib, ptr  # noqa: E402
from ocrs_models_amd.augment import detection_batch  # noqa: E402
from ocrs_models_amd.datasets import SHRINK_DISTANCE, DevicePageLoader, HierText  # noqa: E402

IMAGES_PER_S = {"bf16": 2648.0, "fp32": 1061.0}


def word_boxes(r: random.Random, w: int, h: int, n: int) -> list:
    """n word quads in text rows: heights 12 .. 40, widths 2 .. 6 heights, corners jittered by a pixel or two."""
    out, y = [], r.randint(0, 20)
    while len(out) < n:
        bh = r.randint(12, 40)
        x = r.randint(-10, 40)
        while x < w and len(out) < n:
            bw = r.randint(2 * bh, 6 * bh)
            j = lambda: r.randint(-2, 2)  # noqa: E731
            out.append([(x + j(), y + j()), (x + bw + j(), y + j()), (x + bw + j(), y + bh + j()), (x + j(), y + bh + j())])
            x += bw + r.randint(6, 30)
        y += bh + r.randint(4, 20)
        if y >= h:
            y = r.randint(0, 20)
    return out


def shrink_on_device(polys: list, dev) -> list:
    """The store's shrink for a list of polygons -> [[(x, y) int, ...] or []], read back once."""
    counts = np.array([len(p) for p in polys], dtype=np.int32)
    offs = np.cumsum(counts, dtype=np.int64) - counts
    verts = torch.tensor([v for p in polys for v in p], dtype=torch.int32, device=dev).reshape(-1, 2)
    V = verts.shape[0]
    d_offs, d_counts = torch.from_numpy(offs).to(dev), torch.from_numpy(counts).to(dev)
    ws = torch.empty(3 * V, dtype=torch.int32, device=dev)
    xy = torch.empty(2 * V, 2, dtype=torch.float64, device=dev)
    iv = torch.empty(2 * V, 2, dtype=torch.int32, device=dev)
    cnt = torch.empty(len(polys), dtype=torch.int32, device=dev)
    rows = torch.empty(len(polys), 2, dtype=torch.int32, device=dev)
    lib().shrink_polygons(ptr(verts), ptr(d_offs), ptr(d_counts), len(polys), SHRINK_DISTANCE, ptr(ws), ptr(xy), ptr(iv), ptr(cnt), ptr(rows))
    iv, cnt = iv.cpu().tolist(), cnt.cpu().tolist()
    return [[tuple(v) for v in iv[2 * o:2 * o + n]] for o, n in zip(offs.tolist(), cnt)]


def pil_page_mask(w: int, h: int, shrunk: list) -> np.ndarray:
    from PIL import Image, ImageDraw

    im = Image.new("1", (w, h), 0)
    draw = ImageDraw.Draw(im)
    for poly in shrunk:
        if poly:
            draw.polygon(poly, fill="white", outline=None)
    return np.array(im, dtype=np.uint8)


class HostFed:
    """(b) with the same index plan: PIL masks per batch, then detection_batch from host tensors"""

    def __init__(self, pages, shrunk, plan, dev, augment):
        self.pages, self.shrunk, self.plan, self.dev, self.augment = [torch.from_numpy(p)[None] for p in pages], shrunk, plan, dev, augment

    def __iter__(self):
        for idx in self.plan:
            masks = [torch.from_numpy(pil_page_mask(self.pages[i].shape[2], self.pages[i].shape[1], self.shrunk[i]))[None] for i in idx]
            yield detection_batch([self.pages[i] for i in idx], masks, self.dev, augment=self.augment)


def time_batches(loader, iters, warmup):
    it = iter(loader)
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    lib().timing = {"page_batch": [], "augment_det": []}
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
            "page_batch_device_ms": med([a.elapsed_time(b) for a, b, _ in timing["page_batch"]]),
            "augment_det_device_ms": med([a.elapsed_time(b) for a, b, _ in timing["augment_det"]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--augment", default=True, action=argparse.BooleanOptionalAction)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    r, rs = random.Random(0), np.random.RandomState(0)
    pages = [rs.randint(0, 256, (args.height, args.width), dtype=np.uint8) for _ in range(args.pages)]
    polys = [word_boxes(r, args.width, args.height, args.boxes) for _ in range(args.pages)]
    t0 = time.perf_counter()
    ds = HierText.from_pages(pages, polys, augment=args.augment, device=dev)
    torch.cuda.synchronize()
    made = time.perf_counter() - t0
    flat = shrink_on_device([q for p in polys for q in p], dev)
    shrunk = [flat[k * args.boxes:(k + 1) * args.boxes] for k in range(args.pages)]
    plan = [[int(i) for i in np.random.RandomState(k).randint(0, len(ds), args.batch)] for k in range(args.iters + args.warmup)]
    device_loader = DevicePageLoader(ds, batch_size=args.batch)
    device_loader.plan = lambda: iter(plan)
    routes = {"device": (device_loader, args.iters, args.warmup), "host": (HostFed(pages, shrunk, plan, dev, args.augment), args.host_iters, 1)}
    res = {}
    for name, (loader, iters, warmup) in routes.items():
        torch.manual_seed(1234)
        random.seed(1234)
        res[name] = time_batches(loader, iters, warmup)
        print(json.dumps({"what": "batch", "route": name, "B": args.batch, "page": [args.height, args.width], "boxes": args.boxes,
                          "skipped": ds.skipped, "augment": args.augment, "iters": iters, **res[name], "gpu": torch.cuda.get_device_name(0)}), flush=True)
    d = res["device"]
    steps = {k: round(1e3 * args.batch / v, 2) for k, v in IMAGES_PER_S.items()}
    print(json.dumps({"what": "summary", "construct_s": round(made, 3), "train_step_ms": steps,
                      "device_route_of_bf16_step": round(d["median_ms"] / steps["bf16"], 3),
                      "device_kernels_of_bf16_step": round((d["page_batch_device_ms"] + d["augment_det_device_ms"]) / steps["bf16"], 3),
                      "host_route_over_device_route": round(res["host"]["median_ms"] / d["median_ms"], 2)}), flush=True)


if __name__ == "__main__":
    main()

"""What detecting a large page in overlapping tiles costs on the GPU, stage by stage, next to the untiled ``detect_words`` of
the same page.

    python tools/tiles_time.py [--reps 10] [--words 1200] [--page 3508 2480] [--tile 1600 1200] [--tile-batch 16]

One synthetic 300 dpi A4 scan (3508x2480, about ``--words`` slightly rotated word bars of small print).  The detection model has its default
initialisation, so the probability maps the later stages work on are painted from the bars -- per tile window for the tiled leg, for the
whole page for the untiled one -- and the real forward is timed as a stage of its own and added to both totals.  One JSON line per leg:
median ms between device synchronisations over ``--reps`` runs after two warm-up calls of the same shapes.  Every stage is timed alone,
synchronised before and after, so the stages add up to more than the whole call.
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
from ocrs_models_amd.postprocess import extract_cc_quads_device  # noqa: E402


def make_page(H, W, words, seed=0):
    """(page (1,H,W) uint8, mask (H,W) uint8 of the word bars): bars about 20 px high, the x-height of 10 pt print at 300 dpi"""
    r = np.random.RandomState(seed)
    cols = 12
    rows = -(-words // cols)
    page = np.full((H, W), 235, np.float32) + r.uniform(-10, 10, (H, W)).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    for i in range(words):
        cy, cx = (i // cols + 0.5) * H / rows, (i % cols + 0.5) * W / cols
        lng, sht, t = r.uniform(80, 170), r.uniform(16, 22), np.deg2rad(r.uniform(-2, 2))
        ys, xs = slice(max(int(cy) - 100, 0), min(int(cy) + 100, H)), slice(max(int(cx) - 100, 0), min(int(cx) + 100, W))
        y, x = np.mgrid[ys, xs]
        pu = (x - cx) * np.cos(t) + (y - cy) * np.sin(t)
        pv = -(x - cx) * np.sin(t) + (y - cy) * np.cos(t)
        inside = (np.abs(pu) <= lng / 2) & (np.abs(pv) <= sht / 2)
        mask[ys, xs][inside] = 1
        page[ys, xs][inside & ((x // 3 + y // 5) % 2 == 0)] = 30
    return torch.from_numpy(np.clip(page, 0, 255).astype(np.uint8))[None], torch.from_numpy(mask)


class Painted(torch.nn.Module):
    """a detector that returns fixed probability maps: with ``tiled`` set the tile maps, chunk after chunk, otherwise the page map"""

    def __init__(self, tile_probs, page_probs):
        super().__init__()
        self.tile_probs, self.page_probs, self.at, self.tiled = tile_probs, page_probs, 0, False

    def forward(self, x):
        if self.tiled:
            a, self.at = self.at, (self.at + x.shape[0]) % self.tile_probs.shape[0]
            return self.tile_probs[a:a + x.shape[0], None]
        return self.page_probs[None, None]


def gpu_ms(fn, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--words", type=int, default=1200)
    ap.add_argument("--page", type=int, nargs=2, default=[3508, 2480], metavar=("H", "W"))
    ap.add_argument("--tile", type=int, nargs=2, default=[1600, 1200], metavar=("TH", "TW"))
    ap.add_argument("--tile-batch", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    torch.manual_seed(1234)
    H, W = args.page
    tile, size = tuple(args.tile), inf.MASK_SIZE
    det_real = oa.DetectionModel().to(dev).eval()
    page_h, mask_h = make_page(H, W, args.words)
    page = page_h.to(dev)
    plan = inf.tile_plan(H, W, tile)
    T = len(plan.windows)

    def nearest(m):
        return F.interpolate(m[None, None].float(), size=size, mode="nearest")[0, 0] * 0.9

    tile_probs = torch.stack([nearest(mask_h[y0:y0 + th, x0:x0 + tw]) for y0, x0, th, tw in plan.windows]).to(dev)
    det = Painted(tile_probs, nearest(mask_h).to(dev)).eval()
    common = {"page": [H, W], "tile": list(tile), "tiles": T, "size": list(size), "gpu": gpu}

    def emit(leg, ms, **kw):
        print(json.dumps({"leg": leg, "ms": ms, **kw, **common}), flush=True)

    # ---- the tiled stages, each alone
    store = (page.view(-1), torch.zeros(1, dtype=torch.int64, device=dev), torch.tensor([[H, W]], dtype=torch.int32, device=dev))
    emit("tiled stage: tile_plan + tile_tables (host, one copy)", gpu_ms(lambda: inf.tile_tables([inf.tile_plan(H, W, tile)], dev), args.reps))
    tables = inf.tile_tables([plan], dev)
    emit("tiled stage: tile batch", gpu_ms(lambda: inf.tile_batch(*store, tables.tiles, tables.max_th, size), args.reps),
         page_bytes=H * W, out_bytes=T * size[0] * size[1] * 4)
    imgs = inf.tile_batch(*store, tables.tiles, tables.max_th, size)

    def forward_tiles():
        with torch.inference_mode():
            return [det_real(imgs[a:a + args.tile_batch]) for a in range(0, T, args.tile_batch)]

    fwd_t = gpu_ms(forward_tiles, args.reps)
    emit("tiled stage: forward", fwd_t, chunks=-(-T // args.tile_batch))
    emit("tiled stage: compose", gpu_ms(lambda: inf.binarize_resize_tiles(tile_probs, tables, (H, W)), args.reps), canvas_bytes=H * W)
    mask_t = inf.binarize_resize_tiles(tile_probs, tables, (H, W))[0]
    emit("tiled stage: components (+ count to the host)", gpu_ms(lambda: extract_cc_quads_device(mask_t), args.reps), n=int(extract_cc_quads_device(mask_t).shape[0]))
    det.tiled = True
    whole_t = gpu_ms(lambda: inf.detect_words(det, page, tile=tile, tile_batch=args.tile_batch), args.reps)
    emit("tiled: detect_words (painted detector)", whole_t)
    emit("tiled: detect_words + forward", round(whole_t + fwd_t, 3))

    # ---- the untiled call of the same page
    det.tiled = False
    emit("untiled stage: transform_image + resize", gpu_ms(lambda: ip.resize(ip.transform_image(page), size), args.reps))
    img = ip.resize(ip.transform_image(page), size)

    def forward_page():
        with torch.inference_mode():
            return det_real(img.unsqueeze(0))

    fwd_p = gpu_ms(forward_page, args.reps)
    emit("untiled stage: forward", fwd_p)
    emit("untiled stage: binarize_resize", gpu_ms(lambda: inf.binarize_resize(det.page_probs, (H, W)), args.reps))
    mask_p = inf.binarize_resize(det.page_probs, (H, W))
    emit("untiled stage: components (+ count to the host)", gpu_ms(lambda: extract_cc_quads_device(mask_p), args.reps), n=int(extract_cc_quads_device(mask_p).shape[0]))
    whole_p = gpu_ms(lambda: inf.detect_words(det, page), args.reps)
    emit("untiled: detect_words (painted detector)", whole_p)
    emit("untiled: detect_words + forward", round(whole_p + fwd_p, 3))


if __name__ == "__main__":
    main()

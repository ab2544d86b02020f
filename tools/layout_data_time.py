"""Time per batch of the layout training data, and of one training epoch, with the device-resident loader and with what a user would
otherwise run.

    python tools/layout_data_time.py [--pages 2000] [--iters 20] [--warmup 5] [--no-epoch]

2 000 synthetic pages of 300-700 words are written to a temporary directory (1 600 train), N = 64, W = 500, randomize=True, shuffle on.
  (a) device   ocrs_models_amd.datasets.DeviceWebLayoutLoader: a plan of 64 indices and jitters, one pinned upload, one launch
  (b) stock    torch DataLoader(pin_memory=True) over the CPU restatement of the reference's dataset (tests/weblayout_ref.py: re-opens
               and re-parses a JSON file per item, as web_layout.py:76-186 does), followed by .to(device)
Per loader one JSON line: median / min / max ms per batch between hipEvents recorded on the stream before and after the batch is
produced (the host produces the batch, so this is the batch's wall time as the device sees it), the host's own median, and the one-time
construction cost.  Then, unless --no-epoch, one JSON line per loader with the wall time of a full train_layout.train() epoch (25 steps,
exact-fp32 parity mode, one warm-up step before the clock starts).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import tempfile
import time

import torch
from torch.utils.data import DataLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ocrs_models_amd as oa  # noqa: E402
from ocrs_models_amd.datasets import DeviceWebLayoutLoader, WebLayout  # noqa: E402
from tests.weblayout_ref import RefWebLayout  # noqa: E402

N, W, MAX_JITTER = 64, 500, 10


def write_pages(dst, pages, seed=0):
    r = random.Random(seed)
    for k in range(pages):
        left, paras, y = r.randint(300, 700), [], 10.0
        while left > 0:
            words = []
            for _ in range(min(left, r.randint(1, 60))):
                if not words or x > 1100:
                    x, y = 40.0, y + 22.0
                w = r.uniform(15, 110)
                words.append({"text": "w", "coords": [x, y, x + w, y + 17.5]})
                x += w + 5.5
            left -= len(words)
            paras.append({"words": words})
            y += 14.0
        with open(os.path.join(dst, f"page_{k:05d}.json"), "w") as f:
            json.dump({"resolution": {"width": 1280, "height": 720}, "paragraphs": paras}, f)


class _ToDevice:
    """(b): the stock loader with the copy train_layout.train() would make"""

    def __init__(self, loader, dev):
        self.loader, self.dev, self.dataset = loader, dev, loader.dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for x, y in self.loader:
            yield x.to(self.dev, non_blocking=True), y.to(self.dev, non_blocking=True)


def time_batches(loader, iters, warmup):
    it = iter(loader)
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    ev, host = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        batch = next(it)
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return batch, {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
                   "host_median_ms": round(sorted(host)[len(host) // 2], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-epoch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(randomize=True, padded_size=W, normalize_coords=False, max_jitter=MAX_JITTER)
    with tempfile.TemporaryDirectory() as d:
        write_pages(d, args.pages)
        made = {}

        def device_loader():
            t0 = time.perf_counter()
            ds = WebLayout(d, device=dev, **kw)
            torch.cuda.synchronize()
            made["device"] = time.perf_counter() - t0
            return DeviceWebLayoutLoader(ds, batch_size=N, shuffle=True)

        def stock_loader():
            t0 = time.perf_counter()
            ds = RefWebLayout(d, **kw)
            made["stock"] = time.perf_counter() - t0
            return _ToDevice(DataLoader(ds, batch_size=N, shuffle=True, pin_memory=True), dev)

        loaders = {"device": device_loader(), "stock": stock_loader()}
        assert len(loaders["device"]) >= args.iters + args.warmup, "not enough pages for iters + warmup batches in one epoch"
        checks = {}
        for name, loader in loaders.items():
            torch.manual_seed(1234)
            batch, res = time_batches(loader, args.iters, args.warmup)
            checks[name] = batch
            print(json.dumps({"what": "batch", "loader": name, "N": N, "W": W, "pages": len(loader.dataset), "iters": args.iters, **res,
                              "construct_s": round(made[name], 3), "gpu": torch.cuda.get_device_name(0)}), flush=True)
        same = all(torch.equal(a, b) for a, b in zip(checks["device"], checks["stock"]))
        print(json.dumps({"what": "check", "last_timed_batches_bit_equal": bool(same)}), flush=True)
        if args.no_epoch:
            return
        for name, loader in loaders.items():
            torch.manual_seed(1234)
            model = oa.LayoutModel().to(dev)
            opt = oa.train_layout.make_optimizer(model)
            model.train()
            oa.train_layout.train_step(model, opt, checks[name], dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = oa.train_layout.train(0, dev, loader, model, opt)
            dt = time.perf_counter() - t0
            print(json.dumps({"what": "epoch", "loader": name, "steps": len(loader), "epoch_s": round(dt, 3),
                              "ms_per_step": round(dt * 1e3 / len(loader), 3), "loss": round(loss, 6)}), flush=True)


if __name__ == "__main__":
    main()

"""Device time of the layout train step at the real size (N = 64 pages x W = 500 words): forward, weighted loss, backward, Adam.

    python tools/layout_time.py [--iters 20] [--warmup 5] [--modes hip_fp32,hip_x3,stock_fp32] [--once MODE]

hip_fp32: LayoutModel on the exact-fp32 GEMMs; hip_x3: the same under torch.autocast(bfloat16) (split-bf16 x3 GEMMs); stock_fp32: the stock
nn.TransformerEncoder model (export.AtenGraph's module in training mode, i.e. what a user of the reference runs today) with
torch.optim.Adam, same parameters, same batch, dropout 0.1 in all three.  Per mode one JSON line: median / min / max step time in ms from
hipEvents around each whole step (the host is kept ahead of the device by not synchronising inside the loop; warm-up steps excluded).
``--once MODE`` runs three warm-up steps and ONE step of a mode, for a kernel trace of a single step (run it under
``rocprofv3 --kernel-trace --stats -- python tools/layout_time.py --once hip_fp32``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ocrs_models_amd as oa  # noqa: E402

N, W = 64, 500


def batch(dev):
    g = torch.Generator().manual_seed(0)
    boxes = (torch.rand(N, W, 4, generator=g) * 1999).round()
    target = (torch.rand(N, W, 2, generator=g) < 0.08).float()
    return boxes.to(dev), target.to(dev)


def make_step(mode, dev):
    torch.manual_seed(1234)
    model = oa.LayoutModel().to(dev).train()
    boxes, target = batch(dev)
    if mode == "stock_fp32":
        class Stock(nn.Module):
            def __init__(self, m):
                super().__init__()
                self.m = m

            def forward(self, x):
                return self.m.classify(self.m.encode(self.m.embed(x)))

        net = Stock(model)
        opt = torch.optim.Adam(net.parameters(), lr=3e-4)
        loss_fn = nn.BCEWithLogitsLoss(pos_weight=torch.tensor((10.0, 10.0), device=dev))

        def step():
            opt.zero_grad()
            loss = loss_fn(net(boxes), target)
            loss.backward()
            opt.step()
            return loss
        return step
    opt = oa.train_layout.make_optimizer(model)
    loss_fn = oa.train_layout.weighted_loss()

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "hip_x3")):
            return oa.train_layout.train_step(model, opt, (boxes, target), dev, loss_fn)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="hip_fp32,hip_x3,stock_fp32")
    ap.add_argument("--once")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.once:
        step = make_step(args.once, dev)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        step()
        torch.cuda.synchronize()
        return
    for mode in args.modes.split(","):
        step = make_step(mode, dev)
        for _ in range(args.warmup):
            loss = step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for e0, e1 in ev:
            e0.record()
            loss = step()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        print(json.dumps({"mode": mode, "N": N, "W": W, "iters": args.iters, "median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3),
                          "max_ms": round(ms[-1], 3), "loss": round(float(loss), 6), "gpu": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()

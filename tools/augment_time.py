"""Device time of the training augmentations (ocrs_models_amd/augment.py) per batch, with hipEvents (no profiler).

    python tools/augment_time.py [--iters 20]

detection: B=32 uint8 1600x1200 sources + uint8 masks -> (32,1,800,600), mixed branches, fp32 and bf16 images.
recognition: B=256 uint8 48x300 crops + line masks -> (256,1,64,Wpad).
Per batch it prints one JSON line: the C entry point's device ms (kernels only, events around the call), the whole call's device ms from
host tensors (pinned pack + H2D copy + kernels), the kernel launches per call as csrc/augment.hip issues them (a fixed count, not
measured), the H2D copies and bytes (measured: the pinned staging buffers of the call) and the host time of the parameter sampler.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ocrs_models_amd import augment as A  # noqa: E402
from ocrs_models_amd._lib import lib  # noqa: E402

LAUNCHES = {"augment_det": 3, "augment_lines": 5}  # kernels per entry-point call, independent of B (csrc/augment.hip), not measured

_staged = []  # bytes of each pinned staging buffer (= one H2D copy) of the current call


def _counting_pin(parts, _pin=A.pin):
    host, offs = _pin(parts)
    _staged.append(host.numel())
    return host, offs


A.pin = _counting_pin


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def run(name, entry, sample, call, iters):
    L = lib()
    g = torch.Generator().manual_seed(0)
    rng = random.Random(0)
    for _ in range(3):
        call(sample(g, rng))
    torch.cuda.synchronize()
    kern, whole, host = [], [], []
    for _ in range(iters):
        _staged.clear()
        t0 = time.perf_counter()
        params = sample(g, rng)
        host.append((time.perf_counter() - t0) * 1e3)
        L.timing = {entry: []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(params)
        e1.record()
        torch.cuda.synchronize()
        (k0, k1, _), = L.timing[entry]
        kern.append(k0.elapsed_time(k1))
        whole.append(e0.elapsed_time(e1))
        L.timing = None
    print(json.dumps({"case": name, "kernel_ms": round(_median(kern), 4), "call_ms": round(_median(whole), 4),
                      "launches_expected": LAUNCHES[entry], "h2d_copies": len(_staged), "h2d_bytes": sum(_staged),
                      "sampler_host_ms": round(_median(host), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)

    sizes = [(1600, 1200)] * 32
    imgs = [torch.randint(0, 256, (1, h, w), generator=gen, dtype=torch.uint8) for h, w in sizes]
    masks = [(torch.rand(1, h, w, generator=gen) > 0.8).to(torch.uint8) for h, w in sizes]
    for dt in (torch.float32, torch.bfloat16):
        run(f"detection B=32 1600x1200 -> 800x600 {str(dt)[6:]}", "augment_det", lambda g, r: A.sample_detection_params(sizes, g, r),
            lambda p, dt=dt: A.detection_batch(imgs, masks, dev, augment=True, dtype=dt, params=p), a.iters)

    lsz = [(48, 300)] * 256
    lines = [{"image": torch.randint(0, 256, (1, h, w), generator=gen, dtype=torch.uint8), "text_seq": torch.ones(8, dtype=torch.int32),
              "mask": (torch.rand(1, h, w, generator=gen) > 0.1).to(torch.uint8)} for h, w in lsz]
    run("recognition B=256 48x300 -> 64xW fp32", "augment_lines", lambda g, r: A.sample_line_params(lsz, g, r),
        lambda p: A.collate_lines(lines, dev, augment=True, params=p), a.iters)


if __name__ == "__main__":
    main()

"""What grouping words into text lines costs on the GPU (inference.find_lines, csrc/text_lines.hip), next to the numpy restatement of the same
rule on the host (tests/lines_ref.py).

    python tools/lines_time.py [--reps 50]

Two synthetic sets of word quads, no models: a 2048x1536 page of about 300 slightly rotated words in about 30 lines, and a larger case of
4096 axis-aligned words in 64 lines (above the single-workgroup limit of the ranking stage).  One JSON line per stage and case: the median
ms between stream events around that stage's entry point over ``--reps`` runs, then the whole call between device synchronisations (which
includes the launch overhead of its 8+ kernels and the allocation of its outputs), and the host restatement's ms for orientation only.
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

from ocrs_models_amd import inference as inf  # noqa: E402
from ocrs_models_amd._lib import lib  # noqa: E402
from tests import lines_ref as R  # noqa: E402

H, W = 2048, 1536
STAGES = ("line_links", "line_rank", "line_order", "line_quads")


def page_words(rows=30, cols=10, seed=0):
    """about rows * cols words on the 2048x1536 page: rows of words 105..135 long and 24..34 high at a pitch of 153, turned by up to 2 degrees
    about a row direction of up to 3 degrees, so that neighbours are within max_gap of each other"""
    r = np.random.RandomState(seed)
    quads = []
    for i in range(rows):
        slope = np.deg2rad(r.uniform(-3, 3))
        for j in range(cols):
            cx = (j + 0.5) * W / cols
            cy = (i + 0.5) * H / rows + (cx - W / 2) * np.tan(slope)
            quads.append(R.rotated_rect(cx, cy, r.uniform(105, 135), r.uniform(24, 34), np.rad2deg(slope) + r.uniform(-2, 2)))
    q = np.stack(quads)
    return q[r.permutation(len(q))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    L = lib()
    for name, quads_h in (("page 2048x1536", page_words()), ("4096 words", R.grid_case(64, 64, seed=1))):
        quads = torch.from_numpy(quads_h).to(dev)
        for _ in range(3):
            lines = inf.find_lines(quads)
        n_lines = int(lines.n_lines)
        t0 = time.perf_counter()
        ref = R.find_lines(quads_h)
        host_ms = round((time.perf_counter() - t0) * 1e3, 3)
        assert ref["n_lines"] == n_lines, (ref["n_lines"], n_lines)
        L.timing = {s: [] for s in STAGES}
        for _ in range(args.reps):
            inf.find_lines(quads)
        torch.cuda.synchronize()
        timing, L.timing = L.timing, None
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf.find_lines(quads)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        common = {"case": name, "words": len(quads_h), "lines": n_lines, "gpu": gpu}
        for s in STAGES:
            ms = statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing[s])
            print(json.dumps({"stage": s, "gpu_ms": round(ms, 4), **common}), flush=True)
        print(json.dumps({"stage": "find_lines, whole call", "gpu_ms": round(statistics.median(wall), 4), "host_ms": host_ms, **common}), flush=True)


if __name__ == "__main__":
    main()

"""What putting text lines into reading order costs on the GPU (inference.reading_order, csrc/reading_order.hip), next to the numpy
restatement of the same rule on the host (tests/reading_ref.py).

    python tools/reading_order_time.py [--reps 50]

Three synthetic sets of line quads, no models: a two-column page of 60 lines under a heading (slightly rotated, as a scan is), a page of 1024
one-word lines in four columns, and a batch of 8 such 60-line pages.  One JSON line per stage and case: the median ms between stream events
around that stage's entry point over ``--reps`` runs, then the whole call between device synchronisations (which includes the launch
overhead of its six kernels and the allocation of its outputs and workspace), and the host restatement's ms for orientation only.
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
from tests import lines_ref as LR  # noqa: E402
from tests import reading_ref as RR  # noqa: E402

STAGES = ("reading_relation", "reading_peel", "reading_blocks")


def two_column_page(seed=0, deg=1.5):
    """60 lines: a heading across the page, then two columns of 29 and 30 lines 700 wide and 30 high at a pitch of 44 on a 1536-wide page, the
    right column 9 lower, the whole page turned by ``deg`` degrees; in find_lines' order"""
    r = np.random.RandomState(seed)
    lines = [LR.rotated_rect(768, 60, 1400, 40, 0)]
    for c, n in ((0, 29), (1, 30)):
        for k in range(n):
            w = 700 if k < n - 1 else r.uniform(200, 500)
            lines.append(LR.rotated_rect(50 + 736 * c + w / 2, 140 + 9 * c + 44 * k, w, 30, r.uniform(-0.3, 0.3)))
    q = np.stack(lines).astype(np.float64)
    t = np.deg2rad(deg)
    rot = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    q = ((q - [768, 1024]) @ rot.T + [768, 1024]).astype(np.float32)
    return RR.sort_lines(q)[0]


def text_lines(quads_h, offs, dev):
    n = len(quads_h)
    i32 = dict(dtype=torch.int32, device=dev)
    e = torch.empty(n, **i32)
    return inf.TextLines(torch.from_numpy(quads_h).to(dev), torch.tensor([n], **i32), e, e, torch.empty(n + 1, **i32), e,
                         None if offs is None else torch.tensor(offs, **i32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    L = lib()
    page = two_column_page()
    cases = (("two-column page, 60 lines", page, None),
             ("1024 one-word lines, four columns", RR.columns_case(1024, 4, h=8, row_pitch=12), None),
             ("8 pages of 60 lines", np.concatenate([two_column_page(seed) for seed in range(8)]), [60 * p for p in range(9)]))
    for name, quads_h, offs in cases:
        tl = text_lines(quads_h, offs, dev)
        for _ in range(3):
            ro = inf.reading_order(tl)
        t0 = time.perf_counter()
        ref = RR.reading_order(quads_h, offs)
        host_ms = round((time.perf_counter() - t0) * 1e3, 3)
        assert ro.line_order.cpu().tolist() == ref["line_order"].tolist() and ro.new_block.cpu().tolist() == ref["new_block"].tolist(), name
        L.timing = {s: [] for s in STAGES}
        for _ in range(args.reps):
            inf.reading_order(tl)
        torch.cuda.synchronize()
        timing, L.timing = L.timing, None
        wall = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inf.reading_order(tl)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        common = {"case": name, "lines": len(quads_h), "pages": 1 if offs is None else len(offs) - 1, "blocks": int(ref["new_block"].sum()),
                  "forced": ref["forced"], "gpu": gpu}
        for s in STAGES:
            ms = statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing[s])
            print(json.dumps({"stage": s, "gpu_ms": round(ms, 4), **common}), flush=True)
        print(json.dumps({"stage": "reading_order, whole call", "gpu_ms": round(statistics.median(wall), 4), "host_ms": host_ms, **common}), flush=True)


if __name__ == "__main__":
    main()

"""What cutting line crops along the word chain costs on the GPU (csrc/line_chain.hip: inference.line_spines, crop_plan_chain, rectify_chain; DESIGN.md
§21), next to the quad path on the line quads of the same lines (inference.crop_plan + rectify_crops).

    python tools/chain_time.py [--reps 50]

Two synthetic 2880 x 1536 pages, no models: 58 slightly rotated rows of 7 words (a few of which break into two lines), and 48 arcs of
radius 600 px over 44 degrees with 7 words each (word heights 24..34 px), grouped by ``inference.find_lines`` as ``ocr_lines`` does.  One JSON
line per page: the median ms between stream events around each stage's entry point over ``--reps`` runs, the two paths alternating in the
same loop, and the packed crop elements each path samples (the quad path cuts the rectangle around the whole arc).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrs_models_amd import inference as inf  # noqa: E402
from ocrs_models_amd._lib import lib  # noqa: E402
from tests import lines_ref as R  # noqa: E402

H, W = 2880, 1536
STAGES = ("line_spines", "crop_plan_dims", "rectify_chain", "crop_plan", "rectify_crops")


def straight_words(rows=58, cols=7, seed=0, pitch=48):
    """rows of words 165..190 long and 24..34 high, turned by up to 2 degrees about a row direction of up to 1 degree"""
    r = np.random.RandomState(seed)
    quads = []
    for i in range(rows):
        slope = np.deg2rad(r.uniform(-1, 1))
        for j in range(cols):
            cx = (j + 0.5) * W / cols
            cy = (i + 0.5) * pitch + (cx - W / 2) * np.tan(slope)
            quads.append(R.rotated_rect(cx, cy, r.uniform(165, 190), r.uniform(24, 34), np.rad2deg(slope) + r.uniform(-2, 2)))
    q = np.stack(quads)
    return q[r.permutation(len(q))], rows


def arc_words(rows=24, per_row=2, cols=7, seed=1, radius=600.0, span=44.0, pitch=118):
    """arcs of ``cols`` words 48..62 long and 24..34 high whose centres lie on a circle of ``radius``, tangent to it, the text running over the top"""
    r = np.random.RandomState(seed)
    quads = []
    for i in range(rows):
        for j in range(per_row):
            cx, top = (j + 0.5) * W / per_row, 30.0 + i * pitch
            for a in np.linspace(-span / 2, span / 2, cols):
                t = np.deg2rad(a)
                quads.append(R.rotated_rect(cx + radius * np.sin(t), top + radius * (1 - np.cos(t)), r.uniform(48, 62), r.uniform(24, 34), a))
    q = np.stack(quads)
    return q[r.permutation(len(q))], rows * per_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    L = lib()
    y, x = np.mgrid[0:H, 0:W]
    page = torch.from_numpy(np.clip(np.rint(127.5 + 80 * np.sin(x / 37.0) + 47 * np.cos(y / 53.0 + x / 91.0)), 0, 255).astype(np.uint8))[None].to(dev)
    for name, (words_h, want_lines) in (("straight", straight_words()), ("arcs", arc_words())):
        lines = inf.find_lines(torch.from_numpy(words_h).to(dev))

        def run():
            spines = inf.line_spines(lines)
            plan = inf.crop_plan_chain(spines)
            chain = inf.rectify_chain(page, spines, plan)
            qplan = inf.crop_plan(lines.quads, 64, lines.n_lines)
            quad = inf.rectify_crops(page, lines.quads, qplan)
            return plan, qplan, chain, quad

        for _ in range(3):
            plan, qplan, chain, quad = run()
        torch.cuda.synchronize()
        n_lines = plan.host()[0]
        assert n_lines == qplan.host()[0] and (name == "straight" or n_lines == want_lines)  # every arc chained into one line
        L.timing = {s: [] for s in STAGES}
        for _ in range(args.reps):
            run()
        torch.cuda.synchronize()
        timing, L.timing = L.timing, None
        ms = {s: round(statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing[s]), 4) for s in STAGES}
        heights = plan.table[:n_lines, 0].float().mean().item(), qplan.table[:n_lines, 0].float().mean().item()
        print(json.dumps({"page": name, "words": len(words_h), "lines": n_lines, "gpu_ms": ms, "chain_ms": round(sum(ms[s] for s in STAGES[:3]), 4),
                          "quad_ms": round(sum(ms[s] for s in STAGES[3:]), 4), "chain_elements": plan.host()[1], "quad_elements": qplan.host()[1],
                          "mean_crop_height": {"chain": round(heights[0], 1), "quad": round(heights[1], 1)}, "gpu": gpu}), flush=True)


if __name__ == "__main__":
    main()

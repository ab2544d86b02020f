"""What the characters of a page cost on the GPU (csrc/char_spans.hip: text.greedy_decode_spans_async, inference.char_boxes, inference.word_chars),
with the plain greedy decode (``ocrs_ctc_greedy_decode``, csrc/rec_seq.hip) on the same log-probs next to the one that keeps the spans.

    python tools/chars_time.py [--reps 50]

A synthetic page, no models: about 300 slightly rotated lines of 7 words (about 2000 words), grouped by ``inference.find_lines`` and planned by
``inference.crop_plan`` as ``ocr_lines`` does; synthetic log-probs (T = 209, C = 97: the recogniser's shape for the widest chunk) whose
arg-max runs look like text (runs of 1..6 steps of a class, blanks between).  One JSON line per stage: the median ms between stream events
around that stage's entry point over ``--reps`` runs, the two decodes alternating in the same loop on the same chunk of N = 256 samples.
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
from ocrs_models_amd import text  # noqa: E402
from ocrs_models_amd._lib import lib  # noqa: E402
from tests import lines_ref as R  # noqa: E402

T, N, C = 209, 256, 97
STAGES = ("ctc_decode_spans", "ctc_greedy_decode", "char_boxes", "word_chars")


def page_words(rows=300, cols=7, seed=0, W=1536, pitch=48):
    """rows * cols words: rows of words 165..190 long and 24..34 high, turned by up to 2 degrees about a row direction of up to 1 degree"""
    r = np.random.RandomState(seed)
    quads = []
    for i in range(rows):
        slope = np.deg2rad(r.uniform(-1, 1))
        for j in range(cols):
            cx = (j + 0.5) * W / cols
            cy = (i + 0.5) * pitch + (cx - W / 2) * np.tan(slope)
            quads.append(R.rotated_rect(cx, cy, r.uniform(165, 190), r.uniform(24, 34), np.rad2deg(slope) + r.uniform(-2, 2)))
    q = np.stack(quads)
    return q[r.permutation(len(q))]


def text_like_log_probs(n, seed=0):
    """(T, n, C) float32 log-probs whose arg-max is runs of 1..6 steps of one class with 0..3 blank steps between"""
    r = np.random.RandomState(seed)
    x = r.standard_normal((T, n, C)).astype(np.float32)
    for s in range(n):
        t = 0
        while t < T:
            t += int(r.randint(0, 4))
            e = min(T, t + int(r.randint(1, 7)))
            x[t:e, s, int(r.randint(1, C))] += 8.0
            t = e
    x[:, :, 0] += 4.0
    return torch.log_softmax(torch.from_numpy(x), dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    L = lib()
    text._DECODE_SIDE = False  # every stage on the one stream the events are recorded on
    words_h = page_words()
    lines = inf.find_lines(torch.from_numpy(words_h).to(dev))
    plan = inf.crop_plan(lines.quads, 64, lines.n_lines)
    n_lines = plan.host()[0]
    table = plan.table[:n_lines]
    in_len = (table[table[:, 7].long(), 2] // 4).long()  # by sorted position, as the chunks are
    lp = text_like_log_probs(n_lines).to(dev)
    chunks = [(a, min(a + N, n_lines)) for a in range(0, n_lines, N)]
    lps = [lp[:, a:b].contiguous() for a, b in chunks]
    spans = inf.CharSpans(*text.span_arrays(n_lines, T, dev))

    def run():
        for (a, b), x in zip(chunks, lps):
            text.greedy_decode_spans_async(x, in_len[a:b], spans.arrays(), a)
            if b - a == N:
                text.greedy_decode_batch_async(x, in_len[a:b])
        boxes = inf.char_boxes(lines.quads, plan, spans)
        return inf.word_chars(lines, plan, spans, boxes)

    for _ in range(3):
        ranges = run()
    torch.cuda.synchronize()
    chars = int(spans.lens.sum())
    assert int((ranges[:, 1] - ranges[:, 0]).clamp(min=0).sum()) <= chars
    L.timing = {s: [] for s in STAGES}
    for _ in range(args.reps):
        run()
    torch.cuda.synchronize()
    timing, L.timing = L.timing, None
    common = {"words": len(words_h), "lines": n_lines, "chars": chars, "gpu": gpu}
    for s in STAGES:
        recs = timing[s]
        if s == "ctc_decode_spans":  # the full chunk only: the shape the plain decode is timed at
            recs = [r for r in recs if r[2][5] == N]
        ms = statistics.median(e0.elapsed_time(e1) for e0, e1, _ in recs)
        shape = {"T": T, "N": N, "C": C} if s.startswith("ctc") else {}
        print(json.dumps({"stage": s, "gpu_ms": round(ms, 4), **shape, **common}), flush=True)


if __name__ == "__main__":
    main()

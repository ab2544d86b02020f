"""Time the end-to-end accuracy stage on one call: ``OcrAccuracyStats.update`` on the device -- one upload, the pair IoU, the
matching, the text comparison and the counters -- against the host restatement of the same rule (tests/eval_ref.py) on the same inputs, and
next to ``ocr_pages`` on as many pages of as many words, the work whose results it scores.  Synthetic pages: annotated words on a jittered
grid, predictions = perturbed copies (a few missing, a few extra), texts of 1 to 12 characters of which some are misread.  ``update`` is timed
with events around single calls (median of ``--reps`` after ``--warmup``); the event pair includes the host-side packing that precedes the
launches, which is part of what a caller waits for.  Prints one JSON line; checks that both paths give the same counters.

    python tools/eval_time.py [--pages 32] [--words 300] [--reps 20] [--warmup 5] [--host-pages N | --no-host] [--no-ocr]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rect(cx, cy, w, h, deg):
    t = np.deg2rad(deg)
    u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
    c = np.array([cx, cy])
    return np.array([c - w / 2 * u - h / 2 * v, c + w / 2 * u - h / 2 * v, c + w / 2 * u + h / 2 * v, c - w / 2 * u + h / 2 * v]).astype(np.float32)


def synthetic_page(words: int, r):
    """-> ((pred quads, pred texts), (gt quads, gt texts, ignore))"""
    cols = 15
    centres = [(30 + 40 * (k % cols) + r.uniform(-3, 3), 20 + 26 * (k // cols) + r.uniform(-2, 2)) for k in range(words)]
    text = lambda: "".join(chr(int(c)) for c in r.randint(97, 123, size=r.randint(1, 13)))  # noqa: E731
    gq = [rect(cx, cy, r.uniform(24, 34), r.uniform(10, 16), r.uniform(-4, 4)) for cx, cy in centres]
    gt = [text() for _ in gq]
    gi = [bool(r.rand() < 0.05) for _ in gq]
    pq, pt = [], []
    for (cx, cy), t in zip(centres, gt):
        if r.rand() < 0.05:
            continue  # a missed word
        pq.append(rect(cx + r.uniform(-2, 2), cy + r.uniform(-1, 1), r.uniform(24, 34), r.uniform(10, 16), r.uniform(-5, 5)))
        pt.append(t if r.rand() < 0.8 else text())
    for _ in range(words // 20):  # false positives anywhere on the page
        pq.append(rect(r.uniform(0, 40 * cols), r.uniform(0, 26 * (words // cols + 1)), r.uniform(24, 34), r.uniform(10, 16), r.uniform(-5, 5)))
        pt.append(text())
    return (pq, pt), (gq, gt, gi)


class DarkIsText(torch.nn.Module):
    """a detector without weights: dark pixels are text (the pages below are bars on white)"""

    def forward(self, x):
        return (x < 0).to(torch.float32)


def bar_pages(n: int, words: int, dev):
    H, W = 800, 600
    cols = 15
    page = np.full((H, W), 230, np.uint8)
    for k in range(words):
        x, y = 8 + 39 * (k % cols), 8 + 26 * (k // cols)
        if y + 10 < H:
            page[y:y + 10, x:x + 28] = 20
    return [torch.from_numpy(page.copy())[None].to(dev) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-pages", type=int, default=None, help="time the host restatement on the first N pages only (default: all)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-ocr", action="store_true", help="skip the ocr_pages timing")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the device path")
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.datasets import WordTruth
    from tests import eval_ref as R

    dev = torch.device("cuda:0")
    r = np.random.RandomState(0)
    cases = [synthetic_page(a.words, r) for _ in range(a.pages)]
    preds, truth = [c[0] for c in cases], [c[1] for c in cases]
    results = [[{"quad": q.tolist(), "text": t} for q, t in zip(pq, pt)] for pq, pt in preds]
    records = [WordTruth(None, np.stack(gq), gt, np.array(gi)) for gq, gt, gi in truth]

    times = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(a.warmup + a.reps):
        stats = inf.OcrAccuracyStats(dev)
        torch.cuda.synchronize()
        e0.record()
        stats.update(results, records)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append(e0.elapsed_time(e1))
    got = stats.counters()
    # the device share of it: events around each entry point (the library's own timing hooks), a run of their own
    L = oa._lib.lib()
    stages = ("eval_pair_iou", "eval_match", "eval_text_update")
    L.timing = {s: [] for s in stages}
    for _ in range(a.reps):
        inf.OcrAccuracyStats(dev).update(results, records)
    torch.cuda.synchronize()
    stage_ms = {s: round(statistics.median(e0_.elapsed_time(e1_) for e0_, e1_, _ in L.timing[s]), 4) for s in stages}
    L.timing = None
    res = {"stage_ms": stage_ms,"tool": "eval_time", "pages": a.pages, "words_per_page": a.words, "predictions": sum(len(p[0]) for p in preds),
           "pairs": stats.last["matches"].pair_offs[-1], "update_ms": round(statistics.median(times), 3), "update_ms_min": round(min(times), 3),
           "reps": a.reps, "counters": got}

    if not a.no_host:
        n = a.pages if a.host_pages is None else min(a.pages, a.host_pages)
        t0 = time.perf_counter()
        _, want = R.evaluate(preds[:n], truth[:n])
        host_ms = (time.perf_counter() - t0) * 1e3 * a.pages / n
        res.update({"host_ms": round(host_ms, 1), "host_pages_timed": n, "speedup": round(host_ms / res["update_ms"], 1)})
        if n == a.pages:
            res["identical"] = want == got
            if want != got:
                print(json.dumps(res))
                raise SystemExit("device and host counters differ")

    if not a.no_ocr:
        det, rec = DarkIsText().eval(), oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev).eval()
        pages = bar_pages(a.pages, a.words, dev)
        ocr = []
        for k in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inf.ocr_pages(det, rec, pages, lines=True, chars=True)
            torch.cuda.synchronize()
            if k:
                ocr.append((time.perf_counter() - t0) * 1e3)
        res.update({"ocr_pages_ms": round(min(ocr), 1), "ocr_words": sum(len(d["words"]) for p in out for d in p)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()

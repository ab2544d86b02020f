"""What reading a batch of pages costs on the GPU: ``ocr_pages`` next to a Python loop of ``ocr_lines`` over the same pages,
which is how a batch was read before ``ocr_pages`` existed.

    python tools/ocr_pages_time.py [--reps 10] [--words 300] [--batches 1,4,16]

The synthetic 2048x1536 page of tools/ocr_time.py (about ``--words`` slightly rotated word bars; every page of a batch is drawn with another
seed).  The detection model has its default initialisation, so the probability maps the later stages work on are painted from the bars; the
real forward is timed as a stage of its own and added to both totals.  One JSON line per leg and batch size: median ms between device
synchronisations over ``--reps`` runs, pages per second, and the number of host waits of one call (counted as tests/test_lines_gpu.py counts
them).  The per-stage lines of ``ocr_pages`` time each stage alone, synchronised before and after, so they add up to more than the whole call.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ocrs_models_amd as oa  # noqa: E402
from ocrs_models_amd import inference as inf  # noqa: E402
from ocrs_models_amd import input_pipeline as ip  # noqa: E402
from ocr_time import H, W, make_page  # noqa: E402


class Painted(torch.nn.Module):
    """a detector that returns fixed probability maps: (B,1,h,w) for the batch it was painted for, map k for the k-th single page"""

    def __init__(self, probs):
        super().__init__()
        self.probs = probs
        self.k = 0

    def forward(self, x):
        if x.shape[0] == self.probs.shape[0]:
            return self.probs[:, None]
        k, self.k = self.k, (self.k + 1) % self.probs.shape[0]
        return self.probs[k][None, None]


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


def count_waits(fn):
    calls = []
    saved = [(torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize"), (torch.cuda, "synchronize")]
    originals = [getattr(o, n) for o, n in saved]

    def counting(f):
        def g(*a, **k):
            calls.append(f.__qualname__)
            return f(*a, **k)
        return g

    for (o, n), f in zip(saved, originals):
        setattr(o, n, counting(f))
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        for (o, n), f in zip(saved, originals):
            setattr(o, n, f)
    return len(calls) + sum("synchroniz" in str(w.message).lower() for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--batches", default="1,4,16")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    torch.manual_seed(1234)
    det_real = oa.DetectionModel().to(dev).eval()
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev).eval()
    sizes = [int(b) for b in args.batches.split(",")]
    made = [make_page(args.words, seed) for seed in range(max(sizes))]
    all_pages = [p.to(dev) for p, _ in made]
    all_probs = torch.stack([F.interpolate(m[None, None].float(), size=inf.MASK_SIZE, mode="nearest")[0, 0] for _, m in made]).to(dev) * 0.9

    for B in sizes:
        pages, det = all_pages[:B], Painted(all_probs[:B].contiguous()).eval()
        common = {"B": B, "page": [H, W], "gpu": gpu}

        def emit(leg, ms, **kw):
            print(json.dumps({"leg": leg, "ms": ms, **kw, **common}), flush=True)

        def forward_batch():
            with torch.inference_mode():
                return det_real(torch.stack([ip.resize(ip.transform_image(p), inf.MASK_SIZE) for p in pages]))

        def forward_loop():
            with torch.inference_mode():
                return [det_real(ip.resize(ip.transform_image(p), inf.MASK_SIZE).unsqueeze(0)) for p in pages]

        fwd_b, fwd_l = gpu_ms(forward_batch, args.reps), gpu_ms(forward_loop, args.reps)
        emit("detection input + forward, one batch", fwd_b)
        emit("detection input + forward, one page at a time", fwd_l)

        def batch():
            return inf.ocr_pages(det, rec, pages)

        def loop():
            det.k = 0
            return [inf.ocr_lines(det, rec, p) for p in pages]

        got, ref = batch(), loop()
        assert [len(g) for g in got] == [len(r) for r in ref], ([len(g) for g in got], [len(r) for r in ref])
        assert all(a["quad"] == b["quad"] and a["words"] == b["words"] for g, r in zip(got, ref) for a, b in zip(g, r))
        n_lines, n_words = sum(len(g) for g in got), sum(len(l["words"]) for g in got for l in g)
        ms_b, ms_l = gpu_ms(batch, args.reps), gpu_ms(loop, args.reps)
        waits_b, waits_l = count_waits(batch), count_waits(loop)
        emit("ocr_pages (painted detector)", ms_b, host_waits=waits_b, words=n_words, lines=n_lines)
        emit("loop of ocr_lines (painted detector)", ms_l, host_waits=waits_l, words=n_words, lines=n_lines)
        emit("ocr_pages + forward", round(ms_b + fwd_b, 3), pages_per_s=round(B / (ms_b + fwd_b) * 1e3, 2), host_waits=waits_b)
        emit("loop of ocr_lines + forward", round(ms_l + fwd_l, 3), pages_per_s=round(B / (ms_l + fwd_l) * 1e3, 2), host_waits=waits_l)

        # the stages of ocr_pages, each alone
        page_sizes = torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev)
        probs = det.probs
        emit("stage: binarize_resize_pages", gpu_ms(lambda: inf.binarize_resize_pages(probs, page_sizes, (H, W)), args.reps))
        canvas = inf.binarize_resize_pages(probs, page_sizes, (H, W))
        emit("stage: cc_quads + gather (+ word offsets to the host)", gpu_ms(lambda: inf.cc_quads_pages(canvas), args.reps))
        flat, page_of_word, word_offs, _ = inf.cc_quads_pages(canvas)
        quads = inf.expand_quads(flat, inf.SHRINK_DISTANCE)
        emit("stage: pack_pages", gpu_ms(lambda: inf.pack_pages(pages), args.reps))
        store = inf.pack_pages(pages)
        emit("stage: find_lines_pages", gpu_ms(lambda: inf.find_lines_pages(quads, page_of_word, word_offs), args.reps))
        emit("stage: find_lines on the concatenation, for scale", gpu_ms(lambda: inf.find_lines(quads), args.reps))
        tl = inf.find_lines_pages(quads, page_of_word, word_offs)
        emit("stage: crop_plan (+ totals to the host)", gpu_ms(lambda: inf.crop_plan(tl.quads, count=tl.n_lines).host(), args.reps))
        plan = inf.crop_plan(tl.quads, count=tl.n_lines)
        emit("stage: rectify_crops_pages", gpu_ms(lambda: inf.rectify_crops_pages(*store, tl.quads, tl.page_of_line, plan), args.reps), packed_floats=plan.host()[1])
        packed = inf.rectify_crops_pages(*store, tl.quads, tl.page_of_line, plan)
        emit("stage: crops_to_batches", gpu_ms(lambda: inf.crops_to_batches(packed, plan), args.reps))
        batches = inf.crops_to_batches(packed, plan)
        emit("stage: recognize_crops", gpu_ms(lambda: inf.recognize_crops(rec, batches), args.reps), batches=[list(b.shape) for b in batches[0]])


if __name__ == "__main__":
    main()

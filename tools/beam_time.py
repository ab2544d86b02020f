"""What the beam-search decode costs on the GPU (csrc/ctc_beam.hip: text.beam_decode_spans_async) next to the greedy decode that keeps the spans
(``ocrs_ctc_decode_spans``, csrc/char_spans.hip) on the same log-probs, and next to the recogniser's eval forward of the batch they come from.

    python tools/beam_time.py [--reps 30]

No page, no trained model: synthetic log-probs of one full chunk (T = 209, N = 256, C = 97: the recogniser's shape for a 256 x 64 x 836 batch)
whose arg-max runs look like text (tools/chars_time.py's generator), input lengths spread over T/2..T.  One JSON line per stage: the median ms
between stream events around that stage's entry point over ``--reps`` runs -- ``ocrs_ctc_beam_decode`` at W = 4, 16 and 32,
``ocrs_ctc_align_spans`` on the W = 16 labellings, ``ocrs_ctc_decode_spans`` -- all alternating in one loop, then the eval forward of a
randomly initialised ``RecognitionModel`` on a 256 x 1 x 64 x 836 batch between events of its own, and the share of (forward + beam + align)
that the W = 16 beam with its alignment takes.  Then the language-model form: ``ocrs_ctc_beam_decode_lm`` with random gain
tables of orders 1, 2 and 3 next to ``ocrs_ctc_beam_decode`` at W = 4, 16 and 64, the four entry points alternating in one loop of their own
(no alignment launches), with the ratio of each order's median to the plain beam's at the same width.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrs_models_amd import text  # noqa: E402
from ocrs_models_amd._lib import lib  # noqa: E402
from ocrs_models_amd.recognition import RecognitionModel  # noqa: E402
from tools.chars_time import C, N, T, text_like_log_probs  # noqa: E402

WIDTHS = (4, 16, 32)
LM_WIDTHS, LM_ORDERS = (4, 16, 64), (1, 2, 3)


def random_gain(order: int, dev) -> torch.Tensor:
    """a dense table shaped like a smoothed model's: 0.7 log-softmax(1.5 N(0,1)) + 0.5 over the labels, column 0 (never read) at -inf"""
    g = torch.Generator().manual_seed(order)
    logp = torch.log_softmax(1.5 * torch.randn((C,) * (order - 1) + (C - 1,), generator=g, dtype=torch.float64), dim=-1)
    table = torch.full((C,) * order, float("-inf"), dtype=torch.float64)
    table[..., 1:] = 0.7 * logp + 0.5
    return table.float().contiguous().to(dev)


def time_lm(L, lp, in_len, reps: int, common: dict):
    """plain and LM entry points alternating in one loop -> one JSON line per (W, order) and per W for the plain beam"""
    dev = lp.device
    tables = {o: random_gain(o, dev) for o in LM_ORDERS}
    _, labels, _, _, _, lens = text.span_arrays(N, T, dev)
    score, lm_score = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    ws = torch.empty(L.ctc_beam_ws_bytes(T, N, max(LM_WIDTHS)), dtype=torch.uint8, device=dev)
    p = [t.data_ptr() for t in (lp, in_len, labels, lens, score, lm_score, ws)]

    def run():
        for w in LM_WIDTHS:
            L.ctc_beam_decode(p[0], p[1], T, N, C, w, 0, T, p[2], p[3], p[4], p[6], ws.numel())
            for o in LM_ORDERS:
                L.ctc_beam_decode_lm(p[0], p[1], T, N, C, w, tables[o].data_ptr(), o, 0, T, p[2], p[3], p[4], p[5], p[6], ws.numel())

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    L.timing = {s: [] for s in ("ctc_beam_decode", "ctc_beam_decode_lm")}
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    timing, L.timing = L.timing, None
    for w in LM_WIDTHS:  # (W is argument 5 of both entry points, the order argument 7 of the LM one)
        plain = statistics.median(e0.elapsed_time(e1) for e0, e1, a in timing["ctc_beam_decode"] if a[5] == w)
        print(json.dumps({"stage": "ctc_beam_decode", "loop": "lm", "W": w, "gpu_ms": round(plain, 4), **common}), flush=True)
        for o in LM_ORDERS:
            ms = statistics.median(e0.elapsed_time(e1) for e0, e1, a in timing["ctc_beam_decode_lm"] if a[5] == w and a[7] == o)
            print(json.dumps({"stage": "ctc_beam_decode_lm", "W": w, "order": o, "table_bytes": 4 * C ** o, "gpu_ms": round(ms, 4),
                              "ratio_to_plain": round(ms / plain, 4), **common}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    L = lib()
    lp = text_like_log_probs(N).to(dev)
    in_len = torch.linspace(T // 2, T, N).long().to(dev)
    out = {w: (text.span_arrays(N, T, dev), torch.empty(N, dtype=torch.float32, device=dev)) for w in WIDTHS}
    greedy = text.span_arrays(N, T, dev)

    def run():
        for w in WIDTHS:
            text.beam_decode_spans_async(lp, in_len, w, out[w][0], 0, out[w][1])
        text.greedy_decode_spans_async(lp, in_len, greedy, 0)

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    chars = {w: int(out[w][0][5].clamp(min=0).sum()) for w in WIDTHS}
    differ = {w: int((out[w][0][5] != greedy[5]).sum()) for w in WIDTHS}
    L.timing = {s: [] for s in ("ctc_beam_decode", "ctc_align_spans", "ctc_decode_spans")}
    for _ in range(args.reps):
        run()
    torch.cuda.synchronize()
    timing, L.timing = L.timing, None
    common = {"T": T, "N": N, "C": C, "gpu": gpu}
    ms = {}
    for w in WIDTHS:  # (the W of a call is argument 5 of ocrs_ctc_beam_decode)
        ms[w] = statistics.median(e0.elapsed_time(e1) for e0, e1, a in timing["ctc_beam_decode"] if a[5] == w)
        print(json.dumps({"stage": "ctc_beam_decode", "W": w, "gpu_ms": round(ms[w], 4), "chars": chars[w], "rows_whose_length_differs_from_greedy": differ[w],
                          **common}), flush=True)
    align = statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing["ctc_align_spans"][1::len(WIDTHS)])  # the W = 16 labellings
    print(json.dumps({"stage": "ctc_align_spans", "gpu_ms": round(align, 4), **common}), flush=True)
    spans = statistics.median(e0.elapsed_time(e1) for e0, e1, _ in timing["ctc_decode_spans"])
    print(json.dumps({"stage": "ctc_decode_spans", "gpu_ms": round(spans, 4), **common}), flush=True)
    time_lm(L, lp, in_len, args.reps, common)

    model = RecognitionModel(text.DEFAULT_ALPHABET).to(dev).eval()
    img = torch.rand(N, 1, 64, 4 * T, device=dev) - 0.5
    with torch.inference_mode():
        for _ in range(3):
            y = model(img)
        assert tuple(y.shape) == (T + 1, N, C), tuple(y.shape)  # (one step more than the 836 // 4 = 209 the decoders read)
        torch.cuda.synchronize()
        fwd = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(img)
            e1.record()
            fwd.append((e0, e1))
        torch.cuda.synchronize()
    forward = statistics.median(e0.elapsed_time(e1) for e0, e1 in fwd)
    print(json.dumps({"stage": "recognition_forward", "gpu_ms": round(forward, 4), "batch": [N, 1, 64, 4 * T], "gpu": gpu}), flush=True)
    share = (ms[16] + align) / (forward + ms[16] + align)
    print(json.dumps({"stage": "share", "beam16_plus_align_ms": round(ms[16] + align, 4), "greedy_spans_ms": round(spans, 4),
                      "share_of_forward_plus_decode": round(share, 4), "gpu": gpu}), flush=True)


if __name__ == "__main__":
    main()

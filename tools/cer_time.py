"""What the recognition loop's accuracy stats cost per training step, host against device (B = 256 x 1 x 64 x 400, T = 101).

    python tools/cer_time.py [--lengths 20,50,100] [--reps 5] [--steps 20] [--host-steps 3] [--warmup 5]

Per target length it times ``train_rec.train_step`` in four configurations, each with its own identically seeded model and optimizer:
  none         stats=None
  decode_only  the shim bench.py's CRNN leg uses (arg-max + collapse + copy to the host + list conversion, no edit distances)
  host         text.RecognitionAccuracyStats (what ``train_rec.train()`` runs by default)
  device       text.DeviceRecognitionAccuracyStats (``train(..., stats="device")``)
``--reps`` windows per configuration, interleaved (one window of each configuration per round), each window = ``--steps`` steps
(``--host-steps`` for `host`, whose steps take up to a second) between two device synchronisations; one JSON line per configuration with
the median / min / max of the windows' ms per step, and the mean decoded length the model produced (an untrained model decodes short
strings, which makes `host` cheaper than it is on a trained one).

The update alone is timed on synthetic log-probs that decode to about as many labels as the target has: `update_us_events` = hipEvents
around each ``update`` call (median of 50; includes the gaps between its launches), `update_us_graph` = the same update captured in a graph
and replayed 50 times between two events (device time of the launches alone), `decode_us_events` = the existing
``greedy_decode_batch_async`` the same way (arg-max + collapse + copies, on the main stream), `host_update_ms` = one host-stats update of
the same batch (wall clock).
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

import ocrs_models_amd as oa  # noqa: E402
from ocrs_models_amd import text, train_rec  # noqa: E402

B, H, W, C = 256, 64, 400, 97
T = W // 4 + 1


def labels_without_repeats(r, n, L):
    """(n, L) labels in [1, C) with no two equal neighbours (L = 100 targets stay CTC-feasible for the 100 usable time steps)"""
    y = r.randint(1, C, size=(n, L))
    for j in range(1, L):
        same = y[:, j] == y[:, j - 1]
        y[same, j] = y[same, j] % (C - 1) + 1
    return y.astype(np.int32)


def make_batches(L, n=4):
    r = np.random.RandomState(L)
    out = []
    for _ in range(n):
        textp = torch.zeros(B, text.round_up(L, 64), dtype=torch.int32)
        textp[:, :L] = torch.from_numpy(labels_without_repeats(r, B, L))
        out.append({"image": torch.from_numpy(r.uniform(-0.5, 0.5, (B, 1, H, W)).astype(np.float32)), "text_seq": textp,
                    "text_len": torch.full((B,), L, dtype=torch.int64), "image_width": torch.full((B,), W, dtype=torch.int64)})
    return out


class DecodeOnly:
    def update_async(self, targets, target_lengths, preds, pred_lengths):
        return text.greedy_decode_batch_async(preds, pred_lengths).result


def make_step(mode, dev):
    torch.manual_seed(1234)
    model = oa.RecognitionModel(text.DEFAULT_ALPHABET).to(dev).train()
    opt = train_rec.make_optimizer(model)
    loss_fn = oa.CTCLoss()
    stats = {"none": None, "decode_only": DecodeOnly(), "host": text.RecognitionAccuracyStats(),
             "device": text.DeviceRecognitionAccuracyStats()}[mode]

    def step(batch):
        return train_rec.train_step(model, opt, batch, dev, stats, loss_fn, check_nan=False)[0]
    return step, model


def synthetic_log_probs(r, L):
    """(T, B, C) log-probs whose greedy decode has L labels (min(L, T) without repeats): label, then blanks"""
    y = labels_without_repeats(r, B, T)
    cls = np.zeros((T, B), dtype=np.int64)
    n = min(L, T)
    cls[:n] = y[:, :n].T
    x = r.randn(T, B, C).astype(np.float32)
    np.put_along_axis(x, cls[..., None], 10.0, axis=-1)
    return torch.from_numpy(x).log_softmax(-1)


def time_update_alone(L, dev):
    r = np.random.RandomState(1000 + L)
    lp = synthetic_log_probs(r, L).to(dev)
    tg_h = torch.zeros(B, text.round_up(L, 64), dtype=torch.int32)
    tg_h[:, :L] = torch.from_numpy(labels_without_repeats(r, B, L))
    tl_h, il_h = [L] * B, [T - 1] * B
    tg, tl, il = tg_h.to(dev), torch.tensor(tl_h).to(dev), torch.tensor(il_h).to(dev)
    dstats, hstats = text.DeviceRecognitionAccuracyStats(), text.RecognitionAccuracyStats()

    def events(fn, n=50):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3

    upd = events(lambda: dstats.update(tg, tl, lp, il))
    side, text._DECODE_SIDE = text._DECODE_SIDE, False
    dec = events(lambda: text.greedy_decode_batch_async(lp, il))
    text._DECODE_SIDE = side
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dstats.update(tg, tl, lp, il)
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    gr = e0.elapsed_time(e1) * 1e3 / 50
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hstats.update(tg_h, tl_h, lp, il_h)
    host_ms = (time.perf_counter() - t0) * 1e3
    one = text.DeviceRecognitionAccuracyStats()
    one.update(tg, tl, lp, il)
    assert (one.char_errors, one.total_chars) == (hstats.char_errors, hstats.total_chars)
    return {"update_us_events": round(upd, 1), "update_us_graph": round(gr, 1), "decode_us_events": round(dec, 1), "host_update_ms": round(host_ms, 2),
            "char_errors": one.char_errors, "total_chars": one.total_chars}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="20,50,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="none,decode_only,host,device")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)
    modes = args.modes.split(",")
    for L in (int(v) for v in args.lengths.split(",")):
        batches = make_batches(L)
        steps, windows = {}, {m: [] for m in modes}
        for m in modes:
            steps[m], model = make_step(m, dev)
            for i in range(2 if m == "host" else args.warmup):
                steps[m](batches[i % len(batches)])
        torch.cuda.synchronize()
        with torch.no_grad():
            dec, _ = text.greedy_decode_batch(model(batches[0]["image"].to(dev)).float(), [T - 1] * B)
        pred_len = sum(len(row) for row in dec) / B
        for _ in range(args.reps):
            for m in modes:
                n = args.host_steps if m == "host" else args.steps
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    steps[m](batches[i % len(batches)])
                torch.cuda.synchronize()
                windows[m].append((time.perf_counter() - t0) * 1e3 / n)
        for m in modes:
            w = sorted(windows[m])
            print(json.dumps({"target_len": L, "mode": m, "ms_per_step_median": round(w[len(w) // 2], 3), "min": round(w[0], 3), "max": round(w[-1], 3),
                              "windows": len(w), "steps_per_window": args.host_steps if m == "host" else args.steps,
                              "mean_decoded_len": round(pred_len, 1), "B": B, "T": T, "gpu": gpu}), flush=True)
        print(json.dumps({"target_len": L, "mode": "update_alone", **time_update_alone(L, dev), "gpu": gpu}), flush=True)


if __name__ == "__main__":
    main()

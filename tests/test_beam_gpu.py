"""CTC prefix beam search and forced alignment on the GPU (csrc/ctc_beam.hip; text.beam_decode_spans / ctc_align_spans and ``beam_width`` of
the page drivers) against the numpy restatement of DESIGN.md §18 (tests/beam_ref.py, pinned by tests/test_beam_host.py).

Exhaustive regime.  Shapes small enough to score every labelling, W at least the number of prefixes: nothing is pruned, so the labels must be
the brute-force arg-max and the score the float64 CTC log-likelihood.  A case whose two best labellings are closer than 1e-4 is skipped, at
most 5 % (the host test asserts the same cap for the same inputs).

Pruned regime.  Peaky inputs like a trained recogniser's, mixed input lengths, one batch at row0 > 0.  The float64 restatement supplies the
final top-1 / top-2 gap and the smallest gap between the best surviving prefix of the answer and the first pruned candidate; a case with
either below 1e-3 is skipped, at most 10 %.  Otherwise labels equal float64 exactly and the score stays within the bound.

Score bound.  Each step adds at most about three fp32 roundings at the running magnitude S and one logaddexp evaluation:
|score - score64| <= T (3 * 2^-24 * S + 1e-6), S = max(1, |score64|); the 1e-6 stands for the hardware exp2 / log2 and is measured here: the
tests print the largest error they saw (DESIGN.md §18 records it).

Alignment.  Integer-valued log-probs make every sum exact in fp32 and ties frequent: t0, t1, peak and lens equal the restatement with ``==``.
Gaussian ones: the path the spans describe, summed in float64, reaches the float64 Viterbi optimum within T * 2^-24 * S."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beam_ref as B
from tests import ocr_ref
from tests import test_chars_gpu as CG
from tests import test_lines_gpu as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def det_model(dev):
    import ocrs_models_amd as oa

    m = oa.DetectionModel()
    m.load_state_dict(TL._golden_state("det"))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def rec_model(dev):
    import ocrs_models_amd as oa

    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    m.load_state_dict(TL._golden_state("rec"))
    return m.to(dev).eval()


def _split(buf, rows, ld):
    labels, t0, t1, peak_bits = (buf[k * rows * ld:(k + 1) * rows * ld].reshape(rows, ld) for k in range(4))
    return dict(labels=labels, t0=t0, t1=t1, peak_bits=peak_bits, peak=peak_bits.view(np.float32), lens=buf[4 * rows * ld:])


def _beam(dev, lp_ntc, in_len, W, row0=0, rows=None, ld=None):
    """one beam_decode_spans_async call on (N,T,C) host log-probs into sentinel-filled arrays -> the arrays on the host, and the scores"""
    from ocrs_models_amd import text

    N, T, C = lp_ntc.shape
    rows, ld = N + row0 if rows is None else rows, T if ld is None else ld
    lp = torch.from_numpy(np.ascontiguousarray(np.transpose(lp_ntc, (1, 0, 2)))).to(dev)
    out = text.span_arrays(rows, ld, dev)
    out[0].fill_(SENT)
    scores = torch.full((rows,), float(SENT), dtype=torch.float32, device=dev)
    assert text.beam_decode_spans_async(lp, [int(v) for v in in_len], W, out, row0, scores) is None
    return _split(out[0].cpu().numpy(), rows, ld), scores.cpu().numpy()


def _untouched(a, sc, row0, N):
    """nothing past a row's length, nothing in the rows of other calls"""
    rows = len(a["lens"])
    outside = [i for i in range(rows) if not row0 <= i < row0 + N]
    for key in ("labels", "t0", "t1", "peak_bits"):
        assert (a[key][outside] == SENT).all()
        for n in range(N):
            assert (a[key][row0 + n, max(int(a["lens"][row0 + n]), 0):] == SENT).all(), (key, n)
    assert (a["lens"][outside] == SENT).all() and (sc[outside] == SENT).all()


def _spans_are_a_path(a, row, lp, in_len):
    """the spans of a row describe one alignment of its labels: ascending, disjoint, inside the input, a blank between equal neighbours, and
    peak is the largest log-prob of the label over the span, copied"""
    k = int(a["lens"][row])
    lab, t0, t1 = a["labels"][row, :k], a["t0"][row, :k], a["t1"][row, :k]
    assert (t0 <= t1).all() and (t0 >= 0).all() and (t1 < max(min(int(in_len), lp.shape[0]), 1)).all()
    assert (t0[1:] > t1[:-1]).all()
    assert all(t0[j + 1] > t1[j] + 1 for j in range(k - 1) if lab[j] == lab[j + 1])
    for j in range(k):
        assert a["peak"][row, j].tobytes() == lp[t0[j]:t1[j] + 1, lab[j]].max().tobytes()


# ------------------------------------------------------------------ exhaustive regime -------------------------------------------------------
@pytest.mark.parametrize("shape", B.EXHAUSTIVE_SHAPES)
def test_unpruned_beam_is_the_brute_force_argmax(dev, shape):
    C, T, W = shape
    lp = B.exhaustive_inputs(C, T)
    a, sc = _beam(dev, lp, [T] * len(lp), W)
    skipped, worst, worst_abs = 0, 0.0, 0.0
    for n, x in enumerate(lp):
        labels, ll, gap = B.best_labellings(x)
        if gap < B.EXHAUSTIVE_MIN_GAP:
            skipped += 1
            continue
        assert a["labels"][n, :a["lens"][n]].tolist() == labels, n
        worst, worst_abs = max(worst, abs(sc[n] - ll) / B.score_bound(T, ll)), max(worst_abs, abs(sc[n] - ll))
        _spans_are_a_path(a, n, x, T)
    print(f"(C, T, W) = {shape}: skipped {skipped} of {len(lp)}; score off by at most {worst_abs:.2e} = {worst:.3f} of the bound")
    assert skipped <= B.EXHAUSTIVE_MAX_SKIP * len(lp)
    assert worst <= 1.0
    _untouched(a, sc, 0, len(lp))


# ------------------------------------------------------------------ pruned regime -----------------------------------------------------------
@pytest.fixture(scope="module")
def pruned(dev):
    """every pruned shape once: the inputs, the float64 restatement and the GPU's answer (the second shape at row0 = 3 of a larger buffer)"""
    out = {}
    for k, (C, T, W, J) in enumerate(B.PRUNED_SHAPES):
        lp, in_len = B.peaky_inputs(C, T, J)
        row0 = 3 if k == 1 else 0
        a, sc = _beam(dev, lp, in_len, W, row0=row0, rows=len(lp) + row0 + 2, ld=T + (5 if k == 1 else 0))
        out[(C, T, W)] = (lp, in_len, row0, a, sc, [B.beam_search(x, il, W) for x, il in zip(lp, in_len)])
    return out


@pytest.mark.parametrize("shape", [s[:3] for s in B.PRUNED_SHAPES])
def test_pruned_beam_equals_the_float64_restatement(pruned, shape):
    C, T, W = shape
    lp, in_len, row0, a, sc, ref = pruned[shape]
    skipped, worst, worst_abs = 0, 0.0, 0.0
    for n, (x, il, r) in enumerate(zip(lp, in_len, ref)):
        row = row0 + n
        assert 0 <= a["lens"][row] <= il and ((a["labels"][row, :a["lens"][row]] >= 1) & (a["labels"][row, :a["lens"][row]] < C)).all()
        if min(r["gap"], r["prune_gap"]) < B.PRUNED_MIN_MARGIN:
            skipped += 1
            continue
        assert a["labels"][row, :a["lens"][row]].tolist() == r["labels"], n
        err = abs(sc[row] - r["score"])
        worst, worst_abs = max(worst, err / B.score_bound(T, r["score"])), max(worst_abs, err)
        _spans_are_a_path(a, row, x, il)
    print(f"(C, T, W) = {shape}: skipped {skipped} of {len(lp)}; score off by at most {worst_abs:.2e} = {worst:.3f} of the bound")
    assert skipped <= B.PRUNED_MAX_SKIP * len(lp)
    assert worst <= 1.0
    _untouched(a, sc, row0, len(lp))


def test_the_beam_differs_from_greedy_somewhere(pruned):
    n = 0
    for (C, T, W), (lp, in_len, row0, a, sc, ref) in pruned.items():
        n += sum(a["labels"][row0 + i, :a["lens"][row0 + i]].tolist() != B.greedy(x, il) for i, (x, il) in enumerate(zip(lp, in_len)))
    print(f"beam != greedy in {n} of {sum(len(v[0]) for v in pruned.values())} cases")
    assert n >= 1


# ------------------------------------------------------------------ invariants on arbitrary inputs ------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 64])
@pytest.mark.parametrize("CT", [(97, 40), (5, 70)])
def test_score_never_exceeds_the_labellings_likelihood(dev, CT, W):
    C, T = CT
    rng = np.random.default_rng([C, T, W])
    lp = B.log_softmax(rng.standard_normal((6, T, C))).astype(np.float32)
    in_len = [T, T, T - 1, T // 2, T + 5, 1]
    a, sc = _beam(dev, lp, in_len, W)
    worst = -np.inf
    for n, x in enumerate(lp):
        k, il = int(a["lens"][n]), min(in_len[n], T)
        lab = a["labels"][n, :k]
        assert 0 <= k <= il and ((lab >= 1) & (lab < C)).all()
        ll = B.ctc_log_likelihood(x[:il], lab.tolist())
        worst = max(worst, (sc[n] - ll) / B.score_bound(T, ll))
        _spans_are_a_path(a, n, x, il)
    print(f"C = {C}, T = {T}, W = {W}: score - log-likelihood of the labelling at most {worst:.3f} of the bound")
    assert worst <= 1.0
    _untouched(a, sc, 0, len(lp))


# ------------------------------------------------------------------ edges -------------------------------------------------------------------
def _against_ref(a, sc, lp, in_len, W, row0=0):
    """labels equal the float64 restatement wherever its margins allow, the score stays within the bound -> cases compared"""
    T, compared = lp.shape[1], 0
    for n, (x, il) in enumerate(zip(lp, in_len)):
        r, row = B.beam_search(x, il, W), row0 + n
        assert not np.isnan(sc[row]) and not np.isnan(a["peak"][row, :max(a["lens"][row], 0)]).any()
        if min(r["gap"], r["prune_gap"]) >= 1e-3:
            assert a["labels"][row, :max(a["lens"][row], 0)].tolist() == r["labels"], n
            assert (sc[row] == r["score"]) if np.isinf(r["score"]) else abs(sc[row] - r["score"]) <= B.score_bound(T, r["score"]), n
            compared += 1
    return compared


def test_input_lengths_all_blank_and_two_classes(dev):
    T = 9
    for C, W in ((2, 1), (2, 64), (6, 1), (6, 5), (6, 64)):
        lp, _ = B.peaky_inputs(C, T, 8.0, seed=3, cases=7)
        lp[5] = -9.0
        lp[5, :, 0] = -0.001  # all blank
        lp[6] = np.log(1.0 / C)  # every candidate of a step ties
        in_len = [0, 1, T - 1, T, T + 5, T, T]
        a, sc = _beam(dev, lp, in_len, W, row0=1, rows=10, ld=T + 2)
        assert a["lens"][1] == 0 and sc[1] == 0.0  # in_len 0: the empty labelling at score 0
        assert a["lens"][2] <= 1 and a["lens"][6] == 0
        assert abs(sc[6] - T * -0.001) < 1e-4
        assert _against_ref(a, sc, lp, in_len, W, row0=1) >= 3
        _untouched(a, sc, 1, 7)
        for n in range(7):
            _spans_are_a_path(a, 1 + n, lp[n], in_len[n])


def test_classes_at_minus_infinity_give_no_nan(dev):
    C, T = 5, 12
    rng = np.random.default_rng(11)
    lp = B.log_softmax(rng.standard_normal((6, T, C))).astype(np.float32)
    lp[0, :, 2] = -np.inf          # a class that never occurs
    lp[1, 3, 0] = -np.inf          # a step without the blank
    lp[2, :, 1:] = -np.inf         # only the blank
    lp[3, :, 0] = -np.inf          # never the blank
    lp[4, 5, :] = -np.inf          # a step without any class: nothing survives it
    for W in (1, 4, 64):
        a, sc = _beam(dev, lp, [T] * 6, W)
        assert not np.isnan(sc).any()
        assert _against_ref(a, sc, lp, [T] * 6, W) >= 2
        assert a["lens"][2] == 0 and sc[4] == -np.inf
        assert a["lens"][4] == -1  # no labelling of finite mass: the beam leaves the empty one at -inf, which the alignment marks
        assert not (a["labels"][0, :a["lens"][0]] == 2).any() and a["lens"][3] >= 1
        _untouched(a, sc, 0, 6)


@pytest.mark.parametrize("W", [1, 3, 64])
def test_equal_totals_keep_the_candidate_order(dev, W):
    """values whose sums are exact, so that totals tie exactly: slot ascending, stay before extend, label ascending"""
    lp = np.full((4, 2, 5), -1.0, dtype=np.float32)
    lp[1, :, 0] = -2.0   # the extensions tie above the stay: the lowest label
    lp[2, 0, 2] = -0.5   # step 0 decides for label 2; at step 1 its stay (-1.5 + log 2) beats every extension
    lp[3, 0, :3] = -3.0  # labels 3 and 4 tie
    a, sc = _beam(dev, lp, [1, 1, 2, 1], W)
    assert [a["labels"][n, :a["lens"][n]].tolist() for n in range(4)] == [[], [1], [2], [3]]
    assert sc[0] == -1.0 and sc[1] == -1.0 and sc[3] == -1.0
    for n in range(4):
        r = B.beam_search(lp[n], [1, 1, 2, 1][n], W)
        assert r["labels"] == a["labels"][n, :a["lens"][n]].tolist() and abs(r["score"] - sc[n]) < 1e-6


@pytest.mark.parametrize("N", [1, 70])
def test_batch_sizes_widths_and_equal_bytes(dev, N):
    from ocrs_models_amd import text

    C, T = 17, 30
    lp, in_len = B.peaky_inputs(C, T, 10.0, seed=7, cases=N)
    for W in (1, 64):
        a, sc = _beam(dev, lp, in_len, W, row0=2, rows=N + 4, ld=T + 1)
        b, sd = _beam(dev, lp, in_len, W, row0=2, rows=N + 4, ld=T + 1)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a) and sc.tobytes() == sd.tobytes()
        _untouched(a, sc, 2, N)
        if N == 1 or W == 1:
            assert _against_ref(a, sc, lp[:8], in_len[:8], W, row0=2) >= 1
    # arrays of its own: the same values through the handle
    res = text.beam_decode_spans(torch.from_numpy(np.ascontiguousarray(lp.transpose(1, 0, 2))).to(dev), in_len.tolist(), 64)
    for n, r in enumerate(res):
        k = a["lens"][2 + n]
        assert set(r) == {"labels", "t0", "t1", "peak", "score"} and r["score"] == sc[2 + n]
        assert r["labels"] == a["labels"][2 + n, :k].tolist() and r["t0"] == a["t0"][2 + n, :k].tolist() and r["t1"] == a["t1"][2 + n, :k].tolist()
        assert np.asarray(r["peak"], dtype=np.float32).tobytes() == a["peak"][2 + n, :k].tobytes()


def test_unsupported_widths_and_class_counts_are_refused(dev):
    from ocrs_models_amd import text
    from ocrs_models_amd._lib import lib, ptr

    T, N = 4, 2
    for C, W in ((4, 0), (4, 65), (4, -1), (1, 4), (257, 4)):
        lp = torch.zeros(T, N, C, device=dev)
        il = torch.full((N,), T, dtype=torch.int64, device=dev)
        out = text.span_arrays(N, T, dev)
        out[0].fill_(SENT)
        sc = torch.full((N,), float(SENT), device=dev)
        ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match="bad argument"):
            lib().ctc_beam_decode(ptr(lp), ptr(il), T, N, C, W, 0, T, ptr(out[1]), ptr(out[5]), ptr(sc), ptr(ws), ws.numel())
        torch.cuda.synchronize()
        assert (out[0] == SENT).all() and (sc == SENT).all()  # nothing was launched
        with pytest.raises(RuntimeError):
            text.beam_decode_spans(lp, il, W)
    lp = torch.zeros(T, N, 4, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):  # a workspace that is too small
        lib().ctc_beam_decode(ptr(lp), ptr(il), T, N, 4, 8, 0, T, ptr(out[1]), ptr(out[5]), ptr(sc), ptr(ws), 8)
    with pytest.raises(RuntimeError, match="input lengths"):
        text.beam_decode_spans(lp, [T], 4)
    with pytest.raises(RuntimeError, match="do not fit"):
        text.beam_decode_spans_async(lp, [T, T], 4, text.span_arrays(N, T, dev), 1, sc)
    with pytest.raises(RuntimeError, match="scores"):
        text.beam_decode_spans_async(lp, [T, T], 4, text.span_arrays(N, T, dev), 0, None)


# ------------------------------------------------------------------ alignment ---------------------------------------------------------------
def _align(dev, lp_ntc, in_len, labellings):
    from ocrs_models_amd import text

    N, T, C = lp_ntc.shape
    L = max(max(len(l) for l in labellings), 1)
    lab = np.full((N, L), 1, dtype=np.int32)
    for n, l in enumerate(labellings):
        lab[n, :len(l)] = l
    lp = torch.from_numpy(np.ascontiguousarray(np.transpose(lp_ntc, (1, 0, 2)))).to(dev)
    out = text.ctc_align_spans(lp, [int(v) for v in in_len], torch.from_numpy(lab), [len(l) for l in labellings])
    return _split(out[0].cpu().numpy(), N, max(T, L))


def _labellings(rng, N, T, C):
    """lengths 0..T with repeats, among them T distinct-neighbour labels (every step a character) and T equal ones (infeasible beyond T = 1)"""
    out = [rng.integers(1, C, size=int(rng.integers(0, T + 1))).tolist() for _ in range(N - 4)]
    return out + [[1 + (k % (C - 1)) for k in range(T)], [1] * T, [2] * ((T + 1) // 2), [1] * (T + 1)]


@pytest.mark.parametrize("T", [5, 64, 70])
def test_alignment_of_integer_log_probs_equals_the_restatement(dev, T):
    C, N = 4, 24
    rng = np.random.default_rng(T)
    lp = rng.integers(-8, 1, size=(N, T, C)).astype(np.float32)
    labellings = _labellings(rng, N, T, C)
    in_len = [T] * N
    in_len[0], in_len[1] = T - 1, T + 5
    a = _align(dev, lp, in_len, labellings)
    feasible = 0
    for n, l in enumerate(labellings):
        r = B.align(lp[n], in_len[n], l, np.float32)
        assert a["lens"][n] == r["lens"], n
        if r["lens"] < 0:
            continue
        feasible += 1
        k = len(l)
        assert a["t0"][n, :k].tolist() == r["t0"] and a["t1"][n, :k].tolist() == r["t1"], n
        assert a["peak"][n, :k].tobytes() == np.asarray(r["peak"], dtype=np.float32).tobytes(), n
        assert a["labels"][n, :k].tolist() == l
    assert feasible >= N // 3 and a["lens"][N - 1] == -1 and (T == 1 or a["lens"][N - 3] == -1) and a["lens"][N - 4] == T


@pytest.mark.parametrize("T", [5, 64, 70])
def test_alignment_of_gaussian_log_probs_reaches_the_viterbi_optimum(dev, T):
    C, N = 6, 16
    rng = np.random.default_rng(100 + T)
    lp = B.log_softmax(rng.standard_normal((N, T, C))).astype(np.float32)
    labellings = _labellings(rng, N, T, C)
    a = _align(dev, lp, [T] * N, labellings)
    worst = 0.0
    for n, l in enumerate(labellings):
        r = B.align(lp[n], T, l, np.float64)
        assert a["lens"][n] == r["lens"], n
        if r["lens"] < 0:
            continue
        _spans_are_a_path(a, n, lp[n], T)
        got, _ = B.path_score(lp[n], l, a["t0"][n, :len(l)].tolist(), a["t1"][n, :len(l)].tolist())
        bound = T * 2.0 ** -24 * max(1.0, abs(r["score"]))
        worst = max(worst, (r["score"] - got) / bound)
        assert got <= r["score"] + 1e-9
    print(f"T = {T}: the aligned path misses the float64 optimum by at most {worst:.3f} of the bound")
    assert worst <= 1.0


def test_infeasible_labellings_and_alignment_arguments(dev):
    from ocrs_models_amd import text

    lp = np.zeros((5, 4, 3), dtype=np.float32)
    lp[4, 1, 0] = lp[4, 1, 2] = -np.inf  # the only step that could hold the blank between the two 1s cannot
    a = _align(dev, lp, [4, 2, 4, 3, 4], [[1, 2, 1, 2, 1], [1, 1], [1, 1, 1], [1, 2], [1, 1]])
    assert a["lens"].tolist() == [-1, -1, -1, 2, 2]  # L > T; no room for the blank (twice); feasible; -inf leaves other ways
    a = _align(dev, lp, [4, 4, 4, 4, 4], [[1, 3], [0], [1, 1], [], [2, 1, 2, 1]])
    assert a["lens"].tolist() == [-1, -1, 2, 0, 4]  # labels outside 1..C-1
    lp[4, :, 0] = -np.inf
    assert _align(dev, lp, [4] * 5, [[1]] * 4 + [[1, 1]])["lens"].tolist() == [1, 1, 1, 1, -1]
    x = torch.zeros(4, 2, 3, device=dev)
    with pytest.raises(RuntimeError, match="label rows"):
        text.ctc_align_spans(x, [4, 4], [[1]], [1])
    with pytest.raises(RuntimeError, match="input lengths"):
        text.ctc_align_spans(x, [4], [[1], [1]], [1, 1])


def test_one_hot_inputs_give_the_greedy_spans(dev):
    from ocrs_models_amd import text

    for T, N, C, W in ((70, 9, 7, 4), (209, 5, 97, 16), (5, 3, 2, 1)):
        rng = np.random.default_rng(T)
        lp = rng.uniform(-40.0, -35.0, size=(N, T, C)).astype(np.float32)
        for n in range(N):
            win = np.repeat(rng.integers(0, C, size=T), rng.integers(1, 5, size=T))[:T]
            lp[n, np.arange(T), win] = rng.uniform(-1.0, 0.0, size=T).astype(np.float32)
        in_len = [T] * N
        in_len[0] = T - 2
        x = torch.from_numpy(np.ascontiguousarray(lp.transpose(1, 0, 2))).to(dev)
        greedy, beam = text.greedy_decode_spans(x, in_len), text.beam_decode_spans(x, in_len, W)
        for g, b in zip(greedy, beam):
            assert {k: b[k] for k in g} == g
            assert b["score"] <= 0.0


# ------------------------------------------------------------------ end to end: painted detector, stub recogniser ----------------------------
def _reference_rows(stub, batches, W):
    """what the restatement reads from the stub's log-probs for every crop, in quad order: (text, score, gap)"""
    from ocrs_models_amd.text import DEFAULT_ALPHABET, decode_text

    rows = []
    for img, iw in zip(batches[0], batches[1]):
        lp = stub(torch.zeros(1, 1, 64, img.shape[-1]))[:, 0].numpy()
        for w in iw.tolist():
            r = B.beam_search(lp, w // 4, W)
            rows.append((decode_text(r["labels"], list(DEFAULT_ALPHABET)), r["score"], min(r["gap"], r["prune_gap"]), max(w // 4, 1)))
    return [rows[p] for p in batches[2]]


def test_prescribed_log_probs_where_beam_and_greedy_disagree(dev):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    rows, cols, W = 4, 3, 8
    bars = [(15 + 52 * c, 18 + 40 * r, 40, 12) for r in range(rows) for c in range(cols)]
    page, det = TL.bar_page(190, 200, bars, dev)
    size = (190, 200)
    found = inf.detect_words(det, page, size=size)
    lines = inf.find_lines(found["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    ow = int(plan.table.cpu().numpy()[0, 2])
    T = ow // 4
    # visible characters (three steps above the blank) and a hidden one: two steps just below the blank, -0.6 and -0.725 against -0.5, so
    # every step's arg-max is the blank while the alignments that say "x" together outweigh the one that does not
    steps = [3 + 5 * k for k in range(6)]
    assert steps[-1] + 8 < T
    chars = [(t - 1, t + 1, DEFAULT_ALPHABET.index(ch) + 1, -(k + 1) / 64) for k, (ch, t) in enumerate(zip("ab cde", steps))]
    hidden = steps[-1] + 4
    stub = CG.Stub(chars + [(hidden, hidden + 1, DEFAULT_ALPHABET.index("x") + 1, -0.6)], len(DEFAULT_ALPHABET) + 1).eval()

    def staged(quads, count=None):
        p = inf.crop_plan(quads, count=count)
        return _reference_rows(stub, inf.crops_to_batches(inf.rectify_crops(page, quads, p), p), W)

    ref_lines, ref_words = staged(lines.quads, lines.n_lines), staged(found["quads"])
    assert all(r[0] == "ab cdex" and r[2] > 1e-3 for r in ref_lines) and all(r[2] > 1e-3 for r in ref_words)
    greedy = inf.ocr_lines(det, stub, page, size=size)
    assert [g["text"] for g in greedy] == ["ab cde"] * rows  # the greedy decode misses the hidden character on every line

    def check(got, ref, keys):
        assert len(got) == len(ref)
        for g, (text, score, _, steps_) in zip(got, ref):
            assert set(g) == keys and g["text"] == text and abs(g["log_prob"] - score) <= B.score_bound(steps_, score)

    line_keys = {"quad", "text", "words", "log_prob"}
    char_keys = {"char_quads", "char_log_probs"}
    plain = inf.ocr_lines(det, stub, page, size=size, beam_width=W)
    check(plain, ref_lines, line_keys)
    assert [{k: v for k, v in p.items() if k != "log_prob"} | {"text": "ab cde"} for p in plain] == greedy  # everything but the decode is unchanged
    full = inf.ocr_lines(det, stub, page, size=size, beam_width=W, chars=True)
    check(full, ref_lines, line_keys | char_keys | {"word_chars", "word_texts"})
    for g, p in zip(full, plain):
        assert {k: g[k] for k in p} == p
        assert len(g["char_quads"]) == len(g["char_log_probs"]) == len(g["text"]) == 7
        assert g["char_log_probs"][:6] == [c[3] for c in chars] and g["char_log_probs"][6] == float(np.float32(-0.6))  # the peak of every span, untouched
        assert [g["text"][s:e] for s, e in g["word_chars"]] == g["word_texts"] and len(g["word_chars"]) == len(g["words"]) == cols
        xs = [np.mean([pt[0] for pt in q]) for q in g["char_quads"]]
        assert all(b > a for a, b in zip(xs, xs[1:]))  # left to right along the line
        ys = [pt[1] for q in g["char_quads"] for pt in q]
        assert abs(min(ys) - min(pt[1] for pt in g["quad"])) < 1e-3 and abs(max(ys) - max(pt[1] for pt in g["quad"])) < 1e-3  # the line's own height
        f = ocr_ref.crop_frame(g["quad"], np.float64)
        pts = np.asarray(g["char_quads"], dtype=np.float64).reshape(-1, 2) - f["origin"]
        s, r = pts @ f["u"], pts @ f["v"]
        assert max(-s.min(), s.max() - f["long"], -r.min(), r.max() - f["short"]) <= 8 * CG.R.ulp32(float(np.abs(np.asarray(g["quad"])).max()))
    words = inf.ocr_page(det, stub, page, size=size, beam_width=W)
    check(words, ref_words, {"quad", "text", "log_prob"})
    wchars = inf.ocr_page(det, stub, page, size=size, beam_width=W, chars=True)
    check(wchars, ref_words, {"quad", "text", "log_prob"} | char_keys)
    assert all(len(w["char_quads"]) == len(w["text"]) == len(w["char_log_probs"]) for w in wchars)
    assert inf.ocr_pages(det, stub, [page], size=size, beam_width=W) == [plain]
    assert inf.ocr_pages(det, stub, [page], size=size, beam_width=W, chars=True) == [full]
    assert inf.ocr_pages(det, stub, [page], lines=False, size=size, beam_width=W) == [words]
    assert inf.ocr_pages(det, stub, [page], lines=False, size=size, beam_width=W, chars=True) == [wchars]
    ro = inf.ocr_lines(det, stub, page, size=size, beam_width=W, reading_order=True)
    assert sorted(json.dumps({k: v for k, v in d.items() if k != "block"}, sort_keys=True) for d in ro) == sorted(json.dumps(p, sort_keys=True) for p in plain)


# ------------------------------------------------------------------ end to end: golden weights ----------------------------------------------
SIZE = (160, 120)


def test_golden_weights_structure(dev, det_model, rec_model):
    from ocrs_models_amd import inference as inf

    page = TL.dot_page(320, 240).to(dev)
    greedy = inf.ocr_lines(det_model, rec_model, page, size=SIZE, chars=True)
    assert inf.ocr_lines(det_model, rec_model, page, size=SIZE, chars=True, beam_width=None) == greedy
    assert inf.ocr_lines(det_model, rec_model, page, size=SIZE, beam_width=None) == inf.ocr_lines(det_model, rec_model, page, size=SIZE)
    assert inf.ocr_page(det_model, rec_model, page, size=SIZE, beam_width=None) == inf.ocr_page(det_model, rec_model, page, size=SIZE)
    assert inf.ocr_pages(det_model, rec_model, [page], size=SIZE, chars=True, beam_width=None) == [greedy]
    beam = inf.ocr_lines(det_model, rec_model, page, size=SIZE, chars=True, beam_width=8)
    assert len(beam) == len(greedy) > 0
    for b, g in zip(beam, greedy):
        assert set(b) == set(g) | {"log_prob"} and b["quad"] == g["quad"] and b["words"] == g["words"]
        assert len(b["char_quads"]) == len(b["char_log_probs"]) == len(b["text"])
        assert isinstance(b["log_prob"], float) and b["log_prob"] <= 1e-4 and all(v <= 0.0 for v in b["char_log_probs"])
        assert [b["text"][s:e] for s, e in b["word_chars"]] == b["word_texts"]
    assert inf.ocr_lines(det_model, rec_model, page, size=SIZE, chars=True, beam_width=8) == beam  # two runs, equal results
    assert [{k: c[k] for k in p} for p, c in zip(inf.ocr_lines(det_model, rec_model, page, size=SIZE, beam_width=8), beam)] == \
        inf.ocr_lines(det_model, rec_model, page, size=SIZE, beam_width=8)
    # the spans themselves: one row per crop, t0 non-decreasing, t0 <= t1, and a score per row
    det = inf.detect_words(det_model, page, size=SIZE)
    lines = inf.find_lines(det["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    batches = inf.crops_to_batches(inf.rectify_crops(page, lines.quads, plan), plan)
    texts, spans, scores = inf.recognize_crops(rec_model, batches, chars=True, beam_width=8)
    assert (texts, scores) == inf.recognize_crops(rec_model, batches, beam_width=8) and texts == [b["text"] for b in beam]
    assert scores == [b["log_prob"] for b in beam] and spans.scores is not None
    lens, t0, t1 = spans.lens.cpu().numpy(), spans.t0.cpu().numpy(), spans.t1.cpu().numpy()
    for p, k in enumerate(lens):
        assert k >= 0 and (np.diff(t0[p, :k]) > 0).all() and (t0[p, :k] <= t1[p, :k]).all()
    assert inf.decode_crop_spans(rec_model, batches).scores is None
    print(f"golden models: {len(beam)} lines; beam text differs from greedy on {sum(b['text'] != g['text'] for b, g in zip(beam, greedy))}")


def test_beam_adds_no_host_wait(dev, rec_model):
    """both beam forms decode into one span buffer that is copied once: the waits of a page stay what they are for the greedy decode"""
    from ocrs_models_amd import inference as inf

    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)]
    page, det = TL.bar_page(230, 340, bars, dev)
    kw = dict(size=(230, 340))
    calls = {
        "lines": lambda **k: inf.ocr_lines(det, rec_model, page, **kw, **k),
        "lines+chars": lambda **k: inf.ocr_lines(det, rec_model, page, chars=True, **kw, **k),
        "words": lambda **k: inf.ocr_page(det, rec_model, page, **kw, **k),
        "words+chars": lambda **k: inf.ocr_page(det, rec_model, page, chars=True, **kw, **k),
    }
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        for f in calls.values():
            f(), f(beam_width=8)
    for name, f in calls.items():
        _, n_greedy, what = TL._count_waits(f)
        got, n_beam, what_beam = TL._count_waits(lambda: f(beam_width=8))
        print(f"host waits of {name}: greedy {n_greedy} {what}, beam {n_beam} {what_beam}")
        assert n_beam == n_greedy and len(got) in (5, 30) and all("log_prob" in d for d in got)


def test_eval_detection_cli_with_beam_width(dev, det_model, rec_model, tmp_path):
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.checkpoint import save_checkpoint
    from PIL import Image

    det = oa.DetectionModel()
    det.load_state_dict(TL._golden_state("det"))
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    rec.load_state_dict(TL._golden_state("rec"))
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    save_checkpoint(str(tmp_path / "rec.pt"), rec, oa.optim.Adam(rec.parameters()), 0)
    page_h = TL.dot_page(800, 600)
    Image.fromarray(page_h[0].numpy()).save(tmp_path / "page.png")
    cmd = [sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), str(tmp_path / "out")]
    r = subprocess.run(cmd + ["--beam-width", "8"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--beam-width needs --rec-model" in r.stderr  # (argument parsing: no GPU work)
    r = subprocess.run(cmd + ["--rec-model", str(tmp_path / "rec.pt"), "--lines", "--chars", "--beam-width", "8"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert got and all(set(g) == {"quad", "text", "words", "char_quads", "char_log_probs", "word_chars", "word_texts", "log_prob"} for g in got)
    assert got == inf.ocr_lines(det_model, rec_model, page_h.to(dev), chars=True, beam_width=8)

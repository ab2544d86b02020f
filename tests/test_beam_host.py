"""CPU checks of the beam-search rule: the numpy restatement tests/beam_ref.py against brute force over every labelling and
against torch's CTC loss, the alignment restatement against an exhaustive path search, the share of cases the GPU tests will skip for
exactly their generators and seeds, the workspace size queries and the argument errors of the Python wrappers (none needs a GPU)."""
import math

import numpy as np
import pytest
import torch

from tests import beam_ref as B

NEW_SYMBOLS = ("ocrs_ctc_beam_ws_bytes", "ocrs_ctc_align_ws_bytes", "ocrs_ctc_beam_decode", "ocrs_ctc_align_spans")


@pytest.fixture(scope="module")
def exhaustive():
    """per exhaustive shape: the log-probs and, per case, the brute-force (labels, log-likelihood, gap): computed once"""
    return {(C, T, W): (lp, [B.best_labellings(x) for x in lp]) for C, T, W in B.EXHAUSTIVE_SHAPES for lp in [B.exhaustive_inputs(C, T)]}


def test_the_two_step_example():
    lp = np.log(np.array([[0.6, 0.4], [0.6, 0.4]]))
    assert B.greedy(lp, 2) == []
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-6)):
        r = B.beam_search(lp, 2, 4, dtype)
        assert r["labels"] == [1] and abs(r["score"] - math.log(0.64)) < tol
        assert abs(r["gap"] - (math.log(0.64) - math.log(0.36))) < 10 * tol
    assert B.beam_search(lp, 0, 4) == dict(labels=[], score=0.0, gap=float("inf"), prune_gap=float("inf"))
    assert B.beam_search(lp, 7, 4)["labels"] == [1]  # clamped to T


@pytest.mark.parametrize("shape", B.EXHAUSTIVE_SHAPES)
def test_beam_without_pruning_is_the_brute_force_argmax(exhaustive, shape):
    C, T, W = shape
    assert W >= sum((C - 1) ** n for n in range(T + 1))  # every prefix fits: nothing is ever pruned
    lp, brute = exhaustive[shape]
    skipped, worst32 = 0, 0.0
    for x, (labels, ll, gap) in zip(lp, brute):
        r = B.beam_search(x, T, W)
        assert r["prune_gap"] == float("inf")
        assert abs(r["score"] - B.ctc_log_likelihood(x, r["labels"])) < 1e-9  # the mass of what it returns, whatever it returns
        if gap < B.EXHAUSTIVE_MIN_GAP:
            skipped += 1
            continue
        assert r["labels"] == labels and abs(r["score"] - ll) < 1e-9
        r32 = B.beam_search(x, T, W, np.float32)
        assert r32["labels"] == labels
        worst32 = max(worst32, abs(r32["score"] - ll) / B.score_bound(T, ll))
    print(f"(C, T, W) = {shape}: skipped {skipped} of {len(lp)}; float32 restatement at most {worst32:.3f} of the score bound")
    assert skipped <= B.EXHAUSTIVE_MAX_SKIP * len(lp) and worst32 <= 1.0


def test_the_brute_force_scorer_is_torch_ctc_loss(exhaustive):
    for (C, T, W), (lp, brute) in exhaustive.items():
        x = torch.from_numpy(lp[:8].astype(np.float64)).permute(1, 0, 2).contiguous()  # (T, N, C)
        for labels in B.all_labellings(C, T)[:12]:
            tg = torch.tensor([list(labels)] * 8, dtype=torch.long).reshape(8, len(labels))
            loss = torch.nn.functional.ctc_loss(x, tg, torch.full((8,), T), torch.full((8,), len(labels)), reduction="none", zero_infinity=False)
            for n in range(8):
                ll = B.ctc_log_likelihood(lp[n], labels)
                assert (ll == -np.inf and loss[n].item() == np.inf) or abs(ll + loss[n].item()) < 1e-9, (C, T, labels, n)


@pytest.mark.parametrize("shape", B.PRUNED_SHAPES)
def test_pruned_regime_margins(shape):
    """what tests/test_beam_gpu.py will skip, and that float32 arithmetic decides nothing else: the same generator, seed and widths"""
    C, T, W, J = shape
    lp, in_len = B.peaky_inputs(C, T, J)
    skipped = differ = 0
    worst = 0.0
    for x, il in zip(lp, in_len):
        r = B.beam_search(x, il, W)
        assert r["score"] <= B.ctc_log_likelihood(x[:il], r["labels"]) + 1e-9  # pruning only ever loses mass
        if min(r["gap"], r["prune_gap"]) < B.PRUNED_MIN_MARGIN:
            skipped += 1
            continue
        r32 = B.beam_search(x, il, W, np.float32)
        assert r32["labels"] == r["labels"]
        worst = max(worst, abs(r32["score"] - r["score"]))
        differ += r["labels"] != B.greedy(x, il)
    print(f"(C, T, W) = {shape[:3]}: skipped {skipped} of {len(lp)}, beam != greedy in {differ}, float32 restatement off by at most {worst:.2e}")
    assert skipped <= B.PRUNED_MAX_SKIP * len(lp)
    assert worst <= B.score_bound(T, 1.0)


def test_beam_differs_from_greedy_somewhere():
    n = 0
    for C, T, W, J in B.PRUNED_SHAPES:
        lp, in_len = B.peaky_inputs(C, T, J)
        n += sum(B.beam_search(x, il, W)["labels"] != B.greedy(x, il) for x, il in zip(lp, in_len))
    assert n >= 1


def test_alignment_restatement_against_every_path():
    rng = np.random.default_rng(5)
    checked = infeasible = 0
    for T, C in ((1, 2), (2, 3), (3, 3), (4, 3), (5, 3), (6, 2), (6, 3)):
        lp = rng.standard_normal((T, C)) - 2.0
        ilp = rng.integers(-8, 1, size=(T, C)).astype(np.float64)  # integer values: ties
        for labels in B.all_labellings(C, min(T, 4)) + [tuple([1] * (T + 1))]:
            for x in (lp, ilp):
                want = B.best_path(x, labels)
                for dtype in (np.float64, np.float32):
                    r = B.align(x.astype(dtype), T, list(labels), dtype)
                    if want == -np.inf:
                        assert r == dict(lens=-1)
                        infeasible += 1
                        continue
                    assert r["lens"] == len(labels)
                    assert abs(r["score"] - want) < (1e-12 if dtype == np.float64 else 1e-5)
                    total, cls = B.path_score(x, labels, r["t0"], r["t1"])
                    assert abs(total - want) < (1e-12 if dtype == np.float64 or x is ilp else 1e-5)
                    assert [0 if s % 2 == 0 else labels[s >> 1] for s in r["states"]] == cls.tolist()
                    assert all(p == x.astype(dtype)[a:b + 1, l].max() for l, a, b, p in zip(labels, r["t0"], r["t1"], r["peak"]))
                    checked += 1
    assert checked > 300 and infeasible > 20
    assert B.align(np.zeros((2, 3)), 2, [1, 1]) == dict(lens=-1)  # no room for the blank between equal neighbours
    assert B.align(np.zeros((3, 3)), 3, [1, 1])["t0"] == [0, 2]
    assert B.align(np.zeros((3, 3)), 2, [1, 2, 1]) == dict(lens=-1)  # more labels than steps
    assert B.align(np.zeros((4, 3)), 4, [2])["states"] == [1, 2, 2, 2]  # ties: the final blank wins the end, staying wins every step
    assert B.align(np.zeros((4, 3)), 4, [])["lens"] == 0 and B.align(np.zeros((4, 3)), 0, [])["lens"] == 0


def test_abi_and_workspace_queries():
    from ocrs_models_amd._lib import ARG_NAMES, SIGNATURES, lib

    for name in NEW_SYMBOLS:
        assert name in SIGNATURES
    assert ARG_NAMES["ocrs_ctc_beam_decode"] == ["lp", "in_len", "T", "N", "C", "W", "row0", "ld", "labels", "lens", "score", "ws", "ws_bytes", "st"]
    assert ARG_NAMES["ocrs_ctc_align_spans"] == ["lp", "in_len", "T", "N", "C", "row0", "ld", "labels", "lens", "t0", "t1", "peak", "ws", "ws_bytes", "st"]
    header = open(__import__("ocrs_models_amd._lib", fromlist=["HEADER_PATH"]).HEADER_PATH).read()
    section = header[header.index("beam search -----"):header.index("layout model -----")]
    assert section.count("datasets/util.py:147-177") >= 3
    L = lib()  # loads without a GPU; the size queries are host code
    assert L.ctc_beam_ws_bytes(209, 256, 16) == 256 * (209 * 16 + 1) * 8
    assert L.ctc_beam_ws_bytes(1, 1, 1) == 16 and L.ctc_beam_ws_bytes(5, 3, 64) == 3 * 321 * 8
    assert L.ctc_beam_ws_bytes(0, 4, 8) == 0 and L.ctc_beam_ws_bytes(4, 0, 8) == 0 and L.ctc_beam_ws_bytes(4, 4, 0) == 0 and L.ctc_beam_ws_bytes(4, 4, 65) == 0
    assert L.ctc_align_ws_bytes(209, 256, 209) == 256 * 209 * 7 * 16  # 419 states: seven rounds of 64
    assert L.ctc_align_ws_bytes(209, 256, 5000) == L.ctc_align_ws_bytes(209, 256, 209)  # no labelling longer than T can align
    assert L.ctc_align_ws_bytes(70, 2, 31) == 2 * 70 * 16 and L.ctc_align_ws_bytes(70, 2, 32) == 2 * 70 * 2 * 16 and L.ctc_align_ws_bytes(70, 2, 0) == 2 * 70 * 16
    assert L.ctc_align_ws_bytes(0, 2, 3) == 0 and L.ctc_align_ws_bytes(3, 0, 3) == 0 and L.ctc_align_ws_bytes(3, 2, -1) == 0


def test_wrapper_argument_errors_need_no_gpu():
    import inspect

    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text

    lp = torch.zeros(5, 2, 4)
    for bad in (0, 65, -1, 2.0, None, True):
        with pytest.raises(RuntimeError, match="beam_width"):
            text.beam_decode_spans_async(lp, [5, 5], bad)
    with pytest.raises(RuntimeError, match="on the GPU"):
        text.beam_decode_spans(lp, [5, 5], 4)
    with pytest.raises(RuntimeError, match="on the GPU"):
        text.beam_decode_spans(lp[0], [5, 5], 4)
    with pytest.raises(RuntimeError, match="classes"):
        text.beam_decode_spans(torch.zeros(5, 2, 1), [5, 5], 4)
    with pytest.raises(RuntimeError, match="classes"):
        text.beam_decode_spans(torch.zeros(5, 2, 257), [5, 5], 4)
    with pytest.raises(RuntimeError, match="on the GPU"):
        text.ctc_align_spans(lp, [5, 5], [[1], [2]], [1, 1])
    for f in (inf.decode_crop_spans, inf.recognize_crops, inf.read_lines, inf.ocr_page, inf.ocr_lines, inf.ocr_pages, inf._read_crops):
        assert inspect.signature(f).parameters["beam_width"].default is None
    assert inf.CharSpans(*[None] * 6).scores is None

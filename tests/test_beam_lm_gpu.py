"""CTC prefix beam search with a character n-gram language model fused into the ranking, on the GPU (the LM form of k_ctc_beam in
csrc/ctc_beam.hip, ``ocrs_ctc_beam_decode_lm``; ``lm=`` of text.beam_decode_spans and of the page drivers) against the numpy restatement of
DESIGN.md §19 (tests/beam_lm_ref.py, pinned by tests/test_beam_lm_host.py).

Exhaustive regime.  The shapes of tests/beam_ref.py at which nothing is pruned, tables of orders 1 to 3: the labels are the brute-force
arg-max of log-likelihood + gains over every labelling (a case whose two best are closer than 1e-4 is skipped, at most 5 %).

Pruned regime.  The peaky inputs of tests/beam_ref.py with ``random_gain`` tables; the float64 restatement supplies the margins of the
RANKS (final top-1 / top-2, and best surviving prefix of the answer against the first pruned candidate); a case with either below 1e-3 is
skipped, at most 10 % (the host test asserts both caps for the same inputs).  Otherwise labels equal float64's.

Bounds.  |score - score64| <= beam_ref.score_bound(T, score64): the CTC numbers are those of the plain beam.  |lm_score - lm64| <= L 2^-24
max(1, sum |g_k|): L fp32 adds at a running magnitude of at most sum |g_k|, float64 summing the same float32 entries.  The tests print the
worst share of each bound (DESIGN.md §19 records them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beam_lm_ref as R
from tests import beam_ref as B
from tests import test_beam_gpu as BG
from tests import test_chars_gpu as CG
from tests import test_lines_gpu as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = BG.SENT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rec_model(dev):
    import ocrs_models_amd as oa

    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    m.load_state_dict(TL._golden_state("rec"))
    return m.to(dev).eval()


def _gain(dev, table):
    from ocrs_models_amd import text

    return text.LMGain(table, dev)


def _beam_lm(dev, lp_ntc, in_len, W, gain, row0=0, rows=None, ld=None):
    """one beam_decode_spans_async call with ``lm`` on (N,T,C) host log-probs into sentinel-filled arrays -> the arrays on the host, the
    scores and the lm scores; ``gain`` a numpy table, or None for the plain beam (lm scores None)"""
    from ocrs_models_amd import text

    N, T, C = lp_ntc.shape
    rows, ld = N + row0 if rows is None else rows, T if ld is None else ld
    lp = torch.from_numpy(np.ascontiguousarray(np.transpose(lp_ntc, (1, 0, 2)))).to(dev)
    out = text.span_arrays(rows, ld, dev)
    out[0].fill_(SENT)
    scores = torch.full((rows,), float(SENT), dtype=torch.float32, device=dev)
    lms = None if gain is None else torch.full((rows,), float(SENT), dtype=torch.float32, device=dev)
    lm = None if gain is None else _gain(dev, gain)
    assert text.beam_decode_spans_async(lp, [int(v) for v in in_len], W, out, row0, scores, lm=lm, lm_scores=lms) is None
    return BG._split(out[0].cpu().numpy(), rows, ld), scores.cpu().numpy(), None if lms is None else lms.cpu().numpy()


def _untouched(a, sc, lms, row0, N):
    BG._untouched(a, sc, row0, N)
    outside = [i for i in range(len(sc)) if not row0 <= i < row0 + N]
    assert (lms[outside] == SENT).all()


def _share(err, bound):
    """err as a share of bound; an empty labelling's lm_score has the bound 0 and must be exact"""
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


def _labels(a, row):
    return a["labels"][row, :max(int(a["lens"][row]), 0)].tolist()


# ------------------------------------------------------------------ exhaustive regime -------------------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("shape", B.EXHAUSTIVE_SHAPES)
def test_unpruned_beam_is_the_brute_force_argmax_of_likelihood_plus_gains(dev, shape, order):
    C, T, W = shape
    lp, gain = B.exhaustive_inputs(C, T), R.random_gain(C, order)
    a, sc, lms = _beam_lm(dev, lp, [T] * len(lp), W, gain)
    skipped, worst, worst_lm = 0, 0.0, 0.0
    for n, (x, (labels, value, gap, ll)) in enumerate(zip(lp, R.best_labellings_lm(C, T, gain))):
        if gap < B.EXHAUSTIVE_MIN_GAP:
            skipped += 1
            continue
        assert _labels(a, n) == labels, n
        worst = max(worst, abs(sc[n] - ll) / B.score_bound(T, ll))
        worst_lm = max(worst_lm, _share(abs(lms[n] - R.lm_sum(labels, gain)), R.lm_bound(labels, gain)))
        BG._spans_are_a_path(a, n, x, T)
    print(f"(C, T, W) = {shape}, order {order}: skipped {skipped} of {len(lp)}; score at {worst:.3f} of its bound, lm_score at {worst_lm:.3f}")
    assert skipped <= B.EXHAUSTIVE_MAX_SKIP * len(lp)
    assert worst <= 1.0 and worst_lm <= 1.0
    _untouched(a, sc, lms, 0, len(lp))


# ------------------------------------------------------------------ pruned regime -----------------------------------------------------------
@pytest.fixture(scope="module")
def pruned(dev):
    """every pruned shape and order once: the GPU's answer next to the cached float64 restatement (the second shape at row0 = 3 of a larger,
    wider buffer)"""
    out = {}
    for k, (C, T, W, J) in enumerate(B.PRUNED_SHAPES):
        for order in R.ORDERS:
            lp, in_len, gain, ref = R.pruned_reference(k, order)
            row0 = 3 if k == 1 else 0
            got = _beam_lm(dev, lp, in_len, W, gain, row0=row0, rows=len(lp) + row0 + 2, ld=T + (5 if k == 1 else 0))
            out[(k, order)] = (lp, in_len, gain, ref, row0, *got)
    return out


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("k", range(len(B.PRUNED_SHAPES)))
def test_pruned_beam_equals_the_float64_restatement(pruned, k, order):
    C, T, W, _ = B.PRUNED_SHAPES[k]
    lp, in_len, gain, ref, row0, a, sc, lms = pruned[(k, order)]
    skipped, worst, worst_lm = 0, 0.0, 0.0
    for n, (x, il, r) in enumerate(zip(lp, in_len, ref)):
        row = row0 + n
        lab = a["labels"][row, :a["lens"][row]]
        assert 0 <= a["lens"][row] <= il and ((lab >= 1) & (lab < C)).all()
        if min(r["gap"], r["prune_gap"]) < B.PRUNED_MIN_MARGIN:
            skipped += 1
            continue
        assert lab.tolist() == r["labels"], n
        worst = max(worst, abs(sc[row] - r["score"]) / B.score_bound(T, r["score"]))
        worst_lm = max(worst_lm, _share(abs(lms[row] - r["lm_score"]), R.lm_bound(r["labels"], gain)))
        BG._spans_are_a_path(a, row, x, il)
    print(f"(C, T, W) = {(C, T, W)}, order {order}: skipped {skipped} of {len(lp)}; score at {worst:.3f} of its bound, lm_score at {worst_lm:.3f}")
    assert skipped <= B.PRUNED_MAX_SKIP * len(lp)
    assert worst <= 1.0 and worst_lm <= 1.0
    _untouched(a, sc, lms, row0, len(lp))


def test_the_table_changes_the_plain_beams_answer(pruned):
    for k in range(len(B.PRUNED_SHAPES)):
        plain = R.plain_reference(k)
        for order in R.ORDERS:
            lp, in_len, gain, ref, row0, a, sc, lms = pruned[(k, order)]
            assert sum(_labels(a, row0 + n) != p["labels"] for n, p in enumerate(plain)) >= 1


# ------------------------------------------------------------------ a table of zeros --------------------------------------------------------
def test_a_table_of_zeros_gives_the_plain_beams_bytes(dev):
    C, T, W, J = B.PRUNED_SHAPES[1]
    assert (C, T, W) == (97, 40, 16)
    lp, in_len = B.peaky_inputs(C, T, J)
    a, sc, _ = _beam_lm(dev, lp, in_len, W, None, row0=1, rows=len(lp) + 2)
    for order in R.ORDERS:
        b, sd, lms = _beam_lm(dev, lp, in_len, W, np.zeros((C,) * order, dtype=np.float32), row0=1, rows=len(lp) + 2)
        assert all(a[key].tobytes() == b[key].tobytes() for key in a) and sc.tobytes() == sd.tobytes()
        assert (lms[1:-1] == 0.0).all() and not np.signbit(lms[1:-1]).any()
        _untouched(b, sd, lms, 1, len(lp))


# ------------------------------------------------------------------ edges -------------------------------------------------------------------
def _against_ref(a, sc, lms, lp, in_len, W, gain, row0=0):
    """labels equal the float64 restatement wherever its margins allow, the scores stay within their bounds -> cases compared"""
    T, compared = lp.shape[1], 0
    for n, (x, il) in enumerate(zip(lp, in_len)):
        r, row = R.beam_search_lm(x, il, W, gain), row0 + n
        assert not np.isnan(sc[row]) and not np.isnan(lms[row]) and not np.isnan(a["peak"][row, :max(a["lens"][row], 0)]).any()
        if min(r["gap"], r["prune_gap"]) >= B.PRUNED_MIN_MARGIN:
            assert _labels(a, row) == r["labels"], n
            assert (sc[row] == r["score"]) if np.isinf(r["score"]) else abs(sc[row] - r["score"]) <= B.score_bound(T, r["score"]), n
            assert abs(lms[row] - r["lm_score"]) <= R.lm_bound(r["labels"], gain), n
            compared += 1
    return compared


def test_input_lengths_and_class_counts(dev):
    T = 9
    for C, W, order in ((2, 1, 2), (2, 64, 2), (256, 5, 2), (6, 1, 1), (6, 5, 3), (6, 64, 2)):
        lp, _ = B.peaky_inputs(C, T, 8.0, seed=3, cases=5)
        gain = R.random_gain(C, order, seed=4)
        in_len = [0, 1, T - 1, T, T + 5]
        a, sc, lms = _beam_lm(dev, lp, in_len, W, gain, row0=1, rows=8, ld=T + 2)
        assert a["lens"][1] == 0 and sc[1] == 0.0 and lms[1] == 0.0  # in_len 0: the empty labelling at score 0, lm_score 0
        assert a["lens"][2] <= 1
        assert _against_ref(a, sc, lms, lp, in_len, W, gain, row0=1) >= 3
        _untouched(a, sc, lms, 1, 5)
        for n in range(5):
            BG._spans_are_a_path(a, 1 + n, lp[n], in_len[n])


def test_forbidden_transitions(dev):
    C, T = 5, 12
    rng = np.random.default_rng(12)
    lp = B.log_softmax(rng.standard_normal((4, T, C))).astype(np.float32)
    path = np.array([1, 1, 0, 2, 2, 0, 1, 0, 2, 0, 3, 3])
    lp[1] = -9.0
    lp[1, np.arange(T), path] = -0.01  # says 1 2 1 2 3 loudly
    lp[2, :, 0] = -np.inf               # never the blank: with every label forbidden nothing survives step 0
    lp[3, 4, 0] = -np.inf               # one step without the blank: with every label forbidden nothing survives it
    for W in (1, 4, 64):
        # (a) one entry at -inf: the transition 1 -> 2 never appears in the answer
        g = R.random_gain(C, 2, seed=5)
        g[1, 2] = -np.inf
        a, sc, lms = _beam_lm(dev, lp[:2], [T, T], W, g)
        assert B.beam_search(lp[1], T, W)["labels"] == [1, 2, 1, 2, 3]
        for n in range(2):
            lab = _labels(a, n)
            assert all((x, y) != (1, 2) for x, y in zip(lab, lab[1:])) and np.isfinite(lms[n]) and np.isfinite(sc[n])
        assert _against_ref(a, sc, lms, lp[:2], [T, T], W, g) >= 1
        # (b) the same through a trigram: 2 after (0, 1) only, so the second "1 2" may stay
        g3 = np.zeros((C,) * 3, dtype=np.float32)
        g3[0, 1, 2] = -np.inf
        a, sc, lms = _beam_lm(dev, lp[:2], [T, T], W, g3)
        assert _labels(a, 1)[:2] != [1, 2] and lms[1] == 0.0
        assert _against_ref(a, sc, lms, lp[:2], [T, T], W, g3) >= 1
        # (c) whole rows at -inf: no label may ever be appended
        for order in R.ORDERS:
            g = np.full((C,) * order, -np.inf, dtype=np.float32)
            a, sc, lms = _beam_lm(dev, lp, [T] * 4, W, g)
            assert not np.isnan(sc).any() and not np.isnan(lms).any()
            assert [_labels(a, n) for n in range(4)] == [[]] * 4 and (lms == 0.0).all()
            assert np.isfinite(sc[0]) and abs(sc[0] - lp[0, :, 0].astype(np.float64).sum()) <= B.score_bound(T, sc[0])  # the all-blank path alone
            assert sc[2] == -np.inf and sc[3] == -np.inf and a["lens"][2] == -1 and a["lens"][3] == -1  # nothing survived
            assert a["lens"][0] == 0 and a["lens"][1] == 0
            _untouched(a, sc, lms, 0, 4)
        # (d) only the start-of-line row at -inf (order 2): the same, since no first label exists
        g = np.zeros((C, C), dtype=np.float32)
        g[0, :] = -np.inf
        a, sc, lms = _beam_lm(dev, lp, [T] * 4, W, g)
        assert [_labels(a, n) for n in range(4)] == [[]] * 4 and sc[2] == -np.inf and not np.isnan(sc).any()


@pytest.mark.parametrize("W", [1, 3, 64])
def test_equal_ranks_keep_the_candidate_order(dev, W):
    """integer-valued log-probs and gains, so that ranks are exact and tie exactly: slot ascending, stay before extend, label ascending"""
    C = 5
    lp = np.full((4, 2, C), -1.0, dtype=np.float32)
    lp[2:, 1, 0] = -np.inf  # samples 2 and 3, step 1: no blank, so every stay is its prefix's repeat alone and every number is an integer
    uni = np.array([-np.inf, 0.0, 1.0, 1.0, 0.0], dtype=np.float32)  # labels 2 and 3 tie above the rest
    zero = np.zeros(C, dtype=np.float32)                              # everything ties: the stay comes first
    a, sc, lms = _beam_lm(dev, lp, [1, 1, 2, 2], W, uni)
    assert [_labels(a, n) for n in range(4)] == [[2], [2], [2, 3], [2, 3]]  # [2 3] and [3 2] tie at rank 0: [2] is the lower slot
    assert sc.tolist() == [-1.0, -1.0, -2.0, -2.0] and lms.tolist() == [1.0, 1.0, 2.0, 2.0]
    b, sd, lmz = _beam_lm(dev, lp[:2], [1, 1], W, zero)
    assert [_labels(b, n) for n in range(2)] == [[], []] and sd.tolist() == [-1.0, -1.0] and lmz.tolist() == [0.0, 0.0]
    bi = np.zeros((C, C), dtype=np.float32)
    bi[0, 1:] = [0.0, 2.0, 2.0, 1.0]  # first label: 2 or 3
    bi[2, 4] = bi[3, 1] = 3.0         # then [2 4] and [3 1] tie: slot order decides, not the label
    a, sc, lms = _beam_lm(dev, lp[2:], [2, 2], W, bi)
    assert [_labels(a, n) for n in range(2)] == [[2, 4], [2, 4]] and sc.tolist() == [-2.0, -2.0] and lms.tolist() == [5.0, 5.0]
    for n, (x, il, g) in enumerate(((lp[0], 1, uni), (lp[2], 2, uni), (lp[2], 2, bi), (lp[0], 1, zero))):
        for dtype in (np.float64, np.float32):
            r = R.beam_search_lm(x, il, W, g, dtype)
            assert r["labels"] == [[2], [2, 3], [2, 4], []][n] and r["score"] == [-1.0, -2.0, -2.0, -1.0][n] and r["lm_score"] == [1.0, 2.0, 5.0, 0.0][n]


@pytest.mark.parametrize("N", [1, 70])
def test_batch_sizes_widths_and_equal_bytes(dev, N):
    from ocrs_models_amd import text

    C, T = 17, 30
    lp, in_len = B.peaky_inputs(C, T, 10.0, seed=7, cases=N)
    gain = R.random_gain(C, 3, seed=8)
    for W in (1, 64):
        a, sc, lms = _beam_lm(dev, lp, in_len, W, gain, row0=2, rows=N + 4, ld=T + 1)
        b, sd, lmt = _beam_lm(dev, lp, in_len, W, gain, row0=2, rows=N + 4, ld=T + 1)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a) and sc.tobytes() == sd.tobytes() and lms.tobytes() == lmt.tobytes()
        _untouched(a, sc, lms, 2, N)
        if N == 1 or W == 1:
            assert _against_ref(a, sc, lms, lp[:8], in_len[:8], W, gain, row0=2) >= 1
    # arrays of its own: the same values through the handle
    x = torch.from_numpy(np.ascontiguousarray(lp.transpose(1, 0, 2))).to(dev)
    res = text.beam_decode_spans(x, in_len.tolist(), 64, lm=_gain(dev, gain))
    for n, r in enumerate(res):
        k = a["lens"][2 + n]
        assert set(r) == {"labels", "t0", "t1", "peak", "score", "lm_score"} and r["score"] == sc[2 + n] and r["lm_score"] == lms[2 + n]
        assert r["labels"] == a["labels"][2 + n, :k].tolist() and r["t0"] == a["t0"][2 + n, :k].tolist() and r["t1"] == a["t1"][2 + n, :k].tolist()
    assert all(set(r) == {"labels", "t0", "t1", "peak", "score"} for r in text.beam_decode_spans(x, in_len.tolist(), 64, lm=None))


def test_refused_orders_tables_and_class_counts(dev):
    from ocrs_models_amd import text
    from ocrs_models_amd._lib import lib, ptr

    T, N, C = 4, 2, 4
    lp = torch.zeros(T, N, C, device=dev)
    il = torch.full((N,), T, dtype=torch.int64, device=dev)
    out = text.span_arrays(N, T, dev)
    out[0].fill_(SENT)
    sc = torch.full((N,), float(SENT), device=dev)
    lms = torch.full((N,), float(SENT), device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    table = torch.zeros(C ** 3, device=dev)

    def call(W=4, gain=table, order=2, lm_score=lms, ws_bytes=ws.numel(), classes=C):
        lib().ctc_beam_decode_lm(ptr(lp), ptr(il), T, N, classes, W, ptr(gain), order, 0, T, ptr(out[1]), ptr(out[5]), ptr(sc), ptr(lm_score), ptr(ws), ws_bytes)

    for kw in (dict(order=0), dict(order=4), dict(order=-1), dict(gain=None), dict(lm_score=None), dict(W=0), dict(W=65), dict(classes=1), dict(classes=257),
               dict(ws_bytes=8)):
        with pytest.raises(RuntimeError, match="bad argument"):
            call(**kw)
    torch.cuda.synchronize()
    assert (out[0] == SENT).all() and (sc == SENT).all() and (lms == SENT).all()  # nothing was launched
    good = text.LMGain(np.zeros((C, C), dtype=np.float32), dev)
    with pytest.raises(RuntimeError, match="5 classes, the log-probs 4"):
        text.beam_decode_spans(lp, il, 4, lm=text.LMGain(np.zeros((5, 5), dtype=np.float32), dev))
    with pytest.raises(RuntimeError, match="is on cpu"):
        text.beam_decode_spans(lp, il, 4, lm=text.LMGain(np.zeros((C, C), dtype=np.float32), "cpu"))
    with pytest.raises(RuntimeError, match="lm_scores"):
        text.beam_decode_spans_async(lp, il, 4, text.span_arrays(N, T, dev), 0, sc, lm=good, lm_scores=None)
    with pytest.raises(RuntimeError, match="lm_scores"):
        text.beam_decode_spans_async(lp, il, 4, text.span_arrays(N, T, dev), 0, sc, lm=good, lm_scores=torch.zeros(N + 1, device=dev))
    call()  # and the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert (lms == 0.0).all() and (out[5] >= 0).all() and (sc != SENT).all()  # this one ran: a table of zeros gives lm_score 0


# ------------------------------------------------------------------ end to end: painted detector, stub recogniser ----------------------------
def _reference_rows(stub, batches, W, gain):
    """what the restatement reads from the stub's log-probs for every crop, in quad order: (text, score, lm score, margin, steps, labels);
    ``gain`` None: the plain beam"""
    from ocrs_models_amd.text import DEFAULT_ALPHABET, decode_text

    rows = []
    for img, iw in zip(batches[0], batches[1]):
        lp = stub(torch.zeros(1, 1, 64, img.shape[-1]))[:, 0].numpy()
        for w in iw.tolist():
            r = B.beam_search(lp, w // 4, W) if gain is None else R.beam_search_lm(lp, w // 4, W, gain)
            rows.append((decode_text(r["labels"], list(DEFAULT_ALPHABET)), r["score"], r.get("lm_score"), min(r["gap"], r["prune_gap"]), max(w // 4, 1),
                         r["labels"]))
    return [rows[p] for p in batches[2]]


def test_prescribed_log_probs_where_the_language_model_decides(dev):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    rows, cols, W = 4, 3, 8
    bars = [(15 + 52 * c, 18 + 40 * r, 40, 12) for r in range(rows) for c in range(cols)]
    page, det = TL.bar_page(190, 200, bars, dev)
    size = (190, 200)
    found = inf.detect_words(det, page, size=size)
    lines = inf.find_lines(found["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    T = int(plan.table.cpu().numpy()[0, 2]) // 4
    # five characters everyone agrees on, then three steps on which "l" is a little louder than "1": the recogniser alone reads "ab cdl", a
    # model that has only ever seen "ab cd1" reads "ab cd1"
    steps = [3 + 5 * k for k in range(6)]
    assert steps[-1] + 8 < T
    idx = {ch: DEFAULT_ALPHABET.index(ch) + 1 for ch in "ab cdl1"}
    chars = [(t - 1, t + 1, idx[ch], -(k + 1) / 64) for k, (ch, t) in enumerate(zip("ab cd", steps))]
    t_last = steps[-1]
    stub = CG.Stub(chars + [(t_last - 1, t_last + 1, idx["l"], -0.0625), (t_last - 1, t_last + 1, idx["1"], -0.125)], len(DEFAULT_ALPHABET) + 1).eval()
    model = text.CharLM.from_texts(["ab cd1"] * 3 + ["ab", "cd1"], order=3)
    lm = model.gain(1.0, 0.0, device=dev)
    assert lm is model.gain(1.0, 0.0, device=dev) and lm.C == len(DEFAULT_ALPHABET) + 1 and lm.order == 3
    table = lm.table.cpu().numpy()

    def staged(quads, gain, count=None):
        p = inf.crop_plan(quads, count=count)
        return _reference_rows(stub, inf.crops_to_batches(inf.rectify_crops(page, quads, p), p), W, gain)

    ref_lines, ref_words = staged(lines.quads, table, lines.n_lines), staged(found["quads"], table)
    plain_lines = staged(lines.quads, None, lines.n_lines)
    assert all(r[0] == "ab cd1" and r[3] > 1e-3 for r in ref_lines) and all(r[3] > 1e-3 for r in ref_words)
    assert all(r[0] == "ab cdl" and r[3] > 1e-3 for r in plain_lines)

    def check(got, ref, keys):
        assert len(got) == len(ref)
        for g, (txt, score, lm_score, _, steps_, labels) in zip(got, ref):
            assert set(g) == keys and g["text"] == txt and abs(g["log_prob"] - score) <= B.score_bound(steps_, score)
            assert abs(g["lm_score"] - lm_score) <= R.lm_bound(labels, table)

    line_keys = {"quad", "text", "words", "log_prob", "lm_score"}
    char_keys = {"char_quads", "char_log_probs"}
    kw = dict(size=size, beam_width=W)
    beam = inf.ocr_lines(det, stub, page, **kw)
    assert [b["text"] for b in beam] == ["ab cdl"] * rows and all("lm_score" not in b for b in beam)
    assert inf.ocr_lines(det, stub, page, lm=None, **kw) == beam  # lm=None is omitting the keyword
    assert inf.ocr_lines(det, stub, page, chars=True, lm=None, **kw) == inf.ocr_lines(det, stub, page, chars=True, **kw)
    assert inf.ocr_page(det, stub, page, lm=None, **kw) == inf.ocr_page(det, stub, page, **kw)
    assert inf.ocr_pages(det, stub, [page], lm=None, **kw) == [beam]
    plain = inf.ocr_lines(det, stub, page, lm=lm, **kw)
    check(plain, ref_lines, line_keys)
    assert [{k: v for k, v in p.items() if k not in ("log_prob", "lm_score", "text")} for p in plain] == \
        [{k: v for k, v in b.items() if k not in ("log_prob", "text")} for b in beam]  # everything but the decode is unchanged
    full = inf.ocr_lines(det, stub, page, chars=True, lm=lm, **kw)
    check(full, ref_lines, line_keys | char_keys | {"word_chars", "word_texts"})
    for g, p in zip(full, plain):
        assert {k: g[k] for k in p} == p
        assert len(g["char_quads"]) == len(g["char_log_probs"]) == len(g["text"]) == 6
        assert g["char_log_probs"][:5] == [c[3] for c in chars] and g["char_log_probs"][5] == -0.125  # the spans are those of the LM's answer: "1"
        assert [g["text"][s:e] for s, e in g["word_chars"]] == g["word_texts"] and len(g["word_chars"]) == len(g["words"]) == cols
        xs = [np.mean([pt[0] for pt in q]) for q in g["char_quads"]]
        assert all(b > a for a, b in zip(xs, xs[1:]))  # left to right along the line
    words = inf.ocr_page(det, stub, page, lm=lm, **kw)
    check(words, ref_words, {"quad", "text", "log_prob", "lm_score"})
    wchars = inf.ocr_page(det, stub, page, chars=True, lm=lm, **kw)
    check(wchars, ref_words, {"quad", "text", "log_prob", "lm_score"} | char_keys)
    assert all(len(w["char_quads"]) == len(w["text"]) == len(w["char_log_probs"]) for w in wchars)
    assert inf.ocr_pages(det, stub, [page], lm=lm, **kw) == [plain]
    assert inf.ocr_pages(det, stub, [page], chars=True, lm=lm, **kw) == [full]
    assert inf.ocr_pages(det, stub, [page], lines=False, lm=lm, **kw) == [words]
    assert inf.ocr_pages(det, stub, [page], lines=False, chars=True, lm=lm, **kw) == [wchars]
    # the spans form a path of the LM's labelling on the stub's log-probs
    p = inf.crop_plan(lines.quads, count=lines.n_lines)
    batches = inf.crops_to_batches(inf.rectify_crops(page, lines.quads, p), p)
    texts, spans, scores, lm_scores = inf.recognize_crops(stub, batches, chars=True, beam_width=W, lm=lm)
    assert (texts, scores, lm_scores) == inf.recognize_crops(stub, batches, beam_width=W, lm=lm) and texts == [g["text"] for g in plain]
    assert spans.lm_scores is not None and inf.decode_crop_spans(stub, batches, W).lm_scores is None
    a = BG._split(spans.buf.cpu().numpy(), *spans.labels.shape)
    row = 0
    for img, iw in zip(batches[0], batches[1]):
        x = stub(torch.zeros(1, 1, 64, img.shape[-1]))[:, 0].numpy()
        for w in iw.tolist():
            BG._spans_are_a_path(a, row, x, w // 4)
            row += 1
    with pytest.raises(RuntimeError, match="lm needs beam_width"):
        inf.ocr_lines(det, stub, page, size=size, lm=lm)


def test_the_language_model_adds_no_host_wait(dev, rec_model):
    """the lm scores are copied with the span buffer and the scores: the waits of a page stay what they are for the plain beam"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text

    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)]
    page, det = TL.bar_page(230, 340, bars, dev)
    lm = text.CharLM.from_texts(["The quick brown fox", "jumps over the lazy dog 0123"], order=3).gain(0.5, 0.25, device=dev)
    kw = dict(size=(230, 340), beam_width=8)
    calls = {
        "lines": lambda **k: inf.ocr_lines(det, rec_model, page, **kw, **k),
        "lines+chars": lambda **k: inf.ocr_lines(det, rec_model, page, chars=True, **kw, **k),
        "words": lambda **k: inf.ocr_page(det, rec_model, page, **kw, **k),
        "words+chars": lambda **k: inf.ocr_page(det, rec_model, page, chars=True, **kw, **k),
        "pages": lambda **k: inf.ocr_pages(det, rec_model, [page], **kw, **k)[0],
    }
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        for f in calls.values():
            f(), f(lm=lm)
    for name, f in calls.items():
        _, n_beam, what = TL._count_waits(f)
        got, n_lm, what_lm = TL._count_waits(lambda: f(lm=lm))
        print(f"host waits of {name}: beam {n_beam} {what}, beam + lm {n_lm} {what_lm}")
        assert n_lm == n_beam and len(got) in (5, 30) and all("lm_score" in d and "log_prob" in d for d in got)


def test_eval_detection_cli_with_a_language_model(dev, rec_model, tmp_path):
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text
    from ocrs_models_amd.checkpoint import save_checkpoint
    from PIL import Image

    det = oa.DetectionModel()
    det.load_state_dict(TL._golden_state("det"))
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    rec.load_state_dict(TL._golden_state("rec"))
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    save_checkpoint(str(tmp_path / "rec.pt"), rec, oa.optim.Adam(rec.parameters()), 0)
    model = text.CharLM.from_texts(["The quick brown fox", "jumps over the lazy dog 0123"], order=2)
    model.save(str(tmp_path / "lm.npz"))
    page_h = TL.dot_page(800, 600)
    Image.fromarray(page_h[0].numpy()).save(tmp_path / "page.png")
    cmd = [sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), str(tmp_path / "out"), "--rec-model",
           str(tmp_path / "rec.pt"), "--lm", str(tmp_path / "lm.npz")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--lm needs --beam-width" in r.stderr  # (argument parsing: no GPU work)
    r = subprocess.run(cmd + ["--lines", "--beam-width", "8", "--lm-weight", "0.5", "--lm-bonus", "0.25"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert got and all(set(g) == {"quad", "text", "words", "log_prob", "lm_score"} for g in got)
    assert got == inf.ocr_lines(det.to(dev).eval(), rec_model, page_h.to(dev), beam_width=8, lm=text.CharLM.load(str(tmp_path / "lm.npz")).gain(0.5, 0.25, device=dev))

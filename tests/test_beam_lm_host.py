"""The rule of DESIGN.md §19 -- CTC prefix beam search ranked by log-mass + character n-gram gains -- on the host: the numpy restatement
(tests/beam_lm_ref.py) against tests/beam_ref.py, against brute force and on a hand example; the skipped-share caps of
tests/test_beam_lm_gpu.py for exactly its generator, seeds, widths and tables; ``text.CharLM`` (counting, interpolated Witten-Bell, save /
load, gain tables); the new ABI symbol and the wrappers' argument errors.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

from tests import beam_lm_ref as R
from tests import beam_ref as B


# ------------------------------------------------------------------ the restatement ---------------------------------------------------------
@pytest.mark.parametrize("k", range(len(B.PRUNED_SHAPES)))
def test_a_table_of_zeros_is_the_plain_beam(k):
    C, T, W, J = B.PRUNED_SHAPES[k]
    lp, in_len = B.peaky_inputs(C, T, J)
    for order in R.ORDERS:
        zero = np.zeros((C,) * order, dtype=np.float32)
        for dtype in (np.float64, np.float32):
            for x, il in list(zip(lp, in_len))[:40 if (order == 2 and dtype is np.float64) else 6]:
                a, b = B.beam_search(x, il, W, dtype), R.beam_search_lm(x, il, W, zero, dtype)
                assert a["labels"] == b["labels"] and a["score"] == b["score"] and b["lm_score"] == 0.0
                assert a["gap"] == b["gap"] and a["prune_gap"] == b["prune_gap"]


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("shape", B.EXHAUSTIVE_SHAPES)
def test_unpruned_beam_is_the_brute_force_argmax_of_likelihood_plus_gains(shape, order):
    C, T, W = shape
    assert W >= sum((C - 1) ** n for n in range(T + 1))  # every prefix fits: nothing is ever pruned
    lp, gain = B.exhaustive_inputs(C, T), R.random_gain(C, order)
    skipped = 0
    for x, (labels, value, gap, ll) in zip(lp, R.best_labellings_lm(C, T, gain)):
        if gap < B.EXHAUSTIVE_MIN_GAP:
            skipped += 1
            continue
        r = R.beam_search_lm(x, T, W, gain)
        assert r["labels"] == labels
        assert abs(r["score"] + r["lm_score"] - value) <= 1e-9
        assert abs(r["score"] - ll) <= 1e-9 and ll == B.ctc_log_likelihood(x, labels) and abs(r["lm_score"] - R.lm_sum(labels, gain)) <= 1e-12
    print(f"(C, T, W) = {shape}, order {order}: skipped {skipped} of {len(lp)}")
    assert skipped <= B.EXHAUSTIVE_MAX_SKIP * len(lp)


def test_a_hand_example_where_the_table_flips_the_answer():
    """two steps, labels 1 and 2: step 0 says 1 (0.55) or 2 (0.45), step 1 the blank.  The plain beam reads [1]; a bigram table that forbids
    1 at the start of a line, or merely prefers 2 by more than log(0.55 / 0.45), reads [2]; a unigram table that taxes every label reads []"""
    lp = np.log(np.array([[1e-9, 0.55, 0.45], [0.98, 0.01, 0.01]]))
    lp = lp - np.log(np.exp(lp).sum(axis=1, keepdims=True))
    assert B.beam_search(lp, 2, 4)["labels"] == [1]
    G = np.zeros((3, 3), dtype=np.float32)
    G[0, 1] = -np.inf
    r = R.beam_search_lm(lp, 2, 4, G)
    assert r["labels"] == [2] and r["lm_score"] == 0.0 and abs(r["score"] - B.ctc_log_likelihood(lp, [2])) < 1e-12
    G[0, 1], G[0, 2] = 0.0, 0.25  # log(0.55 / 0.45) = 0.2007
    r = R.beam_search_lm(lp, 2, 4, G)
    assert r["labels"] == [2] and r["lm_score"] == 0.25 and abs(r["gap"] - (0.25 - np.log(0.55 / 0.45))) < 1e-6
    G[0, 2] = 0.125
    assert R.beam_search_lm(lp, 2, 4, G)["labels"] == [1]
    r = R.beam_search_lm(lp, 2, 4, np.full(3, -30.0, dtype=np.float32))
    assert r["labels"] == [] and r["lm_score"] == 0.0
    # a trigram reads the label before the last: after [1, 2] label 1 is forbidden, after [2, 2] it is not
    G3 = np.zeros((3, 3, 3), dtype=np.float32)
    G3[1, 2, 1] = -np.inf
    x = np.log(np.array([[0.02, 0.96, 0.02], [0.02, 0.02, 0.96], [0.02, 0.9, 0.08]]))
    assert B.beam_search(x, 3, 8)["labels"] == [1, 2, 1]
    assert R.beam_search_lm(x, 3, 8, G3)["labels"] == [1, 2]
    assert R.gains_of([1, 2, 1], G3)[2] == -np.inf and R.gains_of([2, 2, 1], G3) == [0.0, 0.0, 0.0]
    # edges: no steps, and a table that forbids everything
    r = R.beam_search_lm(x, 0, 8, G3)
    assert (r["labels"], r["score"], r["lm_score"]) == ([], 0.0, 0.0)
    x[1, 0] = -np.inf  # step 1 cannot be the blank, and no label may be appended: nothing survives
    r = R.beam_search_lm(x[:, :2], 3, 8, np.full((2, 2), -np.inf, dtype=np.float32))
    assert (r["labels"], r["score"], r["lm_score"]) == ([], -np.inf, 0.0)


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("k", range(len(B.PRUNED_SHAPES)))
def test_pruned_regime_margins(k, order):
    """what tests/test_beam_lm_gpu.py will skip, and that float32 arithmetic decides nothing else: the same generator, seed, widths, tables"""
    lp, in_len, gain, ref = R.pruned_reference(k, order)
    ref32 = R.pruned_reference(k, order, "float32")[3]
    skipped = 0
    for r, r32 in zip(ref, ref32):
        if min(r["gap"], r["prune_gap"]) < B.PRUNED_MIN_MARGIN:
            skipped += 1
            continue
        assert r32["labels"] == r["labels"]
        assert abs(r32["score"] - r["score"]) <= B.score_bound(lp.shape[1], r["score"])
        assert abs(r32["lm_score"] - r["lm_score"]) <= R.lm_bound(r["labels"], gain)
        assert abs(r["lm_score"] - R.lm_sum(r["labels"], gain)) <= 1e-9
    changed = sum(r["labels"] != p["labels"] for r, p in zip(ref, R.plain_reference(k)))
    print(f"(C, T, W) = {B.PRUNED_SHAPES[k][:3]}, order {order}: skipped {skipped} of {len(ref)}; the table changes the answer in {changed}")
    assert skipped <= B.PRUNED_MAX_SKIP * len(ref)
    assert changed >= 1


def test_random_gain_is_as_specified():
    for C, order in ((5, 1), (12, 2), (97, 3)):
        g = R.random_gain(C, order)
        assert g.dtype == np.float32 and g.shape == (C,) * order and np.isneginf(g[..., 0]).all() and np.isfinite(g[..., 1:]).all()
        p = np.exp((g[..., 1:].astype(np.float64) - R.GAIN_BONUS) / R.GAIN_WEIGHT).sum(axis=-1)
        assert np.abs(p - 1.0).max() < 1e-5
        assert g.tobytes() == R.random_gain(C, order).tobytes()


# ------------------------------------------------------------------ CharLM ------------------------------------------------------------------
def test_witten_bell_on_a_corpus_counted_by_hand():
    from ocrs_models_amd import text

    m = text.CharLM.from_texts(["ab", "ab", "ac"], alphabet="abc", unknown_char="a", order=2)
    assert m.order == 2 and m.alphabet == "abc" and m.log_probs.shape == (4, 4) and m.log_probs.dtype == np.float32
    counts = text.CharLM.count([[1, 2], [1, 2], [1, 3]], [2, 2, 2], 4, 2)
    assert counts[0, 1] == 3 and counts[1, 2] == 2 and counts[1, 3] == 1 and counts.sum() == 6
    p = text.witten_bell(counts)
    a, b, c = 1, 2, 3
    uni = {a: 4 / 9, b: 3 / 9, c: 2 / 9}  # (n + 3 / 3) / (6 + 3): three distinct followers of the empty context
    assert abs(p[a, b] - (2 + 2 * 3 / 9) / 5) < 1e-15 and abs(p[a, c] - (1 + 2 * 2 / 9) / 5) < 1e-15 and abs(p[a, a] - (2 * 4 / 9) / 5) < 1e-15
    assert abs(p[0, a] - (3 + 1 * 4 / 9) / 4) < 1e-15  # the start of a line is a context like any other
    for x in (b, c):  # contexts never seen: the back-off itself
        assert [p[x, y] for y in (a, b, c)] == [text.witten_bell(counts.sum(axis=0))[y] for y in (a, b, c)]
        assert all(abs(p[x, y] - uni[y]) < 1e-15 for y in (a, b, c))
    assert (p[:, 0] == 0).all() and np.abs(p.sum(axis=1) - 1).max() <= 1e-12
    assert np.isneginf(m.log_probs[:, 0]).all() and m.log_probs[:, 1:].tobytes() == np.log(p[:, 1:]).astype(np.float32).tobytes()


@pytest.mark.parametrize("order", R.ORDERS)
def test_rows_sum_to_one_and_texts_equal_labels(order):
    from ocrs_models_amd import text

    rng = np.random.default_rng(order)
    alphabet = "abcdefg "
    texts = ["".join(alphabet[i] for i in rng.integers(0, 6, size=int(rng.integers(0, 12)))) for _ in range(60)] + ["", "g"]
    C = len(alphabet) + 1
    m = text.CharLM.from_texts(texts, alphabet=alphabet, order=order, unknown_char="a")
    rows = np.zeros((len(texts), 12), dtype=np.int64)
    for i, t in enumerate(texts):
        rows[i, :len(t)] = [alphabet.index(ch) + 1 for ch in t]
    lengths = [len(t) for t in texts]
    p = text.witten_bell(text.CharLM.count(rows, lengths, C, order))
    assert p.shape == (C,) * order and np.abs(p.sum(axis=-1) - 1).max() <= 1e-12 and (p[..., 0] == 0).all() and (p[..., 1:] > 0).all()
    m2 = text.CharLM.from_labels(torch.from_numpy(rows), torch.tensor(lengths), C, order)
    assert m2.log_probs.tobytes() == m.log_probs.tobytes() and m2.alphabet is None and m2.order == order
    assert m.log_probs.tobytes() == text.CharLM.from_texts(texts, alphabet=alphabet, order=order, unknown_char="a").log_probs.tobytes()
    if order > 1:  # a context that never has a follower (g ends its only line) backs off to the shorter context's row
        lower = text.witten_bell(text.CharLM.count(rows, lengths, C, order - 1))
        assert (p[..., 7, 7, :] == lower[..., 7, :]).all() if order == 3 else (p[7] == lower).all()


def test_empty_corpus_unknown_characters_and_refused_arguments():
    from ocrs_models_amd import text

    for order in R.ORDERS:
        m = text.CharLM.from_texts([], alphabet="abc", unknown_char="a", order=order)
        assert np.isneginf(m.log_probs[..., 0]).all() and (m.log_probs[..., 1:] == np.float32(np.log(1 / 3))).all()
    a = text.CharLM.from_texts(["a#b", "zz?"], alphabet="ab?", order=2)
    b = text.CharLM.from_texts(["a?b", "???"], alphabet="ab?", order=2)
    assert a.log_probs.tobytes() == b.log_probs.tobytes()
    assert a.log_probs.tobytes() != text.CharLM.from_texts(["ab", "?"], alphabet="ab?", order=2).log_probs.tobytes()
    d = text.CharLM.from_texts(["hello world"])
    assert d.order == 3 and d.alphabet == text.DEFAULT_ALPHABET and d.log_probs.shape == (len(text.DEFAULT_ALPHABET) + 1,) * 3
    for bad in (0, 4, 2.0, True):
        with pytest.raises(RuntimeError, match="order"):
            text.CharLM.from_texts(["ab"], alphabet="ab", unknown_char="a", order=bad)
    with pytest.raises(RuntimeError, match="labels"):
        text.CharLM.from_labels([[1, 4]], [2], 4, 2)
    with pytest.raises(RuntimeError, match="labels"):
        text.CharLM.from_labels([[1, 0, 2]], [3], 4, 2)
    text.CharLM.from_labels([[1, 0, 9]], [1], 4, 2)  # entries past a row's length are not read
    with pytest.raises(RuntimeError, match="alphabet"):
        text.CharLM(np.zeros((4, 4), dtype=np.float32), "ab")


def test_save_and_load_give_equal_bytes(tmp_path):
    from ocrs_models_amd import text

    for k, m in enumerate((text.CharLM.from_texts(["ab€", "ba"], alphabet="ab€ ", unknown_char="a", order=3), text.CharLM.from_labels([[1, 2, 3]], [3], 5, 1))):
        path = str(tmp_path / f"lm{k}.npz")
        m.save(path)
        got = text.CharLM.load(path)
        assert got.log_probs.tobytes() == m.log_probs.tobytes() and got.log_probs.dtype == np.float32
        assert got.alphabet == m.alphabet and got.order == m.order
        with np.load(path) as z:
            assert sorted(z.files) == ["alphabet", "log_probs", "order"]


def test_gain_arithmetic_cache_and_refusals():
    from ocrs_models_amd import text

    m = text.CharLM.from_texts(["abab", "ba"], alphabet="ab", unknown_char="a", order=2)
    for w, b in ((1.0, 0.0), (0.7, 0.5), (0.0, 1.25), (2.5, -0.125)):
        g = m.gain(w, b, device="cpu")
        assert isinstance(g, text.LMGain) and g.order == 2 and g.C == 3 and g.table.dtype == torch.float32 and g.table.is_contiguous()
        want = (w * m.log_probs[:, 1:].astype(np.float64) + b).astype(np.float32)
        assert g.table.numpy()[:, 1:].tobytes() == want.tobytes() and np.isneginf(g.table.numpy()[:, 0]).all()
        assert m.gain(w, b, device="cpu") is g
    assert m.gain(1.0, 0.0, device="cpu") is not m.gain(1.0, 0.5, device="cpu")
    forbidding = text.CharLM(np.array([[-np.inf, 0.0, -np.inf]] * 3, dtype=np.float32), "ab")  # label 2 never follows anything
    assert np.isneginf(forbidding.gain(1.0, 0.0, device="cpu").table.numpy()[:, 2]).all()
    with pytest.raises(RuntimeError, match="NaN"):
        forbidding.gain(0.0, 0.0, device="cpu")   # 0 * -inf
    with pytest.raises(RuntimeError, match="inf"):
        forbidding.gain(-1.0, 0.0, device="cpu")  # -1 * -inf
    with pytest.raises(RuntimeError, match="NaN"):
        m.gain(float("nan"), 0.0, device="cpu")
    with pytest.raises(RuntimeError, match="inf"):
        m.gain(1.0, float("inf"), device="cpu")
    t = np.zeros((3, 3), dtype=np.float32)
    for bad in (np.nan, np.inf):
        t[1, 2] = bad
        with pytest.raises(RuntimeError, match="NaN or \\+inf"):
            text.LMGain(t, "cpu")
    t[1, 2] = -np.inf
    assert text.LMGain(t, "cpu").table[1, 2] == -np.inf
    for shape in ((3, 4), (3,) * 4, (1,), ()):
        with pytest.raises(RuntimeError, match="shape"):
            text.LMGain(np.zeros(shape, dtype=np.float32), "cpu")


def test_the_model_builder_reads_the_line_texts_without_a_gpu(tmp_path):
    """``python -m ocrs_models_amd.char_lm hiertext``'s main on a two-line lines file (an existing lines file is used as it is)"""
    import gzip
    import json

    from ocrs_models_amd import char_lm, text

    (tmp_path / "gt").mkdir()
    (tmp_path / "train").mkdir()
    with gzip.open(tmp_path / "gt" / "train.jsonl.gz", "wt") as f:
        f.write("{}\n")
    texts = ["Hello world", "Hello €5", "last"]
    with open(tmp_path / "gt" / "train-lines.jsonl", "w") as f:
        for t in texts:
            f.write(json.dumps({"image_id": "x", "vertices": [[0, 0], [9, 0], [9, 9], [0, 9]], "text": t}) + "\n")
    out = str(tmp_path / "lm.npz")
    char_lm.main(["hiertext", str(tmp_path), out, "--order", "2", "--max-images", "2"])
    got = text.CharLM.load(out)
    assert got.order == 2 and got.alphabet == text.DEFAULT_ALPHABET
    assert got.log_probs.tobytes() == text.CharLM.from_texts(texts[:2], order=2).log_probs.tobytes()
    with pytest.raises(SystemExit):
        char_lm.main(["hiertext", str(tmp_path), out, "--order", "4"])


# ------------------------------------------------------------------ ABI and wrappers --------------------------------------------------------
def test_abi_symbol():
    import ctypes

    from ocrs_models_amd._lib import ARG_NAMES, LIB_PATH, SIGNATURES, lib

    assert ARG_NAMES["ocrs_ctc_beam_decode_lm"] == ["lp", "in_len", "T", "N", "C", "W", "gain", "order", "row0", "ld", "labels", "lens", "score", "lm_score", "ws",
                                                    "ws_bytes", "st"]
    assert SIGNATURES["ocrs_ctc_beam_decode_lm"] == ("i", "ppiiiipilipppppls")
    assert hasattr(ctypes.CDLL(LIB_PATH), "ocrs_ctc_beam_decode_lm") and callable(lib().ctc_beam_decode_lm)
    # the argument checks are host code: error 1 before any launch (null pointers everywhere: nothing could run anyway)
    raw = lib()._raw_ocrs_ctc_beam_decode_lm
    for order in (0, 4, -1):
        assert raw(None, None, 4, 2, 4, 4, None, order, 0, 4, None, None, None, None, None, 0, None) == 1
    assert raw(None, None, 4, 2, 4, 4, None, 2, 0, 4, None, None, None, None, None, 0, None) == 1  # no table
    assert raw(None, None, 4, 0, 4, 65, None, 2, 0, 4, None, None, None, None, None, 0, None) == 1  # the width, even for no samples


def test_wrapper_argument_errors_need_no_gpu():
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text

    lp = torch.zeros(5, 2, 4)
    lm = text.LMGain(np.zeros((4, 4), dtype=np.float32), "cpu")
    with pytest.raises(RuntimeError, match="LMGain"):
        text.beam_decode_spans_async(lp, [5, 5], 4, lm=np.zeros((4, 4), dtype=np.float32))
    with pytest.raises(RuntimeError, match="LMGain"):
        text.beam_decode_spans(lp, [5, 5], 4, lm=text.CharLM.from_texts(["ab"], alphabet="abc", unknown_char="a"))
    with pytest.raises(RuntimeError, match="3 classes, the log-probs 4"):
        text.beam_decode_spans(lp, [5, 5], 4, lm=text.LMGain(np.zeros((3, 3), dtype=np.float32), "cpu"))
    with pytest.raises(RuntimeError, match="lm_scores without lm"):
        text.beam_decode_spans_async(lp, [5, 5], 4, lm_scores=torch.zeros(2))
    with pytest.raises(RuntimeError, match="beam_width"):
        text.beam_decode_spans(lp, [5, 5], 0, lm=lm)
    with pytest.raises(RuntimeError, match="on the GPU"):  # the remaining checks are those of the plain beam
        text.beam_decode_spans(lp, [5, 5], 4, lm=lm)
    for f in (inf.decode_crop_spans, inf.recognize_crops, inf.read_lines, inf.ocr_page, inf.ocr_lines, inf.ocr_pages, inf._read_crops):
        assert inspect.signature(f).parameters["lm"].default is None
    assert inspect.signature(text.beam_decode_spans_async).parameters["lm"].default is None
    assert inspect.signature(text.beam_decode_spans_async).parameters["lm_scores"].default is None
    assert inf.CharSpans(*[None] * 6).lm_scores is None
    page = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda **k: inf.ocr_page(None, None, page, **k), lambda **k: inf.ocr_lines(None, None, page, **k),
                 lambda **k: inf.ocr_pages(None, None, [page], **k), lambda **k: inf.read_lines(None, page, None, **k),
                 lambda **k: inf.recognize_crops(None, ([], [], []), **k), lambda **k: inf.decode_crop_spans(None, ([], [], []), **k)):
        with pytest.raises(RuntimeError, match="lm needs beam_width"):
            call(lm=lm)
        with pytest.raises(RuntimeError, match="LMGain"):
            call(beam_width=4, lm="model.npz")

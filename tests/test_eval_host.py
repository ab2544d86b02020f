"""CPU-only: the host side of the end-to-end accuracy.  The restatement's greedy matching against an exhaustive search for the
same rule; the ground-truth readers on a small HierText tree; the derived metrics at zero denominators; the new C-ABI symbols; and the Python
surface's refusal of CPU tensors."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest
import torch

from tests import eval_ref as R
from tests.detdata_ref import annotation_words, hiertext_annotations, write_hiertext_tree


def test_greedy_matching_equals_the_exhaustive_search():
    rng = np.random.RandomState(7)
    cases = matched = 0
    for _ in range(400):
        P, G = rng.randint(0, 6), rng.randint(0, 6)
        iou = np.round(rng.uniform(0.3, 1.0, (P, G)), 1 if rng.rand() < 0.5 else 6)  # one decimal: many exact ties, decided by the indices
        iou[rng.rand(P, G) < 0.3] = 0.0
        ignore = rng.rand(G) < 0.2
        got, want = R.greedy_match(iou, ignore), R.exhaustive_match(iou, ignore)
        assert got == want, (iou, ignore)
        gop, pog = got
        assert all(pog[j] == i for i, j in enumerate(gop) if j >= 0) and all(gop[i] == j for j, i in enumerate(pog) if i >= 0)
        assert all(not ignore[j] and iou[i, j] > 0.5 for i, j in enumerate(gop) if j >= 0)
        cases += 1
        matched += sum(j >= 0 for j in gop)
    assert cases == 400 and matched > 400


def test_arg_max_per_prediction_is_not_the_rule():
    iou = np.array([[0.8, 0.0], [0.7, 0.6]])
    assert R.greedy_match(iou, [False, False]) == ([0, 1], [0, 1]) == R.exhaustive_match(iou, [False, False])
    assert R.greedy_match(np.array([[0.9], [0.9]]), [False]) == ([0, -1], [0])  # a tie: the lower prediction index wins


def _tree_with_odd_words(root):
    """write_hiertext_tree's validation split with some words of its first page changed: five vertices, a concave quad, illegible, empty text,
    vertical.  -> (annotations as written, index of each changed word)"""
    write_hiertext_tree(root, "validation")
    anns = hiertext_annotations()
    words = [w for para in anns[0]["paragraphs"] for line in para["lines"] for w in line["words"]]
    assert len(words) >= 5
    words[0]["vertices"] = [[10, 10], [30, 8], [42, 14], [40, 30], [12, 28]]
    words[1]["vertices"] = [[10, 10], [40, 10], [20, 16], [10, 30]]  # concave at the third vertex
    words[2]["legible"] = False
    words[3]["text"] = ""
    words[4]["vertical"] = True
    with gzip.open(os.path.join(root, "gt", "validation.jsonl.gz"), "wt") as f:
        json.dump({"annotations": anns}, f)
    lines_file = os.path.join(root, "gt", "validation.jsonl")
    if os.path.exists(lines_file):
        os.remove(lines_file)
    return anns


def test_hiertext_word_truth_reads_the_tree(tmp_path):
    from ocrs_models_amd import datasets as D
    from ocrs_models_amd.postprocess import _area, _hull, _min_area_rect

    written = write_hiertext_tree(str(tmp_path), "validation")
    truth = D.hiertext_word_truth(str(tmp_path))
    assert [t.image_id for t in truth] == [w[0] for w in written]
    anns = hiertext_annotations()
    for t, ann, (_, polys) in zip(truth, anns, written):
        assert polys == annotation_words(ann) == D.hiertext_word_polygons(ann)
        assert t.quads.dtype == np.float32 and t.quads.shape == (len(polys), 4, 2) and t.ignore.dtype == bool and t.ignore.shape == (len(polys),)
        assert t.texts == [w["text"] for para in ann["paragraphs"] for line in para["lines"] for w in line["words"]]
        assert not t.ignore.any()
        for q, poly in zip(t.quads, polys):  # a convex quad is kept as it is, anything else becomes the rectangle of its hull
            v = np.array(poly, dtype=np.float64)
            e = np.roll(v, -1, axis=0) - v
            turn = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
            convex = _area(v) > 0 and ((turn >= 0).all() or (turn <= 0).all())
            want = v if convex else _min_area_rect(_hull(np.array(poly)))
            assert np.array_equal(q, np.asarray(want, dtype=np.float32))
    assert len(D.hiertext_word_truth(str(tmp_path), max_images=2)) == 2
    assert not os.path.exists(tmp_path / "train")  # no image directory of another split is needed, and no image is read
    with pytest.raises(Exception):
        D.hiertext_word_truth(str(tmp_path), train=True)


def test_hiertext_word_truth_regions_and_flags(tmp_path):
    from ocrs_models_amd import datasets as D
    from ocrs_models_amd.postprocess import _area, _hull, _min_area_rect

    anns = _tree_with_odd_words(str(tmp_path))
    truth = D.hiertext_word_truth(str(tmp_path))
    t = truth[0]
    polys = D.hiertext_word_polygons(anns[0])
    for k in (0, 1):
        want = _min_area_rect(_hull(np.array(polys[k])))
        assert np.array_equal(t.quads[k], want.astype(np.float32))
        assert _area(t.quads[k].astype(np.float64)) >= _area(_hull(np.array(polys[k]))) - 1e-3  # the rectangle encloses the hull
    assert t.ignore.tolist()[:5] == [False, False, True, True, False] and not t.ignore[5:].any()
    assert t.texts[3] == ""
    flagged = D.hiertext_word_truth(str(tmp_path), ignore_vertical=True)[0]
    assert flagged.ignore.tolist()[:5] == [False, False, True, True, True]
    assert all(not u.ignore.any() for u in truth[1:])
    # every region the device stage will see is a convex quad
    for u in truth:
        for q in u.quads.astype(np.float64):
            e = np.roll(q, -1, axis=0) - q
            turn = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
            assert (turn >= -1e-6).all() or (turn <= 1e-6).all()


def test_hiertext_line_truth(tmp_path):
    from ocrs_models_amd import datasets as D
    from ocrs_models_amd.postprocess import _hull, _min_area_rect

    anns = _tree_with_odd_words(str(tmp_path))
    anns[1]["paragraphs"][0]["lines"][0]["legible"] = False
    with gzip.open(os.path.join(str(tmp_path), "gt", "validation.jsonl.gz"), "wt") as f:
        json.dump({"annotations": anns}, f)
    truth = D.hiertext_line_truth(str(tmp_path))
    for t, ann in zip(truth, anns):
        lines = [line for para in ann["paragraphs"] for line in para["lines"]]
        assert t.texts == [line["text"] for line in lines] and t.quads.shape == (len(lines), 4, 2)
        for q, line in zip(t.quads, lines):
            pts = np.array([v for w in line["words"] for v in w["vertices"]])
            assert np.array_equal(q, _min_area_rect(_hull(pts)).astype(np.float32))
    assert truth[1].ignore.tolist()[0] is True and not truth[0].ignore.any() and not truth[1].ignore[1:].any()


def test_from_words_builds_the_same_records():
    from ocrs_models_amd import datasets as D

    sq = [[0, 0], [10, 0], [10, 4], [0, 4]]
    recs = D.from_words([[sq, [[0, 0], [10, 0], [4, 2], [0, 8]]], []], [["ab", ""], []], [[False, False], []], ["x", "y"])
    assert [r.image_id for r in recs] == ["x", "y"]
    assert np.array_equal(recs[0].quads[0], np.array(sq, dtype=np.float32)) and recs[0].ignore.tolist() == [False, True]  # no text: ignored
    from ocrs_models_amd.postprocess import _hull, _min_area_rect

    want = _min_area_rect(_hull(np.array([[0, 0], [10, 0], [4, 2], [0, 8]])))  # concave: the rectangle of its hull
    assert np.array_equal(recs[0].quads[1], want.astype(np.float32)) and not np.array_equal(recs[0].quads[1][2], np.array([4, 2], dtype=np.float32))
    assert recs[1].quads.shape == (0, 4, 2) and recs[1].texts == [] and recs[1].ignore.shape == (0,)
    assert D.from_words([[sq]], [["a"]])[0].ignore.tolist() == [False]
    with pytest.raises(ValueError):
        D.from_words([[sq]], [["a", "b"]])


def test_metrics_at_zero_denominators():
    from ocrs_models_amd.inference.evaluate import COUNTERS, metrics

    assert COUNTERS == R.COUNTERS and len(COUNTERS) == 12
    zero = dict.fromkeys(COUNTERS, 0)
    m = metrics(zero)
    assert m["precision"] == m["recall"] == m["e2e_precision"] == m["e2e_recall"] == m["e2e_precision_ci"] == m["e2e_recall_ci"] == 1.0
    assert m["f1"] == m["e2e_f1"] == m["e2e_f1_ci"] == 1.0 and m["cer_matched"] == 0.0 and m["cer_page"] == 0.0 and m["counters"] == zero
    only_gt = {**zero, "gt": 3, "gt_chars": 9, "gt_chars_unmatched": 9}
    m = metrics(only_gt)
    assert m["precision"] == 1.0 and m["recall"] == 0.0 and m["f1"] == 0.0 and m["cer_matched"] == 0.0 and m["cer_page"] == 1.0
    only_pred = {**zero, "pred": 2, "pred_chars_unmatched": 5}
    m = metrics(only_pred)
    assert m["precision"] == 0.0 and m["recall"] == 1.0 and m["f1"] == 0.0 and m["cer_page"] == 0.0
    c = {**zero, "pages": 1, "pred": 4, "gt": 5, "matched": 3, "exact": 1, "exact_ci": 2, "edit_sum": 3, "gt_chars_matched": 12, "pred_chars_unmatched": 2,
         "gt_chars_unmatched": 7, "gt_chars": 19}
    m = metrics(c)
    assert m == {**R.metrics(c), "counters": c}
    assert m["precision"] == 3 / 4 and m["recall"] == 3 / 5 and m["e2e_precision"] == 1 / 4 and m["e2e_recall_ci"] == 2 / 5
    assert m["cer_matched"] == 3 / 12 and m["cer_page"] == 12 / 19


def test_reference_text_pairs():
    assert R.text_pair("", "") == (0, 3) and R.text_pair("", "hello") == (5, 0) and R.text_pair("Word", "word") == (1, 2)
    assert R.text_pair("École", "école") == (1, 0)  # only ASCII A-Z is folded
    assert R.levenshtein("kitten", "sitting") == 3


def test_new_symbols_are_declared_and_exported():
    from ocrs_models_amd import build as b
    from ocrs_models_amd._lib import HEADER_PATH, LIB_PATH, lib, parse_header

    b.build(verbose=False)
    sigs = parse_header(HEADER_PATH)
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("ocrs_eval_pair_iou", "ocrs_eval_match_ws_bytes", "ocrs_eval_match", "ocrs_eval_text_update"):
        assert name in sigs and hasattr(dll, name), name
    assert sigs["ocrs_eval_match"][1].count("d") == 1  # min_iou travels as a double
    L = lib()
    assert L.eval_match_ws_bytes(300, 270) >= (300 + 270) * 4 and L.eval_match_ws_bytes(0, 0) > 0 and L.eval_match_ws_bytes(-1, 0) == 0


def test_public_surface_and_no_cpu_path():
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.inference import evaluate as E

    assert inf.match_words is E.match_words and inf.OcrAccuracyStats is E.OcrAccuracyStats and inf.evaluate_pages is E.evaluate_pages
    q = torch.zeros(1, 4, 2)
    with pytest.raises(RuntimeError):
        inf.match_words(q, [0, 1], q, [0, 1], torch.zeros(1, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        inf.OcrAccuracyStats("cpu")
    with pytest.raises(RuntimeError):
        inf.evaluate_pages(None, None, [torch.zeros(1, 8, 8, dtype=torch.uint8)], [None, None])
    with pytest.raises(RuntimeError):  # line results without the words' texts: the message says what to pass
        E._predictions([{"quad": [[0, 0]] * 4, "text": "a b", "words": [[[0, 0]] * 4] * 2}], "word")
    try:
        E._predictions([{"quad": [[0, 0]] * 4, "text": "a b", "words": [[[0, 0]] * 4] * 2}], "word")
    except RuntimeError as e:
        assert "chars=True" in str(e)
    quads, texts = E._predictions([{"quad": 1, "text": "a b", "words": [2, 3], "word_texts": ["a", "b"]}, {"quad": 4, "text": "c"}], "word")
    assert quads == [2, 3, 4] and texts == ["a", "b", "c"]
    assert E._predictions([{"quad": 1, "text": "a b", "words": [2, 3]}], "line") == ([1], ["a b"])


def test_eval_ocr_cli_has_no_cpu_path(tmp_path):
    """without a GPU the CLI raises before it reads anything, like the other CLIs; with one it gets as far as the missing dataset"""
    from ocrs_models_amd import eval_ocr

    argv = ["hiertext", str(tmp_path / "missing"), "--det-model", "a", "--rec-model", "b"]
    if torch.cuda.is_available():
        with pytest.raises(Exception, match="not found"):
            eval_ocr.main(argv)
    else:
        with pytest.raises(RuntimeError, match="GPU"):
            eval_ocr.main(argv)
    with pytest.raises(SystemExit):
        eval_ocr.main(["hiertext", str(tmp_path), "--det-model", "a", "--rec-model", "b", "--lm", "x.npz"])  # --lm needs --beam-width

"""End-to-end accuracy of page OCR on the GPU (csrc/ocr_eval.hip; inference.match_words, OcrAccuracyStats, evaluate_pages and the eval_ocr
command line) against the host restatement (tests/eval_ref.py, pinned by tests/test_eval_host.py).

IoU.  The device repeats the host's fp64 operations in the host's order (the standard tests/test_postprocess_gpu.py holds ``quad_inter`` to, with
the BLAS caveat of DESIGN.md §8): every stored IoU must be bit-equal.

Matching, ignore rule, text, counters.  Integers, and IoUs that are compared but never combined: everything must equal the restatement with
``==``.  So that a last-bit difference in an IoU could not flip a decision anyway, every case asserts on the host that no two candidate IoUs of
a page lie within 1e-9 of each other or of ``min_iou`` (ties built from bit-identical quads excepted, and declared)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import chars_ref as CR
from tests import eval_ref as R
from tests import lines_ref as LR
from tests import ocr_ref
from tests import test_lines_gpu as TL
from tests.test_eval_host import _tree_with_odd_words

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _truth(gq, gt, gi, image_id=None):
    from ocrs_models_amd.datasets import WordTruth

    return WordTruth(image_id, np.asarray(gq, dtype=np.float32).reshape(-1, 4, 2), list(gt), np.asarray(gi, dtype=bool).reshape(-1))


def _results(pq, pt):
    """word dicts as ocr_page returns them"""
    return [{"quad": np.asarray(q, dtype=np.float32).tolist(), "text": t} for q, t in zip(pq, pt)]


def _texts(n, seed, lo=1, hi=12):
    rng = np.random.RandomState(seed)
    return ["".join(chr(int(c)) for c in rng.randint(97, 123, size=rng.randint(lo, hi + 1))) for _ in range(n)]


def _rounds(iou, ignore, min_iou=0.5):
    """how many rounds of mutually-best pairs the page needs (the last round, which finds nothing, not counted)"""
    gop, pog, rounds = [-1] * iou.shape[0], [-1] * iou.shape[1], 0
    while True:
        free = [(i, j) for i, j in R.candidates(iou, ignore, min_iou) if gop[i] == -1 and pog[j] == -1]
        bg, bp = {}, {}
        for i, j in free:  # in the total order: the first pair seen for an end is its best
            bg.setdefault(i, j), bp.setdefault(j, i)
        took = [(i, j) for i, j in bg.items() if bp[j] == i]
        if not took:
            return rounds
        for i, j in took:
            gop[i], pog[j] = j, i
        rounds += 1


def _check(dev, pred_pages, truth_pages, min_iou=0.5, ties=None, stats=None):
    """one update on the device against the restatement: matches, IoUs, distances, flags.  -> (reference pages, reference counters, stats)"""
    from ocrs_models_amd.inference import OcrAccuracyStats

    stats = stats or OcrAccuracyStats(dev, min_iou)
    stats.update([_results(q, t) for q, t in pred_pages], [_truth(*g) for g in truth_pages])
    ref, counters = R.evaluate(pred_pages, truth_pages, min_iou)
    m, last = stats.last["matches"], stats.last
    gop, pog, iop, iou = m.gt_of_pred.cpu().numpy(), m.pred_of_gt.cpu().numpy(), m.iou_of_pred.cpu().numpy(), m.pair_iou.cpu().numpy()
    dist, flags = last["dist"].cpu().numpy(), last["flags"].cpu().numpy()
    p0 = g0 = 0
    for b, (r, (pq, _), (gq, _, gi)) in enumerate(zip(ref, pred_pages, truth_pages)):
        P, G = len(pq), len(gq)
        gap = R.closest_gap(r["iou"], gi, min_iou, (ties or {}).get(b, ()))
        assert gap >= MARGIN, (b, gap)
        assert iou[m.pair_offs[b]:m.pair_offs[b + 1]].tobytes() == r["iou"].astype(np.float64).tobytes(), b
        assert gop[p0:p0 + P].tolist() == r["gt_of_pred"], (b, gop[p0:p0 + P].tolist(), r["gt_of_pred"])
        assert pog[g0:g0 + G].tolist() == r["pred_of_gt"], b
        assert iop[p0:p0 + P].tobytes() == np.array(r["iou_of_pred"], dtype=np.float64).tobytes(), b
        assert dist[p0:p0 + P].tolist() == r["dist"] and flags[p0:p0 + P].tolist() == r["flags"], b
        p0, g0 = p0 + P, g0 + G
    assert p0 == len(gop) and g0 == len(pog) and m.pair_offs[-1] == len(iou)
    return ref, counters, stats


# ------------------------------------------------------------------ IoU -----------------------------------------------------------------
def test_pair_iou_is_bit_equal_to_the_host(dev):
    from ocrs_models_amd import inference as inf

    rng = np.random.RandomState(2)
    rr = lambda: ocr_ref.rotated_rect(rng.uniform(40, 260), rng.uniform(40, 200), rng.uniform(30, 120), rng.uniform(8, 40), rng.uniform(-90, 90))  # noqa: E731
    pred = [rr() for _ in range(40)]
    gt = [rr() for _ in range(37)]
    gt[0], gt[1] = pred[0].copy(), pred[1].copy()                                  # identical pairs
    pred[2], gt[2] = LR.box(300, 10, 40, 12), LR.box(340, 10, 30, 12)                # sharing an edge: the strict bbox test fails
    pred[3], gt[3] = LR.box(300, 40, 40, 12), LR.box(320, 52, 40, 12)                # sharing half an edge
    pred[4] = np.array([[50, 50], [90, 70], [90, 70], [50, 50]], dtype=np.float32)   # zero area on the prediction side
    gt[4] = np.array([[60, 60], [100, 80], [100, 80], [60, 60]], dtype=np.float32)   # and on the annotation side, across other quads
    pred[5], gt[5] = ocr_ref.rotated_rect(150, 120, 80, 30, 20, flip=True), ocr_ref.rotated_rect(155, 118, 80, 30, 17)  # one given clockwise
    gt[6] = ocr_ref.rotated_rect(100, 100, 60, 20, -30, flip=True)
    pred, gt = np.stack(pred), np.stack(gt)
    want, _, _ = R.pair_geometry(pred, gt)
    m = inf.match_words(torch.from_numpy(pred).to(dev), [0, 40], torch.from_numpy(gt).to(dev), [0, 37], torch.zeros(37, dtype=torch.bool, device=dev))
    got = m.pair_iou.cpu().numpy().reshape(40, 37)
    assert m.pair_offs == [0, 40 * 37]
    assert want[0, 0] == 1.0 or abs(want[0, 0] - 1.0) < 1e-12
    assert want[2, 2] == 0.0 and want[3, 3] == 0.0 and (want[4] == 0.0).all() and (want[:, 4] == 0.0).all() and want[5, 5] > 0.5
    nz = int((want > 0).sum())
    print(f"pair IoU: {nz} of {want.size} pairs overlap, {int((want > 0.5).sum())} above 0.5")
    assert nz > 200
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    # the offsets may also be device tensors (read once), and the result is the same bytes
    offs = lambda n: torch.tensor([0, n], dtype=torch.int32, device=dev)  # noqa: E731
    again = inf.match_words(torch.from_numpy(pred).to(dev), offs(40), torch.from_numpy(gt).to(dev), offs(37), torch.zeros(37, dtype=torch.uint8, device=dev))
    assert all(torch.equal(a, b) for a, b in zip(m[:4], again[:4]))
    ref = R.match_page(pred, gt, np.zeros(37, bool))
    assert m.gt_of_pred.tolist() == ref["gt_of_pred"] and m.pred_of_gt.tolist() == ref["pred_of_gt"]


def test_match_words_arguments(dev):
    from ocrs_models_amd import inference as inf

    q = torch.zeros(2, 4, 2, device=dev)
    ign = torch.zeros(2, dtype=torch.bool, device=dev)
    with pytest.raises(RuntimeError):
        inf.match_words(q.cpu(), [0, 2], q, [0, 2], ign)
    with pytest.raises(RuntimeError):
        inf.match_words(q, [0, 2], q, [0, 2], ign.cpu())
    with pytest.raises(RuntimeError):
        inf.match_words(q, torch.tensor([0, 2], dtype=torch.int32), q, [0, 2], ign)  # a CPU tensor of offsets
    with pytest.raises(RuntimeError):
        inf.match_words(q, [0, 1], q, [0, 2], ign)  # offsets that do not end at the number of quads
    with pytest.raises(RuntimeError):
        inf.match_words(q, [0, 1, 2], q, [0, 2], ign)  # different page counts
    with pytest.raises(RuntimeError):
        inf.match_words(q.double(), [0, 2], q, [0, 2], ign)
    m = inf.match_words(q[:0], [0], q[:0], [0], ign[:0])  # no pages: nothing is launched
    assert m.gt_of_pred.numel() == 0 and m.pred_of_gt.numel() == 0 and m.pair_offs == [0]


# ------------------------------------------------------------------ matching ------------------------------------------------------------
def _ybox(y, dx=0.0, w=100.0, h=60.0):
    return LR.box(dx, y, w, h)


def test_arg_max_per_prediction_would_be_wrong(dev):
    gq = [LR.box(0, 0, 100, 20), LR.box(0, 8.5, 100, 20)]
    pq = [LR.box(0, -5, 100, 25), LR.box(0, 3.5, 100, 20)]
    ref, _, _ = _check(dev, [(pq, ["a", "b"])], [(gq, ["a", "b"], [False, False])])
    iou = ref[0]["iou"]
    assert abs(iou[0, 0] - 0.8) < 1e-12 and abs(iou[1, 0] - 16.5 / 23.5) < 1e-12 and abs(iou[1, 1] - 0.6) < 1e-12 and iou[1, 0] > iou[1, 1]
    assert ref[0]["gt_of_pred"] == [0, 1] and ref[0]["pred_of_gt"] == [0, 1]


def test_identical_predictions_the_lower_index_wins(dev):
    gq = [LR.box(0, 0, 100, 20)]
    pq = [LR.box(0, 0, 100, 22), LR.box(0, 0, 100, 22)]
    ref, c, _ = _check(dev, [(pq, ["a", "a"])], [(gq, ["a"], [False])], ties={0: [[(0, 0), (1, 0)]]})
    assert ref[0]["gt_of_pred"] == [0, -1] and c["matched"] == 1 and c["pred"] == 2 and c["pred_chars_unmatched"] == 1


def _chain_case(n=9):
    """g_k and p_k one below the other: p_k lies d_k = 1 + 2k above g_k and 2 + 2k below g_{k-1}'s successor position, so the offsets
    p_0 g_0 | p_1 g_0 | p_1 g_1 | p_2 g_1 | ... grow by one: every p_{k+1} prefers g_k, which prefers p_k.  Each prediction is moved sideways by
    its own amount so that no two IoUs of the page coincide."""
    ys = [0.0]
    for k in range(n - 1):
        ys.append(ys[-1] + 5 + 4 * k)
    gq = [_ybox(y) for y in ys]
    pq = [_ybox(y - (1 + 2 * k), dx=0.013 * (k + 1) ** 1.5) for k, y in enumerate(ys)]
    return pq, gq


def test_a_chain_of_dependencies_needs_many_rounds(dev):
    pq, gq = _chain_case()
    n = len(pq)
    ref, c, _ = _check(dev, [(pq, _texts(n, 1))], [(gq, _texts(n, 2), [False] * n)])
    assert _rounds(ref[0]["iou"], [False] * n) >= 8
    assert ref[0]["gt_of_pred"] == list(range(n)) and c["matched"] == n
    best = ref[0]["iou"].argmax(axis=1).tolist()
    assert best[1:] == list(range(n - 1))  # every prediction but the first would rather have the annotation above its own


def _grid_case(seed, cols=21, rows=15, n_gt=270, first_pred=15, n_pred=300, doubles=20):
    """a jittered grid of words: annotations in the cells 0 .. n_gt - 1, predictions (perturbed copies) in the cells from first_pred on -- the
    first ``doubles`` of them twice -- so some annotations have no prediction and the reverse; both lists shuffled"""
    rng = np.random.RandomState(seed)
    cell = lambda k: (30 + 64 * (k % cols) + rng.uniform(-3, 3), 20 + 34 * (k // cols) + rng.uniform(-2, 2))  # noqa: E731
    centres = [cell(k) for k in range(cols * rows)]
    gq = [ocr_ref.rotated_rect(cx, cy, rng.uniform(40, 54), rng.uniform(14, 22), rng.uniform(-4, 4)) for cx, cy in centres[:n_gt]]
    cells = list(range(first_pred, first_pred + n_pred - doubles)) + list(range(first_pred, first_pred + doubles))
    assert len(cells) == n_pred and max(cells) < cols * rows
    pq = [ocr_ref.rotated_rect(centres[k][0] + rng.uniform(-4, 4), centres[k][1] + rng.uniform(-2, 2), rng.uniform(40, 54), rng.uniform(14, 22), rng.uniform(-5, 5))
          for k in cells]
    pq = [pq[i] for i in rng.permutation(len(pq))]
    gq = [gq[i] for i in rng.permutation(len(gq))]
    return pq, gq


def test_a_page_of_300_by_270_words(dev):
    pq, gq = _grid_case(5)
    assert len(pq) == 300 and len(gq) == 270
    ign = (np.arange(270) % 17 == 3)
    ref, c, _ = _check(dev, [(pq, _texts(300, 3))], [(gq, _texts(270, 4), ign)])
    gop = ref[0]["gt_of_pred"]
    print(f"300 x 270: {c['matched']} matched, {gop.count(-1)} unmatched and {gop.count(-2)} ignored predictions, {ref[0]['pred_of_gt'].count(-1)} annotations "
          f"without one, {_rounds(ref[0]['iou'], ign)} rounds")
    assert c["matched"] > 150 and gop.count(-1) > 30 and gop.count(-2) > 5 and ref[0]["pred_of_gt"].count(-1) > 20


def test_four_pages_nothing_matches_across_pages(dev):
    pq0, gq0 = _grid_case(8, cols=6, rows=5, n_gt=24, first_pred=3, n_pred=27, doubles=4)
    far = [LR.box(3000 + 70 * k, 3000, 50, 20) for k in range(5)]
    pages_p = [pq0, [g.copy() for g in gq0], [p.copy() for p in pq0], far[:3]]     # page 1's predictions are page 0's annotations
    pages_g = [gq0, far, [g.copy() for g in gq0], [p.copy() for p in pq0[:7]]]     # page 3's annotations are page 0's predictions
    preds = [(p, _texts(len(p), 10 + b)) for b, p in enumerate(pages_p)]
    truth = [(g, _texts(len(g), 20 + b), [False] * len(g)) for b, g in enumerate(pages_g)]
    ref, c, _ = _check(dev, preds, truth)
    assert ref[0]["gt_of_pred"] == ref[2]["gt_of_pred"] and sum(j >= 0 for j in ref[0]["gt_of_pred"]) > 15
    assert set(ref[1]["gt_of_pred"]) == {-1} and set(ref[3]["gt_of_pred"]) == {-1} and set(ref[3]["pred_of_gt"]) == {-1}
    assert c["pages"] == 4 and c["matched"] == 2 * sum(j >= 0 for j in ref[0]["gt_of_pred"])


def test_pages_without_predictions_or_annotations(dev):
    pq, gq = _grid_case(9, cols=5, rows=4, n_gt=18, first_pred=2, n_pred=18, doubles=2)
    preds = [([], []), (pq, _texts(18, 1)), (pq[:5], _texts(5, 2)), ([], []), (pq, _texts(18, 3))]
    truth = [(gq[:6], _texts(6, 4), [False] * 6), (gq, _texts(18, 5), [False] * 18), ([], [], []), ([], [], []), (gq, _texts(18, 6), [k % 4 == 0 for k in range(18)])]
    ref, c, stats = _check(dev, preds, truth)
    assert ref[0]["pred_of_gt"] == [-1] * 6 and ref[2]["gt_of_pred"] == [-1] * 5 and ref[3]["gt_of_pred"] == [] and ref[3]["pred_of_gt"] == []
    assert stats.counters() == c and c["pages"] == 5
    # and a call in which no page has anything
    _, c0, stats0 = _check(dev, [([], []), ([], [])], [([], [], []), ([], [], [])])
    assert stats0.counters() == c0 == {**dict.fromkeys(R.COUNTERS, 0), "pages": 2}
    assert stats0.result()["precision"] == 1.0 and stats0.result()["cer_page"] == 0.0


# ------------------------------------------------------------------ ignore rule ---------------------------------------------------------
def test_the_ignore_rule(dev):
    gq = [LR.box(0, 0, 200, 40), LR.box(300, 0, 100, 20), LR.box(0, 100, 100, 20), LR.box(20, 195, 100, 20)]
    gi = [True, True, False, True]
    pq = [LR.box(50, 10, 60, 20),      # inside the ignored word 0: ignored
          LR.box(300, 0, 100, 22),     # IoU 0.91 against the ignored word 1 and nothing else near: not a match (and ignored)
          LR.box(0, 100, 100, 21),     # the one true match
          LR.box(0, 200, 40, 10),      # half inside the ignored word 3, at exactly 0.5: not ignored
          LR.box(500, 500, 30, 10)]    # far from everything
    ref, c, stats = _check(dev, [(pq, ["in", "over", "match", "half", "far"])], [(gq, ["", "ignored", "match", "x"], gi)])
    assert ref[0]["gt_of_pred"] == [-2, -2, 2, -1, -1] and ref[0]["pred_of_gt"] == [-1, -1, 2, -1]
    _, inter, pa = R.pair_geometry(pq, gq)
    assert inter[3, 3] / pa[3] == 0.5 and ref[0]["iou"][1, 1] > 0.9
    assert c["pred_ignored"] == 2 and c["pred"] == 3 and c["gt"] == 1 and c["matched"] == 1 and c["exact"] == 1 and c["gt_chars"] == 5
    assert c["pred_chars_unmatched"] == len("half") + len("far")
    r = stats.result()
    assert r["counters"] == c and r["precision"] == 1 / 3 and r["recall"] == 1.0  # the ignored predictions count in neither


# ------------------------------------------------------------------ text ----------------------------------------------------------------
def test_text_distances_and_flags(dev):
    rng = np.random.RandomState(4)
    word = lambda n, lo=0x61, hi=0x7b: "".join(chr(int(c)) for c in rng.randint(lo, hi, size=n))  # noqa: E731
    high = "".join(chr(c) for c in (0x1F600, 0x10348, 0x4E2D, 0x1F601, 0x20000))
    long64, tail = word(64), word(65, 0x61, 0x64)
    pairs = [("", ""), ("", word(5)), (word(5), ""), ("a", "a"), ("a", "b"), (long64, long64), (word(64), word(64)), (word(65), word(64)), (word(64), word(65)),
             (word(130), word(70)), (word(70), word(130)), (long64 + "x" + tail, long64 + tail),
             (high, high), (high, high[:2] + chr(0x1F602) + high[3:]), (word(3) + high, high + word(3)),
             ("Hello World", "hello world"), ("HELLO", "hello"), ("École", "école"), ("École", "École"), ("straße", "STRASSE"), ("[Z@`{", "[z@`{")]
    quads = [LR.box(0, 40 * k, 100, 20) for k in range(len(pairs))]
    over = [LR.box(0, 40 * k, 100, 20 + 0.25 * (k + 1)) for k in range(len(pairs))]  # every pair has an IoU of its own
    ref, c, stats = _check(dev, [(over, [p for p, _ in pairs])], [(quads, [g for _, g in pairs], [False] * len(pairs))])
    r = ref[0]
    assert r["gt_of_pred"] == list(range(len(pairs)))
    by = {pair: (d, f) for pair, d, f in zip(pairs, r["dist"], r["flags"])}
    assert by[("", "")] == (0, 3) and by[("a", "b")] == (1, 0) and by[(long64, long64)] == (0, 3) and by[(high, high)] == (0, 3)
    assert by[pairs[1]] == (5, 0) and by[pairs[2]] == (5, 0) and by[pairs[11]] == (1, 0) and by[pairs[13]] == (1, 0)
    assert by[("Hello World", "hello world")] == (2, 2) and by[("HELLO", "hello")] == (5, 2)
    assert by[("École", "école")] == (1, 0) and by[("École", "École")] == (0, 3) and by[("[Z@`{", "[z@`{")] == (1, 2)
    assert stats.counters() == c and c["edit_sum"] == sum(r["dist"]) and c["exact"] == sum(f & 1 for f in r["flags"]) and c["exact_ci"] == sum(f >> 1 for f in r["flags"])


# ------------------------------------------------------------------ counters ------------------------------------------------------------
def _counter_cases():
    pq, gq = _grid_case(12, cols=8, rows=6, n_gt=40, first_pred=5, n_pred=43, doubles=6)
    gt_t, gi = _texts(40, 30), [k % 9 == 0 for k in range(40)]
    over = R.match_page(pq, gq, gi)["gt_of_pred"]  # which annotation each prediction lies over decides what it "reads"
    pt = []
    for k, j in enumerate(over):  # a third reads its annotation's text, a third reads it in capitals, the rest something else
        t = gt_t[j] if j >= 0 else "stray"
        pt.append(t if k % 3 == 0 else (t.upper() if k % 3 == 1 else t[::-1] + "q"))
    a = ([(pq, pt)], [(gq, gt_t, gi)])
    pq2, gq2 = _grid_case(13, cols=5, rows=4, n_gt=17, first_pred=0, n_pred=20, doubles=3)
    b = ([(pq2, _texts(20, 32)), ([], [])], [(gq2, _texts(17, 33), [False] * 17), (gq2[:3], ["abc", "de", "f"], [False, True, False])])
    return a, b


def test_two_updates_add_up_and_two_runs_give_identical_bytes(dev):
    from ocrs_models_amd.inference import OcrAccuracyStats

    a, b = _counter_cases()
    _, ca, sa = _check(dev, *a)
    _, cb, sb = _check(dev, *b)
    assert sa.counters() == ca and sb.counters() == cb and len(ca) == 12
    assert ca["matched"] > 10 and ca["exact"] > 0 and ca["exact_ci"] > ca["exact"] and ca["edit_sum"] > 0 and ca["pred_ignored"] > 0
    both = OcrAccuracyStats(dev)
    _check(dev, *a, stats=both)
    _check(dev, *b, stats=both)
    total = {k: ca[k] + cb[k] for k in ca}
    assert both.counters() == total
    got = both.result()
    assert got == {**R.metrics(total), "counters": total}
    assert 0 < got["e2e_f1"] < got["e2e_f1_ci"] < got["f1"] < 1 and 0 < got["cer_matched"] and got["cer_page"] > 0
    again = OcrAccuracyStats(dev)
    _check(dev, *a, stats=again)
    snapshot = [t.cpu().numpy().tobytes() for t in (*again.last["matches"][:4], again.last["dist"], again.last["flags"])]
    assert snapshot == [t.cpu().numpy().tobytes() for t in (*sa.last["matches"][:4], sa.last["dist"], sa.last["flags"])]
    _check(dev, *b, stats=again)
    assert again.state.cpu().numpy().tobytes() == both.state.cpu().numpy().tobytes()


def test_update_does_not_wait(dev):
    """update queues one upload and the launches; the counters are read in result().  Counted the way tests/test_chars_gpu.py counts waits."""
    from ocrs_models_amd.inference import OcrAccuracyStats

    (preds, truth), _ = _counter_cases()
    results, records = [_results(q, t) for q, t in preds], [_truth(*g) for g in truth]
    stats = OcrAccuracyStats(dev)
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        stats.update(results, records)
    _, n, what = TL._count_waits(lambda: stats.update(results, records))
    assert n == 0, what
    _, n_result, _ = TL._count_waits(stats.result)
    assert n_result >= 1
    assert stats.counters() == {k: 3 * v for k, v in R.evaluate(preds, truth)[1].items()}


def test_update_reads_line_dicts_and_refuses_them_without_word_texts(dev):
    from ocrs_models_amd.inference import OcrAccuracyStats

    words = [LR.box(0, 0, 40, 12), LR.box(50, 0, 40, 12), LR.box(0, 30, 40, 12)]
    line_q = [LR.box(0, 0, 90, 12), LR.box(0, 30, 40, 12)]
    lines = [{"quad": line_q[0].tolist(), "text": "ab cd", "words": [w.tolist() for w in words[:2]], "word_texts": ["ab", "cd"]},
             {"quad": line_q[1].tolist(), "text": "ef", "words": [words[2].tolist()], "word_texts": ["ef"]}]
    stats = OcrAccuracyStats(dev)
    stats.update([lines], [_truth(words, ["ab", "cd", "ef"], [False] * 3)])
    assert stats.result()["e2e_f1"] == 1.0 and stats.counters()["matched"] == 3
    by_line = OcrAccuracyStats(dev)
    by_line.update([lines], [_truth(line_q, ["ab cd", "ef"], [False] * 2)], level="line")
    assert by_line.result()["e2e_f1"] == 1.0 and by_line.counters()["matched"] == 2 and by_line.counters()["gt_chars"] == 7
    with pytest.raises(RuntimeError, match="chars=True"):
        stats.update([[{k: v for k, v in d.items() if k != "word_texts"} for d in lines]], [_truth(words, ["ab", "cd", "ef"], [False] * 3)])
    with pytest.raises(RuntimeError):
        stats.update([lines], [])
    with pytest.raises(RuntimeError):
        stats.update([lines], [_truth(words, ["ab", "cd", "ef"], [False] * 3)], level="char")


# ------------------------------------------------------------------ end to end: painted detector, stub recogniser ----------------------------
class Stub(torch.nn.Module):
    """a recogniser whose log-probs are prescribed, as in tests/test_chars_gpu.py: (n,1,64,Wpad) -> (Wpad // 4 + 1, n, C), the same for every
    sample: class ``c`` wins the steps t0..t1 of each ``(t0, t1, c, value)``, the blank everywhere else"""

    def __init__(self, chars, C):
        super().__init__()
        self.chars, self.C = chars, C

    def forward(self, x):
        n, _, h, wpad = x.shape
        assert h == 64
        T = wpad // 4 + 1
        lp = torch.full((T, n, self.C), -10.0, device=x.device)
        lp[:, :, 0] = -0.5
        for t0, t1, c, value in self.chars:
            if t1 < T:
                lp[t0:t1 + 1, :, c] = value - 0.125
                lp[(t0 + t1) // 2, :, c] = value
        return lp


ROWS, COLS, SIZE = 4, 3, (190, 200)
BARS = [(15 + 52 * c, 18 + 40 * r, 40, 12) for r in range(ROWS) for c in range(COLS)]


@pytest.fixture(scope="module")
def painted(dev):
    """(page, painted detector, stub that says "ab c def" over every row of three bars, the truth of that page)"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    page, det = TL.bar_page(190, 200, BARS, dev)
    found = inf.detect_words(det, page, size=SIZE)
    lines = inf.find_lines(found["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    assert plan.host()[0] == ROWS
    table, lq, wq = plan.table.cpu().numpy(), lines.quads.cpu().numpy(), found["quads"].cpu().numpy()
    order, offs = lines.word_order.cpu().numpy(), lines.line_offsets.cpu().numpy()
    ow = int(table[0, 2])
    wb = CR.word_bounds(lq[0], wq[order[offs[0]:offs[1]]], np.float64)
    lng = float(ocr_ref.crop_frame(lq[0])["long"])
    lo, hi = wb["lo"], wb["hi"]
    where = [("a", lo[0] + 0.25 * (hi[0] - lo[0])), ("b", lo[0] + 0.7 * (hi[0] - lo[0])), (" ", hi[0] - 1.0),
             ("c", lo[1] + 0.2 * (hi[1] - lo[1])), (" ", lo[1] + 0.5 * (hi[1] - lo[1])), ("d", lo[1] + 0.85 * (hi[1] - lo[1])),
             ("e", lo[2] + 0.1 * (hi[2] - lo[2])), ("f", lo[2] + 0.7 * (hi[2] - lo[2]))]
    steps = [int(round(s / lng * ow / 4)) for _, s in where]
    assert all(b - a >= 4 for a, b in zip(steps, steps[1:])) and steps[0] >= 1 and steps[-1] + 1 < ow // 4
    stub = Stub([(t - 1, t + 1, DEFAULT_ALPHABET.index(ch) + 1, -(k + 1) / 64) for k, ((ch, _), t) in enumerate(zip(where, steps))], len(DEFAULT_ALPHABET) + 1).eval()
    # the painted geometry: a bar's component spans its pixel centres, and the drivers expand it by SHRINK_DISTANCE on every side
    e = inf.SHRINK_DISTANCE
    quads = [LR.box(x - e, y - e, w - 1 + 2 * e, h - 1 + 2 * e) for x, y, w, h in BARS]
    texts = ["ab", "c d", "ef"] * ROWS
    return page, det, stub, quads, texts


def test_evaluate_pages_on_a_painted_page(dev, painted):
    from ocrs_models_amd import inference as inf

    page, det, stub, quads, texts = painted
    n = len(quads)
    truth = [_truth(quads, texts, [False] * n, "painted")]
    got = inf.evaluate_pages(det, stub, [page], truth, size=SIZE)
    c = got["counters"]
    print("painted page:", json.dumps(got))
    assert c == {"pages": 1, "pred": n, "gt": n, "pred_ignored": 0, "matched": n, "exact": n, "exact_ci": n, "edit_sum": 0, "gt_chars_matched": sum(map(len, texts)),
                 "pred_chars_unmatched": 0, "gt_chars_unmatched": 0, "gt_chars": sum(map(len, texts))}
    assert got["precision"] == got["recall"] == got["e2e_f1"] == got["f1"] == got["e2e_f1_ci"] == 1.0 and got["cer_matched"] == 0.0 and got["cer_page"] == 0.0
    # one annotated text off by two characters, one annotated word gone
    changed = list(texts)
    changed[4] = "x y"
    wrong = [_truth(quads[:7] + quads[8:], changed[:7] + changed[8:], [False] * (n - 1))]
    bad = inf.evaluate_pages(det, stub, [page], wrong, size=SIZE)
    cb = bad["counters"]
    assert cb["matched"] == n - 1 and cb["exact"] == n - 2 and cb["edit_sum"] == 2 and cb["pred"] == n and cb["gt"] == n - 1
    assert cb["pred_chars_unmatched"] == len(texts[7]) and cb["gt_chars_unmatched"] == 0
    assert bad["cer_page"] == (2 + len(texts[7])) / cb["gt_chars"] and bad["cer_matched"] == 2 / cb["gt_chars_matched"] and bad["recall"] == 1.0
    assert bad["precision"] == (n - 1) / n and bad["e2e_recall"] == (n - 2) / (n - 1)
    # other decoders and crops read the same page the same way: the stub's distributions are peaked
    assert inf.evaluate_pages(det, stub, [page], truth, size=SIZE, beam_width=4)["counters"] == c
    assert inf.evaluate_pages(det, stub, [page], truth, size=SIZE, rectify="chain")["counters"] == c
    # lines against annotated lines, and two batches of one page against one batch of two
    e = inf.SHRINK_DISTANCE  # a row's line quad: from its first bar's left edge to its last bar's right edge
    line_truth = [_truth([LR.box(BARS[3 * r][0] - e, BARS[3 * r][1] - e, BARS[3 * r + 2][0] + 39 + 2 * e - BARS[3 * r][0], 11 + 2 * e) for r in range(ROWS)],
                         ["ab c def"] * ROWS, [False] * ROWS)]
    by_line = inf.evaluate_pages(det, stub, [page], line_truth, level="line", size=SIZE)
    assert by_line["e2e_f1"] == 1.0 and by_line["counters"]["matched"] == ROWS and by_line["counters"]["gt_chars"] == 8 * ROWS
    twice = inf.evaluate_pages(det, stub, [page, page], truth * 2, size=SIZE, batch_pages=1)
    assert twice["counters"] == {k: 2 * v for k, v in c.items()}
    with pytest.raises(RuntimeError):
        inf.evaluate_pages(det, stub, [page], truth * 2, size=SIZE)


# ------------------------------------------------------------------ command line --------------------------------------------------------
def test_eval_ocr_cli_on_a_small_tree(dev, tmp_path, capsys):
    import ocrs_models_amd as oa
    from ocrs_models_amd import eval_ocr
    from ocrs_models_amd.checkpoint import save_checkpoint

    anns = _tree_with_odd_words(str(tmp_path / "data"))
    torch.manual_seed(0)
    det, rec = oa.DetectionModel(), oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    save_checkpoint(str(tmp_path / "rec.pt"), rec, oa.optim.Adam(rec.parameters()), 0)
    words = [w for a in anns for para in a["paragraphs"] for line in para["lines"] for w in line["words"]]
    capsys.readouterr()
    eval_ocr.main(["hiertext", str(tmp_path / "data"), "--det-model", str(tmp_path / "det.pt"), "--rec-model", str(tmp_path / "rec.pt"), "--batch-pages", "3",
                   "--ignore-vertical"])
    out = [line for line in capsys.readouterr().out.splitlines() if line.strip()]
    assert len(out) == 1
    got = json.loads(out[0])
    assert got["options"]["images"] == len(anns) == 5 and got["options"]["level"] == "word" and got["options"]["split"] == "validation"
    assert got["counters"]["pages"] == 5 and got["counters"]["gt"] == len(words) - 3  # illegible, empty and (with the flag) vertical
    assert got["counters"]["gt_chars"] == sum(len(w["text"]) for k, w in enumerate(words) if k not in (2, 3, 4))
    assert set(got) >= {"precision", "recall", "f1", "e2e_precision", "e2e_recall", "e2e_f1", "e2e_f1_ci", "cer_matched", "cer_page", "counters", "options"}
    assert os.path.exists(tmp_path / "data" / "gt" / "validation.jsonl")

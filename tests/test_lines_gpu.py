"""Text lines on the GPU (csrc/text_lines.hip, inference.find_lines / ocr_lines) against the numpy restatement of the rule (tests/lines_ref.py,
pinned by tests/test_lines_host.py).

Exact cases.  Axis-aligned words with integer corners below 4096: centres are multiples of 0.25 below 4096, side lengths integers, u is
(1, 0) or (0, 1), every product and sum of the rule is an integer multiple of 1/8 below 2^15, and the direction sum of a line is (sum of
integers, 0): all exact in fp32.  So EVERYTHING must equal the float32 restatement with ``==``, line quads included.

Rotated lines.  Decisions are at least a pixel from their thresholds (tests/lines_ref.py::decision_margin, checked on the host), so links and
order must equal the float64 restatement; line-quad corners within 8 * ulp32(largest |coordinate|): u_L carries a relative error of a few
2^-24 (a sum of roundings, a square root, a division), a projection x*u.x + y*u.y three roundings, mapping back three more, each on
magnitudes up to the largest coordinate -- the bound the issue sets; the test prints the measured maximum (DESIGN.md §14 records it).

End to end.  Detection is a fixed module that returns a painted probability map where the geometry has to be known (rows of bars, words far
apart), the golden detection weights where any components will do; recognition always runs the golden recognition weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lines_ref as R
from tests.golden_util import DET_CASES, REC_CASE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_F, SENT_I = -12345.0, -77


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _golden_state(kind):
    from oracle.params import detection_specs, make_state, recognition_specs, state_dict_from

    specs, seed = (detection_specs(), DET_CASES["det1"]["seed"]) if kind == "det" else (recognition_specs(), REC_CASE["seed"])
    P, Bf = make_state(specs, seed)
    return state_dict_from(P, Bf, specs)


@pytest.fixture(scope="module")
def det_model(dev):
    import ocrs_models_amd as oa

    m = oa.DetectionModel()
    m.load_state_dict(_golden_state("det"))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def rec_model(dev):
    import ocrs_models_amd as oa

    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    m.load_state_dict(_golden_state("rec"))
    return m.to(dev).eval()


def _sentinel_out(n, dev):
    from ocrs_models_amd import inference as inf

    i32 = dict(dtype=torch.int32, device=dev)
    return inf.TextLines(torch.full((n, 4, 2), SENT_F, device=dev), torch.full((1,), SENT_I, **i32), torch.full((n,), SENT_I, **i32),
                         torch.full((n,), SENT_I, **i32), torch.full((n + 1,), SENT_I, **i32), torch.full((n,), SENT_I, **i32))


def _run(dev, quads, count=None, **kw):
    """find_lines into sentinel-filled outputs -> (host numpy dict, L)"""
    from ocrs_models_amd import inference as inf

    q = torch.from_numpy(np.ascontiguousarray(quads, dtype=np.float32)).to(dev)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    out = _sentinel_out(len(quads), dev)
    got = inf.find_lines(q, cnt, out=out, **kw)
    assert got is out
    fresh = inf.find_lines(q, cnt, **kw)  # tensors of its own: the same values wherever they are defined
    L = int(out.n_lines.item())
    n = len(quads) if count is None else min(count, len(quads))
    assert int(fresh.n_lines.item()) == L and torch.equal(fresh.quads[:L], out.quads[:L]) and torch.equal(fresh.line_offsets[:L + 1], out.line_offsets[:L + 1])
    for k in ("line_of_word", "word_order", "next_word"):
        assert torch.equal(getattr(fresh, k)[:n], getattr(out, k)[:n]), k
    return {k: getattr(out, k).cpu().numpy() for k in ("quads", "n_lines", "line_of_word", "word_order", "line_offsets", "next_word")}, L


def _check_exact(dev, quads, count=None, want_lines=None, **kw):
    n = len(quads) if count is None else count
    got, L = _run(dev, quads, count, **kw)
    ref = R.find_lines(quads[:n], dtype=np.float32, **kw)
    if want_lines is not None:
        assert ref["lines"] == want_lines
    assert L == ref["n_lines"]
    assert np.array_equal(got["next_word"][:n], ref["next_word"])
    assert np.array_equal(got["line_of_word"][:n], ref["line_of_word"])
    assert np.array_equal(got["word_order"][:n], ref["word_order"])
    assert np.array_equal(got["line_offsets"][:L + 1], ref["line_offsets"])
    assert ref["quads"].dtype == np.float32 and np.array_equal(got["quads"][:L], ref["quads"])
    # nothing past the valid part is written: line quads from L on, offsets after L, per-word entries from the count on
    assert (got["quads"][L:] == SENT_F).all() and (got["line_offsets"][L + 1:] == SENT_I).all()
    for k in ("next_word", "line_of_word", "word_order"):
        assert (got[k][n:] == SENT_I).all(), k
    return got, ref


def _chain(n, w, h, gap):
    q = np.stack(R.row_of_words(3, 5, n, w, h, gap))
    assert q.max() < 4096
    return q


EXACT = {
    "one word": lambda: (R.box(10, 20, 60, 20)[None], [[0]]),
    "two words": lambda: (np.stack(R.row_of_words(0, 0, 2)), [[0, 1]]),
    "row, gap, row": R.case_row_gap_row,
    "competing predecessors": R.case_competing,
    "acceptance tie": R.case_accept_tie,
    "choice tie": R.case_choice_tie,
    "choice tie, swapped": lambda: R.case_choice_tie(True),
    "tall boxes link downward": lambda: (np.stack([R.box(0, 80 * k, 20, 60) for k in range(4)])[::-1], [[3, 2, 1, 0]]),
    "wide boxes stacked": lambda: (np.stack([R.box(0, 30 * k, 60, 20) for k in range(4)]), [[0], [1], [2], [3]]),
    "N = 256": lambda: (R.grid_case(23, 23, seed=2)[:256], None),            # one full LDS tile
    "N = 257": lambda: (R.grid_case(23, 23, seed=2)[:257], None),            # one word into the second tile
    "N = 513": lambda: (R.grid_case(23, 23, seed=4)[:513], None),            # three tiles, the last with one word
    "chain of 70": lambda: (_chain(70, 40, 14, 10), [list(range(70))]),      # longer than a wave; 7 jump rounds
    "chain of 300": lambda: (_chain(300, 9, 4, 4), [list(range(300))]),      # crosses a tile; 9 rounds; five chunks of the direction sum
    "chain of 300, shuffled": lambda: (_chain(300, 9, 4, 4)[np.random.RandomState(8).permutation(300)], None),
    "64 lines of 5, shuffled": lambda: (R.grid_case(64, 5, seed=6), None),
    "N = 2100 (one launch per jump round)": lambda: (R.grid_case(42, 50, seed=9), None),  # above the single-workgroup limit of 2048
}


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_equal_the_float32_restatement(dev, name):
    quads, want = EXACT[name]()
    assert quads.max() < 4096 and (quads == np.rint(quads)).all()
    got, ref = _check_exact(dev, quads, want_lines=want)
    if name.startswith("64 lines"):
        assert ref["n_lines"] == 64 and all(len(c) == 5 for c in ref["lines"])
    if name.startswith("N = 2100"):
        assert len(quads) > 2048 and ref["n_lines"] == 42 and all(len(c) == 50 for c in ref["lines"])
    if name == "chain of 300, shuffled":
        assert ref["n_lines"] == 1 and got["quads"][0].tolist() == [[3, 5], [3 + 299 * 13 + 9, 5], [3 + 299 * 13 + 9, 9], [3, 9]]


def test_rule_parameters_reach_the_kernel(dev):
    quads, _ = R.case_row_gap_row()
    _check_exact(dev, quads, max_gap=4.0, want_lines=[[0, 1, 2, 3, 4]])
    _check_exact(dev, quads, max_gap=0.5, want_lines=[[0], [1], [2], [3], [4]])


def test_device_count_below_the_buffer(dev):
    """a padded buffer: rows past the device count are not words (here they would be a tenth line), outputs past it stay untouched"""
    words = R.grid_case(9, 7, seed=3)
    pad = np.stack(R.row_of_words(0, 9 * 40, 37))  # a tenth row: a line of its own if it were read
    quads = np.concatenate([words, pad])
    got, ref = _check_exact(dev, quads, count=len(words))
    assert ref["n_lines"] == 9 and got["n_lines"][0] == 9
    _check_exact(dev, quads, count=0)
    _check_exact(dev, quads, count=1)
    full, _ = _check_exact(dev, quads)
    assert full["n_lines"][0] == 10
    big, _ = _run(dev, quads, count=10 ** 6)  # a count beyond the buffer is clamped to it
    for k in full:
        assert np.array_equal(big[k], full[k]), k


def test_no_words_no_launch(dev):
    from ocrs_models_amd import inference as inf

    r = inf.find_lines(torch.empty(0, 4, 2, device=dev))
    assert tuple(r.quads.shape) == (0, 4, 2) and r.n_lines.tolist() == [0] and r.line_of_word.numel() == 0 and r.word_order.numel() == 0
    assert tuple(r.line_offsets.shape) == (1,) and r.next_word.numel() == 0
    with pytest.raises(RuntimeError):
        inf.find_lines(torch.empty(3, 4, 2))  # no CPU path
    with pytest.raises(RuntimeError):
        inf.find_lines(torch.empty(3, 4, 2, device=dev).double())


def test_find_lines_makes_no_host_sync(dev):
    from ocrs_models_amd import inference as inf

    quads = torch.from_numpy(R.grid_case(42, 50, seed=9)).to(dev)  # above the single-workgroup limit: every kernel of the stage runs
    small, cnt = quads[:300].contiguous(), torch.tensor([280], dtype=torch.int32, device=dev)
    want = [inf.find_lines(quads), inf.find_lines(small, cnt)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [inf.find_lines(quads), inf.find_lines(small, cnt)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for g, w in zip(got, want):
        L = int(w.n_lines)
        assert int(g.n_lines) == L and torch.equal(g.quads[:L], w.quads[:L]) and torch.equal(g.line_offsets[:L + 1], w.line_offsets[:L + 1])


# ------------------------------------------------------------------ rotated lines ------------------------------------------------------
@pytest.fixture(scope="module")
def rotated(dev):
    quads = R.rotated_case()
    return quads, R.find_lines(quads, dtype=np.float64), _run(dev, quads)


def test_rotated_lines_against_float64(rotated):
    quads, ref, (got, L) = rotated
    n = len(quads)
    assert R.decision_margin(quads) > 1.0 and max(len(c) for c in ref["lines"]) == 7
    assert L == ref["n_lines"]
    assert np.array_equal(got["next_word"], ref["next_word"]) and np.array_equal(got["line_of_word"], ref["line_of_word"])
    assert np.array_equal(got["word_order"], ref["word_order"]) and np.array_equal(got["line_offsets"][:L + 1], ref["line_offsets"])
    top = float(np.abs(ref["quads"]).max())
    bound = 8 * R.ulp32(top)
    err = float(np.abs(got["quads"][:L].astype(np.float64) - ref["quads"]).max())
    print(f"rotated lines: {n} words, {L} lines, max corner error {err:.3e} = {err / R.ulp32(top):.2f} ulp32({top:.1f}), bound {bound:.3e}")
    assert err <= bound
    assert (got["quads"][L:] == SENT_F).all()


def test_one_word_lines_are_bit_copies(rotated):
    quads, ref, (got, L) = rotated
    singles = [(l, c[0]) for l, c in enumerate(ref["lines"]) if len(c) == 1]
    assert len(singles) == 10
    for l, w in singles:
        assert got["quads"][l].tobytes() == quads[w].tobytes()


def test_two_runs_give_identical_bytes(dev, rotated):
    cases = [rotated[0], R.grid_case(42, 50, seed=9), R.case_accept_tie()[0]]
    for quads in cases:
        a, _ = _run(dev, quads)
        b, _ = _run(dev, quads)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------ crop_plan(count=) --------------------------------------------------
def test_crop_plan_with_a_device_count(dev):
    from ocrs_models_amd import inference as inf

    quads = torch.from_numpy(R.rotated_case()).to(dev)
    c = 41
    cnt = torch.tensor([c], dtype=torch.int32, device=dev)
    whole, part = inf.crop_plan(quads[:c].contiguous()), inf.crop_plan(quads, count=cnt)
    assert tuple(part.table.shape) == (len(quads), 8)
    assert torch.equal(part.table[:c], whole.table) and torch.equal(part.totals, whole.totals)
    assert part.host() == whole.host() and part.host()[0] == c and part.host_perm() == whole.host_perm()
    assert torch.equal(inf.crop_plan(quads, 48, cnt).table[:c], inf.crop_plan(quads[:c].contiguous(), 48).table)
    # the later stages work from the plan's count: same crops, same batches
    page = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (1, 2400, 3000)).astype(np.uint8)).to(dev)
    pa, pb = inf.rectify_crops(page, quads[:c].contiguous(), whole), inf.rectify_crops(page, quads, part)
    assert torch.equal(pa, pb)
    (ba, wa, perm_a), (bb, wb, perm_b) = inf.crops_to_batches(pa, whole, 16), inf.crops_to_batches(pb, part, 16)
    assert perm_a == perm_b and len(ba) == len(bb) == 3
    assert all(torch.equal(x, y) for x, y in zip(ba, bb)) and all(torch.equal(x, y) for x, y in zip(wa, wb))
    with pytest.raises(RuntimeError):
        inf.crop_plan(quads, count=torch.tensor([c], dtype=torch.int64, device=dev))


# ------------------------------------------------------------------ end to end ---------------------------------------------------------
class Painted(torch.nn.Module):
    """a detector that returns a fixed probability map (1,1,h,w), whatever the page"""

    def __init__(self, probs):
        super().__init__()
        self.probs = probs

    def forward(self, x):
        assert tuple(x.shape[-2:]) == tuple(self.probs.shape[-2:])
        return self.probs[None, None]


def bar_page(H, W, bars, dev):
    """(page (1,H,W) uint8 with dark bars, detector painted with the same bars); bars = (x, y, w, h) in pixels"""
    page = np.full((H, W), 230, np.uint8)
    probs = np.zeros((H, W), np.float32)
    for k, (x, y, w, h) in enumerate(bars):
        page[y:y + h, x:x + w] = 20 + 7 * (k % 9)
        page[y + 2:y + h - 2:3, x + 2:x + w - 2:4] = 200
        probs[y:y + h, x:x + w] = 0.9
    return torch.from_numpy(page)[None].to(dev), Painted(torch.from_numpy(probs).to(dev)).eval()


def dot_page(H, W, step=16, size=6):
    y, x = np.mgrid[0:H, 0:W]
    p = np.full((H, W), 230, np.uint8)
    p[((y % step) < size) & ((x % step) < size)] = 20
    return torch.from_numpy(p)[None]


def test_ocr_lines_equals_the_stages_chained_by_hand(dev, det_model, rec_model):
    from ocrs_models_amd import inference as inf

    page = dot_page(320, 240).to(dev)
    size = (160, 120)
    det = inf.detect_words(det_model, page, size=size)
    assert det["n"] > 0
    lines = inf.find_lines(det["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    packed = inf.rectify_crops(page, lines.quads, plan)
    texts = inf.recognize_crops(rec_model, inf.crops_to_batches(packed, plan))
    L = int(lines.n_lines.item())
    got = inf.ocr_lines(det_model, rec_model, page, size=size)
    assert len(got) == L == plan.host()[0] == len(texts) and 0 < L <= det["n"]
    assert [g["text"] for g in got] == texts
    assert torch.equal(torch.tensor([g["quad"] for g in got]), lines.quads[:L].cpu())
    order, offs, quads = lines.word_order.cpu().tolist(), lines.line_offsets.cpu().tolist(), det["quads"].cpu()
    assert offs[L] == det["n"]
    for l, g in enumerate(got):
        assert set(g) == {"quad", "text", "words"}
        assert torch.equal(torch.tensor(g["words"]), quads[order[offs[l]:offs[l + 1]]])
    # and they are the rule's lines: the kernels follow the float32 restatement operation by operation, so even a comparison that falls on
    # its threshold on these unconstructed quads is decided the same way
    ref = R.find_lines(quads.numpy(), dtype=np.float32)
    print(f"golden detector: {det['n']} words, {L} lines, longest {max(len(c) for c in ref['lines'])}")
    assert [order[offs[l]:offs[l + 1]] for l in range(L)] == ref["lines"]


def test_words_too_far_apart_stay_one_line_each(dev, rec_model):
    from ocrs_models_amd import inference as inf

    # 40 x 12 bars, 80 apart in x (after the expansion by 3: 74 > max_gap * 18) and 40 in y (> half a height); odd columns 5 lower
    bars = [(20 + 120 * c, 20 + 40 * r + 5 * (c % 2), 40, 12) for r in range(6) for c in range(4)]
    page, det = bar_page(280, 500, bars, dev)
    words = inf.ocr_page(det, rec_model, page, size=(280, 500))
    lines = inf.ocr_lines(det, rec_model, page, size=(280, 500))
    assert len(words) == len(lines) == len(bars)
    assert all(len(g["words"]) == 1 and g["words"][0] == g["quad"] for g in lines)

    def as_set(rs):
        return {(tuple(map(tuple, r["quad"])), r["text"]) for r in rs}

    assert as_set(words) == as_set(lines) and len(as_set(words)) == len(bars)
    f = R.word_frames(np.array([g["quad"] for g in lines], dtype=np.float32))
    keys = list(zip(f["cy"].tolist(), f["cx"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)  # the line-sort order (no two heads share a centre, so the index never decides)
    # with a reach that spans the gaps the rows link up: 4 words per line
    linked = inf.ocr_lines(det, rec_model, page, size=(280, 500), max_gap=5.0, min_cos=0.9)
    assert len(linked) == 6 and all(len(g["words"]) == 4 for g in linked)


def _count_waits(fn):
    """(result, number of host waits): calls of Stream.synchronize / Event.synchronize / torch.cuda.synchronize plus every operation torch's
    synchronisation debug mode reports"""
    import warnings

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
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        for (o, n), f in zip(saved, originals):
            setattr(o, n, f)
    reported = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    return out, len(calls) + len(reported), calls + reported


def test_ocr_lines_waits_no_more_often_than_ocr_page(dev, rec_model):
    """the three synchronisations of ocr_page (component count, plan totals, labels) are all ocr_lines has: the line count comes with the
    plan's totals, the line table and the quads with the labels.  Counted on a page with one chunk of crops either way."""
    from ocrs_models_amd import inference as inf

    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)]
    page, det = bar_page(230, 340, bars, dev)
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        inf.ocr_page(det, rec_model, page, size=(230, 340)), inf.ocr_lines(det, rec_model, page, size=(230, 340))
    words, n_page, what_page = _count_waits(lambda: inf.ocr_page(det, rec_model, page, size=(230, 340)))
    lines, n_lines, what_lines = _count_waits(lambda: inf.ocr_lines(det, rec_model, page, size=(230, 340)))
    print(f"host waits: ocr_page {n_page} {what_page}, ocr_lines {n_lines} {what_lines}")
    assert len(words) == 30 and len(lines) == 5
    assert n_page >= 3 and n_lines <= n_page


def test_rows_of_bars_become_one_line_per_row(dev, rec_model):
    from ocrs_models_amd import inference as inf

    rows, cols = 5, 6
    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(rows) for c in range(cols)]  # 12 apart: 6 after the expansion
    page, det = bar_page(230, 340, bars, dev)
    lines = inf.ocr_lines(det, rec_model, page, size=(230, 340))
    assert len(lines) == rows
    for r, g in enumerate(lines):
        assert len(g["words"]) == cols and isinstance(g["text"], str)
        xs = [np.mean([p[0] for p in w]) for w in g["words"]]
        assert xs == sorted(xs) and len(set(xs)) == cols  # left to right
        ys = [p[1] for w in g["words"] for p in w]
        assert 18 + 40 * r - 4 <= min(ys) and max(ys) <= 18 + 40 * r + 2 + 12 + 4  # this row's bars
        q = np.array(g["quad"])
        assert q[:, 0].min() <= 15 - 2 and q[:, 0].max() >= 15 + 52 * (cols - 1) + 40 + 1  # the line quad spans the row


def test_ocr_lines_of_an_empty_page(dev, det_model):
    from ocrs_models_amd import inference as inf

    class NeverCalled(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the recogniser must not run for a page without words")

    page = torch.full((1, 200, 160), 255, dtype=torch.uint8, device=dev)
    assert inf.ocr_lines(det_model, NeverCalled().eval(), page, size=(128, 96), threshold=1.0) == []


# ------------------------------------------------------------------ CLI ----------------------------------------------------------------
def test_eval_detection_cli_with_and_without_lines(dev, det_model, rec_model, tmp_path):
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.checkpoint import save_checkpoint
    from PIL import Image

    det = oa.DetectionModel()
    det.load_state_dict(_golden_state("det"))
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    rec.load_state_dict(_golden_state("rec"))
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    save_checkpoint(str(tmp_path / "rec.pt"), rec, oa.optim.Adam(rec.parameters()), 0)
    W, H = 600, 800
    page_h = dot_page(H, W)
    Image.fromarray(page_h[0].numpy()).save(tmp_path / "page.png")

    def run(base, *flags):
        r = subprocess.run([sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), base,
                            "--rec-model", str(tmp_path / "rec.pt"), *flags], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return [line for line in r.stdout.splitlines() if line.strip()]

    page = page_h.to(dev)
    # with --lines: the extra picture, and one JSON object per line with the three keys -- what ocr_lines returns for the page
    base = str(tmp_path / "lines")
    out = run(base, "--lines")
    for name in ("input", "text-regions", "text-probs", "text-words", "text-lines"):
        with Image.open(f"{base}-{name}.png") as im:
            assert im.size == (W, H), name
    with Image.open(f"{base}-text-lines.png") as im:
        assert im.mode == "RGB"
    got = [json.loads(line) for line in out]
    assert got and all(set(g) == {"quad", "text", "words"} and np.asarray(g["quad"]).shape == (4, 2) and np.asarray(g["words"]).shape[1:] == (4, 2) for g in got)
    assert got == inf.ocr_lines(det_model, rec_model, page)
    # without: what it printed before (one object per word, ocr_page's) and no line picture
    base = str(tmp_path / "words")
    out = run(base)
    assert not os.path.exists(f"{base}-text-lines.png") and os.path.exists(f"{base}-text-words.png")
    assert out == [json.dumps(w) for w in inf.ocr_page(det_model, rec_model, page)]

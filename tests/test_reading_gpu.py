"""Reading order on the GPU (csrc/reading_order.hip, inference.reading_order and the ``reading_order=`` keyword of the drivers) against the
numpy restatement of the rule (tests/reading_ref.py, pinned by tests/test_reading_host.py).

Exact cases.  Axis-aligned line quads with integer corners below 4096: u_l is an axis, lng_l an integer, the direction sum a sum of integers,
so U = (1, 0) exactly and every projection, extent and yc is a multiple of 1/4 below 4096; gaps and block_gap * height are exact for the
block_gap values used.  So line_order, new_block and the WHOLE before matrix must equal the float32 restatement with ``==``.

Rotated lines.  The two-column page as word quads turned about the page centre goes through find_lines and then reading_order.  Every decision
of both stages is at least 1.5 px from its threshold (lines_ref.decision_margin, reading_ref.decision_margin, asserted on the host), while the
float32 extents are within a few ulp32(1000) ~ 6e-5 px of the float64 ones, so order, block flags and the relation must equal the float64
restatement's on the same line quads, and through the line names the unrotated order.

End to end.  A painted probability map for a detector (the geometry has to be known) and the golden recognition weights, as
tests/test_lines_gpu.py does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lines_ref as LR
from tests import reading_ref as RR
from tests.test_lines_gpu import _count_waits, _golden_state, bar_page, dot_page

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77
PAD = 5  # rows of the buffers past L


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rec_model(dev):
    import ocrs_models_amd as oa

    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    m.load_state_dict(_golden_state("rec"))
    return m.to(dev).eval()


def _text_lines(dev, quads, offs=None, pad=PAD):
    """the TextLines a line stage would hand over for these line quads: L lines in a buffer of L + pad rows (the rows past L are NaN: they
    must not be read); only quads, n_lines and line_page_offs are the reading order's input"""
    from ocrs_models_amd import inference as inf

    L, n = len(quads), len(quads) + pad
    buf = np.full((n, 4, 2), np.nan, dtype=np.float32)
    buf[:L] = quads
    i32 = dict(dtype=torch.int32, device=dev)
    junk = torch.full((n,), SENT, **i32)
    return inf.TextLines(torch.from_numpy(buf).to(dev), torch.tensor([L], **i32), junk, junk, torch.full((n + 1,), SENT, **i32), junk,
                         None if offs is None else torch.tensor(offs, **i32))


def _sentinel_out(n, dev):
    from ocrs_models_amd import inference as inf

    i32 = dict(dtype=torch.int32, device=dev)
    return inf.ReadingOrder(torch.full((n,), SENT, **i32), torch.full((n,), SENT, **i32), torch.full((n, (n + 31) // 32), SENT, **i32))


def _words(before: torch.Tensor) -> np.ndarray:
    return before.cpu().numpy().view(np.uint32)


def _unpack(before: torch.Tensor) -> np.ndarray:
    """(n, n) bool from the kernel's bit words"""
    w = _words(before)
    n = w.shape[0]
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1)[:, :n].astype(bool)


def _check_exact(dev, quads, offs=None, block_gap=1.0):
    from ocrs_models_amd import inference as inf

    assert quads.max() < 4096 and quads.min() >= 0 and (quads == np.rint(quads)).all()
    L, n = len(quads), len(quads) + PAD
    tl = _text_lines(dev, quads, offs)
    out = _sentinel_out(n, dev)
    got = inf.reading_order(tl, block_gap, out=out)
    assert got is out
    fresh = inf.reading_order(tl, block_gap)  # tensors of its own: the same values wherever they are defined
    assert torch.equal(fresh.line_order[:L], out.line_order[:L]) and torch.equal(fresh.new_block[:L], out.new_block[:L]) and torch.equal(fresh.before, out.before)
    ref = RR.reading_order(quads, offs, block_gap, np.float32)
    order, flags = out.line_order.cpu().numpy(), out.new_block.cpu().numpy()
    assert np.array_equal(order[:L], ref["line_order"])
    assert np.array_equal(flags[:L], ref["new_block"])
    assert np.array_equal(_words(out.before), RR.pack_bits(ref["before"], n))  # every word: rows and columns from L on are 0
    assert (order[L:] == SENT).all() and (flags[L:] == SENT).all()
    return ref


def test_two_columns(dev):
    quads, names, want = RR.case_two_columns()
    ref = _check_exact(dev, quads)
    assert [names[i] for i in ref["line_order"]] == want and ref["forced"] == 0 and names != want
    _check_exact(dev, quads, block_gap=0.7)
    _check_exact(dev, quads, block_gap=1.5)


def test_three_columns(dev):
    quads, names, want = RR.case_three_columns()
    ref = _check_exact(dev, quads)
    assert [names[i] for i in ref["line_order"]] == want and ref["forced"] == 0


def test_cycle_takes_the_forced_emission(dev):
    ref = _check_exact(dev, RR.case_cycle())
    assert ref["forced"] >= 1 and ref["line_order"].tolist() == RR.CYCLE_ORDER


SIZES = {
    "L = 1": lambda: RR.xyxy(5, 7, 90, 21)[None],
    "L = 2 with equal yc": lambda: np.stack([RR.xyxy(0, 10, 100, 30), RR.xyxy(50, 5, 150, 35)]),
    "L = 33": lambda: RR.columns_case(33, 2, headers=(9,))[:33],                      # one bit into the second word
    "L = 257": lambda: RR.columns_case(257, 3, h=8, row_pitch=12),                    # one line into the second tile and row tile
    "L = 513": lambda: RR.columns_case(513, 3, h=4, row_pitch=7),                     # three tiles, the last with one line
    "L = 259 with spanning lines": lambda: RR.columns_case(257, 3, h=8, row_pitch=12, headers=(30, 60)),
    "L = 2100": lambda: RR.columns_case(2098, 4, h=4, row_pitch=7, headers=(100, 300)),  # in-degrees in the workspace; blockers in later tiles
}


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes_equal_the_float32_restatement(dev, name):
    quads = SIZES[name]()
    ref = _check_exact(dev, quads)
    assert len(quads) == int(name.split()[2])
    if name == "L = 2100":
        xs = quads[ref["line_order"], 0, 0]
        assert len(quads) > 2048 and ref["forced"] == 0 and not (np.diff(xs) >= 0).all()  # the spanning lines cut the columns into sections
    if name in ("L = 257", "L = 513"):
        assert (np.diff(quads[ref["line_order"], 0, 0]) >= 0).all() and int(ref["new_block"].sum()) == 3  # column by column


def test_block_gap_reaches_the_kernel(dev):
    for gap in (19, 20, 21):
        quads = np.stack([RR.xyxy(0, 0, 200, 20), RR.xyxy(10, 20 + gap, 150, 40 + gap)])
        assert _check_exact(dev, quads)["new_block"].tolist() == [1, int(gap > 20)]
        assert _check_exact(dev, quads, block_gap=2.0)["new_block"].tolist() == [1, 0]
        assert _check_exact(dev, quads, block_gap=0.5)["new_block"].tolist() == [1, 1]


def _peel(dev, before, n_lines=None):
    """ocrs_reading_peel alone on a hand-made matrix"""
    from ocrs_models_amd._lib import lib, ptr

    n = before.shape[0]
    L = lib()
    i32 = dict(dtype=torch.int32, device=dev)
    bits = torch.from_numpy(RR.pack_bits(before, n).view(np.int32)).to(dev)
    count = torch.tensor([n if n_lines is None else n_lines], **i32)
    order = torch.full((n,), SENT, **i32)
    ws_bytes = L.reading_order_ws_bytes(n, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    L.reading_peel(ptr(count), None, 1, n, ptr(bits), ptr(order), ptr(ws), ws_bytes)
    return order.cpu().tolist()


def test_peel_of_a_hand_made_matrix(dev):
    before = np.zeros((6, 6), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5)):  # a 3-cycle, then a chain hanging off it
        before[a, b] = True
    for m in (before, before[::-1, ::-1].copy()):
        want, forced = RR.peel(m, [0, 6])
        assert forced >= 1
        assert _peel(dev, m) == want.tolist()
    assert _peel(dev, before) == [0, 1, 2, 3, 4, 5] and _peel(dev, before[::-1, ::-1].copy()) == [0, 1, 2, 3, 5, 4]
    assert _peel(dev, before, n_lines=4) == RR.peel(before[:4, :4], [0, 4])[0].tolist() + [SENT, SENT]  # bits of rows and columns from L on are not read


# ------------------------------------------------------------------ batches -----------------------------------------------------------
def test_exact_batch_with_an_empty_page(dev):
    q1, q3 = RR.case_two_columns()[0], RR.case_cycle()
    quads, offs = np.concatenate([q1, q3]), [0, len(q1), len(q1), len(q1) + len(q3)]
    ref = _check_exact(dev, quads, offs)
    a = len(q1)
    assert not ref["before"][:a, a:].any() and not ref["before"][a:, :a].any() and ref["line_order"][a:].tolist() == [a + i for i in RR.CYCLE_ORDER]
    # the same lines as ONE page are another matter: the pages would be related
    assert RR.reading_order(quads)["before"][:a, a:].any()


def test_batch_equals_each_page_shifted(dev):
    """reading_order on find_lines_pages' output against reading_order on find_lines' output of every page"""
    from ocrs_models_amd import inference as inf

    pages = [RR.case_two_columns()[0], np.zeros((0, 4, 2), np.float32), RR.case_three_columns()[0][::-1].copy()]
    flat = torch.from_numpy(np.concatenate(pages)).to(dev)
    counts = [len(p) for p in pages]
    word_offs = torch.tensor(np.cumsum([0] + counts), dtype=torch.int32, device=dev)
    page_of_word = torch.tensor(sum(([p] * c for p, c in enumerate(counts)), []), dtype=torch.int32, device=dev)
    tl = inf.find_lines_pages(flat, page_of_word, word_offs, max_gap=1.0)  # (at 2.0 a line of the left column would reach the right one)
    ro = inf.reading_order(tl)
    lpo = tl.line_page_offs.cpu().tolist()
    assert lpo == [0, 17, 17, 31] and int(tl.n_lines) == 31
    bits = _unpack(ro.before)
    seen = np.zeros_like(bits)
    for p, words in enumerate(pages):
        lo, hi = lpo[p], lpo[p + 1]
        if not len(words):
            continue
        one_lines = inf.find_lines(torch.from_numpy(words).to(dev), max_gap=1.0)
        one = inf.reading_order(one_lines)
        L = int(one_lines.n_lines)
        assert L == hi - lo
        assert torch.equal(ro.line_order[lo:hi], one.line_order[:L] + lo)
        assert torch.equal(ro.new_block[lo:hi], one.new_block[:L])
        assert torch.equal(torch.from_numpy(bits[lo:hi, lo:hi]), torch.from_numpy(_unpack(one.before)[:L, :L]))
        seen[lo:hi, lo:hi] = True
        ref = RR.reading_order(one_lines.quads[:L].cpu().numpy())
        assert np.array_equal(one.line_order[:L].cpu().numpy(), ref["line_order"]) and ref["forced"] == 0
    assert bits.any() and not (bits & ~seen).any()  # no bit across a page seam


def test_no_lines_no_launch_and_argument_errors(dev):
    from ocrs_models_amd import inference as inf

    empty = inf.reading_order(inf.find_lines(torch.empty(0, 4, 2, device=dev)))
    assert empty.line_order.numel() == 0 and empty.new_block.numel() == 0 and tuple(empty.before.shape) == (0, 0)
    tl = _text_lines(dev, RR.case_cycle())
    with pytest.raises(RuntimeError):
        inf.reading_order(tl.quads)  # not a TextLines
    with pytest.raises(RuntimeError):
        inf.reading_order(inf.TextLines(tl.quads.cpu(), tl.n_lines, tl.line_of_word, tl.word_order, tl.line_offsets, tl.next_word))  # no CPU path
    with pytest.raises(RuntimeError):
        inf.reading_order(inf.TextLines(tl.quads.double(), tl.n_lines, tl.line_of_word, tl.word_order, tl.line_offsets, tl.next_word))
    with pytest.raises(RuntimeError):
        inf.reading_order(inf.TextLines(tl.quads, tl.n_lines.long(), tl.line_of_word, tl.word_order, tl.line_offsets, tl.next_word))
    with pytest.raises(RuntimeError):
        inf.reading_order(inf.TextLines(tl.quads, tl.n_lines, tl.line_of_word, tl.word_order, tl.line_offsets, tl.next_word, tl.n_lines.long()))
    with pytest.raises(RuntimeError):
        inf.reading_order(tl, out=_sentinel_out(3, dev))


# ------------------------------------------------------------------ rotation -----------------------------------------------------------
def _two_column_words():
    """every box of the two-column page as a row of words 15 apart: five of 68 for the lines across the page, three of 50 for a column's"""
    words = []
    for _, (x0, y0, x1, y1) in RR.two_column_boxes():
        n, w = (5, 68) if x1 - x0 == 400 else (3, 50)
        words += [RR.xyxy(x0 + k * (w + 15), y0, x0 + k * (w + 15) + w, y1) for k in range(n)]
    return np.stack(words).astype(np.float64)


@pytest.mark.parametrize("deg", [5, -5, 20, -20])
def test_rotated_two_columns_against_float64(dev, deg):
    from ocrs_models_amd import inference as inf

    named = RR.two_column_boxes()
    t = np.deg2rad(deg)
    rot = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    centre, shift = np.array([200.0, 165.0]), 300.0
    words = ((_two_column_words() - centre) @ rot.T + centre + shift).astype(np.float32)
    words = words[np.random.RandomState(3).permutation(len(words))]
    m_lines = LR.decision_margin(words, max_gap=1.0)
    tl = inf.find_lines(torch.from_numpy(words).to(dev), max_gap=1.0)  # (at 2.0 a line of the left column would reach the right one)
    L = int(tl.n_lines)
    lq = tl.quads[:L].cpu().numpy()
    ref_lines = LR.find_lines(words, max_gap=1.0, dtype=np.float64)
    top = float(np.abs(ref_lines["quads"]).max())
    err = float(np.abs(lq.astype(np.float64) - ref_lines["quads"]).max()) if L == ref_lines["n_lines"] else float("nan")
    m_read = RR.decision_margin(lq, block_gap=0.7)
    print(f"rotated two columns, {deg:+d} deg: {len(words)} words, {L} lines, margins find_lines {m_lines:.3f} px, reading_order {m_read:.3f} px; "
          f"max line-quad corner error {err:.3e} px = {err / LR.ulp32(top):.2f} ulp32({top:.1f})")
    assert m_lines >= 1.5 and m_read >= 1.5
    assert L == len(named) == ref_lines["n_lines"] and err <= 8 * LR.ulp32(top)
    ro = inf.reading_order(tl, block_gap=0.7)
    ref = RR.reading_order(lq, block_gap=0.7, dtype=np.float64)
    order = ro.line_order[:L].cpu().numpy()
    assert np.array_equal(order, ref["line_order"]) and ref["forced"] == 0
    assert np.array_equal(ro.new_block[:L].cpu().numpy(), ref["new_block"])
    assert np.array_equal(_unpack(ro.before)[:L, :L], ref["before"])
    # back through the line names: the centre of every line, turned back, is the centre of one box
    back = (lq.astype(np.float64).mean(1) - shift - centre) @ rot + centre
    boxes = np.array([[(b[0] + b[2]) / 2, (b[1] + b[3]) / 2] for _, b in named])
    dist = np.abs(back[:, None, :] - boxes[None]).max(2)
    assert (dist.min(1) < 0.01).all()
    names = [named[i][0] for i in dist.argmin(1)]
    unrotated = RR.case_two_columns()
    assert [names[i] for i in order] == unrotated[2] == [n for n, _ in named]
    # blocks at block_gap = 0.7: the two lines across the page and the four columns
    assert [names[i] for i, f in zip(order, ro.new_block[:L].cpu().tolist()) if f] == ["H1", "A0", "B0", "H2", "C0", "D0"]


# ------------------------------------------------------------------ waits, determinism ---------------------------------------------------
def test_reading_order_makes_no_host_sync_and_repeats_its_bytes(dev):
    from ocrs_models_amd import inference as inf

    q1, q3 = RR.case_two_columns()[0], RR.case_cycle()
    cases = [_text_lines(dev, SIZES["L = 2100"]()), _text_lines(dev, np.concatenate([q1, q3]), [0, len(q1), len(q1), len(q1) + len(q3)]),
             _text_lines(dev, RR.case_cycle(), pad=0)]
    want = [inf.reading_order(tl) for tl in cases]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [inf.reading_order(tl) for tl in cases]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for tl, g, w in zip(cases, got, want):
        L = int(tl.n_lines)
        for k in ("line_order", "new_block"):
            assert getattr(g, k)[:L].cpu().numpy().tobytes() == getattr(w, k)[:L].cpu().numpy().tobytes(), k
        assert g.before.cpu().numpy().tobytes() == w.before.cpu().numpy().tobytes()


# ------------------------------------------------------------------ end to end ---------------------------------------------------------
ROWS, PAGE = 5, (180, 380)


def _two_column_page(dev):
    """two columns of ROWS lines, three bars of 40 x 12 a line, 12 apart (6 after the expansion by 3: linked); the columns 60 apart (54 after
    the expansion, beyond max_gap * 18 = 36: never linked); rows 30 apart (a gap of 12 <= 18 between expanded lines: one block a column); the
    right column 4 higher, so line order takes R0, L0, R1, L1, ..."""
    bars = [(x0 + 52 * c, y0 + 30 * r, 40, 12) for x0, y0 in ((15, 22), (219, 18)) for r in range(ROWS) for c in range(3)]
    return bar_page(*PAGE, bars, dev)


def _side(line):
    return "L" if np.mean([p[0] for p in line["quad"]]) < 190 else "R"


def _key(line):
    return (tuple(map(tuple, line["quad"])), line["text"], tuple(tuple(map(tuple, w)) for w in line["words"]))


def test_ocr_lines_in_reading_order(dev, rec_model):
    from ocrs_models_amd import inference as inf

    page, det = _two_column_page(dev)
    plain = inf.ocr_lines(det, rec_model, page, size=PAGE)
    assert len(plain) == 2 * ROWS and all(len(g["words"]) == 3 and set(g) == {"quad", "text", "words"} for g in plain)
    assert [_side(g) for g in plain] == ["R", "L"] * ROWS  # today's list interleaves the columns
    read = inf.ocr_lines(det, rec_model, page, size=PAGE, reading_order=True)
    assert all(set(g) == {"quad", "text", "words", "block"} for g in read)
    assert [_side(g) for g in read] == ["L"] * ROWS + ["R"] * ROWS
    tops = [min(p[1] for p in g["quad"]) for g in read]
    assert tops[:ROWS] == sorted(tops[:ROWS]) and tops[ROWS:] == sorted(tops[ROWS:])  # each column top to bottom
    assert sorted(map(_key, plain)) == sorted(map(_key, read)) and len(set(map(_key, read))) == 2 * ROWS  # the same lines, crops and strings
    assert [g["block"] for g in read] == [0] * ROWS + [1] * ROWS
    assert inf.ocr_pages(det, rec_model, [page], size=PAGE, reading_order=True) == [read]
    assert inf.ocr_pages(det, rec_model, [page], size=PAGE) == [plain]
    text = inf.page_text(read)
    assert text == "\n".join(g["text"] for g in read[:ROWS]) + "\n\n" + "\n".join(g["text"] for g in read[ROWS:])
    numbered = inf.page_text([{**g, "text": f"line {k}"} for k, g in enumerate(read)])
    assert numbered.count("\n\n") == 1 and numbered.split("\n").count("") == 1 and len(numbered.split("\n")) == 2 * ROWS + 1  # exactly one blank line
    assert inf.page_text(plain) == "\n".join(g["text"] for g in plain) and inf.page_text([]) == ""
    # a tighter block_gap reaches the kernel through the driver: every line its own block
    apart = inf.ocr_lines(det, rec_model, page, size=PAGE, reading_order=True, block_gap=0.5)
    assert [g["block"] for g in apart] == list(range(2 * ROWS)) and [_key(g) for g in apart] == [_key(g) for g in read]


def test_reading_order_adds_no_wait_to_ocr_lines(dev, rec_model):
    from ocrs_models_amd import inference as inf

    page, det = _two_column_page(dev)
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        inf.ocr_lines(det, rec_model, page, size=PAGE), inf.ocr_lines(det, rec_model, page, size=PAGE, reading_order=True)
    plain, n_plain, what_plain = _count_waits(lambda: inf.ocr_lines(det, rec_model, page, size=PAGE))
    read, n_read, what_read = _count_waits(lambda: inf.ocr_lines(det, rec_model, page, size=PAGE, reading_order=True))
    print(f"host waits: ocr_lines {n_plain} {what_plain}, with reading_order {n_read} {what_read}")
    assert len(plain) == len(read) == 2 * ROWS and "block" in read[0]
    assert n_plain >= 3 and n_read <= n_plain


def test_ocr_pages_in_reading_order_of_two_pages(dev, rec_model):
    """page-wise order and blocks from one batch: the two-column page twice, the second time with a blank page before it"""
    from ocrs_models_amd import inference as inf
    from tests.test_ocr_batch_gpu import PaintedBatch

    page, det = _two_column_page(dev)
    blank = torch.full_like(page, 230)
    det_all = PaintedBatch(torch.stack([det.probs, torch.zeros_like(det.probs), det.probs])).eval()
    got = inf.ocr_pages(det_all, rec_model, [page, blank, page], size=PAGE, reading_order=True)
    assert [len(g) for g in got] == [2 * ROWS, 0, 2 * ROWS]
    for g in (got[0], got[2]):
        assert [_side(l) for l in g] == ["L"] * ROWS + ["R"] * ROWS and [l["block"] for l in g] == [0] * ROWS + [1] * ROWS
    plain = inf.ocr_pages(det_all, rec_model, [page, blank, page], size=PAGE)
    assert [sorted(map(_key, g)) for g in got] == [sorted(map(_key, g)) for g in plain]


# ------------------------------------------------------------------ CLI ----------------------------------------------------------------
def test_eval_detection_cli_prints_lines_in_reading_order(dev, rec_model, tmp_path):
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
    page_h = dot_page(800, 600)
    Image.fromarray(page_h[0].numpy()).save(tmp_path / "page.png")

    def start(base, *flags):
        return subprocess.Popen([sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"),
                                 str(tmp_path / base), "--rec-model", str(tmp_path / "rec.pt"), *flags], cwd=ROOT, stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)

    procs = [start("lines", "--lines"), start("read", "--lines", "--reading-order")]  # (side by side: two short-lived processes)
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
        outs.append([json.loads(line) for line in out.splitlines() if line.strip()])
    plain, read = outs
    assert plain and all(set(g) == {"quad", "text", "words"} for g in plain) and all(set(g) == {"quad", "text", "words", "block"} for g in read)
    assert sorted(map(_key, plain)) == sorted(map(_key, read))  # the same set of lines
    det_d = det.to(dev).eval()
    page = page_h.to(dev)
    assert read == inf.ocr_lines(det_d, rec_model, page, reading_order=True)  # in the new order
    assert os.path.exists(tmp_path / "read-text-lines.png")
    bad = subprocess.run([sys.executable, "-m", "ocrs_models_amd.eval_detection", "x", "y", "z", "--reading-order"], cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "--reading-order needs --lines" in bad.stderr

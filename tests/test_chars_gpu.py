"""Characters of recognised lines on the GPU (csrc/char_spans.hip; text.greedy_decode_spans, inference.char_boxes / word_chars and ``chars=True``
of the page drivers) against the numpy restatement of the rule (tests/chars_ref.py, pinned by tests/test_chars_host.py).

Spans.  Integers and bit copies: every written value must equal the restatement with ``==``, nothing past a row's length or outside the rows
of the call may be touched, and labels and lengths must be those of ``ocrs_ctc_greedy_decode`` on the same log-probs.

Boxes, exact.  Axis-aligned quads with integer corners below 4096 whose long side and output width are powers of two: a / ow, the product
with the long side and every term of P(s, r) are exact in fp32, so the result must equal the float32 restatement with ``==`` whatever the
compiler contracts.

Boxes, rotated.  Against the float64 restatement within 8 * ulp32(largest |coordinate|): counting as DESIGN.md §14 does for line quads, s
carries two roundings (the division and the product), a corner coordinate three (two products, two sums, of which the compiler may fuse one
pair), and u a relative error of a few 2^-24 (a sum of roundings, a square root, a division), all on magnitudes up to the largest coordinate
-- the bound the issue sets; the test prints the measured maximum (DESIGN.md §17 records it).

Words.  The centres c = 0.5f * (a / ow * long) sums are single fp32 operations in the kernel and in the float32 restatement alike, and for
axis-aligned integer words the projections are exact: ranges must equal the float32 restatement.  Rotated lines: characters are kept at
least 0.5 px from every boundary (asserted on the host in float64), then ranges must equal the float64 restatement.

End to end.  A painted detector (rows of bars) with a stub recogniser whose log-probs are prescribed, so text and positions are known; then
the golden detection and recognition weights, where the text is arbitrary and the properties are checked."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import chars_ref as R
from tests import lines_ref as LR
from tests import ocr_ref
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


# ------------------------------------------------------------------ spans ---------------------------------------------------------------
KINDS = ("all blank", "one class", "alternating classes", "alternating with blanks", "ties", "len 0", "len 1", "len T-1", "len T", "len T+5",
         "ends at 63, starts at 64", "random runs")


def _runs(T, C, rng):
    a = np.repeat(rng.randint(0, C, size=T), rng.randint(1, 9, size=T))[:T]
    assert len(a) == T
    return a


def _row(kind, T, C, rng):
    """-> (log-probs (T,C) float32 of one sample, its input length)"""
    lp = (rng.standard_normal((T, C)) - 3.0).astype(np.float32)
    in_len, a, t = T, None, np.arange(T)
    if kind == "all blank":
        a = np.zeros(T, dtype=int)
    elif kind == "one class":  # one run across every round boundary, its peak anywhere
        a = np.full(T, C - 1)
    elif kind == "alternating classes":  # T characters (with two classes there is only one to alternate with the blank)
        a = np.where(t % 2 == 0, 1, C - 1) if C > 2 else (t + 1) % 2
    elif kind == "alternating with blanks":
        a = np.where(t % 2 == 0, min(C - 1, 5), 0)
    elif kind == "ties":  # three values only: equal maxima in most rows, the first class must win
        lp = rng.randint(-2, 1, size=(T, C)).astype(np.float32)
    else:
        a = _runs(T, C, rng)
        in_len = {"len 0": 0, "len 1": 1, "len T-1": T - 1, "len T+5": T + 5}.get(kind, T)
        if kind.startswith("ends at 63") and T > 64:
            a[56:64], a[64:72] = 1, (C - 1 if C > 2 else 0)
            a[55] = 0
    if a is not None:
        lp[t, a] += 10.0
    return lp, in_len


@pytest.mark.parametrize("C", [2, 97])
@pytest.mark.parametrize("N", [1, 3, 65])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130, 209])
def test_spans_equal_the_restatement_and_the_greedy_decode(dev, T, N, C):
    from ocrs_models_amd import text

    rng = np.random.RandomState(1000 * T + 10 * N + C)
    row0, ld, rows = 2, T + 3, N + 5  # a non-zero first row, a pitch above T, rows behind the last one
    for first in range(0, len(KINDS), N):  # every kind of row at every shape: sample n is kind (first + n) % 12
        built = [_row(KINDS[(first + n) % len(KINDS)], T, C, rng) for n in range(N)]
        lp_h = np.stack([b[0] for b in built], axis=1)
        in_len = [b[1] for b in built]
        lp = torch.from_numpy(lp_h).to(dev)
        out = text.span_arrays(rows, ld, dev)
        out[0].fill_(SENT)
        assert text.greedy_decode_spans_async(lp, in_len, out, row0) is None
        buf = out[0].cpu().numpy()
        labels, t0, t1, peak_bits = (buf[k * rows * ld:(k + 1) * rows * ld].reshape(rows, ld) for k in range(4))
        peak, lens = peak_bits.view(np.float32), buf[4 * rows * ld:]
        ref = R.decode_spans(lp_h, in_len)
        greedy, _ = text.greedy_decode_batch(lp, in_len)
        for n in range(N):
            r, k = ref[n], len(ref[n]["labels"])
            kind = KINDS[(first + n) % len(KINDS)]
            assert lens[row0 + n] == k, (kind, n)
            assert labels[row0 + n, :k].tolist() == r["labels"] == greedy[n], (kind, n)
            assert t0[row0 + n, :k].tolist() == r["t0"] and t1[row0 + n, :k].tolist() == r["t1"], (kind, n)
            assert peak[row0 + n, :k].tobytes() == r["peak"].tobytes(), (kind, n)
            for arr in (labels, t0, t1, peak_bits):  # nothing past the length
                assert (arr[row0 + n, k:] == SENT).all(), (kind, n)
            if kind == "alternating classes" and C > 2:
                assert k == T
            if kind == "one class":
                assert k == 1 and r["t1"] == [T - 1]
        outside = [i for i in range(rows) if not row0 <= i < row0 + N]
        for arr in (labels, t0, t1, peak_bits):  # nor in the rows of other calls
            assert (arr[outside] == SENT).all()
        assert (lens[outside] == SENT).all()
        # arrays of its own: the same values through the handle
        own = text.greedy_decode_spans(lp, in_len)
        for n in range(N):
            assert own[n]["labels"] == ref[n]["labels"] and own[n]["t0"] == ref[n]["t0"] and own[n]["t1"] == ref[n]["t1"]
            assert np.array(own[n]["peak"], dtype=np.float32).tobytes() == ref[n]["peak"].tobytes()


def test_spans_arguments(dev):
    from ocrs_models_amd import text

    lp = torch.zeros(5, 2, 3, device=dev)
    with pytest.raises(RuntimeError):
        text.greedy_decode_spans_async(torch.zeros(5, 2, 3), [5, 5])  # no CPU path
    with pytest.raises(RuntimeError):
        text.greedy_decode_spans_async(lp, [5, 5], text.span_arrays(2, 4, dev), 0)  # pitch below T
    with pytest.raises(RuntimeError):
        text.greedy_decode_spans_async(lp, [5, 5], text.span_arrays(2, 5, dev), 1)  # rows past the arrays
    assert text.greedy_decode_spans(torch.zeros(5, 0, 3, device=dev), []) == []  # no samples: no launch


# ------------------------------------------------------------------ boxes ---------------------------------------------------------------
def _spans_from_host(dev, rows, ld, per_row):
    """CharSpans with the given per-row dicts (labels, t0, t1, optional peak), everything else the sentinel"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text

    spans = inf.CharSpans(*text.span_arrays(rows, ld, dev))
    host = np.full(4 * rows * ld + rows, SENT, dtype=np.int32)
    parts = [host[k * rows * ld:(k + 1) * rows * ld].reshape(rows, ld) for k in range(4)]
    for p, r in enumerate(per_row):
        k = len(r["labels"])
        assert k <= ld
        parts[0][p, :k], parts[1][p, :k], parts[2][p, :k] = r["labels"], r["t0"], r["t1"]
        parts[3].view(np.float32)[p, :k] = r.get("peak", np.zeros(k, np.float32))
        host[4 * rows * ld + p] = k
    spans.buf.copy_(torch.from_numpy(host))
    return spans


def _random_chars(ow, rng, space=1, nlabels=6):
    """characters over the ow // 4 steps of a crop: runs of 1..4 steps, 0..3 blank steps apart; labels 1..nlabels, about a third spaces"""
    Ti, t, out = ow // 4, 0, {"labels": [], "t0": [], "t1": []}
    while True:
        t += int(rng.randint(0, 4))
        e = t + int(rng.randint(0, 4))
        if e >= Ti:
            return out
        out["labels"].append(space if rng.rand() < 0.3 else int(rng.randint(2, nlabels + 1)))
        out["t0"].append(t), out["t1"].append(e)
        t = e + 1


def _boxes_case(dev, quads_h, seed):
    """crop plan and random characters for the quads -> (plan table on the host, per-quad chars, CharBoxes on the host as numpy, ld)"""
    from ocrs_models_amd import inference as inf

    q = torch.from_numpy(np.ascontiguousarray(quads_h, dtype=np.float32)).to(dev)
    plan = inf.crop_plan(q)
    n = plan.host()[0]
    table = plan.table.cpu().numpy()
    rng = np.random.RandomState(seed)
    chars = [_random_chars(int(table[i, 2]), rng) for i in range(n)]
    ld = max(len(c["labels"]) for c in chars) + 2
    spans = _spans_from_host(dev, n, ld, [chars[int(table[p, 7])] for p in range(n)])
    out = inf.CharBoxes(torch.full((n, ld), float(SENT), device=dev), torch.full((n, ld), float(SENT), device=dev), torch.full((n, ld, 4, 2), float(SENT), device=dev))
    fresh = inf.char_boxes(q, plan, spans)
    from ocrs_models_amd._lib import lib, ptr
    lib().char_boxes(ptr(q), ptr(plan.table), n, n, ld, ptr(spans.lens), ptr(spans.t0), ptr(spans.t1), ptr(out.s0), ptr(out.s1), ptr(out.quads))
    got = {k: getattr(out, k).cpu().numpy() for k in ("s0", "s1", "quads")}
    for i in range(n):  # tensors of its own: the same values wherever they are defined; nothing past a row's length is written
        p, k = int(table[i, 6]), len(chars[i]["labels"])
        for name in got:
            assert np.array_equal(getattr(fresh, name)[p, :k].cpu().numpy(), got[name][p, :k])
            assert (got[name][p, k:] == SENT).all()
    return table, chars, got


def test_boxes_exact(dev):
    quads = np.stack([LR.box(100, 200, 256, 64), LR.box(7, 900, 256, 32), LR.box(1024, 2048, 512, 128), LR.box(3000, 100, 64, 256),
                      LR.box(0, 0, 256, 64), LR.box(3500, 3900, 512, 128)])
    assert quads.max() < 4096 and (quads == np.rint(quads)).all()
    table, chars, got = _boxes_case(dev, quads, seed=5)
    assert table[:, 2].tolist() == [256, 512, 256, 256, 256, 256]
    for i, q in enumerate(quads):
        p, c = int(table[i, 6]), chars[i]
        k = len(c["labels"])
        assert k > 5
        ref = R.char_boxes(q, int(table[i, 2]), c["t0"], c["t1"], np.float32)
        assert np.array_equal(got["s0"][p, :k], ref["s0"]) and np.array_equal(got["s1"][p, :k], ref["s1"])
        assert ref["quads"].dtype == np.float32 and np.array_equal(got["quads"][p, :k], ref["quads"])
        a0, a1 = R.char_extent(c["t0"], c["t1"], int(table[i, 2]))
        assert (a0 < a1).all() and a0[0] >= 0
    # the vertical crop: characters run down the page from the top right corner
    v = got["quads"][int(table[3, 6])]
    assert v[0, 0].tolist()[0] == 3064.0 and v[0, 3].tolist()[0] == 3000.0 and v[0, 1][1] > v[0, 0][1]


def test_boxes_rotated_against_float64(dev):
    rng = np.random.RandomState(3)
    quads = np.stack([LR.rotated_rect(rng.uniform(400, 3500), rng.uniform(400, 3500), rng.uniform(60, 700), rng.uniform(12, 60), deg)
                      for deg in (-80, -47, -20, -5, -1, 0.5, 3, 10, 31, 45, 62, 89) for _ in range(3)])
    table, chars, got = _boxes_case(dev, quads, seed=6)
    top = float(np.abs(quads).max())
    bound, worst = 8 * R.ulp32(top), 0.0
    for i, q in enumerate(quads):
        p, c = int(table[i, 6]), chars[i]
        k = len(c["labels"])
        ref = R.char_boxes(q, int(table[i, 2]), c["t0"], c["t1"], np.float64)
        worst = max(worst, float(np.abs(got["quads"][p, :k].astype(np.float64) - ref["quads"]).max()))
        assert np.abs(got["s0"][p, :k] - ref["s0"]).max() <= bound and np.abs(got["s1"][p, :k] - ref["s1"]).max() <= bound
    print(f"rotated character boxes: {len(quads)} crops, max corner error {worst:.3e} = {worst / R.ulp32(top):.2f} ulp32({top:.1f}), bound {bound:.3e}")
    assert worst <= bound


# ------------------------------------------------------------------ words ---------------------------------------------------------------
def _words_case(dev, lines, words_h, seed, dtype=np.float32, min_margin=None):
    """random characters for every line of ``lines`` (device TextLines over ``words_h``), char_boxes + word_chars on the device, and the
    restatement in ``dtype`` line by line.  ``min_margin``: characters nearer than that to a boundary (float64) are left out first."""
    from ocrs_models_amd import inference as inf

    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    L = plan.host()[0]
    table = plan.table.cpu().numpy()
    lq, order, offs = lines.quads.cpu().numpy(), lines.word_order.cpu().numpy(), lines.line_offsets.cpu().numpy()
    rng = np.random.RandomState(seed)
    chars, chains = [], [order[offs[l]:offs[l + 1]] for l in range(L)]
    for l in range(L):
        c = _random_chars(int(table[l, 2]), rng)
        if min_margin is not None:
            r = R.line_words(lq[l], words_h[chains[l]], int(table[l, 2]), c["t0"], c["t1"], c["labels"], 1, np.float64)
            d = np.abs(r["centre"][:, None] - r["B"][None, :]).min(axis=1) if len(r["B"]) else np.full(len(c["labels"]), np.inf)
            c = {k: [v for v, keep in zip(c[k], d >= min_margin) if keep] for k in c}
        chars.append(c)
    ld = max(len(c["labels"]) for c in chars) + 1
    spans = _spans_from_host(dev, L, ld, [chars[int(table[p, 7])] for p in range(L)])
    boxes = inf.char_boxes(lines.quads, plan, spans)
    n = len(words_h)
    alphabet = " abcdefgh"  # the space is label 1
    got = inf.word_chars(lines, plan, spans, boxes, alphabet).cpu().numpy()
    assert got.shape == (n, 2)
    again = inf.word_chars(lines, plan, spans, boxes, alphabet).cpu().numpy()
    assert got.tobytes() == again.tobytes()  # (every word is in a line: every entry is written)
    untrimmed = inf.word_chars(lines, plan, spans, boxes, "abcdefgh").cpu().numpy()
    margin, empty, trimmed = np.inf, 0, 0
    for l in range(L):
        c, ow = chars[l], int(table[l, 2])
        r = R.line_words(lq[l], words_h[chains[l]], ow, c["t0"], c["t1"], c["labels"], 1, dtype)
        assert np.array_equal(got[chains[l]], r["ranges"]), (l, got[chains[l]].tolist(), r["ranges"].tolist())
        raw = R.word_ranges(r["B"], r["centre"], c["labels"], -1)
        assert np.array_equal(untrimmed[chains[l]], raw), l
        assert raw[0, 0] == 0 and raw[-1, 1] == len(c["labels"]) and (raw[1:, 0] == raw[:-1, 1]).all()  # untrimmed ranges tile the line
        if dtype == np.float32:
            p, k = int(table[l, 6]), len(c["labels"])
            assert np.array_equal(boxes.s0[p, :k].cpu().numpy(), r["s0"]) and np.array_equal(boxes.s1[p, :k].cpu().numpy(), r["s1"])
        margin = min(margin, r["margin"])
        empty += int((r["ranges"][:, 0] == r["ranges"][:, 1]).sum())
        trimmed += int((raw != r["ranges"]).any(axis=1).sum())
    return {"L": L, "margin": margin, "empty": empty, "trimmed": trimmed, "chains": chains}


def _chain(n, w, h, gap):
    q = np.stack(LR.row_of_words(3, 5, n, w, h, gap))
    assert q.max() < 4096
    return q


WORDS_EXACT = {
    "1 word": lambda: (LR.box(10, 20, 250, 20)[None], 1),
    "2 words": lambda: (np.stack(LR.row_of_words(0, 0, 2, 120, 30, 20)), 2),
    "64 words": lambda: (_chain(64, 40, 14, 10), 64),
    "65 words": lambda: (_chain(65, 40, 14, 10), 65),
    "300 words": lambda: (_chain(300, 9, 4, 4), 300),
    "300 words, shuffled": lambda: (_chain(300, 9, 4, 4)[np.random.RandomState(8).permutation(300)], 300),
    "64 lines of 5, shuffled": lambda: (LR.grid_case(64, 5, seed=6), 5),
    "tall words down the page": lambda: (np.stack([LR.box(0, 80 * k, 20, 60) for k in range(4)])[::-1].copy(), 4),
}


@pytest.mark.parametrize("name", list(WORDS_EXACT))
def test_words_exact_cases_equal_the_float32_restatement(dev, name):
    from ocrs_models_amd import inference as inf

    words, longest = WORDS_EXACT[name]()
    assert words.max() < 4096 and (words == np.rint(words)).all()
    lines = inf.find_lines(torch.from_numpy(words).to(dev))
    r = _words_case(dev, lines, words, seed=len(name))
    assert max(len(c) for c in r["chains"]) == longest
    print(f"{name}: {r['L']} lines, {r['empty']} empty ranges, {r['trimmed']} trimmed")
    if longest >= 64:
        assert r["empty"] > 0 and r["trimmed"] > 0


def test_words_of_two_pages(dev):
    from ocrs_models_amd import inference as inf

    per_page = [LR.grid_case(9, 7, seed=3), LR.grid_case(12, 20, seed=5)]
    words = np.concatenate(per_page)
    q = torch.from_numpy(words).to(dev)
    pow_ = torch.tensor([0] * len(per_page[0]) + [1] * len(per_page[1]), dtype=torch.int32, device=dev)
    offs = torch.tensor([0, len(per_page[0]), len(words)], dtype=torch.int32, device=dev)
    lines = inf.find_lines_pages(q, pow_, offs)
    r = _words_case(dev, lines, words, seed=12)
    assert r["L"] == 21 and sorted(len(c) for c in r["chains"]) == [7] * 9 + [20] * 12
    assert min(int(c.min()) for c in r["chains"][9:]) == len(per_page[0])  # the second page's ranges sit at its flat word indices


def test_words_of_rotated_lines_against_float64(dev):
    from ocrs_models_amd import inference as inf

    words = LR.rotated_case()
    lines = inf.find_lines(torch.from_numpy(words).to(dev))
    r = _words_case(dev, lines, words, seed=4, dtype=np.float64, min_margin=0.5)
    print(f"rotated lines: {r['L']} lines, longest chain {max(len(c) for c in r['chains'])}, smallest |centre - boundary| {r['margin']:.3f} px")
    assert r["margin"] >= 0.5 and max(len(c) for c in r["chains"]) == 7


def test_stage_arguments(dev):
    from ocrs_models_amd import inference as inf

    words = LR.grid_case(3, 4)
    q = torch.from_numpy(words).to(dev)
    lines = inf.find_lines(q)
    assert lines.words is not None and torch.equal(lines.words, q)
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    spans = _spans_from_host(dev, 3, 4, [{"labels": [2], "t0": [1], "t1": [2]}] * 3)
    boxes = inf.char_boxes(lines.quads, plan, spans)
    with pytest.raises(RuntimeError):
        inf.char_boxes(lines.quads[:5], plan, spans)  # not the quads of the plan
    with pytest.raises(RuntimeError):
        inf.word_chars(inf.TextLines(*[getattr(lines, k) for k in ("quads", "n_lines", "line_of_word", "word_order", "line_offsets", "next_word")]), plan, spans,
                       boxes)  # lines that do not know their words
    with pytest.raises(RuntimeError):
        inf.word_chars(lines, plan, spans, inf.CharBoxes(boxes.s0[:2], boxes.s1[:2], boxes.quads[:2]))
    assert inf.space_label(" ab") == 1 and inf.space_label("ab") == -1


# ------------------------------------------------------------------ end to end: painted detector, stub recogniser ----------------------------
class Stub(torch.nn.Module):
    """a recogniser whose log-probs are prescribed: (n,1,64,Wpad) -> (Wpad // 4 + 1, n, C), the same for every sample: class ``c`` wins the
    steps t0..t1 of each ``(t0, t1, c, value)`` with ``value`` at step (t0 + t1) // 2 and less on either side, the blank everywhere else"""

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
            assert 0 <= t0 <= t1
            if t1 < T:  # (a narrower batch than the one the steps were laid out for: what does not fit is not said)
                lp[t0:t1 + 1, :, c] = value - 0.125
                lp[(t0 + t1) // 2, :, c] = value
        return lp


def test_prescribed_text_lands_in_the_words_it_lies_over(dev):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    rows, cols = 4, 3
    bars = [(15 + 52 * c, 18 + 40 * r, 40, 12) for r in range(rows) for c in range(cols)]  # 12 apart: 6 after the expansion
    page, det = TL.bar_page(190, 200, bars, dev)
    size = (190, 200)
    # the geometry the drivers will see, staged by hand: every row is one line of three words with the same extents along the line
    found = inf.detect_words(det, page, size=size)
    lines = inf.find_lines(found["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    assert plan.host()[0] == rows
    table, lq, wq = plan.table.cpu().numpy(), lines.quads.cpu().numpy(), found["quads"].cpu().numpy()
    order, offs = lines.word_order.cpu().numpy(), lines.line_offsets.cpu().numpy()
    ow = int(table[0, 2])
    assert (table[:rows, 2] == ow).all() and ow < 800
    wb = R.word_bounds(lq[0], wq[order[offs[0]:offs[1]]], np.float64)
    lng = float(ocr_ref.crop_frame(lq[0])["long"])
    lo, hi = wb["lo"], wb["hi"]
    assert len(lo) == 3 and lo[1] - hi[0] > 3 and lo[2] - hi[1] > 3
    # "ab c def": a space at the end of the first word, none between the second and the third, one inside the second word
    where = [("a", lo[0] + 0.25 * (hi[0] - lo[0])), ("b", lo[0] + 0.7 * (hi[0] - lo[0])), (" ", hi[0] - 1.0),
             ("c", lo[1] + 0.2 * (hi[1] - lo[1])), (" ", lo[1] + 0.5 * (hi[1] - lo[1])), ("d", lo[1] + 0.85 * (hi[1] - lo[1])),
             ("e", lo[2] + 0.1 * (hi[2] - lo[2])), ("f", lo[2] + 0.7 * (hi[2] - lo[2]))]
    steps = [int(round(s / lng * ow / 4)) for _, s in where]
    assert all(b - a >= 4 for a, b in zip(steps, steps[1:])) and steps[0] >= 1 and steps[-1] + 1 < ow // 4
    values = [-(k + 1) / 64 for k in range(len(where))]
    stub = Stub([(t - 1, t + 1, DEFAULT_ALPHABET.index(ch) + 1, v) for (ch, _), t, v in zip(where, steps, values)], len(DEFAULT_ALPHABET) + 1).eval()
    # the centre of step t on the line, against the boundaries: which word the rule gives each character
    centres = np.array([4 * t / ow * lng for t in steps])
    assert [int((wb["B"] <= c).sum()) for c in centres] == [0, 0, 0, 1, 1, 1, 2, 2] and np.abs(centres[:, None] - wb["B"][None, :]).min() > 1.0

    got = inf.ocr_lines(det, stub, page, size=size, chars=True)
    plain = inf.ocr_lines(det, stub, page, size=size)
    assert len(got) == rows
    for g, pl in zip(got, plain):
        assert set(g) == {"quad", "text", "words", "char_quads", "char_log_probs", "word_chars", "word_texts"}
        assert {k: g[k] for k in pl} == pl
        assert g["text"] == "ab c def" and g["word_texts"] == ["ab", "c d", "ef"] and g["word_chars"] == [[0, 2], [3, 6], [6, 8]]
        assert g["char_log_probs"] == values  # the peak of every run, untouched
        assert len(g["char_quads"]) == 8
        for k, word in ((0, 0), (1, 0), (3, 1), (5, 1), (6, 2), (7, 2)):  # every letter sits over its word
            cx = np.mean([p[0] for p in g["char_quads"][k]])
            xs = [p[0] for p in g["words"][word]]
            assert min(xs) < cx < max(xs), (k, word)
        ys = [p[1] for q in g["char_quads"] for p in q]
        assert abs(min(ys) - min(p[1] for p in g["quad"])) < 1e-3 and abs(max(ys) - max(p[1] for p in g["quad"])) < 1e-3  # the line's own height
    # word crops see the same log-probs, cut at their own length: the keys of ocr_page, one quad per character
    words = inf.ocr_page(det, stub, page, size=size, chars=True)
    assert len(words) == rows * cols and all(set(w) == {"quad", "text", "char_quads", "char_log_probs"} for w in words)
    assert all(len(w["char_quads"]) == len(w["text"]) == len(w["char_log_probs"]) > 0 for w in words)


# ------------------------------------------------------------------ end to end: golden weights ----------------------------------------------
SIZE = (160, 120)


@pytest.fixture(scope="module")
def golden(dev, det_model, rec_model):
    from ocrs_models_amd import inference as inf

    page = TL.dot_page(320, 240).to(dev)
    return page, inf.ocr_lines(det_model, rec_model, page, size=SIZE), inf.ocr_lines(det_model, rec_model, page, size=SIZE, chars=True)


def test_chars_keep_every_key_and_add_theirs(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, plain, chars = golden
    assert len(plain) == len(chars) > 0
    for a, b in zip(plain, chars):
        assert set(b) == set(a) | {"char_quads", "char_log_probs", "word_chars", "word_texts"}
        assert {k: b[k] for k in a} == a
        assert len(b["char_quads"]) == len(b["char_log_probs"]) == len(b["text"])
        assert all(np.asarray(q).shape == (4, 2) for q in b["char_quads"]) and all(isinstance(v, float) and v <= 0.0 for v in b["char_log_probs"])
        assert len(b["word_chars"]) == len(b["word_texts"]) == len(b["words"])
        assert [b["text"][s:e] for s, e in b["word_chars"]] == b["word_texts"]
    print(f"golden models: {len(chars)} lines, {sum(len(b['text']) for b in chars)} characters, {sum(len(b['words']) for b in chars)} words")
    # word mode, reading order and page batches carry the same keys with the same values
    wp, wc = inf.ocr_page(det_model, rec_model, page, size=SIZE), inf.ocr_page(det_model, rec_model, page, size=SIZE, chars=True)
    assert [{k: c[k] for k in p} for p, c in zip(wp, wc)] == wp and all(len(c["char_quads"]) == len(c["text"]) for c in wc)
    ro = inf.ocr_lines(det_model, rec_model, page, size=SIZE, reading_order=True, chars=True)
    assert ro == [{**chars[chars.index({k: v for k, v in d.items() if k != "block"})], "block": d["block"]} for d in ro] and len(ro) == len(chars)
    assert inf.ocr_pages(det_model, rec_model, [page], size=SIZE, chars=True) == [chars]
    assert inf.ocr_pages(det_model, rec_model, [page], lines=False, size=SIZE, chars=True) == [wc]
    pages = inf.ocr_pages(det_model, rec_model, [page, page[:, :200].contiguous()], size=SIZE, chars=True)
    plain_pages = inf.ocr_pages(det_model, rec_model, [page, page[:, :200].contiguous()], size=SIZE)
    assert [[{k: c[k] for k in p} for p, c in zip(pp, pc)] for pp, pc in zip(plain_pages, pages)] == plain_pages
    assert all([c["text"][s:e] for s, e in c["word_chars"]] == c["word_texts"] for pc in pages for c in pc)


def test_ranges_ascend_and_cover_every_non_space_character(golden):
    _, _, chars = golden
    for b in chars:
        covered, last = set(), 0
        for s, e in b["word_chars"]:
            assert last <= s <= e <= len(b["text"])
            covered.update(range(s, e))
            last = e
        assert all(ch == " " for k, ch in enumerate(b["text"]) if k not in covered)
        assert all(t == t.strip(" ") for t in b["word_texts"])


def test_character_quads_lie_within_their_line(golden):
    _, _, chars = golden
    worst = 0.0
    for b in chars:
        f = ocr_ref.crop_frame(b["quad"], np.float64)
        eps = 8 * R.ulp32(float(np.abs(np.asarray(b["quad"])).max()))
        pts = np.asarray(b["char_quads"], dtype=np.float64).reshape(-1, 2) - f["origin"]
        if not len(pts):
            continue
        s, r = pts @ f["u"], pts @ f["v"]
        out = max(-s.min(), s.max() - f["long"], -r.min(), r.max() - f["short"])
        worst = max(worst, out / eps)
        assert out <= eps, (out, eps)
    print(f"character corners outside their line quad: at most {worst:.2f} of the bound")


def test_ocr_lines_with_chars_equals_the_stages_chained_by_hand(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, _, chars = golden
    det = inf.detect_words(det_model, page, size=SIZE)
    lines = inf.find_lines(det["quads"])
    plan = inf.crop_plan(lines.quads, count=lines.n_lines)
    batches = inf.crops_to_batches(inf.rectify_crops(page, lines.quads, plan), plan)
    texts, spans = inf.recognize_crops(rec_model, batches, chars=True)
    assert texts == inf.recognize_crops(rec_model, batches) == [c["text"] for c in chars]
    boxes = inf.char_boxes(lines.quads, plan, spans)
    sorted_texts, per_row, ranges = inf.chars_to_host(spans, boxes, ranges=inf.word_chars(lines, plan, spans, boxes))
    perm, order, offs = batches[2], lines.word_order.cpu().tolist(), lines.line_offsets.cpu().tolist()
    for l, c in enumerate(chars):
        assert sorted_texts[perm[l]] == c["text"]
        assert per_row[perm[l]] == {"char_quads": c["char_quads"], "char_log_probs": c["char_log_probs"]}
        assert [ranges[i] for i in order[offs[l]:offs[l + 1]]] == c["word_chars"]
    # and they are the rule's: spans of the recogniser's own log-probs; ranges by the restatement wherever these unconstructed quads keep every
    # centre a thousandth of a pixel from every boundary (float64), so that the last bits of a projection cannot decide
    table, lq, wq = plan.table.cpu().numpy(), lines.quads.cpu().numpy(), det["quads"].cpu().numpy()
    with torch.inference_mode():
        lp = rec_model(batches[0][0])
    ref = R.decode_spans(lp.cpu().numpy(), batches[1][0].div(4, rounding_mode="floor").tolist())
    compared = 0
    for p, r in enumerate(ref):
        l = int(table[p, 7])
        assert inf.decode_text(r["labels"], list(inf.DEFAULT_ALPHABET)) == chars[l]["text"]
        assert [float(v) for v in r["peak"]] == chars[l]["char_log_probs"]
        w = R.line_words(lq[l], wq[order[offs[l]:offs[l + 1]]], int(table[l, 2]), r["t0"], r["t1"], r["labels"], 1, np.float64)
        if w["margin"] > 1e-3:
            compared += 1
            assert w["ranges"].tolist() == chars[l]["word_chars"], l
    print(f"{compared} of {len(ref)} lines compared with the restatement's ranges")
    assert compared > 0


def test_chars_add_no_host_wait(dev, rec_model):
    """the boxes and the word ranges are queued behind the decodes and copied with the labels: the three waits stay three.  Counted the way
    tests/test_lines_gpu.py counts them, on a page with one chunk of crops."""
    from ocrs_models_amd import inference as inf

    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)]
    page, det = TL.bar_page(230, 340, bars, dev)
    kw = dict(size=(230, 340))
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        inf.ocr_lines(det, rec_model, page, **kw), inf.ocr_lines(det, rec_model, page, chars=True, **kw), inf.ocr_page(det, rec_model, page, chars=True, **kw)
    plain, n_plain, what_plain = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, **kw))
    chars, n_chars, what_chars = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, chars=True, **kw))
    words, n_words, what_words = TL._count_waits(lambda: inf.ocr_page(det, rec_model, page, **kw))
    wchars, n_wchars, what_wchars = TL._count_waits(lambda: inf.ocr_page(det, rec_model, page, chars=True, **kw))
    print(f"host waits: ocr_lines {n_plain} {what_plain}, with chars {n_chars} {what_chars}; ocr_page {n_words}, with chars {n_wchars} {what_wchars}")
    assert len(plain) == len(chars) == 5 and len(words) == len(wchars) == 30
    assert n_plain >= 3 and n_chars == n_plain and n_wchars == n_words


def test_an_empty_page_with_chars(dev, det_model):
    from ocrs_models_amd import inference as inf

    class NeverCalled(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the recogniser must not run for a page without words")

    page = torch.full((1, 200, 160), 255, dtype=torch.uint8, device=dev)
    kw = dict(size=(128, 96), threshold=1.0, chars=True)
    assert inf.ocr_lines(det_model, NeverCalled().eval(), page, **kw) == []
    assert inf.ocr_page(det_model, NeverCalled().eval(), page, **kw) == []
    assert inf.ocr_pages(det_model, NeverCalled().eval(), [page, page], **kw) == [[], []]


def test_two_runs_give_identical_bytes(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, _, chars = golden
    again = inf.ocr_lines(det_model, rec_model, page, size=SIZE, chars=True)
    assert json.dumps(again) == json.dumps(chars)


# ------------------------------------------------------------------ CLI ----------------------------------------------------------------
def test_eval_detection_cli_with_chars(dev, det_model, rec_model, tmp_path):
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

    def run(base, *flags):
        r = subprocess.run([sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), base,
                            "--rec-model", str(tmp_path / "rec.pt"), *flags], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return [json.loads(line) for line in r.stdout.splitlines() if line.strip()]

    page = page_h.to(dev)
    got = run(str(tmp_path / "lines"), "--lines", "--chars")
    assert got and all(set(g) == {"quad", "text", "words", "char_quads", "char_log_probs", "word_chars", "word_texts"} for g in got)
    assert got == inf.ocr_lines(det_model, rec_model, page, chars=True)
    got = run(str(tmp_path / "words"), "--chars")
    assert got and all(set(g) == {"quad", "text", "char_quads", "char_log_probs"} for g in got)
    assert got == inf.ocr_page(det_model, rec_model, page, chars=True)

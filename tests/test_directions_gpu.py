"""Mixed directions on the GPU (csrc/line_dirs.hip; inference/directions.py and ``directions="mixed"`` of the drivers) against the numpy
restatement of the rule (tests/directions_ref.py, pinned by tests/test_directions_host.py).

The split follows the float32 restatement operation by operation, the flip is a permutation of elements and the flag one fp64 comparison:
all three are compared with ``==``.  End to end: the painted stand-in detector of tests/test_lines_gpu.py on a page of bars, where the rule's
decisions are kept 1.5 px from their thresholds, and the golden detection and recognition weights on a page of dots, where the driver must
equal its stages chained by hand.  Which way up the probe finds a line means nothing on untrained weights and is not asserted; how far the
two scores lie apart on real sideways text is not measured here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import directions_ref as D
from tests import lines_ref as LR
from tests import orient_ref as O
from tests import test_lines_gpu as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (160, 120)
SENT_F, SENT_I = -12345.0, -77


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


# ------------------------------------------------------------------ 1. the split ---------------------------------------------------------
def box(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float32)


def special_quads():
    """the 45 degree tie, the side-length tie, zero lengths and NaN (tests/test_directions_host.py pins what the restatement says of them)"""
    nan = np.float32(np.nan)
    tall_nan0, tall_nan2 = box(0, 0, 10, 40), box(0, 0, 10, 40)
    tall_nan0[0, 0], tall_nan2[2, 1] = nan, nan
    return np.stack([np.array([[0, 0], [16, 16], [14, 18], [-2, 2]], np.float32), np.array([[0, 0], [16, 17], [14, 19], [-2, 2]], np.float32),
                     np.array([[0, 0], [17, 16], [15, 18], [-2, 2]], np.float32), np.array([[0, 0], [-16, -17], [-14, -19], [2, -2]], np.float32),
                     box(0, 0, 10, 10), np.roll(box(0, 0, 10, 10), 1, axis=0), np.roll(box(0, 0, 10, 40), 1, axis=0), box(5, 5, 0, 0), box(0, 0, 0, 30),
                     box(0, 0, 30, 0), tall_nan0, tall_nan2, np.full((4, 2), nan, np.float32), box(0, 0, np.float32(np.inf), 3)])


def split_quads(n, kind, seed=0):
    r = np.random.RandomState(1000 * seed + n)
    x, y, lng, sht = r.uniform(0, 2000, n), r.uniform(0, 3000, n), r.uniform(45, 300, n), r.uniform(2, 40, n)
    if kind == "upright":
        return np.stack([box(x[k], y[k], lng[k], sht[k]) for k in range(n)])
    if kind == "sideways":
        return np.stack([box(x[k], y[k], sht[k], lng[k]) for k in range(n)])
    if kind == "alternating":
        return np.stack([box(x[k], y[k], lng[k], sht[k]) if k % 2 == 0 else box(x[k], y[k], sht[k], lng[k]) for k in range(n)])
    q = np.stack([LR.rotated_rect(x[k], y[k], lng[k], sht[k], r.uniform(0, 360)) for k in range(n)])
    q[::7] = np.roll(q[::7], 1, axis=1)  # the long side second
    if kind == "random with specials":
        sp = special_quads()
        q[r.choice(n, min(n, len(sp)), replace=False)] = sp[:min(n, len(sp))]
    return q


def _split_raw(dev, quads, H, W, count=None, cap=None):
    """``ocrs_axis_split`` into sentinel-filled buffers of ``cap`` rows -> the four outputs on the host"""
    from ocrs_models_amd._lib import lib, ptr

    n = len(quads)
    cap = n if cap is None else cap
    q = torch.zeros(cap, 4, 2, device=dev)
    q[:n] = torch.from_numpy(np.ascontiguousarray(quads)).to(dev)
    out = torch.full((cap + 2, 4, 2), SENT_F, device=dev)
    page = torch.full((cap + 2,), SENT_I, dtype=torch.int32, device=dev)
    src = torch.full((cap + 2,), SENT_I, dtype=torch.int32, device=dev)
    offs = torch.full((5,), SENT_I, dtype=torch.int32, device=dev)
    count_d = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    lib().axis_split(ptr(q), cap, ptr(count_d), H, W, ptr(out), ptr(page), ptr(offs), ptr(src))
    return out.cpu().numpy(), page.cpu().numpy(), offs.cpu().numpy(), src.cpu().numpy()


def _check_split(dev, quads, H, W, count=None, cap=None):
    out, page, offs, src = _split_raw(dev, quads, H, W, count, cap)
    padded = quads if cap is None else np.concatenate([quads, np.zeros((cap - len(quads), 4, 2), np.float32)])
    ref = D.axis_split(padded, H, W, count)
    m = int(ref["word_offs"][2])
    assert offs[:3].tolist() == ref["word_offs"].tolist() and (offs[3:] == SENT_I).all()
    assert out[:m].tobytes() == ref["quads"].tobytes()
    assert page[:m].tolist() == ref["page_of_word"].tolist() and src[:m].tolist() == ref["source_index"].tolist()
    assert sorted(src[:m].tolist()) == list(range(m))  # a permutation of the counted rows
    assert (out[m:] == SENT_F).all() and (page[m:] == SENT_I).all() and (src[m:] == SENT_I).all()  # nothing past the count, nothing past word_offs[2]
    return ref


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513, 2100])
def test_axis_split_equals_the_float32_restatement(dev, n):
    for kind in ("upright", "sideways", "alternating", "random", "random with specials"):
        ref = _check_split(dev, split_quads(n, kind), 3508, 2480)
        U = int(ref["word_offs"][1])
        assert U == {"upright": n, "sideways": 0, "alternating": (n + 1) // 2}.get(kind, U)
    if n >= 255:
        assert 0 < int(_check_split(dev, split_quads(n, "random", 3), 3508, 2480)["word_offs"][1]) < n


def test_axis_split_ties_zero_lengths_and_nan(dev):
    sp = special_quads()
    ref = _check_split(dev, sp, 100, 200)
    assert D.sideways(sp).tolist() == [False, True, False, True, False, False, True, False, True, False, False, False, False, False]
    assert ref["word_offs"].tolist() == [0, 10, 14] and ref["source_index"].tolist() == [0, 2, 4, 5, 7, 9, 10, 11, 12, 13, 1, 3, 6, 8]


@pytest.mark.parametrize("count", [0, 1, 256, 300, 700, 9999])
def test_axis_split_with_a_device_count_in_a_padded_buffer(dev, count):
    _check_split(dev, split_quads(700, "random with specials", 5), 3508, 2480, count=count, cap=1000)


@pytest.mark.parametrize("page", [(1, 1), (63, 65), (3508, 2480)], ids=lambda p: f"{p[0]}x{p[1]}")
def test_axis_split_turns_like_turn_quads_and_twice_alike_without_a_host_sync(dev, page):
    from ocrs_models_amd import inference as inf

    H, W = page
    q = torch.from_numpy(split_quads(1500, "random with specials", 9)).to(dev)
    count = torch.tensor([1234], dtype=torch.int32, device=dev)
    first = inf.split_by_axis(q, H, W)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = inf.split_by_axis(q, H, W)
        counted = inf.split_by_axis(q, H, W, count=count)
        nothing = inf.split_by_axis(q[:0], H, W)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for name in ("quads", "page_of_word", "word_offs", "source_index"):
        assert getattr(first, name).cpu().numpy().tobytes() == getattr(again, name).cpu().numpy().tobytes(), name
    _, U, m = first.word_offs.tolist()
    assert m == 1500 and 0 < U < m and counted.word_offs.tolist()[2] == 1234 and nothing.word_offs.tolist() == [0, 0, 0]
    src = first.source_index.long()
    assert first.quads[:U].cpu().numpy().tobytes() == q[src[:U]].cpu().numpy().tobytes()  # page 0: bit copies (the NaN quads among them)
    turned = inf.turn_quads(q[src[U:]].contiguous(), 1, H, W, inverse=True)
    assert first.quads[U:].cpu().numpy().tobytes() == turned.cpu().numpy().tobytes()  # page 1: the bits of turn_quads
    assert first.page_of_word.tolist() == [0] * U + [1] * (m - U)
    for bad in (lambda: inf.split_by_axis(q.cpu(), H, W), lambda: inf.split_by_axis(q.double(), H, W), lambda: inf.split_by_axis(q, 0, W),
                lambda: inf.split_by_axis(q, H, W, count=torch.tensor([3], device=dev))):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------ 2. the flip ----------------------------------------------------------
FLIP_SHAPES = [(n, OH, Wpad) for n in (1, 3, 65) for OH in (8, 64) for Wpad in (1, 37, 64, 192, 832)]


def _width_options(Wpad):
    return sorted({min(max(w, 1), Wpad) for w in (1, 2, 10, Wpad - 1, Wpad)})


def _cpu_flip(bits, widths, flags):
    """torch.flip of every flagged crop's valid span, on the CPU, on the int32 views"""
    want = bits.clone()
    for i, w in enumerate(widths):
        if flags is None or flags[i]:
            want[i, 0, :, :w] = torch.flip(bits[i, 0, :, :w], dims=(0, 1))
    return want


@pytest.mark.parametrize("shape", FLIP_SHAPES, ids=[f"{n}x{oh}x{w}" for n, oh, w in FLIP_SHAPES])
def test_flip_crops_is_the_flip_of_every_valid_span(dev, shape):
    from ocrs_models_amd import inference as inf

    n, OH, Wpad = shape
    numel, guard = n * OH * Wpad, 64
    g = torch.Generator().manual_seed(n * 100000 + OH * 1000 + Wpad)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 1, OH, Wpad), generator=g, dtype=torch.int64).to(torch.int32)  # any bit pattern, pad columns included
    options = _width_options(Wpad)
    for shift in range(len(options) if n <= 3 else 1):  # a batch shorter than the list of widths takes every width in turn
        widths = [options[(i + shift) % len(options)] for i in range(n)]
        widths_d = torch.tensor(widths, dtype=torch.int64, device=dev)
        for base in (0, 1):  # the batches start on a 16-byte boundary, and one float behind one
            src = torch.empty(numel + 8, dtype=torch.int32, device=dev)[base:base + numel].view(n, 1, OH, Wpad)
            src.copy_(bits)
            for flags in (None, [1] * n, [0] * n, [i % 2 for i in range(n)]):
                buf = torch.full((numel + guard + 8,), SENT_F, device=dev)
                out = buf[base:base + numel].view(n, 1, OH, Wpad)
                flags_d = None if flags is None else torch.tensor(flags, dtype=torch.int32, device=dev)
                got = inf.flip_crops(src.view(torch.float32), widths_d, flags_d, out=out)
                assert got is out
                assert torch.equal(out.view(torch.int32).cpu(), _cpu_flip(bits, widths, flags)), (shape, shift, base, flags)
                assert (buf[:base] == SENT_F).all() and (buf[base + numel:] == SENT_F).all(), (shape, shift, base, flags)
                back = inf.flip_crops(out, widths_d, flags_d)  # twice restores the bits (into a fresh, aligned tensor)
                assert torch.equal(back.view(torch.int32).cpu(), bits), (shape, shift, base, flags)


def test_flip_crops_argument_errors_and_no_host_sync(dev):
    from ocrs_models_amd import inference as inf

    batch = torch.randn(3, 1, 8, 12, device=dev)
    widths = torch.tensor([12, 5, 1], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = inf.flip_crops(batch, widths)
        flags = inf.flip_flags(torch.zeros(3, dtype=torch.float64, device=dev), torch.ones(3, dtype=torch.float64, device=dev), torch.ones(3, dtype=torch.int32, device=dev))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(got.cpu().numpy(), D.flip_crops(batch.cpu().numpy(), [12, 5, 1])) and flags.tolist() == [1, 1, 1]
    assert inf.flip_crops(batch[:0], widths[:0]).shape == (0, 1, 8, 12)
    for bad in (lambda: inf.flip_crops(batch.cpu(), widths), lambda: inf.flip_crops(batch, widths.int()), lambda: inf.flip_crops(batch, widths[:2]),
                lambda: inf.flip_crops(batch[:, 0], widths), lambda: inf.flip_crops(batch.double(), widths), lambda: inf.flip_crops(batch[..., ::2], widths),
                lambda: inf.flip_crops(batch, widths, torch.ones(3, device=dev)), lambda: inf.flip_crops(batch, widths, out=batch),
                lambda: inf.flip_crops(batch, widths, out=torch.empty(3, 1, 8, 13, device=dev))):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------ 3. the flags ---------------------------------------------------------
def test_flip_flags_equal_the_restatement(dev):
    from ocrs_models_amd import inference as inf

    r = np.random.RandomState(3)
    s_plain = r.uniform(-8, 0, 600)
    s_flip = r.uniform(-8, 0, 600)
    s_flip[::5] = s_plain[::5]                              # equal scores: no flip
    s_flip[1::50] = np.nextafter(s_plain[1::50], 0.0)       # one ulp larger: a flip
    s_flip[2::50] = np.nextafter(s_plain[2::50], -9.0)      # one ulp smaller
    s_plain[3::40], s_flip[4::40] = np.nan, np.nan
    s_plain[7], s_flip[7] = np.nan, np.nan
    probe = (r.uniform(0, 1, 600) < 0.6).astype(np.int32)
    probe[1::50], probe[11] = 1, 5
    want = D.flip_flags(s_plain, s_flip, probe)
    got = inf.flip_flags(*(torch.from_numpy(a).to(dev) for a in (s_plain, s_flip, probe)))
    assert got.dtype == torch.int32 and got.tolist() == want.tolist()
    larger_unprobed = (probe == 0) & (s_flip > s_plain)
    assert larger_unprobed.sum() > 50 and not want[larger_unprobed].any()  # unprobed lines whose flipped score is larger stay
    assert want[1::50].all() and not want[::5].any() and 100 < want.sum() < 300
    assert inf.flip_flags(*(torch.from_numpy(a[:0]).to(dev) for a in (s_plain, s_flip, probe))).shape == (0,)
    with pytest.raises(RuntimeError):
        inf.flip_flags(torch.zeros(2, device=dev), torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------ 4. the stages on painted bars ---------------------------------------
PAGE_H, PAGE_W = 290, 380
ROWS = [[(15 + 52 * c, 20 + 40 * r, 40, 12) for c in range(4)] for r in range(3)]            # three rows of four horizontal bars
COLUMNS = [[(260 - 2 * k, 20 + 52 * k, 12, 40) for k in range(4)],                           # drifts 2 px to the left per word: every d.x < 0
           [(330 - 3 * k, 27 + 52 * k, 12, 40) for k in range(4)]]                           # drifts 3 px, and starts 7 px lower (no two heads share c.y)
# (a column that stands exactly upright IS chained by the rule of DESIGN.md §14 -- its tie "d.x == 0 and d.y > 0" lets it through -- so both
# columns lean to the left: then no link of a column advances in x, and the rule cannot chain it even in principle)


@pytest.fixture(scope="module")
def bars(dev):
    flat = [b for row in ROWS for b in row] + [b for col in COLUMNS for b in col]
    page, det = TL.bar_page(PAGE_H, PAGE_W, flat, dev)
    return page, det


def _word_key(word):
    """which bar a word quad of a result is: its rounded centre"""
    c = np.mean(np.array(word, dtype=np.float64), axis=0)
    return (round(float(c[0]), 1), round(float(c[1]), 1))


def _bar_key(bar):
    x, y, w, h = bar
    return (round(x + (w - 1) / 2, 1), round(y + (h - 1) / 2, 1))


def test_the_bars_keep_every_decision_away_from_its_threshold(dev, bars):
    from ocrs_models_amd import inference as inf

    page, det = bars
    quads = inf.detect_words(det, page, size=(PAGE_H, PAGE_W))["quads"].cpu().numpy()
    assert len(quads) == 20
    split = D.axis_split(quads, PAGE_H, PAGE_W)
    assert split["word_offs"].tolist() == [0, 12, 20]
    e1, e2 = quads[:, 1] - quads[:, 0], quads[:, 2] - quads[:, 1]
    long_side = np.where((np.hypot(*e1.T) >= np.hypot(*e2.T))[:, None], e1, e2)
    assert (np.abs(np.abs(long_side[:, 1]) - np.abs(long_side[:, 0])) >= 1.5).all()  # the axis decision too: every long side is far from 45 degrees
    margins = {"as given": LR.decision_margin(quads), "page 0": LR.decision_margin(split["quads"][:12]), "page 1": LR.decision_margin(split["quads"][12:])}
    print("decision margins in px:", {k: round(v, 3) for k, v in margins.items()})
    assert all(m >= 1.5 for m in margins.values())
    # what the rule says: as given every vertical bar is a line of its own; on the turned page each column is one line
    assert sorted(len(c) for c in LR.find_lines(quads)["lines"]) == [1] * 8 + [4] * 3
    assert sorted(len(c) for c in LR.find_lines(split["quads"][12:])["lines"]) == [4, 4]
    straight = np.stack([box(100, 10 + 52 * k, 17, 45) for k in range(4)])  # the tie named above: an exactly upright column is one line already
    assert [len(c) for c in LR.find_lines(straight)["lines"]] == [4]


def test_without_directions_every_vertical_bar_is_a_line_of_its_own(dev, bars, rec_model):
    """the limit of DESIGN.md §14 that ``directions="mixed"`` lifts (this test passes without the feature too)"""
    from ocrs_models_amd import inference as inf

    page, det = bars
    lines = inf.ocr_lines(det, rec_model, page, size=(PAGE_H, PAGE_W))
    assert sorted(len(g["words"]) for g in lines) == [1] * 8 + [4] * 3
    vertical = {_bar_key(b) for col in COLUMNS for b in col}
    assert {_word_key(g["words"][0]) for g in lines if len(g["words"]) == 1} == vertical
    assert all(set(g) == {"quad", "text", "words"} for g in lines)


@pytest.mark.parametrize("rectify", ["quad", "chain"])
def test_mixed_reads_each_column_as_one_line(dev, bars, rec_model, rectify):
    from ocrs_models_amd import inference as inf

    page, det = bars
    kw = dict(size=(PAGE_H, PAGE_W), rectify=rectify)
    plain = inf.ocr_lines(det, rec_model, page, **kw)
    mixed = inf.ocr_lines(det, rec_model, page, directions="mixed", **kw)
    assert len(mixed) == 5 and [len(g["words"]) for g in mixed] == [4] * 5
    keys = ["quad", "text", "words"] + (["spine", "height"] if rectify == "chain" else []) + ["direction", "direction_scores"]
    assert all(list(g) == keys for g in mixed)
    # the horizontal rows first, in line order: the lines directions=None finds for those words.  (Their crops sit at other batch positions than
    # in the plain call, and nobody has pinned that the recogniser's text does not depend on that: the geometry is compared, the text is not.)
    rows = [p for p in plain if len(p["words"]) == 4]
    geometry = [k for k in keys if k not in ("text", "direction", "direction_scores")]
    assert [{k: g[k] for k in geometry} for g in mixed[:3]] == [{k: p[k] for k in geometry} for p in rows]
    assert all(g["direction"] == 0 and g["direction_scores"] is None for g in mixed[:3])
    for g, col in zip(mixed[3:], COLUMNS[::-1]):  # then the columns in the turned page's line order: by c.y there, which is descending x here
        assert g["direction"] in (1, 3) and isinstance(g["text"], str)
        s_plain, s_flip = g["direction_scores"]
        assert g["direction"] == (3 if s_flip > s_plain else 1) and np.isfinite([s_plain, s_flip]).all()
        top_down = [_bar_key(b) for b in col]
        assert [_word_key(w) for w in g["words"]] == (top_down if g["direction"] == 1 else top_down[::-1])
        q = np.array(g["quad"])
        xs, ys = [b[0] for b in col], [b[1] for b in col]
        assert q[:, 0].min() <= min(xs) - 2 and q[:, 0].max() >= max(xs) + 12 + 1 and q[:, 1].min() <= min(ys) - 2 and q[:, 1].max() >= max(ys) + 40 + 1
        if rectify == "chain":
            sy = [p[1] for p in g["spine"]]
            assert len(sy) == 8 and sy == sorted(sy, reverse=g["direction"] == 3)  # the spine runs in reading direction
    assert _word_key(mixed[3]["words"][0])[0] > _word_key(mixed[4]["words"][0])[0]
    for g in mixed:  # every quad lies on the page that was passed
        pts = np.array([p for key in geometry if key != "height" for p in np.array(g[key], dtype=np.float64).reshape(-1, 2)])
        assert (pts >= -4).all() and (pts[:, 0] <= PAGE_W + 3).all() and (pts[:, 1] <= PAGE_H + 3).all()
    assert inf.ocr_lines(det, rec_model, page, directions="mixed", **kw) == mixed  # and a second run gives the same


def test_mixed_with_reading_order_counts_blocks_on(dev, bars, rec_model):
    from ocrs_models_amd import inference as inf

    page, det = bars
    kw = dict(size=(PAGE_H, PAGE_W), reading_order=True)
    plain = [p for p in inf.ocr_lines(det, rec_model, page, **kw) if len(p["words"]) == 4]
    mixed = inf.ocr_lines(det, rec_model, page, directions="mixed", **kw)
    assert len(mixed) == 5 and all(list(g) == ["quad", "text", "words", "direction", "direction_scores", "block"] for g in mixed)
    assert [g["direction"] for g in mixed[:3]] == [0, 0, 0] and all(g["direction"] in (1, 3) for g in mixed[3:])
    assert [g["words"] for g in mixed[:3]] == [p["words"] for p in plain]
    blocks = [g["block"] for g in mixed]
    assert blocks[0] == 0 and all(b - a in (0, 1) for a, b in zip(blocks, blocks[1:]))  # from 0, no gaps, across the two groups
    assert blocks[3] == blocks[2] + 1  # the first sideways line starts a block of its own page


def test_a_page_without_sideways_words_is_the_plain_result(dev, rec_model):
    from ocrs_models_amd import inference as inf

    page, det = TL.bar_page(230, 340, [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)], dev)
    for kw in (dict(), dict(reading_order=True), dict(rectify="chain", beam_width=4)):
        plain = inf.ocr_lines(det, rec_model, page, size=(230, 340), **kw)
        mixed = inf.ocr_lines(det, rec_model, page, size=(230, 340), directions="mixed", **kw)
        want = [{**{k: v for k, v in p.items() if k != "block"}, "direction": 0, "direction_scores": None, **({"block": p["block"]} if "block" in p else {})}
                for p in plain]
        assert len(plain) == 5 and mixed == want and [list(m) for m in mixed] == [list(w) for w in want]


def test_the_driver_probes_the_sideways_crops_and_leaves_the_upright_ones(dev, bars, rec_model, monkeypatch):
    """what the driver hands to the probe and to the final read, recorded through the stage functions it calls: the probe mask against one
    derived without the plan's table (from the lines' pages and the host permutation), and the upright crops bit for bit as they were cut"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.inference import directions as dirs

    page, det = bars
    seen = {}
    probe_of, turn_of = dirs.line_directions, dirs.turn_flagged

    def recording_probe(rec, batches, widths, probe):
        seen.update(batches=[b.clone() for b in batches], probe=probe.clone())
        seen["flags"], seen["scores"] = probe_of(rec, batches, widths, probe)
        return seen["flags"], seen["scores"]

    def recording_turn(batches, widths, flags):
        seen["final"] = turn_of(batches, widths, flags)
        return seen["final"]

    monkeypatch.setattr(dirs, "line_directions", recording_probe)
    monkeypatch.setattr(dirs, "turn_flagged", recording_turn)
    mixed = inf.ocr_lines(det, rec_model, page, size=(PAGE_H, PAGE_W), directions="mixed")
    quads = inf.detect_words(det, page, size=(PAGE_H, PAGE_W))["quads"]
    split = inf.split_by_axis(quads, PAGE_H, PAGE_W)
    found = inf.find_lines_pages(split.quads, split.page_of_word, split.word_offs)
    plan = inf.crop_plan(found.quads, 64, found.n_lines)
    perm = plan.host_perm()
    assert len(perm) == 5 and found.page_of_line[:5].tolist() == [0, 0, 0, 1, 1]
    want = torch.zeros(5, dtype=torch.int32)
    want[torch.tensor(perm)] = found.page_of_line[:5].cpu()
    assert seen["probe"].cpu().tolist() == want.tolist() and sum(want.tolist()) == 2
    flags = seen["flags"].cpu()
    assert not flags[want == 0].any()
    assert [g["direction"] for g in mixed] == [0, 0, 0] + [3 if flags[perm[l]] else 1 for l in (3, 4)]
    rows = torch.cat([b.flatten(1) for b in seen["batches"]]), torch.cat([f.flatten(1) for f in seen["final"]])  # (one chunk: one padded width)
    upright_rows = (want == 0).to(dev)
    assert torch.equal(rows[0][upright_rows], rows[1][upright_rows])
    widths = inf.crops_to_batches(inf.rectify_crops_pages(*inf.pack_pages([page, inf.turn_page(page, 1)]), found.quads, found.page_of_line, plan), plan)[1]
    flipped = torch.from_numpy(D.flip_crops(seen["batches"][0].cpu().numpy(), widths[0].tolist(), flags.tolist())).to(dev)
    assert torch.equal(seen["final"][0], flipped)


def test_a_page_with_sideways_words_only(dev, rec_model):
    """virtual page 0 is empty: the split, the line stage, the plan and the results with no upright word at all"""
    from ocrs_models_amd import inference as inf

    flat = [b for col in COLUMNS for b in col]
    page, det = TL.bar_page(PAGE_H, PAGE_W, flat, dev)
    for kw in (dict(), dict(reading_order=True, rectify="chain")):
        mixed = inf.ocr_lines(det, rec_model, page, size=(PAGE_H, PAGE_W), directions="mixed", **kw)
        assert len(mixed) == 2 and [len(g["words"]) for g in mixed] == [4, 4] and all(g["direction"] in (1, 3) for g in mixed)
        for g, col in zip(mixed, COLUMNS[::-1]):
            top_down = [_bar_key(b) for b in col]
            assert [_word_key(w) for w in g["words"]] == (top_down if g["direction"] == 1 else top_down[::-1])
            assert g["direction"] == (3 if g["direction_scores"][1] > g["direction_scores"][0] else 1)
        if "reading_order" in kw:
            assert [g["block"] for g in mixed] == [0, 1] and list(mixed[0])[-3:] == ["direction", "direction_scores", "block"]
    two_d = inf.read_lines(rec_model, page[0], inf.detect_words(det, page, size=(PAGE_H, PAGE_W))["quads"], directions="mixed")
    assert two_d == inf.ocr_lines(det, rec_model, page, size=(PAGE_H, PAGE_W), directions="mixed")  # an (H,W) page, as the plain read_lines takes


# ------------------------------------------------------------------ 5. the driver against its stages ------------------------------------
def _mixed_by_hand(dev, det_model, rec_model, page, rectify="quad", reading_order=False, beam_width=None):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    H, W = page.shape[-2:]
    det = inf.detect_words(det_model, page, size=SIZE)
    split = inf.split_by_axis(det["quads"], H, W)
    found = inf.find_lines_pages(split.quads, split.page_of_word, split.word_offs)
    order = inf.reading_order(found) if reading_order else None
    store = inf.pack_pages([page, inf.turn_page(page, 1)])
    spines = None
    if rectify == "chain":
        spines = inf.line_spines(found)
        plan = inf.crop_plan_chain(spines, 64)
        packed = inf.rectify_chain_pages(*store, spines, found.page_of_line, plan)
    else:
        plan = inf.crop_plan(found.quads, 64, found.n_lines)
        packed = inf.rectify_crops_pages(*store, found.quads, found.page_of_line, plan)
    batches, widths, perm = inf.crops_to_batches(packed, plan)
    n = plan.host()[0]
    page_of_line = found.page_of_line[:n].cpu()
    probe = page_of_line[plan.table[:n, 7].cpu().long()].to(dev)
    by_perm = torch.zeros(n, dtype=torch.int32)  # the same mask without the plan's table: crop perm[l] is line l's
    by_perm[torch.tensor(perm)] = page_of_line
    assert torch.equal(by_perm, probe.cpu()) and int(by_perm.sum()) == n - found.line_page_offs.tolist()[1]
    flags, scores = inf.line_directions(rec_model, batches, widths, probe)
    assert not flags.cpu()[by_perm == 0].any()  # an upright line is never flipped, whatever its scores
    # the probe by its parts: the scores of both batches, the flag rule and the flip, each against its restatement
    with torch.inference_mode():
        s_plain = torch.cat([inf.path_confidence(rec_model(b), (w // 4).int()) for b, w in zip(batches, widths)])
        s_flip = torch.cat([inf.path_confidence(rec_model(torch.from_numpy(D.flip_crops(b.cpu().numpy(), w.tolist())).to(dev)), (w // 4).int())
                            for b, w in zip(batches, widths)])
    assert scores.cpu().numpy().tobytes() == torch.stack([s_plain, s_flip], dim=1).cpu().numpy().tobytes()
    assert flags.tolist() == D.flip_flags(s_plain.cpu().numpy(), s_flip.cpu().numpy(), probe.cpu().numpy()).tolist()
    final, row = [], 0
    for b, w in zip(batches, widths):
        final.append(torch.from_numpy(D.flip_crops(b.cpu().numpy(), w.tolist(), flags[row:row + len(w)].tolist())).to(dev))
        row += len(w)
    assert all(torch.equal(a, b) for a, b in zip(final, inf.turn_flagged(batches, widths, flags)))
    row = 0
    for f, b in zip(final, batches):  # the crops of upright lines reach the recogniser as they were cut
        upright_rows = (by_perm[row:row + len(b)] == 0).to(dev)
        assert torch.equal(f[upright_rows], b[upright_rows])
        row += len(b)
    lpo = found.line_page_offs.tolist()
    flat = inf._read_crops(rec_model, (final, widths, perm), DEFAULT_ALPHABET, split.quads, found, n, order, lpo, None, beam_width, None, spines)
    line_at = list(range(n)) if order is None else order.line_order[:n].tolist()
    flags_h, scores_h = flags.tolist(), scores.tolist()
    want = inf.mixed_results(flat, lpo, line_at, [flags_h[p] for p in perm], [scores_h[p] for p in perm], H, W)
    return want, dict(words=det["n"], upright=split.word_offs.tolist()[1], lines=n, upright_lines=lpo[1], flipped=int(sum(flags_h)))


@pytest.mark.parametrize("kw", [dict(), dict(rectify="chain"), dict(reading_order=True), dict(beam_width=4)], ids=["quad", "chain", "reading_order", "beam4"])
def test_ocr_lines_mixed_equals_the_stages_chained_by_hand(dev, det_model, rec_model, kw):
    from ocrs_models_amd import inference as inf

    page = TL.dot_page(320, 240).to(dev)
    want, seen = _mixed_by_hand(dev, det_model, rec_model, page, **kw)
    got = inf.ocr_lines(det_model, rec_model, page, size=SIZE, directions="mixed", **kw)
    print(f"golden weights {kw}: {seen}")
    assert seen["lines"] > 0 and len(got) == seen["lines"]
    assert json.dumps(got) == json.dumps(want)  # the same values under the same keys in the same order
    assert [g["direction"] for g in got[:seen["upright_lines"]]] == [0] * seen["upright_lines"]
    assert all(g["direction"] in (1, 3) for g in got[seen["upright_lines"]:])
    det = inf.detect_words(det_model, page, size=SIZE)
    assert inf.read_lines(rec_model, page, det["quads"], directions="mixed", **kw) == got


def test_orientation_composes_from_outside(dev, bars, rec_model):
    from ocrs_models_amd import inference as inf

    page, det = bars
    fed = inf.turn_page(page, 3)  # the page that arrives: one quarter turn counter-clockwise makes it upright
    assert torch.equal(inf.turn_page(fed, 1), page)
    upright = inf.ocr_lines(det, rec_model, page, size=(PAGE_H, PAGE_W), directions="mixed")
    got = inf.ocr_lines(det, rec_model, fed, size=(PAGE_H, PAGE_W), orientation=1, directions="mixed")
    assert got == O.turn_results(upright, 1, *fed.shape[-2:]) and len(got) == 5
    assert all(list(g) == ["quad", "text", "words", "direction", "direction_scores", "turns"] and g["turns"] == 1 for g in got)
    assert [g["direction"] for g in got] == [u["direction"] for u in upright]  # the directions are those of the upright page
    quads = inf.detect_words(det, page, size=(PAGE_H, PAGE_W))["quads"]
    assert inf.read_lines(rec_model, page, quads, orientation=1, directions="mixed") == got


# ------------------------------------------------------------------ 6. waits, errors, CLI ------------------------------------------------
def test_mixed_waits_no_more_often_than_the_plain_call(dev, bars, rec_model):
    """counted the way tests/test_lines_gpu.py counts them: the component count, the plan's totals, the labels"""
    from ocrs_models_amd import inference as inf

    page, det = bars
    kw = dict(size=(PAGE_H, PAGE_W))
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        inf.ocr_lines(det, rec_model, page, **kw), inf.ocr_lines(det, rec_model, page, directions="mixed", **kw)
        inf.ocr_lines(det, rec_model, page, directions="mixed", reading_order=True, rectify="chain", **kw)
    plain, n_plain, what_plain = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, **kw))
    mixed, n_mixed, what_mixed = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, directions="mixed", **kw))
    full, n_full, what_full = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, directions="mixed", reading_order=True, rectify="chain", **kw))
    print(f"host waits: plain {n_plain} {what_plain}, mixed {n_mixed} {what_mixed}, mixed with reading order and chain crops {n_full} {what_full}")
    assert len(plain) == 11 and len(mixed) == len(full) == 5
    assert n_plain >= 3 and n_mixed <= n_plain and n_full <= n_plain


def test_argument_errors_come_before_any_launch(dev, det_model, rec_model):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd._lib import lib

    page = TL.dot_page(320, 240).to(dev)
    quads = torch.from_numpy(np.stack([box(10, 10, 40, 10), box(100, 20, 10, 40)])).to(dev)
    L = lib()
    launched = []
    L.timing = {name: launched for name in ("axis_split", "flip_crops", "flip_flags", "turn_page_u8", "path_confidence", "crop_plan", "binarize_resize_nearest",
                                            "line_links", "line_links_pages")}
    try:
        for bad in ("Mixed", "vertical", True, 1, ["mixed"]):
            for call in (lambda: inf.ocr_lines(det_model, rec_model, page, size=SIZE, directions=bad),
                         lambda: inf.read_lines(rec_model, page, quads, directions=bad)):
                with pytest.raises(RuntimeError, match="directions must be None or"):
                    call()
        for call in (lambda: inf.ocr_lines(det_model, rec_model, page, size=SIZE, directions="mixed", chars=True),
                     lambda: inf.read_lines(rec_model, page, quads, directions="mixed", chars=True)):
            with pytest.raises(RuntimeError, match="does not go with chars"):
                call()
        with pytest.raises(RuntimeError):
            inf.read_lines(rec_model, page.transpose(1, 2), quads, directions="mixed")  # a page that is not contiguous
        with pytest.raises(TypeError):
            inf.ocr_pages(det_model, rec_model, [page], size=SIZE, directions="mixed")  # out of scope
        assert launched == []
    finally:
        L.timing = None


def test_eval_detection_cli_with_directions(dev, det_model, rec_model, tmp_path):
    import ocrs_models_amd as oa
    from ocrs_models_amd import eval_detection
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.checkpoint import save_checkpoint
    from PIL import Image

    det = oa.DetectionModel()
    det.load_state_dict(TL._golden_state("det"))
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    rec.load_state_dict(TL._golden_state("rec"))
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    save_checkpoint(str(tmp_path / "rec.pt"), rec, oa.optim.Adam(rec.parameters()), 0)
    page_h = TL.dot_page(400, 300)
    Image.fromarray(page_h[0].numpy()).save(tmp_path / "page.png")
    args = [str(tmp_path / "det.pt"), str(tmp_path / "page.png"), str(tmp_path / "out")]
    rec_args = ["--rec-model", str(tmp_path / "rec.pt")]
    for bad in ([*rec_args, "--directions", "mixed"], ["--lines", "--directions", "mixed"], [*rec_args, "--lines", "--directions", "vertical"],
                [*rec_args, "--lines", "--chars", "--directions", "mixed"]):  # refused by the argument parser, before any file is read
        with pytest.raises(SystemExit) as e:
            eval_detection.main([*args, *bad])
        assert e.value.code == 2
    r = subprocess.run([sys.executable, "-m", "ocrs_models_amd.eval_detection", *args, *rec_args, "--lines", "--directions", "mixed"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    want = inf.ocr_lines(det_model, rec_model, page_h.to(dev), directions="mixed")
    assert got and got == want and all(list(g) == ["quad", "text", "words", "direction", "direction_scores"] for g in got)

"""Orientation on the GPU (csrc/page_orient.hip; inference/orient.py and ``orientation=`` of the drivers) against the numpy restatement of the
rules (tests/orient_ref.py, pinned by tests/test_orient_host.py).

The turn is a permutation of bytes and the quad table one fp32 operation per coordinate: both are compared with ``==``.  The vote's counts and
picks are compared with ``==`` (the lengths are the restatement's float32 lengths bit by bit), its two sums within 1e-12 relative: they are
fp64 sums of at most a few thousand fp32 lengths, so only the summation tree differs.  The path confidence is compared within
1e-12 * max(1, |ref|): exact maxima, an fp64 sum of at most 101 terms of magnitude below 20.

End to end: the golden detection and recognition weights on a page of dots, as tests/test_chain_gpu.py.  These tests pin the rule and the
mechanics; how well the rule separates real pages is not measured here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ocr_ref as R
from tests import orient_ref as O
from tests import test_lines_gpu as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (160, 120)
SENT_F, SENT_B = -12345.0, 0xA5
VOTE_RTOL, SCORE_TOL = 1e-12, 1e-12


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


class DarkIsText(torch.nn.Module):
    """a detector that needs no weights and fits a page any way up: dark pixels are text"""

    def forward(self, x):
        return (x < 0).float() * 0.9


class NeverCalled(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("the recogniser must not run")


def _ramp_page(H, W, seed=0):
    """a byte ramp plus noise: neighbouring pixels differ in both directions and no two rows or columns are alike"""
    y, x = np.mgrid[0:H, 0:W]
    noise = np.random.RandomState(seed + 131 * H + W).randint(0, 64, (H, W))
    return torch.from_numpy(((3 * x + 7 * y + noise) % 256).astype(np.uint8))


# ------------------------------------------------------------------ 1. the turn ----------------------------------------------------------
TURN_SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (130, 257), (68, 132)]  # the last: several ragged tiles on the dword path


@pytest.mark.parametrize("shape", TURN_SHAPES, ids=[f"{h}x{w}" for h, w in TURN_SHAPES])
def test_turn_page_equals_rot90(dev, shape):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd._lib import lib, ptr

    H, W = shape
    page = _ramp_page(H, W)
    on_dev = page.to(dev)
    guard = 256
    for k in range(4):
        want = torch.rot90(page, k, dims=(-2, -1)).contiguous()
        got2, got3 = inf.turn_page(on_dev, k), inf.turn_page(on_dev[None], k)
        assert tuple(got2.shape) == O.turn_shape(H, W, k) == tuple(want.shape) and tuple(got3.shape) == (1, *want.shape)
        assert got2.is_contiguous() and torch.equal(got2.cpu(), want) and torch.equal(got3.cpu()[0], want), (shape, k)
        if k == 0:
            assert got2 is on_dev
            continue
        for shift in (0, 1):  # an output (and an input) that starts on and off a 16-byte boundary; the guard behind it stays as it was
            src = torch.empty(H * W + 16, dtype=torch.uint8, device=dev)[shift:shift + H * W]
            src.copy_(on_dev.view(-1))
            buf = torch.full((H * W + guard + 16,), SENT_B, dtype=torch.uint8, device=dev)[shift:]
            lib().turn_page_u8(ptr(src), H, W, k, ptr(buf))
            out = buf.cpu()
            assert torch.equal(out[:H * W].view(*want.shape), want), (shape, k, shift)
            assert (out[H * W:] == SENT_B).all(), (shape, k, shift)


def test_turn_page_argument_errors(dev):
    from ocrs_models_amd import inference as inf

    page = _ramp_page(12, 20).to(dev)
    for bad in (page.cpu(), page.float(), page.t(), page[:, ::2], page[None, None], torch.empty(0, 4, dtype=torch.uint8, device=dev)):
        with pytest.raises(RuntimeError):
            inf.turn_page(bad, 1)
        with pytest.raises(RuntimeError):
            inf.turn_page(bad, 0)
    for bad in (True, 4, -1, "upright", 1.0):
        with pytest.raises(RuntimeError, match="orientation"):
            inf.turn_page(page, bad)


# ------------------------------------------------------------------ 2. quads -------------------------------------------------------------
def test_turn_quads_equals_the_float32_restatement(dev):
    from ocrs_models_amd import inference as inf

    H, W = 301, 517
    r = np.random.RandomState(5)
    exact = (r.randint(-40, 1200, (300, 4, 2)) * 0.5).astype(np.float32)  # integers and half-integers
    rough = (r.uniform(-50.0, 600.0, (300, 4, 2))).astype(np.float32)
    for q in (exact, rough):
        q_d = torch.from_numpy(q).to(dev)
        for k in range(4):
            for inverse in (False, True):
                got = inf.turn_quads(q_d, k, H, W, inverse=inverse)
                assert got.cpu().numpy().tobytes() == O.turn_quads(q, k, H, W, inverse, np.float32).tobytes(), (k, inverse)
            back = inf.turn_quads(inf.turn_quads(q_d, k, H, W), k, H, W, inverse=True)
            if q is exact:
                assert torch.equal(back, q_d), k
    # corner j -> corner j: the quad of a turned page's rectangle is the turned rectangle
    q = torch.from_numpy(R.rotated_rect(100.0, 80.0, 60.0, 20.0, 10)[None]).to(dev)
    assert torch.equal(inf.turn_quads(q, 2, H, W)[0, 1], torch.tensor([W - 1, H - 1], device=dev) - q[0, 1])


def test_turn_quads_with_a_device_count(dev):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd._lib import lib, ptr

    q = torch.from_numpy(np.random.RandomState(1).uniform(0, 200, (40, 4, 2)).astype(np.float32)).to(dev)
    for n in (0, 1, 17, 40, 55):
        out = torch.full((40, 4, 2), SENT_F, device=dev)
        lib().turn_quads(ptr(q), 40, ptr(torch.tensor([n], dtype=torch.int32, device=dev)), 250, 210, 3, 0, ptr(out))
        m = min(n, 40)
        assert out[:m].cpu().numpy().tobytes() == O.turn_quads(q[:m].cpu().numpy(), 3, 250, 210, False, np.float32).tobytes()
        assert (out[m:] == SENT_F).all()
    got = inf.turn_quads(q, 1, 250, 210, count=torch.tensor([3], dtype=torch.int32, device=dev))
    assert got[:3].cpu().numpy().tobytes() == O.turn_quads(q[:3].cpu().numpy(), 1, 250, 210, False, np.float32).tobytes()
    assert inf.turn_quads(q[:0], 1, 250, 210).shape == (0, 4, 2)
    for bad in (lambda: inf.turn_quads(q.cpu(), 1, 250, 210), lambda: inf.turn_quads(q.double(), 1, 250, 210), lambda: inf.turn_quads(q, 1, 0, 210),
                lambda: inf.turn_quads(q, 1, 250, 210, count=torch.tensor([3], device=dev))):
        with pytest.raises(RuntimeError):
            bad()


# ------------------------------------------------------------------ 3. votes and picks ---------------------------------------------------
def box(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float32)


def vote_cases():
    r = np.random.RandomState(11)
    rand = np.stack([R.rotated_rect(r.uniform(0, 2000), r.uniform(0, 3000), r.uniform(5, 300), r.uniform(2, 40), r.uniform(0, 360), flip=bool(k % 2))
                     for k in range(1000)])
    ties = np.stack([box(10 * k, 0, 30 if k % 3 else 45, 10) for k in range(40)])  # many equal lengths: the smaller index goes first
    return {
        "none": np.zeros((0, 4, 2), np.float32),
        "one": box(3, 4, 50, 10)[None],
        "one that does not vote": box(3, 4, 10, 10)[None],
        "horizontal only": np.stack([box(0, 20 * k, 40 + k, 10) for k in range(9)]),
        "vertical only": np.stack([box(20 * k, 0, 10, 40 + k) for k in range(9)]),
        "45 degrees": np.stack([np.array([[0, 0], [16, 16], [14, 18], [-2, 2]], np.float32), np.array([[0, 0], [16, 17], [14, 19], [-2, 2]], np.float32),
                                np.array([[0, 0], [-16, 16], [-18, 14], [-2, -2]], np.float32)]),
        "aspect 1.5 and just below": np.stack([box(0, 0, 15, 10), box(0, 20, np.nextafter(np.float32(15), np.float32(0)), 10), box(0, 40, 10, 15),
                                               box(0, 60, 14.5, 10)]),
        "zero area and zero length": np.stack([box(0, 0, 30, 0), box(0, 0, 0, 30), box(5, 5, 0, 0), box(0, 0, 30, 10)]),
        "ties": ties,
        "square sides tie": np.stack([box(0, 0, 10, 10), np.roll(box(0, 0, 10, 10), 1, axis=0), box(0, 0, 40, 10)]),
        "random": rand,
    }


def _votes(dev, quads, **kw):
    from ocrs_models_amd import inference as inf

    sums, counts, picks = inf.orientation_votes(torch.from_numpy(np.ascontiguousarray(quads)).to(dev), **kw)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int32 and picks.dtype == torch.int32
    return sums.cpu().tolist(), counts.cpu().tolist(), picks.cpu().tolist()


def _check_votes(dev, quads, min_aspect=1.5, sample=64, count=None):
    kw = dict(min_aspect=min_aspect, sample=sample)
    if count is not None:
        kw["count"] = torch.tensor([count], dtype=torch.int32, device=dev)
    (h, v), (voters, K), picks = _votes(dev, quads, **kw)
    ref = O.votes(quads if count is None else quads[:max(0, min(count, len(quads)))], min_aspect, sample)
    assert (voters, K) == (ref["voters"], ref["K"]) and picks == ref["picks"] and len(picks) == sample
    assert abs(h - ref["H"]) <= VOTE_RTOL * abs(ref["H"]) and abs(v - ref["V"]) <= VOTE_RTOL * abs(ref["V"])
    return ref


@pytest.mark.parametrize("name", list(vote_cases()))
def test_votes_and_picks_equal_the_restatement(dev, name):
    quads = vote_cases()[name]
    ref = _check_votes(dev, quads)
    for sample in sorted({1, max(ref["voters"] - 1, 1), max(ref["voters"], 1), ref["voters"] + 1, 7}):  # below, at and above the voter count
        _check_votes(dev, quads, sample=sample)
    expected = {"none": (0, 0, 0), "one": (1, 1, 0), "one that does not vote": (0, 0, 0), "horizontal only": (9, 9, 0), "vertical only": (9, 0, 9),
                "45 degrees": (3, 2, 1), "aspect 1.5 and just below": (2, 1, 1), "zero area and zero length": (1, 1, 0), "square sides tie": (1, 1, 0)}
    if name in expected:
        voters, nh, nv = expected[name]
        lng, _, horiz = O.long_sides(quads)
        assert ref["voters"] == voters and int((ref["voter"] & horiz).sum()) == nh and int((ref["voter"] & ~horiz).sum()) == nv
    if name == "ties":
        assert ref["picks"][:14] == [k for k in range(40) if k % 3 == 0] and ref["picks"][14:40] == [k for k in range(40) if k % 3]
    if name == "random":
        assert 600 < ref["voters"] < 1000 and ref["H"] > 0 and ref["V"] > 0
        _check_votes(dev, quads, min_aspect=4.0, sample=200)
        _check_votes(dev, quads, count=300)
        _check_votes(dev, quads, count=0)
        _check_votes(dev, quads, count=5000)


def test_votes_are_reproducible_and_make_no_host_sync(dev):
    from ocrs_models_amd import inference as inf

    q = torch.from_numpy(vote_cases()["random"]).to(dev)
    page = _ramp_page(130, 257).to(dev)
    first = inf.orientation_votes(q)
    turned = inf.turn_page(page, 1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = inf.orientation_votes(q)
        turned_again = [inf.turn_page(page, k) for k in (1, 2, 3)]
        quads_again = inf.turn_quads(q, 3, 3000, 2000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(first, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert torch.equal(turned, turned_again[0]) and quads_again.shape == q.shape
    with pytest.raises(RuntimeError):
        inf.orientation_votes(q, sample=0)
    with pytest.raises(RuntimeError):
        inf.orientation_votes(q.cpu())


# ------------------------------------------------------------------ 4. confidence --------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7, 101])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_path_confidence_against_float64(dev, T, B):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    C = len(DEFAULT_ALPHABET) + 1
    g = torch.Generator().manual_seed(100 * T + B)
    lp = torch.log_softmax(4.0 * torch.randn(T, B, C, generator=g), dim=-1)
    lp[T - 1, B - 1] = lp[T - 1, B - 1].sort().values  # the maximum in the last class
    if T * B > 1:
        lp[0, 0] = float(np.log(1.0 / C))  # a row of equal values
    assert int(lp[T - 1, B - 1].argmax()) == C - 1
    steps = [1 + (7 * b + 3) % T for b in range(B)]
    steps[0], steps[-1] = (1, T) if B > 1 else (T, T)
    if B > 2:
        steps[1] = max(1, T // 2)
    got = inf.path_confidence(lp.to(dev), torch.tensor(steps, dtype=torch.int32, device=dev)).cpu().numpy()
    want = O.path_confidence(lp.numpy(), steps)
    assert got.dtype == np.float64 and got.shape == (B,)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"T {T}, B {B}, C {C}: steps {min(steps)}..{max(steps)}, largest error {err.max():.3e}, bound {SCORE_TOL:.0e}")
    assert (err <= SCORE_TOL).all()
    if T == 1:
        assert got[0] == float(lp[0, 0].double().max())


# ------------------------------------------------------------------ 5. explicit turns, end to end ------------------------------------------
@pytest.fixture(scope="module")
def golden(dev):
    return TL.dot_page(320, 240).to(dev)


def _same_but_coordinates(got, plain, k, H, W):
    """``got`` (on the page that was passed, H x W) is ``plain`` (read on the turned page) with the coordinate keys through the table"""
    assert len(got) == len(plain) > 0
    assert [g["text"] for g in got] == [p["text"] for p in plain]
    assert got == O.turn_results(plain, k, H, W)
    assert all(list(g) == [*p, "turns"] and g["turns"] == k for g, p in zip(got, plain))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_explicit_turns_equal_the_plain_call_on_the_turned_page(dev, det_model, rec_model, golden, k):
    from ocrs_models_amd import inference as inf

    H, W = golden.shape[-2:]
    turned = inf.turn_page(golden, k)
    assert torch.equal(turned.cpu(), torch.rot90(golden.cpu(), k, dims=(-2, -1)))
    _same_but_coordinates(inf.ocr_lines(det_model, rec_model, golden, size=SIZE, orientation=k), inf.ocr_lines(det_model, rec_model, turned, size=SIZE), k, H, W)
    _same_but_coordinates(inf.ocr_page(det_model, rec_model, golden, size=SIZE, orientation=k), inf.ocr_page(det_model, rec_model, turned, size=SIZE), k, H, W)
    kw = dict(size=SIZE, chars=True, rectify="chain", reading_order=True, beam_width=4)
    full, plain = inf.ocr_lines(det_model, rec_model, golden, orientation=k, **kw), inf.ocr_lines(det_model, rec_model, turned, **kw)
    _same_but_coordinates(full, plain, k, H, W)
    assert list(full[0]) == ["quad", "text", "words", "spine", "height", "char_quads", "char_log_probs", "log_prob", "word_chars", "word_texts", "block", "turns"]
    for key in O.COORD_KEYS:  # every mapped key is on the page that was passed: what the float32 device table gives, as Python floats
        flat = np.array([p for g in full for p in np.array(g[key], dtype=np.float64).reshape(-1, 2)])
        flat_plain = np.array([p for g in plain for p in np.array(g[key], dtype=np.float64).reshape(-1, 2)])
        assert len(flat) == len(flat_plain) > 0 and np.array_equal(flat, O.turn_quads(flat_plain, k, H, W))
    assert [g["height"] for g in full] == [p["height"] for p in plain]
    words = inf.ocr_page(det_model, rec_model, golden, size=SIZE, chars=True, orientation=k)
    _same_but_coordinates(words, inf.ocr_page(det_model, rec_model, turned, size=SIZE, chars=True), k, H, W)
    # the halves after detection take the upright page and the int
    det = inf.detect_words(det_model, turned, size=SIZE)
    assert inf.read_lines(rec_model, turned, det["quads"], orientation=k) == inf.ocr_lines(det_model, rec_model, golden, size=SIZE, orientation=k)
    assert inf.read_words(rec_model, turned, det["quads"], orientation=k) == inf.ocr_page(det_model, rec_model, golden, size=SIZE, orientation=k)


def test_orientation_0_and_none(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    plain = inf.ocr_lines(det_model, rec_model, golden, size=SIZE)
    assert all(list(p) == ["quad", "text", "words"] for p in plain)  # None: exactly the keys there were
    assert json.dumps(inf.ocr_lines(det_model, rec_model, golden, size=SIZE, orientation=None)) == json.dumps(plain)
    assert inf.ocr_lines(det_model, rec_model, golden, size=SIZE, orientation=0) == [{**p, "turns": 0} for p in plain]
    words = inf.ocr_page(det_model, rec_model, golden, size=SIZE)
    assert all(list(p) == ["quad", "text"] for p in words)
    assert inf.ocr_page(det_model, rec_model, golden, size=SIZE, orientation=0) == [{**p, "turns": 0} for p in words]
    assert inf.ocr_pages(det_model, rec_model, [golden], size=SIZE, orientation=0) == [[{**p, "turns": 0} for p in plain]]
    assert inf.ocr_pages(det_model, rec_model, [golden], size=SIZE, orientation=None) == [plain]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_page_turned_away_is_read_as_the_upright_page(dev, det_model, rec_model, golden, k):
    """the scanner's view: U is upright, the page that arrives is U turned by -k; orientation=k reads U's texts, with quads on the page that arrived"""
    from ocrs_models_amd import inference as inf

    fed = inf.turn_page(golden, (4 - k) % 4)
    assert torch.equal(inf.turn_page(fed, k), golden)
    upright = inf.ocr_lines(det_model, rec_model, golden, size=SIZE)
    got = inf.ocr_lines(det_model, rec_model, fed, size=SIZE, orientation=k)
    _same_but_coordinates(got, upright, k, *fed.shape[-2:])
    Hf, Wf = fed.shape[-2:]
    centres = np.array([np.mean(g["quad"], axis=0) for g in got])  # on the fed page, where the upright page's lines lie on it
    assert (centres >= 0).all() and (centres[:, 0] <= Wf - 1).all() and (centres[:, 1] <= Hf - 1).all()
    assert np.allclose(centres, np.stack(O.turn_point(*np.array([np.mean(u["quad"], axis=0) for u in upright]).T, k, Hf, Wf), axis=1), atol=1e-9)


def test_ocr_pages_with_an_orientation_per_page(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    pages = [golden, golden[:, :200].contiguous(), golden[:, :, :170].contiguous(), golden[:, 40:300, 30:].contiguous()]
    turns = [0, 1, 2, 3]
    got = inf.ocr_pages(det_model, rec_model, pages, size=SIZE, orientation=turns)
    plain = inf.ocr_pages(det_model, rec_model, [inf.turn_page(p, k) for p, k in zip(pages, turns)], size=SIZE)
    assert len(got) == 4
    for p, k, g, pl in zip(pages, turns, got, plain):
        _same_but_coordinates(g, pl, k, *p.shape[-2:])
        alone = inf.ocr_lines(det_model, rec_model, p, size=SIZE, orientation=k)  # (a crop's padded width, and so its text, depends on the batch)
        assert len(alone) == len(g) and all(a[key] == b[key] for a, b in zip(alone, g) for key in ("quad", "words", "turns"))
    same = inf.ocr_pages(det_model, rec_model, pages[:2], size=SIZE, orientation=3, lines=False)
    assert same == [O.turn_results(r, 3, *p.shape[-2:]) for r, p in
                    zip(inf.ocr_pages(det_model, rec_model, [inf.turn_page(p, 3) for p in pages[:2]], size=SIZE, lines=False), pages[:2])]
    kw = dict(size=SIZE, chars=True, rectify="chain", reading_order=True, beam_width=4)
    full = inf.ocr_pages(det_model, rec_model, pages[:2], orientation=[2, 1], **kw)
    assert full == [O.turn_results(r, k, *p.shape[-2:]) for r, k, p in
                    zip(inf.ocr_pages(det_model, rec_model, [inf.turn_page(pages[0], 2), inf.turn_page(pages[1], 1)], **kw), [2, 1], pages[:2])]


# ------------------------------------------------------------------ 6. auto ----------------------------------------------------------------
def _orientation_by_hand(dev, det_model, rec_model, page, min_aspect=1.5, sample=64):
    """the rule from the stages: detect_words, the reference vote on the copied quads, the crops of the picks from the two turned pages (turned
    on the CPU; the quads by the float32 restatement), the recogniser's log-probs copied to the CPU, the reference mean"""
    from ocrs_models_amd import inference as inf

    H, W = page.shape[-2:]
    det = inf.detect_words(det_model, page, size=SIZE)
    quads = det["quads"].cpu().numpy()
    ref = O.votes(quads, min_aspect, sample)
    if ref["voters"] == 0:
        return det, ref, None
    K, a = ref["K"], 1 if ref["V"] > ref["H"] else 0
    picked = quads[ref["picks"][:K]]
    pages = [torch.rot90(page.cpu(), k, dims=(-2, -1)).contiguous().to(dev) for k in (a, a + 2)]
    both = torch.from_numpy(np.concatenate([O.turn_quads(picked, k, H, W, True, np.float32) for k in (a, a + 2)])).to(dev)
    plan = inf.crop_plan(both)
    page_of_quad = torch.tensor([0] * K + [1] * K, dtype=torch.int32, device=dev)
    batches, widths, perm = inf.crops_to_batches(inf.rectify_crops_pages(*inf.pack_pages(pages), both, page_of_quad, plan), plan)
    with torch.inference_mode():
        scores = np.concatenate([O.path_confidence(rec_model(img).cpu().numpy(), (iw // 4).cpu().tolist()) for img, iw in zip(batches, widths)])
    by_quad = scores[perm]
    means = {a: O.mean_in_order(by_quad[:K]), a + 2: O.mean_in_order(by_quad[K:])}
    return det, ref, O.decide(ref["H"], ref["V"], means.get)


def test_page_orientation_equals_the_stages_by_hand(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    decidable = 0
    for k_fed in range(4):
        page = inf.turn_page(golden, (4 - k_fed) % 4)
        found = inf.page_orientation(det_model, rec_model, page, size=SIZE)
        det, ref, rule = _orientation_by_hand(dev, det_model, rec_model, page)
        assert list(found) == ["turns", "votes", "voters", "sampled", "scores", "det"]
        assert torch.equal(found["det"]["quads"], det["quads"]) and found["det"]["n"] == det["n"] > 0
        assert (found["voters"], found["sampled"]) == (ref["voters"], ref["K"])
        for got, want in zip(found["votes"], (ref["H"], ref["V"])):
            assert abs(got - want) <= VOTE_RTOL * abs(want)
        if rule is None:
            print(f"page turned by -{k_fed}: {det['n']} words, no voters")
            assert found["turns"] == 0 and found["scores"] is None
            continue
        for got, want in zip(found["scores"], rule["scores"]):
            assert abs(got - want) <= SCORE_TOL * max(1.0, abs(want))
        axis_margin, sign_margin = abs(ref["V"] - ref["H"]), abs(rule["scores"][1] - rule["scores"][0])
        axis_ok = axis_margin > VOTE_RTOL * max(ref["H"], ref["V"])
        sign_ok = sign_margin > 2 * SCORE_TOL * max(1.0, *map(abs, rule["scores"]))
        print(f"page turned by -{k_fed}: {det['n']} words, {ref['voters']} voters, K {ref['K']}, H {ref['H']:.3f}, V {ref['V']:.3f} (margin {axis_margin:.3e}), "
              f"scores {rule['scores'][0]:.6f} / {rule['scores'][1]:.6f} (margin {sign_margin:.3e}): turns {found['turns']}, by hand {rule['turns']}")
        if axis_ok:
            assert found["turns"] % 2 == rule["a"]
        if axis_ok and sign_ok:
            decidable += 1
            assert found["turns"] == rule["turns"]
        auto = inf.ocr_lines(det_model, rec_model, page, size=SIZE, orientation="auto")
        assert auto == inf.ocr_lines(det_model, rec_model, page, size=SIZE, orientation=found["turns"])
        assert auto and all(g["turns"] == found["turns"] for g in auto)
    assert decidable > 0, "no page had a decidable margin: nothing was compared"
    words = inf.ocr_page(det_model, rec_model, golden, size=SIZE, orientation="auto")
    assert words == inf.ocr_page(det_model, rec_model, golden, size=SIZE, orientation=words[0]["turns"])
    pages = [golden, inf.turn_page(golden, 1)]
    per_page = [inf.page_orientation(det_model, rec_model, p, size=SIZE)["turns"] for p in pages]
    assert inf.ocr_pages(det_model, rec_model, pages, size=SIZE, orientation="auto") == inf.ocr_pages(det_model, rec_model, pages, size=SIZE, orientation=per_page)
    assert inf.ocr_pages(det_model, rec_model, pages, size=SIZE, orientation=["auto", per_page[1]]) == inf.ocr_pages(det_model, rec_model, pages, size=SIZE, orientation=per_page)


def _bars_page(dev, vertical: bool):
    """long thin bars, 8 x 60, on a 200 x 260 page -> (page, det dict with their quads expanded by 3)"""
    H, W = 200, 260
    page = np.full((H, W), 230, np.uint8)
    quads = []
    for r in range(2):
        for c in range(6):
            x, y, w, h = (20 + 36 * c, 20 + 90 * r, 8, 60) if vertical else (20 + 80 * (c % 3), 15 + 30 * (c // 3) + 100 * r, 60, 8)
            page[y:y + h, x:x + w] = 30
            page[y + 2:y + h - 2:3, x + 2:x + w - 2:3] = 180
            quads.append(box(x - 3, y - 3, w - 1 + 6, h - 1 + 6))
    q = torch.from_numpy(np.stack(quads)).to(dev)
    return torch.from_numpy(page)[None].to(dev), {"quads": q, "n": len(quads)}


def test_the_axis_of_long_thin_bars(dev, rec_model):
    from ocrs_models_amd import inference as inf

    for vertical in (True, False):
        page, det = _bars_page(dev, vertical)
        found = inf.page_orientation(None, rec_model, page, det=det)
        h, v = found["votes"]
        assert found["det"] is det and found["voters"] == found["sampled"] == 12 and found["scores"] is not None
        assert (v, h) == (12 * 65.0, 0.0) if vertical else (h, v) == (12 * 65.0, 0.0)
        assert found["turns"] % 2 == (1 if vertical else 0)
        assert found["turns"] == (found["turns"] % 2) + (2 if found["scores"][1] > found["scores"][0] else 0)
        fewer = inf.page_orientation(None, rec_model, page, det=det, sample=5, min_aspect=3.0)
        assert fewer["sampled"] == 5 and fewer["voters"] == 12 and fewer["turns"] % 2 == found["turns"] % 2
        assert inf.page_orientation(None, NeverCalled().eval(), page, det=det, min_aspect=20.0)["scores"] is None  # no voters: no probe


def test_a_page_without_words_is_upright_and_launches_no_recogniser(dev):
    from ocrs_models_amd import inference as inf

    page = torch.full((1, 120, 90), 255, dtype=torch.uint8, device=dev)
    found = inf.page_orientation(DarkIsText().eval(), NeverCalled().eval(), page, size=(120, 90))
    assert found["turns"] == 0 and found["scores"] is None and found["voters"] == 0 and found["sampled"] == 0 and found["det"]["n"] == 0
    assert found["votes"] == (0.0, 0.0)
    for who in (inf.ocr_page, inf.ocr_lines):
        assert who(DarkIsText().eval(), NeverCalled().eval(), page, size=(120, 90), orientation="auto") == []
        assert who(DarkIsText().eval(), NeverCalled().eval(), page, size=(120, 90), orientation=3) == []
    assert inf.ocr_pages(DarkIsText().eval(), NeverCalled().eval(), [page, page], size=(120, 90), orientation=["auto", 1]) == [[], []]


# ------------------------------------------------------------------ 7. waits ---------------------------------------------------------------
def test_orientation_waits(dev, rec_model):
    """Counted the way tests/test_lines_gpu.py counts them, on a page of bars with one chunk of crops and a detector that fits the page any way
    up.  An int costs no wait; "auto" at most three (votes, probe plan, scores), and the turned page's detection where it finds a turn."""
    from ocrs_models_amd import inference as inf

    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)]
    upright, _ = TL.bar_page(230, 340, bars, dev)
    det = DarkIsText().eval()
    kw = dict(size=(230, 340))
    fed = {0: upright, 2: inf.turn_page(upright, 2)}
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        for page in fed.values():
            inf.ocr_lines(det, rec_model, page, **kw), inf.ocr_lines(det, rec_model, page, orientation=2, **kw), inf.ocr_lines(det, rec_model, page, orientation="auto", **kw)
    seen = set()
    for name, page in fed.items():
        plain, n_plain, what_plain = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, **kw))
        turned, n_turned, what_turned = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, orientation=2, **kw))
        auto, n_auto, what_auto = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, orientation="auto", **kw))
        found = auto[0]["turns"]
        seen.add(found)
        print(f"page fed turned by {name}: host waits plain {n_plain} {what_plain}, orientation=2 {n_turned} {what_turned}, auto (found {found}) {n_auto} {what_auto}")
        assert len(plain) == len(turned) == len(auto) == 5
        assert n_plain >= 3 and n_turned <= n_plain
        assert n_auto <= n_plain + (3 if found == 0 else 4)
        assert found in (0, 2)
    print(f"auto found {sorted(seen)}")
    batch, n_batch, _ = TL._count_waits(lambda: inf.ocr_pages(det, rec_model, [upright, fed[2]], **kw))
    turned, n_turned, _ = TL._count_waits(lambda: inf.ocr_pages(det, rec_model, [upright, fed[2]], orientation=[0, 2], **kw))
    assert n_turned <= n_batch and [len(b) for b in batch] == [len(t) for t in turned] == [5, 5]


# ------------------------------------------------------------------ 8. argument errors -------------------------------------------------------
def test_argument_errors_come_before_any_launch(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd._lib import lib

    L = lib()
    launched = []
    L.timing = {name: launched for name in ("turn_page_u8", "turn_quads", "orient_votes", "path_confidence", "crop_plan", "binarize_resize_nearest")}
    try:
        for bad in (True, 4, -1, "upright", [0, 1], 2.0):
            for call in (lambda: inf.ocr_page(det_model, rec_model, golden, size=SIZE, orientation=bad),
                         lambda: inf.ocr_lines(det_model, rec_model, golden, size=SIZE, orientation=bad),
                         lambda: inf.ocr_pages(det_model, rec_model, [golden], size=SIZE, orientation=bad)):
                with pytest.raises(RuntimeError, match="orientation"):
                    call()
        with pytest.raises(RuntimeError, match="one entry per page"):
            inf.ocr_pages(det_model, rec_model, [golden, golden], size=SIZE, orientation=[0])
        with pytest.raises(RuntimeError, match="orientation"):
            inf.ocr_pages(det_model, rec_model, [golden, golden], size=SIZE, orientation=[0, "upright"])
        two_d = golden[0]
        for bad_page in (golden.cpu(), golden.float(), golden.transpose(1, 2), golden[:, :, ::2]):
            for orientation in (1, 0, "auto"):
                with pytest.raises(RuntimeError):
                    inf.ocr_lines(det_model, rec_model, bad_page, size=SIZE, orientation=orientation)
                with pytest.raises(RuntimeError):
                    inf.ocr_page(det_model, rec_model, bad_page, size=SIZE, orientation=orientation)
            with pytest.raises(RuntimeError):
                inf.page_orientation(det_model, rec_model, bad_page, size=SIZE)
            with pytest.raises(RuntimeError):
                inf.ocr_pages(det_model, rec_model, [golden, bad_page], size=SIZE, orientation=1)
        with pytest.raises(RuntimeError):
            inf.page_orientation(det_model, rec_model, two_d, size=SIZE)
        with pytest.raises(RuntimeError):
            inf.page_orientation(det_model, rec_model, golden, size=SIZE, sample=0)
        assert launched == []
    finally:
        L.timing = None


# ------------------------------------------------------------------ 9. CLI ------------------------------------------------------------------
def test_eval_detection_cli_with_orientation(dev, det_model, rec_model, tmp_path):
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
    cmd = [sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), str(tmp_path / "out"), "--rec-model",
           str(tmp_path / "rec.pt")]
    for bad in (["--orientation", "4"], ["--orientation", "upright"]):  # refused by the argument parser, before any file is read
        with pytest.raises(SystemExit) as e:
            eval_detection.main([*cmd[3:], *bad])
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:  # auto needs the recogniser
        eval_detection.main([*cmd[3:6], "--orientation", "auto"])
    assert e.value.code == 2
    page = page_h.to(dev)
    for orientation in ("1", "auto"):
        r = subprocess.run([*cmd, "--lines", "--orientation", orientation], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
        want = inf.ocr_lines(det_model, rec_model, page, orientation=1 if orientation == "1" else "auto")
        assert got and got == want and all(list(g) == ["quad", "text", "words", "turns"] for g in got)
        with open(tmp_path / "out-orientation.json") as f:
            recorded = json.load(f)
        assert recorded["turns"] == got[0]["turns"] and f"Orientation: {recorded['turns']} quarter turn" in r.stderr
        if orientation == "auto":
            found = inf.page_orientation(det_model, rec_model, page)
            assert recorded == {"turns": found["turns"], "votes": list(found["votes"]), "voters": found["voters"], "sampled": found["sampled"],
                                "scores": None if found["scores"] is None else list(found["scores"])}
        upright = Image.open(tmp_path / "out-text-lines.png")
        assert upright.size == ((400, 300) if recorded["turns"] % 2 else (300, 400))  # the pictures show the upright page

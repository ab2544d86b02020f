"""Chain crops on the GPU (csrc/line_chain.hip, the plan in csrc/ocr_infer.hip; inference/chain.py and ``rectify="chain"`` of the line drivers)
against the numpy restatement of the rule (tests/chain_ref.py, pinned by tests/test_chain_host.py).

Exact cases.  Axis-aligned words with integer corners below 4096, every word of a line centred on one baseline: side lengths are integers,
u is (1, 0), the knots are multiples of 0.5, every gap vector is (integer, 0), and the running sum adds integers below 4096: all exact in
fp32.  So the spine table, the dims and the plan must equal the float32 restatement with ``==``.

Rotated and curved lines.  Tables and character quads against float64 within 2 * K_TABLE ulp32(max(S, largest |coordinate|)), crops within
2 * K_CROP * ulp32(largest page coordinate) * (value range 1.0) + the blend's roundings: twice what the float32 restatement needs against the
float64 one (the constants of chain_ref.py), the margin test_ocr_gpu.py uses for ``rectify_crops``.  Every gap of these cases is > 0, so the
map is continuous across knots and no sample is left out; the tests print the measured maxima (DESIGN.md §21 records them).

End to end.  The golden detection and recognition weights on a page of dots, as tests/test_lines_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import chain_ref as C
from tests import lines_ref as LR
from tests import ocr_ref as R
from tests import test_lines_gpu as TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_F, SENT_I = -12345.0, -77
SIZE = (160, 120)


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


# ------------------------------------------------------------------ helpers --------------------------------------------------------------
def _lines(dev, words, chains, pad=0, page_of_line=None):
    """a ``TextLines`` staged by hand: ``words`` (n,4,2) plus ``pad`` sentinel rows, line l = the words ``chains[l]`` in that order; entries
    past the lines hold sentinels (no kernel may read them)"""
    from ocrs_models_amd import inference as inf

    n, L = len(words) + pad, len(chains)
    i32 = dict(dtype=torch.int32, device=dev)
    w = torch.full((n, 4, 2), SENT_F, device=dev)
    w[:len(words)] = torch.from_numpy(np.ascontiguousarray(words, dtype=np.float32)).to(dev)
    order = [i for c in chains for i in c]
    word_order, offs = torch.full((n,), SENT_I, **i32), torch.full((n + 1,), SENT_I, **i32)
    word_order[:len(order)] = torch.tensor(order, **i32)
    offs[:L + 1] = torch.tensor(np.cumsum([0] + [len(c) for c in chains]), **i32)
    out = inf.TextLines(torch.zeros(n, 4, 2, device=dev), torch.tensor([L], **i32), torch.zeros(n, **i32), word_order, offs, torch.zeros(n, **i32), words=w)
    if page_of_line is not None:
        out.page_of_line = torch.full((n,), SENT_I, **i32)
        out.page_of_line[:L] = torch.tensor(page_of_line, **i32)
    return out


def _one_table(cases):
    """name -> words in chain order  =>  (all words shuffled (N,4,2), chains into them, in the cases' order)"""
    words = np.concatenate(list(cases.values()))
    perm = np.random.RandomState(3).permutation(len(words))
    inv = np.argsort(perm)
    chains, at = [], 0
    for w in cases.values():
        chains.append([int(inv[at + k]) for k in range(len(w))])
        at += len(w)
    return words[perm], chains


def _plan_ref(rows):
    """the plan table and totals of crops (h, w, ow) in index order, as ocrs_crop_plan lays them out"""
    n = len(rows)
    table, po, ho, to = np.zeros((n, 8), dtype=np.int64), 0, 0, 0
    for i, (h, w, ow) in enumerate(rows):
        table[i, :6] = h, w, ow, po, ho, to
        po, ho, to = po + ((h * w + 3) & ~3), ho + h * ow, to + -(-h * w // 1024)
    for r, i in enumerate(sorted(range(n), key=lambda i: (rows[i][2], i))):
        table[i, 6], table[r, 7] = r, i
    return table, [n, po, ho, to] + np.bincount([r[2] for r in rows], minlength=801).tolist()


def _crops_of(packed, plan, n):
    table = plan.table.cpu().numpy()
    return [packed[int(o):int(o) + int(h) * int(w)].view(int(h), int(w)) for h, w, _, o in table[:n, :4]]


def _crop_bound(k):
    return k * R.ulp32(1023.0) * 1.0 + R.RECTIFY_BLEND_ROUNDINGS * R.ulp32(0.5) / 2


def _stage_spans(dev, table, n, steps):
    """``CharSpans`` staged by hand: row p is the crop of line table[p, 7] and gets the characters ``steps(line) -> (labels, t0, t1)``"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import text

    per_row = [steps(int(table[p, 7])) for p in range(n)]
    ld = max(max(len(r[0]) for r in per_row), 1) + 3
    spans = inf.CharSpans(*text.span_arrays(n, ld, dev))
    spans.buf.fill_(SENT_I)
    for p, (labels, t0, t1) in enumerate(per_row):
        k = len(labels)
        spans.labels[p, :k], spans.t0[p, :k], spans.t1[p, :k] = (torch.tensor(list(v), dtype=torch.int32, device=dev) for v in (labels, t0, t1))
        spans.lens[p] = k
    return spans, per_row


# ------------------------------------------------------------------ exact ----------------------------------------------------------------
def _exact_line(x, yc, n, w=14, step=20, heights=(6, 8, 12)):
    """n axis-aligned integer words ``w`` wide every ``step`` pixels (step < w: they overlap), centred on the baseline yc, heights cycling"""
    return np.stack([LR.box(x + k * step, yc - heights[k % len(heights)] // 2, w, heights[k % len(heights)]) for k in range(n)])


def exact_cases():
    cases = {f"{n} words": _exact_line(3, 100 * (i + 1), n) for i, n in enumerate([1, 2, 64, 65, 200])}
    cases["overlapping"] = _exact_line(40, 700, 5, step=10)  # neighbours overlap by 4: every gap has length 0
    mixed = np.concatenate([_exact_line(30, 800, 3, step=10), _exact_line(81, 800, 2)])  # two zero gaps, then gaps of 17 (64 -> 81) and 6
    cases["overlap then gap"] = mixed
    assert max(float(np.abs(w).max()) for w in cases.values()) < 4096
    return cases


def _check_exact(dev, words, chains, pad=0, lines=None):
    """the spine table, dims and plan of the lines against the float32 restatement with ==; sentinels survive past the lines"""
    from ocrs_models_amd import inference as inf

    lines = _lines(dev, words, chains, pad) if lines is None else lines
    n, L, nw = lines.words.shape[0], len(chains), sum(len(c) for c in chains)
    out = inf.LineSpines(torch.full((2 * n, 8), SENT_F, device=dev), torch.full((n, 2), SENT_F, device=dev), None)
    got = inf.line_spines(lines, out=out)
    assert got is out and out.lines is lines
    fresh = inf.line_spines(lines)
    spine, dims = out.spine.cpu().numpy(), out.line_dims.cpu().numpy()
    ref_spine, ref_dims, sps = C.table(words, chains, np.float32)
    assert ref_spine.dtype == np.float32 and ref_dims.dtype == np.float32 and np.array_equal(spine[:2 * nw], ref_spine)
    assert np.array_equal(dims[:L], ref_dims)
    assert (spine[2 * nw:] == SENT_F).all() and (dims[L:] == SENT_F).all()
    assert torch.equal(fresh.spine[:2 * nw], out.spine[:2 * nw]) and torch.equal(fresh.line_dims[:L], out.line_dims[:L])
    for oh in (64, 48):
        plan = inf.crop_plan_chain(out, oh)
        table, totals = _plan_ref([C.plan_row(sp, oh) for sp in sps])
        assert tuple(plan.table.shape) == (n, 8) and np.array_equal(plan.table.cpu().numpy()[:L], table)
        assert plan.totals.cpu().tolist() == totals and plan.host()[0] == L
    return out, sps


def test_exact_tables_equal_the_float32_restatement(dev):
    cases = exact_cases()
    assert [len(w) for w in cases.values()][:5] == [1, 2, 64, 65, 200]
    words, chains = _one_table(cases)
    _, sps = _check_exact(dev, words, chains)
    assert all((sp["rows"][1:-1:2, 1] == 0).all() for sp in (sps[5],)) and (sps[6]["rows"][1:-1:2, 1] == [0, 0, 17, 6]).all()
    assert float(sps[4]["S"]) == 200 * 14 + 199 * 6 and float(sps[4]["H"]) == 12
    for name, w in cases.items():  # and every line alone, in chain order
        _check_exact(dev, w, [list(range(len(w)))])


def test_exact_tables_in_a_padded_buffer_with_a_device_count(dev):
    """more rows than words, and fewer lines counted than the line table describes: the rows of the uncounted lines keep their sentinels"""
    words, chains = _one_table(exact_cases())
    _check_exact(dev, words, chains, pad=37)
    lines = _lines(dev, words, chains, pad=5)
    lines.n_lines.fill_(3)
    _check_exact(dev, words, chains[:3], lines=lines)


def test_exact_tables_from_find_lines_pages(dev):
    from ocrs_models_amd import inference as inf

    a, b = LR.grid_case(3, 5, seed=4), LR.grid_case(4, 3, seed=6, w=52, h=18, gap=12)
    words = np.concatenate([a, b])
    i32 = dict(dtype=torch.int32, device=dev)
    found = inf.find_lines_pages(torch.from_numpy(words).to(dev), torch.tensor([0] * len(a) + [1] * len(b), **i32), torch.tensor([0, len(a), len(words)], **i32))
    L = int(found.n_lines)
    order, offs = found.word_order.cpu().tolist(), found.line_offsets.cpu().tolist()
    chains = [order[offs[l]:offs[l + 1]] for l in range(L)]
    assert L == 7 and sorted(len(c) for c in chains) == [3, 3, 3, 3, 5, 5, 5] and found.page_of_line[:L].tolist() == [0, 0, 0, 1, 1, 1, 1]
    _check_exact(dev, words, chains, lines=found)
    single = inf.find_lines(torch.from_numpy(a).to(dev))
    order, offs = single.word_order.cpu().tolist(), single.line_offsets.cpu().tolist()
    _check_exact(dev, a, [order[offs[l]:offs[l + 1]] for l in range(int(single.n_lines))], lines=single)


def test_no_lines_launch_nothing(dev):
    from ocrs_models_amd import inference as inf

    lines = inf.find_lines(torch.empty(0, 4, 2, device=dev))
    sp = inf.line_spines(lines)
    assert tuple(sp.spine.shape) == (0, 8) and tuple(sp.line_dims.shape) == (0, 2)
    plan = inf.crop_plan_chain(sp)
    assert plan.host()[:4] == [0, 0, 0, 0]
    assert inf.rectify_chain(torch.zeros(1, 8, 8, dtype=torch.uint8, device=dev), sp, plan).numel() == 0
    with pytest.raises(RuntimeError):
        inf.line_spines(inf.TextLines(*[None] * 6))
    with pytest.raises(RuntimeError):
        inf.rectify_chain(torch.zeros(1, 8, 8, dtype=torch.uint8, device=dev), sp, inf.crop_plan(torch.zeros(2, 4, 2, device=dev)))


# ------------------------------------------------------------------ rotated and curved ----------------------------------------------------
@pytest.fixture(scope="module")
def curved(dev):
    """the curved cases and the 200-word arc as one table on the page of ``rectify_case``: spines, plan and crops, computed once"""
    from ocrs_models_amd import inference as inf

    page, _ = R.rectify_case()
    cases = {**C.curved_cases(), "long arc": C.long_arc_case()}
    words, chains = _one_table(cases)
    lines = _lines(dev, words, chains)
    sp = inf.line_spines(lines)
    plan = inf.crop_plan_chain(sp)
    packed = inf.rectify_chain(page.to(dev), sp, plan)
    sp64 = [C.line_spine(w, np.float64) for w in cases.values()]
    return dict(page=page, cases=cases, words=words, chains=chains, lines=lines, sp=sp, plan=plan, packed=packed, sp64=sp64)


def test_curved_tables_against_float64(curved):
    sp, plan = curved["sp"], curved["plan"]
    spine, dims, table = sp.spine.cpu().numpy().astype(np.float64), sp.line_dims.cpu().numpy().astype(np.float64), plan.table.cpu().numpy()
    at, worst = 0, 0.0
    for l, (name, words) in enumerate(curved["cases"].items()):
        ref, n = curved["sp64"][l], len(words)
        if n <= 16:
            top = max(float(ref["S"]), float(np.abs(words).max()))
            err = max(np.abs(spine[2 * at:2 * (at + n)] - ref["rows"]).max(), abs(dims[l, 0] - ref["S"]), abs(dims[l, 1] - ref["H"]))
            print(f"{name}: table error {err:.3e} = {err / R.ulp32(top):.2f} ulp32({top:.1f}), bound {2 * C.K_TABLE} ulp32")
            worst = max(worst, err / R.ulp32(top))
            assert err <= 2 * C.K_TABLE * R.ulp32(top)
        assert tuple(table[l, :3]) == C.plan_row(ref)
        at += n
    print(f"curved tables: at most {worst:.2f} ulp32")
    assert plan.host()[0] == len(curved["cases"])


def test_curved_crops_against_float64(curved):
    page, packed = curved["page"], curved["packed"].cpu()
    bound, ulp = _crop_bound(2 * C.K_CROP), R.ulp32(1023.0)
    worst = 0.0
    assert max(len(w) for w in curved["cases"].values()) == 200  # the line whose rows do not fit the sampler's LDS budget
    for (name, words), ref, crop in zip(curved["cases"].items(), curved["sp64"], _crops_of(packed, curved["plan"], len(curved["cases"]))):
        assert (ref["rows"][1:2 * ref["n"] - 1:2, 1] > 0).all()  # every gap has a length: the map is continuous, no sample is left out
        want = C.rectify(page, ref, np.float64)
        assert tuple(crop.shape) == tuple(want.shape)
        err = float(np.abs(crop.double().numpy() - want).max())
        print(f"{name}: crop {tuple(want.shape)}, max error {err:.3e} = {err / ulp:.2f} ulp32(1023), bound {bound:.3e}")
        worst = max(worst, err)
        assert err <= bound
    print(f"rectify_chain: max error {worst:.3e} = {worst / ulp:.2f} ulp32(1023), bound {bound:.3e} (k = {2 * C.K_CROP})")
    # a lane's four samples of the 200-word line do cross knots: its segments are shorter than four columns
    assert float(curved["sp64"][-1]["rows"][:-1, 1].max()) < 4.5 and curved["sp64"][-1]["n"] * 2 - 1 > 256


def test_zero_gap_crop_against_the_float32_restatement(dev):
    """where the spine jumps, the float64 map is not continuous: compared with the float32 restatement, except the samples whose s is within
    4 ulp32(S) of a jump (there one rounding of S decides the segment)"""
    from ocrs_models_amd import inference as inf

    page, _ = R.rectify_case()
    words = C.overlap_case()
    sp = inf.line_spines(_lines(dev, words, [[0, 1, 2]]))
    plan = inf.crop_plan_chain(sp)
    crop = _crops_of(inf.rectify_chain(page.to(dev), sp, plan).cpu(), plan, 1)[0].numpy()
    ref = C.line_spine(words, np.float32)
    want = C.rectify(page, ref, np.float32)
    assert crop.shape == want.shape == C.crop_size(ref) and (ref["rows"][[1, 3], 1] == 0).all()
    s, _ = C.sample_coords(ref, np.float32)
    jumps = ref["rows"][[2, 4], 0].astype(np.float64)
    keep = (np.abs(s.astype(np.float64)[:, None] - jumps[None, :]) > 4 * R.ulp32(float(ref["S"]))).all(axis=1)
    assert (~keep).sum() * crop.shape[0] < 0.01 * crop.size
    err = float(np.abs(crop[:, keep].astype(np.float64) - want[:, keep]).max())
    bound = _crop_bound(2 * C.K_CROP)
    print(f"zero-gap line: crop {crop.shape}, {int((~keep).sum())} columns skipped, max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_one_word_lines_are_the_quad_path(dev):
    """plan rows equal crop_plan of the word quads exactly; crops within the sum of the two bounds of rectify_crops of the same quads"""
    from ocrs_models_amd import inference as inf

    page, quads = R.rectify_case()
    n = len(quads)
    sp = inf.line_spines(_lines(dev, quads.numpy(), [[i] for i in range(n)]))
    plan, qplan = inf.crop_plan_chain(sp), inf.crop_plan(quads.to(dev))
    assert torch.equal(plan.table, qplan.table) and torch.equal(plan.totals, qplan.totals)
    got, want = inf.rectify_chain(page.to(dev), sp, plan).cpu(), inf.rectify_crops(page.to(dev), quads.to(dev), qplan).cpu()
    bound = _crop_bound(2 * C.K_CROP) + _crop_bound(2 * R.RECTIFY_K_CPU)
    worst = max(float((a - b).abs().max()) for a, b in zip(_crops_of(got, plan, n), _crops_of(want, qplan, n)))
    print(f"one-word lines: chain against quad crops, max difference {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


def test_page_store_gives_every_crop_its_own_pages_bytes(dev, curved):
    from ocrs_models_amd import inference as inf

    page0 = curved["page"].to(dev)
    page1 = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (1, 300, 500)).astype(np.uint8)).to(dev)
    cases = C.curved_cases()
    on0 = {k: cases[k] for k in ("arc 300", "plus 20")}
    on1 = {"flat": C.straight_line(20.0, 80.0, 4.0, [70.0, 64.0, 80.0, 58.0], [22.0, 28.0, 24.0, 30.0], [12.0] * 3),
           "one": R.rotated_rect(250.0, 200.0, 120.0, 30.0, -8)[None], "over the edge": C.straight_line(380.0, 250.0, -3.0, [60.0, 70.0], [24.0, 24.0], [9.0])}
    words, chains = _one_table({**on0, **on1})
    page_of_line = [0, 0, 1, 1, 1]
    lines = _lines(dev, words, chains, page_of_line=page_of_line)
    sp = inf.line_spines(lines)
    plan = inf.crop_plan_chain(sp)
    pooled = _crops_of(inf.rectify_chain_pages(*inf.pack_pages([page0, page1]), sp, lines.page_of_line, plan).cpu(), plan, 5)
    for p, page in enumerate((page0, page1)):
        mine = [l for l in range(5) if page_of_line[l] == p]
        sp_p = inf.line_spines(_lines(dev, words, [chains[l] for l in mine]))
        plan_p = inf.crop_plan_chain(sp_p)
        for l, crop in zip(mine, _crops_of(inf.rectify_chain(page, sp_p, plan_p).cpu(), plan_p, len(mine))):
            assert crop.shape == pooled[l].shape and crop.numpy().tobytes() == pooled[l].numpy().tobytes(), (p, l)
    with pytest.raises(RuntimeError):
        inf.rectify_chain_pages(*inf.pack_pages([page0, page1]), sp, lines.page_of_line.long(), plan)


# ------------------------------------------------------------------ characters -------------------------------------------------------------
def test_char_boxes_chain_against_float64(curved):
    from ocrs_models_amd import inference as inf

    dev = curved["sp"].spine.device
    sp, plan, names = curved["sp"], curved["plan"], list(curved["cases"])
    n = len(names)
    table = plan.table.cpu().numpy()

    def steps(line):
        t0 = np.arange(0, int(table[line, 2]) // 4, 3)
        return np.ones_like(t0) + 4, t0, t0 + 2

    spans, per_row = _stage_spans(dev, table, n, steps)
    boxes = inf.char_boxes_chain(sp, plan, spans)
    s0, s1, quads = boxes.s0.cpu().numpy(), boxes.s1.cpu().numpy(), boxes.quads.cpu().numpy()  # (entries past a row's length are not written)
    worst = 0.0
    for p in range(n):
        line = int(table[p, 7])
        if len(curved["cases"][names[line]]) > 16:
            continue
        ref64 = curved["sp64"][line]
        _, t0, t1 = per_row[p]
        want = C.char_boxes(ref64, int(table[line, 2]), t0, t1, np.float64)
        k = len(t0)
        top = max(float(ref64["S"]), float(np.abs(curved["cases"][names[line]]).max()))
        err = max(np.abs(quads[p, :k].astype(np.float64) - want["quads"]).max(), np.abs(s0[p, :k].astype(np.float64) - want["s0"]).max(),
                  np.abs(s1[p, :k].astype(np.float64) - want["s1"]).max())
        print(f"{names[line]}: {k} characters, box error {err:.3e} = {err / R.ulp32(top):.2f} ulp32({top:.1f}), bound {2 * C.K_TABLE} ulp32")
        worst = max(worst, err / R.ulp32(top))
        assert err <= 2 * C.K_TABLE * R.ulp32(top)
    print(f"char_boxes_chain: at most {worst:.2f} ulp32")


def test_word_chars_chain_on_exact_lines(dev):
    """three words 40 long, 20 apart (S = 160, ow = 512: a / ow * S is exact): boxes and ranges equal the float32 restatement with ==.  Line 0
    has a space at the end of its first word and a middle word that holds one space only (an empty range); line 1 has no space between its
    first two words, and a space label of -1 trims nothing."""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    space = inf.space_label(DEFAULT_ALPHABET)
    a = C.straight_line(10.0, 50.0, 0.0, [40.0, 40.0, 40.0], [20.0] * 3, [20.0, 20.0])
    b = C.straight_line(10.0, 150.0, 0.0, [40.0, 40.0, 40.0], [20.0] * 3, [20.0, 20.0])
    words = np.concatenate([a, b])[[3, 0, 5, 1, 4, 2]]
    chains = [[1, 3, 5], [0, 4, 2]]
    lines = _lines(dev, words, chains)
    sp = inf.line_spines(lines)
    plan = inf.crop_plan_chain(sp)
    table = plan.table.cpu().numpy()
    assert [tuple(r) for r in table[:2, :3]] == [(20, 160, 512)] * 2
    c = [space + 1 + k for k in range(6)]  # six labels that are not the space
    # centres 1.25 t against the boundaries 50 and 110: line 0 -> words 0 0 0 0 0 | 1 | 2 2, line 1 -> 0 0 | 1 1 1 | 2 2
    chars = {0: ([c[0], c[1], c[2], c[3], space, space, space, c[4]], [0, 10, 20, 30, 39, 50, 90, 120]),
             1: ([c[0], c[1], c[2], c[3], c[4], space, c[5]], [4, 39, 41, 60, 87, 100, 126])}
    spans, per_row = _stage_spans(dev, table, 2, lambda line: (chars[line][0], chars[line][1], chars[line][1]))
    boxes = inf.char_boxes_chain(sp, plan, spans)
    want = {True: {0: [[0, 4], [6, 6], [7, 8]], 1: [[0, 2], [2, 5], [6, 7]]}, False: {0: [[0, 5], [5, 6], [6, 8]], 1: [[0, 2], [2, 5], [5, 7]]}}
    for sp_label, trimmed in ((space, True), (-1, False)):
        alphabet = DEFAULT_ALPHABET if trimmed else [c for c in DEFAULT_ALPHABET if c != " "]
        ranges = inf.word_chars_chain(sp, plan, spans, boxes, alphabet).cpu().numpy()
        for p in range(2):
            line = int(table[p, 7])
            ref = C.line_spine(words[chains[line]], np.float32)
            labels, t0, t1 = per_row[p]
            box = C.char_boxes(ref, 512, t0, t1, np.float32)
            k = len(t0)
            assert np.array_equal(boxes.s0[p, :k].cpu().numpy(), box["s0"]) and np.array_equal(boxes.quads[p, :k].cpu().numpy(), box["quads"])
            got = ranges[chains[line]].tolist()
            assert got == C.word_ranges(C.word_bounds(ref), box["centre"], labels, sp_label).tolist()
            assert got == want[trimmed][line], (trimmed, line, got)


# ------------------------------------------------------------------ end to end: golden weights ----------------------------------------------
@pytest.fixture(scope="module")
def golden(dev, det_model, rec_model):
    from ocrs_models_amd import inference as inf

    page = TL.dot_page(320, 240).to(dev)
    return page, inf.ocr_lines(det_model, rec_model, page, size=SIZE), inf.ocr_lines(det_model, rec_model, page, size=SIZE, rectify="chain")


def test_ocr_lines_chain_equals_the_stages_chained_by_hand(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, quad, chain = golden
    det = inf.detect_words(det_model, page, size=SIZE)
    lines = inf.find_lines(det["quads"])
    sp = inf.line_spines(lines)
    plan = inf.crop_plan_chain(sp)
    texts = inf.recognize_crops(rec_model, inf.crops_to_batches(inf.rectify_chain(page, sp, plan), plan))
    L = int(lines.n_lines)
    assert len(chain) == len(quad) == L == plan.host()[0] and L > 0
    offs = lines.line_offsets.cpu().tolist()
    knots, dims = sp.knots().cpu(), sp.line_dims.cpu()
    longest = 0
    for l, (c, q) in enumerate(zip(chain, quad)):
        assert list(c) == ["quad", "text", "words", "spine", "height"]
        assert c["quad"] == q["quad"] and c["words"] == q["words"] and c["text"] == texts[l]
        assert c["spine"] == knots[offs[l]:offs[l + 1]].reshape(-1, 2).tolist() and len(c["spine"]) == 2 * len(c["words"])
        assert c["height"] == float(dims[l, 1])
        longest = max(longest, len(c["words"]))
        # the rule's spine for these words
        ref = C.line_spine(np.array(c["words"], dtype=np.float32), np.float64)
        top = max(float(ref["S"]), float(np.abs(np.array(c["words"])).max()))
        assert np.abs(np.array(c["spine"]) - ref["knots"].reshape(-1, 2)).max() <= 2 * C.K_TABLE * R.ulp32(top)
    print(f"golden detector: {det['n']} words, {L} lines, longest {longest}; texts differing from the quad path: {sum(c['text'] != q['text'] for c, q in zip(chain, quad))}")


def test_rectify_quad_is_the_call_without_the_keyword(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, quad, _ = golden
    assert json.dumps(inf.ocr_lines(det_model, rec_model, page, size=SIZE, rectify="quad")) == json.dumps(quad)
    assert inf.ocr_pages(det_model, rec_model, [page], size=SIZE, rectify="quad") == inf.ocr_pages(det_model, rec_model, [page], size=SIZE) == [quad]
    det = inf.detect_words(det_model, page, size=SIZE)
    assert inf.read_lines(rec_model, page, det["quads"], rectify="quad") == quad
    kw = dict(size=SIZE, chars=True, reading_order=True)
    assert inf.ocr_lines(det_model, rec_model, page, rectify="quad", **kw) == inf.ocr_lines(det_model, rec_model, page, **kw)


def test_ocr_pages_chain_equals_ocr_lines_per_page(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, _, chain = golden
    assert inf.ocr_pages(det_model, rec_model, [page], size=SIZE, rectify="chain") == [chain]
    pages = [page, page[:, :200].contiguous()]
    got = inf.ocr_pages(det_model, rec_model, pages, size=SIZE, rectify="chain")
    assert len(got) == 2
    for p, res in zip(pages, got):  # (a crop's chunk, and with it the padded width its text was read at, depends on the whole batch)
        alone = inf.ocr_lines(det_model, rec_model, p, size=SIZE, rectify="chain")
        assert len(alone) == len(res) > 0
        for a, b in zip(alone, res):
            assert list(a) == list(b) and all(a[k] == b[k] for k in ("quad", "words", "spine", "height"))
    # the crops themselves: the batch's store against each page alone
    det = inf.detect_words_batch(det_model, pages, size=SIZE)
    found = inf.find_lines_pages(det["quads"], det["page_of_word"], det["word_offs"])
    sp = inf.line_spines(found)
    plan = inf.crop_plan_chain(sp)
    L, lpo = plan.host()[0], found.line_page_offs.cpu().tolist()
    pooled = _crops_of(inf.rectify_chain_pages(*inf.pack_pages(pages), sp, found.page_of_line, plan).cpu(), plan, L)
    assert lpo[-1] == L == len(got[0]) + len(got[1])
    for p in range(2):
        one = inf.find_lines(inf.detect_words(det_model, pages[p], size=SIZE)["quads"])
        sp1 = inf.line_spines(one)
        plan1 = inf.crop_plan_chain(sp1)
        crops1 = _crops_of(inf.rectify_chain(pages[p], sp1, plan1).cpu(), plan1, plan1.host()[0])
        assert len(crops1) == lpo[p + 1] - lpo[p]
        for a, b in zip(crops1, pooled[lpo[p]:lpo[p + 1]]):
            assert torch.equal(a, b)


def test_chain_composes_with_chars_reading_order_and_beam(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page, _, chain = golden
    full = inf.ocr_lines(det_model, rec_model, page, size=SIZE, rectify="chain", chars=True, reading_order=True, beam_width=4)
    assert len(full) == len(chain)
    by_quad = {json.dumps(c["quad"]): c for c in chain}
    for d in full:
        base = by_quad[json.dumps(d["quad"])]
        assert list(d) == ["quad", "text", "words", "spine", "height", "char_quads", "char_log_probs", "log_prob", "word_chars", "word_texts", "block"]
        assert all(d[k] == base[k] for k in ("words", "spine", "height"))
        assert len(d["char_quads"]) == len(d["text"]) and [d["text"][a:b] for a, b in d["word_chars"]] == d["word_texts"]
        # every character's quad straddles the spine: its corners lie half the crop height to either side, within rounding
        if d["char_quads"]:
            ref = C.line_spine(np.array(d["words"], dtype=np.float32), np.float64)
            q = np.array(d["char_quads"])
            mid = 0.5 * (q[:, 0] + q[:, 3])
            seg = np.array(d["spine"]).reshape(-1, 2)
            dist = np.min(np.linalg.norm(mid[:, None, :] - _polyline(seg, 400)[None], axis=2), axis=1)
            assert dist.max() < 0.75, dist.max()
            assert np.abs(np.linalg.norm(q[:, 0] - q[:, 3], axis=1) - float(ref["H"])).max() < 1e-2
    chars = inf.ocr_lines(det_model, rec_model, page, size=SIZE, rectify="chain", chars=True)
    assert [{k: c[k] for k in b} for b, c in zip(chain, chars)] == chain


def _polyline(pts, per):
    t = np.linspace(0.0, 1.0, per)[:, None]
    return np.concatenate([a + t * (b - a) for a, b in zip(pts[:-1], pts[1:])]) if len(pts) > 1 else pts


def test_argument_errors(dev, det_model, rec_model, golden):
    from ocrs_models_amd import inference as inf

    page = golden[0]
    with pytest.raises(RuntimeError, match="rectify"):
        inf.ocr_lines(det_model, rec_model, page, size=SIZE, rectify="spline")
    with pytest.raises(RuntimeError, match="rectify"):
        inf.ocr_pages(det_model, rec_model, [page], size=SIZE, rectify="Chain")
    with pytest.raises(RuntimeError, match="lines=True"):
        inf.ocr_pages(det_model, rec_model, [page], lines=False, size=SIZE, rectify="chain")
    lines = inf.find_lines(inf.detect_words(det_model, page, size=SIZE)["quads"])
    sp = inf.line_spines(lines)
    with pytest.raises(RuntimeError):
        inf.rectify_chain(page, sp, inf.crop_plan(lines.quads[:2].contiguous()))
    with pytest.raises(RuntimeError):
        inf.rectify_chain(page.float(), sp, inf.crop_plan_chain(sp))
    with pytest.raises(RuntimeError):
        inf.line_spines(lines, out=inf.LineSpines(sp.spine[:-1], sp.line_dims, lines))


# ------------------------------------------------------------------ waits, reproducibility -------------------------------------------------
def test_line_spines_and_the_plan_make_no_host_sync(dev, curved):
    from ocrs_models_amd import inference as inf

    lines = curved["lines"]
    want = inf.line_spines(lines)
    want_plan = inf.crop_plan_chain(want)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = inf.line_spines(lines)
        plan = inf.crop_plan_chain(got)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    nw = sum(len(c) for c in curved["chains"])
    assert torch.equal(got.spine[:2 * nw], want.spine[:2 * nw]) and torch.equal(plan.totals, want_plan.totals)


def test_chain_waits_no_more_often_than_the_default(dev, rec_model):
    """the spine table and the heights are copied with the other line tables ahead of the recogniser: the waits of ocr_lines stay what they
    are.  Counted the way tests/test_lines_gpu.py counts them, on a page with one chunk of crops."""
    from ocrs_models_amd import inference as inf

    bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)]
    page, det = TL.bar_page(230, 340, bars, dev)
    kw = dict(size=(230, 340))
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        inf.ocr_lines(det, rec_model, page, **kw), inf.ocr_lines(det, rec_model, page, rectify="chain", **kw), inf.ocr_lines(det, rec_model, page, rectify="chain", chars=True, **kw)
    plain, n_plain, what_plain = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, **kw))
    chain, n_chain, what_chain = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, rectify="chain", **kw))
    chars, n_chars, what_chars = TL._count_waits(lambda: inf.ocr_lines(det, rec_model, page, rectify="chain", chars=True, **kw))
    print(f"host waits: ocr_lines {n_plain} {what_plain}, chain {n_chain} {what_chain}, chain with chars {n_chars} {what_chars}")
    assert len(plain) == len(chain) == len(chars) == 5 and all(len(c["spine"]) == 12 for c in chain)
    assert n_plain >= 3 and n_chain <= n_plain and n_chars <= n_plain


def test_two_runs_give_identical_bytes(dev, det_model, rec_model, curved, golden):
    from ocrs_models_amd import inference as inf

    sp = inf.line_spines(curved["lines"])
    plan = inf.crop_plan_chain(sp)
    packed = inf.rectify_chain(curved["page"].to(dev), sp, plan)
    nw = sum(len(c) for c in curved["chains"])
    assert torch.equal(sp.spine[:2 * nw], curved["sp"].spine[:2 * nw]) and torch.equal(sp.line_dims[:6], curved["sp"].line_dims[:6])
    assert torch.equal(plan.table[:6], curved["plan"].table[:6]) and torch.equal(plan.totals, curved["plan"].totals)
    assert packed.cpu().numpy().tobytes() == curved["packed"].cpu().numpy().tobytes()
    page, _, chain = golden
    assert json.dumps(inf.ocr_lines(det_model, rec_model, page, size=SIZE, rectify="chain")) == json.dumps(chain)


# ------------------------------------------------------------------ CLI ----------------------------------------------------------------
def test_eval_detection_cli_with_rectify_chain(dev, det_model, rec_model, tmp_path):
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
    cmd = [sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), str(tmp_path / "out"), "--rec-model",
           str(tmp_path / "rec.pt")]
    from ocrs_models_amd import eval_detection

    for bad in (["--rectify", "chain"], ["--lines", "--rectify", "polygon"]):  # refused by the argument parser, before any file is read
        with pytest.raises(SystemExit) as e:
            eval_detection.main([*cmd[3:], *bad])
        assert e.value.code == 2
    r = subprocess.run([*cmd, "--lines", "--rectify", "chain"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert got and all(list(g) == ["quad", "text", "words", "spine", "height"] for g in got)
    assert got == inf.ocr_lines(det_model, rec_model, page_h.to(dev), rectify="chain")

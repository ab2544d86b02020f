"""CPU-only: what the restatement of the chain-crop rule (tests/chain_ref.py) means, independently of any kernel -- a one-word
line is the quad rule, the spine follows an arc, overlapping words jump, degenerate words stay finite, word boundaries ascend -- and how far
its float32 form is from its float64 form on the cases tests/test_chain_gpu.py uses (the constants K_TABLE and K_CROP)."""
import math

import numpy as np
import pytest

from tests import chain_ref as C
from tests import chars_ref as CH
from tests import ocr_ref as R


def test_one_word_line_is_the_quad_rule():
    """same (h, w, ow), and the sample positions of ocr_ref.sample_positions(crop_frame(q)) to 1e-9 px in float64"""
    _, quads = R.rectify_case()
    for q in quads.numpy():
        fr = R.crop_frame(q, np.float64)
        sp = C.line_spine(q[None], np.float64)
        assert C.crop_size(sp) == (fr["h"], fr["w"]) and C.plan_row(sp)[2] == R.line_output_width(fr["h"], fr["w"])
        assert sp["S"] == fr["long"] and sp["H"] == fr["short"] and sp["rows"].shape == (2, 8) and not sp["rows"][1].any()
        px, py = C.sample_positions(sp, np.float64)
        qx, qy = R.sample_positions(fr, np.float64)
        assert px.shape == qx.shape
        assert max(np.abs(px - qx).max(), np.abs(py - qy).max()) <= 1e-9
    # in float32 the plan row is the quad's too: S is 0 + long, H the one short side
    for q in quads.numpy():
        fr, sp = R.crop_frame(q, np.float32), C.line_spine(q[None], np.float32)
        assert C.crop_size(sp) == (fr["h"], fr["w"]) and sp["S"] == fr["long"] and sp["H"] == fr["short"]


def test_one_word_line_gives_the_quad_rules_character_boxes():
    _, quads = R.rectify_case()
    t0, t1 = [0, 3, 9, 20], [1, 7, 9, 30]
    for q in quads.numpy()[:8]:
        sp = C.line_spine(q[None], np.float64)
        ow = C.plan_row(sp)[2]
        a, b = C.char_boxes(sp, ow, t0, t1, np.float64), CH.char_boxes(q, ow, t0, t1, np.float64)
        assert np.abs(a["quads"] - b["quads"]).max() <= 1e-9 and np.array_equal(a["s0"], b["s0"]) and np.array_equal(a["centre"], b["centre"])


def _arc_bound(case, sp):
    """the largest sagitta c^2 / (8 R) of a word of the case plus the largest of a gap: how far the spine may leave the arc"""
    lens = sp["rows"][:2 * sp["n"] - 1, 1]
    return float((lens[0::2] ** 2).max() / (8 * case["radius"]) + (lens[1::2] ** 2).max() / (8 * case["radius"]))


@pytest.mark.parametrize("case", [C.ARC_600, C.ARC_300], ids=["600", "300"])
def test_the_spine_follows_an_arc(case):
    words = C.arc_line(**case)
    sp = C.line_spine(words, np.float64)
    assert (sp["rows"][1:2 * sp["n"] - 1:2, 1] > 0).all()  # every gap has a length
    assert sp["H"] == max(R.crop_frame(q, np.float64)["short"] for q in words) and abs(sp["H"] - max(case["heights"])) < 1e-4
    bound = _arc_bound(case, sp)
    s = np.linspace(0.0, float(sp["S"]), 4001)
    px, py = C.point(sp, s, 0.0)
    off = np.abs(np.hypot(px - case["cx"], py - case["cy"]) - case["radius"])
    print(f"arc of radius {case['radius']}: spine within {off.max():.3f} px of the arc, bound {bound:.3f}; crop {C.crop_size(sp)}")
    assert off.max() <= bound + 1e-3  # (1e-3: the corners are float32)
    # neighbouring columns of the crop are at most a pixel and that sagitta apart on the page, on every row
    px, py = C.sample_positions(sp)
    step = np.hypot(np.diff(px, axis=1), np.diff(py, axis=1))
    assert step.max() <= 1.0 + bound
    # the crop is as high as its text, not as the rectangle around the arc
    rect = R.crop_frame(_line_quad(words), np.float64)
    assert C.crop_size(sp)[0] == round(max(case["heights"])) and rect["h"] > 1.5 * C.crop_size(sp)[0]


def _line_quad(words):
    from tests import lines_ref as L

    return L.line_quad(words, L.word_frames(words, np.float64), list(range(len(words))), np.float64)


def test_overlapping_words_make_a_zero_gap_that_is_never_chosen():
    words = C.overlap_case()
    for T in (np.float32, np.float64):
        sp = C.line_spine(words, T)
        rows = sp["rows"]
        assert rows[1, 1] == 0 and rows[3, 1] == 0 and not rows[1, 4:6].any()
        assert rows[1, 0] == rows[2, 0] and rows[3, 0] == rows[4, 0]  # a zero gap shares its start with the word behind it
        s, _ = C.sample_coords(sp, T)
        seg = C.segment_of(sp, s)
        assert set(seg.tolist()) == {0, 2, 4}
        assert C.segment_of(sp, rows[[2, 4], 0]).tolist() == [2, 4]  # exactly at the shared start: the word
        assert abs(float(sp["S"]) - 270.0) < 1e-3


def test_a_single_pixel_word_is_one_finite_sample():
    for q in (np.array([[33, 44]] * 4, dtype=np.float32), np.array([[7, 9], [7.4, 9], [7.4, 9.3], [7, 9.3]], dtype=np.float32)):
        for T in (np.float32, np.float64):
            sp = C.line_spine(q[None], T)
            assert C.crop_size(sp) == (1, 1)
            px, py = C.sample_positions(sp, T)
            assert px.shape == (1, 1) and np.isfinite(px).all() and np.isfinite(py).all()
            assert abs(px[0, 0] - q[:, 0].mean()) <= 0.5 and abs(py[0, 0] - q[:, 1].mean()) <= 0.5
    # two coincident points as a line: the gap has no length, and nothing divides by it
    sp = C.line_spine(np.array([[[5, 5]] * 4, [[5, 5]] * 4], dtype=np.float32), np.float32)
    assert sp["S"] == 0 and C.crop_size(sp) == (1, 1) and np.isfinite(np.stack(C.sample_positions(sp, np.float32))).all()


def _all_cases():
    return {**C.curved_cases(), "long arc": C.long_arc_case(), "overlap": C.overlap_case()}


def test_word_boundaries_do_not_decrease():
    for name, words in _all_cases().items():
        for T in (np.float32, np.float64):
            sp = C.line_spine(words, T)
            b = C.word_bounds(sp)
            assert len(b) == len(words) - 1 and (np.diff(b) >= 0).all(), name
            assert (b >= sp["rows"][1:-1:2, 0]).all() and (b <= sp["rows"][2::2, 0]).all(), name  # inside its gap


def test_word_ranges_split_in_the_middle_of_the_gap():
    words = C.straight_line(10.0, 50.0, 0.0, [40.0, 40.0, 40.0], [20.0] * 3, [20.0, 20.0])  # S = 160, words at 0..40, 60..100, 120..160
    sp = C.line_spine(words, np.float32)
    assert sp["S"] == 160 and C.word_bounds(sp).tolist() == [50.0, 110.0] and C.plan_row(sp) == (20, 160, 512)
    # characters 16 columns = 5 px wide: edges a -> s = a / 512 * 160
    t0 = [0, 10, 20, 30, 39, 50, 90, 120]
    box = C.char_boxes(sp, 512, t0, t0, np.float32)
    labels = [5, 6, 1, 7, 8, 1, 1, 9]  # 1 = the space
    got = C.word_ranges(C.word_bounds(sp), box["centre"], labels, 1)
    centres = [160 * (4 * t) / 512 for t in t0]  # 0, 12.5, 25, 37.5, 48.75 | 62.5 | 112.5, 150
    assert [sum(c >= b for b in (50.0, 110.0)) for c in centres] == [0, 0, 0, 0, 0, 1, 2, 2]
    assert got.tolist() == [[0, 5], [6, 6], [7, 8]]  # the middle word holds one space: an empty range


def _table_error(words):
    """(largest |float32 - float64| over the spine table, the dims and the character quads, the magnitude its ulp is taken at)"""
    s32, s64 = C.line_spine(words, np.float32), C.line_spine(words, np.float64)
    top = max(float(s64["S"]), float(np.abs(np.asarray(words)).max()))
    err = max(np.abs(s32["rows"].astype(np.float64) - s64["rows"]).max(), abs(float(s32["S"]) - float(s64["S"])), abs(float(s32["H"]) - float(s64["H"])))
    assert C.plan_row(s32) == C.plan_row(s64)
    ow = C.plan_row(s64)[2]
    t0 = np.arange(0, ow // 4, 3)
    b32, b64 = C.char_boxes(s32, ow, t0, t0 + 2, np.float32), C.char_boxes(s64, ow, t0, t0 + 2, np.float64)
    err = max(err, np.abs(b32["quads"].astype(np.float64) - b64["quads"]).max(), np.abs(b32["s0"].astype(np.float64) - b64["s0"]).max())
    return float(err), top


def test_float32_restatement_stays_within_k_ulp_of_the_float64_one():
    """The bounds of tests/test_chain_gpu.py are twice what the float32 restatement of the rule needs against the float64 one on the same
    cases, as the bound of test_ocr_gpu.py::test_rectify_crops is.  This pins that need: K_TABLE for the spine table, the dims and the
    character quads (lines of at most 16 words), K_CROP for the crop values next to the blend's roundings (those lines and the 200-word one)."""
    page, _ = R.rectify_case()
    worst_t = 0.0
    for name, words in C.curved_cases().items():
        assert len(words) <= 16
        err, top = _table_error(words)
        print(f"{name}: table float32 vs float64 {err:.3e} = {err / R.ulp32(top):.2f} ulp32({top:.1f})")
        worst_t = max(worst_t, err / R.ulp32(top))
    ulp, blend = R.ulp32(1023.0), R.RECTIFY_BLEND_ROUNDINGS * R.ulp32(0.5) / 2
    worst_c = 0.0
    for name, words in {**C.curved_cases(), "long arc": C.long_arc_case()}.items():
        s32, s64 = C.line_spine(words, np.float32), C.line_spine(words, np.float64)
        assert (s64["rows"][1:2 * s64["n"] - 1:2, 1] > 0).all() and C.crop_size(s32) == C.crop_size(s64)
        err = float(np.abs(C.rectify(page, s32, np.float32).astype(np.float64) - C.rectify(page, s64, np.float64)).max())
        print(f"{name}: crop float32 vs float64 {err:.3e} = {err / ulp:.2f} ulp32(1023), crop {C.crop_size(s64)}")
        worst_c = max(worst_c, err)
    k_table, k_crop = math.ceil(worst_t), math.ceil(max(0.0, worst_c - blend) / ulp)
    print(f"K_TABLE = {k_table} ({worst_t:.2f}), K_CROP = {k_crop}")
    assert k_table == C.K_TABLE and k_crop == C.K_CROP


def test_argument_errors_come_before_any_launch():
    from ocrs_models_amd import inference as inf

    for bad in ("polygon", None, 1):
        with pytest.raises(RuntimeError, match="rectify"):
            inf.ocr_lines(None, None, None, rectify=bad)
        with pytest.raises(RuntimeError, match="rectify"):
            inf.read_lines(None, None, None, rectify=bad)
        with pytest.raises(RuntimeError, match="rectify"):
            inf.ocr_pages(None, None, [], rectify=bad)
    with pytest.raises(RuntimeError, match="lines=True"):
        inf.ocr_pages(None, None, [], lines=False, rectify="chain")
    assert inf.ocr_pages(None, None, [], rectify="chain") == []
    with pytest.raises(RuntimeError, match="line_spines"):
        inf.line_spines("lines")
    with pytest.raises(RuntimeError, match="crop_plan_chain"):
        inf.crop_plan_chain("spines")


def test_abi_section_and_refusals_without_a_gpu():
    from ocrs_models_amd._lib import ARG_NAMES, HEADER_PATH, lib

    text = open(HEADER_PATH).read()
    section = text[text.index("chain crops ---"):text.index("beam search ---")]
    names = ["ocrs_line_spines", "ocrs_crop_plan_dims", "ocrs_rectify_chain", "ocrs_rectify_chain_pages", "ocrs_char_boxes_chain", "ocrs_word_chars_chain"]
    assert all(f"int {n}(" in section for n in names) and all(n in ARG_NAMES for n in names)
    raw = lib()._dll  # (argtypes come from the header; the last argument is the stream)
    # nothing to do launches nothing and is no error; a missing pointer or a count out of range is refused before any launch
    assert raw.ocrs_line_spines(None, 0, None, 0, None, None, None, None, None) == 0
    assert raw.ocrs_rectify_chain(None, 4, 4, None, None, None, 0, None, None, 0, None, 0, None) == 0
    assert raw.ocrs_char_boxes_chain(None, None, None, 0, None, 0, 0, 1, None, None, None, None, None, None, None) == 0
    assert raw.ocrs_word_chars_chain(None, 0, None, 0, None, None, None, 0, 1, None, None, None, None, -1, None, None) == 0
    assert raw.ocrs_line_spines(None, 4, None, 4, None, None, None, None, None) == 1      # lines but no buffers
    assert raw.ocrs_line_spines(None, 2, None, 4, None, None, None, None, None) == 1      # more lines than words
    assert raw.ocrs_crop_plan_dims(None, None, 4, 64, None, None, None) == 1
    assert raw.ocrs_rectify_chain(None, 0, 4, None, None, None, 0, None, None, 1, None, 0, None) == 1   # an empty page
    assert raw.ocrs_rectify_chain(None, 4, 4, None, None, None, 4, None, None, 1, None, 0, None) == 1   # tiles but no buffers
    assert raw.ocrs_rectify_chain_pages(None, 0, None, None, 1, None, None, None, 4, None, None, None, 1, None, 0, None) == 1
    assert raw.ocrs_char_boxes_chain(None, None, None, 4, None, 4, 5, 1, None, None, None, None, None, None, None) == 1   # more rows than lines
    assert raw.ocrs_word_chars_chain(None, 4, None, 4, None, None, None, 1, 0, None, None, None, None, -1, None, None) == 1  # ld < 1

"""CPU-only checks of the page-inference path (csrc/ocr_infer.hip, ocrs_models_amd/inference/): the ABI is declared and exported, the size
query answers without a GPU, the CPU restatement of the geometry rules (tests/ocr_ref.py) gives the closed-form answers the rules imply, and
the device functions have no CPU fallback."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import ocr_ref as R

ENTRY_POINTS = ("ocrs_binarize_resize_nearest", "ocrs_expand_quads", "ocrs_crop_plan", "ocrs_rectify_crops", "ocrs_resize_aa_packed",
                "ocrs_resize_aa_packed_ws_floats")


def test_header_declares_and_library_exports_the_page_inference_entry_points():
    from ocrs_models_amd import build as b
    from ocrs_models_amd._lib import HEADER_PATH, LIB_PATH, parse_header

    sigs = parse_header(HEADER_PATH)
    assert not [n for n in ENTRY_POINTS if n not in sigs]
    b.build(verbose=False)
    dll = ctypes.CDLL(LIB_PATH)
    assert not [n for n in ENTRY_POINTS if not hasattr(dll, n)]
    # every launcher takes its counts as device pointers plus a capacity, and ends with the stream
    for n in ENTRY_POINTS[:5]:
        assert sigs[n][1].endswith("s"), n


def test_packed_resize_workspace_query_answers_without_gpu():
    from ocrs_models_amd._lib import lib

    L = lib()
    assert L.resize_aa_packed_ws_floats(0) == 0 and L.resize_aa_packed_ws_floats(-5) == 0
    for n in (1, 4, 1000, 64 * 800 * 300 + 1):
        got = L.resize_aa_packed_ws_floats(n)
        assert n <= got < n + 4 and got % 4 == 0


def test_package_re_exports_the_inference_functions():
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference, postprocess

    for name in ("binarize_resize", "expand_quads", "detect_words", "crop_plan", "rectify_crops", "crops_to_batches", "recognize_crops", "ocr_page"):
        assert getattr(oa, name) is getattr(inference, name)
    assert oa.MASK_SIZE == (800, 600) and oa.SHRINK_DISTANCE == 3.0
    assert callable(postprocess.expand_quads_device)


# ------------------------------------------------------------------ expansion rule ------------------------------------------------------
def _corner_sets_equal(a, b, tol=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return all(np.abs(b - p).sum(1).min() < tol for p in a) and all(np.abs(a - p).sum(1).min() < tol for p in b)


def test_expand_axis_aligned_rectangle():
    q = [[10, 20], [50, 20], [50, 30], [10, 30]]
    assert np.allclose(R.expand_quad(q, 3.0), [[7, 17], [53, 17], [53, 33], [7, 33]], atol=1e-12)


def test_expand_rotated_rectangle():
    q = R.rotated_rect(100, 200, 80, 20, 30).astype(np.float64)
    want = R.rotated_rect(100, 200, 86, 26, 30).astype(np.float64)
    got = R.expand_quad(q, 3.0)
    assert np.abs(got - want).max() < 2e-5  # rotated_rect rounds its corners to fp32
    # every edge of the result is parallel to, and 3 away from, the corresponding input edge
    for k in range(4):
        e = q[(k + 1) % 4] - q[k]
        nrm = np.array([e[1], -e[0]]) / np.hypot(*e)
        assert abs(abs(float((got[k] - q[k]) @ nrm)) - 3.0) < 1e-4


def test_expand_single_point_is_unchanged():
    q = np.array([[5.0, 7.0]] * 4)
    assert np.array_equal(R.expand_quad(q, 3.0), q)


def test_expand_segment_becomes_the_rectangle_around_it():
    got = R.expand_quad([[10, 5], [20, 5], [20, 5], [10, 5]], 3.0)
    assert _corner_sets_equal(got, [[7, 2], [23, 2], [23, 8], [7, 8]])
    got = R.expand_quad([[4, 1], [4, 1], [4, 9], [4, 9]], 2.0)  # the other pairing of the hull's two points
    assert _corner_sets_equal(got, [[2, -1], [6, -1], [6, 11], [2, 11]])


@pytest.mark.parametrize("flip", [False, True])
def test_expand_keeps_corner_correspondence_in_both_orientations(flip):
    q = R.rotated_rect(300, 100, 60, 24, -20, flip=flip).astype(np.float64)
    got = R.expand_quad(q, 3.0)
    c = q.mean(0)
    for k in range(4):  # corner k moves straight away from the centre's side of both of its edges, by (3, 3) in the rectangle's own axes
        d = got[k] - q[k]
        assert abs(np.hypot(*d) - 3.0 * math.sqrt(2.0)) < 1e-4
        assert float(d @ (q[k] - c)) > 0
    assert _corner_sets_equal(got, R.rotated_rect(300, 100, 66, 30, -20).astype(np.float64), tol=1e-4)


def test_expand_quads_keeps_the_shape():
    q = torch.rand(2, 3, 4, 2)
    assert R.expand_quads(q, 1.0).shape == q.shape


# ------------------------------------------------------------------ crop-frame rule ------------------------------------------------------
def test_frame_upright_text():
    fr = R.crop_frame(R.rotated_rect(100, 50, 80.2, 20.3, 0))
    assert np.allclose(fr["u"], [1, 0]) and np.allclose(fr["v"], [0, 1])
    assert np.allclose(fr["origin"], [100 - 40.1, 50 - 10.15], atol=1e-4) and (fr["h"], fr["w"]) == (20, 80)


@pytest.mark.parametrize("deg", [20, -20])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("start", [0, 1, 2, 3])
def test_frame_rotated_text_is_never_mirrored(deg, flip, start):
    q = np.roll(R.rotated_rect(200, 300, 120.3, 30.4, deg, flip=flip), start, axis=0)
    fr = R.crop_frame(q)
    t = np.deg2rad(deg)
    assert np.allclose(fr["u"], [np.cos(t), np.sin(t)], atol=1e-5)
    assert np.allclose(fr["v"], [-np.sin(t), np.cos(t)], atol=1e-5) and fr["v"][1] > 0
    want_origin = np.array([200, 300]) - 60.15 * fr["u"] - 15.2 * fr["v"]
    assert np.allclose(fr["origin"], want_origin, atol=1e-3) and (fr["h"], fr["w"]) == (30, 120)
    px, py = R.sample_positions(fr)
    # the first sample sits half a sample inside the origin corner, the last one half a sample inside the opposite corner
    assert np.allclose([px[0, 0], py[0, 0]], fr["origin"] + 0.5 * 120.3 / 120 * fr["u"] + 0.5 * 30.4 / 30 * fr["v"], atol=1e-3)
    assert np.allclose([px[-1, -1], py[-1, -1]], np.array([200, 300]) * 2 - [px[0, 0], py[0, 0]], atol=1e-3)


def test_frame_vertical_quad_reads_downwards():
    fr = R.crop_frame(R.rotated_rect(50, 400, 100.2, 20.3, 90))
    assert np.allclose(fr["u"], [0, 1], atol=1e-6) and np.allclose(fr["v"], [-1, 0], atol=1e-6)
    assert (fr["h"], fr["w"]) == (20, 100)
    assert np.allclose(fr["origin"], [50 + 10.15, 400 - 50.1], atol=1e-4)  # top-right corner: u runs down, v runs left


def test_frame_tie_takes_the_side_with_the_larger_x_component():
    for start in range(4):
        fr = R.crop_frame(np.roll(R.rotated_rect(40, 40, 32, 32, 0), start, axis=0))
        assert np.allclose(fr["u"], [1, 0]) and np.allclose(fr["origin"], [24, 24]) and (fr["h"], fr["w"]) == (32, 32)


def test_frame_of_degenerate_quads():
    fr = R.crop_frame(np.array([[3, 4]] * 4, dtype=np.float32))
    assert np.allclose(fr["u"], [1, 0]) and (fr["h"], fr["w"]) == (1, 1) and np.allclose(fr["origin"], [3, 4])
    fr = R.crop_frame(np.array([[9, 2], [1, 2], [1, 2], [9, 2]], dtype=np.float32))
    assert np.allclose(fr["u"], [1, 0]) and (fr["h"], fr["w"]) == (1, 8) and np.allclose(fr["origin"], [1, 2])


def test_float32_restatement_of_the_rectification_stays_within_k_ulp_of_the_float64_one():
    """The bound of tests/test_ocr_gpu.py::test_rectify_crops is k * ulp32(largest page coordinate) * (value range 1.0) + the fp32 roundings of
    the blend, with k twice what the float32 restatement of the rule needs against the float64 one on the same case.  This pins that need: 2."""
    page, quads = R.rectify_case()
    ulp, blend = R.ulp32(1023.0), R.RECTIFY_BLEND_ROUNDINGS * R.ulp32(0.5) / 2
    worst = 0.0
    for q in quads:
        worst = max(worst, float(np.abs(R.rectify_f64(page, q).numpy() - R.rectify_f32(page, q)).max()))
    k = math.ceil(max(0.0, worst - blend) / ulp)
    print(f"float32 restatement vs float64: max {worst:.3e} = {worst / ulp:.2f} ulp32(1023) -> k = {k}")
    assert k == R.RECTIFY_K_CPU == 2


def test_batching_rule():
    order, chunks, ows = R.batching([(20, 100), (64, 64), (10, 400), (30, 30), (64, 64)], max_batch=2, width_unit=64)
    assert ows == [320, 64, 800, 64, 64]
    assert order == [1, 3, 4, 0, 2] and chunks == [(0, 2, 128), (2, 2, 384), (4, 1, 832)]


def test_plan_chunks_matches_the_restated_batching_rule():
    from ocrs_models_amd.inference import plan_chunks

    r = np.random.RandomState(3)
    hw = [(int(r.randint(1, 80)), int(r.randint(1, 600))) for _ in range(300)]
    for max_batch, unit in ((256, 64), (7, 64), (1, 4), (300, 256), (1000, 64)):
        _, chunks, ows = R.batching(hw, max_batch, unit)
        hist = np.bincount(ows, minlength=801).tolist()
        assert plan_chunks(hist, max_batch, unit) == chunks
    assert plan_chunks([0] * 801, 256, 64) == []


# ------------------------------------------------------------------ span buffer layout --------------------------------------------------
def test_span_views_state_the_buffer_layout_on_a_cpu_buffer():
    """labels | t0 | t1 | peak | lens: what is written through the views of ``span_arrays`` is read back through ``span_views`` of the flat
    buffer and through the host reader of the decode handles; a beam row without a labelling (-1) and an empty row both read as empty."""
    from ocrs_models_amd import text

    rows, ld = 3, 4
    buf, labels, t0, t1, peak, lens = text.span_arrays(rows, ld, "cpu")
    assert buf.dtype == torch.int32 and buf.numel() == 4 * rows * ld + rows
    buf.fill_(-7)
    labels[0, :2] = torch.tensor([5, 9], dtype=torch.int32)
    t0[0, :2] = torch.tensor([0, 3], dtype=torch.int32)
    t1[0, :2] = torch.tensor([1, 3], dtype=torch.int32)
    peak[0, :2] = torch.tensor([-0.125, -1.5])
    lens.copy_(torch.tensor([2, 0, -1], dtype=torch.int32))
    # the views alias the one buffer, part after part
    assert buf[:2].tolist() == [5, 9] and buf[rows * ld:rows * ld + 2].tolist() == [0, 3] and buf[2 * rows * ld:2 * rows * ld + 2].tolist() == [1, 3]
    assert buf[3 * rows * ld:3 * rows * ld + 2].view(torch.float32).tolist() == [-0.125, -1.5] and buf[4 * rows * ld:].tolist() == [2, 0, -1]
    got = text.span_views(buf.clone(), rows, ld)  # (the pinned copy of a device buffer is such a flat tensor)
    assert [tuple(v.shape) for v in got] == [(rows, ld)] * 4 + [(rows,)]
    assert got[3].dtype == torch.float32 and all(v.dtype == torch.int32 for v in got[:3] + got[4:])
    assert got[0][0, :2].tolist() == [5, 9] and got[1][0, :2].tolist() == [0, 3] and got[2][0, :2].tolist() == [1, 3]
    assert got[3][0, :2].tolist() == [-0.125, -1.5]
    assert got[4].tolist() == [2, 0, -1] and text.span_lengths(got[4]) == [2, 0, 0]

    class Arrived:
        def synchronize(self):
            pass

    handle = text._DecodeSpans((buf, labels, t0, t1, peak, lens), buf.clone(), Arrived(), rows, ld, None)
    empty = {"labels": [], "t0": [], "t1": [], "peak": []}
    assert handle.result() == [{"labels": [5, 9], "t0": [0, 3], "t1": [1, 3], "peak": [-0.125, -1.5]}, empty, empty]


# ------------------------------------------------------------------ result assembly -----------------------------------------------------
def _quad(i):
    return [[10.0 * i, 0.0], [10.0 * i + 8, 0.0], [10.0 * i + 8, 4.0], [10.0 * i, 4.0]]


_WORDS = [_quad(i) for i in range(5)]                 # words 0..2 on page 0, 3..4 on page 1, in raster order
_LINE_QUADS = [_quad(20), _quad(21), _quad(22)]       # lines 0, 1 on page 0, line 2 on page 1
_LINES = (_LINE_QUADS, [2, 0, 1, 3, 4], [0, 2, 3, 5])  # line 0 = words 2, 0 (chain order is not raster order), line 1 = word 1, line 2 = words 3, 4
_READING = ([1, 0, 2], [0, 1, 0], [0, 2, 3])           # page 0 is read line 1, then line 0 in a block of its own; page 1 starts again at block 0
_LINE_TEXTS = ["ab cd", "ef", "gh i"]
_LINE_RANGES = [[3, 5], [0, 2], [0, 2], [0, 2], [3, 4]]  # by flat word index
_WORD_TEXTS = ["w0", "w1", "w2", "w3", "w4"]
_OPTIONS = [dict(), dict(beam=True), dict(beam=True, lm=True), dict(chars=True), dict(chars=True, beam=True), dict(chars=True, beam=True, lm=True)]


def _record(texts, perm, ranges=None, chars=False, beam=False, lm=False):
    """the ``Decoded`` of crops whose rows arrive in width-sorted order: row ``perm[i]`` is quad i's.  -> (record, the per-quad values)"""
    from ocrs_models_amd.inference import Decoded

    n = len(texts)
    assert sorted(perm) == list(range(n)) and perm != list(range(n))
    want = {"text": texts}
    if chars:
        want["char_quads"] = [[_quad(100 * i + k) for k in range(len(t))] for i, t in enumerate(texts)]
        want["char_log_probs"] = [[-0.25 * (k + 1) - i for k in range(len(t))] for i, t in enumerate(texts)]
    if beam:
        want["log_prob"] = [-1.5 - i for i in range(n)]
    if lm:
        want["lm_score"] = [-0.5 * i for i in range(n)]
    rows = {key: [None] * n for key in want}
    for i, p in enumerate(perm):
        for key in want:
            rows[key][p] = want[key][i]
    char_rows = [{"char_quads": q, "char_log_probs": s} for q, s in zip(rows["char_quads"], rows["char_log_probs"])] if chars else None
    rec = Decoded.in_quad_order(perm, rows["text"], rows.get("log_prob"), rows.get("lm_score"), char_rows, ranges if chars else None)
    return rec, want


@pytest.mark.parametrize("opts", _OPTIONS, ids=lambda o: "+".join(o) or "greedy")
def test_assemble_results_word_dicts(opts):
    from ocrs_models_amd.inference import assemble_results

    rec, want = _record(_WORD_TEXTS, [3, 0, 4, 1, 2], **opts)
    keys = ["quad", "text"] + [k for k in ("char_quads", "char_log_probs", "log_prob", "lm_score") if k in want]
    got = assemble_results(rec, _WORDS)
    assert got == [{"quad": _WORDS[i], **{k: want[k][i] for k in keys[1:]}} for i in range(5)]
    assert all(list(d) == keys for d in got)


@pytest.mark.parametrize("reading", [False, True], ids=["line-order", "reading-order"])
@pytest.mark.parametrize("opts", _OPTIONS, ids=lambda o: "+".join(o) or "greedy")
def test_assemble_results_line_dicts(opts, reading):
    from ocrs_models_amd.inference import assemble_results

    rec, want = _record(_LINE_TEXTS, [2, 0, 1], _LINE_RANGES, **opts)
    words_of = [[_WORDS[2], _WORDS[0]], [_WORDS[1]], [_WORDS[3], _WORDS[4]]]
    lines = []
    for l in range(3):
        d = {"quad": _LINE_QUADS[l], "text": _LINE_TEXTS[l], "words": words_of[l]}
        d.update({k: want[k][l] for k in ("char_quads", "char_log_probs", "log_prob", "lm_score") if k in want})
        lines.append(d)
    keys = ["quad", "text", "words"] + [k for k in ("char_quads", "char_log_probs", "log_prob", "lm_score") if k in want]
    if opts.get("chars"):
        for d, rg, texts in zip(lines, ([[0, 2], [3, 5]], [[0, 2]], [[0, 2], [3, 4]]), (["ab", "cd"], ["ef"], ["gh", "i"])):
            d["word_chars"], d["word_texts"] = rg, texts
        keys += ["word_chars", "word_texts"]
    if reading:
        lines = [{**lines[1], "block": 0}, {**lines[0], "block": 1}, {**lines[2], "block": 0}]  # block restarts on the second page
        keys += ["block"]
    got = assemble_results(rec, _WORDS, _LINES, _READING if reading else None)
    assert got == lines
    assert all(list(d) == keys for d in got)


def test_assemble_results_needs_nothing_from_the_gpu_side():
    import ast
    import inspect

    from ocrs_models_amd.inference import assemble

    imported = [n for n in ast.walk(ast.parse(inspect.getsource(assemble))) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert [getattr(n, "module", None) for n in imported] == ["__future__"]


# ------------------------------------------------------------------ no CPU path ---------------------------------------------------------
def test_inference_has_no_cpu_path():
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.postprocess import expand_quads_device

    q = torch.zeros(2, 4, 2)
    page = torch.zeros(1, 32, 32, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        inf.binarize_resize(torch.zeros(1, 1, 8, 8), (16, 16))
    with pytest.raises(RuntimeError):
        inf.expand_quads(q, 3.0)
    with pytest.raises(RuntimeError):
        expand_quads_device(q, 3.0)
    with pytest.raises(RuntimeError):
        inf.crop_plan(q)
    with pytest.raises(RuntimeError):
        inf.detect_words(oa.DetectionModel().eval(), page)
    with pytest.raises(RuntimeError):
        inf.ocr_page(oa.DetectionModel().eval(), oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).eval(), page)
    plan = inf.CropPlan(torch.zeros(2, 8, dtype=torch.int32), torch.zeros(805, dtype=torch.int64), 64)
    with pytest.raises(RuntimeError):
        inf.rectify_crops(page, q, plan)
    with pytest.raises(RuntimeError):
        inf.crops_to_batches(torch.zeros(16), plan)
    with pytest.raises(RuntimeError):
        inf.recognize_crops(oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).eval(), ([torch.zeros(1, 1, 64, 64)], [torch.tensor([64])], [0]))

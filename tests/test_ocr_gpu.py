"""Page inference on the GPU (csrc/ocr_infer.hip, ocrs_models_amd/inference/) against the CPU restatement of its rules (tests/ocr_ref.py),
torch's CPU operators and the package's own single-crop functions.

Tolerances.  binarize_resize, the pad columns, chunking and the per-crop resize are BIT-EXACT (a compare and an index rule; the same filter
code as ``resize``).  expand_quads: 4 * ulp32(largest |coordinate|), derived from the inputs.  rectify_crops: k * ulp32(largest page
coordinate) * (value range 1.0) + the fp32 roundings of the blend, k = 4 = twice what the float32 CPU restatement needs against the float64
one (tests/test_ocr_host.py pins that 2).  The tests print the measured maxima before they assert (DESIGN.md §11 records them)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ocr_ref as R
from tests.golden_util import DET_CASES, REC_CASE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def dot_page(H, W, step=16, size=6):
    """dark dots on a light page: with the golden detection weights this gives several hundred separate components"""
    y, x = np.mgrid[0:H, 0:W]
    p = np.full((H, W), 230, np.uint8)
    p[((y % step) < size) & ((x % step) < size)] = 20
    return torch.from_numpy(p)[None]


# ------------------------------------------------------------------ binarize_resize ------------------------------------------------------
@pytest.mark.parametrize("size", [(1024, 768), (1333, 1000), (601, 799), (800, 600), (300, 200)])
@pytest.mark.parametrize("B", [1, 3])
def test_binarize_resize_bit_exact(dev, size, B):
    from ocrs_models_amd import inference as inf

    g = torch.Generator().manual_seed(size[0] + B)
    p = torch.rand(B, 1, 800, 600, generator=g)
    p[:, :, ::7, ::5] = 0.5  # values on the threshold are background (strict >)
    want = F.interpolate((p > 0.5).float(), size=size, mode="nearest").to(torch.uint8)
    got = inf.binarize_resize(p.to(dev), size, 0.5)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 1, *size)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(inf.binarize_resize(p[0, 0].to(dev), size).cpu(), want[0, 0])
    t = 0.8125
    assert torch.equal(inf.binarize_resize(p.to(dev), size, t).cpu(), R.binarize_resize(p, size, t))


# ------------------------------------------------------------------ expand_quads --------------------------------------------------------
def _expand_inputs():
    r = np.random.RandomState(7)
    quads = [R.rotated_rect(r.uniform(50, 1900), r.uniform(50, 1400), r.uniform(2, 300), r.uniform(1, 80), r.uniform(-180, 180), flip=bool(i & 1))
             for i in range(61)]
    quads += [np.array([[5, 7]] * 4, dtype=np.float32), np.array([[10, 5], [20, 5], [20, 5], [10, 5]], dtype=np.float32),
              np.array([[4, 1], [4, 1], [4, 9], [4, 9]], dtype=np.float32)]
    return torch.from_numpy(np.stack(quads))


def test_expand_quads_matches_the_rule(dev):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.postprocess import expand_quads_device

    q = _expand_inputs()
    bound = 4 * R.ulp32(float(q.abs().max()) + 3.0)
    got = inf.expand_quads(q.to(dev), 3.0)
    err = (got.cpu().double() - R.expand_quads(q, 3.0)).abs().max().item()
    print(f"expand_quads: max error {err:.3e} = {err / R.ulp32(float(q.abs().max()) + 3.0):.2f} ulp32, bound {bound:.3e}")
    assert got.shape == q.shape and got.dtype == torch.float32 and err <= bound
    assert torch.equal(got[61].cpu(), q[61])  # a point is returned unchanged
    assert torch.equal(expand_quads_device(q.to(dev), 3.0), got)


def test_expand_quads_with_counts_leaves_the_rest_untouched(dev):
    from ocrs_models_amd import inference as inf

    q = _expand_inputs().reshape(4, 16, 4, 2)
    counts = torch.tensor([16, 0, 5, 11], dtype=torch.int32)
    got = inf.expand_quads(q.to(dev), 2.5, counts.to(dev)).cpu()
    want = R.expand_quads(q, 2.5)
    bound = 4 * R.ulp32(float(q.abs().max()) + 2.5)
    assert got.shape == q.shape
    for b, n in enumerate(counts.tolist()):
        assert (got[b, :n].double() - want[b, :n]).abs().max().item() <= bound if n else True
        assert torch.equal(got[b, n:], q[b, n:])
    assert (inf.expand_quads(q.to(dev), 2.5).cpu().double() - want).abs().max().item() <= bound


# ------------------------------------------------------------------ crop_plan / rectify_crops ---------------------------------------------
def _crops_of(packed, plan):
    tab = plan.table.cpu()
    return [packed[int(o):int(o) + int(h) * int(w)].view(int(h), int(w)) for h, w, _, o in tab[:, :4].tolist()]


def test_crop_plan_follows_the_frame_and_batching_rules(dev):
    from ocrs_models_amd import inference as inf

    _, quads = R.rectify_case()
    plan = inf.crop_plan(quads.to(dev))
    tab, tot = plan.table.cpu(), plan.host()
    frames = [R.crop_frame(q, np.float32) for q in quads]
    hw = [(f["h"], f["w"]) for f in frames]
    assert [tuple(r) for r in tab[:, :2].tolist()] == hw
    order, _, ows = R.batching(hw, 256, 64)
    assert tab[:, 2].tolist() == ows
    assert tab[:, 7].tolist() == order and [order[p] for p in tab[:, 6].tolist()] == list(range(len(hw)))
    offs = np.cumsum([0] + [(h * w + 3) // 4 * 4 for h, w in hw])
    assert tab[:, 3].tolist() == offs[:-1].tolist() and tot[1] == offs[-1]
    assert tab[:, 4].tolist() == np.cumsum([0] + [h * o for (h, _), o in zip(hw, ows)])[:-1].tolist() and tot[2] == sum(h * o for (h, _), o in zip(hw, ows))
    assert tab[:, 5].tolist() == np.cumsum([0] + [(h * w + 1023) // 1024 for h, w in hw])[:-1].tolist() and tot[3] == sum((h * w + 1023) // 1024 for h, w in hw)
    assert tot[0] == len(hw) and tot[4:] == np.bincount(ows, minlength=801).tolist()


def test_rectify_crops_matches_grid_sample(dev):
    from ocrs_models_amd import inference as inf

    page, quads = R.rectify_case()
    assert len(quads) == 12
    plan = inf.crop_plan(quads.to(dev))
    packed = inf.rectify_crops(page.to(dev), quads.to(dev), plan).cpu()
    k = 2 * R.RECTIFY_K_CPU
    ulp = R.ulp32(max(page.shape[-2:]) - 1)
    bound = k * ulp * 1.0 + R.RECTIFY_BLEND_ROUNDINGS * R.ulp32(0.5) / 2
    worst = 0.0
    for q, crop in zip(quads, _crops_of(packed, plan)):
        want = R.rectify_f64(page, q)
        assert tuple(crop.shape) == tuple(want.shape)
        worst = max(worst, (crop.double() - want).abs().max().item())
    print(f"rectify_crops: max error {worst:.3e} = {worst / ulp:.2f} ulp32({max(page.shape[-2:]) - 1}), bound {bound:.3e} (k = {k})")
    assert worst <= bound


# ------------------------------------------------------------------ crops_to_batches ----------------------------------------------------
def _many_quads(n, seed, H=1024, W=768):
    r = np.random.RandomState(seed)
    return torch.from_numpy(np.stack([R.rotated_rect(r.uniform(0, W), r.uniform(0, H), r.uniform(1, 260), r.uniform(1, 70), r.uniform(-40, 40))
                                      for _ in range(n)]))


@pytest.mark.parametrize("max_batch,unit", [(256, 64), (16, 64), (5, 4)])
def test_crops_to_batches_bit_identical_to_resize_line(dev, max_batch, unit):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import input_pipeline as ip
    from oracle import input_pipe as oip

    page, quads = R.rectify_case()
    quads = torch.cat([quads, _many_quads(40, 5)])
    plan = inf.crop_plan(quads.to(dev))
    packed = inf.rectify_crops(page.to(dev), quads.to(dev), plan)
    batches, widths, perm = inf.crops_to_batches(packed, plan, max_batch, unit)
    crops = _crops_of(packed, plan)
    order, chunks, ows = R.batching([tuple(c.shape) for c in crops], max_batch, unit)
    assert len(batches) == len(chunks) == len(widths)
    assert isinstance(perm, list) and [order[p] for p in perm] == list(range(len(crops)))
    worst = 0.0
    for (p0, cnt, wpad), b, iw in zip(chunks, batches, widths):
        assert tuple(b.shape) == (cnt, 1, 64, wpad) and b.dtype == torch.float32
        assert iw.dtype == torch.int64 and iw.tolist() == [ows[i] for i in order[p0:p0 + cnt]]
        for slot, i in enumerate(order[p0:p0 + cnt]):
            alone = ip.resize_line(crops[i][None].contiguous())
            assert alone.shape[-1] == ows[i]
            assert torch.equal(b[slot, :, :, :ows[i]], alone)
            assert (b[slot, :, :, ows[i]:] == 0.0).all()
            worst = max(worst, (b[slot, :, :, :ows[i]].cpu() - oip.resize_aa(crops[i][None].cpu(), [64, ows[i]])).abs().max().item())
    assert worst < 2e-6


# ------------------------------------------------------------------ detect_words --------------------------------------------------------
def test_detect_words_equals_the_stages_chained_by_hand(dev, det_model):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import input_pipeline as ip
    from ocrs_models_amd.postprocess import extract_cc_quads_device

    page = dot_page(320, 240).to(dev)
    size = (160, 120)
    det = inf.detect_words(det_model, page, size=size)
    with torch.inference_mode():
        probs = det_model(ip.resize(ip.transform_image(page), size).unsqueeze(0))[0, 0]
    assert tuple(det["probs"].shape) == size and torch.equal(det["probs"], probs)
    mask = inf.binarize_resize(probs, (320, 240), 0.5)
    assert det["text_mask"].dtype == torch.uint8 and torch.equal(det["text_mask"], mask)
    assert torch.equal(det["text_mask"].cpu(), R.binarize_resize(probs.cpu(), (320, 240), 0.5))
    quads = inf.expand_quads(extract_cc_quads_device(mask), inf.SHRINK_DISTANCE)
    assert det["n"] == quads.shape[0] > 0 and torch.equal(det["quads"], quads)
    with pytest.raises(RuntimeError):
        inf.detect_words(det_model, page.float())


def test_quads_of_five_rotated_bars(dev):
    """a hand-painted mask of five separated rotated bars: device quads + device expansion == ocr_ref.expand_quads of the host quads, as corner
    sets (the vertex order of a quad is UNPINNED)"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.postprocess import extract_cc_quads, extract_cc_quads_device

    H, W = 400, 600
    y, x = np.mgrid[0:H, 0:W]
    mask = np.zeros((H, W), np.uint8)
    for cx, cy, lng, sht, deg in [(100, 60, 120, 18, 0), (400, 80, 150, 24, 12), (150, 220, 130, 20, -25), (450, 260, 160, 16, 40), (300, 350, 90, 30, 90)]:
        t = np.deg2rad(deg)
        pu, pv = (x - cx) * np.cos(t) + (y - cy) * np.sin(t), -(x - cx) * np.sin(t) + (y - cy) * np.cos(t)
        mask[(np.abs(pu) <= lng / 2) & (np.abs(pv) <= sht / 2)] = 1
    m = torch.from_numpy(mask)
    host = extract_cc_quads(m)
    assert host.shape[0] == 5
    want = R.expand_quads(host, 3.0)
    got = inf.expand_quads(extract_cc_quads_device(m.to(dev)), 3.0).cpu().double()
    assert got.shape == want.shape
    # the expand_quads bound, from the largest coordinate that occurs (the expanded corners are the larger ones)
    top = max(float(host.abs().max()), float(want.abs().max()))
    bound = 4 * R.ulp32(top)
    worst = 0.0
    for g, w in zip(got, want):
        d = (g[:, None, :] - w[None, :, :]).abs().amax(-1)  # [device corner][host corner]
        worst = max(worst, d.min(1).values.max().item(), d.min(0).values.max().item())
    print(f"five bars: max corner distance {worst:.3e} = {worst / R.ulp32(top):.2f} ulp32({top:.1f}), bound {bound:.3e}")
    assert worst <= bound


# ------------------------------------------------------------------ ocr_page -----------------------------------------------------------
def _stages(det_model, rec_model, page, size, max_batch):
    from ocrs_models_amd import inference as inf

    det = inf.detect_words(det_model, page, size=size)
    plan = inf.crop_plan(det["quads"])
    packed = inf.rectify_crops(page, det["quads"], plan)
    batches = inf.crops_to_batches(packed, plan, max_batch)
    return det, batches, inf.recognize_crops(rec_model, batches)


def test_ocr_page_equals_the_stages_and_keeps_raster_order(dev, det_model, rec_model):
    from ocrs_models_amd import inference as inf

    page = dot_page(320, 240).to(dev)
    size = (160, 120)
    for max_batch in (256, 100):
        det, batches, texts = _stages(det_model, rec_model, page, size, max_batch)
        assert det["n"] > max_batch and len(batches[0]) == -(-det["n"] // max_batch) > 1  # more components than one chunk holds
        got = inf.ocr_page(det_model, rec_model, page, size=size, max_batch=max_batch)
        assert [g["text"] for g in got] == texts and len(got) == det["n"]
        # raster order is extract_cc_quads_device's: ocr_page keeps it if its quads are detect_words' quads, row for row
        assert torch.equal(torch.tensor([g["quad"] for g in got]), det["quads"].cpu())


def test_ocr_page_of_an_empty_page(dev, det_model):
    from ocrs_models_amd import inference as inf

    class NeverCalled(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the recogniser must not run for a page without words")

    page = torch.full((1, 200, 160), 255, dtype=torch.uint8, device=dev)
    assert inf.ocr_page(det_model, NeverCalled().eval(), page, size=(128, 96), threshold=1.0) == []
    det = inf.detect_words(det_model, page, size=(128, 96), threshold=1.0)
    assert det["n"] == 0 and tuple(det["quads"].shape) == (0, 4, 2) and int(det["text_mask"].sum()) == 0
    plan = inf.crop_plan(det["quads"])
    batches, widths, perm = inf.crops_to_batches(inf.rectify_crops(page, det["quads"], plan), plan)
    assert batches == [] and widths == [] and perm == []


@pytest.mark.parametrize("opts", [{}, {"chars": True, "beam_width": 4}], ids=["greedy", "chars+beam4"])
def test_read_words_is_the_half_of_ocr_page_after_detection(dev, rec_model, opts):
    """30 bars of five widths, so the width-sorted crops are no run of the raster order, in chunks of 8: read_words on detect_words' quads
    returns what ocr_page returns for the page, dict for dict"""
    from ocrs_models_amd import inference as inf
    from tests.test_lines_gpu import bar_page

    bars = [(15 + 52 * c, 18 + 40 * r, 24 + 4 * ((7 * (6 * r + c)) % 5), 12) for r in range(5) for c in range(6)]
    page, det_model = bar_page(230, 340, bars, dev)
    det = inf.detect_words(det_model, page, size=(230, 340))
    assert det["n"] == 30
    perm = inf.crop_plan(det["quads"]).host_perm()
    assert sorted(perm) == list(range(30)) and perm != list(range(30))
    want = inf.ocr_page(det_model, rec_model, page, size=(230, 340), max_batch=8, **opts)
    got = inf.read_words(rec_model, page, det["quads"], max_batch=8, **opts)
    keys = ["quad", "text"] + (["char_quads", "char_log_probs", "log_prob"] if opts else [])
    assert len(got) == 30 and all(list(d) == keys for d in got)
    assert got == want
    assert torch.equal(torch.tensor([d["quad"] for d in got]), det["quads"].cpu())


# ------------------------------------------------------------------ CLI ----------------------------------------------------------------
def test_eval_detection_cli_writes_the_four_files(dev, tmp_path):
    import ocrs_models_amd as oa
    from ocrs_models_amd.checkpoint import save_checkpoint
    from PIL import Image

    det = oa.DetectionModel()
    det.load_state_dict(_golden_state("det"))
    rec = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    rec.load_state_dict(_golden_state("rec"))
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    save_checkpoint(str(tmp_path / "rec.pt"), rec, oa.optim.Adam(rec.parameters()), 0)
    W, H = 600, 800  # the evaluation size, so the two pictures the reference writes at that size have the page's size too
    Image.fromarray(dot_page(H, W)[0].numpy()).save(tmp_path / "page.png")
    base = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "ocrs_models_amd.eval_detection", str(tmp_path / "det.pt"), str(tmp_path / "page.png"), base,
                        "--rec-model", str(tmp_path / "rec.pt")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Predicted text in" in r.stderr
    for name in ("input", "text-regions", "text-probs", "text-words"):
        with Image.open(f"{base}-{name}.png") as im:
            assert im.size == (W, H), name
    with Image.open(f"{base}-text-words.png") as im:
        assert im.mode == "RGB"
    import json

    words = [json.loads(line) for line in r.stdout.splitlines() if line.strip()]
    assert words and all(set(w) == {"quad", "text"} and np.asarray(w["quad"]).shape == (4, 2) for w in words)

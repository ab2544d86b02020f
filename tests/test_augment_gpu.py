"""The training augmentations (ocrs_models_amd/augment.py, csrc/augment.hip) against the CPU comparand tests/augment_ref.py.

Tolerances: every path is a short chain of fp32 operations restated from ATen's CPU kernels, FMAs included, so 2e-6 absolute on values in
[-0.5, 1] covers the contrast mean's summation order and the resize's accumulation order.  The nearest affine path rounds grid
coordinates: an ulp there flips exact .5 ties, so at most 1e-4 of its pixels may differ by more.  bf16 output: one bf16 ulp of the fp32
comparand (plus the fp32 tolerance)."""
import random

import pytest
import torch

from ocrs_models_amd import augment as A
from tests import augment_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-6
DET_SIZES = [(1600, 1200), (599, 601), (480, 640), (500, 480), (2001, 37)]
LINE_SIZES = [(48, 300), (37, 211), (64, 64), (20, 500), (90, 40), (1, 9)]


def _u8(h, w, seed):
    return torch.randint(0, 256, (1, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _mask(h, w, seed):
    return (torch.rand(1, h, w, generator=torch.Generator().manual_seed(seed + 1000)) > 0.7).to(torch.uint8)


def _pf(x):
    return x.float() / 255.0 - 0.5


def _draw(branch, size, line=False):
    """A real draw of the sampler that took the wanted branch (seeded, so the test is fixed)."""
    sampler = A.sample_line_params if line else A.sample_detection_params
    for s in range(1000):
        p = sampler([size], torch.Generator().manual_seed(s), random.Random(s))[0]
        if p.branch == branch:
            return p
    raise AssertionError("branch never drawn")


def _check(got, want, nearest=False):
    d = (got.float().cpu() - want).abs()
    if nearest:
        assert (d > TOL).float().mean().item() <= 1e-4, (d > TOL).float().mean().item()
    else:
        assert d.max().item() <= TOL, d.max().item()


@pytest.mark.parametrize("size", DET_SIZES)
@pytest.mark.parametrize("branch", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.float32])
def test_detection_branch_matches_comparand(dev, size, branch, mask_dtype):
    h, w = size
    img, m = _u8(h, w, h * 7 + w), _mask(h, w, h + w)
    m = m.to(mask_dtype)
    p = _draw(branch, size) if branch >= 0 else A.AugParams(-1, size, size)
    out = A.detection_batch([img], [m], dev, augment=True, params=[p])
    wi, wm = R.det_sample(_pf(img), m.float(), p)
    assert out["image"].shape == (1, 1, 800, 600) and out["text_mask"].dtype == torch.float32
    _check(out["image"][0], wi, nearest=branch == 1)
    _check(out["text_mask"][0], wm, nearest=branch == 1)
    if branch == 0 or branch == 2:  # bf16 image output
        o16 = A.detection_batch([img], [m], dev, augment=True, params=[p], dtype=torch.bfloat16)
        assert o16["image"].dtype == torch.bfloat16
        d = (o16["image"][0].float().cpu() - wi).abs()
        assert (d <= wi.abs() * 2.0**-7 + TOL).all()
        assert torch.equal(o16["text_mask"], out["text_mask"])


@pytest.mark.parametrize("size", DET_SIZES)
def test_detection_no_augment_is_plain_resize(dev, size):
    h, w = size
    img, m = _u8(h, w, 3), _mask(h, w, 3).float()
    out = A.detection_batch([img], [m], dev, augment=False)
    x = torch.nn.functional.interpolate(torch.stack([_pf(img), m]), size=(800, 600), mode="bilinear", align_corners=False, antialias=False)
    _check(out["image"][0], x[0])
    _check(out["text_mask"][0], x[1])


def test_detection_mixed_batch_reproducible(dev):
    sizes = [DET_SIZES[k % len(DET_SIZES)] for k in range(32)]
    imgs = [_u8(h, w, k) for k, (h, w) in enumerate(sizes)]
    masks = [_mask(h, w, k) for k, (h, w) in enumerate(sizes)]
    params = A.sample_detection_params(sizes, torch.Generator().manual_seed(11), random.Random(11))
    assert {p.branch for p in params} == {-1, 0, 1, 2, 3}
    a = A.detection_batch(imgs, masks, dev, augment=True, params=params)
    b = A.detection_batch([t.to(dev) for t in imgs], [t.to(dev) for t in masks], dev, augment=True, params=params)  # device inputs
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["text_mask"], b["text_mask"])
    for k, p in enumerate(params):
        wi, wm = R.det_sample(_pf(imgs[k]), masks[k].float(), p)
        _check(a["image"][k], wi, nearest=p.branch == 1)
        _check(a["text_mask"][k], wm, nearest=p.branch == 1)
    # seeded sampling inside the call gives the same draw, and the same bits
    c = A.detection_batch(imgs, masks, dev, augment=True, generator=torch.Generator().manual_seed(11), rng=random.Random(11))
    assert torch.equal(a["image"], c["image"]) and torch.equal(a["text_mask"], c["text_mask"])


def _line_samples(with_mask, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, (h, w) in enumerate(LINE_SIZES):
        s = {"image": _u8(h, w, seed + k), "text_seq": torch.randint(1, 97, (1 + (k * 5) % 17,), generator=g, dtype=torch.int32)}
        if with_mask:
            s["mask"] = _mask(h, w, seed + k)
        out.append(s)
    return out


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("branch", [-1, 0, 1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lines_branch_matches_comparand(dev, with_mask, branch, dtype):
    from ocrs_models_amd import input_pipeline as ip

    samples = _line_samples(with_mask, seed=branch + 5)
    params = [_draw(branch, tuple(s["image"].shape[-2:]), line=True) if branch >= 0 else A.AugParams(-1, tuple(s["image"].shape[-2:]),
              tuple(s["image"].shape[-2:])) for s in samples]
    got = A.collate_lines(samples, dev, augment=True, params=params, dtype=dtype)
    ref = [{"image": R.line_sample(_pf(s["image"]), p, s.get("mask")), "text_seq": s["text_seq"]} for s, p in zip(samples, params)]
    want = ip.collate_samples(ref, dev)
    for k in ("text_seq", "text_len", "image_width"):
        assert torch.equal(got[k], want[k]), k
    assert got["image"].shape == want["image"].shape and got["image"].dtype == dtype
    if dtype == torch.float32:
        _check(got["image"], want["image"].cpu())
    else:
        w32 = want["image"].cpu()
        assert ((got["image"].float().cpu() - w32).abs() <= w32.abs() * 2.0**-7 + TOL).all()


def test_lines_drop_rule_and_no_augment_equals_collate_samples(dev):
    from ocrs_models_amd import input_pipeline as ip

    samples = _line_samples(False, seed=1)
    samples[4]["text_seq"] = torch.arange(1, 40, dtype=torch.int32)  # 90x40 -> width 28: 7 steps < 39 labels, dropped
    got = A.collate_lines(samples, dev, augment=False)
    resized = [{"image": ip.resize_line(ip.transform_image(s["image"].to(dev))).cpu(), "text_seq": s["text_seq"]} for s in samples]
    want = ip.collate_samples(resized, dev)
    assert got["image"].shape[0] == len(samples) - 1
    for k in ("image", "text_seq", "text_len", "image_width"):
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    # device inputs, fp32 crops: the same bits
    fs = [{"image": ip.transform_image(s["image"].to(dev)), "text_seq": s["text_seq"]} for s in samples]
    assert torch.equal(A.collate_lines(fs, dev, augment=False)["image"], got["image"])


def test_lines_mixed_batch_reproducible(dev):
    samples = _line_samples(True, seed=9) * 6
    a = A.collate_lines(samples, dev, augment=True, generator=torch.Generator().manual_seed(3), rng=random.Random(3))
    b = A.collate_lines(samples, dev, augment=True, generator=torch.Generator().manual_seed(3), rng=random.Random(3))
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_train_steps_on_augmented_batches(dev):
    import ocrs_models_amd as oa
    from ocrs_models_amd import train_detection, train_rec

    torch.manual_seed(0)
    sizes = [(1600, 1200), (480, 640)]
    batch = A.detection_batch([_u8(h, w, 1) for h, w in sizes], [_mask(h, w, 1) for h, w in sizes], dev, augment=True,
                              generator=torch.Generator().manual_seed(2), rng=random.Random(2))
    m = oa.DetectionModel().to(dev)
    m.train()
    loss = train_detection.train_step(m, train_detection.make_optimizer(m), batch, dev)
    assert torch.isfinite(loss).item()

    rb = A.collate_lines(_line_samples(True, seed=4), dev, augment=True, generator=torch.Generator().manual_seed(4), rng=random.Random(4))
    rm = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
    rm.train()
    rloss, gn = train_rec.train_step(rm, train_rec.make_optimizer(rm), rb, dev)
    assert torch.isfinite(rloss).item() and torch.isfinite(gn).item()


@pytest.mark.parametrize("size", [(1600, 1200), (2001, 37)])
def test_detection_jitter_contrast_first(dev, size):
    """Contrast before brightness with b > 1: the jittered mask reaches the upper end of the [0, 1] clamp."""
    h, w = size
    img, m = _u8(h, w, 21), _mask(h, w, 21)
    p = A.AugParams(0, size, size, order=(3, 1, 0, 2), brightness=1.09, contrast=0.93)
    out = A.detection_batch([img], [m], dev, augment=True, params=[p])
    wi, wm = R.det_sample(_pf(img), m.float(), p)
    assert R.color_jitter(m.float().unsqueeze(0), p.order, p.brightness, p.contrast).max().item() == 1.0
    _check(out["image"][0], wi)
    _check(out["text_mask"][0], wm)


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("branch", [-1, 0, 1, 2])
def test_lines_clamps_on_out_of_range_fp32_crops(dev, with_mask, branch):
    """fp32 crops in [-1, 1.3]: the recognition clamp(-0.5, 0.5) and ColorJitter's [0, 1] clamp (contrast first, b > 1) both bite."""
    from ocrs_models_amd import input_pipeline as ip

    samples = _line_samples(with_mask, seed=30 + branch)
    g = torch.Generator().manual_seed(31)
    for s in samples:
        s["image"] = torch.rand(s["image"].shape, generator=g) * 2.3 - 1.0
    params = []
    for s in samples:
        size = tuple(s["image"].shape[-2:])
        if branch == 0:
            params.append(A.AugParams(0, size, size, order=(1, 2, 0, 3), brightness=1.08, contrast=1.06))
        elif branch > 0:
            params.append(_draw(branch, size, line=True))
        else:
            params.append(A.AugParams(-1, size, size))
    got = A.collate_lines(samples, dev, augment=True, params=params)
    ref = [{"image": R.line_sample(s["image"], p, s.get("mask")), "text_seq": s["text_seq"]} for s, p in zip(samples, params)]
    want = ip.collate_samples(ref, dev)
    for k in ("text_seq", "text_len", "image_width"):
        assert torch.equal(got[k], want[k]), k
    _check(got["image"], want["image"].cpu())
    unclamped = A.collate_lines(samples, dev, augment=False, params=params)  # no clamp: differs wherever the clamp bit
    assert (unclamped["image"] - got["image"]).abs().max().item() > 0.1


def test_mixed_residency_inputs(dev):
    """Each input list may be on the host or the GPU on its own: device crops / images with host masks give the same bits."""
    samples = _line_samples(True, seed=40)
    params = A.sample_line_params([tuple(s["image"].shape[-2:]) for s in samples], torch.Generator().manual_seed(41), random.Random(41))
    host = A.collate_lines(samples, dev, augment=True, params=params)
    mixed = A.collate_lines([{**s, "image": s["image"].to(dev)} for s in samples], dev, augment=True, params=params)
    assert torch.equal(host["image"], mixed["image"])
    mixed2 = A.collate_lines([{**s, "mask": s["mask"].to(dev)} for s in samples], dev, augment=True, params=params)
    assert torch.equal(host["image"], mixed2["image"])
    unmasked = A.collate_lines([{k: v for k, v in s.items() if k != "mask"} for s in samples], dev, augment=True, params=params)
    assert not torch.equal(host["image"], unmasked["image"])  # the masks are applied

    sizes = [(640, 480), (599, 601)]
    imgs, masks = [_u8(h, w, 42) for h, w in sizes], [_mask(h, w, 42) for h, w in sizes]
    dp = A.sample_detection_params(sizes, torch.Generator().manual_seed(43), random.Random(43))
    a = A.detection_batch(imgs, masks, dev, augment=True, params=dp)
    b = A.detection_batch([t.to(dev) for t in imgs], masks, dev, augment=True, params=dp)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["text_mask"], b["text_mask"])

    with pytest.raises(RuntimeError, match="all on the host or all on the GPU"):
        A.detection_batch(imgs, [masks[0].to(dev), masks[1]], dev, augment=True, params=dp)

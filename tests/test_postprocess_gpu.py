"""The device validation metrics (csrc/postprocess.hip via ocrs_models_amd/postprocess.py) against the host restatement they mirror:
labelling vs scipy.ndimage.label (8-connectivity, raster-order numbering), quads vs extract_cc_quads, the four per-image metrics vs
mask_metrics / box_match_metrics (exactly equal), train_detection.test(metrics_fn="device") vs the default path, and no host sync."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

from ocrs_models_amd import postprocess as pp

pytestmark = pytest.mark.gpu

KEYS = ("precision", "recall", "merged_frac", "split_frac")


def word_mask(H, W, n, seed):
    """~n rotated word boxes (10-80 px long, 6-20 px high, +-0.3 rad) placed uniformly at random"""
    r = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        cx, cy, w, h, t = r.uniform(0, W), r.uniform(0, H), r.uniform(10, 80), r.uniform(6, 20), r.uniform(-0.3, 0.3)
        R = int(math.ceil(math.hypot(w, h) / 2)) + 1
        x0, x1, y0, y1 = max(0, int(cx) - R), min(W, int(cx) + R + 1), max(0, int(cy) - R), min(H, int(cy) + R + 1)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1]
        u = (xx - cx) * math.cos(t) + (yy - cy) * math.sin(t)
        v = -(xx - cx) * math.sin(t) + (yy - cy) * math.cos(t)
        m[y0:y1, x0:x1] |= ((np.abs(u) <= w / 2) & (np.abs(v) <= h / 2)).astype(np.uint8)
    return m


def perturb(m, seed):
    """a prediction-like mask: shifted, some words dilated into their neighbours (merges), some cut (splits), some dropped"""
    r = np.random.RandomState(seed)
    p = np.roll(m, (r.randint(-2, 3), r.randint(-2, 3)), axis=(0, 1)).copy()
    H, W = m.shape
    for _ in range(20):
        y, x = r.randint(0, H - 40), r.randint(0, W - 100)
        p[y:y + 30, x:x + 90] = ndimage.binary_dilation(p[y:y + 30, x:x + 90], iterations=3)
    for _ in range(15):                               # bands that swallow several words whole
        y, x = r.randint(0, H - 40), r.randint(0, W - 260)
        p[y:y + 40, x:x + 260] = 1
    for _ in range(20):
        x = r.randint(0, W)
        p[:, x:x + 2] = 0
    for _ in range(10):
        y, x = r.randint(0, H - 30), r.randint(0, W - 30)
        p[y:y + 30, x:x + 30] = 0
    return p


def speckle(H, W, density, seed):
    return (np.random.RandomState(seed).uniform(0, 1, (H, W)) < density).astype(np.uint8)


def serpentine(H, W):
    m = np.zeros((H, W), np.uint8)
    m[::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def spiral(n):
    m = np.zeros((n, n), np.uint8)
    y0, x0, y1, x1 = 0, 0, n - 1, n - 1
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        if y1 > y0 + 1:
            m[y1, x0:x1 + 1] = 1
        if x1 > x0 + 2 and y1 > y0 + 2:
            m[y0 + 2:y1 + 1, x0] = 1
            m[y0 + 2, x0:x0 + 2] = 1
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return m


def diagonals(H, W):
    m = np.zeros((H, W), np.uint8)
    for k in range(-H, W, 7):
        for y in range(H):
            if 0 <= y + k < W:
                m[y, y + k] = 1
    m[H // 2, :] = 0                                  # cut: each chain becomes two components
    return m


def checkerboard(H, W):
    return ((np.add.outer(np.arange(H), np.arange(W)) % 2) == 0).astype(np.uint8)


def lattice(H, W):
    m = np.zeros((H, W), np.uint8)
    m[::2, ::2] = 1
    return m


def labels_of(masks_np):
    t = torch.from_numpy(np.stack(masks_np)).cuda()
    lab, n = pp.label_components_device(t)
    return lab.cpu().numpy(), n.cpu().numpy()


LABEL_CASES = {
    **{f"speckle{d}": (lambda d=d: speckle(200, 300, d, int(d * 10))) for d in (0.1, 0.3, 0.45, 0.6, 0.7)},
    "serpentine": lambda: serpentine(257, 301),
    "spiral": lambda: spiral(301),
    "diagonals": lambda: diagonals(150, 211),
    "checkerboard": lambda: checkerboard(129, 190),
    "lattice": lambda: lattice(131, 97),
    "zeros": lambda: np.zeros((70, 80), np.uint8),
    "ones": lambda: np.ones((70, 80), np.uint8),
    "1x1": lambda: np.ones((1, 1), np.uint8),
    "1xW": lambda: speckle(1, 1000, 0.5, 3),
    "Hx1": lambda: speckle(1000, 1, 0.5, 4),
    "63x97": lambda: speckle(63, 97, 0.4, 5),
    "1024sq": lambda: speckle(1024, 1024, 0.45, 6),
}


@pytest.mark.parametrize("case", list(LABEL_CASES))
def test_labels_match_scipy(dev, case):
    m = LABEL_CASES[case]()
    want, n = ndimage.label(m, structure=np.ones((3, 3), dtype=bool))
    got, cnt = labels_of([m])
    assert int(cnt[0]) == n
    assert np.array_equal(got[0], want)  # same partition AND scipy's raster-order numbering
    if case == "lattice":
        assert n == math.ceil(131 / 2) * math.ceil(97 / 2)
    if case == "checkerboard":
        assert n == 1


def test_labels_batch_of_different_images(dev):
    ims = [speckle(96, 130, 0.5, 11), spiral(96)[:, :1].repeat(130, 1) * 0, lattice(96, 130), serpentine(96, 130), np.ones((96, 130), np.uint8)]
    got, cnt = labels_of(ims)
    for i, m in enumerate(ims):
        want, n = ndimage.label(m, structure=np.ones((3, 3), dtype=bool))
        assert int(cnt[i]) == n and np.array_equal(got[i], want), i
    # fp32 input binarised with > threshold, as binarize_mask does
    f = torch.from_numpy(np.random.RandomState(1).uniform(0, 1, (2, 1, 64, 64)).astype(np.float32)).cuda()
    lab, n = pp.label_components_device(f, threshold=0.7)
    for i in range(2):
        want, k = ndimage.label(f[i, 0].cpu().numpy() > 0.7, structure=np.ones((3, 3), dtype=bool))
        assert int(n[i]) == k and np.array_equal(lab[i].cpu().numpy(), want)


def assert_quads_equal(got, want, tol=1e-4):
    assert got.shape == want.shape, (got.shape, want.shape)
    for i in range(len(want)):
        best = min(float((torch.roll(got[i], s, 0) - want[i]).abs().max()) for s in range(4))
        assert best <= tol, (i, got[i], want[i])


@pytest.mark.parametrize("seed", [0, 1])
def test_quads_match_host_on_word_masks(dev, seed):
    m = word_mask(512, 768, 120, seed)
    want = pp.extract_cc_quads(torch.from_numpy(m))
    got = pp.extract_cc_quads_device(torch.from_numpy(m).cuda()).cpu()
    assert len(want) > 50
    assert_quads_equal(got, want)


def test_quads_match_host_on_degenerate_components(dev):
    m = np.zeros((64, 96), np.uint8)
    m[3, 5] = 1                        # one pixel
    m[10, 10:30] = 1                   # horizontal line
    m[20:40, 50] = 1                   # vertical line
    for i in range(12):
        m[30 + i, 5 + i] = 1           # diagonal
        m[50 - i, 70 + i] = 1          # anti-diagonal
    m[60, 90:92] = 1                   # two pixels
    m[45:47, 30:32] = 1                # 2x2 block
    m[55, 40] = m[56, 41] = m[55, 42] = 1  # a "v"
    want = pp.extract_cc_quads(torch.from_numpy(m))
    for mask in (torch.from_numpy(m).cuda(), torch.from_numpy(m).cuda().bool()[None], torch.from_numpy(m).cuda().float()):
        got = pp.extract_cc_quads_device(mask).cpu()
        assert_quads_equal(got, want, tol=1e-5)
    assert pp.extract_cc_quads_device(torch.zeros(8, 8, device="cuda")).shape == (0, 4, 2)


def device_metrics(preds, tgts):
    p = torch.from_numpy(np.stack(preds)[:, None]).cuda()
    t = torch.from_numpy(np.stack(tgts)[:, None]).cuda()
    return pp.batch_mask_metrics(p, t).cpu()


def host_metrics(preds, tgts):
    return [pp.mask_metrics(torch.from_numpy(a), torch.from_numpy(b)) for a, b in zip(preds, tgts)]


def assert_metrics_equal(got, want):
    assert got.dtype == torch.float64 and got.shape == (len(want), 4)
    for i, w in enumerate(want):
        assert tuple(got[i].tolist()) == tuple(w[k] for k in KEYS), (i, got[i].tolist(), w)


def test_metrics_match_host_on_1024_word_batch(dev):
    tgts = [word_mask(1024, 1024, 240, 100 + i) for i in range(4)]
    preds = [perturb(t, 200 + i) for i, t in enumerate(tgts)]
    want = host_metrics(preds, tgts)
    assert all(0 < w["precision"] < 1 and w["merged_frac"] > 0 and w["split_frac"] > 0 for w in want), want
    assert_metrics_equal(device_metrics(preds, tgts), want)
    # fp32 masks (the test loop's input) binarised on the device give the same numbers
    p = torch.from_numpy(np.stack(preds)[:, None].astype(np.float32)).cuda() * 0.9
    t = torch.from_numpy(np.stack(tgts)[:, None].astype(np.float32)).cuda()
    assert_metrics_equal(pp.batch_mask_metrics(p, t).cpu(), want)


@pytest.mark.parametrize("density", [0.02, 0.05, 0.1])
def test_metrics_match_host_on_speckle(dev, density):
    tgts = [speckle(256, 320, density, 7), speckle(300, 300, density * 1.5, 8)]
    tgts[1] = tgts[1][:256, :300]
    tgts = [t[:256, :300] for t in tgts]
    preds = [np.maximum(t, speckle(256, 300, density, 9 + i)) for i, t in enumerate(tgts)]
    want = host_metrics(preds, tgts)
    assert_metrics_equal(device_metrics(preds, tgts), want)


def test_metrics_with_thousands_of_components(dev):
    t = ndimage.binary_dilation(lattice(400, 400) * (np.random.RandomState(3).uniform(0, 1, (400, 400)) < 0.08)).astype(np.uint8)
    p = np.roll(t, 1, axis=1) | (speckle(400, 400, 0.01, 4))
    n = ndimage.label(t, structure=np.ones((3, 3), dtype=bool))[1]
    assert n > 2000
    assert_metrics_equal(device_metrics([p], [t]), host_metrics([p], [t]))


def test_metrics_empty_sets(dev):
    e = np.zeros((64, 96), np.uint8)
    w = word_mask(64, 96, 4, 1)
    assert w.any()
    preds, tgts = [e, w, e], [w, e, e]
    want = host_metrics(preds, tgts)
    assert want[2] == {"precision": 1.0, "recall": 1.0, "merged_frac": 0.0, "split_frac": 0.0}
    assert_metrics_equal(device_metrics(preds, tgts), want)


def _rect_mask(H, W, boxes):
    m = np.zeros((H, W), np.uint8)
    for x0, y0, x1, y1 in boxes:
        m[y0:y1 + 1, x0:x1 + 1] = 1
    return m


def test_known_answer_scenes(dev):
    box = lambda x0, y0, x1, y1: [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]  # noqa: E731
    T = torch.tensor([box(0, 0, 10, 4), box(20, 0, 30, 4), box(0, 10, 10, 14), box(20, 10, 30, 14)], dtype=torch.float32)
    P = torch.tensor([box(0, 0, 30, 4), box(0, 10, 8, 14), box(20, 10, 25, 14), box(25, 10, 30, 14)], dtype=torch.float32)
    e = torch.zeros(0, 4, 2)
    for a, b in ((T, T), (e, T), (T, e), (P, T), (e, e),
                 (torch.tensor([box(0, 0, 10, 2)], dtype=torch.float32), torch.tensor([box(0, 0, 10, 4)], dtype=torch.float32))):
        assert pp.box_match_metrics_device(a.cuda(), b.cuda()) == pp.box_match_metrics(a, b)
    m = pp.box_match_metrics_device(P.cuda(), T.cuda())
    assert m["precision"] == 1 / 4 and m["recall"] == 1 / 4 and m["merged_frac"] == 2 / 4 and m["split_frac"] == 1 / 4
    # rotated quads: the clipper on general convex pairs
    r = np.random.RandomState(0)
    def rnd(n):
        out = []
        for _ in range(n):
            cx, cy, w, h, t = r.uniform(0, 20), r.uniform(0, 20), r.uniform(1, 8), r.uniform(1, 8), r.uniform(0, math.pi)
            R = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])
            out.append((np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) / 2) @ R.T + [cx, cy])
        return torch.tensor(np.array(out), dtype=torch.float32)
    for _ in range(5):
        a, b = rnd(30), rnd(25)
        assert pp.box_match_metrics_device(a.cuda(), b.cuda()) == pp.box_match_metrics(a, b)
    # the end-to-end scene of tests/test_postprocess.py
    tgt = _rect_mask(64, 96, [(4, 4, 30, 10), (40, 4, 80, 10), (4, 30, 50, 38)])
    pred = _rect_mask(64, 96, [(4, 4, 30, 10), (40, 5, 80, 10), (60, 50, 70, 55)])
    got = device_metrics([pred], [tgt])
    assert got[0].tolist() == [2 / 3, 2 / 3, 0.0, 0.0]


def test_batch_mask_metrics_makes_no_host_sync(dev):
    t = torch.from_numpy(np.stack([word_mask(256, 256, 30, i) for i in range(2)])[:, None].astype(np.float32)).cuda()
    p = torch.roll(t, 1, -1)
    want = pp.batch_mask_metrics(p, t)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = pp.batch_mask_metrics(p, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, want)


def _load_model(seed):
    import ocrs_models_amd as oa
    from oracle.params import detection_specs, make_state, state_dict_from

    specs = detection_specs()
    P, Bf = make_state(specs, seed)
    m = oa.DetectionModel()
    m.load_state_dict(state_dict_from(P, Bf, specs))
    return m


def _assert_same_test_result(dev, m, batches):
    from ocrs_models_amd import train_detection as td

    loss_h, met_h = td.test(dev, batches, m)
    loss_d, met_d = td.test(dev, batches, m, metrics_fn="device")
    assert loss_d == loss_h
    assert set(met_d) == set(met_h) == set(KEYS)
    for k in KEYS:
        assert abs(met_d[k] - met_h[k]) <= 1e-12, (k, met_d[k], met_h[k])
    return met_h


def test_validation_loop_device_metrics_match_default(dev):
    m = _load_model(21).to(dev)
    g = torch.Generator().manual_seed(4)
    batches = []
    for b in (2, 1):
        batches.append({"image": torch.rand(b, 1, 64, 96, generator=g) - 0.5, "text_mask": (torch.rand(b, 1, 64, 96, generator=g) > 0.8).float(),
                        "path": ["x"] * b})
    _assert_same_test_result(dev, m, batches)
    from ocrs_models_amd import train_detection as td
    assert td.test(dev, [], m, metrics_fn="device") == td.test(dev, [], m)


def test_validation_loop_device_metrics_1024(dev):
    m = _load_model(5).to(dev)
    tg = np.stack([word_mask(1024, 1024, 200, 40 + i) for i in range(2)])[:, None].astype(np.float32)
    img = torch.from_numpy(tg - 0.5) + 0.05 * torch.randn(tg.shape, generator=torch.Generator().manual_seed(2))
    batch = {"image": img, "text_mask": torch.from_numpy(tg), "path": ["x"] * 2}
    _assert_same_test_result(dev, m, [batch])

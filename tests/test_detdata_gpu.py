"""The detection datasets on the GPU (ocrs_models_amd/datasets/pages.py, csrc/page_data.hip): the shrink kernel against its host restatement, page
masks against PIL fed the restatement's float vertices (tests/detdata_ref.py), batches and items against the existing ``detection_batch``
fed host pages and reference masks, train steps from the loader, and the training command line end to end on a tiny tree.  Everything
short of the model runs at ``mask_size=(64, 48)``; the train steps run at (64, 64), the smallest size ``DetectionModel`` accepts.

Masks, pixels, items and batches are compared with ``torch.equal``: the masks are integer rasterisation of vertices both sides truncate from
the same doubles, and what follows them is the same kernel sequence on the same bytes, so there is no tolerance to choose.  The shrunk
coordinates are held to 1e-9 (bit equality is expected and the difference is printed): device and host run the same IEEE operations in
the same order, and the inputs keep every coordinate a whole number or 1e-6 away from one, so the truncated integers must be equal."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import detdata_ref as ref

pytestmark = pytest.mark.gpu
MASK = (64, 48)
# DetectionModel pools 2x2 six times and refuses a side under 64 (as the reference's U-Net would fail on it), so the two tests that run the
# model in this process cannot use MASK; they use the smallest size the model takes.  Every test that stops short of the model uses MASK.
MODEL_MASK = (64, 64)


def _shrink_on_device(dev, polys, dist):
    from ocrs_models_amd._lib import lib, ptr

    counts = np.array([len(p) for p in polys], dtype=np.int32)
    offs = np.cumsum(counts, dtype=np.int64) - counts
    verts = np.array([v for p in polys for v in p], dtype=np.int32).reshape(-1, 2)
    V = len(verts)
    d_verts, d_offs, d_counts = (torch.from_numpy(a).to(dev) for a in (verts, offs, counts))
    ws = torch.empty(3 * V, dtype=torch.int32, device=dev)
    xy = torch.full((2 * V + 8, 2), 7.5, dtype=torch.float64, device=dev)
    iv = torch.full((2 * V + 8, 2), 77, dtype=torch.int32, device=dev)
    cnt = torch.empty(len(polys), dtype=torch.int32, device=dev)
    rows = torch.empty(len(polys), 2, dtype=torch.int32, device=dev)
    lib().shrink_polygons(ptr(d_verts), ptr(d_offs), ptr(d_counts), len(polys), dist, ptr(ws), ptr(xy), ptr(iv), ptr(cnt), ptr(rows))
    xy, iv = xy.cpu().numpy(), iv.cpu().numpy()
    assert (xy[2 * V:] == 7.5).all() and (iv[2 * V:] == 77).all()  # nothing written past the last polygon
    return xy, iv, cnt.cpu().tolist(), rows.cpu().tolist(), offs.tolist()


def test_shrink_kernel_equals_the_host_rule(dev):
    cases = ref.shrink_cases()
    want = [ref.shrink_polygon(p, 3.0) for _, p in cases]
    for (name, _), w in zip(cases, want):  # the condition on the inputs, on the reference alone
        assert all(c == round(c) or abs(c - round(c)) >= 1e-6 for pt in w for c in pt), name
    assert sum(1 for w in want if not w) >= 8 and sum(1 for (_, p), w in zip(cases, want) if len(w) > len(ref.dedupe(p))) >= 2
    xy, iv, cnt, rows, offs = _shrink_on_device(dev, [p for _, p in cases], 3.0)
    worst = 0.0
    for (name, _), w, n, (y0, y1), o in zip(cases, want, cnt, rows, offs):
        assert n == len(w), (name, n, len(w))  # the skipped flag and the bevels
        if not w:
            assert (y0, y1) == (0, -1), name
            continue
        got = xy[2 * o:2 * o + n]
        worst = max(worst, float(np.abs(got - np.array(w)).max()))
        assert np.array_equal(iv[2 * o:2 * o + n], np.array([[int(x), int(y)] for x, y in w])), name
        assert (y0, y1) == (min(int(y) for _, y in w), max(int(y) for _, y in w)), name
    print("shrink: max |device - host| =", worst)
    assert worst <= 1e-9
    # dist 0: the vertices as they are
    xy0, iv0, cnt0, rows0, offs0 = _shrink_on_device(dev, [p for _, p in cases[:30]], 0.0)
    for (name, p), n, o in zip(cases[:30], cnt0, offs0):
        assert n == len(p) and iv0[2 * o:2 * o + n].tolist() == [list(v) for v in p], name


@pytest.fixture(scope="module")
def mask_store(dev):
    pages = ref.mask_pages()
    px = [ref.page_pixels(w, h, 11 + k) for k, (_, (w, h), _) in enumerate(pages)]
    want = [ref.page_mask(w, h, polys, 3.0) for _, (w, h), polys in pages]
    return pages, px, want


def test_page_masks_equal_pil(dev, mask_store):
    from ocrs_models_amd.datasets import HierText

    pages, px, want = mask_store
    ds = HierText.from_pages(px, [polys for _, _, polys in pages], device=dev, mask_size=MASK)
    assert ds.skipped == 3 and [n for n, _, _ in pages][5] == "all-skipped" and want[0].sum() == 0 and want[5].sum() == 0
    # the "dense" page: one band's slice of the sorted records is longer than two 64-lane passes, with the 24-vertex ring in the second
    assert pages[9][0] == "dense" and len(pages[9][2][76]) == 24
    records, bands = ds._tensors()[4].cpu(), ds._tensors()[6].cpu()
    lo, hi = bands[int((bands[:, 1] - bands[:, 0]).argmax())].tolist()
    assert hi - lo > 128 and 64 <= records[lo:hi, 1].tolist().index(24) < 128
    order = [6, 0, 3, 8, 1, 9, 5, 2, 7, 4, 6]  # one batch, pages of different sizes, one of them twice
    raw = ds.raw(order)
    for i, (page, mask) in zip(order, raw):
        name = pages[i][0]
        assert page.dtype == torch.uint8 and tuple(page.shape) == (1, *px[i].shape)
        assert torch.equal(page.cpu()[0], torch.from_numpy(px[i])), name  # the gathered pixels
        diff = int((mask.cpu()[0].numpy() != want[i]).sum())
        assert diff == 0, (name, diff)
        assert set(np.unique(mask.cpu().numpy()).tolist()) <= {0, 1}
    one = ds.raw([4])[0][1]  # and a batch of one
    assert np.array_equal(one.cpu()[0].numpy(), want[4])


def test_unshrunk_masks_equal_pil(dev, mask_store):
    from ocrs_models_amd.datasets import HierText
    from tests.hiertext_ref import pil_mask

    pages, px, _ = mask_store
    ds = HierText.from_pages(px, [polys for _, _, polys in pages], device=dev, mask_size=MASK, shrink_dist=0.0)
    for (name, (w, h), polys), (_, mask) in zip(pages, ds.raw(range(len(pages)))):
        want = np.zeros((h, w), np.uint8)
        for p in polys:
            want |= pil_mask(w, h, p)
        assert np.array_equal(mask.cpu()[0].numpy(), want), name
        assert np.array_equal(want, ref.page_mask(w, h, polys, 0.0)), name


def _params(kind: int, size):
    from ocrs_models_amd.augment import AugParams, sample_detection_params

    if kind < 0:
        return AugParams(-1, size, size)
    g = torch.Generator().manual_seed(100 + kind)
    import random

    rng = random.Random(kind)
    for _ in range(400):  # one fixed draw of the wanted kind
        p = sample_detection_params([size], g, rng)[0]
        if p.branch == kind:
            return p
    raise AssertionError(kind)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_equals_detection_batch_on_host_inputs(dev, mask_store, dtype):
    from ocrs_models_amd.augment import detection_batch
    from ocrs_models_amd.datasets import HierText

    pages, px, want = mask_store
    ds = HierText.from_pages(px, [polys for _, _, polys in pages], paths=[n for n, _, _ in pages], device=dev, mask_size=MASK, augment=True)
    idx = [6, 2, 8, 3, 0]
    host_img = [torch.from_numpy(px[i])[None] for i in idx]
    host_msk = [torch.from_numpy(want[i])[None] for i in idx]
    for kinds in ([-1] * 5, [0, 1, 2, 3, -1], [3, 2, 1, 0, 0]):
        params = [_params(k, ds.sizes[i]) for k, i in zip(kinds, idx)]
        got = ds.batch(idx, params, dtype=dtype)
        host = detection_batch(host_img, host_msk, dev, augment=True, dtype=dtype, params=params, mask_size=MASK)
        assert got["path"] == [pages[i][0] for i in idx]
        assert got["image"].dtype == dtype and tuple(got["image"].shape) == (5, 1, *MASK) and got["text_mask"].dtype == torch.float32
        assert torch.equal(got["image"], host["image"]) and torch.equal(got["text_mask"], host["text_mask"]), kinds
    import random  # the loader's own draw is draw_params': the same streams give the same batch

    random.seed(4)
    torch.manual_seed(3)
    state = random.getstate()
    a = ds.batch(idx, dtype=dtype)
    random.setstate(state)
    torch.manual_seed(3)
    b = ds.batch(idx, ds.draw_params(idx), dtype=dtype)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["text_mask"], b["text_mask"])


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    h = str(tmp_path_factory.mktemp("hiertext_det"))
    words = ref.write_hiertext_tree(h, "train")
    ref.write_hiertext_tree(h, "validation", seed=9)
    d = str(tmp_path_factory.mktemp("ddi"))
    quads = ref.write_ddi_tree(d)
    return h, words, d, quads


def test_trees_give_the_references_items(dev, trees):
    from ocrs_models_amd.augment import detection_batch
    from ocrs_models_amd.datasets import DDI100, DevicePageLoader, HierText

    h, words, d, quads = trees
    for ds, files, polys in ((HierText(h, device=dev, mask_size=MASK), [f"{h}/train/{pid}.jpg" for pid, _ in words], [w for _, w in words]),
                             (DDI100(d, device=dev, mask_size=MASK), [f"{d}/gen_imgs/{n}" for n, _ in quads[:18]], [q for _, q in quads[:18]])):
        assert len(ds) == len(files)
        pages = [ref.read_gray(f) for f in files]
        masks = [ref.page_mask(p.shape[1], p.shape[0], q, 3.0) for p, q in zip(pages, polys)]
        host = detection_batch([torch.from_numpy(p)[None] for p in pages], [torch.from_numpy(m)[None] for m in masks], dev, augment=False, mask_size=MASK)
        for i in range(len(ds)):
            item = ds[i]
            assert sorted(item) == ["image", "path", "text_mask"] and item["path"] == files[i]
            assert item["image"].is_cuda and item["image"].dtype == torch.float32 and tuple(item["image"].shape) == (1, *MASK)
            assert tuple(item["text_mask"].shape) == (1, *MASK)
            assert torch.equal(item["image"], host["image"][i]) and torch.equal(item["text_mask"], host["text_mask"][i]), (type(ds).__name__, i)
        assert float(host["text_mask"].sum()) > 0
        batches = list(DevicePageLoader(ds, batch_size=4))
        assert len(batches) == (len(ds) + 3) // 4 and torch.equal(torch.cat([b["text_mask"] for b in batches]), host["text_mask"])
        assert [p for b in batches for p in b["path"]] == files


def test_train_steps_from_the_loader(dev, trees):
    import ocrs_models_amd as oa
    from ocrs_models_amd.augment import detection_batch
    from ocrs_models_amd.datasets import DevicePageLoader, HierText
    from ocrs_models_amd.train_detection import make_optimizer, train_step

    h, words, _, _ = trees
    ds = HierText(h, device=dev, mask_size=MODEL_MASK)
    files = [f"{h}/train/{pid}.jpg" for pid, _ in words]
    pages = [ref.read_gray(f) for f in files]
    masks = [ref.page_mask(p.shape[1], p.shape[0], q, 3.0) for p, (_, q) in zip(pages, words)]

    def run(batches):
        torch.manual_seed(11)
        model = oa.DetectionModel().to(dev).train()
        opt = make_optimizer(model)
        return [float(train_step(model, opt, b, dev)) for b in batches]

    loader = DevicePageLoader(ds, batch_size=2)
    got = run([b for _, b in zip(range(2), loader)])
    host = [detection_batch([torch.from_numpy(pages[i])[None] for i in idx], [torch.from_numpy(masks[i])[None] for i in idx], dev, augment=False,
                            mask_size=MODEL_MASK) for idx in ([0, 1], [2, 3])]
    want = run(host)
    print("train steps from the loader:", got, "host-fed:", want)
    assert all(np.isfinite(got)) and got == want


def test_debug_images_leave_the_training_loop_as_it_is(dev, trees, tmp_path):
    """``--debug-images`` wraps the loader (``_DebugImages``): the epoch's loss is the plain loop's, and the reference's files appear."""
    import ocrs_models_amd as oa
    from ocrs_models_amd.datasets import DevicePageLoader, HierText
    from ocrs_models_amd.losses import balanced_cross_entropy_loss
    from ocrs_models_amd.train_detection import _DebugImages, make_optimizer, train

    ds = HierText(trees[0], max_images=4, device=dev, mask_size=MODEL_MASK)

    def run(wrap):
        torch.manual_seed(11)
        model = oa.DetectionModel().to(dev)
        return train(0, dev, wrap(DevicePageLoader(ds, batch_size=2), model), model, balanced_cross_entropy_loss, make_optimizer(model))

    plain = run(lambda loader, model: loader)
    base = str(tmp_path / "train-sample")
    assert run(lambda loader, model: _DebugImages(loader, model, base)) == plain and np.isfinite(plain)
    from PIL import Image

    assert sorted(p.name for p in tmp_path.iterdir()) == [f"train-sample_{k}.png" for k in ("input", "input_scaled", "mask_0", "pred_mask_0")]
    for k in ("input_scaled", "mask_0", "pred_mask_0"):
        with Image.open(f"{base}_{k}.png") as im:
            assert im.mode == "L" and im.size == MODEL_MASK[::-1]


def test_command_line_trains_and_validates(dev, trees, tmp_path, monkeypatch, capsys):
    h = trees[0]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=repo + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "ocrs_models_amd.train_detection", "hiertext", h, "--max-images", "4", "--batch-size", "2"]
    r = subprocess.run(cmd + ["--max-epochs", "1", "--no-augment"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert "Training dataset: images 4 in 2 batches" in out and "Validation dataset: images 5 in 3 batches" in out, out
    epoch = [ln for ln in out if ln.startswith("Epoch 0 train loss ")]
    assert len(epoch) == 1 and " validation loss " in epoch[0] and any(ln.startswith("Epoch 0 validation metrics:") for ln in out)
    ckpt = tmp_path / "text-detection-checkpoint.pt"
    assert ckpt.exists() and torch.load(ckpt, map_location="cpu")["epoch"] == 0
    val_loss = epoch[0].split()[-1]
    assert np.isfinite(float(val_loss)) and np.isfinite(float(epoch[0].split()[4]))
    r = subprocess.run(cmd + ["--validate-only", "--checkpoint", str(ckpt), "--no-augment"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"Validation loss {val_loss}" in r.stdout.splitlines(), r.stdout
    assert any(ln.startswith("Validation metrics:") for ln in r.stdout.splitlines())
    # --debug-images: the reference's PNGs of the last batch (train_detection.py:37-60, 186-189), and the same loss with them
    assert not list(tmp_path.glob("*.png"))
    from ocrs_models_amd import train_detection

    monkeypatch.chdir(tmp_path)  # (in this process: main() is the script, and a third child would only pay for another start)
    train_detection.main(cmd[3:] + ["--validate-only", "--checkpoint", str(ckpt), "--no-augment", "--debug-images"])
    assert f"Validation loss {val_loss}" in capsys.readouterr().out.splitlines()
    from PIL import Image

    assert sorted(p.name for p in tmp_path.glob("*.png")) == [f"test-sample_{k}.png" for k in ("input", "input_scaled", "mask_0", "pred_mask_0")]
    with open(tmp_path / "test-sample_input.png", "rb") as a, open(f"{h}/validation/page_e.jpg", "rb") as b:
        assert a.read() == b.read()  # the page's file, copied under that name as the reference copies it
    for k in ("input_scaled", "mask_0", "pred_mask_0"):
        with Image.open(tmp_path / f"test-sample_{k}.png") as im:
            assert im.mode == "L" and im.size == (600, 800)

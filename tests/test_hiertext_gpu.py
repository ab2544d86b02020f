"""The recognition dataset on the GPU (ocrs_models_amd/datasets/hiertext.py, csrc/line_data.hip): the polygon-mask kernel against PIL, items and
batches against the host restatement (tests/hiertext_ref.py) fed through the existing ``collate_lines``, the crop cache, the bucketed
sampler, the training CLI end to end on a tiny tree, and the data-parallel hook on a 1-rank RCCL group.

Every comparison of masks, crops, items and batches is ``torch.equal``: the masks are integer rasterisation restated operation by operation,
and what follows them is the same kernel sequence on the same bytes, so there is no tolerance to choose."""
from __future__ import annotations

import os
import random
import socket

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from tests import hiertext_ref as ref

pytestmark = pytest.mark.gpu


def test_mask_kernel_equals_pil(dev):
    from ocrs_models_amd._lib import lib, ptr

    cases = ref.all_polygon_cases()  # four seeds
    assert len(cases) >= 300
    verts = np.array([v for _, _, _, p in cases for v in p], dtype=np.int32).reshape(-1, 2)
    counts = np.array([len(p) for _, _, _, p in cases], dtype=np.int32)
    sizes = np.array([(h, w) for _, w, h, _ in cases], dtype=np.int32)
    area = sizes[:, 0].astype(np.int64) * sizes[:, 1]
    offs = np.cumsum(area) - area
    # (named, so that every input outlives the launch)
    d_verts, d_voffs, d_counts, d_sizes, d_offs = (torch.from_numpy(a).to(dev) for a in
                                                   (verts, np.cumsum(counts, dtype=np.int64) - counts, counts, sizes, offs))
    out = torch.full((int(area.sum()) + 64,), 7, dtype=torch.uint8, device=dev)
    lib().line_mask(ptr(d_verts), ptr(d_voffs), ptr(d_counts), ptr(d_sizes), ptr(d_offs), ptr(out), len(cases), int(sizes[:, 0].max()))
    got = out.cpu().numpy()
    assert (got[int(area.sum()):] == 7).all()  # nothing written past the last mask
    bad = []
    for (fam, w, h, p), o in zip(cases, offs.tolist()):
        diff = int((got[o:o + h * w].reshape(h, w) != ref.pil_mask(w, h, p)).sum())
        if diff:
            bad.append((fam, w, h, p, diff))
    assert not bad, bad[:3]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("hiertext"))
    kept = ref.write_tree(root, "train")
    ref.write_tree(root, "validation", seed=2)
    pages = {name: ref.read_gray(os.path.join(root, "train", name + ".jpg")) for name in ref.PAGES}
    return root, kept, pages


def _host_samples(kept, pages, alphabet):
    from ocrs_models_amd.text import encode_text

    out = []
    for pid, vertices, text in kept:
        crop, mask, masked = ref.item(pages[pid], vertices)
        out.append({"image": crop, "mask": mask, "masked": masked, "text_seq": encode_text(text, alphabet, unknown_char="?"), "image_id": pid})
    return out


def test_items_equal_the_reference(dev, tree):
    from ocrs_models_amd.augment import collate_lines
    from ocrs_models_amd.datasets import HierTextRecognition
    from ocrs_models_amd.input_pipeline import line_output_width

    root, kept, pages = tree
    ds = HierTextRecognition(root, device=dev)
    want = _host_samples(kept, pages, ds.alphabet)
    assert len(ds) == len(want) == 9
    raw = ds.raw(range(len(ds)))
    for i, s in enumerate(want):
        crop, mask = raw[i]
        assert torch.equal(crop.cpu(), s["image"]) and torch.equal(mask.cpu(), s["mask"]), i
        img, m = crop.cpu().float() / 255.0 - 0.5, mask.cpu().float()  # (hiertext.py:273-274 on the host: ATen's CPU division)
        assert torch.equal(torch.full(img.shape, -0.5) * (1.0 - m) + img * m, s["masked"]), i
        item = ds[i]
        h, w = s["image"].shape[-2:]
        ow = line_output_width(h, w)
        assert item["image_id"] == s["image_id"] and torch.equal(item["text_seq"], s["text_seq"])
        assert item["image"].is_cuda and item["image"].dtype == torch.float32 and tuple(item["image"].shape) == (1, 64, ow)
        assert ds.widths[i] == ow
    # the existing pipeline fed with the reference crops and PIL masks, one sample at a time (an infeasible sample is dropped by
    # collate_lines, so those are compared through a feasible text)
    for i, s in enumerate(want):
        one = dict(s, text_seq=s["text_seq"][:1])
        host = collate_lines([one], dev, augment=False)["image"]
        assert torch.equal(ds[i]["image"], host[0, :, :, :ds.widths[i]]), i


@pytest.mark.parametrize("augment", [False, True])
def test_loader_equals_the_host_fed_route(dev, tree, augment):
    from ocrs_models_amd.augment import collate_lines, sample_line_params
    from ocrs_models_amd.datasets import DeviceLineLoader, HierTextRecognition

    root, kept, pages = tree
    ds = HierTextRecognition(root, augment=augment, device=dev)
    want = _host_samples(kept, pages, ds.alphabet)
    g = torch.Generator().manual_seed(5)
    stock = DataLoader(list(range(len(ds))), batch_size=5, shuffle=True, generator=g)
    order = [[int(i) for i in b] for b in stock]
    loader = DeviceLineLoader(ds, batch_size=5, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert len(loader) == len(stock) == 2
    assert list(DeviceLineLoader(ds, batch_size=5, shuffle=True, generator=torch.Generator().manual_seed(5)).plan()) == order
    # the draws: the loader takes them from the global generators in batch order; the host route is given the same ones
    torch.manual_seed(9)
    random.seed(9)
    got = list(loader)
    torch.manual_seed(9)
    random.seed(9)
    dropped = 0
    for idx, b in zip(order, got):
        samples = [want[i] for i in idx]
        sizes = [tuple(s["image"].shape[-2:]) for s in samples]
        params = sample_line_params(sizes) if augment else None
        host = collate_lines(samples, dev, augment=augment, params=params)
        dropped += len(idx) - b["image"].shape[0]
        assert b["image"].is_cuda and torch.equal(b["image"], host["image"])
        for key in ("text_seq", "text_len", "image_width"):
            assert torch.equal(b[key], host[key]), key
    assert dropped == 1  # the line whose text cannot fit its width


def test_cache_is_the_references_and_is_enough(dev, tmp_path):
    from ocrs_models_amd.datasets import HierTextRecognition

    root = str(tmp_path)
    kept = ref.write_tree(root)
    ds = HierTextRecognition(root, device=dev)
    for pid, vertices, _ in kept:
        x0, y0, x1, y1 = ref.line_box(vertices)
        assert os.path.exists(f"{root}/train-lines-cache/{pid}/{x0}_{y0}_{x1}_{y1}.png")
    assert not [f for _, _, fs in os.walk(f"{root}/train-lines-cache") for f in fs if f.endswith(".tmp")]
    first = [ds[i] for i in range(len(ds))]
    for name in ref.PAGES:
        os.remove(f"{root}/train/{name}.jpg")
    again = HierTextRecognition(root, device=dev)
    assert len(again) == len(ds)
    for a, b in zip(first, [again[i] for i in range(len(again))]):
        assert a["image_id"] == b["image_id"] and torch.equal(a["image"], b["image"]) and torch.equal(a["text_seq"], b["text_seq"])


def test_bucketed_sampler_hook(dev, tree):
    from ocrs_models_amd.datasets import DeviceLineLoader, HierTextRecognition
    from ocrs_models_amd.sampler import WidthBucketedDistributedSampler

    root, kept, _ = tree
    ds = HierTextRecognition(root, device=dev)
    sampler = WidthBucketedDistributedSampler(ds.widths, batch_size=2, drop_last=False)
    schedule = sampler.schedule()
    loader = DeviceLineLoader(ds, batch_sampler=sampler)
    assert len(loader) == len(schedule)
    seen = []
    for (bucket, idx), batch in zip(schedule, loader):
        seen += idx
        assert batch["image"].shape[-1] == bucket  # round_up(max width, 256) of a batch from one bucket is the bucket
    assert set(seen) == set(range(len(ds)))
    # one sample per batch: every index exactly once, padded to its own bucket
    from ocrs_models_amd.sampler import bucket_of

    single = WidthBucketedDistributedSampler(ds.widths, batch_size=1)
    once = [i for _, idx in single.schedule() for i in idx]
    assert sorted(once) == list(range(len(ds)))
    feasible = [b for b in DeviceLineLoader(ds, batch_sampler=single) if b["image"].shape[0]]
    assert len(feasible) == len(ds) - 1 and all(b["image"].shape[-1] == bucket_of(int(b["image_width"][0])) for b in feasible)


def test_main_trains_resumes_validates_and_exports(dev, tmp_path, monkeypatch, capsys):
    import math

    from ocrs_models_amd import train_rec
    from ocrs_models_amd.export import AtenGraph
    # a tree of its own without the infeasible line: a last batch holding nothing else would be empty after collate_samples' drop rule, which
    # the reference's script does not survive either
    root = str(tmp_path / "data")
    lines = [ln for ln in ref.tree_lines() if len(ln[1]["text"]) < 20]
    ref.write_tree(root, "train", lines=lines)
    ref.write_tree(root, "validation", seed=2, lines=lines)
    monkeypatch.chdir(tmp_path)
    train_rec.main(["hiertext", root, "--max-images", "8", "--batch-size", "4", "--max-epochs", "2"])
    lines = capsys.readouterr().out.splitlines()
    lines = [ln for ln in lines if not ln.startswith(("Sample test prediction", "Mean grad norm"))]
    first = [k for k, ln in enumerate(lines) if ln.startswith("Model param count ")]
    assert len(first) == 1 and lines[0].startswith("Extracting text line annotations from ")  # the validation lines file is made here
    lines = lines[first[0]:]
    assert lines[0].startswith("Model param count ") and len(lines) == 1 + 3 * 2, lines
    for e in range(2):
        a, b, c = lines[1 + 3 * e: 4 + 3 * e]
        assert a.startswith(f"Epoch {e} train loss ") and " char error rate " in a
        assert b.startswith(f"Epoch {e} validation loss ") and " char error rate " in b
        assert c.startswith("Current learning rate [")
        assert math.isfinite(float(a.split()[4])) and math.isfinite(float(b.split()[4]))
    ckpt = str(tmp_path / "text-rec-checkpoint.pt")
    assert os.path.exists(ckpt) and torch.load(ckpt, map_location="cpu")["epoch"] == 1
    before = torch.load(ckpt, map_location="cpu")["model_state"]

    train_rec.main(["hiertext", root, "--max-images", "8", "--batch-size", "4", "--max-epochs", "3", "--checkpoint", ckpt, "--no-augment",
                    "--stats", "device"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch ")]
    assert [ln.split()[1] for ln in lines] == ["1", "1", "2", "2"]  # load_checkpoint's epoch is where training goes on, as in the reference

    before = torch.load(ckpt, map_location="cpu")["model_state"]  # (the resumed run saved again)
    (tmp_path / "v").mkdir()
    monkeypatch.chdir(tmp_path / "v")
    seen = {}
    real_test = train_rec.test

    def spy_test(device, dataloader, model, **kw):
        seen["model"] = model
        return real_test(device, dataloader, model, **kw)

    def no_train(*a, **k):
        raise AssertionError("--validate-only must not train")

    with monkeypatch.context() as mp:
        mp.setattr(train_rec, "test", spy_test)
        mp.setattr(train_rec, "train", no_train)
        train_rec.main(["hiertext", root, "--max-images", "8", "--batch-size", "4", "--validate-only", "--checkpoint", ckpt])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("Sample test prediction")]
    assert len(lines) == 2 and lines[1].startswith("Validation loss ") and " char error rate " in lines[1]
    assert not os.path.exists("text-rec-checkpoint.pt")
    after = {k: v.cpu() for k, v in seen["model"].state_dict().items()}  # the model main() validated, after it returned
    assert set(after) == set(before) and all(torch.equal(before[k], after[k]) for k in before)

    # --export: main() loads the checkpoint, takes the first validation batch and hands both to export.export_onnx.  Without the onnx
    # package torch.onnx.export cannot run, so export_onnx is replaced by what the existing export tests do with its graph: a trace.
    import importlib.util

    from ocrs_models_amd import export

    if importlib.util.find_spec("onnx") is not None:
        train_rec.main(["hiertext", root, "--max-images", "8", "--batch-size", "4", "--export", "rec.onnx", "--checkpoint", ckpt])
        assert os.path.getsize("rec.onnx") > 0
    else:
        calls = []

        def trace_export(model, path, sample):
            g = AtenGraph(model).eval()
            tr = torch.jit.trace(g, sample, check_trace=False)
            with torch.no_grad():
                calls.append((type(model).__name__, path, tuple(sample.shape), tuple(tr(sample).shape)))
            torch.jit.save(tr, path)

        with monkeypatch.context() as mp:
            mp.setattr(export, "export_onnx", trace_export)
            mp.setattr(train_rec, "train", no_train)
            train_rec.main(["hiertext", root, "--max-images", "8", "--batch-size", "4", "--export", "rec.pt", "--checkpoint", ckpt])
        (name, path, shape, out_shape), = calls
        assert name == "RecognitionModel" and path == "rec.pt" and shape[:3] == (4, 1, 64) and shape[3] % 256 == 0
        assert out_shape[1] == 4 and os.path.getsize("rec.pt") > 0
        assert [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("Epoch", "Validation"))] == []


# ------------------------------------------------------------------------------------------------ data-parallel hook
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(port, root, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", OCRS_DDP_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = {}
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    except Exception:  # noqa: BLE001
        import traceback

        q.put({"error": traceback.format_exc()})
        return
    try:
        import ocrs_models_amd as oa
        from ocrs_models_amd.datasets import DeviceLineLoader, HierTextRecognition
        from ocrs_models_amd.ddp import DistributedDataParallel
        from ocrs_models_amd.losses import CTCLoss
        from ocrs_models_amd.sampler import WidthBucketedDistributedSampler

        torch.manual_seed(3)
        m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev).train()
        ds = HierTextRecognition(root, device=dev)
        sampler = WidthBucketedDistributedSampler(ds.widths, batch_size=3, rank=0, world_size=1, drop_last=False)
        batch = next(iter(DeviceLineLoader(ds, batch_sampler=sampler)))
        loss_fn = CTCLoss()

        names = [n for n, _ in m.named_parameters()]
        atomic = [n.endswith("bias") or n.startswith("conv.0.") for n in names]  # summed with fp32 atomics

        def run(net):
            m.zero_grad()
            with torch.autocast(device_type="cuda", dtype=torch.bfloat16):  # as train_rec.train_step runs it
                pred = net(batch["image"])
                loss = loss_fn(pred, batch["text_seq"].to(dev), batch["image_width"].div(4, rounding_mode="floor"), batch["text_len"])
            loss.backward()
            torch.cuda.synchronize()
            return [p.grad.clone() for p in m.parameters()]

        def compare(got, want):
            flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])  # noqa: E731
            rel = float((flat(got) - flat(want)).abs().max() / flat(want).abs().max())
            return rel, [n for n, a, g, w in zip(names, atomic, got, want) if not a and not torch.equal(g, w)]

        local = run(m)
        out["nonzero"] = all(bool(torch.isfinite(g).all()) for g in local) and any(bool(g.abs().max() > 0) for g in local)
        out["repeat"] = compare(run(m), local)  # two undistributed runs
        out["ddp"] = compare(run(DistributedDataParallel(m)), local)
    except Exception:  # noqa: BLE001
        import traceback

        out["error"] = traceback.format_exc()
    finally:
        dist.destroy_process_group()
    q.put(out)


def test_ddp_one_rank_rccl(dev, tree):
    """RecognitionModel under ddp.DistributedDataParallel in a 1-rank RCCL group with the collectives forced on (a fresh child process), fed by
    DeviceLineLoader through the bucketed sampler, bf16 autocast as in train_step: the gradients are the unwrapped model's.  The CRNN step
    is bit-reproducible except the bias and first-layer (conv.0) gradients, which are summed with fp32 atomics in no fixed order
    (tests/test_rec_gpu.py::test_recognition_bf16_step_is_bit_stable): every other gradient must be bit-equal,
    and those within the 1e-5 of the largest gradient that test and test_train_loop_gpu.py::test_ddp_one_rank_rccl_hip_models hold them to.
    Two undistributed runs are held to the same, so a failure of the wrapped run alone points at the hook."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ddp_worker, args=(_free_port(), tree[0], q))
    p.start()
    try:
        out = q.get(timeout=240)
    finally:
        p.join(60)
        if p.is_alive():
            p.kill()
    assert "error" not in out, out["error"]
    print("recognition DDP, 1 rank:", out)
    assert out["nonzero"], out
    for key in ("repeat", "ddp"):
        rel, unequal = out[key]
        assert rel <= 1e-5 and not unequal, (key, out)

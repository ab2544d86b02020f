"""The device-resident layout dataset on the GPU (ocrs_models_amd/datasets/web_layout.py, csrc/layout_data.hip): items against the reference's recorded
outputs, batches against a stock DataLoader over the CPU restatement (tests/weblayout_ref.py), the training CLI end to end on a small
directory, and the data-parallel hook of the layout backward on a 1-rank RCCL group.

Every comparison of items and batches is ``torch.equal``: each coordinate is a chain of single IEEE fp64 operations followed by one rounding
to fp32, on the device as in the reference, so there is no tolerance to choose."""
from __future__ import annotations

import json
import os
import random
import socket

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from tests import weblayout_ref as ref

pytestmark = pytest.mark.gpu


def test_items_equal_the_reference(dev):
    from ocrs_models_amd.datasets import WebLayout

    gold = np.load(ref.GOLDEN)
    by_config = {}
    for key, name, normalize, padded, seed, jitter in ref.golden_cases():
        by_config.setdefault((normalize, padded, jitter), []).append((key, name, seed))
    seen = 0
    for (normalize, padded, jitter), cases in by_config.items():
        for train in (True, False):  # the two splits partition the fixture directory
            ds = WebLayout(ref.PAGES, randomize=jitter is not None, padded_size=padded, train=train, normalize_coords=normalize,
                           max_jitter=jitter or 25, device=dev)
            for key, name, seed in cases:
                if name not in ds._files:
                    continue
                if seed is not None:
                    torch.manual_seed(seed)
                x, y = ds[ds._files.index(name)]
                want = torch.from_numpy(gold[key])
                assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32
                assert x.shape == want[:, :4].shape and y.shape == want[:, 4:].shape, key
                assert torch.equal(x.cpu(), want[:, :4]) and torch.equal(y.cpu(), want[:, 4:]), key
                seen += 1
    assert seen == len(gold.files)


def test_loader_equals_stock_dataloader(dev, tmp_path):
    """padded_size 16 against pages of 1 ... 40 words, batches of 5, 5 and 2, shuffled, jittered, two epochs."""
    from ocrs_models_amd.datasets import DeviceWebLayoutLoader, WebLayout

    d = ref.copy_pages(tmp_path)
    kw = dict(randomize=True, padded_size=16, normalize_coords=True, max_jitter=25)
    stock = DataLoader(ref.RefWebLayout(d, **kw), batch_size=5, shuffle=True)
    torch.manual_seed(7)
    want = [list(stock), list(stock)]
    loader = DeviceWebLayoutLoader(WebLayout(d, device=dev, **kw), batch_size=5, shuffle=True)
    assert len(loader) == 3
    torch.manual_seed(7)
    for epoch in range(2):
        got = list(loader)
        assert [tuple(b[0].shape) for b in got] == [(5, 16, 4), (5, 16, 4), (2, 16, 4)]
        for (x, y), (wx, wy) in zip(got, want[epoch]):
            assert torch.equal(x.cpu(), wx) and torch.equal(y.cpu(), wy)


def test_batch_of_64_by_64(dev):
    """The largest shape: 64 pages (the 12 fixtures repeated, each with its own jitter) by 64 slots, several workgroups."""
    from ocrs_models_amd.datasets import WebLayout

    files = ref.select_files(ref.PAGES, train=True) + ref.select_files(ref.PAGES, train=False)
    g = torch.Generator().manual_seed(11)
    jit = (torch.rand(64, 2, generator=g, dtype=torch.float64) * 25).tolist()
    for train in (True, False):
        ds = WebLayout(ref.PAGES, padded_size=64, train=train, device=dev)
        pages = [i % len(ds) for i in range(64)]
        x, y = ds.batch(pages, [j[0] for j in jit], [j[1] for j in jit])
        items = [ref.item(os.path.join(ref.PAGES, ds._files[p]), True, 64, tuple(j)) for p, j in zip(pages, jit)]
        assert torch.equal(x.cpu(), torch.stack([i[0] for i in items])) and torch.equal(y.cpu(), torch.stack([i[1] for i in items]))
    assert len(files) == 12
    with pytest.raises(IndexError):
        ds.batch([len(ds)], [0.0], [0.0])


def _synthetic_pages(dst, n=8, seed=5):
    r = random.Random(seed)
    for k in range(n):
        paras, y = [], 20.0
        for _ in range(r.randint(2, 5)):
            words = []
            for _ in range(r.randint(1, 3)):  # lines
                x = 30.0
                for _ in range(r.randint(1, 5)):
                    w = r.uniform(20, 90)
                    words.append({"coords": [x, y, x + w, y + 18.0]})
                    x += w + 6
                y += 24.0
            paras.append({"words": words})
            y += 12.0
        with open(os.path.join(dst, f"synthetic_{k}.json"), "w") as f:
            json.dump({"resolution": {"width": 1280, "height": 720}, "paragraphs": paras}, f)


def test_main_trains_checkpoints_and_validates(dev, tmp_path, monkeypatch, capsys):
    """``main`` on 20 pages (16 train in batches of 4, one validation batch of 4): writes the checkpoint, is bit-stable for its seed (the
    dropout keys come from the seeded CPU generator), and --validate-only reproduces the validation line of the epoch that was saved (one
    batch, so its shuffled page order only permutes the attention's keys: the line's three decimals are those of the same counts)."""
    from ocrs_models_amd import LayoutModel, train_layout

    data = tmp_path / "data"
    data.mkdir()
    ref.copy_pages(data, extra=0)
    _synthetic_pages(str(data))
    monkeypatch.setattr(train_layout, "N_WORDS", 16)
    monkeypatch.setattr(train_layout, "BATCH_SIZE", 4)
    outs = []
    for run in ("run1", "run2"):
        (tmp_path / run).mkdir()
        monkeypatch.chdir(tmp_path / run)
        train_layout.main([str(data), "--max-epochs", "2"])
        outs.append(capsys.readouterr().out.splitlines())
        assert os.path.exists("text-layout-checkpoint.pt")
    assert outs[0] == outs[1]
    lines = outs[0]
    assert lines[0].startswith("Model param count ") and len(lines) == 1 + 2 * 4
    for e in range(2):
        blk = lines[1 + 4 * e: 5 + 4 * e]
        assert blk[0].startswith(f"Epoch {e} train loss ") and " val loss " in blk[0]
        assert blk[1].startswith(f"Epoch {e} train stats: line start prec/recall ")
        assert blk[2].startswith(f"Epoch {e} val stats: line start prec/recall ")
        assert blk[3].startswith(f"Epoch {e} lr ")
    ckpt_path = str(tmp_path / "run1" / "text-layout-checkpoint.pt")
    model = LayoutModel().to(dev)
    ckpt = train_layout.load_checkpoint(ckpt_path, model, train_layout.make_optimizer(model), dev)
    assert ckpt["epoch"] in (0, 1)
    train_layout.main([str(data), "--validate-only", "--checkpoint", ckpt_path])
    val = capsys.readouterr().out.splitlines()
    assert val[1:] == [lines[1 + 4 * ckpt["epoch"] + 2]]


# ------------------------------------------------------------------------------------------------ data-parallel hook
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker(port, q):
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
        from ocrs_models_amd.ddp import DistributedDataParallel

        torch.manual_seed(3)
        m = oa.LayoutModel().to(dev).train()
        m.dropout_p = 0.0
        g = torch.Generator().manual_seed(4)
        boxes = (torch.rand(5, 33, 4, generator=g) * 1500).round().to(dev)
        target = (torch.rand(5, 33, 2, generator=g) < 0.2).float().to(dev)
        loss_fn = oa.train_layout.weighted_loss()

        def run(net):
            m.zero_grad()
            loss_fn(net(boxes), target).backward()
            torch.cuda.synchronize()
            return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()

        local = run(m)
        out["n"] = local.numel()
        out["layer"] = sum(p.numel() for p in m.encode.layers[0].parameters())
        out["nonzero"] = bool(local.abs().max() > 0)
        for name, bucket_bytes in (("small", 1 << 20), ("one", 1 << 30)):
            ddp = DistributedDataParallel(m, bucket_bytes=bucket_bytes)
            got = run(ddp)
            out[name] = (bool(torch.equal(got, local)), list(ddp.bucketer.last_ranges))
            del m._grad_bucketer
    except Exception:  # noqa: BLE001
        import traceback

        out["error"] = traceback.format_exc()
    finally:
        dist.destroy_process_group()
    q.put(out)


def test_ddp_hook_one_rank_rccl(dev):
    """LayoutModel under ddp.DistributedDataParallel in a 1-rank RCCL group with the collectives forced on (a fresh child process): the
    gradients are the unwrapped model's bit for bit, the reported ranges tile the flat buffer in order, and buckets smaller than an encoder
    layer (1 MiB against 3.2 MB) go out as more than one range."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ddp_worker, args=(_free_port(), q))
    p.start()
    try:
        out = q.get(timeout=240)
    finally:
        p.join(60)
        if p.is_alive():
            p.kill()
    assert "error" not in out, out["error"]
    n = out["n"]
    assert out["nonzero"] and n == 6 * out["layer"] + 256 * 2 + 2 and (1 << 20) < 4 * out["layer"]
    for name in ("small", "one"):
        equal, ranges = out[name]
        assert equal, name
        assert ranges and ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), ranges
    assert len(out["small"][1]) > 1 and len(out["one"][1]) == 1

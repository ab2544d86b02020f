"""CPU checks of the layout dataset (ocrs_models_amd/datasets/web_layout.py): the restatement the GPU tests compare against equals the reference's
recorded items; file selection, load-time refusals and the random stream of DeviceWebLayoutLoader need no GPU; the CLI parses and refuses
to run without one."""
import itertools
import json
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from ocrs_models_amd import datasets, train_layout
from tests import weblayout_ref as ref

GOLDEN, golden_cases = ref.GOLDEN, ref.golden_cases


def test_golden_covers_the_issue_cases():
    cases = golden_cases()
    names = {c[1] for c in cases}
    assert names == {f for f in os.listdir(ref.PAGES) if f.endswith(".json")} and len(names) == 12
    assert {(c[2], c[3]) for c in cases} == set(itertools.product((False, True), (None, 1, 16, 64)))
    assert {(c[4], c[5]) for c in cases} == {(None, None)} | set(itertools.product((0, 1234), (10, 25)))
    assert len(cases) == 12 * 8 * 5
    gold = np.load(GOLDEN)
    counts = sorted(gold[f"{n}|n0|pNone|fixed"].shape[0] for n in names)
    assert {1, 15, 16, 17, 40} <= set(counts)
    # word 16 decides the line_end of word 15 both ways, in the 17- and in the 40-word pages
    for n in (17, 40):
        ends = {float(gold[f"words{n}_{v}.json|n0|p16|fixed"][15, 5]) for v in ("same_line", "next_line")}
        assert ends == {0.0, 1.0}


def test_restatement_equals_every_golden():
    gold = np.load(GOLDEN)
    for key, name, normalize, padded, seed, jitter in golden_cases():
        jit = (0.0, 0.0)
        if seed is not None:
            torch.manual_seed(seed)
            a, b, c = torch.rand(3).tolist()
            jit = (a * jitter, b * jitter)
        x, y = ref.item(os.path.join(ref.PAGES, name), normalize, padded, jit)
        want = torch.from_numpy(gold[key])
        assert torch.equal(x, want[:, :4]) and torch.equal(y, want[:, 4:]), key


def _page(path, words=((1.0, 2.0, 3.0, 4.0),)):
    with open(path, "w") as f:
        json.dump({"resolution": {"width": 100, "height": 50}, "paragraphs": [{"words": [{"coords": list(w)} for w in words]}]}, f)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 12])
def test_file_selection(tmp_path, n):
    for i in range(n):
        _page(tmp_path / f"p{(i * 7) % 13:02d}.json")
    (tmp_path / "notes.txt").write_text("x")
    (tmp_path / "dir.json").mkdir()
    listed = [f for f in os.listdir(tmp_path) if f.endswith(".json") and f != "dir.json"]
    train = datasets.WebLayout(str(tmp_path), train=True)
    val = datasets.WebLayout(str(tmp_path), train=False)
    assert len(train) == round(n * 4 / 5) and len(val) == n - len(train)
    assert train._files + val._files == listed  # a partition, both parts in os.listdir order
    assert train._files == ref.select_files(str(tmp_path), True) and val._files == ref.select_files(str(tmp_path), False)
    if n >= 7:
        first = train._files[0]
        got = datasets.WebLayout(str(tmp_path), max_images=3, filter=lambda f: f != first)._files
        assert got == train._files[1:3]  # max_images first, then the filter (the other order would keep three)
        assert datasets.WebLayout(str(tmp_path), max_images=2)._files == train._files[:2]


def test_load_time_refusals(tmp_path):
    for sub in ("fine", "negative", "empty"):
        (tmp_path / sub).mkdir()
    _page(tmp_path / "fine" / "fine.json")
    assert len(datasets.WebLayout(str(tmp_path / "fine"))) == 1
    _page(tmp_path / "negative" / "negative.json", words=((1.0, 2.0, 3.0, 4.0), (5.0, -0.25, 6.0, 7.0)))
    with pytest.raises(ValueError, match="negative.json"):
        datasets.WebLayout(str(tmp_path / "negative"))
    with open(tmp_path / "empty" / "empty.json", "w") as f:
        json.dump({"resolution": {"width": 100, "height": 50}, "paragraphs": [{"words": []}, {"words": []}]}, f)
    with pytest.raises(ValueError, match="empty.json"):
        datasets.WebLayout(str(tmp_path / "empty"))


@pytest.mark.parametrize("seed", [0, 1234])
@pytest.mark.parametrize("batch_size", [1, 5, 64])
@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_plan_is_the_stock_dataloaders_random_stream(tmp_path, seed, batch_size, shuffle):
    """The (index, jitter) plan DeviceWebLayoutLoader draws equals what DataLoader(dataset, batch_size, shuffle) over the restatement
    consumes: compared through the batches, two epochs in a row."""
    d = ref.copy_pages(tmp_path)
    kw = dict(randomize=True, padded_size=16, normalize_coords=False, max_jitter=10)
    stock = DataLoader(ref.RefWebLayout(d, **kw), batch_size=batch_size, shuffle=shuffle)
    torch.manual_seed(seed)
    want = [list(stock), list(stock)]
    ds = datasets.WebLayout(d, **kw)
    loader = datasets.DeviceWebLayoutLoader(ds, batch_size=batch_size, shuffle=shuffle)
    assert len(ds) == 12 and len(loader) == len(stock)
    torch.manual_seed(seed)
    for epoch in range(2):
        plan = list(loader.plan())
        assert len(plan) == len(want[epoch])
        for (pages, jx, jy), (wx, wy) in zip(plan, want[epoch]):
            assert pages.dtype == torch.int64 and jx.dtype == torch.float64 and jy.dtype == torch.float64
            items = [ref.item(os.path.join(d, ds._files[p]), False, 16, (a, b)) for p, a, b in zip(pages.tolist(), jx.tolist(), jy.tolist())]
            assert torch.equal(torch.stack([i[0] for i in items]), wx) and torch.equal(torch.stack([i[1] for i in items]), wy)
    if shuffle:
        assert not all(torch.equal(a[0], b[0]) for a, b in zip(want[0], want[1]))


def test_main_help_exits_0(capsys):
    with pytest.raises(SystemExit) as e:
        train_layout.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for arg in ("data_dir", "--checkpoint", "--export", "--max-epochs", "--validate-only"):
        assert arg in out


def test_main_refuses_to_run_without_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match=r"MI355X only \(no CPU path\)"):
        train_layout.main([ref.copy_pages(tmp_path)])
    ds = datasets.WebLayout(str(tmp_path), padded_size=16)
    with pytest.raises(RuntimeError, match=r"MI355X only \(no CPU path\)"):
        ds[0]

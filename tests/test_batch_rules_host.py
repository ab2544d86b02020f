"""The batch rules of the data path, pinned to what they gave before they were stated once (CPU: host arithmetic only, no kernel runs).

Four things feed every batch the data path makes, and each had several hand-written copies before ``text.collate_plan``,
``augment.resolve_params`` and the ``datasets`` package: a change to one of them must not move a single number.

* the collate plan (padded width with the ``round_up`` quirk, padded target length, infeasible-sample drop, the three metadata tensors),
  through both entry points that run on the host: ``text.collate_samples`` and the line-batch plan of ``augment``.  For the same input the
  two must give the same metadata (``test_the_host_entry_points_agree``); ``input_pipeline.collate_samples`` needs the library and is
  compared with ``text.collate_samples`` by tests/test_input_pipeline_gpu.py.
* the device records and line offsets a seeded augmentation draw is packed into, and how much of torch's and Python's global random
  streams the draw consumes (the next number of each stream is recorded).
* ``draw_params`` of a page store and of a line store, with the augmentations on and off.
* the import graph: each data-path module can be the first one a fresh interpreter imports.

tests/golden/batch_rules.json maps a case name to its answer; it was written by running this file as a script on the commit before the
rules were stated once (``answers()`` enumerates the cases; every function is looked up under its present name, then under that commit's):

    python tests/test_batch_rules_host.py > tests/golden/batch_rules.json
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_rules.json")
WIDTHS = (10, 40, 255, 256, 257, 512, 800)
LENGTHS = (0, 1, 63, 64, 65)
SIZES = [(30, 40), (64, 300), (601, 799), (1200, 900)]
SEEDS = range(4)
MODULES = ("text", "augment", "input_pipeline", "datasets")


def _augment():
    from ocrs_models_amd import augment as A

    return A, getattr(A, "records", None) or A._records, getattr(A, "line_records", None) or A._line_records, \
        getattr(A, "line_batch_plan", None) or A._line_batch_plan


def _seq(length: int) -> torch.Tensor:
    return (torch.arange(length, dtype=torch.int32) % 90) + 1  # no two neighbours equal: feasible from ``length`` steps on


def collate_cases() -> dict:
    """name -> ([(width, text_seq)], pad_to)"""
    dropped = (40, torch.full((6,), 7, dtype=torch.int32))  # six equal labels need 11 steps, width 40 gives 10
    assert dropped[0] // 4 == 10
    fine = [(257, _seq(5)), (40, _seq(3))]
    cases = {f"one_w{w}_l{n}": ([(w, _seq(n))], None) for w in WIDTHS for n in LENGTHS}
    cases["every_width"] = ([(w, _seq(LENGTHS[k % len(LENGTHS)])) for k, w in enumerate(WIDTHS)], None)
    cases["every_length_at_800"] = ([(800, _seq(n)) for n in LENGTHS], None)
    cases["all_dropped"] = ([dropped, (10, _seq(63))], None)
    cases["first_dropped"] = ([dropped] + fine, None)
    cases["middle_dropped"] = ([fine[0], dropped, fine[1]], None)
    for name, pad_to in (("below", 256), ("equal", 512), ("above", 1024)):
        cases[f"pad_to_{name}"] = (fine, pad_to)
    cases["pad_to_above_first_dropped"] = ([dropped] + fine, 768)
    return cases


def _tensor(t: torch.Tensor) -> dict:
    return {"dtype": str(t.dtype), "shape": list(t.shape), "values": t.tolist()}


def _meta(batch: dict) -> dict:
    return {k: _tensor(batch[k]) for k in ("text_seq", "text_len", "image_width")}


def _through_collate_samples(samples, pad_to) -> dict:
    from ocrs_models_amd import text

    # sample k is filled with (k + 1) / 16, so the first pixel of every row of the batch names the position it was kept from
    batch = text.collate_samples([{"image": torch.full((1, 64, w), (k + 1) / 16), "text_seq": t} for k, (w, t) in enumerate(samples)], pad_to=pad_to)
    image = batch["image"]
    keep = [int(v * 16) - 1 for v in image[:, 0, 0, 0].tolist()]
    for i, k in enumerate(keep):
        w = samples[k][0]
        assert bool((image[i, :, :, :w] == (k + 1) / 16).all()) and bool((image[i, :, :, w:] == 0).all())
    return {"keep": keep, "padded_width": image.shape[-1], "image": {"dtype": str(image.dtype), "shape": list(image.shape)}, **_meta(batch)}


def _through_line_plan(samples) -> dict:
    A, _, _, plan = _augment()
    params = [A.AugParams(-1, (64, w), (64, w)) for w, _ in samples]  # height 64 already: the resized width is the width
    image, meta, keep = plan([t for _, t in samples], params, 64, torch.float32, "cpu")
    return {"keep": list(keep), "padded_width": image.shape[-1], "image": {"dtype": str(image.dtype), "shape": list(image.shape)}, **_meta(meta)}


def _draw(sample, pack) -> dict:
    """what ``pack(sample(SIZES))`` is for every seed, and the next number of both global streams after the draw"""
    out = {}
    for s in SEEDS:
        torch.manual_seed(s)
        random.seed(s)
        packed = pack(sample(SIZES))
        out[f"seed{s}"] = {**{k: np.ascontiguousarray(v).tobytes().hex() for k, v in packed.items()}, "torch_next": torch.rand(1).item(),
                           "python_next": random.random()}
    return out


def _stores():
    from ocrs_models_amd.datasets import HierText, HierTextRecognition

    pages = [np.zeros(s, np.uint8) for s in SIZES]
    lines = [[(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)] for h, w in SIZES]
    return {(kind, on): (HierText.from_pages(pages, [[] for _ in pages], augment=on, device="cpu") if kind == "pages" else
                         HierTextRecognition.from_lines(pages, lines, [_seq(3) for _ in pages], augment=on, device="cpu"))
            for kind in ("pages", "lines") for on in (False, True)}


def answers() -> dict:
    A, records, line_records, _ = _augment()
    out = {}
    for name, (samples, pad_to) in collate_cases().items():
        out[f"collate_samples/{name}"] = _through_collate_samples(samples, pad_to)
        if pad_to is None:
            out[f"line_plan/{name}"] = _through_line_plan(samples)
    pack_det = lambda params: {"records": records(params, line=False)}  # noqa: E731
    pack_lines = lambda params: dict(zip(("records", "offsets"), line_records(params, 64)))  # noqa: E731
    out["records/detection"] = _draw(A.sample_detection_params, pack_det)
    out["records/lines"] = _draw(A.sample_line_params, pack_lines)
    for (kind, on), ds in _stores().items():
        out[f"draw_params/{kind}/augment_{'on' if on else 'off'}"] = _draw(lambda sizes: ds.draw_params(range(len(sizes))),
                                                                            pack_det if kind == "pages" else pack_lines)
    return out


GOT = {}


def _got() -> dict:
    if not GOT:
        GOT.update(json.loads(json.dumps(answers())))  # (through JSON, as the golden went: tuples become lists)
    return GOT


def test_golden_covers_every_case():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(_got())
    names = collate_cases()
    assert len(names) == len(WIDTHS) * len(LENGTHS) + 9
    assert golden["collate_samples/all_dropped"]["keep"] == [] and golden["collate_samples/all_dropped"]["image"]["shape"] == [0, 1, 64, 256]
    assert golden["collate_samples/first_dropped"]["keep"] == [1, 2] and golden["collate_samples/middle_dropped"]["keep"] == [0, 2]
    assert [golden[f"collate_samples/pad_to_{n}"]["padded_width"] for n in ("below", "equal", "above")] == [512, 512, 1024]
    assert golden["collate_samples/one_w256_l1"]["padded_width"] == 512 and golden["collate_samples/one_w255_l1"]["padded_width"] == 256  # the quirk
    assert golden["collate_samples/one_w800_l64"]["text_seq"]["shape"] == [1, 128]  # and the same quirk on the target length


def test_batch_rules_match_the_recorded_ones():
    golden, got = json.load(open(GOLDEN)), _got()
    wrong = [name for name in golden if got[name] != golden[name]]
    assert not wrong, (wrong[:10], got[wrong[0]], golden[wrong[0]])


def test_the_host_entry_points_agree():
    got = _got()
    plans = [name for name in got if name.startswith("line_plan/")]
    assert len(plans) == len(collate_cases()) - 4
    for name in plans:
        a, b = got[name], got["collate_samples/" + name.split("/", 1)[1]]
        for key in ("keep", "padded_width", "text_seq", "text_len", "image_width"):
            assert a[key] == b[key], (name, key)
        assert a["image"] == b["image"], name  # (with no sample left collate_samples falls back to height 64, which is the plan's here)


def test_each_module_can_be_imported_first():
    for mod in MODULES:
        r = subprocess.run([sys.executable, "-c", f"import ocrs_models_amd.{mod}"], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mod, r.stderr[-2000:])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in sorted(answers().items())) + "\n}")

"""The detection datasets without a GPU (ocrs_models_amd/datasets/ HierText / DDI100 / DevicePageLoader, train_detection.main): the shrink
rule's known answers on the host restatement the kernel mirrors (tests/detdata_ref.py), PIL's conversion of float vertices, the dataset
files and selection rules, and the command line.  The shrink tests run on the restatement alone: they pin, by answers derivable by hand,
the rule that tests/test_detdata_gpu.py holds the kernel to, case by case."""
from __future__ import annotations

import gzip
import json
import math
import os
import pickle
import time

import numpy as np
import pytest
import torch
from PIL import Image
from torch.utils.data import DataLoader

from ocrs_models_amd import train_detection
from ocrs_models_amd.datasets import DDI100, DDI100Unpickler, DevicePageLoader, HierText
from tests import detdata_ref as ref

assert callable(train_detection.main)  # the feature's names: without it this module does not import
CPU = "cpu"  # host-side construction: nothing is uploaded, _tensors() refuses


# ---- the shrink rule ---------------------------------------------------------------------------------------------------------------
def test_rectangle_shrinks_to_exact_integers_in_both_orientations():
    rect = [(10, 10), (40, 10), (40, 30), (10, 30)]
    assert ref.shrink_polygon(rect, 3.0) == [(13.0, 13.0), (37.0, 13.0), (37.0, 27.0), (13.0, 27.0)]
    assert ref.shrink_polygon(rect[::-1], 3.0) == [(13.0, 27.0), (37.0, 27.0), (37.0, 13.0), (13.0, 13.0)]


@pytest.mark.parametrize("height", [1, 3, 5, 6])
def test_thin_rectangle_is_empty(height):
    assert ref.shrink_polygon([(0, 0), (50, 0), (50, height), (0, height)], 3.0) == []
    assert ref.shrink_polygon([(0, 0), (height, 0), (height, 50), (0, 50)][::-1], 3.0) == []


def test_seven_pixels_survive():
    assert ref.shrink_polygon([(0, 0), (50, 0), (50, 7), (0, 7)], 3.0) == [(3.0, 3.0), (47.0, 3.0), (47.0, 4.0), (3.0, 4.0)]


def test_rotated_square_shrinks_about_its_centre():
    sq = [(50, 20), (80, 50), (50, 80), (20, 50)]
    d = 3.0 * math.sqrt(2.0)
    want = [(50, 20 + d), (80 - d, 50), (50, 80 - d), (20 + d, 50)]
    for got in (ref.shrink_polygon(sq, 3.0), ref.shrink_polygon(sq[::-1], 3.0)[::-1]):
        assert len(got) == 4
        for (gx, gy), (wx, wy) in zip(got, want):
            assert abs(gx - wx) < 1e-12 and abs(gy - wy) < 1e-12


def test_l_shape_reflex_corner_moves_diagonally():
    ell = [(0, 0), (60, 0), (60, 20), (20, 20), (20, 50), (0, 50)]
    assert ref.shrink_polygon(ell, 3.0) == [(3.0, 3.0), (57.0, 3.0), (57.0, 17.0), (17.0, 17.0), (17.0, 47.0), (3.0, 47.0)]  # (20, 20) -> (17, 17)


def test_needle_reflex_vertex_is_bevelled():
    needle = [(0, 0), (100, 0), (100, 60), (52, 60), (50, 8), (48, 60), (0, 60)]
    got = ref.shrink_polygon(needle, 3.0)
    assert len(got) == 8
    a, b = got[4], got[5]  # the two bevel points of (50, 8): the vertex moved by 3 along each neighbour's normal
    for p in (a, b):
        assert abs(math.hypot(p[0] - 50, p[1] - 8) - 3.0) < 1e-12
    length = math.hypot(2, 52)
    assert abs(a[0] - (50 + 3 * 52 / length)) < 1e-12 and abs(a[1] - (8 - 3 * 2 / length)) < 1e-12
    assert abs(b[0] - (50 - 3 * 52 / length)) < 1e-12 and abs(b[1] - (8 - 3 * 2 / length)) < 1e-12
    # below the limit the corner keeps its mitre: one point, on the bisector
    blunt = ref.shrink_polygon([(0, 0), (100, 0), (100, 60), (70, 60), (50, 40), (30, 60), (0, 60)], 3.0)
    assert len(blunt) == 7 and abs(blunt[4][0] - 50) < 1e-12 and abs(blunt[4][1] - (40 - 3 * math.sqrt(2.0))) < 1e-12


def test_closing_vertex_and_duplicates_change_nothing():
    q = [(10, 10), (70, 14), (78, 40), (18, 36)]
    want = ref.shrink_polygon(q, 3.0)
    assert len(want) == 4
    assert ref.shrink_polygon(q + [q[0]], 3.0) == want
    assert ref.shrink_polygon([q[0], q[0], q[1], q[2], q[2], q[2], q[3], q[0]], 3.0) == want


def test_degenerate_rings_are_skipped():
    assert ref.shrink_polygon([(0, 0), (10, 10), (20, 20)], 3.0) == []  # zero area
    assert ref.shrink_polygon([(0, 0), (9, 9)], 3.0) == []
    assert ref.shrink_polygon([(0, 0), (40, 0), (40, 20), (20, 20), (20, 40), (20, 20), (0, 20)], 3.0) == []  # anti-parallel neighbours
    assert ref.shrink_polygon([(3, 4), (9, 9)], 0.0) == [(3.0, 4.0), (9.0, 9.0)]  # dist 0 bypasses the rule


def test_pil_truncates_float_vertices():
    """The conversion the kernel's (int) restates: PIL fed floats fills what it fills for the coordinates truncated towards zero."""
    from tests.hiertext_ref import pil_mask

    for poly in ([(2.6, 1.6), (9.4, 1.6), (9.4, 5.4), (2.6, 5.4)], [(-0.7, -0.9), (8.9, 0.2), (7.99, 6.5), (0.3, 5.999)],
                 ref.shrink_polygon([(10, 10), (70, 14), (78, 40), (18, 36)], 3.0)):
        im = Image.new("1", (90, 50), 0)
        from PIL import ImageDraw

        ImageDraw.Draw(im).polygon(poly, fill="white", outline=None)
        assert np.array_equal(np.array(im, dtype=np.uint8), pil_mask(90, 50, [(int(x), int(y)) for x, y in poly]))


def test_shrink_cases_meet_the_truncation_condition():
    """What the device test assumes of its inputs: every reference coordinate is a whole number or at least 1e-6 away from one."""
    for name, poly in ref.shrink_cases():
        for p in ref.shrink_polygon(poly, 3.0):
            for c in p:
                assert c == round(c) or abs(c - round(c)) >= 1e-6, (name, c)


# ---- datasets ----------------------------------------------------------------------------------------------------------------------
def test_hiertext_jsonl_words_and_max_images(tmp_path, capsys):
    root = str(tmp_path)
    want = ref.write_hiertext_tree(root, "train")
    ds = HierText(root, device=CPU)
    assert "Converting annotations from JSON to JSONL format..." in capsys.readouterr().out
    lines_file = f"{root}/gt/train.jsonl"
    with gzip.open(f"{root}/gt/train.jsonl.gz") as f:
        anns = json.load(f)["annotations"]
    assert open(lines_file).read() == "".join(json.dumps(a) + "\n" for a in anns)  # the reference's file, line by line
    assert len(ds) == len(want) == 5 and ds.paths == [f"{root}/train/{pid}.jpg" for pid, _ in want]
    assert ds.sizes == [(h, w) for w, h in ref.HIERTEXT_PAGES.values()]
    assert ds.poly_counts == [len(words) for _, words in want]
    verts = ds._host[3].tolist()
    assert verts == [list(v) for _, words in want for q in words for v in q]  # paragraphs -> lines -> words
    # the mtime rule: an up-to-date lines file is read as it is, an older one is rewritten
    with open(lines_file, "w") as f:
        f.write(json.dumps(anns[1]) + "\n")
    assert HierText(root, device=CPU).paths == [f"{root}/train/page_b.jpg"]
    old = time.time() - 100
    os.utime(lines_file, (old, old))
    assert len(HierText(root, device=CPU)) == 5
    assert len(HierText(root, max_images=2, device=CPU)) == 2 and HierText(root, max_images=2, device=CPU).paths == ds.paths[:2]
    with pytest.raises(Exception, match="not found"):
        HierText(root, train=False, device=CPU)


def test_transform_is_refused(tmp_path):
    for cls in (HierText, DDI100):
        with pytest.raises(TypeError, match="augment=True/False"):
            cls(str(tmp_path), transform=lambda x: x)
        with pytest.raises(TypeError, match="augment=True/False"):
            cls(str(tmp_path), augment=lambda x: x)


def test_ddi_split_unpickler_and_channels(tmp_path):
    root = str(tmp_path)
    want = ref.write_ddi_tree(root)
    names = [n for n, _ in want]
    train, val = DDI100(root, device=CPU), DDI100(root, train=False, device=CPU)
    assert train.paths == [f"{root}/gen_imgs/{n}" for n in names[:18]] and val.paths == [f"{root}/gen_imgs/{n}" for n in names[18:]]
    # max_images first, then the 90/10 split
    assert DDI100(root, max_images=10, device=CPU).paths == train.paths[:9]
    assert DDI100(root, max_images=10, train=False, device=CPU).paths == train.paths[9:10]
    assert train.sizes == [(h, w) for _, (w, h) in ref.DDI_PAGES[:18]]
    assert train._host[3].tolist() == [list(v) for _, quads in want[:18] for q in quads for v in q]  # w["box"] as it is
    # a foreign class in a pickle
    with open(f"{root}/gen_boxes/000.pickle", "wb") as f:
        pickle.dump([{"box": complex(1, 2)}, os.path.join], f)
    with pytest.raises(pickle.UnpicklingError, match="Disallowed class"):
        DDI100(root, device=CPU)
    import io

    with pytest.raises(pickle.UnpicklingError, match="Disallowed class collections.OrderedDict"):
        DDI100Unpickler(io.BytesIO(pickle.dumps(__import__("collections").OrderedDict(a=1)))).load()
    assert DDI100Unpickler(io.BytesIO(pickle.dumps([{"box": np.arange(8).reshape(4, 2)}]))).load()[0]["box"].tolist()[3] == [6, 7]
    ref.write_ddi_tree(root)
    # a multi-channel page
    Image.fromarray(np.zeros((40, 50, 3), np.uint8), "RGB").save(f"{root}/gen_imgs/003.png")
    with pytest.raises(RuntimeError, match="one channel.*3"):
        DDI100(root, device=CPU)


def test_store_limits_and_no_cpu_path():
    page = np.zeros((30, 40), np.uint8)
    with pytest.raises(RuntimeError, match="512"):
        HierText.from_pages([page], [[[(0, k) for k in range(513)]]], device=CPU)
    assert HierText.from_pages([page], [[[(0, k) for k in range(512)]]], device=CPU).skipped is None  # (known once on the device)
    with pytest.raises(RuntimeError, match="65535"):
        HierText.from_pages([page], [[[(0, 0), (70000, 0), (70000, 9)]]], device=CPU)
    with pytest.raises(RuntimeError, match="whole numbers"):
        HierText.from_pages([page], [[[(0.5, 0), (20, 0), (20, 9)]]], device=CPU)
    with pytest.raises(RuntimeError, match="uint8"):
        HierText.from_pages([page.astype(np.float32)], [[]], device=CPU)
    ds = HierText.from_pages([page], [[[(2, 2), (30, 2), (30, 20), (2, 20)]]], device=CPU)
    assert len(ds) == 1 and ds.mask_size == (800, 600)
    with pytest.raises(RuntimeError, match=r"runs on MI355X only \(no CPU path\)"):
        ds._tensors()


def test_loader_order_is_dataloaders():
    pages = [np.zeros((20 + k, 30), np.uint8) for k in range(11)]
    ds = HierText.from_pages(pages, [[] for _ in pages], device=CPU)
    stock = DataLoader(list(range(11)), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(5))
    loader = DevicePageLoader(ds, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert len(loader) == len(stock) == 3
    assert list(loader.plan()) == [[int(i) for i in b] for b in stock]
    assert list(DevicePageLoader(ds, batch_size=4).plan()) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
    torch.manual_seed(7)  # the global generator, as the training script uses it
    a = list(DevicePageLoader(ds, batch_size=3, shuffle=True).plan())
    torch.manual_seed(7)
    assert a == [[int(i) for i in b] for b in DataLoader(list(range(11)), batch_size=3, shuffle=True)]


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_main_arguments(capsys):
    with pytest.raises(SystemExit) as e:
        train_detection.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--batch-size", "--checkpoint", "--debug-images", "--export", "--max-epochs", "--max-images", "--validate-only", "--augment, --no-augment",
                 "{ddi,hiertext}"):
        assert flag in out, flag
    for argv, msg in ((["coco", "x"], "invalid choice: 'coco'"), (["hiertext"], "the following arguments are required: data_dir"),
                      (["ddi", "x", "--batch-size", "four"], "invalid int value"), (["ddi", "x", "--bf16"], "unrecognized arguments")):
        with pytest.raises(SystemExit) as e:
            train_detection.main(argv)
        assert e.value.code == 2 and msg in capsys.readouterr().err, argv
    assert callable(train_detection.prepare_loaders)

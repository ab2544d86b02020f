"""CPU-only checks of the recognition dataset's host side (ocrs_models_amd/datasets/hiertext.py): the line-annotation filter against a hand-written
lines file, the regeneration rule, and the pin of tests/hiertext_ref.polygon_mask -- the restatement csrc/line_data.hip was ported from --
to the installed PIL on the polygon families the GPU test uses."""
from __future__ import annotations

import gzip
import json
import os

import numpy as np

from tests import hiertext_ref as ref


def _box(x0, y0, x1, y1):
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def _line(vertices, text, legible=True, vertical=False, words=None):
    return {"vertices": vertices, "text": text, "legible": legible, "vertical": vertical, "handwritten": False,
            "words": [{"vertices": w} for w in (words or [vertices])]}


def test_annotation_filter_writes_the_reference_lines_file(tmp_path, capsys):
    from ocrs_models_amd.datasets import generate_text_line_annotations

    lines = [
        _line(_box(0, 0, 50, 20), "good one"),
        _line(_box(0, 0, 50, 20), "illegible", legible=False),
        _line(_box(0, 0, 50, 20), "vertical", vertical=True),
        _line(_box(0, 0, 9, 9), "small"),                                   # 9 x 9 (aspect 1.0)
        _line(_box(0, 0, 10, 10), "exactly 10 x 10, aspect exactly 1"),     # both thresholds met exactly
        _line(_box(0, 0, 100, 10), "words cover 0.79", words=[_box(0, 0, 79, 10)]),
        _line(_box(0, 0, 100, 10), "words cover exactly 0.8", words=[_box(0, 0, 40, 10), _box(30, 0, 80, 10)]),
        _line(_box(0, 0, 20, 21), "aspect below 1"),
        _line([[3, 4], [60, 2], [61, 30], [2, 28]], "quad € \"quoted\""),
    ]
    anns = [{"image_id": "img1", "paragraphs": [{"lines": lines[:4]}, {"lines": lines[4:7]}]},
            {"image_id": "img2", "paragraphs": [{"lines": lines[7:]}]}]
    src, dst = tmp_path / "train.jsonl.gz", tmp_path / "train-lines.jsonl"
    with gzip.open(src, "wt") as f:
        json.dump({"annotations": anns}, f)
    generate_text_line_annotations(str(src), str(dst))
    expected = (
        '{"image_id": "img1", "vertices": [[0, 0], [50, 0], [50, 20], [0, 20]], "text": "good one"}\n'
        '{"image_id": "img1", "vertices": [[0, 0], [10, 0], [10, 10], [0, 10]], "text": "exactly 10 x 10, aspect exactly 1"}\n'
        '{"image_id": "img1", "vertices": [[0, 0], [100, 0], [100, 10], [0, 10]], "text": "words cover exactly 0.8"}\n'
        '{"image_id": "img2", "vertices": [[3, 4], [60, 2], [61, 30], [2, 28]], "text": "quad \\u20ac \\"quoted\\""}\n'
    )
    assert dst.read_bytes() == expected.encode()
    out = capsys.readouterr().out.splitlines()
    assert out == [
        f"Extracting text line annotations from {src}",
        "Total lines: 9 (100.0%)",
        "Total usable for training: 4 (44.4%)",
        "Legible: 8 (88.9%)",
        "Horizontal: 8 (88.9%)",
        "Aspect ratio (width/height) >= 1.0: 8 (88.9%)",
        "Width >= 10 and Height >= 10: 8 (88.9%)",
        "Words/line area ratio >= 0.8: 8 (88.9%)",
    ]
    # a lines file at least as new as the annotations is left alone (whoever wrote it) ...
    dst.write_text("kept\n")
    os.utime(dst, (os.path.getmtime(src) + 5, os.path.getmtime(src) + 5))
    generate_text_line_annotations(str(src), str(dst))
    assert dst.read_text() == "kept\n"
    # ... an older one is regenerated
    os.utime(dst, (os.path.getmtime(src) - 5, os.path.getmtime(src) - 5))
    generate_text_line_annotations(str(src), str(dst))
    assert dst.read_bytes() == expected.encode()


def test_polygon_restatement_equals_pil():
    cases = ref.all_polygon_cases()  # four seeds
    assert len(cases) >= 300 and {(1, 1), (1, 40), (40, 1), (67, 13), (300, 41), (801, 23)} <= {(w, h) for _, w, h, _ in cases}
    bad = [(fam, w, h, p) for fam, w, h, p in cases if not np.array_equal(ref.polygon_mask(w, h, p), ref.pil_mask(w, h, p))]
    assert not bad, bad[:3]


def test_dataset_refuses_a_transform_and_needs_a_gpu(tmp_path):
    import pytest

    from ocrs_models_amd.datasets import HierTextRecognition

    ref.write_tree(str(tmp_path))
    with pytest.raises(TypeError, match="inside the batch kernels"):
        HierTextRecognition(str(tmp_path), transform=lambda x: x)
    ds = HierTextRecognition(str(tmp_path), device="cpu")  # (a CPU test: nothing is uploaded)
    kept = [k for k in ref.tree_lines() if k[2]]
    assert len(ds) == len(kept) and ds.image_ids == [k[0] for k in kept]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ds[0]

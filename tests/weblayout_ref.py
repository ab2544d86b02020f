"""CPU restatement of the WebLayout item rule (ocrs_models/datasets/web_layout.py:16-186), for the tests and tools/layout_data_time.py only:
written from the rule's description, pinned to the reference's recorded outputs (tests/golden/weblayout.npz) by tests/test_weblayout_host.py.
Plain Python floats (IEEE fp64), one rounding to fp32 at the end, like the reference."""
from __future__ import annotations

import json
import os

import torch
from torch.utils.data import Dataset


def overlap(a, b, c, d):
    """the asymmetric interval rule: touching intervals do not overlap"""
    return b > c if a <= c else d > a


def item(path, normalize=True, padded_size=None, jitter=(0.0, 0.0)):
    """(boxes (W, 4), labels (W, 2)) fp32 of one page file: W = padded_size or the page's word count."""
    with open(path) as f:
        content = json.load(f)
    vw, vh = int(content["resolution"]["width"]), int(content["resolution"]["height"])
    jx, jy = jitter

    def tx(c):
        c = c * 1.0 + jx
        return c / vw - 0.5 if normalize else c

    def ty(c):
        c = c * 1.0 + jy
        return c / vh - 0.5 if normalize else c

    boxes, labels = [], []
    for para in content["paragraphs"]:
        rows = [[tx(w["coords"][0]), ty(w["coords"][1]), tx(w["coords"][2]), ty(w["coords"][3])] for w in para["words"]]
        for i, (left, top, right, bottom) in enumerate(rows):
            start = i == 0 or not overlap(rows[i - 1][1], rows[i - 1][3], top, bottom)
            end = i == len(rows) - 1 or not overlap(top, bottom, rows[i + 1][1], rows[i + 1][3])
            boxes.append([left, top, right, bottom])
            labels.append([float(start), float(end)])
    boxes = torch.tensor(boxes, dtype=torch.float64).to(torch.float32)  # the one rounding, to nearest even
    labels = torch.tensor(labels, dtype=torch.float32)
    if padded_size:
        out_b, out_l = torch.zeros(padded_size, 4), torch.zeros(padded_size, 2)
        n = min(padded_size, boxes.shape[0])
        out_b[:n], out_l[:n] = boxes[:n], labels[:n]  # truncation after labelling
        boxes, labels = out_b, out_l
    return boxes, labels


def select_files(root_dir, train=True, max_images=None, filter=None):
    files = [f for f in os.listdir(root_dir) if os.path.isfile(os.path.join(root_dir, f)) and f.endswith(".json")]
    split = round(len(files) * 4 / 5)
    files = files[:split] if train else files[split:]
    if max_images is not None:
        files = files[:max_images]
    if filter:
        files = [f for f in files if filter(f)]
    return files


class RefWebLayout(Dataset):
    """the dataset on the CPU, with the reference's constructor and its random draws (three numbers per item, the third unused)"""

    def __init__(self, root_dir, randomize=False, padded_size=None, train=True, max_images=None, filter=None, normalize_coords=True, max_jitter=25):
        self.root_dir, self.randomize, self.padded_size = root_dir, randomize, padded_size
        self.normalize_coords, self.max_jitter = normalize_coords, max_jitter
        self.files = select_files(root_dir, train, max_images, filter)

    def __len__(self):
        return len(self.files)

    def draw(self):
        if not self.randomize:
            return 0.0, 0.0
        a, b, c = torch.rand(3).tolist()
        return a * self.max_jitter, b * self.max_jitter

    def __getitem__(self, idx):
        return item(os.path.join(self.root_dir, self.files[idx]), self.normalize_coords, self.padded_size, self.draw())


PAGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weblayout")


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weblayout.npz")


def golden_cases():
    """(key, file name, normalize, padded_size, seed or None, max_jitter or None) of every item recorded from the reference
    (tools/gen_weblayout_goldens.py: an entry is the item's input (W, 4) next to its labels (W, 2))"""
    import numpy as np

    out = []
    for key in np.load(GOLDEN).files:
        name, n, p, mode = key.split("|")
        seed, jitter = (None, None) if mode == "fixed" else tuple(int(v) for v in mode[1:].split("j"))
        out.append((key, name, n == "n1", None if p == "pNone" else int(p[1:]), seed, jitter))
    return out


def copy_pages(dst, extra=3):
    """The fixture pages plus ``extra`` renamed copies in ``dst``: 15 files = 12 train (two batches of 5 and a short one) + 3 validation."""
    import shutil

    names = sorted(f for f in os.listdir(PAGES) if f.endswith(".json"))
    for f in names:
        shutil.copy(os.path.join(PAGES, f), os.path.join(dst, f))
    for f in names[:extra]:
        shutil.copy(os.path.join(PAGES, f), os.path.join(dst, "copy_of_" + f))
    return str(dst)

"""The layout model's dataset (ocrs_models/datasets/web_layout.py), resident on the device.

``WebLayout`` keeps the reference's constructor and file-selection rules, but parses every selected JSON file ONCE, at construction, into four
device tensors (a whole training set is a few megabytes of coordinates).  An item or a batch is then one launch of ``ocrs_weblayout_batch``
(csrc/layout_data.hip): jitter, normalisation, the single fp64 -> fp32 rounding of ``torch.Tensor(words)``, the line_start / line_end labels
and the zero padding, bit-identical to the reference's ``__getitem__`` + ``default_collate``.

``DeviceWebLayoutLoader`` stands where ``DataLoader(WebLayout(...), batch_size, shuffle)`` stands in train_layout.py:233-244.  The random
stream (the sampler's permutation and the three ``torch.rand`` numbers per item) is consumed by a stock ``DataLoader`` over a host-side index
dataset, so it is the reference's by construction; what crosses PCIe per batch is N indices and N jitter pairs.
"""
from __future__ import annotations

import json
import os
from typing import Callable, Optional

import torch
from torch.utils.data import DataLoader, Dataset

from .._lib import lib, ptr
from .util import DeviceStore


def select_files(root_dir: str, train=True, max_images: Optional[int] = None, filter: Optional[Callable[[str], bool]] = None) -> list:
    """web_layout.py:55-71: ``os.listdir`` order, the first round(4/5) of the .json files train, the rest validation; then max_images, then filter."""
    files = [f for f in os.listdir(root_dir) if os.path.isfile(os.path.join(root_dir, f)) and f.endswith(".json")]
    train_split = round(len(files) * 4 / 5)
    files = files[:train_split] if train else files[train_split:]
    if max_images is not None:
        files = files[:max_images]
    if filter:
        files = [f for f in files if filter(f)]
    return files


def parse_page(path: str):
    """One WebLayout file -> (coords [[left, top, right, bottom], ...], paragraph index per word, (int(width), int(height))) in the
    reference's paragraph -> word order (web_layout.py:102-105, 134-139).  ValueError for what the reference fails on per item."""
    with open(path) as file:
        content = json.load(file)
    viewport = (int(content["resolution"]["width"]), int(content["resolution"]["height"]))
    coords, para = [], []
    for pi, p in enumerate(content["paragraphs"]):
        for word in p["words"]:
            left, top, right, bottom = (float(c) for c in word["coords"])
            if not (left >= 0 and right >= 0 and top >= 0 and bottom >= 0):  # web_layout.py:122 (jitter is >= 0: the raw values decide)
                raise ValueError(f"{path}: negative word coordinate {word['coords']}")
            coords.append([left, top, right, bottom])
            para.append(pi)
    if not coords:  # (the reference fails on it inside F.pad)
        raise ValueError(f"{path}: page has no words")
    return coords, para, viewport


class WebLayout(DeviceStore):
    """Layout analysis dataset produced from rendering web pages: the reference's ``WebLayout`` (web_layout.py:11-186, same arguments)
    with the parsed pages in device memory.  ``__getitem__`` returns ``(word boxes (W, 4), labels (W, 2))`` fp32 DEVICE tensors, labels =
    [line_start, line_end]; W = ``padded_size`` or the page's own word count.  The store (``_tensors()``): coords (T, 4) fp64 | para (T,)
    int32 | page_off (P + 1,) int64 | viewport (P, 2) fp64."""

    _keep_host = True  # (a few megabytes of coordinates, which the tests read)

    def __init__(self, root_dir: str, randomize=False, padded_size: Optional[int] = None, train=True, max_images: Optional[int] = None,
                 filter: Optional[Callable[[str], bool]] = None, normalize_coords=True, max_jitter: int = 25, device="cuda"):
        super().__init__()
        self.max_jitter = max_jitter
        self.normalize_coords = normalize_coords
        self.randomize = randomize
        self.root_dir = root_dir
        self.padded_size = padded_size
        self.device = torch.device(device)
        self._files = select_files(root_dir, train, max_images, filter)
        coords, para, offs, viewports = [], [], [0], []
        for f in self._files:
            c, p, v = parse_page(os.path.join(root_dir, f))
            coords += c
            para += p
            offs.append(len(coords))
            viewports.append(v)
        self.counts = [b - a for a, b in zip(offs, offs[1:])]  # words per page (host: sizes an unpadded item without a device read)
        self._set_host((torch.tensor(coords, dtype=torch.float64).reshape(-1, 4), torch.tensor(para, dtype=torch.int32),
                        torch.tensor(offs, dtype=torch.int64), torch.tensor(viewports, dtype=torch.float64).reshape(-1, 2)), bool(self._files))

    def __len__(self):
        return len(self._files)

    def draw_jitter(self) -> tuple[float, float]:
        """web_layout.py:92-100: three numbers from torch's CPU generator (the third, once a scale, is unused), two Python-float products."""
        if not self.randomize:
            return 0.0, 0.0
        a, b, c = torch.rand(3).tolist()
        return a * self.max_jitter, b * self.max_jitter

    def batch(self, pages, jitter_x, jitter_y, width: Optional[int] = None):
        """``pages`` (N,) page indices with their jitters (host tensors or sequences) -> boxes (N, W, 4), labels (N, W, 2) on the device: one
        pinned upload, one launch, no synchronisation."""
        coords, para, page_off, viewport = self._tensors()
        pages = torch.as_tensor(pages, dtype=torch.int32).reshape(-1)
        n = pages.numel()
        if n < 1 or int(pages.min()) < 0 or int(pages.max()) >= len(self):
            raise IndexError(f"page indices must be in 0 .. {len(self) - 1}")
        W = width or self.padded_size
        if not W:
            sizes = {self.counts[i] for i in pages.tolist()}
            if len(sizes) != 1:
                raise RuntimeError(f"pages of {sorted(sizes)} words cannot be stacked: set padded_size (default_collate fails the same way)")
            W = sizes.pop()
        # one host record: N jitter pairs (fp64) then N page indices (int32).  Fresh pinned memory per batch (torch's caching host allocator
        # keeps a block until the copy that reads it has run), so a batch queued behind the device is never rewritten.
        rec = torch.empty(20 * n, dtype=torch.uint8, pin_memory=True)
        jit = rec[:16 * n].view(torch.float64).view(n, 2)
        jit[:, 0] = torch.as_tensor(jitter_x, dtype=torch.float64)
        jit[:, 1] = torch.as_tensor(jitter_y, dtype=torch.float64)
        rec[16 * n:].view(torch.int32).copy_(pages)
        drec = rec.to(self.device, non_blocking=True)
        boxes = torch.empty(n, W, 4, dtype=torch.float32, device=self.device)
        labels = torch.empty(n, W, 2, dtype=torch.float32, device=self.device)
        lib().weblayout_batch(ptr(coords), ptr(para), ptr(page_off), ptr(viewport), len(self), drec.data_ptr() + 16 * n, ptr(drec), n, W,
                              1 if self.normalize_coords else 0, ptr(boxes), ptr(labels))
        return boxes, labels

    def __getitem__(self, idx: int):
        idx = range(len(self))[idx]
        jx, jy = self.draw_jitter()
        boxes, labels = self.batch([idx], [jx], [jy], self.padded_size or self.counts[idx])
        return boxes[0], labels[0]


class _Plan(Dataset):
    """What an item costs the host: its index and its jitter draw, in the order ``WebLayout.__getitem__`` would make it."""

    def __init__(self, dataset: WebLayout):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        jx, jy = self.dataset.draw_jitter()
        return i, jx, jy


class DeviceWebLayoutLoader:
    """Iterable of ``(boxes (N, W, 4), labels (N, W, 2))`` device batches.  For a given ``torch.manual_seed`` these are the batches of
    ``DataLoader(<the reference's WebLayout>, batch_size=batch_size, shuffle=shuffle)`` with num_workers=0, the shorter last one included."""

    def __init__(self, dataset: WebLayout, batch_size: int, shuffle=False):
        self.dataset = dataset
        self.batch_size = batch_size
        self._loader = DataLoader(_Plan(dataset), batch_size=batch_size, shuffle=shuffle)

    def __len__(self):
        return len(self._loader)

    def plan(self):
        """One epoch's ``(page indices int64 (N,), jitter_x fp64 (N,), jitter_y fp64 (N,))`` host tensors per batch; touches no GPU."""
        return iter(self._loader)

    def __iter__(self):
        for pages, jx, jy in self.plan():
            yield self.dataset.batch(pages, jx, jy)

"""What the device-resident datasets share: image decoding, the bounding-box and polygon rules (ocrs_models/datasets/util.py), the
protocol of a store whose tensors live in device memory, and the loader that feeds a store one index batch at a time."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

MAX_POLYGON_VERTICES = 512  # csrc/poly_fill.h's kMaxVerts
SHRINK_DISTANCE = 3.0  # datasets/util.py:18


def bounding_box_size(vertices) -> tuple[int, int]:
    """datasets/util.py:184-194"""
    xs, ys = [v[0] for v in vertices], [v[1] for v in vertices]
    return (max(xs) - min(xs), max(ys) - min(ys))


def line_bounding_box(vertices) -> tuple[int, int, int, int]:
    """(min_x, min_y, max_x, max_y) of hiertext.py:248-253"""
    xs, ys = [v[0] for v in vertices], [v[1] for v in vertices]
    min_x = max(0, min(xs))
    max_x = max(min_x, max(xs))
    min_y = max(0, min(ys))
    max_y = max(min_y, max(ys))
    return min_x, min_y, max_x, max_y


def whole_polygon(poly, what: str) -> list:
    pts = [tuple(c) for c in (poly.tolist() if hasattr(poly, "tolist") else poly)]
    if any(len(c) < 2 or int(c[0]) != c[0] or int(c[1]) != c[1] for c in pts):
        raise RuntimeError(f"{what}: vertex coordinates must be whole numbers (the shrink kernel takes them as integers)")
    pts = [(int(c[0]), int(c[1])) for c in pts]
    if len(pts) > MAX_POLYGON_VERTICES or any(abs(c) > 65535 for v in pts for c in v):
        raise RuntimeError(f"{what}: polygons of at most {MAX_POLYGON_VERTICES} vertices with coordinates within +-65535 are supported, "
                           f"this one has {len(pts)}")
    return pts


def read_gray(path: str) -> np.ndarray:
    """(H, W) uint8.  A JPEG is decoded to libjpeg's own luma (``draft("L")``), as torchvision's ImageReadMode.GRAY asks libjpeg for."""
    from PIL import Image

    with Image.open(path) as im:
        if im.format == "JPEG":
            im.draft("L", im.size)
        return np.array(im.convert("L"), dtype=np.uint8)


def decode_pages(paths: list, read=read_gray) -> list:
    """``read`` over ``paths`` on a pool of threads, in order."""
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        return list(pool.map(read, paths))


class DeviceStore(Dataset):
    """A dataset whose samples live in device memory.  A subclass sets ``device`` and hands ``_set_host`` a tuple of host tensors (None: an
    empty store); ``_tensors()`` gives their device form, made at the first call by ``_upload`` (a plain copy unless overridden), after
    which the host copy is dropped unless ``_keep_host``."""

    _keep_host = False

    def _set_host(self, host, upload_now: bool):
        self._host, self._dev = host, None
        if upload_now and host is not None and torch.cuda.is_available():
            self._tensors()

    def _upload(self, host) -> tuple:
        return tuple(t.to(self.device) for t in host)

    def _tensors(self) -> tuple:
        if self._dev is None:
            name = type(self).__name__
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise RuntimeError(f"ocrs_models_amd.datasets.{name} runs on MI355X only (no CPU path)")
            if self._host is None:
                raise RuntimeError(f"ocrs_models_amd.datasets.{name}: the store is empty")
            self._dev = self._upload(self._host)
            if not self._keep_host:
                self._host = None  # nothing per pixel stays on the host
        return self._dev


class IndexLoader:
    """Iterable of ``dataset.batch(indices, **kwargs)``.  A stock ``DataLoader`` over ``range(len(dataset))`` consumes the sampler's random
    stream, so the order is torch's by construction; a store's augmentation draws follow in batch order."""

    def __init__(self, dataset, batch_size: int = 1, shuffle=False, generator=None, batch_sampler=None, **kwargs):
        self.dataset, self.kwargs = dataset, kwargs
        how = {"batch_sampler": batch_sampler} if batch_sampler is not None else {"batch_size": batch_size, "shuffle": shuffle, "generator": generator}
        self._loader = DataLoader(range(len(dataset)), collate_fn=lambda items: [int(i) for i in items], **how)

    def __len__(self):
        return len(self._loader)

    def plan(self):
        """One epoch's lists of indices, one per batch; touches no GPU."""
        return iter(self._loader)

    def __iter__(self):
        for indices in self.plan():
            yield self.dataset.batch(indices, **self.kwargs)

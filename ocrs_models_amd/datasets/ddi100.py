"""Distorted Document Images (DDI-100) for text detection (ocrs_models/datasets/ddi100.py), resident on the device (the store is pages.py's)."""
from __future__ import annotations

import os
import pickle

import numpy as np

from .pages import PageStore
from .util import decode_pages, read_gray


class DDI100Unpickler(pickle.Unpickler):
    """ddi100.py:11-31: numpy's dtype, ndarray and array reconstructor, nothing else.  (The reconstructor is admitted under the module name
    numpy 2 writes into a pickle as well: it is the same function.)"""

    def find_class(self, module, name):
        path = f"{module}.{name}"
        if path == "numpy.dtype":
            return np.dtype
        if path == "numpy.ndarray":
            return np.ndarray
        if path in ("numpy.core.multiarray._reconstruct", "numpy._core.multiarray._reconstruct"):
            try:
                from numpy._core.multiarray import _reconstruct
            except ImportError:
                from numpy.core.multiarray import _reconstruct
            return _reconstruct
        raise pickle.UnpicklingError(f"Disallowed class {module}.{name}")


def _read_one_channel(path: str) -> np.ndarray:
    from PIL import Image

    with Image.open(path) as im:
        if len(im.getbands()) != 1:
            raise RuntimeError(f"{path}: DDI100 pages must have one channel, this image has {len(im.getbands())} ({im.mode}): convert it to "
                               "greyscale (the reference fails on it when it stacks the image and its mask)")
    return read_gray(path)


class DDI100(PageStore):
    """Distorted Document Images (DDI-100) dataset for text detection: the reference's ``DDI100`` (ddi100.py:34-107; ``gen_imgs/`` and
    ``gen_boxes/*.pickle``, sorted listing, max_images before the 90/10 split) with the pages and word quads resident in device memory.
    The quads are ``w["box"]`` as ``__getitem__`` passes them to generate_mask (ddi100.py:89-93)."""

    def __init__(self, root_dir: str, train=True, augment=False, max_images=None, device="cuda", mask_size=None, transform=None):
        super().__init__()
        self._init_args(augment, device, mask_size, transform)
        self._img_dir = f"{root_dir}/gen_imgs"
        self._boxes_dir = f"{root_dir}/gen_boxes"
        if not os.path.exists(self._img_dir):
            raise Exception(f"Dataset images not found in {self._img_dir}")
        if not os.path.exists(self._boxes_dir):
            raise Exception(f"Dataset masks not found in {self._boxes_dir}")
        self._img_filenames = sorted(os.listdir(self._img_dir))
        if max_images is not None:
            self._img_filenames = self._img_filenames[:max_images]
        train_split_idx = int(len(self._img_filenames) * 0.9)
        self._img_filenames = self._img_filenames[:train_split_idx] if train else self._img_filenames[train_split_idx:]
        paths = [f"{self._img_dir}/{f}" for f in self._img_filenames]
        quads = []
        for f in self._img_filenames:
            with open(f"{self._boxes_dir}/{os.path.splitext(f)[0]}.pickle", "rb") as fp:
                quads.append([w["box"] for w in DDI100Unpickler(fp).load()])
        self._set_store(paths, decode_pages(paths, _read_one_channel), quads)

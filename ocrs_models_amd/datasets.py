"""The device-resident datasets: the layout model's WebLayout and the recognition model's HierTextRecognition (further down).

The layout model's dataset (ocrs_models/datasets/web_layout.py), resident on the device.

``WebLayout`` keeps the reference's constructor and file-selection rules, but parses every selected JSON file ONCE, at construction, into four
device tensors (a whole training set is a few megabytes of coordinates).  An item or a batch is then one launch of ``ocrs_weblayout_batch``
(csrc/layout_data.hip): jitter, normalisation, the single fp64 -> fp32 rounding of ``torch.Tensor(words)``, the line_start / line_end labels
and the zero padding, bit-identical to the reference's ``__getitem__`` + ``default_collate``.

``DeviceWebLayoutLoader`` stands where ``DataLoader(WebLayout(...), batch_size, shuffle)`` stands in train_layout.py:233-244.  The random
stream (the sampler's permutation and the three ``torch.rand`` numbers per item) is consumed by a stock ``DataLoader`` over a host-side index
dataset, so it is the reference's by construction; what crosses PCIe per batch is N indices and N jitter pairs.
"""
from __future__ import annotations

import gzip
import json
import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from ._lib import lib, ptr
from .input_pipeline import line_output_width


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


class WebLayout(Dataset):
    """Layout analysis dataset produced from rendering web pages: the reference's ``WebLayout`` (web_layout.py:11-186, same arguments)
    with the parsed pages in device memory.  ``__getitem__`` returns ``(word boxes (W, 4), labels (W, 2))`` fp32 DEVICE tensors, labels =
    [line_start, line_end]; W = ``padded_size`` or the page's own word count."""

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
        self._host = (torch.tensor(coords, dtype=torch.float64).reshape(-1, 4), torch.tensor(para, dtype=torch.int32),
                      torch.tensor(offs, dtype=torch.int64), torch.tensor(viewports, dtype=torch.float64).reshape(-1, 2))
        self._dev = None
        if self._files and torch.cuda.is_available():
            self._tensors()

    def _tensors(self):
        """coords (T, 4) fp64 | para (T,) int32 | page_off (P + 1,) int64 | viewport (P, 2) fp64 on the device"""
        if self._dev is None:
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise RuntimeError("ocrs_models_amd.datasets.WebLayout runs on MI355X only (no CPU path)")
            self._dev = tuple(t.to(self.device) for t in self._host)
        return self._dev

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


# ---- recognition: HierText text lines (ocrs_models/datasets/hiertext.py:145-427) ------------------------------------------------------
MAX_LINE_VERTICES = 512  # csrc/line_data.hip's kMaxVerts


def bounding_box_size(vertices) -> tuple[int, int]:
    """datasets/util.py:184-194"""
    xs, ys = [v[0] for v in vertices], [v[1] for v in vertices]
    return (max(xs) - min(xs), max(ys) - min(ys))


def generate_text_line_annotations(annotations_file: str, lines_file: str):
    """``HierTextRecognition._generate_text_line_annotations`` (hiertext.py:306-427): the same rule for regeneration, the same five filters,
    the same JSON object per kept line and the same statistics printout, so the two implementations read each other's lines file."""
    if os.path.exists(lines_file) and (os.path.getmtime(lines_file) >= os.path.getmtime(annotations_file)):
        return
    MIN_WIDTH = 10
    MIN_HEIGHT = 10
    MIN_WORD_TO_LINE_AREA_RATIO = 0.8  # area(union of word boxes) / area(line box): below, the line is probably partly illegible
    MIN_ASPECT_RATIO = 1.0  # width / height of the line box: drops severely rotated lines
    total = total_usable = total_legible = total_horizontal = total_size_ok = total_area_ok = total_aspect_ok = 0
    print(f"Extracting text line annotations from {annotations_file}")
    with gzip.open(annotations_file) as in_fp:
        annotations = json.load(in_fp)["annotations"]
        with open(lines_file, "w") as out_fp:
            for ann in annotations:
                for para in ann["paragraphs"]:
                    for line in para["lines"]:
                        vertices = line["vertices"]
                        width, height = bounding_box_size(vertices)
                        aspect_ratio_ok = width / height >= MIN_ASPECT_RATIO
                        words_width, words_height = bounding_box_size([vertex for word in line["words"] for vertex in word["vertices"]])
                        area_ratio_ok = (words_width * words_height) / (width * height) >= MIN_WORD_TO_LINE_AREA_RATIO
                        legible = line["legible"]
                        horizontal = not line["vertical"]
                        size_ok = width >= MIN_WIDTH and height >= MIN_HEIGHT
                        total += 1
                        total_legible += bool(legible)
                        total_horizontal += bool(horizontal)
                        total_size_ok += bool(size_ok)
                        total_area_ok += bool(area_ratio_ok)
                        total_aspect_ok += bool(aspect_ratio_ok)
                        if not (legible and size_ok and horizontal and area_ratio_ok and aspect_ratio_ok):
                            continue
                        total_usable += 1
                        ann_json = json.dumps({"image_id": ann["image_id"], "vertices": vertices, "text": line["text"]})
                        out_fp.write(f"{ann_json}\n")
    stats = {
        "Total lines": total,
        "Total usable for training": total_usable,
        "Legible": total_legible,
        "Horizontal": total_horizontal,
        f"Aspect ratio (width/height) >= {MIN_ASPECT_RATIO}": total_aspect_ok,
        f"Width >= {MIN_WIDTH} and Height >= {MIN_HEIGHT}": total_size_ok,
        f"Words/line area ratio >= {MIN_WORD_TO_LINE_AREA_RATIO}": total_area_ok,
    }
    for description, value in stats.items():
        percent = round((value / total) * 100, 1)
        print(f"{description}: {value} ({percent}%)")


def line_bounding_box(vertices) -> tuple[int, int, int, int]:
    """(min_x, min_y, max_x, max_y) of hiertext.py:248-253"""
    xs, ys = [v[0] for v in vertices], [v[1] for v in vertices]
    min_x = max(0, min(xs))
    max_x = max(min_x, max(xs))
    min_y = max(0, min(ys))
    max_y = max(min_y, max(ys))
    return min_x, min_y, max_x, max_y


def _read_gray(path: str) -> np.ndarray:
    """(H, W) uint8.  A JPEG is decoded to libjpeg's own luma (``draft("L")``), as torchvision's ImageReadMode.GRAY asks libjpeg for."""
    from PIL import Image

    with Image.open(path) as im:
        if im.format == "JPEG":
            im.draft("L", im.size)
        return np.array(im.convert("L"), dtype=np.uint8)


def _page_crops(img_dir: str, cache_dir: str, image_id: str, boxes: list) -> list:
    """The cached crops of one page's boxes (``_get_line_image``, hiertext.py:198-233): read where the cache file exists, otherwise cut from
    the page (decoded once for all of them), written through .tmp + rename.  None for a crop that is empty after clamping."""
    from PIL import Image

    page, out = None, []
    for min_x, min_y, max_x, max_y in boxes:
        cache_path = f"{cache_dir}/{image_id}/{min_x}_{min_y}_{max_x}_{max_y}.png"
        if not os.path.exists(cache_path):
            if page is None:
                page = _read_gray(f"{img_dir}/{image_id}.jpg")
            ph, pw = page.shape
            clamp = lambda v, hi: max(0, min(v, hi))  # noqa: E731
            crop = page[clamp(min_y, ph - 1):clamp(max_y, ph - 1), clamp(min_x, pw - 1):clamp(max_x, pw - 1)]
            if crop.shape[0] == 0 or crop.shape[1] == 0:
                out.append(None)
                continue
            os.makedirs(os.path.dirname(cache_path), exist_ok=True)
            tmp_path = cache_path + ".tmp"
            Image.fromarray(np.ascontiguousarray(crop), "L").save(tmp_path, format="PNG")
            os.rename(tmp_path, cache_path)
        out.append(_read_gray(cache_path))
    return out


def hiertext_text_lines(root_dir: str, train=True, max_images=None):
    """The line selection of ``HierTextRecognition`` (hiertext.py:160-186): the split's lines file, generated from the annotations if it is
    missing, cut to its first ``max_images`` lines -> (image directory, crop cache directory, lines file, its JSON lines).  Reads no image."""
    split = "train" if train else "validation"
    img_dir = f"{root_dir}/{split}"
    annotations_file = f"{root_dir}/gt/{split}.jsonl.gz"
    if not os.path.exists(img_dir):
        raise Exception(f'Image directory "{img_dir}" not found')
    if not os.path.exists(annotations_file):
        raise Exception(f'Label data file "{annotations_file}" not found')
    lines_file = annotations_file.replace(".jsonl.gz", "-lines.jsonl")
    generate_text_line_annotations(annotations_file, lines_file)
    with open(lines_file) as fp:
        text_lines = [line for line in fp]
    if max_images:
        text_lines = text_lines[:max_images]
    return img_dir, f"{root_dir}/{split}-lines-cache", lines_file, text_lines


class HierTextRecognition(Dataset):
    """HierText dataset for text recognition: the reference's ``HierTextRecognition`` (hiertext.py:145-304; same directory layout, lines
    file and crop cache) with every line crop resident in device memory.  ``augment`` stands where the reference takes ``transform``: the
    augmentations run inside the batch kernels (augment.py), so it is a flag.  A line whose crop is empty after clamping to the page is
    dropped at construction with a counted message (the reference fails on such an item)."""

    def __init__(self, root_dir: str, train=True, augment=False, max_images=None, alphabet=None, output_height: int = 64, device="cuda",
                 transform=None):
        super().__init__()
        from .text import DEFAULT_ALPHABET, encode_text

        if transform is not None or callable(augment):
            raise TypeError("HierTextRecognition takes augment=True/False, not a transform: the augmentations of "
                            "text_recognition_data_augmentations() run inside the batch kernels on the device")
        self.alphabet = [c for c in (DEFAULT_ALPHABET if alphabet is None else alphabet)]
        self._img_dir, self._cache_dir, lines_file, text_lines = hiertext_text_lines(root_dir, train, max_images)
        self.augment = bool(augment)
        self.output_height = output_height
        self.device = torch.device(device)

        lines = [json.loads(t) for t in text_lines]
        by_page: dict = {}
        for k, ln in enumerate(lines):
            if any(int(c) != c for v in ln["vertices"] for c in v[:2]):
                raise RuntimeError(f"line {k} of {lines_file} (image {ln['image_id']}): vertex coordinates must be whole numbers "
                                   "(the mask kernel and the cache file names take them as integers)")
            poly = [(int(c[0]), int(c[1])) for c in ln["vertices"]]
            if not 2 <= len(poly) <= MAX_LINE_VERTICES or any(abs(c) > 65535 for v in poly for c in v):
                raise RuntimeError(f"line {k} of {lines_file} (image {ln['image_id']}): polygons of 2 .. {MAX_LINE_VERTICES} vertices with "
                                   f"coordinates within +-65535 are supported, this one has {len(poly)}")
            ln["poly"], ln["box"] = poly, line_bounding_box(poly)
            by_page.setdefault(ln["image_id"], []).append(k)
        crops: list = [None] * len(lines)
        pages = list(by_page.items())
        with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
            for (_, ks), got in zip(pages, pool.map(lambda pg: _page_crops(self._img_dir, self._cache_dir, pg[0], [lines[k]["box"] for k in pg[1]]),
                                                    pages)):
                for k, c in zip(ks, got):
                    crops[k] = c
        keep = [k for k, c in enumerate(crops) if c is not None]
        if len(keep) != len(lines):
            print(f"Dropped {len(lines) - len(keep)} of {len(lines)} lines whose crop is empty after clamping to the page")
        self._set_store([lines[k]["image_id"] for k in keep], [crops[k] for k in keep],
                        [[(x - lines[k]["box"][0], y - lines[k]["box"][1]) for x, y in lines[k]["poly"]] for k in keep],
                        [encode_text(lines[k]["text"], self.alphabet, unknown_char="?") for k in keep])

    @classmethod
    def from_lines(cls, crops, polygons, text_seqs, image_ids=None, augment=False, output_height: int = 64, device="cuda"):
        """A store made from memory instead of a directory (measurement and tests): ``crops`` (h, w) uint8 arrays, ``polygons`` integer
        vertices relative to each crop's origin, ``text_seqs`` encoded int32 tensors."""
        from .text import DEFAULT_ALPHABET

        self = cls.__new__(cls)
        Dataset.__init__(self)
        self.alphabet = [c for c in DEFAULT_ALPHABET]
        self.augment, self.output_height, self.device = bool(augment), output_height, torch.device(device)
        if any(not 2 <= len(p) <= MAX_LINE_VERTICES for p in polygons):
            raise RuntimeError(f"polygons of 2 .. {MAX_LINE_VERTICES} vertices are supported")
        self._set_store(list(image_ids) if image_ids is not None else [str(k) for k in range(len(crops))], [np.ascontiguousarray(c) for c in crops],
                        polygons, list(text_seqs))
        return self

    def _set_store(self, image_ids, crops, polygons, text_seqs):
        self.image_ids, self.text_seqs = image_ids, text_seqs
        self.sizes = [tuple(c.shape) for c in crops]  # (h, w) of every crop
        self.widths = [line_output_width(h, w, self.output_height) for h, w in self.sizes]  # un-augmented item widths, for the samplers
        area = np.array([h * w for h, w in self.sizes], dtype=np.int64)
        counts = np.array([len(p) for p in polygons], dtype=np.int32)
        verts = np.array([v for p in polygons for v in p], dtype=np.int32).reshape(-1, 2)
        self._host = None
        if crops:
            self._host = (torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])), torch.from_numpy(np.cumsum(area) - area),
                          torch.tensor(self.sizes, dtype=torch.int32), torch.from_numpy(verts),
                          torch.from_numpy(np.cumsum(counts, dtype=np.int64) - counts), torch.from_numpy(counts))
        self._dev = None
        if crops and self.device.type == "cuda" and torch.cuda.is_available():
            self._tensors()

    def _tensors(self):
        """pixels uint8 | pixel offsets int64 (L,) | sizes int32 (L, 2) | vertices int32 (V, 2) | vertex offsets int64 (L,) | counts int32 (L,)"""
        if self._dev is None:
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise RuntimeError("ocrs_models_amd.datasets.HierTextRecognition runs on MI355X only (no CPU path)")
            self._dev = tuple(t.to(self.device) for t in self._host)
            self._host = None  # nothing per pixel stays on the host
        return self._dev

    def __len__(self):
        return len(self.image_ids)

    def draw_params(self, indices) -> list:
        """One augmentation draw per line, in order, from torch's and Python's global generators (``augment``), else the identity."""
        from .augment import AugParams, sample_line_params

        sizes = [self.sizes[i] for i in indices]
        return sample_line_params(sizes) if self.augment else [AugParams(-1, s, s) for s in sizes]

    def raw(self, indices):
        """Debug hook: [(crop uint8 (1, h, w), mask uint8 0/1 (1, h, w))] device tensors of the lines, as ``ocrs_line_batch`` makes them
        (the reference's line_img before transform_image, and its generate_mask)."""
        indices = [range(len(self))[int(i)] for i in indices]
        px, px_off, sizes, verts, v_off, v_cnt = self._tensors()
        area = np.array([self.sizes[i][0] * self.sizes[i][1] for i in indices], dtype=np.int64)
        offs = np.zeros((len(indices), 3), dtype=np.int64)
        offs[:, 0] = np.cumsum(area) - area
        from .augment import _upload

        idx_d, offs_d = _upload([np.array(indices, dtype=np.int32), offs], self.device, "HierTextRecognition")
        crops = torch.empty(int(area.sum()), dtype=torch.uint8, device=self.device)
        masks = torch.empty_like(crops)
        lib().line_batch(ptr(px), ptr(px_off), ptr(sizes), ptr(verts), ptr(v_off), ptr(v_cnt), len(self), ptr(idx_d), len(indices),
                         max(self.sizes[i][0] for i in indices), ptr(offs_d), ptr(crops), ptr(masks))
        return [(crops[o:o + a].view(1, *self.sizes[i]), masks[o:o + a].view(1, *self.sizes[i])) for i, o, a in zip(indices, offs[:, 0].tolist(), area.tolist())]

    def batch(self, indices, params=None, drop_infeasible=True, dtype=torch.float32) -> dict:
        """``collate_samples`` over the items ``indices`` (train_rec.py:248-304) with ``image`` on the device: one pinned upload (records,
        offsets, indices), ``ocrs_line_batch`` and the five launches of ``ocrs_augment_lines``; nothing synchronises."""
        from .augment import _launch_lines, _line_batch_plan, _line_records, _upload

        indices = [range(len(self))[int(i)] for i in indices]
        if not indices:
            raise RuntimeError("HierTextRecognition.batch: empty batch")
        params = self.draw_params(indices) if params is None else params
        if [tuple(p.size) for p in params] != [self.sizes[i] for i in indices]:
            raise RuntimeError("HierTextRecognition.batch: params do not match the line sizes")
        texts = [self.text_seqs[i] for i in indices]
        image, meta, keep = _line_batch_plan(texts, params, self.output_height, dtype, self.device)
        if not drop_infeasible and len(keep) != len(indices):
            keep = list(range(len(indices)))
            image = torch.empty(len(keep), *image.shape[1:], dtype=dtype, device=self.device)
        if keep:
            px, px_off, sizes, verts, v_off, v_cnt = self._tensors()
            kp = [params[k] for k in keep]
            rec, offs = _line_records(kp, self.output_height)
            rec_d, offs_d, idx_d = _upload([rec, offs, np.array([indices[k] for k in keep], dtype=np.int32)], self.device, "HierTextRecognition")
            total = sum(p.size[0] * p.size[1] for p in kp)
            crops = torch.empty(total, dtype=torch.uint8, device=self.device)
            masks = torch.empty_like(crops)
            lib().line_batch(ptr(px), ptr(px_off), ptr(sizes), ptr(verts), ptr(v_off), ptr(v_cnt), len(self), ptr(idx_d), len(keep),
                             max(p.size[0] for p in kp), ptr(offs_d), ptr(crops), ptr(masks))
            _launch_lines(crops, masks, offs_d, rec_d, kp, image, self.output_height, 0, self.augment)
        return {"image": image, **meta}

    def __getitem__(self, idx: int):
        """The reference's item: {"image_id", "image": (1, output_height, w) fp32 device tensor, "text_seq"}, augmented per the flag."""
        idx = range(len(self))[idx]
        params = self.draw_params([idx])
        w = line_output_width(params[0].out_size[0], params[0].out_size[1], self.output_height)
        image = self.batch([idx], params, drop_infeasible=False)["image"]
        return {"image_id": self.image_ids[idx], "image": image[0, :, :, :w], "text_seq": self.text_seqs[idx]}


class _LineIndices(Dataset):
    def __init__(self, n: int):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class DeviceLineLoader:
    """Iterable of ``collate_samples`` batch dicts with ``image`` on the device.  It stands where ``DataLoader(HierTextRecognition(...),
    batch_size, shuffle, collate_fn=collate_samples)`` stands in train_rec.py:357-376: a stock ``DataLoader`` over a host index dataset
    consumes the sampler's random stream, so the order is torch's by construction; the augmentation draws follow in batch order.
    ``batch_sampler`` takes e.g. a ``sampler.WidthBucketedDistributedSampler(dataset.widths, ...)``."""

    def __init__(self, dataset: HierTextRecognition, batch_size: int = 1, shuffle=False, generator=None, batch_sampler=None):
        self.dataset = dataset
        collate = lambda items: [int(i) for i in items]  # noqa: E731
        if batch_sampler is not None:
            self._loader = DataLoader(_LineIndices(len(dataset)), batch_sampler=batch_sampler, collate_fn=collate)
        else:
            self._loader = DataLoader(_LineIndices(len(dataset)), batch_size=batch_size, shuffle=shuffle, generator=generator, collate_fn=collate)

    def __len__(self):
        return len(self._loader)

    def plan(self):
        """One epoch's lists of line indices, one per batch; touches no GPU."""
        return iter(self._loader)

    def __iter__(self):
        for indices in self.plan():
            yield self.dataset.batch(indices)


# ---- detection: pages with word polygons (ocrs_models/datasets/hiertext.py:22-130, ddi100.py:34-107) ----------------------------------
MAX_POLYGON_VERTICES = 512  # csrc/poly_fill.h's kMaxVerts
SHRINK_DISTANCE = 3.0  # datasets/util.py:18
BAND_ROWS = 16  # csrc/page_data.hip's kBandRows
_ROW_KEY, _ROW_BIAS = 1 << 22, 1 << 21  # sort key = page * _ROW_KEY + row + _ROW_BIAS (a shrunk ring stays within +-2^20)


def generate_json_lines_annotations(annotations_file: str, lines_file: str):
    """``HierText._generate_json_lines_annotations`` (hiertext.py:107-130): the same file, the same line per image, the same rule for
    regeneration, so the two implementations read each other's file."""
    if os.path.exists(lines_file) and (os.path.getmtime(lines_file) >= os.path.getmtime(annotations_file)):
        return
    print("Converting annotations from JSON to JSONL format...")
    with gzip.open(annotations_file) as in_fp:
        annotations = json.load(in_fp)["annotations"]
        with open(lines_file, "w") as out_fp:
            for ann in annotations:
                ann_json = json.dumps(ann)
                out_fp.write(f"{ann_json}\n")


def hiertext_word_polygons(annotations: dict) -> list:
    """hiertext.py:77-86: every word of every line of every paragraph, in that order."""
    return [[tuple(coord) for coord in word["vertices"]] for para in annotations["paragraphs"] for line in para["lines"] for word in line["words"]]


class WordTruth(NamedTuple):
    """The annotated words (or lines) of one page, as the end-to-end evaluation reads them (inference/evaluate.py)."""
    image_id: Optional[str]
    quads: np.ndarray   # (G, 4, 2) float32: convex quads
    texts: list         # G strings
    ignore: np.ndarray  # (G,) bool: "do not care" regions


def _truth_region(vertices) -> np.ndarray:
    """(4, 2) float64 region of an annotated polygon: its own vertices when they are exactly four and form a convex quad of non-zero area,
    otherwise the minimum-area rectangle of its hull (``postprocess._hull`` / ``_min_area_rect``, which take whole-numbered vertices)."""
    from .postprocess import _hull, _min_area_rect

    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    if len(v) == 4:
        e = np.roll(v, -1, axis=0) - v
        f = np.roll(e, -1, axis=0)
        turn = e[:, 0] * f[:, 1] - e[:, 1] * f[:, 0]
        area2 = float(np.dot(v[:, 0], np.roll(v[:, 1], -1)) - np.dot(v[:, 1], np.roll(v[:, 0], -1)))
        if area2 != 0.0 and ((turn >= 0).all() or (turn <= 0).all()):
            return v
    return np.asarray(_min_area_rect(_hull(np.asarray(vertices).reshape(-1, 2))), dtype=np.float64).reshape(4, 2)


def _truth_record(image_id, polygons, texts, ignore) -> WordTruth:
    quads = np.array([_truth_region(p) for p in polygons], dtype=np.float32).reshape(-1, 4, 2)
    return WordTruth(image_id, quads, [str(t) for t in texts], np.array([bool(i) for i in ignore], dtype=bool).reshape(-1))


def from_words(quads, texts, ignore=None, image_ids=None) -> list:
    """The records of ``hiertext_word_truth`` from lists, one entry per page: ``quads[p]`` = that page's polygons (any vertex count; reduced
    to convex quads by the same rule), ``texts[p]`` its strings, ``ignore[p]`` its flags (None: nothing is ignored beyond empty texts)."""
    if len(quads) != len(texts) or (ignore is not None and len(ignore) != len(quads)) or (image_ids is not None and len(image_ids) != len(quads)):
        raise ValueError("from_words: quads, texts, ignore and image_ids need one entry per page")
    out = []
    for p, (q, t) in enumerate(zip(quads, texts)):
        ig = [False] * len(t) if ignore is None else list(ignore[p])
        if len(q) != len(t) or len(ig) != len(t):
            raise ValueError(f"from_words: page {p} has {len(q)} quads, {len(t)} texts and {len(ig)} flags")
        out.append(_truth_record(None if image_ids is None else image_ids[p], list(q), t, [bool(i) or str(s) == "" for i, s in zip(ig, t)]))
    return out


def _hiertext_annotations(root_dir: str, train: bool, max_images) -> list:
    """the split's JSON-lines file (written from the annotations when it is missing or older) and the selection ``HierText`` makes from it"""
    split = "train" if train else "validation"
    annotations_file = f"{root_dir}/gt/{split}.jsonl.gz"
    if not os.path.exists(annotations_file):
        raise Exception(f'Label data file "{annotations_file}" not found')
    lines_file = annotations_file.replace(".jsonl.gz", ".jsonl")
    generate_json_lines_annotations(annotations_file, lines_file)
    with open(lines_file) as fp:
        annotations = [line for line in fp]
    if max_images:
        annotations = annotations[:max_images]
    return [json.loads(a) for a in annotations]


def _truth_ignored(item: dict, ignore_vertical: bool) -> bool:
    return item.get("legible", True) is False or item.get("text", "") == "" or (ignore_vertical and item.get("vertical", False) is True)


def hiertext_word_truth(root_dir: str, train=False, max_images=None, ignore_vertical=False) -> list:
    """One ``WordTruth`` per image of the split, in ``HierText``'s order, words in the order of ``hiertext_word_polygons``.  A word is ignored
    when it is illegible, has no text or (``ignore_vertical``) is vertical.  No image is read."""
    out = []
    for ann in _hiertext_annotations(root_dir, train, max_images):
        words = [word for para in ann["paragraphs"] for line in para["lines"] for word in line["words"]]
        out.append(_truth_record(ann["image_id"], [w["vertices"] for w in words], [w.get("text", "") for w in words],
                                 [_truth_ignored(w, ignore_vertical) for w in words]))
    return out


def hiertext_line_truth(root_dir: str, train=False, max_images=None, ignore_vertical=False) -> list:
    """``hiertext_word_truth`` for annotated LINES: the region is the minimum-area rectangle of the hull of the line's word vertices, the text
    the line's ``text``; ignored as words are."""
    from .postprocess import _hull, _min_area_rect

    out = []
    for ann in _hiertext_annotations(root_dir, train, max_images):
        lines = [line for para in ann["paragraphs"] for line in para["lines"]]
        quads = [_min_area_rect(_hull(np.array([v for w in line["words"] for v in w["vertices"]]).reshape(-1, 2))) for line in lines]
        out.append(WordTruth(ann["image_id"], np.array(quads, dtype=np.float32).reshape(-1, 4, 2), [str(line.get("text", "")) for line in lines],
                             np.array([_truth_ignored(line, ignore_vertical) for line in lines], dtype=bool).reshape(-1)))
    return out


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


def _whole_polygon(poly, what: str) -> list:
    pts = [tuple(c) for c in (poly.tolist() if hasattr(poly, "tolist") else poly)]
    if any(len(c) < 2 or int(c[0]) != c[0] or int(c[1]) != c[1] for c in pts):
        raise RuntimeError(f"{what}: vertex coordinates must be whole numbers (the shrink kernel takes them as integers)")
    pts = [(int(c[0]), int(c[1])) for c in pts]
    if len(pts) > MAX_POLYGON_VERTICES or any(abs(c) > 65535 for v in pts for c in v):
        raise RuntimeError(f"{what}: polygons of at most {MAX_POLYGON_VERTICES} vertices with coordinates within +-65535 are supported, "
                           f"this one has {len(pts)}")
    return pts


class _PageStore(Dataset):
    """What HierText and DDI100 share: the pages' grey pixels and the word polygons in device memory, shrunk once at construction
    (``ocrs_shrink_polygons``), sorted by first row and binned per band of rows; an item or a batch is then ``ocrs_page_batch`` (gather +
    ``generate_mask``) followed by ``ocrs_augment_det`` (``prepare_transform(mask_size, augment)``)."""

    def _init_args(self, augment, device, mask_size, transform, shrink_dist=SHRINK_DISTANCE):
        name = type(self).__name__
        if transform is not None or callable(augment):
            raise TypeError(f"{name} takes augment=True/False and mask_size, not a transform: prepare_transform(mask_size, augment) runs "
                            "inside the batch kernels on the device")
        self.augment, self.device, self.mask_size, self.shrink_dist = bool(augment), torch.device(device), tuple(mask_size), float(shrink_dist)

    @classmethod
    def from_pages(cls, pages, polygons, paths=None, augment=False, device="cuda", mask_size=None, shrink_dist=SHRINK_DISTANCE):
        """A store made from memory instead of a directory (measurement and tests): ``pages`` (h, w) uint8 arrays, ``polygons`` one list of
        integer-vertex polygons per page."""
        from .augment import MASK_SIZE

        self = cls.__new__(cls)
        Dataset.__init__(self)
        self._init_args(augment, device, mask_size or MASK_SIZE, None, shrink_dist)
        self._set_store(list(paths) if paths is not None else [str(k) for k in range(len(pages))], [np.ascontiguousarray(p) for p in pages], polygons)
        return self

    def _set_store(self, paths, pages, polygons):
        from .augment import _check_sizes

        name = type(self).__name__
        if len(polygons) != len(pages) or len(paths) != len(pages):
            raise RuntimeError(f"{name}: need one path and one polygon list per page")
        if any(p.ndim != 2 or p.dtype != np.uint8 for p in pages):
            raise RuntimeError(f"{name}: pages must be (h, w) uint8 arrays")
        self.paths = paths
        self.sizes = [tuple(int(s) for s in p.shape) for p in pages]  # (h, w) of every page
        _check_sizes(self.sizes, name)
        polys = [[_whole_polygon(q, f"{name}: page {paths[k]}") for q in page_polys] for k, page_polys in enumerate(polygons)]
        self.poly_counts = [len(p) for p in polys]
        area = np.array([h * w for h, w in self.sizes], dtype=np.int64)
        padded = (area + 15) // 16 * 16  # every page starts on a 16-byte boundary (16 bytes per lane in the gather)
        px_off = np.cumsum(padded) - padded
        counts = np.array([len(q) for p in polys for q in p], dtype=np.int32)
        verts = np.array([v for p in polys for q in p for v in q], dtype=np.int32).reshape(-1, 2)
        if 2 * len(verts) >= 2**31:
            raise RuntimeError(f"{name}: {len(verts)} polygon vertices are too many for one store: use max_images")
        self._host = None
        if pages:
            pixels = np.zeros(int(padded.sum()), dtype=np.uint8)
            for p, o, a in zip(pages, px_off.tolist(), area.tolist()):
                pixels[o:o + a] = p.reshape(-1)
            self._host = (torch.from_numpy(pixels), torch.from_numpy(px_off), torch.tensor(self.sizes, dtype=torch.int32), torch.from_numpy(verts),
                          torch.from_numpy(np.cumsum(counts, dtype=np.int64) - counts), torch.from_numpy(counts),
                          torch.from_numpy(np.repeat(np.arange(len(pages), dtype=np.int64), self.poly_counts)))
        self._dev = None
        self.skipped = None  # how many polygons the shrink dropped: known once the store is on the device
        if pages and self.device.type == "cuda" and torch.cuda.is_available():
            self._tensors()

    def _tensors(self):
        """pixels uint8 | pixel offsets int64 (P,) | sizes int32 (P, 2) | shrunk vertices int32 (2V, 2) | polygon records int32 (Q, 4) =
        first vertex, count, y_min, y_max, sorted by (page, y_min) | band offsets int64 (P,) | bands int32 (.., 2)"""
        if self._dev is None:
            name = type(self).__name__
            if self.device.type != "cuda" or not torch.cuda.is_available():
                raise RuntimeError(f"ocrs_models_amd.datasets.{name} runs on MI355X only (no CPU path)")
            if self._host is None:
                raise RuntimeError(f"ocrs_models_amd.datasets.{name}: the store is empty")
            pixels, px_off, sizes, verts, v_off, v_cnt, poly_page = self._host
            V, Q = verts.shape[0], v_cnt.shape[0]
            need = pixels.numel() + 72 * V + 64 * Q + (1 << 20)  # the pages, the shrink's buffers, the records
            free, _ = torch.cuda.mem_get_info(self.device)
            if need > free:
                raise RuntimeError(f"ocrs_models_amd.datasets.{name}: the store needs {need} bytes of device memory ({pixels.numel()} of them "
                                   f"pixels) and {free} are free: load fewer pages with max_images")
            dev = self.device
            d_px, d_pxoff, d_sizes = pixels.to(dev), px_off.to(dev), sizes.to(dev)
            out_verts = torch.zeros(max(2 * V, 1), 2, dtype=torch.int32, device=dev)
            records = torch.zeros(0, 4, dtype=torch.int32, device=dev)
            if Q:
                d_verts, d_voff, d_vcnt, d_page = verts.to(dev), v_off.to(dev), v_cnt.to(dev), poly_page.to(dev)
                ws = torch.empty(max(3 * V, 1), dtype=torch.int32, device=dev)
                out_xy = torch.empty(max(2 * V, 1), 2, dtype=torch.float64, device=dev)
                out_cnt = torch.empty(Q, dtype=torch.int32, device=dev)
                out_rows = torch.empty(Q, 2, dtype=torch.int32, device=dev)
                lib().shrink_polygons(ptr(d_verts), ptr(d_voff), ptr(d_vcnt), Q, self.shrink_dist, ptr(ws), ptr(out_xy), ptr(out_verts), ptr(out_cnt),
                                      ptr(out_rows))
                if bool((out_cnt < 0).any()):  # (construction may wait for the device; a batch never does)
                    raise RuntimeError(f"{name}: a shrunk polygon has more than {MAX_POLYGON_VERTICES} vertices (every reflex corner past the "
                                       "mitre limit adds one)")
                kept = torch.nonzero(out_cnt > 0).reshape(-1)
                key = d_page[kept] * _ROW_KEY + out_rows[kept, 0].long() + _ROW_BIAS
                kept = kept[torch.argsort(key, stable=True)]
                records = torch.stack([(2 * d_voff[kept]).int(), out_cnt[kept], out_rows[kept, 0], out_rows[kept, 1]], dim=1).contiguous()
                self.skipped = Q - int(kept.numel())
                del ws, out_xy
            else:
                self.skipped = 0
            # the band table: polygons [lo, hi) of the sorted records can touch rows [16 k, 16 k + 15] of their page
            nb = (sizes[:, 0].long() + BAND_ROWS - 1) // BAND_ROWS
            band_off = torch.cumsum(nb, 0) - nb
            b_page = torch.repeat_interleave(torch.arange(len(nb)), nb)
            b_row0 = (torch.arange(int(nb.sum())) - band_off[b_page]) * BAND_ROWS
            b_row1 = torch.minimum(b_row0 + BAND_ROWS - 1, sizes[:, 0].long()[b_page] - 1)
            b_page, b_row0, b_row1 = b_page.to(dev), b_row0.to(dev), b_row1.to(dev)
            if records.shape[0]:
                r_page = d_page[kept]
                first_key = r_page * _ROW_KEY + records[:, 2].long() + _ROW_BIAS
                last_key = torch.cummax(r_page * _ROW_KEY + records[:, 3].long() + _ROW_BIAS, 0)[0]
                lo = torch.searchsorted(last_key, b_page * _ROW_KEY + b_row0 + _ROW_BIAS, right=False)
                hi = torch.searchsorted(first_key, b_page * _ROW_KEY + b_row1 + _ROW_BIAS, right=True)
                bands = torch.stack([lo, torch.maximum(hi, lo)], dim=1).int().contiguous()
            else:
                bands = torch.zeros(int(nb.sum()), 2, dtype=torch.int32, device=dev)
            self._dev = (d_px, d_pxoff, d_sizes, out_verts, records, band_off.to(dev), bands)
            self._host = None  # nothing per pixel stays on the host
        return self._dev

    def __len__(self):
        return len(self.paths)

    def draw_params(self, indices) -> list:
        """One ``prepare_transform(mask_size, augment)`` draw per page, in order, from torch's and Python's global generators, else the identity."""
        from .augment import AugParams, sample_detection_params

        sizes = [self.sizes[i] for i in indices]
        return sample_detection_params(sizes) if self.augment else [AugParams(-1, s, s) for s in sizes]

    def _gather(self, indices, extra: list):
        """``ocrs_page_batch`` for checked ``indices`` -> (pages, masks) packed uint8 device buffers, the uploaded offsets and ``extra``
        sections (one pinned upload for all of them), the host offsets."""
        from .augment import _upload

        px, px_off, sizes, verts, records, band_off, bands = self._tensors()
        area = np.array([self.sizes[i][0] * self.sizes[i][1] for i in indices], dtype=np.int64)
        padded = (area + 15) // 16 * 16
        offs = np.cumsum(padded) - padded
        up = _upload([offs, np.array(indices, dtype=np.int32)] + extra, self.device, type(self).__name__)
        pages = torch.empty(int(padded.sum()), dtype=torch.uint8, device=self.device)
        masks = torch.empty_like(pages)
        lib().page_batch(ptr(px), ptr(px_off), ptr(sizes), ptr(verts), verts.shape[0], ptr(records) if records.shape[0] else None, records.shape[0],
                         ptr(band_off), ptr(bands), len(self), ptr(up[1]), len(indices), max(self.sizes[i][0] for i in indices),
                         max(self.sizes[i][1] for i in indices), ptr(up[0]), ptr(pages), ptr(masks))
        return pages, masks, up[0], up[2:], offs

    def raw(self, indices):
        """Debug hook: [(page uint8 (1, h, w), mask uint8 0/1 (1, h, w))] device tensors of the pages, as ``ocrs_page_batch`` makes them
        (the reference's read_image before transform_image, and its generate_mask)."""
        indices = [range(len(self))[int(i)] for i in indices]
        if not indices:
            return []
        pages, masks, _, _, offs = self._gather(indices, [])
        return [(pages[o:o + h * w].view(1, h, w), masks[o:o + h * w].view(1, h, w)) for (h, w), o in zip((self.sizes[i] for i in indices), offs.tolist())]

    def batch(self, indices, params=None, dtype=torch.float32) -> dict:
        """The default collate of the items ``indices`` (train_detection.py:350-366) on the device: {"path": [...], "image": (B, 1, *mask_size)
        ``dtype``, "text_mask": (B, 1, *mask_size) fp32}.  One pinned upload (records, offsets, indices), ``ocrs_page_batch`` and the three
        launches of ``ocrs_augment_det``; nothing synchronises."""
        from .augment import _DT, _records

        name = type(self).__name__
        indices = [range(len(self))[int(i)] for i in indices]
        if not indices:
            raise RuntimeError(f"{name}.batch: empty batch")
        params = self.draw_params(indices) if params is None else params
        if [tuple(p.size) for p in params] != [self.sizes[i] for i in indices]:
            raise RuntimeError(f"{name}.batch: params do not match the page sizes")
        B, (oh, ow) = len(indices), self.mask_size
        pages, masks, offs_d, (rec_d,), _ = self._gather(indices, [_records(params, line=False)])
        image = torch.empty(B, 1, oh, ow, dtype=dtype, device=self.device)
        text_mask = torch.empty(B, 1, oh, ow, dtype=torch.float32, device=self.device)
        ws = torch.empty(lib().augment_det_ws_floats(B), dtype=torch.float32, device=self.device)
        lib().augment_det(ptr(pages), ptr(masks), ptr(offs_d), ptr(rec_d), ptr(ws), ptr(image), ptr(text_mask), B, max(self.sizes[i][0] for i in indices),
                          max(self.sizes[i][1] for i in indices), oh, ow, 0, _DT[dtype])
        return {"path": [self.paths[i] for i in indices], "image": image, "text_mask": text_mask}

    def __getitem__(self, idx: int):
        """The reference's item: {"path", "image": (1, *mask_size) fp32 device tensor, "text_mask": (1, *mask_size)}, augmented per the flag."""
        idx = range(len(self))[idx]
        b = self.batch([idx])
        return {"path": b["path"][0], "image": b["image"][0], "text_mask": b["text_mask"][0]}


def _decode_pages(paths: list, read) -> list:
    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        return list(pool.map(read, paths))


class HierText(_PageStore):
    """HierText dataset for text detection: the reference's ``HierText`` (hiertext.py:22-130; same directory layout and JSONL file) with every
    page and its word polygons resident in device memory.  ``augment`` and ``mask_size`` stand where the reference takes ``transform``:
    ``prepare_transform(mask_size, augment)`` runs inside the batch kernels (augment.py)."""

    def __init__(self, root_dir: str, train=True, augment=False, max_images=None, device="cuda", mask_size=None, transform=None):
        from .augment import MASK_SIZE

        super().__init__()
        self._init_args(augment, device, mask_size or MASK_SIZE, transform)
        split = "train" if train else "validation"
        self._img_dir = f"{root_dir}/{split}"
        annotations_file = f"{root_dir}/gt/{split}.jsonl.gz"
        if not os.path.exists(self._img_dir):
            raise Exception(f'Image directory "{self._img_dir}" not found')
        if not os.path.exists(annotations_file):
            raise Exception(f'Label data file "{annotations_file}" not found')
        lines_file = annotations_file.replace(".jsonl.gz", ".jsonl")
        generate_json_lines_annotations(annotations_file, lines_file)
        with open(lines_file) as fp:
            self._annotations = [line for line in fp]
        if max_images:
            self._annotations = self._annotations[:max_images]
        anns = [json.loads(a) for a in self._annotations]
        paths = [f"{self._img_dir}/{a['image_id']}.jpg" for a in anns]
        self._set_store(paths, _decode_pages(paths, _read_gray), [hiertext_word_polygons(a) for a in anns])


def _read_one_channel(path: str) -> np.ndarray:
    from PIL import Image

    with Image.open(path) as im:
        if len(im.getbands()) != 1:
            raise RuntimeError(f"{path}: DDI100 pages must have one channel, this image has {len(im.getbands())} ({im.mode}): convert it to "
                               "greyscale (the reference fails on it when it stacks the image and its mask)")
    return _read_gray(path)


class DDI100(_PageStore):
    """Distorted Document Images (DDI-100) dataset for text detection: the reference's ``DDI100`` (ddi100.py:34-107; ``gen_imgs/`` and
    ``gen_boxes/*.pickle``, sorted listing, max_images before the 90/10 split) with the pages and word quads resident in device memory.
    The quads are ``w["box"]`` as ``__getitem__`` passes them to generate_mask (ddi100.py:89-93)."""

    def __init__(self, root_dir: str, train=True, augment=False, max_images=None, device="cuda", mask_size=None, transform=None):
        from .augment import MASK_SIZE

        super().__init__()
        self._init_args(augment, device, mask_size or MASK_SIZE, transform)
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
        self._set_store(paths, _decode_pages(paths, _read_one_channel), quads)


class DevicePageLoader:
    """Iterable of detection batch dicts with ``image`` and ``text_mask`` on the device.  It stands where ``DataLoader(HierText(...) or
    DDI100(...), batch_size, shuffle)`` stands in train_detection.py:350-366: a stock ``DataLoader`` over a host index dataset consumes the
    sampler's random stream, so the order is torch's by construction; the augmentation draws follow in batch order."""

    def __init__(self, dataset: _PageStore, batch_size: int = 1, shuffle=False, generator=None, dtype=torch.float32):
        self.dataset, self.dtype = dataset, dtype
        self._loader = DataLoader(_LineIndices(len(dataset)), batch_size=batch_size, shuffle=shuffle, generator=generator,
                                  collate_fn=lambda items: [int(i) for i in items])

    def __len__(self):
        return len(self._loader)

    def plan(self):
        """One epoch's lists of page indices, one per batch; touches no GPU."""
        return iter(self._loader)

    def __iter__(self):
        for indices in self.plan():
            yield self.dataset.batch(indices, dtype=self.dtype)

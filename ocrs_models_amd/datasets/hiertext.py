"""The HierText datasets (ocrs_models/datasets/hiertext.py), resident on the device: ``HierTextRecognition`` (text lines, hiertext.py:145-427)
with its loader, ``HierText`` (pages with word polygons, hiertext.py:22-130; the store is pages.py's), and the word and line ground truth
that the end-to-end evaluation reads from the same annotations."""
from __future__ import annotations

import gzip
import json
import os
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch.utils.data import Dataset

from .._lib import lib, ptr
from ..augment import launch_lines, line_batch_plan, line_records, resolve_params, sample_line_params, upload
from ..postprocess import _hull, _min_area_rect
from ..text import DEFAULT_ALPHABET, encode_text, line_output_width
from .pages import PageStore
from .util import DeviceStore, IndexLoader, bounding_box_size, decode_pages, line_bounding_box, read_gray

MAX_LINE_VERTICES = 512  # csrc/line_data.hip's kMaxVerts


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


def _page_crops(img_dir: str, cache_dir: str, image_id: str, boxes: list) -> list:
    """The cached crops of one page's boxes (``_get_line_image``, hiertext.py:198-233): read where the cache file exists, otherwise cut from
    the page (decoded once for all of them), written through .tmp + rename.  None for a crop that is empty after clamping."""
    from PIL import Image

    page, out = None, []
    for min_x, min_y, max_x, max_y in boxes:
        cache_path = f"{cache_dir}/{image_id}/{min_x}_{min_y}_{max_x}_{max_y}.png"
        if not os.path.exists(cache_path):
            if page is None:
                page = read_gray(f"{img_dir}/{image_id}.jpg")
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
        out.append(read_gray(cache_path))
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


class HierTextRecognition(DeviceStore):
    """HierText dataset for text recognition: the reference's ``HierTextRecognition`` (hiertext.py:145-304; same directory layout, lines
    file and crop cache) with every line crop resident in device memory.  ``augment`` stands where the reference takes ``transform``: the
    augmentations run inside the batch kernels (augment.py), so it is a flag.  A line whose crop is empty after clamping to the page is
    dropped at construction with a counted message (the reference fails on such an item).  The store (``_tensors()``): pixels uint8 | pixel
    offsets int64 (L,) | sizes int32 (L, 2) | vertices int32 (V, 2) | vertex offsets int64 (L,) | counts int32 (L,)."""

    def __init__(self, root_dir: str, train=True, augment=False, max_images=None, alphabet=None, output_height: int = 64, device="cuda",
                 transform=None):
        super().__init__()
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
        host = None
        if crops:
            host = (torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])), torch.from_numpy(np.cumsum(area) - area),
                    torch.tensor(self.sizes, dtype=torch.int32), torch.from_numpy(verts),
                    torch.from_numpy(np.cumsum(counts, dtype=np.int64) - counts), torch.from_numpy(counts))
        self._set_host(host, self.device.type == "cuda")

    def __len__(self):
        return len(self.image_ids)

    def draw_params(self, indices) -> list:
        """One augmentation draw per line, in order, from torch's and Python's global generators (``augment``), else the identity."""
        return self._params(None, indices)

    def _params(self, params, indices) -> list:
        return resolve_params(params, [self.sizes[i] for i in indices], self.augment, sample_line_params, "HierTextRecognition.batch", "line")

    def _gather(self, indices, offs, extra: list):
        """``ocrs_line_batch`` for checked ``indices``, line k to ``offs[k, 0]`` -> (crops, masks) packed uint8 device buffers, the uploaded
        offsets and ``extra`` sections (one pinned upload for all of them)."""
        px, px_off, sizes, verts, v_off, v_cnt = self._tensors()
        up = upload([offs, np.array(indices, dtype=np.int32)] + extra, self.device, "HierTextRecognition")
        crops = torch.empty(sum(self.sizes[i][0] * self.sizes[i][1] for i in indices), dtype=torch.uint8, device=self.device)
        masks = torch.empty_like(crops)
        lib().line_batch(ptr(px), ptr(px_off), ptr(sizes), ptr(verts), ptr(v_off), ptr(v_cnt), len(self), ptr(up[1]), len(indices),
                         max(self.sizes[i][0] for i in indices), ptr(up[0]), ptr(crops), ptr(masks))
        return crops, masks, up[0], up[2:]

    def raw(self, indices):
        """Debug hook: [(crop uint8 (1, h, w), mask uint8 0/1 (1, h, w))] device tensors of the lines, as ``ocrs_line_batch`` makes them
        (the reference's line_img before transform_image, and its generate_mask)."""
        indices = [range(len(self))[int(i)] for i in indices]
        area = np.array([self.sizes[i][0] * self.sizes[i][1] for i in indices], dtype=np.int64)
        offs = np.zeros((len(indices), 3), dtype=np.int64)
        offs[:, 0] = np.cumsum(area) - area
        crops, masks, _, _ = self._gather(indices, offs, [])
        return [(crops[o:o + a].view(1, *self.sizes[i]), masks[o:o + a].view(1, *self.sizes[i])) for i, o, a in zip(indices, offs[:, 0].tolist(), area.tolist())]

    def batch(self, indices, params=None, drop_infeasible=True, dtype=torch.float32) -> dict:
        """``collate_samples`` over the items ``indices`` (train_rec.py:248-304) with ``image`` on the device: one pinned upload (records,
        offsets, indices), ``ocrs_line_batch`` and the five launches of ``ocrs_augment_lines``; nothing synchronises."""
        indices = [range(len(self))[int(i)] for i in indices]
        if not indices:
            raise RuntimeError("HierTextRecognition.batch: empty batch")
        params = self._params(params, indices)
        image, meta, keep = line_batch_plan([self.text_seqs[i] for i in indices], params, self.output_height, dtype, self.device)
        if not drop_infeasible and len(keep) != len(indices):
            keep = list(range(len(indices)))
            image = torch.empty(len(keep), *image.shape[1:], dtype=dtype, device=self.device)
        if keep:
            kp = [params[k] for k in keep]
            rec, offs = line_records(kp, self.output_height)
            crops, masks, offs_d, (rec_d,) = self._gather([indices[k] for k in keep], offs, [rec])
            launch_lines(crops, masks, offs_d, rec_d, kp, image, self.output_height, 0, self.augment)
        return {"image": image, **meta}

    def __getitem__(self, idx: int):
        """The reference's item: {"image_id", "image": (1, output_height, w) fp32 device tensor, "text_seq"}, augmented per the flag."""
        idx = range(len(self))[idx]
        params = self.draw_params([idx])
        w = line_output_width(params[0].out_size[0], params[0].out_size[1], self.output_height)
        image = self.batch([idx], params, drop_infeasible=False)["image"]
        return {"image_id": self.image_ids[idx], "image": image[0, :, :, :w], "text_seq": self.text_seqs[idx]}


class DeviceLineLoader(IndexLoader):
    """Iterable of ``collate_samples`` batch dicts with ``image`` on the device.  It stands where ``DataLoader(HierTextRecognition(...),
    batch_size, shuffle, collate_fn=collate_samples)`` stands in train_rec.py:357-376 (``IndexLoader``: the order is torch's).
    ``batch_sampler`` takes e.g. a ``sampler.WidthBucketedDistributedSampler(dataset.widths, ...)``."""

    def __init__(self, dataset: HierTextRecognition, batch_size: int = 1, shuffle=False, generator=None, batch_sampler=None):
        super().__init__(dataset, batch_size, shuffle, generator, batch_sampler)


# ---- detection pages and the evaluation's ground truth (hiertext.py:22-130) ----------------------------------------------------------
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
    out = []
    for ann in _hiertext_annotations(root_dir, train, max_images):
        lines = [line for para in ann["paragraphs"] for line in para["lines"]]
        quads = [_min_area_rect(_hull(np.array([v for w in line["words"] for v in w["vertices"]]).reshape(-1, 2))) for line in lines]
        out.append(WordTruth(ann["image_id"], np.array(quads, dtype=np.float32).reshape(-1, 4, 2), [str(line.get("text", "")) for line in lines],
                             np.array([_truth_ignored(line, ignore_vertical) for line in lines], dtype=bool).reshape(-1)))
    return out


class HierText(PageStore):
    """HierText dataset for text detection: the reference's ``HierText`` (hiertext.py:22-130; same directory layout and JSONL file) with every
    page and its word polygons resident in device memory.  ``augment`` and ``mask_size`` stand where the reference takes ``transform``:
    ``prepare_transform(mask_size, augment)`` runs inside the batch kernels (augment.py)."""

    def __init__(self, root_dir: str, train=True, augment=False, max_images=None, device="cuda", mask_size=None, transform=None):
        super().__init__()
        self._init_args(augment, device, mask_size, transform)
        self._img_dir = f"{root_dir}/{'train' if train else 'validation'}"
        if not os.path.exists(self._img_dir):
            raise Exception(f'Image directory "{self._img_dir}" not found')
        anns = _hiertext_annotations(root_dir, train, max_images)
        paths = [f"{self._img_dir}/{a['image_id']}.jpg" for a in anns]
        self._set_store(paths, decode_pages(paths), [hiertext_word_polygons(a) for a in anns])

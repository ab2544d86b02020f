"""The device-resident page store that the detection datasets HierText (hiertext.py) and DDI100 (ddi100.py) share, and its loader."""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import Dataset

from .._lib import lib, ptr
from ..augment import MASK_SIZE, check_sizes, launch_det, records, resolve_params, sample_detection_params, upload
from .util import MAX_POLYGON_VERTICES, SHRINK_DISTANCE, DeviceStore, IndexLoader, whole_polygon

BAND_ROWS = 16  # csrc/page_data.hip's kBandRows
_ROW_KEY, _ROW_BIAS = 1 << 22, 1 << 21  # sort key = page * _ROW_KEY + row + _ROW_BIAS (a shrunk ring stays within +-2^20)


class PageStore(DeviceStore):
    """What HierText and DDI100 share: the pages' grey pixels and the word polygons in device memory, shrunk once at construction
    (``ocrs_shrink_polygons``), sorted by first row and binned per band of rows; an item or a batch is then ``ocrs_page_batch`` (gather +
    ``generate_mask``) followed by ``ocrs_augment_det`` (``prepare_transform(mask_size, augment)``).  The store (``_tensors()``): pixels
    uint8 | pixel offsets int64 (P,) | sizes int32 (P, 2) | shrunk vertices int32 (2V, 2) | polygon records int32 (Q, 4) = first vertex,
    count, y_min, y_max, sorted by (page, y_min) | band offsets int64 (P,) | bands int32 (.., 2)."""

    def _init_args(self, augment, device, mask_size, transform, shrink_dist=SHRINK_DISTANCE):
        name = type(self).__name__
        if transform is not None or callable(augment):
            raise TypeError(f"{name} takes augment=True/False and mask_size, not a transform: prepare_transform(mask_size, augment) runs "
                            "inside the batch kernels on the device")
        self.augment, self.device, self.shrink_dist = bool(augment), torch.device(device), float(shrink_dist)
        self.mask_size = tuple(mask_size or MASK_SIZE)

    @classmethod
    def from_pages(cls, pages, polygons, paths=None, augment=False, device="cuda", mask_size=None, shrink_dist=SHRINK_DISTANCE):
        """A store made from memory instead of a directory (measurement and tests): ``pages`` (h, w) uint8 arrays, ``polygons`` one list of
        integer-vertex polygons per page."""
        self = cls.__new__(cls)
        Dataset.__init__(self)
        self._init_args(augment, device, mask_size, None, shrink_dist)
        self._set_store(list(paths) if paths is not None else [str(k) for k in range(len(pages))], [np.ascontiguousarray(p) for p in pages], polygons)
        return self

    def _set_store(self, paths, pages, polygons):
        name = type(self).__name__
        if len(polygons) != len(pages) or len(paths) != len(pages):
            raise RuntimeError(f"{name}: need one path and one polygon list per page")
        if any(p.ndim != 2 or p.dtype != np.uint8 for p in pages):
            raise RuntimeError(f"{name}: pages must be (h, w) uint8 arrays")
        self.paths = paths
        self.sizes = [tuple(int(s) for s in p.shape) for p in pages]  # (h, w) of every page
        check_sizes(self.sizes, name)
        polys = [[whole_polygon(q, f"{name}: page {paths[k]}") for q in page_polys] for k, page_polys in enumerate(polygons)]
        self.poly_counts = [len(p) for p in polys]
        area = np.array([h * w for h, w in self.sizes], dtype=np.int64)
        padded = (area + 15) // 16 * 16  # every page starts on a 16-byte boundary (16 bytes per lane in the gather)
        px_off = np.cumsum(padded) - padded
        counts = np.array([len(q) for p in polys for q in p], dtype=np.int32)
        verts = np.array([v for p in polys for q in p for v in q], dtype=np.int32).reshape(-1, 2)
        if 2 * len(verts) >= 2**31:
            raise RuntimeError(f"{name}: {len(verts)} polygon vertices are too many for one store: use max_images")
        host = None
        if pages:
            pixels = np.zeros(int(padded.sum()), dtype=np.uint8)
            for p, o, a in zip(pages, px_off.tolist(), area.tolist()):
                pixels[o:o + a] = p.reshape(-1)
            host = (torch.from_numpy(pixels), torch.from_numpy(px_off), torch.tensor(self.sizes, dtype=torch.int32), torch.from_numpy(verts),
                    torch.from_numpy(np.cumsum(counts, dtype=np.int64) - counts), torch.from_numpy(counts),
                    torch.from_numpy(np.repeat(np.arange(len(pages), dtype=np.int64), self.poly_counts)))
        self.skipped = None  # how many polygons the shrink dropped: known once the store is on the device
        self._set_host(host, self.device.type == "cuda")

    def _upload(self, host) -> tuple:
        """The construction-time device work: the shrink, the sort by (page, first row) and the band table."""
        name, dev = type(self).__name__, self.device
        pixels, px_off, sizes, verts, v_off, v_cnt, poly_page = host
        V, Q = verts.shape[0], v_cnt.shape[0]
        need = pixels.numel() + 72 * V + 64 * Q + (1 << 20)  # the pages, the shrink's buffers, the records
        free, _ = torch.cuda.mem_get_info(dev)
        if need > free:
            raise RuntimeError(f"ocrs_models_amd.datasets.{name}: the store needs {need} bytes of device memory ({pixels.numel()} of them "
                               f"pixels) and {free} are free: load fewer pages with max_images")
        d_px, d_pxoff, d_sizes = pixels.to(dev), px_off.to(dev), sizes.to(dev)
        out_verts = torch.zeros(max(2 * V, 1), 2, dtype=torch.int32, device=dev)
        records_d = torch.zeros(0, 4, dtype=torch.int32, device=dev)
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
            records_d = torch.stack([(2 * d_voff[kept]).int(), out_cnt[kept], out_rows[kept, 0], out_rows[kept, 1]], dim=1).contiguous()
            del ws, out_xy
        self.skipped = Q - records_d.shape[0]
        # the band table: polygons [lo, hi) of the sorted records can touch rows [16 k, 16 k + 15] of their page
        nb = (sizes[:, 0].long() + BAND_ROWS - 1) // BAND_ROWS
        band_off = torch.cumsum(nb, 0) - nb
        b_page = torch.repeat_interleave(torch.arange(len(nb)), nb)
        b_row0 = (torch.arange(int(nb.sum())) - band_off[b_page]) * BAND_ROWS
        b_row1 = torch.minimum(b_row0 + BAND_ROWS - 1, sizes[:, 0].long()[b_page] - 1)
        b_page, b_row0, b_row1 = b_page.to(dev), b_row0.to(dev), b_row1.to(dev)
        if records_d.shape[0]:
            r_page = d_page[kept]
            first_key = r_page * _ROW_KEY + records_d[:, 2].long() + _ROW_BIAS
            last_key = torch.cummax(r_page * _ROW_KEY + records_d[:, 3].long() + _ROW_BIAS, 0)[0]
            lo = torch.searchsorted(last_key, b_page * _ROW_KEY + b_row0 + _ROW_BIAS, right=False)
            hi = torch.searchsorted(first_key, b_page * _ROW_KEY + b_row1 + _ROW_BIAS, right=True)
            bands = torch.stack([lo, torch.maximum(hi, lo)], dim=1).int().contiguous()
        else:
            bands = torch.zeros(int(nb.sum()), 2, dtype=torch.int32, device=dev)
        return d_px, d_pxoff, d_sizes, out_verts, records_d, band_off.to(dev), bands

    def __len__(self):
        return len(self.paths)

    def draw_params(self, indices) -> list:
        """One ``prepare_transform(mask_size, augment)`` draw per page, in order, from torch's and Python's global generators, else the identity."""
        return self._params(None, indices)

    def _params(self, params, indices) -> list:
        return resolve_params(params, [self.sizes[i] for i in indices], self.augment, sample_detection_params, f"{type(self).__name__}.batch", "page")

    def _gather(self, indices, extra: list):
        """``ocrs_page_batch`` for checked ``indices`` -> (pages, masks) packed uint8 device buffers, the uploaded offsets and ``extra``
        sections (one pinned upload for all of them), the host offsets."""
        px, px_off, sizes, verts, recs, band_off, bands = self._tensors()
        area = np.array([self.sizes[i][0] * self.sizes[i][1] for i in indices], dtype=np.int64)
        padded = (area + 15) // 16 * 16
        offs = np.cumsum(padded) - padded
        up = upload([offs, np.array(indices, dtype=np.int32)] + extra, self.device, type(self).__name__)
        pages = torch.empty(int(padded.sum()), dtype=torch.uint8, device=self.device)
        masks = torch.empty_like(pages)
        lib().page_batch(ptr(px), ptr(px_off), ptr(sizes), ptr(verts), verts.shape[0], ptr(recs) if recs.shape[0] else None, recs.shape[0],
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
        indices = [range(len(self))[int(i)] for i in indices]
        if not indices:
            raise RuntimeError(f"{type(self).__name__}.batch: empty batch")
        params = self._params(params, indices)
        pages, masks, offs_d, (rec_d,), _ = self._gather(indices, [records(params, line=False)])
        image = torch.empty(len(indices), 1, *self.mask_size, dtype=dtype, device=self.device)
        text_mask = torch.empty(len(indices), 1, *self.mask_size, dtype=torch.float32, device=self.device)
        launch_det(pages, masks, offs_d, rec_d, [self.sizes[i] for i in indices], image, text_mask, 0)
        return {"path": [self.paths[i] for i in indices], "image": image, "text_mask": text_mask}

    def __getitem__(self, idx: int):
        """The reference's item: {"path", "image": (1, *mask_size) fp32 device tensor, "text_mask": (1, *mask_size)}, augmented per the flag."""
        idx = range(len(self))[idx]
        b = self.batch([idx])
        return {"path": b["path"][0], "image": b["image"][0], "text_mask": b["text_mask"][0]}


class DevicePageLoader(IndexLoader):
    """Iterable of detection batch dicts with ``image`` and ``text_mask`` on the device.  It stands where ``DataLoader(HierText(...) or
    DDI100(...), batch_size, shuffle)`` stands in train_detection.py:350-366 (``IndexLoader``: the order is torch's)."""

    def __init__(self, dataset: PageStore, batch_size: int = 1, shuffle=False, generator=None, dtype=torch.float32):
        super().__init__(dataset, batch_size, shuffle, generator, dtype=dtype)
        self.dtype = dtype

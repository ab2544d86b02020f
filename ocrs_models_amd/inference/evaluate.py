"""End-to-end accuracy: what ``ocr_page`` / ``ocr_lines`` / ``ocr_pages`` return, scored against annotated words or lines (DESIGN.md §23;
csrc/ocr_eval.hip, C ABI section "end-to-end accuracy"; restated for the tests in tests/eval_ref.py).

``match_words`` assigns predicted to annotated quads one to one, page by page; ``OcrAccuracyStats`` keeps twelve integer counters on the device
across ``update`` calls -- one upload, one memset and four kernels, no wait -- and ``result()`` is the one host wait; ``evaluate_pages`` runs ``ocr_pages``
over a list of pages and feeds the stats.  The ground truth is a list of ``datasets.WordTruth`` records (``hiertext_word_truth``,
``hiertext_line_truth``, ``from_words``)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from . import drivers
from .args import _need_quads

COUNTERS = ("pages", "pred", "gt", "pred_ignored", "matched", "exact", "exact_ci", "edit_sum", "gt_chars_matched", "pred_chars_unmatched",
            "gt_chars_unmatched", "gt_chars")


class Matches(NamedTuple):
    gt_of_pred: torch.Tensor   # (P,) int32: index of the matched annotation within the page, -1 unmatched, -2 ignored
    pred_of_gt: torch.Tensor   # (G,) int32: index of the matched prediction within the page, -1 unmatched
    iou_of_pred: torch.Tensor  # (P,) float64: the matched pair's IoU, 0.0 otherwise
    pair_iou: torch.Tensor     # (n_pairs,) float64: every page's dense (predictions x annotations) IoU matrix, row-major, back to back
    pair_offs: list            # B + 1 host ints: page b's matrix starts at pair_iou[pair_offs[b]]


def _offsets(offs, n: int, who: str, what: str) -> list:
    """page offsets as host ints.  A list (or anything but a tensor) costs nothing; a device int32 tensor is read once (one wait); a CPU tensor
    is refused like every other CPU tensor"""
    if isinstance(offs, torch.Tensor):
        _need_cuda(offs, who)
        if offs.dtype != torch.int32 or offs.dim() != 1:
            raise RuntimeError(f"{who}: {what} must be (B + 1,) int32")
        offs = offs.tolist()
    offs = [int(o) for o in offs]
    if not offs or offs[0] != 0 or offs[-1] != n or any(b < a for a, b in zip(offs, offs[1:])):
        raise RuntimeError(f"{who}: {what} must ascend from 0 to the number of quads ({n})")
    return offs


def _pair_offsets(pred_offs: list, gt_offs: list, who: str) -> tuple[list, int]:
    if len(pred_offs) != len(gt_offs):
        raise RuntimeError(f"{who}: predictions and annotations must have the same pages")
    sizes = [(pred_offs[b + 1] - pred_offs[b]) * (gt_offs[b + 1] - gt_offs[b]) for b in range(len(pred_offs) - 1)]
    if len(sizes) > 65535:
        raise RuntimeError(f"{who}: at most 65535 pages per call")
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return offs, max(sizes, default=0)


def _match(pq, po_d, gq, go_d, ign, pair_offs_d, B, n_pairs, max_pairs, min_iou) -> tuple:
    """the two matching launches on device arrays whose sizes the host knows -> (gt_of_pred, pred_of_gt, iou_of_pred, pair_iou)"""
    dev, L = pq.device, lib()
    P, G = pq.shape[0], gq.shape[0]
    iou = torch.empty(max(n_pairs, 1), dtype=torch.float64, device=dev)
    hit = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    gop, pog = torch.empty(max(P, 1), dtype=torch.int32, device=dev), torch.empty(max(G, 1), dtype=torch.int32, device=dev)
    iop = torch.empty(max(P, 1), dtype=torch.float64, device=dev)
    ws = torch.empty(L.eval_match_ws_bytes(P, G), dtype=torch.uint8, device=dev)
    L.eval_pair_iou(ptr(pq), ptr(po_d), ptr(gq), ptr(go_d), ptr(ign), ptr(pair_offs_d), B, P, G, n_pairs, max_pairs, ptr(iou), ptr(hit))
    L.eval_match(ptr(iou), ptr(pair_offs_d), ptr(po_d), ptr(go_d), ptr(ign), ptr(hit), B, P, G, n_pairs, float(min_iou), ptr(gop), ptr(pog), ptr(iop), ptr(ws))
    return gop[:P], pog[:G], iop[:P], iou[:n_pairs]


def match_words(pred_quads: torch.Tensor, pred_offs, gt_quads: torch.Tensor, gt_offs, gt_ignore: torch.Tensor, min_iou: float = 0.5) -> Matches:
    """The greedy one-to-one assignment of predicted to annotated words of DESIGN.md §23, page by page, on the device.  ``pred_quads`` (P,4,2)
    and ``gt_quads`` (G,4,2) float32 device quads pooled over the pages, ``gt_ignore`` (G,) bool or uint8 on the device; ``pred_offs`` /
    ``gt_offs``: the B + 1 page offsets, as host ints (no wait at all) or as device int32 tensors (read once: one wait, to size the pages'
    IoU matrices).  A pair is a candidate when the annotation is not ignored and IoU > ``min_iou``; candidates are taken in the order (IoU
    descending, prediction ascending, annotation ascending) when both ends are free; an unmatched prediction more than half inside an ignored
    annotation is marked -2."""
    who = "match_words"
    pq, gq = _need_quads(pred_quads, who), _need_quads(gt_quads, who)
    _need_cuda(gt_ignore, who)
    if gt_ignore.dtype not in (torch.bool, torch.uint8) or tuple(gt_ignore.shape) != (gq.shape[0],):
        raise RuntimeError(f"{who}: gt_ignore must be (G,) bool or uint8")
    po, go = _offsets(pred_offs, pq.shape[0], who, "pred_offs"), _offsets(gt_offs, gq.shape[0], who, "gt_offs")
    pair_offs, max_pairs = _pair_offsets(po, go, who)
    B, dev = len(po) - 1, pq.device
    table = torch.tensor(po + go, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    pair_d = torch.tensor(pair_offs, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    ign = gt_ignore.contiguous().view(torch.uint8)
    return Matches(*_match(pq, table[:B + 1], gq, table[B + 1:], ign, pair_d, B, pair_offs[-1], max_pairs, min_iou), pair_offs)


def _predictions(results: list, level: str) -> tuple[list, list]:
    """(quads, texts) of one page's result list"""
    quads, texts = [], []
    for d in results:
        if level == "word" and "words" in d:
            if "word_texts" not in d:
                raise RuntimeError('OcrAccuracyStats.update: level="word" needs the words\' texts of line results: pass chars=True to the driver')
            quads += d["words"]
            texts += d["word_texts"]
        else:
            quads.append(d["quad"])
            texts.append(d["text"])
    return quads, texts


class _Packer:
    """host arrays laid out in one pinned buffer, 16-byte aligned, uploaded with one non-blocking copy"""

    def __init__(self):
        self.parts, self.size = [], 0

    def add(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        self.size = (self.size + 15) // 16 * 16
        self.parts.append((self.size, a))
        self.size += a.nbytes
        return len(self.parts) - 1

    def upload(self, dev) -> list:
        host = torch.empty(max(self.size, 16), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for off, a in self.parts:
            view[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        d = host.to(dev, non_blocking=True)
        return [d[off:off + a.nbytes].view(getattr(torch, a.dtype.name)).view(a.shape) for off, a in self.parts]


def _codes(texts: list) -> tuple[np.ndarray, np.ndarray]:
    """Unicode code points of the strings, pooled, with their n + 1 offsets"""
    offs = np.zeros(len(texts) + 1, dtype=np.int32)
    np.cumsum([len(t) for t in texts], out=offs[1:])
    return np.array([ord(c) for t in texts for c in t], dtype=np.int32), offs


class OcrAccuracyStats:
    """Running end-to-end accuracy on ``device``: twelve int64 counters (``COUNTERS``) that ``update`` adds to with integer atomics."""

    def __init__(self, device, min_iou: float = 0.5):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("OcrAccuracyStats needs a GPU device (the host restatement of the rule is tests/eval_ref.py)")
        self.min_iou = float(min_iou)
        self.state = torch.zeros(len(COUNTERS), dtype=torch.int64, device=self.device)
        self.last = None

    def update(self, results_per_page, truth_per_page, level: str = "word") -> None:
        """``results_per_page``: one result list per page, as ``ocr_pages`` returns them (or ``[ocr_page(...)]`` / ``[ocr_lines(...)]``);
        ``truth_per_page``: the ``WordTruth`` records of the same pages.  ``level="word"`` reads word dicts, or the ``words`` / ``word_texts``
        of line dicts (``chars=True``); ``level="line"`` reads line dicts against annotated lines.  One non-blocking upload from pinned memory,
        then the launches; no host wait.  ``self.last`` keeps the call's device outputs (``Matches``, dist, flags) for inspection."""
        if level not in ("word", "line"):
            raise RuntimeError('OcrAccuracyStats.update: level must be "word" or "line"')
        results_per_page, truth_per_page = list(results_per_page), list(truth_per_page)
        if len(results_per_page) != len(truth_per_page):
            raise RuntimeError("OcrAccuracyStats.update: one result list and one truth record per page")
        B = len(results_per_page)
        if B == 0:
            return
        pq, pt, po, gq, gt, gi, go = [], [], [0], [], [], [], [0]
        for res, truth in zip(results_per_page, truth_per_page):
            q, t = _predictions(res, level)
            pq += q
            pt += t
            po.append(len(pq))
            gq.append(np.asarray(truth.quads, dtype=np.float32).reshape(-1, 4, 2))
            gt += list(truth.texts)
            gi.append(np.asarray(truth.ignore, dtype=bool).reshape(-1))
            go.append(go[-1] + len(truth.texts))
            if not len(gq[-1]) == len(gi[-1]) == len(truth.texts):
                raise RuntimeError("OcrAccuracyStats.update: a truth record needs one quad, one text and one flag per word")
        P, G = len(pq), len(gt)
        pair_offs, max_pairs = _pair_offsets(po, go, "OcrAccuracyStats.update")
        ptext, ptoffs = _codes(pt)
        gtext, gtoffs = _codes(gt)
        pk = _Packer()
        for a in (np.asarray(pq, dtype=np.float32).reshape(-1, 4, 2), np.concatenate(gq) if gq else np.zeros((0, 4, 2), np.float32), np.concatenate(gi).astype(np.uint8),
                  np.array(po, dtype=np.int32), np.array(go, dtype=np.int32), np.array(pair_offs, dtype=np.int64), ptext, ptoffs, gtext, gtoffs):
            pk.add(a)
        pq_d, gq_d, ign, po_d, go_d, pair_d, ptext_d, ptoffs_d, gtext_d, gtoffs_d = pk.upload(self.device)
        gop, pog, iop, iou = _match(pq_d, po_d, gq_d, go_d, ign, pair_d, B, pair_offs[-1], max_pairs, self.min_iou)
        dev = self.device
        bnd = torch.empty(max(len(ptext), 1), dtype=torch.int32, device=dev)
        dist, flags = torch.empty(max(P, 1), dtype=torch.int32, device=dev), torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        lib().eval_text_update(ptr(po_d), ptr(go_d), ptr(ign), B, P, G, max(b - a for a, b in zip(po, po[1:])), ptr(gop), ptr(pog), ptr(ptext_d), ptr(ptoffs_d),
                               len(ptext), ptr(gtext_d), ptr(gtoffs_d), len(gtext), ptr(bnd), ptr(dist), ptr(flags), ptr(self.state))
        self.last = {"matches": Matches(gop, pog, iop, iou, pair_offs), "dist": dist[:P], "flags": flags[:P]}

    def counters(self) -> dict:
        """the raw counters as host ints (the one host wait)"""
        return dict(zip(COUNTERS, self.state.cpu().tolist()))

    def result(self) -> dict:
        return metrics(self.counters())


def _ratio(a: int, b: int, empty: float) -> float:
    return a / b if b > 0 else empty


def _f1(p: float, r: float) -> float:
    return 2 * p * r / (p + r) if p + r > 0 else 0.0


def metrics(c: dict) -> dict:
    """The derived numbers from the twelve counters (host arithmetic on integers).  Zero denominators follow ``box_match_metrics``: precision
    and recall of nothing are 1.0, a CER over zero characters is 0.0."""
    out = {}
    for name, hits in (("", c["matched"]), ("e2e_", c["exact"])):
        p, r = _ratio(hits, c["pred"], 1.0), _ratio(hits, c["gt"], 1.0)
        out.update({f"{name}precision": p, f"{name}recall": r, f"{name}f1": _f1(p, r)})
    p, r = _ratio(c["exact_ci"], c["pred"], 1.0), _ratio(c["exact_ci"], c["gt"], 1.0)
    out.update({"e2e_precision_ci": p, "e2e_recall_ci": r, "e2e_f1_ci": _f1(p, r)})
    out["cer_matched"] = _ratio(c["edit_sum"], c["gt_chars_matched"], 0.0)
    out["cer_page"] = _ratio(c["edit_sum"] + c["pred_chars_unmatched"] + c["gt_chars_unmatched"], c["gt_chars"], 0.0)
    out["counters"] = dict(c)
    return out


def evaluate_pages(det_model, rec_model, pages, truth, level: str = "word", batch_pages: int = 8, min_iou: float = 0.5, **ocr_options) -> dict:
    """``ocr_pages`` over ``pages`` (a list of (1,H,W) uint8 device pages) in batches of ``batch_pages``, scored against ``truth`` (one
    ``WordTruth`` per page) -> the dict of ``OcrAccuracyStats.result``.  Word level forces ``lines=True, chars=True`` (the words' texts come
    from the lines' characters); every other option -- ``beam_width``, ``lm``, ``rectify``, ``tile``, ``overlap``, ``orientation``,
    ``reading_order``, ... -- reaches ``ocr_pages`` untouched."""
    pages, truth = list(pages), list(truth)
    if len(pages) != len(truth):
        raise RuntimeError("evaluate_pages: one truth record per page")
    if batch_pages < 1:
        raise RuntimeError("evaluate_pages: batch_pages must be at least 1")
    if not pages:
        raise RuntimeError("evaluate_pages: no pages")
    opts = dict(ocr_options)
    if level == "word":
        opts.update(lines=True, chars=True)
    elif level == "line":
        opts.update(lines=True)
    else:
        raise RuntimeError('evaluate_pages: level must be "word" or "line"')
    per_page = opts.get("orientation")
    stats = OcrAccuracyStats(pages[0].device, min_iou)
    for k in range(0, len(pages), batch_pages):
        if isinstance(per_page, list):
            opts["orientation"] = per_page[k:k + batch_pages]
        stats.update(drivers.ocr_pages(det_model, rec_model, pages[k:k + batch_pages], **opts), truth[k:k + batch_pages], level)
    return stats.result()

"""Host restatement of the end-to-end accuracy of page OCR (the device stage is csrc/ocr_eval.hip, the Python surface
ocrs_models_amd/inference/evaluate.py), in numpy and plain Python:

* IoU through ``postprocess.quad_intersection_area`` and ``_area``, with the strict bounding-box test and the operations of
  ``box_match_metrics``;
* the greedy one-to-one matching as a literal sort-and-take loop (``greedy_match``), and an exhaustive search for the same rule
  (``exhaustive_match``: of all one-to-one matchings, the one whose pairs, listed in the total order, come first);
* the ignore rule;
* a dynamic-programming Levenshtein on code points;
* the twelve counters and the derived metrics."""
from __future__ import annotations

import numpy as np

from ocrs_models_amd.postprocess import _area, quad_intersection_area

COUNTERS = ("pages", "pred", "gt", "pred_ignored", "matched", "exact", "exact_ci", "edit_sum", "gt_chars_matched", "pred_chars_unmatched",
            "gt_chars_unmatched", "gt_chars")


def pair_geometry(pred, gt):
    """(iou, inter, pa) of float32 quads pred (P,4,2) and gt (G,4,2) in float64: iou (P,G) with 0.0 wherever no intersection is computed or
    it is not positive"""
    P = np.asarray(pred, dtype=np.float32).astype(np.float64).reshape(-1, 4, 2)
    T = np.asarray(gt, dtype=np.float32).astype(np.float64).reshape(-1, 4, 2)
    pa = np.array([_area(p) for p in P])
    ta = np.array([_area(t) for t in T])
    inter = np.zeros((len(P), len(T)))
    iou = np.zeros((len(P), len(T)))
    if len(P) and len(T):
        pmin, pmax, tmin, tmax = P.min(1), P.max(1), T.min(1), T.max(1)
        cand = ((pmin[:, None, :] < tmax[None, :, :]) & (tmin[None, :, :] < pmax[:, None, :])).all(-1)
        for i, j in zip(*np.nonzero(cand)):
            inter[i, j] = quad_intersection_area(P[i], T[j])
            if inter[i, j] > 0:
                iou[i, j] = inter[i, j] / (pa[i] + ta[j] - inter[i, j])
    return iou, inter, pa


def candidates(iou, ignore, min_iou=0.5):
    """the candidate pairs in the total order (IoU descending, prediction ascending, annotation ascending)"""
    c = [(i, j) for i in range(iou.shape[0]) for j in range(iou.shape[1]) if not ignore[j] and iou[i, j] > min_iou]
    return sorted(c, key=lambda ij: (-iou[ij], ij[0], ij[1]))


def greedy_match(iou, ignore, min_iou=0.5):
    """-> (gt_of_pred, pred_of_gt) with -1 = unmatched: take every candidate, in order, whose ends are both free"""
    gop, pog = [-1] * iou.shape[0], [-1] * iou.shape[1]
    for i, j in candidates(iou, ignore, min_iou):
        if gop[i] == -1 and pog[j] == -1:
            gop[i], pog[j] = j, i
    return gop, pog


def exhaustive_match(iou, ignore, min_iou=0.5):
    """The same rule without the loop: every one-to-one matching is the ascending list of its pairs' ranks in the total order; the rule's
    matching is the first of these lists, a list counting as later than any list it is the beginning of."""
    order = candidates(iou, ignore, min_iou)
    rank = {ij: k for k, ij in enumerate(order)}
    P, G = iou.shape
    best = [None, None]

    def walk(i, used, pairs):
        if i == P:
            key = sorted(rank[p] for p in pairs) + [len(order)]  # the sentinel makes a beginning later than its continuations
            if best[0] is None or key < best[0]:
                best[0], best[1] = key, list(pairs)
            return
        walk(i + 1, used, pairs)
        for j in range(G):
            if (i, j) in rank and j not in used:
                walk(i + 1, used | {j}, pairs + [(i, j)])

    walk(0, frozenset(), [])
    gop, pog = [-1] * P, [-1] * G
    for i, j in best[1]:
        gop[i], pog[j] = j, i
    return gop, pog


def match_page(pred, gt, ignore, min_iou=0.5):
    """-> dict(gt_of_pred (with -2 = ignored), pred_of_gt, iou_of_pred, iou)"""
    iou, inter, pa = pair_geometry(pred, gt)
    ignore = np.asarray(ignore, dtype=bool).reshape(-1)
    gop, pog = greedy_match(iou, ignore, min_iou)
    iop = [float(iou[i, j]) if j >= 0 else 0.0 for i, j in enumerate(gop)]
    for i in range(len(gop)):
        if gop[i] == -1 and any(ignore[j] and inter[i, j] > 0 and inter[i, j] / pa[i] > 0.5 for j in range(len(pog))):
            gop[i] = -2
    return {"gt_of_pred": gop, "pred_of_gt": pog, "iou_of_pred": iop, "iou": iou}


def closest_gap(iou, ignore, min_iou=0.5, ties=()):
    """The margin that keeps a last-bit difference from flipping a decision: the smallest distance between two candidate IoUs of a page
    (pairs of a not ignored annotation with IoU > min_iou) or between any positive IoU of such a pair and min_iou.  ``ties``: groups of
    (i, j) pairs that are equal on purpose (bit-identical quads); a group must be exactly equal and counts as one value."""
    live = [(i, j) for i in range(iou.shape[0]) for j in range(iou.shape[1]) if not ignore[j] and iou[i, j] > 0]
    gap = min((abs(float(iou[ij]) - min_iou) for ij in live), default=np.inf)
    tied = {ij for group in ties for ij in group}
    vals = [float(iou[ij]) for ij in live if iou[ij] > min_iou and ij not in tied]
    for group in ties:
        assert len({float(iou[ij]) for ij in group}) == 1, "a declared tie is not exact"
        if iou[group[0]] > min_iou:
            vals.append(float(iou[group[0]]))
    vals.sort()
    return min([gap] + [b - a for a, b in zip(vals, vals[1:])])


def levenshtein(a, b) -> int:
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


def fold_ascii(s: str) -> str:
    return "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in s)


def text_pair(pred: str, gt: str):
    """(distance, flags): flags = 1 (equal) | 2 (equal after folding ASCII A-Z only)"""
    return levenshtein([ord(c) for c in pred], [ord(c) for c in gt]), int(pred == gt) | (2 * int(fold_ascii(pred) == fold_ascii(gt)))


def evaluate(pred_pages, truth_pages, min_iou=0.5):
    """pred_pages: [(quads, texts)], truth_pages: [(quads, texts, ignore)] -> (per-page dicts of match_page + dist + flags, counters)"""
    c = dict.fromkeys(COUNTERS, 0)
    pages = []
    for (pq, pt), (gq, gt, gi) in zip(pred_pages, truth_pages):
        m = match_page(pq, gq, gi, min_iou)
        m["dist"], m["flags"] = [], []
        c["pages"] += 1
        for i, j in enumerate(m["gt_of_pred"]):
            d, f = text_pair(pt[i], gt[j]) if j >= 0 else (-1, 0)
            m["dist"].append(d), m["flags"].append(f)
            if j == -2:
                c["pred_ignored"] += 1
                continue
            c["pred"] += 1
            if j == -1:
                c["pred_chars_unmatched"] += len(pt[i])
                continue
            c["matched"] += 1
            c["exact"] += f & 1
            c["exact_ci"] += f >> 1
            c["edit_sum"] += d
            c["gt_chars_matched"] += len(gt[j])
        for j, i in enumerate(m["pred_of_gt"]):
            if gi[j]:
                continue
            c["gt"] += 1
            c["gt_chars"] += len(gt[j])
            if i < 0:
                c["gt_chars_unmatched"] += len(gt[j])
        pages.append(m)
    return pages, c


def metrics(c: dict) -> dict:
    def ratio(a, b, empty):
        return a / b if b > 0 else empty

    def prf(hits):
        p, r = ratio(hits, c["pred"], 1.0), ratio(hits, c["gt"], 1.0)
        return p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)

    out = dict(zip(("precision", "recall", "f1"), prf(c["matched"])))
    out.update(zip(("e2e_precision", "e2e_recall", "e2e_f1"), prf(c["exact"])))
    out.update(zip(("e2e_precision_ci", "e2e_recall_ci", "e2e_f1_ci"), prf(c["exact_ci"])))
    out["cer_matched"] = ratio(c["edit_sum"], c["gt_chars_matched"], 0.0)
    out["cer_page"] = ratio(c["edit_sum"] + c["pred_chars_unmatched"] + c["gt_chars_unmatched"], c["gt_chars"], 0.0)
    return out

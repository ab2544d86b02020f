"""Orientation (csrc/page_orient.hip, C ABI section "orientation"; restated for the tests in tests/orient_ref.py): pages
scanned sideways or upside down.  ``orientation = k``, k in 0..3, means the upright page is ``torch.rot90(page, k, dims=(-2, -1))``: k quarter
turns counter-clockwise.  A point (x, y) of the turned page of a page of H rows and W columns lies on the original page at

    k = 0: (x, y)    k = 1: ((W-1) - y, x)    k = 2: ((W-1) - x, (H-1) - y)    k = 3: (y, (H-1) - x)

(pixel centres; proper rotations, so corner j of a quad stays corner j).  ``turn_page`` and ``turn_quads`` are the turn and the table on the
device, ``orientation_votes`` and ``page_orientation`` the decision among the four turns, ``turn_results`` the table on the result dicts of the
drivers."""
from __future__ import annotations

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda
from . import crops, detect
from .args import _need_counts, _need_quads, _to_device_async, _to_host_async

COORD_KEYS = ("quad", "words", "char_quads", "spine")  # the keys of a result dict that hold page coordinates


def _check_turns(who: str, k, auto: bool = False):
    """an orientation: an int 0..3 (not a bool), or with ``auto`` the string "auto" """
    if auto and isinstance(k, str) and k == "auto":
        return k
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 3:
        what = 'None, "auto" or an int in 0..3' if auto else "an int in 0..3"
        raise RuntimeError(f"{who}: orientation must be {what} (the quarter turns counter-clockwise that make the page upright)")
    return k


def _check_orientation(who: str, orientation, pages: int | None = None):
    """the ``orientation`` keyword of a driver -> None, "auto", an int, or with ``pages`` (``ocr_pages``) a list of one entry per page"""
    if orientation is None:
        return None
    if pages is not None and isinstance(orientation, (list, tuple)):
        if len(orientation) != pages:
            raise RuntimeError(f"{who}: an orientation list needs one entry per page ({pages}), got {len(orientation)}")
        return [_check_turns(who, k, True) for k in orientation]
    return _check_turns(who, orientation, True)


def _check_turn_page(page_u8, who: str):
    if not isinstance(page_u8, torch.Tensor):
        raise RuntimeError(f"{who}: expected a (1,H,W) or (H,W) uint8 page on the device")
    _need_cuda(page_u8, who)
    if page_u8.dtype != torch.uint8 or not (page_u8.dim() == 2 or (page_u8.dim() == 3 and page_u8.shape[0] == 1)) or min(page_u8.shape[-2:]) < 1:
        raise RuntimeError(f"{who}: expected a (1,H,W) or (H,W) uint8 page")
    if not page_u8.is_contiguous():
        raise RuntimeError(f"{who}: the page must be contiguous (the turn is one pass over its bytes; a hidden copy would be a second)")


def turn_shape(H: int, W: int, k: int) -> tuple[int, int]:
    """(rows, columns) of an (H,W) page turned by k quarter turns"""
    return (H, W) if k % 2 == 0 else (W, H)


def turn_page(page_u8: torch.Tensor, k: int) -> torch.Tensor:
    """``torch.rot90(page_u8, k, dims=(-2, -1))`` of a contiguous (1,H,W) or (H,W) uint8 device page, as a contiguous tensor with the same
    number of dims: one pass over the page's bytes (k = 1, 3: a tiled transpose; k = 2: a reversed copy).  k = 0 returns the input itself.
    No synchronisation."""
    _check_turns("turn_page", k)
    _check_turn_page(page_u8, "turn_page")
    if k == 0:
        return page_u8
    H, W = (int(v) for v in page_u8.shape[-2:])
    shape = turn_shape(H, W, k)
    out = torch.empty(shape if page_u8.dim() == 2 else (1, *shape), dtype=torch.uint8, device=page_u8.device)
    lib().turn_page_u8(ptr(page_u8), H, W, k, ptr(out))
    return out


def turn_quads(quads: torch.Tensor, k: int, H: int, W: int, inverse: bool = False, count: torch.Tensor | None = None) -> torch.Tensor:
    """The module's point table on (N,4,2) fp32 device quads, for a page whose ORIGINAL has H rows and W columns: quads on the turned page
    -> quads on the original page, or with ``inverse`` the other way.  One fp32 operation per coordinate, corner j -> corner j.  ``count``
    (1,) int32 on the device: only the first ``min(count, N)`` rows are written (the others are left as allocated).  No synchronisation."""
    _check_turns("turn_quads", k)
    q = _need_quads(quads, "turn_quads")
    if count is not None:
        count = _need_counts(count, "turn_quads")
    H, W = int(H), int(W)
    if not (1 <= H <= 1 << 24 and 1 <= W <= 1 << 24):
        raise RuntimeError("turn_quads: H and W must be in 1 .. 2^24")
    out = torch.empty_like(q)
    lib().turn_quads(ptr(q), q.shape[0], ptr(count), H, W, k, int(bool(inverse)), ptr(out))
    return out


def orientation_votes(quads: torch.Tensor, count: torch.Tensor | None = None, min_aspect: float = 1.5, sample: int = 64):
    """The axis vote over (N,4,2) fp32 device word quads -> ``(sums, counts, picks)`` on the device: ``sums`` (2,) fp64 = (H, V), the lengths
    of the long sides of the voting quads that run along x and along y; ``counts`` (2,) int32 = (voters, K = min(sample, voters)); ``picks``
    (sample,) int32 = the K voters with the longest long side, ties by the smaller index, then -1.  A quad votes if its short side is > 0
    and its long side at least ``min_aspect`` times the short one (near-square components are dots and single characters and say nothing
    about direction).  The sums are taken in a fixed order: equal input gives equal bytes.  No synchronisation."""
    q = _need_quads(quads, "orientation_votes")
    if count is not None:
        count = _need_counts(count, "orientation_votes")
    if isinstance(sample, bool) or not isinstance(sample, int) or sample < 1:
        raise RuntimeError("orientation_votes: sample must be an int >= 1")
    votes = torch.empty(3, dtype=torch.float64, device=q.device)  # 2 fp64 sums, then 2 int32 counts in the third element's bytes
    picks = torch.empty(sample, dtype=torch.int32, device=q.device)
    lib().orient_votes(ptr(q), q.shape[0], ptr(count), float(min_aspect), sample, ptr(votes), ptr(picks))
    return votes[:2], votes[2:].view(torch.int32), picks


def path_confidence(log_probs: torch.Tensor, steps: torch.Tensor) -> torch.Tensor:
    """(T,B,C) fp32 device log-probs and (B,) int32 valid time steps -> (B,) fp64: the mean over t < steps[b] of max_c log_probs[t, b, c],
    the log-prob per step of the best alignment -- what the greedy decode follows.  No synchronisation."""
    _need_cuda(log_probs, "path_confidence")
    _need_cuda(steps, "path_confidence")
    if log_probs.dtype != torch.float32 or log_probs.dim() != 3 or log_probs.shape[0] < 1 or log_probs.shape[2] < 1:
        raise RuntimeError("path_confidence: expected (T,B,C) float32 log-probs")
    T, B, C = log_probs.shape
    if steps.dtype != torch.int32 or tuple(steps.shape) != (B,):
        raise RuntimeError("path_confidence: steps must be (B,) int32 on the device")
    scores = torch.empty(B, dtype=torch.float64, device=log_probs.device)
    lib().path_confidence(ptr(log_probs.contiguous()), T, B, C, ptr(steps.contiguous()), ptr(scores))
    return scores


def _wait_for_copies(device):
    """wait for what the current stream holds up to here -- the host copies just queued -- by an event of its own"""
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(device))
    done.synchronize()


def probe_batches(page_u8: torch.Tensor, quads: torch.Tensor, a: int, output_height: int = 64, max_batch: int = 256, width_unit: int = 64):
    """The probe's crops: the K ``quads`` (on the page as given) cut from ``turn_page(page, a)`` and from ``turn_page(page, a + 2)`` through a
    two-page store, one plan over the 2K quads (the first K from the first page), ``rectify_crops_pages`` and ``crops_to_batches`` -> the
    batches.  One host synchronisation (the plan's totals)."""
    H, W = (int(v) for v in page_u8.shape[-2:])
    page = page_u8 if page_u8.dim() == 3 else page_u8[None]
    K = quads.shape[0]
    store = detect.pack_pages([turn_page(page, a), turn_page(page, a + 2)])
    both = torch.cat([turn_quads(quads, a, H, W, inverse=True), turn_quads(quads, a + 2, H, W, inverse=True)])
    page_of_quad = _to_device_async([0] * K + [1] * K, torch.int32, page.device)
    plan = crops.crop_plan(both, output_height)
    totals_h, table_h = _to_host_async(plan.totals), _to_host_async(plan.table)
    _wait_for_copies(page.device)
    plan._host, plan._host_table = totals_h.tolist(), table_h  # what ``plan.host()`` would fetch: the probe's one wait here
    if max(plan._host[1:4]) >= 2 ** 31:
        raise RuntimeError("page_orientation: the probe's crops do not fit 32-bit offsets (use a smaller sample)")
    return crops.crops_to_batches(crops.rectify_crops_pages(*store, both, page_of_quad, plan), plan, max_batch, width_unit)


def page_orientation(det_model, rec_model, page_u8: torch.Tensor, size=detect.MASK_SIZE, threshold: float = 0.5, expand: float = detect.SHRINK_DISTANCE,
                     output_height: int = 64, max_batch: int = 256, width_unit: int = 64, min_aspect: float = 1.5, sample: int = 64, tile=None,
                     overlap=None, tile_batch: int = 16, det: dict | None = None) -> dict:
    """Which of the four turns makes the (1,H,W) uint8 device page upright -> ``{"turns": k, "votes": (H, V), "voters": n, "sampled": K,
    "scores": (S_a, S_a2), "det": det}``.

    1. ``det`` is ``detect_words`` on the page as given (or the passed one).  Without words or without voters: turns 0, scores None.
    2. The axis: ``orientation_votes`` over the word quads; a = 1 if V > H (strictly), else 0.
    3. The sign: the K picked quads are cut from ``turn_page(page, a)`` and from ``turn_page(page, a + 2)`` (``probe_batches``), the
       recogniser's eval forward runs on those crops and every crop gets its ``path_confidence``; S_a and S_a2 are the means of the K scores
       of each side, summed in pick order in fp64.  turns = a + 2 if S_a2 > S_a (strictly), else a.

    Host synchronisations beyond the detection's own: at most three (the votes, the probe plan's totals, the scores)."""
    _check_turn_page(page_u8, "page_orientation")
    if page_u8.dim() != 3:
        raise RuntimeError("page_orientation: expected a (1,H,W) uint8 page")
    if rec_model.training:
        raise RuntimeError("page_orientation: the model must be in eval mode (model.eval())")
    if isinstance(sample, bool) or not isinstance(sample, int) or sample < 1:
        raise RuntimeError("page_orientation: sample must be an int >= 1")
    if det is None:
        det = detect.detect_words(det_model, page_u8, size, threshold, expand, tile, overlap, tile_batch)
    out = {"turns": 0, "votes": (0.0, 0.0), "voters": 0, "sampled": 0, "scores": None, "det": det}
    if det["n"] == 0:
        return out
    sums, counts, picks = orientation_votes(det["quads"], None, min_aspect, sample)
    sums_h, counts_h, picks_h = _to_host_async(sums), _to_host_async(counts), _to_host_async(picks)
    _wait_for_copies(page_u8.device)
    (h, v), (voters, K) = sums_h.tolist(), counts_h.tolist()
    out.update(votes=(h, v), voters=voters, sampled=K)
    if voters == 0:
        return out
    a = 1 if v > h else 0
    picked = det["quads"].index_select(0, picks[:K].long())
    batches, image_widths, perm = probe_batches(page_u8, picked, a, output_height, max_batch, width_unit)
    with torch.inference_mode():
        lps = [rec_model(img) for img in batches]
    scores = torch.cat([path_confidence(lp, iw.div(4, rounding_mode="floor").int()) for lp, iw in zip(lps, image_widths)])
    scores_h = _to_host_async(scores)
    _wait_for_copies(page_u8.device)
    by_quad = [scores_h[p].item() for p in perm]  # quad order: the K picks on the page turned by a, then the same on a + 2
    s_a = s_a2 = 0.0
    for i in range(K):  # (a plain loop: one fp64 addition per score, in pick order)
        s_a, s_a2 = s_a + by_quad[i], s_a2 + by_quad[K + i]
    s_a, s_a2 = s_a / K, s_a2 / K
    out.update(turns=a + 2 if s_a2 > s_a else a, scores=(s_a, s_a2))
    return out


def _turn_point(k: int, H: int, W: int):
    """the table as a function of a point ``[x, y]`` of Python floats"""
    if k == 1:
        return lambda p: [(W - 1) - p[1], p[0]]
    if k == 2:
        return lambda p: [(W - 1) - p[0], (H - 1) - p[1]]
    if k == 3:
        return lambda p: [p[1], (H - 1) - p[0]]
    return lambda p: [p[0], p[1]]


def _turn_nested(v, f):
    if len(v) == 2 and not isinstance(v[0], (list, tuple)):
        return f(v)
    return [_turn_nested(e, f) for e in v]


def turn_results(results: list, k: int, H: int, W: int) -> list:
    """The result dicts of a driver that read ``turn_page(page, k)`` -> the same dicts on the page the caller passed, H rows by W columns:
    every point under ``"quad"``, ``"words"``, ``"char_quads"`` and ``"spine"`` goes through the module's table on the Python floats; texts,
    ranges, heights, blocks and scores are untouched; every dict gains ``"turns": k``.  Host work only."""
    f = _turn_point(k, int(H), int(W))
    return [{**{key: (_turn_nested(val, f) if key in COORD_KEYS else val) for key, val in d.items()}, "turns": k} for d in results]


def _upright(who: str, det_model, rec_model, page_u8: torch.Tensor, orientation, probe: dict):
    """``orientation`` (an int or "auto", already checked) of a single-page driver -> ``(the page to read, turns, det or None)``: with
    "auto" ``page_orientation(**probe)`` decides, and where it finds 0 turns its detection is handed on (the page is detected once)."""
    _check_turn_page(page_u8, who)
    det = None
    if orientation == "auto":
        found = page_orientation(det_model, rec_model, page_u8, **probe)
        orientation, det = found["turns"], (found["det"] if found["turns"] == 0 else None)
    return turn_page(page_u8, orientation), orientation, det

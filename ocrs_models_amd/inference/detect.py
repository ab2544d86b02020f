"""Detection: from a page, or a batch of pages, to expanded word quads."""
from __future__ import annotations

import torch

from .._lib import lib, ptr
from ..input_pipeline import _need_cuda, resize, transform_image
from .args import _check_pages, _need_counts, _need_quads, _to_device_async, _to_host_async
from .tiles import _check_tile_args, _detect_tiles

MASK_SIZE = (800, 600)   # train_detection.py's mask_size: the size the detection model is trained and evaluated at
SHRINK_DISTANCE = 3.0    # datasets/util.py: how far text polygons are shrunk when training masks are made


def binarize_resize(prob: torch.Tensor, size, threshold: float = 0.5) -> torch.Tensor:
    """(B,1,h,w) or (h,w) fp32 probabilities -> uint8 0/1 mask (B,1,H,W) or (H,W): ``binarize_mask`` followed by
    ``resize(.., size, InterpolationMode.NEAREST)`` (eval_detection.py:54-57) in one launch."""
    _need_cuda(prob, "binarize_resize")
    if prob.dtype != torch.float32 or not (prob.dim() == 2 or (prob.dim() == 4 and prob.shape[1] == 1)):
        raise RuntimeError("binarize_resize: expected (B,1,h,w) or (h,w) float32 probabilities")
    H, W = int(size[0]), int(size[1])
    h, w = prob.shape[-2:]
    B = prob.shape[0] if prob.dim() == 4 else 1
    src = prob.contiguous()
    out = torch.empty((B, 1, H, W) if prob.dim() == 4 else (H, W), dtype=torch.uint8, device=prob.device)
    lib().binarize_resize_nearest(ptr(src), ptr(out), B, h, w, H, W, float(threshold))
    return out


def expand_quads(quads: torch.Tensor, dist: float, counts: torch.Tensor | None = None) -> torch.Tensor:
    """``expand_quads`` (postprocess.py:68-76) on the device: (N,4,2) or (B,cap,4,2) fp32 -> the same shape, every rectangle's edges moved
    outward by ``dist``.  ``counts`` (B,) int32 on the device: rows past ``counts[b]`` are returned as they came."""
    q = _need_quads(quads, "expand_quads", "(B,cap,4,2)" if quads.dim() == 4 else "(N,4,2)")
    B, cap = (1, q.shape[0]) if q.dim() == 3 else (q.shape[0], q.shape[1])
    if counts is None:
        out = torch.empty_like(q)
    else:
        counts = _need_counts(counts, "expand_quads", B)
        out = q.clone()
    lib().expand_quads(ptr(q), ptr(out), ptr(counts), B, cap, float(dist))
    return out


def detect_words(model, page_u8: torch.Tensor, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE, tile=None, overlap=None,
                 tile_batch: int = 16) -> dict:
    """eval_detection.py:32-67 for one (1,H,W) uint8 page on the device -> ``probs`` (h,w), ``text_mask`` (H,W) uint8, ``quads`` (N,4,2) in
    page coordinates and ``n``.  The model must be in eval mode.  One host synchronisation (the component count).
    ``tile = (Th, Tw)``: detect in overlapping tiles of that many page pixels instead of squeezing the whole page to ``size``:
    every window of ``tile_plan(H, W, tile, overlap)`` is resized to ``size`` on its own, the eval forward runs over the tiles in chunks of
    at most ``tile_batch``, and the tile probabilities are composed into ONE page mask -- every pixel from the tile that owns it -- before the
    components are labelled, so a word across a seam stays one word.  ``probs`` becomes (T,h,w) and the dict gains ``tiles``, the (T,5) int32
    device table ``(page, y0, x0, th, tw)``.  ``overlap=None``: an eighth of the tile.  ``tile=None``, the default, is the path above unchanged;
    the same one synchronisation either way."""
    from ..postprocess import extract_cc_quads_device

    _need_cuda(page_u8, "detect_words")
    if page_u8.dtype != torch.uint8 or page_u8.dim() != 3 or page_u8.shape[0] != 1:
        raise RuntimeError("detect_words: expected a (1,H,W) uint8 page")
    if model.training:
        raise RuntimeError("detect_words: the model must be in eval mode (model.eval())")
    _check_tile_args("detect_words", tile, tile_batch)
    H, W = (int(v) for v in page_u8.shape[-2:])
    extra = {}
    if tile is None:
        img = resize(transform_image(page_u8), size)
        with torch.inference_mode():
            probs = model(img.unsqueeze(0))[0, 0]
        text_mask = binarize_resize(probs, (H, W), threshold)
    else:
        if H < 1 or W < 1:
            raise RuntimeError("detect_words: a tiled page needs at least one pixel")
        dev = page_u8.device
        store = (page_u8.contiguous().view(-1), _to_device_async([0], torch.int64, dev), _to_device_async([[H, W]], torch.int32, dev))  # the page is its own store
        probs, masks, tables = _detect_tiles(model, store, [(H, W)], (H, W), size, threshold, tile, overlap, tile_batch, "detect_words")
        text_mask, extra = masks[0], {"tiles": tables.tiles}
    quads = expand_quads(extract_cc_quads_device(text_mask), expand)
    return {"probs": probs, "text_mask": text_mask, "quads": quads, "n": quads.shape[0], **extra}


def pack_pages(pages):
    """A list of (1,H_p,W_p) uint8 device pages -> ``(pages_packed, page_offs, page_sizes)``: the pages back to back in one uint8 buffer
    (one device-to-device copy each), their byte offsets (B,) int64 and their ``(h, w)`` (B,2) int32 on the device -- the layout of the page
    stores of ``datasets/pages.py``.  No synchronisation."""
    pages = _check_pages(pages, "pack_pages")
    if not pages:
        raise RuntimeError("pack_pages: expected at least one page")
    dev = pages[0].device
    sizes = [(int(p.shape[1]), int(p.shape[2])) for p in pages]
    offs, off = [], 0
    for h, w in sizes:
        offs.append(off)
        off += h * w
    packed = torch.empty(off, dtype=torch.uint8, device=dev)
    for p, o, (h, w) in zip(pages, offs, sizes):
        packed[o:o + h * w].view(1, h, w).copy_(p)
    return packed, _to_device_async(offs, torch.int64, dev), _to_device_async(sizes, torch.int32, dev)


def binarize_resize_pages(probs: torch.Tensor, page_sizes: torch.Tensor, canvas, threshold: float = 0.5) -> torch.Tensor:
    """(B,h,w) fp32 probabilities and (B,2) int32 device page sizes ``(H_p, W_p)`` -> the uint8 canvas (B,Hmax,Wmax), ``canvas = (Hmax, Wmax)``
    at least as large as every page: ``binarize_resize(probs[p], (H_p, W_p))`` in the top left corner of plane p and 0 elsewhere, in one
    launch that writes the padding too."""
    _need_cuda(probs, "binarize_resize_pages")
    _need_cuda(page_sizes, "binarize_resize_pages")
    if probs.dtype != torch.float32 or probs.dim() != 3:
        raise RuntimeError("binarize_resize_pages: expected (B,h,w) float32 probabilities")
    B, h, w = probs.shape
    if page_sizes.dtype != torch.int32 or tuple(page_sizes.shape) != (B, 2):
        raise RuntimeError("binarize_resize_pages: page_sizes must be (B,2) int32 on the device")
    Hmax, Wmax = int(canvas[0]), int(canvas[1])
    out = torch.empty(B, Hmax, Wmax, dtype=torch.uint8, device=probs.device)
    lib().binarize_resize_pages(ptr(probs.contiguous()), ptr(page_sizes.contiguous()), ptr(out), B, h, w, Hmax, Wmax, float(threshold))
    return out


def gather_page_quads(quads: torch.Tensor, counts: torch.Tensor):
    """Quads (B,cap,4,2) fp32 with device counts (B,) int32, as ``ocrs_cc_quads`` writes them -> ``(flat quads (N_total,4,2), page_of_word
    (N_total,) int32, word_offs (B+1,) int32, counts as a host list)``: the rows of every page back to back in their own (raster) order.
    Reading ``word_offs`` to size the flat rows is the one host synchronisation; it stands for the B waits for component counts."""
    q = _need_quads(quads, "gather_page_quads", "(B,cap,4,2)")
    B, cap = q.shape[:2]
    counts = _need_counts(counts, "gather_page_quads", B)
    L = lib()
    word_offs = torch.empty(B + 1, dtype=torch.int32, device=q.device)
    L.gather_page_quads(ptr(q), ptr(counts), B, cap, None, None, ptr(word_offs), 0)
    offs_h = _to_host_async(word_offs)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(q.device))
    done.synchronize()  # (waits for the copy only, not for whatever else the stream holds)
    offs = offs_h.tolist()
    n = offs[B]
    flat = torch.empty(n, 4, 2, dtype=torch.float32, device=q.device)
    page_of_word = torch.empty(n, dtype=torch.int32, device=q.device)
    if n:
        L.gather_page_quads(ptr(q), ptr(counts), B, cap, ptr(flat), ptr(page_of_word), ptr(word_offs), n)
    return flat, page_of_word, word_offs, [b - a for a, b in zip(offs, offs[1:])]


def _cc_quads_pages_sizes(B: int, H: int, W: int):
    L = lib()
    ws_bytes, cap = L.cc_quads_ws_bytes(B, H, W), L.cc_quads_capacity(H, W)
    if ws_bytes <= 0 or B > 65535 or B * cap >= 2 ** 31:
        raise ValueError(f"a batch of {B} masks of {H}x{W} is not supported")
    return ws_bytes, cap


def cc_quads_pages(text_masks: torch.Tensor):
    """``extract_cc_quads_device`` for the (B,Hmax,Wmax) uint8 canvas of ``binarize_resize_pages``: ``ocrs_cc_quads`` on the whole canvas, then
    ``gather_page_quads`` -> ``(quads (N_total,4,2), page_of_word, word_offs, counts)``.  The padding is background, so page p's rows are the
    quads of its own mask in their own order.  One host synchronisation."""
    _need_cuda(text_masks, "cc_quads_pages")
    if text_masks.dtype != torch.uint8 or text_masks.dim() != 3:
        raise RuntimeError("cc_quads_pages: expected a (B,Hmax,Wmax) uint8 canvas")
    B, H, W = text_masks.shape
    ws_bytes, cap = _cc_quads_pages_sizes(B, H, W)
    m = text_masks.contiguous()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=m.device)
    ncomp = torch.empty(B, dtype=torch.int32, device=m.device)
    raw = torch.empty(B, cap, 4, 2, dtype=torch.float32, device=m.device)
    lib().cc_quads(ptr(m), 1, 0.5, B, H, W, ptr(ncomp), ptr(raw), None, ptr(ws))
    return gather_page_quads(raw, ncomp)


def detect_words_batch(model, pages, size=MASK_SIZE, threshold: float = 0.5, expand: float = SHRINK_DISTANCE, tile=None, overlap=None,
                       tile_batch: int = 16, _store=None) -> dict:
    """``detect_words`` for a list of (1,H_p,W_p) uint8 device pages of any sizes: one eval forward of the (B,1,h,w) batch of
    ``resize(transform_image(page), size)``, the masks of all pages in one zero-padded canvas, ``ocrs_cc_quads`` on the canvas, the quads
    compacted and expanded.  -> ``probs`` (B,h,w), ``text_masks`` (B,Hmax,Wmax) uint8, ``quads`` (N_total,4,2) grouped by page in raster order,
    ``page_of_word`` (N_total,) int32, ``word_offs`` (B+1,) int32 and ``counts``, the words per page as a host list.  One host synchronisation
    (the word offsets).  A canvas ``ocrs_cc_quads`` cannot take raises ValueError, as ``extract_cc_quads_device`` does.
    ``tile``: detect every page in overlapping tiles of that many page pixels, as ``detect_words`` describes; the tiles of all
    pages are cut in one call and pooled into the forward chunks; ``probs`` becomes (T,h,w) and the dict gains ``tiles`` (T,5) int32 and
    ``tile_offs`` (B+1,) int32 (page p's tiles are ``tile_offs[p]:tile_offs[p + 1]``).  None, the default, is the path above unchanged; the
    same one synchronisation either way."""
    pages = _check_pages(pages, "detect_words_batch")
    if not pages:
        raise RuntimeError("detect_words_batch: expected at least one page")
    if model.training:
        raise RuntimeError("detect_words_batch: the model must be in eval mode (model.eval())")
    _check_tile_args("detect_words_batch", tile, tile_batch)
    dev = pages[0].device
    sizes = [(int(p.shape[1]), int(p.shape[2])) for p in pages]
    canvas = (max(h for h, _ in sizes), max(w for _, w in sizes))
    _cc_quads_pages_sizes(len(pages), *canvas)  # (refuses the batch before anything is launched)
    extra = {}
    if tile is None:
        img = torch.stack([resize(transform_image(p), size) for p in pages])
        with torch.inference_mode():
            probs = model(img)[:, 0]
        text_masks = binarize_resize_pages(probs, _to_device_async(sizes, torch.int32, dev), canvas, threshold)
    else:
        store = pack_pages(pages) if _store is None else _store
        probs, text_masks, tables = _detect_tiles(model, store, sizes, canvas, size, threshold, tile, overlap, tile_batch, "detect_words_batch")
        extra = {"tiles": tables.tiles, "tile_offs": tables.tile_offs}
    flat, page_of_word, word_offs, counts = cc_quads_pages(text_masks)
    quads = expand_quads(flat, expand) if flat.shape[0] else flat
    return {"probs": probs, "text_masks": text_masks, "quads": quads, "page_of_word": page_of_word, "word_offs": word_offs, "counts": counts, **extra}

"""Training augmentations on the GPU: the reference's ``--augment`` pipelines (torchvision, per sample, fp32, on DataLoader workers) and the
detection loop's plain ``Resize(mask_size, antialias=False)``, batched into a few kernel launches (csrc/augment.hip).

* ``detection_batch``  prepare_transform(mask_size, augment) + default collate     ocrs_models/train_detection.py:266-290
* ``collate_lines``    background mask + text_recognition_data_augmentations() +   ocrs_models/datasets/__init__.py:4-30,
                       clamp + resize_line + collate_samples                       datasets/hiertext.py:271-294, train_rec.py:248-304

The random parameters are drawn on the host by ``sample_detection_params`` / ``sample_line_params`` from the same distributions and in
the same call order as torchvision (``torch`` draws in sequence, Python's ``random.choices`` for the branch), so every output size is known
before the launch and nothing synchronises with the device.  The formulas restate torchvision's tensor code path (see
tests/augment_ref.py); torchvision is not installed where this project runs, so that parity is not pinned.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field

import numpy as np
import torch

from ._lib import DT, lib, ptr
from .text import collate_plan, line_output_width

MASK_SIZE = (800, 600)  # train_detection.py's mask_size
CROP_SIZE = 600  # RandomCrop(size=600)
REC_WORDS = 24  # 32-bit words per device record (include/ocrs_hip.h)

# record kinds of csrc/augment.hip
_IDENTITY, _JITTER, _AFFINE_NEAREST, _PERSPECTIVE, _SHIFT, _AFFINE_BILINEAR = range(6)


@dataclass
class AugParams:
    """One sample's draw.  ``branch`` = index into the reference's RandomChoice list (detection: jitter, affine, perspective, crop;
    recognition: jitter, rotate, pad), -1 = RandomApply left the sample alone.  ``size`` = source (H, W); ``out_size`` = (H, W) after the
    augmentation, before the resize."""

    branch: int
    size: tuple
    out_size: tuple
    order: tuple = ()  # ColorJitter's torch.randperm(4)
    brightness: float = 1.0
    contrast: float = 1.0
    angle: float = 0.0  # RandomAffine / RandomRotation, degrees
    scale: float = 1.0
    shear: float = 0.0
    endpoints: list = field(default_factory=list)  # RandomPerspective
    pad: tuple = (0, 0)  # (top, left) fill added on each side
    offset: tuple = (0, 0)  # RandomCrop's (i, j) in the padded image
    matrix: np.ndarray | None = None  # fp32 inverse map: 2x3 affine or 3x3 perspective (coefficients, 1 appended)


# ---- torchvision's host-side maths ------------------------------------------------------------------------------------------------
def _inverse_affine_matrix(angle: float, scale: float, shear_x: float) -> list[float]:
    """transforms.functional._get_inverse_affine_matrix with center, translate and shear_y all 0."""
    rot, sx = math.radians(angle), math.radians(shear_x)
    a = math.cos(rot)
    b = -math.cos(rot) * math.tan(sx) - math.sin(rot)
    c = math.sin(rot)
    d = -math.sin(rot) * math.tan(sx) + math.cos(rot)
    return [x / scale for x in [d, -b, 0.0, -c, a, 0.0]]


def _affine_output_size(matrix: list[float], w: int, h: int) -> tuple[int, int]:
    """functional_tensor._compute_affine_output_size -> (ow, oh)."""
    pts = torch.tensor([[-0.5 * w, -0.5 * h, 1.0], [-0.5 * w, 0.5 * h, 1.0], [0.5 * w, 0.5 * h, 1.0], [0.5 * w, -0.5 * h, 1.0]])
    new_pts = torch.matmul(pts, torch.tensor(matrix, dtype=torch.float).view(2, 3).T)
    shift = torch.tensor((w * 0.5, h * 0.5))
    lo, hi = new_pts.min(dim=0)[0] + shift, new_pts.max(dim=0)[0] + shift
    size = torch.ceil((hi / 1e-4).trunc_() * 1e-4) - torch.floor((lo / 1e-4).trunc_() * 1e-4)
    return int(size[0]), int(size[1])


def _perspective_coeffs(w: int, h: int, endpoints) -> list[float]:
    """transforms.functional._get_perspective_coeffs from the corners of a (h, w) image."""
    start = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]
    a = torch.zeros(8, 8, dtype=torch.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, start)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b = torch.tensor(start, dtype=torch.float64).view(8)
    return torch.linalg.lstsq(a, b, driver="gels").solution.to(torch.float32).tolist()


def _uniform(lo: float, hi: float, g) -> float:
    return float(torch.empty(1).uniform_(lo, hi, generator=g).item())


def _randint(lo: int, hi: int, g) -> int:
    return int(torch.randint(lo, hi, size=(1,), generator=g).item())


def _apply(g, rng, n: int) -> int:
    """RandomApply(p=0.5) around RandomChoice of n transforms: -1 or the chosen index."""
    if 0.5 < torch.rand(1, generator=g):
        return -1
    return (rng or random).choices(range(n))[0]


def _jitter(p: AugParams, g) -> None:
    """ColorJitter(brightness=0.1, contrast=0.1).get_params: randperm(4), then b, then c (saturation and hue are None)."""
    p.order = tuple(torch.randperm(4, generator=g).tolist())
    p.brightness = _uniform(0.9, 1.1, g)
    p.contrast = _uniform(0.9, 1.1, g)


def sample_detection_params(sizes, generator: torch.Generator | None = None, rng: random.Random | None = None) -> list[AugParams]:
    """One ``prepare_transform(mask_size, augment=True)`` draw per source (H, W), in torchvision's order."""
    out = []
    for h, w in sizes:
        h, w = int(h), int(w)
        p = AugParams(_apply(generator, rng, 4), (h, w), (h, w))
        if p.branch == 0:
            _jitter(p, generator)
        elif p.branch == 1:  # RandomAffine(degrees=5, scale=(0.8, 1.2), shear=5)
            p.angle = _uniform(-5.0, 5.0, generator)
            p.scale = _uniform(0.8, 1.2, generator)
            p.shear = _uniform(-5.0, 5.0, generator)
            p.matrix = np.array(_inverse_affine_matrix(p.angle, p.scale, p.shear), dtype=np.float32).reshape(2, 3)
        elif p.branch == 2:  # RandomPerspective(distortion_scale=0.1, p=1.0)
            torch.rand(1, generator=generator)  # the p=1.0 test
            dw, dh = int(0.1 * (w // 2)), int(0.1 * (h // 2))
            r = lambda lo, hi: _randint(lo, hi, generator)  # noqa: E731
            tl = [r(0, dw + 1), r(0, dh + 1)]
            tr = [r(w - dw - 1, w), r(0, dh + 1)]
            br = [r(w - dw - 1, w), r(h - dh - 1, h)]
            bl = [r(0, dw + 1), r(h - dh - 1, h)]
            p.endpoints = [tl, tr, br, bl]
            p.matrix = np.array(_perspective_coeffs(w, h, p.endpoints) + [1.0], dtype=np.float32).reshape(3, 3)
        elif p.branch == 3:  # RandomCrop(600, pad_if_needed=True): each side gets the whole deficit
            p.pad = (max(CROP_SIZE - h, 0), max(CROP_SIZE - w, 0))
            ph, pw = h + 2 * p.pad[0], w + 2 * p.pad[1]
            if (ph, pw) != (CROP_SIZE, CROP_SIZE):
                p.offset = (_randint(0, ph - CROP_SIZE + 1, generator), _randint(0, pw - CROP_SIZE + 1, generator))
            p.out_size = (CROP_SIZE, CROP_SIZE)
        out.append(p)
    return out


def sample_line_params(sizes, generator: torch.Generator | None = None, rng: random.Random | None = None) -> list[AugParams]:
    """One ``text_recognition_data_augmentations()`` draw per line crop (H, W), in torchvision's order."""
    out = []
    for h, w in sizes:
        h, w = int(h), int(w)
        p = AugParams(_apply(generator, rng, 3), (h, w), (h, w))
        if p.branch == 0:
            _jitter(p, generator)
        elif p.branch == 1:  # RandomRotation(5, expand=True, bilinear, fill=-0.5): F.rotate negates the angle
            p.angle = _uniform(-5.0, 5.0, generator)
            m = _inverse_affine_matrix(-p.angle, 1.0, 0.0)
            p.matrix = np.array(m, dtype=np.float32).reshape(2, 3)
            ow, oh = _affine_output_size(m, w, h)
            p.out_size = (oh, ow)
        elif p.branch == 2:  # Pad(padding=(5, 5), fill=-0.5)
            p.pad = (5, 5)
            p.out_size = (h + 10, w + 10)
        out.append(p)
    return out


# ---- device records ---------------------------------------------------------------------------------------------------------------
def records(params: list[AugParams], line: bool, widths=None) -> np.ndarray:
    """AugParams -> [B][REC_WORDS] int32 device records (layout in include/ocrs_hip.h)."""
    rec = np.zeros((len(params), REC_WORDS), dtype=np.int32)
    f = rec[:, 16:].view(np.float32)
    f32 = np.float32
    for k, p in enumerate(params):
        (h, w), (ih, iw) = p.size, p.out_size
        kind = _IDENTITY
        if p.branch == 0:
            kind = _JITTER
            f[k, :3] = [p.brightness, p.contrast, 1.0 - p.contrast]
            rec[k, 1] = int(p.order.index(0) < p.order.index(1))
        elif p.branch == 1 or (p.branch == 2 and not line):
            m = p.matrix
            if p.branch == 2 and not line:  # _perspective_grid: theta1 rows over (w/2, h/2), then the denominator row
                kind = _PERSPECTIVE
                f[k, :3] = m[0] / f32(0.5 * w)
                f[k, 3:6] = m[1] / f32(0.5 * h)
                f[k, 6:8] = m[2, :2]
            else:  # _gen_affine_grid: base grid centred on the output, theta over the input's (w/2, h/2)
                kind = _AFFINE_BILINEAR if line else _AFFINE_NEAREST
                f[k, :3] = m[0] / f32(0.5 * w)
                f[k, 3:6] = m[1] / f32(0.5 * h)
                f[k, 6:8] = [-iw * 0.5 + 0.5, -ih * 0.5 + 0.5]
        elif p.branch in (2, 3):  # line Pad / detection RandomCrop: an integer shift with fill
            kind = _SHIFT
            rec[k, 6] = p.offset[0] - p.pad[0]
            rec[k, 7] = p.offset[1] - p.pad[1]
        rec[k, :6] = [kind, rec[k, 1], h, w, ih, iw]
        if line:
            rec[k, 8] = widths[k]
    return rec


def check_sizes(sizes, what: str):
    for h, w in sizes:
        if not (0 < h <= 65535 and 0 < w <= 65535 and h * w < 2**31):
            raise RuntimeError(f"{what}: unsupported sample size {(h, w)} (each side 1..65535, H*W < 2^31)")


def _flat(t: torch.Tensor) -> torch.Tensor:
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).reshape(-1)


def _nbytes(part) -> int:
    return part.nbytes if isinstance(part, np.ndarray) else sum(t.numel() * t.element_size() for t in part)


def pin(parts: list) -> tuple[torch.Tensor, list[int]]:
    """Host sections (numpy arrays, or lists of host tensors packed back to back) -> one pinned uint8 buffer with 16-byte aligned sections
    and their offsets.  Every sample is copied once, straight into the buffer."""
    offs, n = [], 0
    for part in parts:
        offs.append(n)
        n += (_nbytes(part) + 15) // 16 * 16
    host = torch.empty(max(n, 16), dtype=torch.uint8, pin_memory=True)
    for part, o in zip(parts, offs):
        if isinstance(part, np.ndarray):
            host[o : o + part.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(part).reshape(-1).view(np.uint8)))
            continue
        dst, k = host[o : o + _nbytes(part)].view(_flat(part[0]).dtype), 0
        for t in part:
            f = _flat(t)
            dst[k : k + f.numel()].copy_(f)
            k += f.numel()
    return host, offs


def upload(parts: list, device, what: str) -> list[torch.Tensor]:
    """Sections -> packed device tensors, in order.  numpy arrays and lists of host tensors go through one pinned buffer and one H2D copy;
    a list of GPU tensors is packed by one torch.cat on the device.  Each list may live on either side, independently of the others."""
    on_dev = []
    for part in parts:
        if isinstance(part, np.ndarray):
            on_dev.append(False)
            continue
        kinds = {t.is_cuda for t in part}
        if len(kinds) != 1:
            raise RuntimeError(f"{what}: the tensors of one list must be all on the host or all on the GPU")
        on_dev.append(kinds.pop())
    host_parts = [part for part, d in zip(parts, on_dev) if not d]
    host, offs = pin(host_parts)
    staged = host.to(device, non_blocking=True)
    ups = iter((staged[o : o + _nbytes(part)], part) for part, o in zip(host_parts, offs))
    out = []
    for part, d in zip(parts, on_dev):
        if d:
            out.append(torch.cat([_flat(t) for t in part]).to(device))
            continue
        raw, part = next(ups)
        out.append(raw.view(torch.from_numpy(part[:0]).dtype if isinstance(part, np.ndarray) else _flat(part[0]).dtype))
    return out


def resolve_params(params, sizes: list, augment: bool, sample, who: str, what: str, generator=None, rng=None) -> list[AugParams]:
    """The draws of a batch: ``params`` when given, else one ``sample`` draw per (H, W) of ``sizes`` (``augment``) or the identity; checked
    against ``sizes`` either way (``who`` and ``what`` name the caller and its samples in the error)."""
    if params is None:
        params = sample(sizes, generator, rng) if augment else [AugParams(-1, s, s) for s in sizes]
    if [tuple(p.size) for p in params] != sizes:
        raise RuntimeError(f"{who}: params do not match the {what} sizes")
    return params


def launch_det(pages_d, masks_d, offs_d, rec_d, sizes: list, image, text_mask, mask_kind: int):
    """The three launches of ocrs_augment_det on packed device pages and masks (0 = uint8 0/1, 1 = fp32) into ``image`` and ``text_mask``."""
    B, (oh, ow) = image.shape[0], image.shape[-2:]
    ws = torch.empty(lib().augment_det_ws_floats(B), dtype=torch.float32, device=image.device)
    lib().augment_det(ptr(pages_d), ptr(masks_d), ptr(offs_d), ptr(rec_d), ptr(ws), ptr(image), ptr(text_mask), B, max(h for h, _ in sizes),
                      max(w for _, w in sizes), oh, ow, mask_kind, DT[image.dtype])


def detection_batch(images, masks, device, augment: bool, dtype: torch.dtype = torch.float32, generator: torch.Generator | None = None,
                    rng: random.Random | None = None, params: list[AugParams] | None = None, mask_size=MASK_SIZE) -> dict:
    """List of (1,H,W) uint8 images and (1,H,W) uint8 (0/1) or fp32 text masks (each list all on the host or all on the GPU) ->
    {"image": (B,1,*mask_size) ``dtype``, "text_mask": (B,1,*mask_size) fp32} on ``device``: ``prepare_transform(mask_size, augment)``
    applied to each [image, mask] pair (images through ``transform_image``) and the default collate.  ``params`` overrides the draw."""
    B = len(images)
    if len(masks) != B:
        raise RuntimeError("detection_batch: need one mask per image")
    if any(im.dtype != torch.uint8 for im in images):
        raise RuntimeError("detection_batch: images must be uint8")
    mdt = {m.dtype for m in masks}
    if not (mdt <= {torch.uint8, torch.bool} or mdt == {torch.float32}):
        raise RuntimeError(f"detection_batch: masks must be all uint8/bool or all float32, got {mdt}")
    sizes = [tuple(im.shape[-2:]) for im in images]
    if any(im.dim() != 3 or im.shape[0] != 1 or tuple(m.shape) != tuple(im.shape) for im, m in zip(images, masks)):
        raise RuntimeError("detection_batch: every image and its mask must be (1, H, W) of the same size")
    check_sizes(sizes, "detection_batch")
    params = resolve_params(params, sizes, augment, sample_detection_params, "detection_batch", "image", generator, rng)
    oh, ow = mask_size
    image = torch.empty(B, 1, oh, ow, dtype=dtype, device=device)
    text_mask = torch.empty(B, 1, oh, ow, dtype=torch.float32, device=device)
    if B == 0:
        return {"image": image, "text_mask": text_mask}
    n = np.array([h * w for h, w in sizes], dtype=np.int64)
    offs = np.cumsum(n) - n
    rec_d, offs_d, img_d, msk_d = upload([records(params, line=False), offs, list(images), list(masks)], device, "detection_batch")
    launch_det(img_d, msk_d, offs_d, rec_d, sizes, image, text_mask, 1 if msk_d.dtype == torch.float32 else 0)
    return {"image": image, "text_mask": text_mask}


def line_batch_plan(text_seqs, params: list[AugParams], output_height: int, dtype, device):
    """``text.collate_plan`` on the resized widths -> (empty (n, 1, output_height, wmax) image on ``device``, {"text_seq", "text_len",
    "image_width"} host tensors, kept positions)."""
    wmax, keep, meta = collate_plan([line_output_width(p.out_size[0], p.out_size[1], output_height) for p in params], text_seqs)
    return torch.empty(len(keep), 1, output_height, wmax, dtype=dtype, device=device), meta, keep


def line_records(kp: list[AugParams], output_height: int):
    """The kept samples' device records and the [n][3] offsets (source, intermediate, horizontal pass) of ocrs_augment_lines."""
    ows = [line_output_width(p.out_size[0], p.out_size[1], output_height) for p in kp]
    rec = records(kp, line=True, widths=ows)
    src = np.array([p.size[0] * p.size[1] for p in kp], dtype=np.int64)
    inter = np.array([p.out_size[0] * p.out_size[1] for p in kp], dtype=np.int64)
    hp = np.array([p.out_size[0] * w for p, w in zip(kp, ows)], dtype=np.int64)
    return rec, np.stack([np.cumsum(a) - a for a in (src, inter, hp)], axis=1)


def launch_lines(crops_d, masks_d, offs_d, rec_d, kp: list[AugParams], image, output_height: int, kind: int, augment: bool):
    """The five launches of ocrs_augment_lines on packed device crops (and masks) into ``image``."""
    inter = sum(p.out_size[0] * p.out_size[1] for p in kp)
    hp = sum(p.out_size[0] * line_output_width(p.out_size[0], p.out_size[1], output_height) for p in kp)
    n = len(kp)
    ws = torch.empty(lib().augment_lines_ws_floats(n, inter, hp), dtype=torch.float32, device=image.device)
    lib().augment_lines(ptr(crops_d), ptr(masks_d), ptr(offs_d), ptr(rec_d), ptr(ws), inter, ptr(image), n, max(p.out_size[0] for p in kp),
                        max(p.out_size[1] for p in kp), output_height, image.shape[-1], kind, int(augment), DT[image.dtype])


def collate_lines(samples: list[dict], device, augment: bool, output_height: int = 64, dtype: torch.dtype = torch.float32,
                  generator: torch.Generator | None = None, rng: random.Random | None = None, params: list[AugParams] | None = None) -> dict:
    """List of {'image': (1,h,w) uint8 or fp32 un-resized line crop, 'text_seq': (L,) int32, optional 'mask': (1,h,w) uint8/bool 0/1}
    -> the dict ``collate_samples`` returns, with ``image`` on ``device``: each crop background-masked, augmented (``augment``), clamped,
    resized to ``output_height`` by ``resize_line``'s rule and collated.  The crops and the masks may each be on the host or the GPU.
    ``params`` (one per sample) overrides the draw."""
    if not samples:
        raise RuntimeError("collate_lines: empty batch")
    sizes = [tuple(s["image"].shape[-2:]) for s in samples]
    if any(s["image"].dim() != 3 or s["image"].shape[0] != 1 for s in samples):
        raise RuntimeError("collate_lines: every image must be (1, h, w)")
    check_sizes(sizes, "collate_lines")
    params = resolve_params(params, sizes, augment, sample_line_params, "collate_lines", "image", generator, rng)
    image, meta, keep = line_batch_plan([s["text_seq"] for s in samples], params, output_height, dtype, device)
    if keep:
        ks = [samples[k] for k in keep]
        kinds = {s["image"].dtype for s in ks}
        if kinds not in ({torch.uint8}, {torch.float32}):
            raise RuntimeError(f"collate_lines: images must be all uint8 or all float32, got {kinds}")
        has_mask = [("mask" in s) and s["mask"] is not None for s in ks]
        if any(has_mask) and not all(has_mask):
            raise RuntimeError("collate_lines: give a mask for every sample or for none")
        if any(has_mask) and any(tuple(s["mask"].shape) != tuple(s["image"].shape) for s in ks):
            raise RuntimeError("collate_lines: a mask must have its image's shape")
        rec, offs = line_records([params[k] for k in keep], output_height)
        if all(has_mask) and any(s["mask"].dtype not in (torch.uint8, torch.bool) for s in ks):
            raise RuntimeError("collate_lines: masks must be uint8 or bool")
        parts = [rec, offs, [s["image"] for s in ks]] + ([[s["mask"] for s in ks]] if all(has_mask) else [])
        up = upload(parts, device, "collate_lines")
        rec_d, offs_d, crops_d = up[:3]
        masks_d = up[3] if len(up) > 3 else None
        launch_lines(crops_d, masks_d, offs_d, rec_d, [params[k] for k in keep], image, output_height, 0 if torch.uint8 in kinds else 1,
                     augment)
    return {"image": image, **meta}

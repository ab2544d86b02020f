"""CPU comparand of the training augmentations (ocrs_models_amd/augment.py): torchvision's tensor code path for the fixed arguments the
reference's two training scripts use, restated in the ATen operators torchvision itself calls (``F.grid_sample``, ``F.interpolate``,
``clamp``, ``mean``, ``torch.linalg.lstsq``).

* detection: ``prepare_transform(mask_size, augment)``                   ocrs_models/train_detection.py:266-290
* recognition: ``text_recognition_data_augmentations()``                 ocrs_models/datasets/__init__.py:4-30, applied at hiertext.py:271-294

torchvision is not installed anywhere this project runs, so these restatements are not pinned against it (the same standing as
``input_pipeline.resize``).  Every function takes the raw parameters of an ``AugParams`` record (angle, scale, shear, end points, factors,
offsets) and recomputes matrices and sizes itself, so the tests also check the sampler's host-side maths.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

MASK_SIZE = (800, 600)


# ---- torchvision.transforms.functional._get_inverse_affine_matrix, center (0, 0), translate (0, 0), shear_y = 0 -------------------
def inverse_affine_matrix(angle: float, scale: float, shear_x: float) -> list[float]:
    rot = math.radians(angle)
    sx = math.radians(shear_x)
    sy = math.radians(0.0)
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [x / scale for x in [d, -b, 0.0, -c, a, 0.0]]
    m[2] += m[0] * (-0.0 - 0.0) + m[1] * (-0.0 - 0.0)
    m[5] += m[3] * (-0.0 - 0.0) + m[4] * (-0.0 - 0.0)
    return m


# ---- functional_tensor._compute_affine_output_size (RandomRotation(expand=True)) -------------------------------------------------
def affine_output_size(matrix: list[float], w: int, h: int) -> tuple[int, int]:
    pts = torch.tensor([[-0.5 * w, -0.5 * h, 1.0], [-0.5 * w, 0.5 * h, 1.0], [0.5 * w, 0.5 * h, 1.0], [0.5 * w, -0.5 * h, 1.0]])
    theta = torch.tensor(matrix, dtype=torch.float).view(2, 3)
    new_pts = torch.matmul(pts, theta.T)
    min_vals, _ = new_pts.min(dim=0)
    max_vals, _ = new_pts.max(dim=0)
    min_vals += torch.tensor((w * 0.5, h * 0.5))
    max_vals += torch.tensor((w * 0.5, h * 0.5))
    tol = 1e-4
    cmax = torch.ceil((max_vals / tol).trunc_() * tol)
    cmin = torch.floor((min_vals / tol).trunc_() * tol)
    size = cmax - cmin
    return int(size[0]), int(size[1])  # (ow, oh)


# ---- functional._get_perspective_coeffs --------------------------------------------------------------------------------------------
def perspective_coeffs(startpoints, endpoints) -> list[float]:
    a_matrix = torch.zeros(2 * len(startpoints), 8, dtype=torch.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a_matrix[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a_matrix[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b_matrix = torch.tensor(startpoints, dtype=torch.float64).view(8)
    return torch.linalg.lstsq(a_matrix, b_matrix, driver="gels").solution.to(torch.float32).tolist()


def perspective_startpoints(w: int, h: int):
    return [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]


# ---- functional_tensor grids -------------------------------------------------------------------------------------------------------
def _bmm3(base_grid: torch.Tensor, theta_t: torch.Tensor) -> torch.Tensor:
    """base_grid.view(1, N, 3).bmm(theta_t) for theta_t (1, 3, 2), written out as (x * t0 + y * t1) + t2 in fp32.  A BLAS GEMM rounds
    this K=3 product differently on different CPUs (with or without FMA), and grid_sample turns one ulp of the grid into ~1e-4 of
    output, so the comparand fixes the unfused order."""
    b = base_grid.reshape(-1, 3)
    t = theta_t[0]
    cols = [(b[:, 0] * t[0, j] + b[:, 1] * t[1, j]) + t[2, j] for j in range(2)]
    return torch.stack(cols, dim=-1).unsqueeze(0)


def gen_affine_grid(theta: torch.Tensor, w: int, h: int, ow: int, oh: int) -> torch.Tensor:
    d = 0.5
    base_grid = torch.empty(1, oh, ow, 3, dtype=theta.dtype)
    base_grid[..., 0].copy_(torch.linspace(-ow * 0.5 + d, ow * 0.5 + d - 1, steps=ow))
    base_grid[..., 1].copy_(torch.linspace(-oh * 0.5 + d, oh * 0.5 + d - 1, steps=oh).unsqueeze_(-1))
    base_grid[..., 2].fill_(1)
    rescaled_theta = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=theta.dtype)
    return _bmm3(base_grid, rescaled_theta).view(1, oh, ow, 2)


def perspective_grid(coeffs: list[float], ow: int, oh: int) -> torch.Tensor:
    theta1 = torch.tensor([[[coeffs[0], coeffs[1], coeffs[2]], [coeffs[3], coeffs[4], coeffs[5]]]], dtype=torch.float32)
    theta2 = torch.tensor([[[coeffs[6], coeffs[7], 1.0], [coeffs[6], coeffs[7], 1.0]]], dtype=torch.float32)
    d = 0.5
    base_grid = torch.empty(1, oh, ow, 3, dtype=torch.float32)
    base_grid[..., 0].copy_(torch.linspace(d, ow * 1.0 + d - 1.0, steps=ow))
    base_grid[..., 1].copy_(torch.linspace(d, oh * 1.0 + d - 1.0, steps=oh).unsqueeze_(-1))
    base_grid[..., 2].fill_(1)
    rescaled_theta1 = theta1.transpose(1, 2) / torch.tensor([0.5 * ow, 0.5 * oh], dtype=torch.float32)
    output_grid1 = _bmm3(base_grid, rescaled_theta1)
    output_grid2 = _bmm3(base_grid, theta2.transpose(1, 2))
    return (output_grid1 / output_grid2 - 1.0).view(1, oh, ow, 2)


def apply_grid_transform(img: torch.Tensor, grid: torch.Tensor, mode: str, fill: float) -> torch.Tensor:
    """functional_tensor._apply_grid_transform: a ones channel rides along as the fill mask."""
    if img.shape[0] > 1:
        grid = grid.expand(img.shape[0], grid.shape[1], grid.shape[2], grid.shape[3])
    mask = torch.ones((img.shape[0], 1, img.shape[2], img.shape[3]), dtype=img.dtype)
    img = torch.cat((img, mask), dim=1)
    img = F.grid_sample(img, grid, mode=mode, padding_mode="zeros", align_corners=False)
    mask = img[:, -1:, :, :]
    img = img[:, :-1, :, :]
    mask = mask.expand_as(img)
    fill_img = torch.tensor([float(fill)], dtype=img.dtype).view(1, 1, 1, 1).expand_as(img)
    if mode == "nearest":
        mask = mask < 0.5
        img[mask] = fill_img[mask]
    else:
        img = img * mask + (1.0 - mask) * fill_img
    return img


# ---- transforms ------------------------------------------------------------------------------------------------------------------
def color_jitter(x: torch.Tensor, order, b: float, c: float) -> torch.Tensor:
    """ColorJitter(brightness=0.1, contrast=0.1) on an (N,1,H,W) batch: adjust_brightness / adjust_contrast = _blend(...).clamp(0, 1)."""
    for fn_id in order:
        if fn_id == 0:
            x = (b * x + (1.0 - b) * torch.zeros_like(x)).clamp(0, 1.0)
        elif fn_id == 1:
            mean = torch.mean(x, dim=(-3, -2, -1), keepdim=True)
            x = (c * x + (1.0 - c) * mean).clamp(0, 1.0)
    return x


def affine(x: torch.Tensor, angle: float, scale: float, shear: float) -> torch.Tensor:
    """RandomAffine(degrees=5, scale=(0.8, 1.2), shear=5): nearest, fill 0."""
    m = inverse_affine_matrix(angle, scale, shear)
    theta = torch.tensor(m, dtype=torch.float32).reshape(1, 2, 3)
    h, w = x.shape[-2:]
    return apply_grid_transform(x, gen_affine_grid(theta, w, h, w, h), "nearest", 0.0)


def perspective(x: torch.Tensor, endpoints) -> torch.Tensor:
    """RandomPerspective(distortion_scale=0.1, p=1.0): bilinear, fill 0."""
    h, w = x.shape[-2:]
    coeffs = perspective_coeffs(perspective_startpoints(w, h), endpoints)
    return apply_grid_transform(x, perspective_grid(coeffs, w, h), "bilinear", 0.0)


def random_crop(x: torch.Tensor, i: int, j: int, size: int = 600) -> torch.Tensor:
    """RandomCrop(600, pad_if_needed=True), fill 0: the width deficit is padded on both left and right, the height one on top and bottom."""
    h, w = x.shape[-2:]
    if w < size:
        x = F.pad(x, [size - w, size - w, 0, 0], value=0.0)
    if h < size:
        x = F.pad(x, [0, 0, size - h, size - h], value=0.0)
    return x[..., i : i + size, j : j + size]


def rotate(x: torch.Tensor, angle: float) -> torch.Tensor:
    """RandomRotation(5, expand=True, bilinear, fill=-0.5)."""
    m = inverse_affine_matrix(-angle, 1.0, 0.0)
    h, w = x.shape[-2:]
    ow, oh = affine_output_size(m, w, h)
    theta = torch.tensor(m, dtype=torch.float32).reshape(1, 2, 3)
    return apply_grid_transform(x, gen_affine_grid(theta, w, h, ow, oh), "bilinear", -0.5)


# ---- whole samples ---------------------------------------------------------------------------------------------------------------
def det_branch(x: torch.Tensor, p) -> torch.Tensor:
    """The RandomApply(RandomChoice([...])) part of prepare_transform on the (2,1,H,W) stack [image, mask]."""
    if p.branch == 0:
        return color_jitter(x, p.order, p.brightness, p.contrast)
    if p.branch == 1:
        return affine(x, p.angle, p.scale, p.shear)
    if p.branch == 2:
        return perspective(x, p.endpoints)
    if p.branch == 3:
        return random_crop(x, *p.offset)
    return x


def det_sample(img: torch.Tensor, mask: torch.Tensor, p, size=MASK_SIZE):
    """(1,H,W) fp32 image in [-0.5, 0.5] and (1,H,W) fp32 mask -> (image, mask), each (1, *size)."""
    x = torch.stack([img, mask])
    if p is not None:
        x = det_branch(x, p)
    x = F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=False)
    return x[0], x[1]


def line_sample(img: torch.Tensor, p, mask: torch.Tensor | None = None, output_height: int = 64) -> torch.Tensor:
    """hiertext.py:271-294 for one (1,h,w) fp32 line crop: background masking, augmentation (p None = transform off), clamp, resize."""
    if mask is not None:
        m = mask.float()
        img = torch.full(img.shape, -0.5) * (1.0 - m) + img * m
    if p is not None:
        x = img.unsqueeze(0)
        if p.branch == 0:
            x = color_jitter(x, p.order, p.brightness, p.contrast)
        elif p.branch == 1:
            x = rotate(x, p.angle)
        elif p.branch == 2:
            x = F.pad(x, [5, 5, 5, 5], value=-0.5)
        img = x[0].clamp(-0.5, 0.5)
    _, h, w = img.shape
    ow = min(800, max(10, int(output_height * (w / h))))
    return F.interpolate(img.unsqueeze(0), size=(output_height, ow), mode="bilinear", align_corners=False, antialias=True)[0]

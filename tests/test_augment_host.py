"""CPU-only: the augmentation parameter sampler (ocrs_models_amd/augment.py) -- torchvision's distributions and ranges, reproducibility,
and the host-side matrices / sizes / coefficients against the comparand tests/augment_ref.py."""
import math
import random

import numpy as np
import pytest
import torch

from ocrs_models_amd import augment as A
from tests import augment_ref as R

N = 20000
EDGES = [599, 600, 601, 1601]


def _freq_ok(count, n, p):
    return abs(count / n - p) <= 4 * math.sqrt(p * (1 - p) / n)


@pytest.mark.parametrize("line", [False, True])
def test_branch_frequencies(line):
    sampler = A.sample_line_params if line else A.sample_detection_params
    ps = sampler([(48, 300)] * N, torch.Generator().manual_seed(1), random.Random(1))
    br = np.array([p.branch for p in ps])
    nb = 3 if line else 4
    assert _freq_ok((br == -1).sum(), N, 0.5)
    for b in range(nb):
        assert _freq_ok((br == b).sum(), N, 0.5 / nb), (b, (br == b).sum())
    assert set(br.tolist()) == {-1, *range(nb)}


def test_detection_parameter_ranges():
    n_each = N // len(EDGES) ** 2
    g, rng = torch.Generator().manual_seed(2), random.Random(2)
    for h in EDGES:
        for w in EDGES:
            ps = A.sample_detection_params([(h, w)] * n_each, g, rng)
            dw, dh = int(0.1 * (w // 2)), int(0.1 * (h // 2))
            crop_i, crop_j, ex, ey = set(), set(), [set() for _ in range(4)], [set() for _ in range(4)]
            for p in ps:
                assert p.size == (h, w)
                if p.branch == 0:
                    assert sorted(p.order) == [0, 1, 2, 3] and 0.9 <= p.brightness <= 1.1 and 0.9 <= p.contrast <= 1.1
                elif p.branch == 1:
                    assert -5 <= p.angle <= 5 and 0.8 <= p.scale <= 1.2 and -5 <= p.shear <= 5 and p.out_size == (h, w)
                elif p.branch == 2:
                    for k, (x, y) in enumerate(p.endpoints):
                        ex[k].add(x), ey[k].add(y)
                elif p.branch == 3:
                    assert p.out_size == (600, 600) and p.pad == (max(600 - h, 0), max(600 - w, 0))
                    crop_i.add(p.offset[0]), crop_j.add(p.offset[1])
                else:
                    assert p.out_size == (h, w)
            near_x, far_x = set(range(0, dw + 1)), set(range(w - dw - 1, w))
            near_y, far_y = set(range(0, dh + 1)), set(range(h - dh - 1, h))
            for k, (sx, sy) in enumerate([(near_x, near_y), (far_x, near_y), (far_x, far_y), (near_x, far_y)]):
                assert ex[k] <= sx and ey[k] <= sy
            ph, pw = h + 2 * max(600 - h, 0), w + 2 * max(600 - w, 0)
            assert crop_i <= set(range(ph - 600 + 1)) and crop_j <= set(range(pw - 600 + 1))
            if ph - 600 < 3:
                assert crop_i == set(range(ph - 600 + 1))
            if pw - 600 < 3:
                assert crop_j == set(range(pw - 600 + 1))


def test_line_parameter_ranges():
    ps = A.sample_line_params([(48, 300)] * N, torch.Generator().manual_seed(3), random.Random(3))
    for p in ps:
        if p.branch == 0:
            assert sorted(p.order) == [0, 1, 2, 3] and 0.9 <= p.brightness <= 1.1 and 0.9 <= p.contrast <= 1.1
        elif p.branch == 1:
            assert -5 <= p.angle <= 5 and p.out_size[0] >= 48 and p.out_size[1] >= 300
        elif p.branch == 2:
            assert p.out_size == (58, 310)


def test_fixed_seed_gives_identical_records():
    sizes = [(1600, 1200), (48, 300), (599, 601)] * 50
    for sampler, line in ((A.sample_detection_params, False), (A.sample_line_params, True)):
        a = sampler(sizes, torch.Generator().manual_seed(5), random.Random(5))
        b = sampler(sizes, torch.Generator().manual_seed(5), random.Random(5))
        w = [100] * len(sizes)
        assert np.array_equal(A.records(a, line, w), A.records(b, line, w))
        c = sampler(sizes, torch.Generator().manual_seed(6), random.Random(6))
        assert not np.array_equal(A.records(a, line, w), A.records(c, line, w))


def test_default_generators_are_used():
    torch.manual_seed(7)
    random.seed(7)
    a = A.sample_detection_params([(64, 64)] * 200)
    torch.manual_seed(7)
    random.seed(7)
    b = A.sample_detection_params([(64, 64)] * 200)
    assert [(p.branch, p.angle, p.endpoints, p.offset, p.brightness) for p in a] == [(p.branch, p.angle, p.endpoints, p.offset, p.brightness)
                                                                                    for p in b]


def test_host_maths_match_comparand():
    sizes = [(1600, 1200), (599, 601), (480, 640), (2001, 37), (48, 300), (37, 211)] * 40
    det = A.sample_detection_params(sizes, torch.Generator().manual_seed(8), random.Random(8))
    lines = A.sample_line_params(sizes + [(1, 9)] * 20, torch.Generator().manual_seed(8), random.Random(8))
    seen = set()
    for p in det:
        h, w = p.size
        if p.branch == 1:
            assert np.array_equal(p.matrix.reshape(-1), np.array(R.inverse_affine_matrix(p.angle, p.scale, p.shear), dtype=np.float32))
        elif p.branch == 2:
            want = R.perspective_coeffs(R.perspective_startpoints(w, h), p.endpoints)
            assert np.array_equal(p.matrix.reshape(-1)[:8], np.array(want, dtype=np.float32)) and p.matrix[2, 2] == 1
        seen.add(("det", p.branch))
    for p in lines:
        h, w = p.size
        if p.branch == 1:
            m = R.inverse_affine_matrix(-p.angle, 1.0, 0.0)
            assert np.array_equal(p.matrix.reshape(-1), np.array(m, dtype=np.float32))
            ow, oh = R.affine_output_size(m, w, h)
            assert p.out_size == (oh, ow)
            x = R.rotate(torch.zeros(1, 1, h, w), p.angle)
            assert tuple(x.shape[-2:]) == p.out_size
        seen.add(("line", p.branch))
    assert len(seen) == 9


def test_records_layout():
    p = A.sample_detection_params([(1200, 1600)], torch.Generator().manual_seed(0), random.Random(0))
    rec = A.records(p, False)
    assert rec.shape == (1, A.REC_WORDS) and rec.dtype == np.int32
    from ocrs_models_amd._lib import SIGNATURES

    for name in ("ocrs_augment_det", "ocrs_augment_det_ws_floats", "ocrs_augment_lines", "ocrs_augment_lines_ws_floats"):
        assert name in SIGNATURES

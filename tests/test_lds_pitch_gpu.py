"""The bf16 kernels around the padded LDS pixel pitch (csrc/common.h: lds_pitch_bf16), through the C ABI, against the CPU references and tolerances of
tests/test_det_ops_gpu.py (fp32 torch forward, rounding-matched float64 oracle backward; the pooled forward output is compared run against run only).

The matrix-core blocks (k_mm_fwd / k_mm_bwd) stage their 32-channel tiles at the padded pitch, except tileX of 32 -> 16 backward; the deep-level
kernels (k_pwb, k_dwf, k_ctf, k_ctd, the ConvTranspose weight gradient) keep the 16-byte pad and are covered here at the same kind of shape.
Shapes: several tiles, a ragged border and the last pixel of a tile under a transpose read -- 40 x 72 (W % 32 != 0: the compiler-waited kernels)
and 16 x 64 (every tile inside the image: the FULL kernels with hand-written waits) for the matrix-core blocks, 24 x 40 for the deep-level
kernels.  Every block case runs twice in one process with another shape in between: the tiles' pad columns are zeroed once per launch and read
by every transpose read, so whatever a previous launch left in LDS must not reach a result -- both runs must agree bit for bit."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import test_det_ops_gpu as ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def run_block(dev, Ca, Cb, Cout, N, H, W, pooled):
    """one DepthwiseConv block forward + backward in bf16 (direct: one gradient; pooled: two gradients through MaxPool2d(2)); the forward is checked
    against fp32 torch on the CPU, the backward against the rounding-matched oracle; -> every tensor the kernels produced"""
    from ocrs_models_amd.models import _Act

    g = torch.Generator().manual_seed(Ca * 1000 + Cb * 10 + Cout + H)
    Cin = Ca + Cb
    xa = torch.randn(N, Ca, H, W, generator=g).to(dev)
    xb = torch.randn(N, Cb, H, W, generator=g).to(dev) if Cb else None
    tra, trb = ops.rand_tr(Ca, dev, g), (ops.rand_tr(Cb, dev, g) if Cb else None)
    pfx = "blk"
    P = {
        f"{pfx}.seq.0.weight": (torch.randn(Cin, 1, 3, 3, generator=g) / 3).to(dev),
        f"{pfx}.seq.1.weight": (torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin)).to(dev),
        f"{pfx}.seq.2.weight": (1 + 0.1 * torch.randn(Cout, generator=g)).to(dev),
        f"{pfx}.seq.2.bias": (0.1 * torch.randn(Cout, generator=g)).to(dev),
    }
    P[f"{pfx}.seq.2.weight"][1] *= -1
    Bf = {f"{pfx}.seq.2.running_mean": torch.zeros(Cout, device=dev), f"{pfx}.seq.2.running_var": torch.ones(Cout, device=dev),
          f"{pfx}.seq.2.num_batches_tracked": torch.zeros((), dtype=torch.int64, device=dev)}
    run = ops.make_run(dev, BF, N, P, Bf)
    xa_s, xb_s = ops.nhwc(xa, BF), (ops.nhwc(xb, BF) if Cb else None)
    out = run.block(pfx, _Act(xa_s, tra, Ca, H, W), _Act(xb_s, trb, Cb, H, W) if Cb else None, Cout, pool=bool(pooled))
    torch.cuda.synchronize()

    xs = [ops.apply_tr(ops.cpu(ops.nchw(xa_s)), ops.cpu(tra))]
    if Cb:
        xs.append(ops.apply_tr(ops.cpu(ops.nchw(xb_s)), ops.cpu(trb)))
    u = F.conv2d(torch.cat(xs, 1), ops.cpu(P[f"{pfx}.seq.0.weight"]), None, 1, 1, 1, Cin)
    z = F.conv2d(u.bfloat16().float(), ops.cpu(P[f"{pfx}.seq.1.weight"]))  # (the kernels round u to bf16 before the MFMA)
    ez = ops.rel(ops.nchw(out.t), z)
    print(f"{Ca}|{Cb}->{Cout} {H}x{W} pooled={pooled}: z vs fp32 torch {ez:.1e}")
    assert ez < ops.TOL[BF], "z"

    Hg, Wg = (H // 2, W // 2) if pooled else (H, W)
    g1 = ops.nhwc(torch.randn(N, Cout, Hg, Wg, generator=g).to(dev), BF)
    g2 = ops.nhwc(torch.randn(N, Cout, Hg, Wg, generator=g).to(dev), BF) if pooled else None
    run.G = {k: torch.zeros_like(v) for k, v in P.items()}
    gxa, gxb = run.block_bwd(pfx, g1, g2, 1 if pooled else 0)
    torch.cuda.synchronize()
    srcs = [(xa_s, tra)] + ([(xb_s, trb)] if Cb else [])
    errs = ops.oracle_block_bwd_check(pfx, P, srcs, g1, g2, 1 if pooled else 0, run, gxa, gxb if Cb else None, z_stored=None if pooled else out.t)
    print("   backward vs rounding-matched oracle:", {k.split(".", 1)[-1]: f"{v:.1e}" for k, v in errs.items()})
    res = {"z": out.t, "tr": out.tr, "gxa": gxa, **{k: v for k, v in run.G.items()}}
    if Cb:
        res["gxb"] = gxb
    if run.pooled_by_block is not None:
        res["pooled"] = run.pooled_by_block
    return {k: v.clone() for k, v in res.items()}


def twice(fn, other):
    first = fn()
    other()
    second = fn()
    for k in first:
        assert torch.equal(first[k], second[k]), f"{k}: the second run differs (stale LDS contents reached a result)"


# (Ca, Cb, Cout, pooled): 32 -> 32 direct | through the max-pool, two gradients | 32 | 32 -> 32 concat | 16 -> 32 | 32 -> 16
MM_BLOCKS = [(32, 0, 32, 0), (32, 0, 32, 1), (32, 32, 32, 0), (16, 0, 32, 0), (32, 0, 16, 0)]


@pytest.mark.parametrize("H,W", [(40, 72), (16, 64)], ids=["40x72", "16x64-full"])
@pytest.mark.parametrize("Ca,Cb,Cout,pooled", MM_BLOCKS)
def test_matrix_core_blocks_at_the_padded_pitch(dev, Ca, Cb, Cout, pooled, H, W):
    twice(lambda: run_block(dev, Ca, Cb, Cout, 2, H, W, pooled), lambda: run_block(dev, 16, 0, 16, 2, 21, 37, 0))


# k_pwb / k_dwf: 32 -> 64 | 64 -> 64 pooled, two gradients | 128 -> 128 | 128 | 128 -> 128 (grid.y = 2)
DEEP_BLOCKS = [(32, 0, 64, 0), (64, 0, 64, 1), (128, 0, 128, 0), (128, 128, 128, 0)]


@pytest.mark.parametrize("Ca,Cb,Cout,pooled", DEEP_BLOCKS)
def test_deep_blocks_twice(dev, Ca, Cb, Cout, pooled):
    twice(lambda: run_block(dev, Ca, Cb, Cout, 2, 24, 40, pooled), lambda: run_block(dev, 64, 0, 128, 2, 9, 13, 0))


@pytest.mark.parametrize("Cup,Cout", [(64, 32), (256, 128)])
def test_deep_conv_transpose_twice(dev, Cup, Cout):
    """k_ctf, k_ctd and the ConvTranspose weight gradient (all on their 16-byte pad) on a 12 x 20 -> 24 x 40 map: the parity test of
    test_det_ops_gpu.py at that shape, another shape, and the first again (each run against the reference, not run against run)"""
    for cu, co, h, w, H, W in ((Cup, Cout, 12, 20, 24, 40), (128, 64, 3, 3, 7, 6), (Cup, Cout, 12, 20, 24, 40)):
        ops.test_conv_transpose(dev, BF, cu, co, h, w, H, W)

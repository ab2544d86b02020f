"""The guarantees the bit-exact GPU tests (tests/test_exact_gpu.py) rest on, checked on the CPU for every case those tests use
(tests/exact_ref.py states the cases once):

  * the reference evaluated in fp32, in float64 and in a bf16-storage emulation gives IDENTICAL values -- so whatever precision and summation
    order a kernel uses, it has exactly one right answer;
  * the magnitude conditions (bf16-storable values, sums below 2^24) hold -- the references assert them when evaluated in float64;
  * every pooled case has at least 10 % of its windows with a positive maximum attained more than once;
  * for every pooled backward case, routing the gradient to the LAST maximum instead of the first moves dx by more than 100x the fp32 bound
    the GPU test applies (4e-4), i.e. by more than 0.04.  100x the bf16 bound (1.5e-2) would exceed any relative L2 distance: at (2, 11, 15) the
    bf16 cases rest on moved > 0.15 (10x their bound), and at (2, 2, 3) -- a handful of windows -- on that same moved > 0.04 against 1.5e-2.
    Where the GPU test is bit-exact (conv0, dz_apply) the other rule moves the result by O(0.4) -- the case can fail.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_ref as X

TIE_FLOOR = 0.10
FP32_GRAD_TOL = 20 * 2e-5  # test_exact_gpu.py's fp32 bound on the pooled backward (test_block_bwd_through_maxpool's own)
BF16_DX_TOL = 1.5e-2       # ... and its bf16 bound on dx (tests/test_det_ops_gpu.py BF16_DX)

_block_keys = sorted({(c, s) for _, _, c, s in X.FWD_CASES}, key=str)
_bwd_keys = sorted({(c, s) for *_, c, s in X.BWD_POOLED_CASES}, key=str)
_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def _modes_equal(fn, keys):
    r64, r32, r16 = fn("f64"), fn("f32"), fn("bf16")
    for k in keys:
        assert r32[k].dtype == torch.float32 and torch.equal(r32[k].double(), r64[k].double()), k
        assert torch.equal(r16[k].double(), r64[k].double()), k
    return r64


@pytest.mark.parametrize("chans,shape", _block_keys, ids=_ids)
def test_block_forward_cases(chans, shape):
    case = X.fwd_block_case(chans, shape)
    lin = {m: dict(zip(("xt", "u", "z"), X.block_linear(case, m))) for m in ("f64", "f32", "bf16")}
    _modes_equal(lambda m: lin[m], ("xt", "u", "z"))
    ref = X.block_reference(case, pooled=True, with_grads=False)  # asserts the magnitude conditions and the ReLU margin
    assert torch.equal(ref["pooled"], F.max_pool2d(ref["y"], 2))
    assert float(ref["z"].abs().max()) < 128
    assert ref["tied"] >= TIE_FLOOR, ref["tied"]


@pytest.mark.parametrize("N,H,W", X.FIRST_BLOCK_SHAPES)
def test_first_block_cases(N, H, W):
    case = X.first_block_case(X.seed_of(3, N, H, W), N, H, W)
    lin = {m: dict(zip(("xt", "u", "z"), X.block_linear(case, m))) for m in ("f64", "f32", "bf16")}
    r = _modes_equal(lambda m: lin[m], ("u", "z"))
    X.storable(r["u"], "u"), X.storable(r["z"], "z")
    X.summable(r["z"] * r["z"], (0, 2, 3), "sum z^2")


@pytest.mark.parametrize("chans,shape", _bwd_keys, ids=_ids)
def test_block_pooled_backward_cases(chans, shape):
    case = X.bwd_block_case(chans, shape)
    lin = {m: dict(zip(("xt", "u", "z"), X.block_linear(case, m))) for m in ("f64", "f32", "bf16")}
    _modes_equal(lambda m: lin[m], ("xt", "u", "z"))
    first, last = X.block_reference(case, pooled=True), X.block_reference(case, pooled=True, last=True)
    assert first["tied"] >= TIE_FLOOR, first["tied"]
    # the tie rule cannot be seen in the forward ...
    assert torch.equal(first["pooled"], last["pooled"]) and torch.equal(first["pooled"], F.max_pool2d(first["y"], 2))
    # ... and first-maximum routing is what torch's max_pool2d does
    y = first["y"].clone().requires_grad_(True)
    gsum = (case["g_pool"][0] + case["g_pool"][1]).double()
    gy_t, = torch.autograd.grad(F.max_pool2d(y, 2), [y], grad_outputs=gsum)
    y2 = first["y"].clone().requires_grad_(True)
    gy_o, = torch.autograd.grad(X.pool(y2), [y2], grad_outputs=gsum)
    assert torch.equal(gy_t, gy_o)
    # sensitivity: the other tie rule moves dx by more than 100x the tolerance applied on the GPU (the larger, bf16, one included)
    moved = X.rel(last["dx"], first["dx"])
    print(f"tied windows {first['tied']:.3f}; last-maximum routing moves dx by {moved:.3f}")
    assert moved > 100 * FP32_GRAD_TOL, moved
    if shape != (2, 2, 3):  # (at (2, 2, 3) the bf16 cases rest on the bound above: 0.04 against 1.5e-2)
        assert moved > 10 * BF16_DX_TOL, moved


@pytest.mark.parametrize("chans,shape", sorted({(c, s) for *_, c, s in X.BWD_FULL_CASES}, key=str), ids=_ids)
def test_block_full_backward_cases(chans, shape):
    case = X.bwd_block_case(chans, shape)
    lin = {m: dict(zip(("xt", "u", "z"), X.block_linear(case, m))) for m in ("f64", "f32", "bf16")}
    _modes_equal(lambda m: lin[m], ("xt", "u", "z"))
    X.block_reference(case, pooled=False)


@pytest.mark.parametrize("dims", X.CONVT_CASES, ids=_ids)
def test_conv_transpose_cases(dims):
    case = X.convt_case(X.seed_of(4, dims), *dims)
    _modes_equal(lambda m: X.convt_reference(case, m), ("out", "dx", "dW", "db"))
    assert int((case["W"] != 0).sum(0).max()) <= 4


@pytest.mark.parametrize("dims", X.CONV_CASES, ids=_ids)
def test_recognition_conv_cases(dims):
    case = X.conv_case(X.seed_of(5, dims), *dims)
    r = _modes_equal(lambda m: X.conv_reference(case, m), ("out", "dx", "dW", "s1"))
    assert float(r["s1"].max()) < 2 ** 24


@pytest.mark.parametrize("shape", X.CONV0_SHAPES, ids=_ids)
def test_conv0_cases(shape):
    case = X.conv0_case(X.seed_of(6, shape), *shape)
    first = _modes_equal(lambda m: X.conv0_reference(case, m), ("out", "dW", "db"))
    assert first["tied"] >= TIE_FLOOR, first["tied"]
    last = X.conv0_reference(case, last=True)
    assert torch.equal(first["out"], last["out"])
    # the GPU test is bit-exact: any movement is a failure there.  Measured: the other tie rule moves dW by O(0.1) relative.
    moved = X.rel(last["dW"], first["dW"])
    print(f"tied windows {first['tied']:.3f}; last-maximum routing moves dW by {moved:.3f}")
    assert moved > 1e-2, moved


@pytest.mark.parametrize("dims", X.POOL_PIECES_CASES, ids=_ids)
def test_pool_pieces_cases(dims):
    case = X.pool_pieces_case(X.seed_of(7, dims), *dims)
    first = _modes_equal(lambda m: X.pool_pieces_reference(case, m), ("out", "gsum", "dz", "dsum"))
    if dims[4] * dims[5] > 1:
        assert first["tied"] >= TIE_FLOOR, first["tied"]
        last = X.pool_pieces_reference(case, last=True)
        assert torch.equal(first["out"], last["out"])
        moved = X.rel(last["dz"], first["dz"])
        print(f"tied windows {first['tied']:.3f}; last-maximum routing moves dz by {moved:.3f}")
        assert moved > 1e-2, moved


@pytest.mark.parametrize("dims", X.AVGPOOL_CASES, ids=_ids)
def test_avgpool_cases(dims):
    """the reference asserts storable / summable itself; here: float32 arithmetic gives the same values, a gradient share on row 4 and a
    [N][W][C] layout would both be seen"""
    N, H, W, C = dims
    case = X.avgpool_case(X.seed_of(12, dims), *dims)
    ref = X.avgpool_reference(case)
    z, tr = case["z"], case["tr"]
    s = ((z[:, :, 0] + z[:, :, 1]) + z[:, :, 2]) + z[:, :, 3]
    seq32 = ((s * 0.25) * tr[0].view(1, C, 1) + tr[1].view(1, C, 1)).permute(2, 0, 1)
    assert seq32.dtype == torch.float32 and torch.equal(seq32.double(), ref["seq"])
    assert torch.equal(ref["dz"][:, :, 4:], ref["tail"])
    if H > 4:
        share = case["coef"][0].double().view(1, C, 1, 1) * (case["gseq"].double().permute(1, 2, 0) * 0.25).unsqueeze(2)
        assert float(share.abs().max()) > 0  # what row 4 would receive
    if N > 1 and W > 1:
        assert not torch.equal(ref["seq"].reshape(-1), ref["seq"].permute(1, 0, 2).reshape(-1))


def _bf16_exact(*ts):
    return all(torch.equal(t.bfloat16().float(), t) for t in ts)


@pytest.mark.parametrize("P,K,M", sorted({(c[0], c[1], c[2]) for c in X.GEMM_CASES + X.GEMM_X3_CASES}))
def test_gemm_cases(P, K, M):
    for salt in (8, 9):  # (the exact-fp32 and the split-bf16 test draw their own operands)
        Xm, W, b = X.gemm_operands(X.seed_of(salt, P, K, M), P, K, M)
        assert _bf16_exact(Xm, W, b)  # the split-bf16 high plane holds the operand, the low planes are zero
        assert torch.equal((Xm @ W + b).double(), Xm.double() @ W.double() + b.double())


@pytest.mark.parametrize("dims", X.WGRAD_GEMM_CASES, ids=_ids)
def test_wgrad_gemm_cases(dims):
    P, CA, ldA, CB, ldB = dims
    A, B, dW0 = X.wgrad_gemm_operands(*dims)
    assert _bf16_exact(A, B, dW0)
    assert torch.equal((dW0 + A[:, :CA].T @ B[:, :CB]).double(), dW0.double() + A[:, :CA].double().T @ B[:, :CB].double())


@pytest.mark.parametrize("dims", X.WGRAD_GATHER_CASES, ids=_ids)
def test_wgrad_gather_cases(dims):
    x, dz, dW0 = X.wgrad_gather_operands(*dims)
    assert _bf16_exact(x, dz, dW0)
    assert torch.equal(X.wgrad_gather_reference(x, dz, dW0, dims[6], torch.float32).double(), X.wgrad_gather_reference(x, dz, dW0, dims[6]))


def test_pool_helpers_state_the_rule():
    """first maximum in row-major order, and the tied share counts positive ties only"""
    y = torch.tensor([[[[1.0, 3.0, 0.0, 0.0], [3.0, 3.0, 0.0, -1.0]]]])
    assert X.pool_index(y).flatten().tolist() == [1, 0] and X.pool_index(y, last=True).flatten().tolist() == [3, 2]
    assert X.tied_share(y) == 0.5
    assert X.pool(y).flatten().tolist() == [3.0, 0.0]

"""Bit-exact tests of the train-step kernels on integer-valued inputs, with tied pooling maxima (tests/exact_ref.py states the recipe and
the cases once; tests/test_exact_host.py proves on the CPU that every case has exactly one right answer, enough ties, and can fail).

Two things the noise-input parity tests cannot see:

  * LINEAR kernels (forward, data gradient and weight gradient of the convolutions, the ConvTranspose, the GEMMs) must equal a float64
    reference BIT FOR BIT on these inputs -- in any summation order and any of the kernels' precisions -- so a single wrong halo element,
    tap, channel pair or tile-edge column fails, and no reduction reorder can make the test flake;
  * the rule "the pooled gradient goes to the FIRST maximum of the window (row-major), and only if it is positive" is exercised by exact
    ties at positive maxima (10-45 % of the windows here; none in fp32 noise).

Every reference runs on the CPU; every case asserts the route it took."""
import functools

import pytest
import torch

from tests import exact_ref as X
from tests.test_det_ops_gpu import TOL, make_run, nchw, nhwc, oracle_block_bwd_check

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
TIE_FLOOR = 0.10
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def host(t):
    """device NHWC tensor -> float64 NCHW on the CPU"""
    return nchw(t).cpu().double()


def same(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return got.shape == want.shape and torch.equal(got, want)


def bn_buffers(pfx, C, dev):
    return {f"{pfx}.seq.2.running_mean": torch.zeros(C, device=dev), f"{pfx}.seq.2.running_var": torch.ones(C, device=dev),
            f"{pfx}.seq.2.num_batches_tracked": torch.zeros((), dtype=torch.int64, device=dev)}


def block_run(dev, dtype, case):
    """-> (run, P on the device, buffers, input activations a / b, their stored tensors)"""
    from ocrs_models_amd.models import _Act

    N, H, W = case["shape"]
    P = {k: v.to(dev) for k, v in case["P"].items()}
    Bf = bn_buffers(case["pfx"], case["Cout"], dev)
    run = make_run(dev, dtype, N, P, Bf)
    xa_s, tra = nhwc(case["xa"], dtype).to(dev), case["tra"].to(dev)
    a = _Act(xa_s, tra, case["Ca"], H, W)
    b = xb_s = trb = None
    if case["Cb"]:
        xb_s, trb = nhwc(case["xb"], dtype).to(dev), case["trb"].to(dev)
        b = _Act(xb_s, trb, case["Cb"], H, W)
    return run, P, Bf, a, b


@functools.lru_cache(maxsize=None)
def fwd_ref(chans, shape):
    return X.block_reference(X.fwd_block_case(chans, shape), pooled=True, with_grads=False)


@functools.lru_cache(maxsize=None)
def bwd_ref(chans, shape, pooled):
    return X.block_reference(X.bwd_block_case(chans, shape), pooled=pooled)


def check_statistics(run, Bf, pfx, ref, n):
    """batch statistics behind the exact z: saved mean / rstd and the running statistics (the bounds of test_matrix_core_block_forward, which are
    at or below test_dwpw_block_fwd_bwd's 5 * TOL in both dtypes)"""
    sv = run.recs[pfx].saved
    assert X.rel(sv[0], ref["mean"]) < 1e-4 and X.rel(sv[1], torch.rsqrt(ref["var"] + X.BN_EPS)) < 1e-4
    assert X.rel(Bf[f"{pfx}.seq.2.running_mean"], 0.1 * ref["mean"]) < 1e-4
    assert X.rel(Bf[f"{pfx}.seq.2.running_var"], 0.9 + 0.1 * ref["var"] * n / (n - 1)) < 1e-4
    assert int(Bf[f"{pfx}.seq.2.num_batches_tracked"]) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. detection block forward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [False, True], ids=["full", "pool"])
@pytest.mark.parametrize("route,dname,chans,shape", X.FWD_CASES, ids=_ids)
def test_block_forward_bit_exact(dev, route, dname, chans, shape, pool):
    """DepthwiseConv block forward -- k_mm_fwd in its border-cut and whole-tile (FULL, at 2 x 32 x 96) variants and the bf16 row-streaming
    k_rs_fwd ("mm"), k_rs32_fwd ("rs32"), k_dwf / k_dwpw_fwd ("tile") and, where the forward has no fused pooling, k_maxpool_fwd -- stored z
    EQUAL to float64; the pooled raw value is
    the z of the reference's first maximum wherever the pooled activation is positive (ties at a positive maximum have equal z, so the VALUE
    does not depend on the tie rule: the backward tests below check the rule) and, where it is 0, any z of the window -- every element of
    such a window is clamped by the ReLU, the latitude csrc/det_fwd.hip documents at the fused pooling ("Ties between different z ...") and
    no more than that."""
    from ocrs_models_amd._lib import ptr

    dtype = DT[dname]
    case, ref = X.fwd_block_case(chans, shape), fwd_ref(chans, shape)
    Ca, Cb, Cout = chans
    N, H, W = shape
    pfx = case["pfx"]
    run, P, Bf, a, b = block_run(dev, dtype, case)
    assert run.fwd_route(Ca, Cb, Cout, H, W) == route
    assert bool(run.L.mm_fwd_supported(Ca, Cb, Cout, run.dt)) == (route == "mm")
    out = run.block(pfx, a, b, Cout, pool=pool)
    torch.cuda.synchronize()
    assert same(host(out.t), ref["z"]), "z"
    check_statistics(run, Bf, pfx, ref, N * H * W)
    y_ours = X.apply_tr(host(out.t), out.tr.cpu().double())
    assert X.rel(y_ours, ref["y"]) < 5 * TOL[dtype], "bn + relu via the load transform"
    if not pool:
        return
    assert ref["tied"] >= TIE_FLOOR
    praw = run.pooled_by_block
    if praw is None:  # no fused pooling in this configuration: the model's separate pass (raw mode)
        assert route == "tile" and not run.L.dwpw_fwd_pool_supported(Ca + Cb, Cout)
        praw = run.empty(N, H // 2, W // 2, Cout)
        run.L.maxpool_fwd(ptr(out.t), ptr(out.tr), ptr(praw), Cout, N, H, W, 1, run.dt)
        torch.cuda.synchronize()
    praw = host(praw)
    zwin = X.windows(ref["z"])
    zsel = zwin.gather(-1, ref["index"].unsqueeze(-1)).squeeze(-1)
    pos = ref["pooled"] > 0
    assert praw.shape == zsel.shape and torch.equal(praw[pos], zsel[pos]), "pooled raw value at a positive maximum"
    member = (zwin == praw.unsqueeze(-1)).any(-1)
    assert bool(member[~pos].all()), "pooled raw value of an all-clamped window is not one of its z"


@pytest.mark.parametrize("uplane", [True, False], ids=["u", "nou"])
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("N,H,W", X.FIRST_BLOCK_SHAPES)
def test_first_block_forward_bit_exact(dev, dname, N, H, W, uplane):
    """the first block (Cin = 1; csrc/det_c1.hip: per-pixel kernels, and 64 columns x 2 rows per wave with the u plane): stored z and u plane
    EQUAL to float64, batch statistics as for the other blocks"""
    dtype = DT[dname]
    case = X.first_block_case(X.seed_of(3, N, H, W), N, H, W)
    _, u, z = X.block_linear(case, "f64")
    pfx = case["pfx"]
    P = {k: v.to(dev) for k, v in case["P"].items()}
    run = make_run(dev, dtype, N, P, bn_buffers(pfx, 8, dev))
    run.c1_u = uplane
    img = case["img"].to(dev)
    run.x = img
    out = run.block_c1(pfx, img, H, W)
    torch.cuda.synchronize()
    assert (out.u is not None) == bool(uplane and run.L.dwpw_c1_u_supported(N, H, W, run.dt))
    assert (out.u is not None) == (uplane and dname == "bf16" and (N, H, W) == (1, 2, 192))
    assert same(host(out.t), z), "z"
    if out.u is not None:
        assert same(out.u.float().cpu().unsqueeze(1), u), "u plane"
    check_statistics(run, run.Bf, pfx, {"mean": z.mean((0, 2, 3)), "var": z.var((0, 2, 3), unbiased=False)}, N * H * W)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. detection block backward with tied maxima
# ---------------------------------------------------------------------------------------------------------------------------------
# the pointwise-backward kernel of the "tile" route, as ocrs_pw_bwd_kernel numbers them
PW_KERNEL = {"k_pwb": 1, "k_pw_bwd2": 2, "k_pw_bwd2 x2": 3, "k_pw_bwd": 4}


def _block_backward(dev, froute, broute, kernel, dname, chans, shape, pooled):
    dtype = DT[dname]
    case, ref = X.bwd_block_case(chans, shape), bwd_ref(chans, shape, pooled)
    Ca, Cb, Cout = chans
    N, H, W = shape
    pfx = case["pfx"]
    run, P, Bf, a, b = block_run(dev, dtype, case)
    # k_pw_bwd2 (det_pw2.hip) takes the shapes the matrix-core kernels take: it runs where those are off (eval-mode routing, use_mm = False)
    run.use_mm = not kernel.startswith("k_pw_bwd2")
    assert run.fwd_route(Ca, Cb, Cout, H, W) == froute
    out = run.block(pfx, a, b, Cout, pool=pooled)
    torch.cuda.synchronize()
    # kernel and reference see the same z, hence the same ties
    assert same(host(out.t), ref["z"]), "z"
    if pooled:
        assert ref["tied"] >= TIE_FLOOR
    assert run.bwd_route(run.recs[pfx], 1 if pooled else 0, True) == broute
    if broute == "tile":  # "tile" alone does not say which of k_pwb / k_pw_bwd2 / k_pw_bwd runs (block_bwd hands ocrs_pw_bwd_fin a workspace)
        assert run.L.pw_bwd_kernel(Ca, Cb, Cout, run.dt) == PW_KERNEL[kernel]
    else:
        assert kernel in {"mm": ("k_mm_bwd",), "rs32": ("k_rs32_bwd", "k_rs32_bwdp")}[broute] and kernel.endswith("p") == (broute == "rs32" and pooled)
    g1, g2 = (nhwc(t, dtype).to(dev) for t in case["g_pool" if pooled else "g_full"])
    run.G = {k: torch.zeros_like(v) for k, v in P.items()}
    gxa, gxb = run.block_bwd(pfx, g1, g2, 1 if pooled else 0)
    torch.cuda.synchronize()
    errs = {"gxa": X.rel(host(gxa), ref["dx"][:, :Ca])}
    if Cb:
        errs["gxb"] = X.rel(host(gxb), ref["dx"][:, Ca:])
    errs.update({k: X.rel(run.G[k], ref["grads"][k]) for k in P})
    print(f"{dname} {froute}/{broute} {kernel} vs float64 autograd:", {k.split(".", 1)[-1]: f"{v:.1e}" for k, v in errs.items()},
          f"tied {ref.get('tied', 0):.3f}")
    if dtype == torch.bfloat16:
        srcs = [(a.t, a.tr)] + ([(b.t, b.tr)] if Cb else [])
        oracle_block_bwd_check(pfx, P, srcs, g1, g2, 1 if pooled else 0, run, gxa, gxb, z_stored=out.t)
        return
    for k, v in errs.items():
        assert v < 20 * TOL[torch.float32], (k, v)


@pytest.mark.parametrize("froute,broute,kernel,dname,chans,shape", X.BWD_POOLED_CASES, ids=_ids)
def test_block_pooled_backward_with_tied_maxima(dev, froute, broute, kernel, dname, chans, shape):
    """test_block_bwd_through_maxpool on the integer recipe: the pooled gradient (two tensors) through MaxPool2d(2) with 10-16 % of the windows
    tied at a positive maximum.  Each case names the kernel that routes the gradient and asserts it: k_mm_bwd's pooled form ("mm"), k_rs32_bwdp
    ("rs32"), and on the "tile" route k_bn_bwd_reduce + one of k_pwb (det_pwb.hip, PPOOL), k_pw_bwd2 (det_pw2.hip: once, and once per source of
    the 32 | 32 concat; reached with the matrix-core kernels off) and the generic k_pw_bwd (fp32), each followed by k_dw_bwd -- against float64
    autograd through max_pool2d(relu(batch_norm(z))) of the float64 z (first asserted EQUAL to the kernel's); fp32: 20 * TOL as there; bf16:
    the rounding-matched oracle at BF16_DX / BF16_GRAD.  Routing the gradient to the last maximum instead moves dx by 0.4-1.2
    (tests/test_exact_host.py)."""
    _block_backward(dev, froute, broute, kernel, dname, chans, shape, True)


@pytest.mark.parametrize("route,kernel,dname,chans,shape", X.BWD_FULL_CASES, ids=_ids)
def test_block_full_backward_on_integer_inputs(dev, route, kernel, dname, chans, shape):
    """the unpooled backward with two gradient tensors, one case per kernel family"""
    _block_backward(dev, route, route, kernel, dname, chans, shape, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ConvTranspose
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", X.CONVT_CASES, ids=_ids)
def test_conv_transpose_bit_exact(dev, dname, dims):
    """test_conv_transpose's cases (cropped and uncropped) on the recipe: ocrs_convt_fwd / ocrs_convt_bwd (tile kernels; fp32: with k_rs32_ctw for
    the weight gradient at the wide levels) and the fp32 row-streaming k_rs32_ctf / k_rs32_ctd -- output, input gradient, weight and bias gradient
    EQUAL to float64.  Where the entry point also produces the producer's BatchNorm-backward sums (float mean / rstd), the linear outputs stay
    equal and the sums keep the existing tolerance."""
    from ocrs_models_amd._lib import ptr

    dtype = DT[dname]
    Cup, Cout, h, w, H, W = dims
    N = 2
    case = X.convt_case(X.seed_of(4, dims), *dims)
    ref = X.convt_reference(case)
    model_rs = dname == "fp32" and (Cup, Cout) in ((16, 8), (32, 16))  # the shapes the model runs on the row-streaming kernels
    run = make_run(dev, dtype, N, {}, {})
    L = run.L
    xs, tr, Wt, bias = nhwc(case["x"], dtype).to(dev), case["tr"].to(dev), case["W"].to(dev), case["b"].to(dev)
    gy = nhwc(case["gy"], dtype).to(dev)
    out = run.empty(N, H, W, Cout)
    L.convt_fwd(ptr(xs), ptr(tr), ptr(run.pack(Wt, 1, 4 * Cup, 4 * Cout, Cup, 0, 0, 0)), ptr(bias), ptr(out), Cup, Cout, N, h, w, H, W, run.dt)
    torch.cuda.synchronize()
    assert same(host(out), ref["out"]), "forward"
    assert bool(L.rs32_convt_fwd_supported(Cup, Cout, run.dt)) == model_rs and bool(L.rs32_convt_dgrad_supported(Cup, Cout, run.dt)) == model_rs
    if model_rs or (dname == "fp32" and (Cup, Cout) == (32, 32)):  # (the entry point also takes 32 -> 32, as test_conv_transpose runs it)
        out2 = torch.full_like(out, float("nan"))
        L.rs32_convt_fwd(ptr(xs), ptr(tr), ptr(Wt), ptr(bias), ptr(out2), Cup, Cout, N, h, w, H, W)
        torch.cuda.synchronize()
        assert same(host(out2), ref["out"]), "row-streaming forward"
    dx = run.empty(N, h, w, Cup)
    dW, db = torch.zeros_like(Wt), torch.zeros_like(bias)
    ws = torch.empty(L.convt_bwd_ws_floats(Cup, Cout, N, h, w, run.dt), device=dev)
    db64 = torch.zeros(Cout, dtype=torch.float64, device=dev)
    L.convt_bwd(ptr(xs), ptr(tr), ptr(gy), ptr(run.pack(Wt, 0, 9 * Cout, Cup, Cout, 1, 9, 9 * Cout)), ptr(dx), ptr(dW), ptr(db), ptr(db64), ptr(ws), None, None,
                Cup, Cout, N, h, w, H, W, run.dt)
    torch.cuda.synchronize()
    assert same(host(dx), ref["dx"]), "dgrad"
    assert same(dW, ref["dW"]), "wgrad"
    assert same(db.double() + db64, ref["db"]), "dbias"

    g = X.gen(X.seed_of(41, dims))
    saved = torch.stack([0.1 * torch.randn(Cup, generator=g), 1 + 0.2 * torch.rand(Cup, generator=g)]).to(dev)  # [mean | rstd]: floats, behind the linear part
    xf = case["x"].double()
    pre = xf * case["tr"][0].double().view(1, -1, 1, 1) + case["tr"][1].double().view(1, -1, 1, 1)
    gh = torch.where(pre > 0, ref["dx"], torch.zeros_like(ref["dx"]))
    zh = (xf - saved[0].cpu().double().view(1, -1, 1, 1)) * saved[1].cpu().double().view(1, -1, 1, 1)
    ref_sums = torch.cat([gh.sum((0, 2, 3)), (gh * zh).sum((0, 2, 3))])
    if L.rs32_convt_dgrad_supported(Cup, Cout, run.dt):
        for with_stats in (False, True):
            dx3 = torch.full_like(dx, float("nan"))
            gsum3 = torch.zeros(2 * Cup, dtype=torch.float64, device=dev)
            L.rs32_convt_dgrad(ptr(gy), ptr(Wt), ptr(dx3), ptr(xs) if with_stats else None, ptr(tr) if with_stats else None, ptr(saved) if with_stats else None,
                               ptr(gsum3) if with_stats else None, Cup, Cout, N, h, w, H, W)
            torch.cuda.synchronize()
            assert same(host(dx3), ref["dx"]), "row-streaming dgrad"
            if with_stats:
                assert same(gsum3[:Cup], ref_sums[:Cup]), "sum of ghat: integers, exact"
                assert X.rel(gsum3, ref_sums) < 1e-5, "BatchNorm-backward sums (row-streaming dgrad)"
    if L.convt_bwd_stats_supported(Cup, Cout, run.dt):
        gsum = torch.zeros(2 * Cup, dtype=torch.float64, device=dev)
        dx2 = run.empty(N, h, w, Cup)
        dW2, db2 = torch.zeros_like(Wt), torch.zeros_like(bias)
        db64b = torch.zeros(Cout, dtype=torch.float64, device=dev)
        L.convt_bwd(ptr(xs), ptr(tr), ptr(gy), ptr(run.pack(Wt, 0, 9 * Cout, Cup, Cout, 1, 9, 9 * Cout)), ptr(dx2), ptr(dW2), ptr(db2), ptr(db64b), ptr(ws),
                    ptr(saved), ptr(gsum), Cup, Cout, N, h, w, H, W, run.dt)
        torch.cuda.synchronize()
        assert same(host(dx2), ref["dx"]) and same(dW2, ref["dW"]) and same(db2.double() + db64b, ref["db"]), "linear outputs with fused sums"
        assert X.rel(gsum, ref_sums) < 1e-4, "BatchNorm-backward sums"


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. recognition convolutions
# ---------------------------------------------------------------------------------------------------------------------------------
def rec_run(dev, dtype, N, H=64, W=64):
    from ocrs_models_amd.recognition import _RecRun

    r = _RecRun({}, {}, dev, dtype, N, H, W)
    r.G = {}
    return r


CONV_KERNEL = {0: "k_conv_igemm", 1: "k_conv3x3_tile", 2: "k_conv3x3_rows", 3: "k_conv3x3_c128"}  # as ocrs_conv_igemm_kernel numbers them
# bf16: (forward, input gradient) kernel of each case
CONV_BF16_KERNELS = {(32, 64, 3, 1, 12, 20, 3): ("k_conv3x3_tile", "k_conv3x3_tile"), (32, 64, 3, 1, 32, 77, 3): ("k_conv3x3_tile", "k_conv3x3_tile"),
                     (64, 128, 3, 1, 9, 17, 3): ("k_conv3x3_rows", "k_conv3x3_rows"), (128, 128, 3, 1, 8, 33, 3): ("k_conv3x3_rows", "k_conv3x3_rows"),
                     (128, 128, 2, 1, 4, 19, 3): ("k_conv3x3_rows", "k_conv3x3_rows"), (128, 128, 3, 1, 21, 16, 3): ("k_conv3x3_rows", "k_conv3x3_rows"),
                     (128, 64, 3, 1, 16, 37, 3): ("k_conv3x3_rows", "k_conv3x3_rows"), (64, 128, 3, 1, 8, 80, 2): ("k_conv3x3_c128", "k_conv_igemm")}


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", X.CONV_CASES, ids=_ids)
def test_recognition_conv_bit_exact(dev, dname, dims, monkeypatch):
    """ocrs_conv_igemm forward (bias + ReLU, batch sums), its input gradient (the same entry point on the flipped pack) and the weight gradient,
    all EQUAL to float64.  The kernel the launcher picks from the shape is asserted through ocrs_conv_igemm_kernel: fp32 -> k_conv_igemm for every
    case, weight gradient k_conv3x3_wgrad (3x3) / k_wgrad_gather (2x2); bf16 -> CONV_BF16_KERNELS above (k_conv3x3_tile where Cin * M <= 2048,
    k_conv3x3_rows for ragged or short rows and the 2x2 layer, k_conv3x3_c128 for the added case, whose 128 -> 64 input gradient none of the
    three takes: the generic k_conv_igemm in bf16), weight gradient k_conv3x3_wgrad_tr / k_wgrad_gather_tr."""
    dtype = DT[dname]
    ci, co, k, pad, H, W, N = dims
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    case = X.conv_case(X.seed_of(5, dims), *dims)
    ref = X.conv_reference(case)
    r = rec_run(dev, dtype, N)
    w, b = case["w"].to(dev), case["b"].to(dev)
    r.P, r.G = {"w": w}, {"w": torch.zeros_like(w)}
    rec = {"conv_igemm": [], "conv3x3_wgrad": [], "wgrad_gather": [], "wgrad_gemm_x3": []}
    monkeypatch.setattr(r.L, "timing", rec)
    xs = nhwc(case["x"], dtype).to(dev)
    out, gstat = r.conv(xs, w, b, True, True, H, W, pad, Ho, Wo)
    torch.cuda.synchronize()
    assert same(host(out), ref["out"]), "forward"
    assert ref["sums_exact"]
    assert same(gstat[:co], ref["s1"]) and same(gstat[co:2 * co], ref["s2"]), "batch sums"
    dz = nhwc(case["dz"], dtype).to(dev)
    dx = r.conv_bwd("w", dz, xs, Ho, Wo, H, W, pad)
    torch.cuda.synchronize()
    assert same(host(dx), ref["dx"]), "dgrad"
    assert same(r.G["w"], ref["dW"]), "wgrad"
    assert len(rec["conv_igemm"]) == 2 and all(a[-1] == r.dt for _, _, a in rec["conv_igemm"])
    # ... and the kernel the launcher took for each of the two, from the arguments the calls were made with
    # (ocrs_conv_igemm(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype))
    took = tuple(CONV_KERNEL[r.L.conv_igemm_kernel(a[1], a[4], a[8], a[9], *a[11:20])] for _, _, a in rec["conv_igemm"])
    assert took == (("k_conv_igemm", "k_conv_igemm") if dname == "fp32" else CONV_BF16_KERNELS[dims]), took
    assert (len(rec["conv3x3_wgrad"]), len(rec["wgrad_gather"]), len(rec["wgrad_gemm_x3"])) == ((1, 0, 0) if k == 3 else (0, 1, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. conv0
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", X.CONV0_SHAPES, ids=_ids)
def test_conv0_bit_exact_with_tied_maxima(dev, dname, shape):
    """ocrs_conv0_fwd / ocrs_conv0_bwd (csrc/rec_conv0.hip: k_conv0_bwd in fp32 and for odd W, k_conv0_bwd_mm for a bf16 gradient with even W)
    on an integer image and ternary weights: pooled output, dW and db EQUAL to float64 autograd of max_pool2d(relu(conv2d)) -- whose rule is:
    the gradient goes to the first maximum of the window in row-major order, and only if it is positive.  13-16 % of the windows are tied at
    a positive maximum; routing to the last maximum instead moves dW by 0.42-0.45 (tests/test_exact_host.py)."""
    from ocrs_models_amd._lib import ptr

    dtype = DT[dname]
    N, H, W = shape
    case = X.conv0_case(X.seed_of(6, shape), *shape)
    ref = X.conv0_reference(case)
    assert ref["tied"] >= TIE_FLOOR
    r = rec_run(dev, dtype, N, H, W)
    img, w, b = case["img"].to(dev), case["w"].to(dev), case["b"].to(dev)
    out = r.empty(N, H // 2, W // 2, 32)
    r.L.conv0_fwd(ptr(img), ptr(w), ptr(b), ptr(out), N, H, W, r.dt)
    gy = nhwc(case["gy"], dtype).to(dev)
    dW, db = torch.zeros_like(w), torch.zeros_like(b)
    r.L.conv0_bwd(ptr(img), ptr(w), ptr(b), ptr(gy), ptr(dW), ptr(db), N, H, W, r.dt)
    torch.cuda.synchronize()
    assert same(host(out), ref["out"]), "pooled output"
    assert same(dW, ref["dW"]), "dW"
    assert same(db, ref["db"]), "db"


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. act_pool_fwd, rec_bn_reduce, dz_apply
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", X.POOL_PIECES_CASES, ids=_ids)
def test_bn_relu_pool_pieces_bit_exact(dev, dname, dims):
    """the cases of test_bn_relu_pool_forward_and_backward_pieces (2x2 / 2x1 / no pooling; windows that tile the tensor exactly and floor mode
    with a partial last row, a partial last column or both: k_dz_apply's EDGE form) with dyadic tr / saved / coef (one negative-scale channel):
    pooled output, gsum, dz and dsum EQUAL to float64, with 19-44 % of the windows tied at a positive maximum."""
    from ocrs_models_amd._lib import lib, ptr
    from ocrs_models_amd.models import _DT

    dtype = DT[dname]
    L, dt = lib(), _DT[dtype]
    N, H, W, C, PH, PW = dims
    case = X.pool_pieces_case(X.seed_of(7, dims), *dims)
    ref = X.pool_pieces_reference(case)
    z, gy = nhwc(case["z"], dtype).to(dev), nhwc(case["gy"], dtype).to(dev)
    tr, saved, coef = case["tr"].contiguous().to(dev), case["saved"].contiguous().to(dev), case["coef"].contiguous().to(dev)
    if PH * PW > 1:
        assert ref["tied"] >= TIE_FLOOR
    out = torch.empty(N, H // PH, W // PW, C, dtype=dtype, device=dev)
    L.act_pool_fwd(ptr(z), ptr(tr), ptr(out), C, N, H, W, PH, PW, dt)
    torch.cuda.synchronize()
    assert same(host(out), ref["out"]), "pooled output"
    gsum = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    L.rec_bn_reduce(ptr(gy), ptr(z), ptr(tr), ptr(saved), ptr(gsum), C, N, H, W, PH, PW, dt)
    dz = torch.empty_like(z)
    dsum = torch.full((C,), 0.25, device=dev)
    L.dz_apply(ptr(gy), ptr(z), ptr(tr), ptr(coef), ptr(dz), C, N, H, W, PH, PW, dt, ptr(dsum))
    torch.cuda.synchronize()
    assert same(gsum, ref["gsum"]), "gsum"
    assert same(host(dz), ref["dz"]), "dz"
    assert same(dsum, ref["dsum"] + 0.25), "dsum"  # (multiples of 0.25 far below 2^22: the caller's 0.25 adds exactly)


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", X.AVGPOOL_CASES, ids=_ids)
def test_avgpool_pieces_bit_exact(dev, dname, dims):
    """BatchNorm + AvgPool2d((4,1)) + permute (ocrs_avgpool_fwd / _bn_reduce / _dz) on integer z and gseq with dyadic tr / saved / coef: seq, gsum and
    dz EQUAL to float64.  Singled out: seq is laid out [W][N][C], and every row of dz from the fifth on is coef1 z + coef2 with no share of
    the gradient (the pool has ONE output row, from rows 0..3)."""
    from ocrs_models_amd._lib import lib, ptr
    from ocrs_models_amd.models import _DT

    dtype = DT[dname]
    L, dt = lib(), _DT[dtype]
    N, H, W, C = dims
    case = X.avgpool_case(X.seed_of(12, dims), *dims)
    ref = X.avgpool_reference(case)
    z, gseq = nhwc(case["z"], dtype).to(dev), case["gseq"].contiguous().to(dev)
    tr, saved, coef = case["tr"].contiguous().to(dev), case["saved"].contiguous().to(dev), case["coef"].contiguous().to(dev)
    seq = torch.full((W, N, C), float("nan"), device=dev)
    L.avgpool_fwd(ptr(z), ptr(tr), ptr(seq), C, N, H, W, dt)
    gsum = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    L.avgpool_bn_reduce(ptr(gseq), ptr(z), ptr(saved), ptr(gsum), C, N, H, W, dt)
    dz = torch.full_like(z, float("nan"))
    L.avgpool_dz(ptr(gseq), ptr(z), ptr(coef), ptr(dz), C, N, H, W, dt)
    torch.cuda.synchronize()
    if N > 1 and W > 1:
        assert not same(seq.view(N, W, C).transpose(0, 1), ref["seq"]), "seq is laid out [N][W][C], not [W][N][C]"
    assert same(seq, ref["seq"]), "seq"
    assert same(gsum, ref["gsum"]), "gsum"
    got = host(dz)
    assert same(got[:, :, 4:], ref["tail"]), "rows 4.. of dz: coef1 z + coef2, no share of the gradient"
    assert same(got[:, :, :4], ref["dz"][:, :, :4]), "rows 0..3 of dz"


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. GEMMs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K,M,ldo", X.GEMM_CASES)
def test_exact_fp32_gemm_bit_exact(dev, P, K, M, ldo):
    """the exact-fp32 packed GEMM of parity mode (_RecRun.gemm: ocrs_conv_igemm as a 1x1 convolution, split-bf16 fragments): EQUAL to float64 on
    integer operands with |v| <= 4 (the low planes of the split are zero here by construction; the noise-input tests keep covering them)."""
    from ocrs_models_amd.packs import fwd_row

    Xm, Wkm, bias = X.gemm_operands(X.seed_of(8, P, K, M), P, K, M)
    r = rec_run(dev, torch.float32, 1)
    w = Wkm.T.contiguous().to(dev)  # [M][K]
    out = r.gemm(Xm.to(dev), K, K, r.packs.fetch(fwd_row(w, 0), dev), bias.to(dev), M, ldo, P)
    torch.cuda.synchronize()
    assert same(out[:, :M], Xm.double() @ Wkm.double() + bias.double())


@pytest.mark.parametrize("P,K,M,km,kw", X.GEMM_X3_CASES)
def test_split_bf16_gemm_bit_exact(dev, P, K, M, km, kw):
    """ocrs_gemm_x3 (both weight layouts, ragged P and M, kw) and, where it takes the shape, the pipelined ocrs_gemm_x3p on the pre-split pack:
    EQUAL to float64 on integer operands with |v| <= 4.  The split-bf16 low planes are zero here by construction -- test_split_bf16_gemm and
    test_pipelined_split_bf16_gemm_is_bit_identical keep covering them."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    Kw = kw or K
    Xm, Wkm, bias = X.gemm_operands(X.seed_of(9, P, K, M), P, K, M)
    Xm[:, Kw:] = 0  # (kw: x's columns [kw, K) are zero, W has only kw rows)
    Wkm = Wkm[:Kw]
    want = Xm[:, :Kw].double() @ Wkm.double() + bias.double()
    Xd, bd = Xm.to(dev), bias.to(dev)
    Wd = (Wkm if km else Wkm.T).contiguous().to(dev)
    M4 = (M + 3) // 4 * 4
    ldo = M4 + 4
    out = torch.full((P, ldo), 7.0, device=dev)
    L.gemm_x3(ptr(Xd), K, K, ptr(Wd), M if km else Kw, km, ptr(bd), ptr(out), ldo, M, P, kw)
    torch.cuda.synchronize()
    assert same(out[:, :M], want)
    assert float(out[:, M:M4].abs().max()) == 0.0 if M4 > M else True
    assert float((out[:, M4:] - 7.0).abs().max()) == 0.0
    assert bool(L.gemm_x3p_supported(K, K, ldo, M, P)) == (M % 128 == 0)
    if L.gemm_x3p_supported(K, K, ldo, M, P):
        wpk = torch.empty(2 * L.pack_frags_bytes(Kw, M, 1), dtype=torch.uint8, device=dev)
        L.pack_frags(ptr(Wd), 2, Kw, M, Kw, 0, M if km else 1, 1 if km else Kw, ptr(wpk), 1)
        out2 = torch.full((P, ldo), 7.0, device=dev)
        L.gemm_x3p(ptr(Xd), K, K, ptr(wpk), ptr(bd), ptr(out2), ldo, M, P)
        torch.cuda.synchronize()
        assert same(out2[:, :M], want) and float((out2[:, M:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("P,CA,ldA,CB,ldB", X.WGRAD_GEMM_CASES)
def test_split_bf16_wgrad_gemm_bit_exact(dev, P, CA, ldA, CB, ldB):
    """ocrs_wgrad_gemm_x3 (leading dimensions != widths, ragged sizes, accumulation into an integer dW): EQUAL to float64.  Low planes zero by
    construction; test_split_bf16_wgrad_gemm keeps covering them."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    A, B, dW0 = X.wgrad_gemm_operands(P, CA, ldA, CB, ldB)
    Ad, Bd, dW = A.to(dev), B.to(dev), dW0.to(dev)
    ws = torch.empty(L.wgrad_gemm_x3_ws_floats(CA, CB, P), dtype=torch.float32, device=dev)
    L.wgrad_gemm_x3(ptr(Ad), ldA, CA, ptr(Bd), ldB, CB, ptr(dW), ptr(ws), P)
    torch.cuda.synchronize()
    assert same(dW, dW0.double() + A[:, :CA].double().T @ B[:, :CB].double())


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("N,CA,CB,H,W,K,pad", X.WGRAD_GATHER_CASES)
def test_gathered_weight_gradient_bit_exact(dev, dname, N, CA, CB, H, W, K, pad):
    """ocrs_wgrad_gather (workspace flush; k_wgrad_gather in fp32, k_wgrad_gather_tr in bf16) as the weight gradient of a stride-1 Conv2d: ragged
    channel counts, positions that are no multiple of the chunk, accumulation into an integer dW -- EQUAL to float64 autograd."""
    from ocrs_models_amd._lib import lib, ptr
    from ocrs_models_amd.models import _DT

    dtype = DT[dname]
    L, dt = lib(), _DT[dtype]
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    x, dz, dW0 = X.wgrad_gather_operands(N, CA, CB, H, W, K, pad)
    dW = dW0.clone().to(dev)
    A, B = nhwc(dz, dtype).to(dev), nhwc(x, dtype).to(dev)
    ws = torch.empty(L.wgrad_gather_ws_floats(CA, CB, K * K, N * Ho * Wo, dt), dtype=torch.float32, device=dev)
    L.wgrad_gather(ptr(A), CA, CA, None, ptr(B), CB, CB, ptr(dW), ptr(ws), N, Ho, Wo, H, W, 1, pad, pad, K, K, dt)
    torch.cuda.synchronize()
    assert same(dW, X.wgrad_gather_reference(x, dz, dW0, pad))

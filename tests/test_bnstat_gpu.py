"""The small kernels every training step runs between the heavy ones, each called on its own through the C ABI and compared with float64 on the
CPU.  tests/bnstat_ref.py states the references, the emulations, the bounds (each with its derivation) and the cases once;
tests/test_bnstat_host.py proves on the CPU what these tests rest on.

  1 ocrs_bn_finalize from exact float64 sums: saved mean | rstd within one float32 ulp of the rounded float64 value (the number of unequal
    elements is printed), tr[0], tr[1] and the running statistics within counted roundings, tr[2] and num_batches_tracked exact, two calls in
    a row, nothing written outside the tensors.  ocrs_bn_finalize_parts on integer partials: bit-identical to ocrs_bn_finalize on the totals.
  2 bn_finalize -> act_pool_fwd -> rec_bn_reduce -> bn_bwd_finalize -> dz_apply against float64 autograd of BatchNorm(train) -> ReLU ->
    max_pool2d: dz per element in the unit 2^-24 (|A ghat| + |B z| + |C|) at most twice what the float32 CPU emulation of the same arithmetic
    reaches (bf16: at most one bf16 ulp from the rounded float64 dz on at most 1 % of the elements), dgamma / dbeta within the bound of the
    sums plus one ulp, and the two sums the coefficient formulas exist for.
  3 the same for BatchNorm -> AvgPool2d((4,1)) -> permute (ocrs_avgpool_*); H outside 4..7 is refused.
  4 ocrs_col_sum: exact on integers for every loop of both kernels, bounded on random floats, and inside a deferral window (exact, reproducible,
    a full job queue, a used-up workspace).
  5 ocrs_fold64_multi: one rounding of the float64 sum.
"""
import numpy as np
import pytest
import torch

from tests import bnstat_ref as R
from tests.lossopt_ref import ulp32

pytestmark = pytest.mark.gpu

SENT = -777.0
DT = {"fp32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def up(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def padded(n, dev, dtype=torch.float32, fill=None, pad=8):
    """-> (buffer of pad + n + pad sentinels, its middle n elements as a view); fill: the view's initial values"""
    buf = torch.full((n + 2 * pad,), SENT if dtype.is_floating_point else int(SENT), dtype=dtype, device=dev)
    view = buf[pad:pad + n]
    if fill is not None:
        view.copy_(fill if torch.is_tensor(fill) else torch.full((n,), fill, dtype=dtype))
    return buf, view


def untouched(buf, n, pad=8):
    b = buf.cpu()
    return bool((b[:pad] == SENT).all()) and bool((b[pad + n:] == SENT).all())


def np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want) / bound
    i = int(err.argmax())
    assert err.flat[i] <= 1.0, f"{what}[{i}]: {np.asarray(got).flat[i]!r} vs {np.asarray(want).flat[i]!r}, {err.flat[i]:.2f}x the bound"
    return float(err.max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the statistics
# ---------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("running", [True, False], ids=["running", "null"])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("count", R.FIN_COUNTS)
@pytest.mark.parametrize("C", R.FIN_C)
def test_bn_finalize_against_float64(dev, C, count, bf16, running):
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    case = R.fin_case(C, count, bf16)
    gstat, gamma, beta = up(case["gstat"].reshape(-1), dev), up(case["gamma"], dev), up(case["beta"], dev)
    tr_buf, tr = padded(3 * C, dev)
    sv_buf, saved = padded(2 * C, dev)
    rm_buf, rm = padded(C, dev, fill=R.FIN_PREFILL[0])
    rv_buf, rv = padded(C, dev, fill=R.FIN_PREFILL[1])
    nbt_buf, nbt = padded(1, dev, torch.int64, fill=R.FIN_PREFILL[2])
    unequal = 0
    for call in (1, 2):  # nbt counts, the running statistics chain: each call is checked from the float32 state the one before left
        old_m, old_v = rm.cpu().numpy(), rv.cpu().numpy()
        L.bn_finalize(ptr(gstat), count, C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(tr), ptr(saved), ptr(rm) if running else None,
                      ptr(rv) if running else None, ptr(nbt) if running else None, R.FIN_LO)
        torch.cuda.synchronize()
        ref = R.finalize_ref64(case["gstat"], count, case["gamma"], case["beta"], old_m, old_v)
        t, s = tr.cpu().numpy().reshape(3, C), saved.cpu().numpy().reshape(2, C)
        for name, got, want in (("saved mean", s[0], ref["mean"]), ("saved rstd", s[1], ref["rstd"])):
            w32 = want.astype(np.float32)
            assert (np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= ulp32(w32)).all(), name
            unequal += int((got != w32).sum())
        within(t[0], ref["sc"], ref["sc_bound"], "tr[0]")
        within(t[1], ref["sh"], ref["sh_bound"], "tr[1]")
        assert (t[2] == np.float32(R.FIN_LO)).all(), "tr[2] is lo"
        if running:
            within(rm.cpu().numpy(), ref["run_mean"], ref["run_mean_bound"], "run_mean")
            within(rv.cpu().numpy(), ref["run_var"], ref["run_var_bound"], "run_var")
            assert int(nbt.item()) == R.FIN_PREFILL[2] + call
        else:
            assert bool((rm == R.FIN_PREFILL[0]).all()) and bool((rv == R.FIN_PREFILL[1]).all()) and int(nbt.item()) == R.FIN_PREFILL[2]
        for buf, n in ((tr_buf, 3 * C), (sv_buf, 2 * C), (rm_buf, C), (rv_buf, C), (nbt_buf, 1)):
            assert untouched(buf, n), "written outside the tensor"
    print(f"bn_finalize C={C} count={count}: {unequal} of {4 * C} saved values not equal to the rounded float64 value")


@pytest.mark.parametrize("nparts,C", R.PARTS_CASES)
def test_bn_finalize_parts_equals_bn_finalize_on_the_totals(dev, nparts, C):
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    case = R.parts_case(nparts, C)
    gamma, beta = up(case["gamma"], dev), up(case["beta"], dev)
    res = []
    for which in ("parts", "totals"):
        bufs = [padded(3 * C, dev), padded(2 * C, dev), padded(C, dev, fill=R.FIN_PREFILL[0]), padded(C, dev, fill=R.FIN_PREFILL[1]),
                padded(1, dev, torch.int64, fill=R.FIN_PREFILL[2])]
        (_, tr), (_, saved), (_, rm), (_, rv), (_, nbt) = bufs
        for _ in range(2):
            if which == "parts":
                parts = up(case["parts"].reshape(-1), dev)
                L.bn_finalize_parts(ptr(parts), nparts, case["count"], C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(tr), ptr(saved), ptr(rm), ptr(rv), ptr(nbt),
                                    R.FIN_LO)
            else:
                gstat = up(case["gstat"].reshape(-1), dev)
                L.bn_finalize(ptr(gstat), case["count"], C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(tr), ptr(saved), ptr(rm), ptr(rv), ptr(nbt), R.FIN_LO)
        torch.cuda.synchronize()
        for (buf, _), n in zip(bufs, (3 * C, 2 * C, C, C, 1)):
            assert untouched(buf, n), "written outside the tensor"
        res.append([b.cpu() for b, _ in bufs])
    for name, a, b in zip(("tr", "saved", "run_mean", "run_var", "nbt"), *res):
        assert torch.equal(a, b), name
    assert int(res[0][4][8]) == R.FIN_PREFILL[2] + 2
    ref = R.finalize_ref64(case["gstat"], case["count"], case["gamma"], case["beta"])
    within(res[0][0][8:8 + C].numpy(), ref["sc"], ref["sc_bound"], "tr[0]")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the backward chains
# ---------------------------------------------------------------------------------------------------------------------------------------


def check_chain(name, case, ref, emul, dname, dz, dgamma, dbeta):
    """dz (NHWC numpy, float32 values), dgamma, dbeta of the kernels against the float64 reference, by the emulation's measure"""
    C = case["gamma"].size
    if dname == "fp32":
        e_emul, e_gpu = R.dz_units(emul["dz"], ref), R.dz_units(dz, ref)
        print(f"{name}: dz in units of 2^-24 (|A ghat| + |B z| + |C|): emulation {e_emul:.2f}, GPU {e_gpu:.2f}")
        assert e_gpu <= 2.0 * e_emul
        bound = 2.0 * e_emul * ref["unit"]
    else:
        worst, share = R.bf16_offsets(dz, ref)
        w_e, s_e = R.bf16_offsets(emul["dz"], ref)
        print(f"{name}: bf16 dz unequal to the rounded float64 dz: emulation {s_e:.5f} (max {w_e:.0f} ulp), GPU {share:.5f} (max {worst:.0f} ulp)")
        assert worst <= 1.0 and share <= R.BF16_OFF_BY_ONE_SHARE
        bound = 1.5 * R.ulp_bf16(R.bf16_from64(ref["dz"]))  # half an ulp of storage rounding and the one allowed above
    e1, e2 = R.gsum_bounds(case, ref)
    b = within(dbeta, ref["dbeta"], e1 + ulp32(ref["dbeta"]), "dbeta")
    g = within(dgamma, ref["dgamma"], e2 + ulp32(ref["dgamma"]), "dgamma")
    i0, i1, _, _ = R.identities(case, ref, dz, bound)
    print(f"{name}: dbeta {b:.3f}, dgamma {g:.3f} of their bounds; sum dz {i0:.3f}, sum dz zhat {i1:.3f} of the summed per-element bound")
    assert i0 <= 1.0 and i1 <= 1.0
    assert dz.shape[-1] == C


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", R.CHAIN_CASES, ids=_ids)
def test_bn_relu_maxpool_backward_chain(dev, dims, dname):
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    dtype, dt = DT[dname]
    N, H, W, C, PH, PW = dims
    case, ref, emul = R.chain_case(dims, dname), R.chain_reference(dims, dname), R.chain_emul(dims, dname)
    assert ref["close"] == 0
    z, gy = up(case["z"], dev, dtype), up(case["gy"], dev, dtype)
    gamma, beta, gstat = up(case["gamma"], dev), up(case["beta"], dev), up(case["gstat"].reshape(-1), dev)
    tr, saved, coef = (torch.full((k * C,), float("nan"), device=dev) for k in (3, 2, 3))
    dgamma, dbeta = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    out = torch.empty(N, H // PH, W // PW, C, dtype=dtype, device=dev)
    gsum = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    dz = torch.empty_like(z)
    L.bn_finalize(ptr(gstat), case["count"], C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(tr), ptr(saved), None, None, None, 0.0)
    L.act_pool_fwd(ptr(z), ptr(tr), ptr(out), C, N, H, W, PH, PW, dt)
    L.rec_bn_reduce(ptr(gy), ptr(z), ptr(tr), ptr(saved), ptr(gsum), C, N, H, W, PH, PW, dt)
    L.bn_bwd_finalize(ptr(gsum), case["count"], C, ptr(gamma), ptr(saved), ptr(coef), ptr(dgamma), ptr(dbeta))
    L.dz_apply(ptr(gy), ptr(z), ptr(tr), ptr(coef), ptr(dz), C, N, H, W, PH, PW, dt, None)
    torch.cuda.synchronize()
    name = f"chain {_ids(dims)} {dname}"
    if dname == "fp32":
        within(np64(out), ref["out"], R.act_out_bound(case), "pooled activation")
    else:
        want = R.bf16_from64(ref["out"])
        assert (np.abs(np64(out) - want) <= R.ulp_bf16(want)).all(), "pooled activation: more than one bf16 ulp"
    check_chain(name, case, ref, emul, dname, np64(dz), dgamma.cpu().numpy(), dbeta.cpu().numpy())


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_bn_avgpool_backward_chain(dev, dname):
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    dtype, dt = DT[dname]
    dims = R.AVG_CHAIN
    N, H, W, C = dims
    case, ref, emul = R.chain_case(dims, dname, None, True), R.chain_reference(dims, dname, None, True), R.chain_emul(dims, dname, None, True)
    z, gseq = up(case["z"], dev, dtype), up(case["gy"], dev)
    gamma, beta, gstat = up(case["gamma"], dev), up(case["beta"], dev), up(case["gstat"].reshape(-1), dev)
    tr, saved, coef = (torch.full((k * C,), float("nan"), device=dev) for k in (3, 2, 3))
    dgamma, dbeta = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    seq = torch.full((W, N, C), float("nan"), device=dev)
    gsum = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    dz = torch.empty_like(z)
    L.bn_finalize(ptr(gstat), case["count"], C, ptr(gamma), ptr(beta), 1e-5, 0.1, ptr(tr), ptr(saved), None, None, None, float("-inf"))
    L.avgpool_fwd(ptr(z), ptr(tr), ptr(seq), C, N, H, W, dt)
    L.avgpool_bn_reduce(ptr(gseq), ptr(z), ptr(saved), ptr(gsum), C, N, H, W, dt)
    L.bn_bwd_finalize(ptr(gsum), case["count"], C, ptr(gamma), ptr(saved), ptr(coef), ptr(dgamma), ptr(dbeta))
    L.avgpool_dz(ptr(gseq), ptr(z), ptr(coef), ptr(dz), C, N, H, W, dt)
    torch.cuda.synchronize()
    within(np64(seq), ref["out"], R.avg_out_bound(case, ref), "seq")
    check_chain(f"avgpool chain {_ids(dims)} {dname}", case, ref, emul, dname, np64(dz), dgamma.cpu().numpy(), dbeta.cpu().numpy())


@pytest.mark.parametrize("H", [3, 8])
def test_avgpool_entry_points_refuse_other_heights(dev, H):
    """One pooled row from rows 0..3: AvgPool2d((4,1)) only for 4 <= H <= 7.  H = 3 (would read past the image) and H = 8 (a second pooled row) are
    OCRS_ERR_ARG for all three, nothing is launched and the outputs keep their sentinel.  z is allocated as if H were 8."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    N, W, C = 2, 6, 128
    z = torch.randn(N, 8, W, C, device=dev)
    tr = torch.stack([torch.ones(C), torch.zeros(C), torch.zeros(C)]).to(dev)
    gseq = torch.randn(W, N, C, device=dev)
    seq, dz = torch.full((W, N, C), 7.0, device=dev), torch.full_like(z, 7.0)
    gsum = torch.full((2 * C,), 7.0, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        L.avgpool_fwd(ptr(z), ptr(tr), ptr(seq), C, N, H, W, 0)
    with pytest.raises(RuntimeError, match="bad argument"):
        L.avgpool_bn_reduce(ptr(gseq), ptr(z), ptr(tr), ptr(gsum), C, N, H, W, 0)
    with pytest.raises(RuntimeError, match="bad argument"):
        L.avgpool_dz(ptr(gseq), ptr(z), ptr(tr), ptr(dz), C, N, H, W, 0)
    with pytest.raises(RuntimeError, match="bad argument"):
        L.avgpool_bn_reduce(ptr(gseq), ptr(z), ptr(tr), ptr(gsum), 24, N, 5, W, 0)  # (256 % (C / 8) stays a condition of the reduce)
    torch.cuda.synchronize()
    for t in (seq, gsum, dz):
        assert bool((t == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. column sums
# ---------------------------------------------------------------------------------------------------------------------------------------


def col_operand(a_np, dev, dtype, off):
    """[rows][ld] -> a device view starting `off` elements into a larger buffer"""
    buf = torch.zeros(a_np.size + 8, dtype=dtype, device=dev)
    v = buf[off:off + a_np.size]
    v.copy_(torch.from_numpy(np.array(a_np)).reshape(-1))
    return v


COL_SHAPES = [(C, ld, 0) for C, ld in R.COL4_SHAPES] + list(R.COL1_SHAPES)


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", COL_SHAPES, ids=_ids)
def test_col_sum_exact_on_integers(dev, shape, dname):
    """out[c] += sum over the rows, on integers in [-2, 2] (one right answer in any order), onto a prefilled out.  Row counts (tests/bnstat_ref.py
    col4_plan states the arithmetic): 1, 3, 16, 17 inside one or two blocks; 4099 the 4-row loop and the tail; 14337, 16389, 40000 at the full grid
    of 2 blocks per CU: the 8-row loop for one thread only / for all with one tail row for five threads / twice, then the 4-row loop or the tail."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    dtype, dt = DT[dname]
    C, ld, off = shape
    vec4 = C % 4 == 0 and ld % 4 == 0 and off == 0
    for rows in R.COL_ROWS:
        if C == 1536 and rows > R.COL_WIDE_MAX_ROWS:
            continue
        a_np = R.col_ints(rows, ld)
        a = col_operand(a_np, dev, dtype, off)
        assert (a.data_ptr() % (16 if dname == "fp32" else 8) == 0) == (off == 0)
        pre = R.col_prefill(C)
        out_buf, out = padded(C, dev, fill=up(pre, dev))
        L.col_sum(ptr(a), ld, C, ptr(out), rows, dt)
        torch.cuda.synchronize()
        want = a_np[:, :C].astype(np.float64).sum(0) + pre
        got = out.cpu().numpy().astype(np.float64)
        assert np.array_equal(got, want), (f"{'k_col_sum4' if vec4 else 'k_col_sum'} rows={rows}: column {int(np.flatnonzero(got != want)[0])}: "
                                           f"{got[got != want][0]} vs {want[got != want][0]}")
        assert untouched(out_buf, C), f"rows={rows}: columns past C written"


@pytest.mark.parametrize("shape,rows", [((128, 132, 0), 40000), ((1536, 1536, 0), 4099), ((97, 128, 0), 40000), ((128, 128, 1), 4099)], ids=_ids)
def test_col_sum_on_random_floats(dev, shape, rows):
    """|out - float64| <= chain * 2^-24 * sum |a| per column: every add of the longest chain between an element and out[c] rounds a partial sum
    that is at most sum |a| (col_chain derives the chain from the grid the launcher picks)"""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    C, ld, off = shape
    a_np = np.random.RandomState(rows + C).standard_normal((rows, ld)).astype(np.float32)
    a = col_operand(a_np, dev, torch.float32, off)
    out = torch.zeros(C, device=dev)
    L.col_sum(ptr(a), ld, C, ptr(out), rows, 0)
    torch.cuda.synchronize()
    a64 = a_np[:, :C].astype(np.float64)
    chain = R.col_chain(rows, off == 0 and C % 4 == 0 and ld % 4 == 0)
    e = within(out.cpu().numpy(), a64.sum(0), chain * R.U * np.abs(a64).sum(0), "column")
    print(f"col_sum {shape} rows={rows}: {e:.4f} of the bound (chain {chain})")


def test_col_sum_inside_a_deferral_window(dev):
    """bwd_defer_begin(None, 0) .. bwd_defer_flush(): the sums are complete after the flush, exact on integers for both kernels, and three identical
    windows on random floats leave identical bytes; a second begin inside an open window is refused."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    jobs = [((128, 132, 0), 40000), ((8, 8, 0), 17), ((97, 128, 0), 4099), ((128, 128, 1), 3)]
    ints = [(s, r, R.col_ints(r, s[1]), col_operand(R.col_ints(r, s[1]), dev, torch.float32, s[2])) for s, r in jobs]
    rnd_np = [np.random.RandomState(5 + i).standard_normal((r, s[1])).astype(np.float32) for i, (s, r) in enumerate(jobs)]
    rnd = [col_operand(a, dev, torch.float32, s[2]) for a, (s, _) in zip(rnd_np, jobs)]
    runs = []
    for rep in range(3):
        outs_i = [padded(s[0], dev, fill=up(R.col_prefill(s[0]), dev)) for s, _ in jobs]
        outs_r = [torch.zeros(s[0], device=dev) for s, _ in jobs]
        L.bwd_defer_begin(None, 0)
        try:
            if rep == 0:
                with pytest.raises(RuntimeError, match="bad argument"):
                    L.bwd_defer_begin(None, 0)
            for (s, r, _, a), (_, o) in zip(ints, outs_i):
                L.col_sum(ptr(a), s[1], s[0], ptr(o), r, 0)
            for (s, r), a, o in zip(jobs, rnd, outs_r):
                L.col_sum(ptr(a), s[1], s[0], ptr(o), r, 0)
        finally:
            L.bwd_defer_flush()
        torch.cuda.synchronize()
        for (s, r, a_np, _), (buf, o) in zip(ints, outs_i):
            assert np.array_equal(o.cpu().numpy().astype(np.float64), a_np[:, :s[0]].astype(np.float64).sum(0) + R.col_prefill(s[0])), (s, r)
            assert untouched(buf, s[0])
        for (s, r), a_np, o in zip(jobs, rnd_np, outs_r):
            a64 = a_np[:, :s[0]].astype(np.float64)
            within(o.cpu().numpy(), a64.sum(0), R.col_chain(r, s[2] == 0 and s[0] % 4 == 0 and s[1] % 4 == 0, True) * R.U * np.abs(a64).sum(0), f"{s} deferred")
        runs.append([o.cpu() for o in outs_r])
    for a, b, c in zip(*runs):
        assert torch.equal(a, b) and torch.equal(a, c), "three identical windows, different bytes"


def test_col_sum_window_with_a_full_queue(dev):
    """50 calls onto 50 outputs in one window: the queue holds 48 jobs, calls 49 and 50 add with atomics at once.  All 50 are right."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    rows, C = 64, 8
    a_np = [R.col_ints(rows, C, seed=100 + i) for i in range(50)]
    a = [col_operand(x, dev, torch.float32, 0) for x in a_np]
    out_buf, out = padded(50 * C, dev, fill=up(np.tile(R.col_prefill(C), 50), dev))
    L.bwd_defer_begin(None, 0)
    try:
        for i in range(50):
            L.col_sum(ptr(a[i]), C, C, ptr(out[i * C:(i + 1) * C]), rows, 0)
    finally:
        L.bwd_defer_flush()
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64).reshape(50, C)
    want = np.stack([x.astype(np.float64).sum(0) + R.col_prefill(C) for x in a_np])
    assert np.array_equal(got, want), f"calls {sorted(set(np.nonzero(got != want)[0] + 1))} are wrong"
    assert untouched(out_buf, 50 * C)


def test_col_sum_window_with_a_used_up_workspace(dev):
    """12 calls at C = 1536, rows = 8192 on one shared input: 512 blocks x 1536 partials = 3 MB each, the 32 MB workspace holds ten; calls 11 and 12
    take the atomic path.  All 12 are right."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    rows, C = 8192, 1536
    assert 10 * 512 * C <= (8 << 20) < 11 * 512 * C
    a_np = R.col_ints(rows, C)
    a = col_operand(a_np, dev, torch.float32, 0)
    out_buf, out = padded(12 * C, dev, fill=up(np.tile(R.col_prefill(C), 12), dev))
    L.bwd_defer_begin(None, 0)
    try:
        for i in range(12):
            L.col_sum(ptr(a), C, C, ptr(out[i * C:(i + 1) * C]), rows, 0)
    finally:
        L.bwd_defer_flush()
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64).reshape(12, C)
    want = a_np.astype(np.float64).sum(0) + R.col_prefill(C)
    assert np.array_equal(got, np.tile(want, (12, 1))), f"calls {sorted(set(np.nonzero(got != want)[0] + 1))} are wrong"
    assert untouched(out_buf, 12 * C)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the float64 folds
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_fold64_multi_is_one_rounding(dev):
    """dst[d + i] = float32(float64(dst[d + i]) + src[s + i]) for every table row, the rest of dst untouched, bit for bit"""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    r = np.random.RandomState(3)
    dst_np = r.standard_normal(R.FOLD_DST).astype(np.float32)
    src_np = r.standard_normal(R.FOLD_SRC) * np.where(np.arange(R.FOLD_SRC) % 2, 1e-3, 1.0)  # (half of them far below dst: the rounding is felt)
    want = dst_np.copy()
    for d, s, n in R.FOLD_TABLE:
        want[d:d + n] = (dst_np[d:d + n].astype(np.float64) + src_np[s:s + n]).astype(np.float32)
    assert (want != dst_np).sum() > 0.99 * sum(n for _, _, n in R.FOLD_TABLE)
    table = torch.tensor(R.FOLD_TABLE, dtype=torch.int32, device=dev)
    dst, src = up(dst_np, dev), up(src_np, dev)
    L.fold64_multi(ptr(table), len(R.FOLD_TABLE), ptr(dst), ptr(src))
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"first difference at {int(np.flatnonzero(got != want)[0])}"

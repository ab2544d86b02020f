"""Float64 references, float32 emulations and the cases of the tests of the small kernels between the heavy ones: the BatchNorm statistics
(k_bn_finalize, k_bn_finalize_parts), the BatchNorm backward coefficients (k_bn_bwd_finalize) as a chain with the window kernels of
csrc/rec_pool.hip, the average-pool stage, ocrs_col_sum alone and inside a deferral window, ocrs_fold64_multi.  Stated once for
tests/test_bnstat_host.py (CPU: proves what the GPU test rests on) and tests/test_bnstat_gpu.py.

CPU only: nothing here imports the GPU package.

Units.  One float32 rounding moves a value by at most 2^-24 of its magnitude, which is at most one `ulp32` of any value at least as large.  Every
bound below is a count of the roundings the kernel's written arithmetic performs, each in ulps of the term it acts on; a contracted multiply-add
only removes one of them.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.exact_ref import SIGN_MARGIN, pool, windows
from tests.lossopt_ref import ulp32

F32 = np.float32
EPS = float(F32(1e-5))   # the values the C ABI receives: floats
MOM = float(F32(0.1))
NUM_CU = 256             # kNumCU of csrc/common.h: the launchers size their grids by it
U = 2.0 ** -24


def bf16_round32(x):
    """float32 -> the float32 value of its bf16 rounding"""
    return torch.from_numpy(np.array(x, dtype=F32)).bfloat16().float().numpy()


def bf16_from64(x):
    """float64 -> nearest bf16 value (8 significant bits, ties to even), as float64; normal range only"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def ulp_bf16(x):
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, e - 8)


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64"""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def exact_sums(z):
    """[count][C] stored values -> gstat [2][C] float64: correctly rounded sums and sums of squares (math.fsum)"""
    z = np.asarray(z, dtype=F32).astype(np.float64)
    return np.array([[math.fsum(col) for col in z.T], [math.fsum(col * col) for col in z.T]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. ocrs_bn_finalize
# ---------------------------------------------------------------------------------------------------------------------------------------

FIN_C = (8, 72, 136)          # 64-thread blocks: one partial block, one full + 8, two full + 8
FIN_COUNTS = (1, 2, 3 * 9 * 13)
FIN_LO = 0.125
FIN_PREFILL = (0.25, 2.0, 7)  # run_mean, run_var, num_batches_tracked
CH_CONST, CH_NEG, CH_1E3, CH_ZERO_GAMMA, CH_1E2, CH_30 = 0, 1, 2, 3, 4, 5  # the channels with a property of their own


@functools.lru_cache(maxsize=None)
def neg_var_column(count):
    """`count` float32 values for which sumsq / count - mean^2 comes out NEGATIVE in float64: one value an ulp above count - 1 copies of a base
    near 1 (true variance 4e-17, the expression's rounding error 1e-16: either is 1e-11 of eps, so the clamp and a contracted fp64 fma decide
    nothing that float32 sees); the first base, searched upwards, with that outcome.  A CONSTANT channel never has it (its mean and mean square
    are exact quotients), and bf16-exact values cannot have it: their smallest non-zero variance, 2^-14 mean^2 / count, is 1e9 rounding errors
    large.  So the bf16 cases carry a second constant channel here."""
    for k in range(1000):
        col = np.full(count, F32(1.0 + 0.00037 * k), F32)
        col[0] = np.nextafter(col[0], F32(np.inf))
        c64 = col.astype(np.float64)
        mean = math.fsum(c64) / count
        if math.fsum(c64 * c64) / count - mean * mean < 0:
            col.setflags(write=False)
            return col
    raise AssertionError("no near-constant channel with a negative float64 variance")


@functools.lru_cache(maxsize=None)
def fin_case(C, count, bf16):
    """-> dict z [count][C] float32 (the stored values; bf16-exact if bf16), gamma, beta, gstat [2][C] float64.  Channel 0 is constant 0.5 (var
    exactly 0), channel 1 is neg_var_column (var < 0 before the clamp; fp32 and count = 351 only, otherwise constant), channels 2 / 4 / 5 have
    |mean| / std = 1e3 / 1e2 / 30, gamma[3] = 0, gamma has both signs."""
    r = np.random.RandomState(1000 * C + count + (7 if bf16 else 0))
    std = r.uniform(0.5, 2.0, C)
    ratio = r.uniform(-2.0, 2.0, C)
    ratio[CH_1E3], ratio[CH_1E2], ratio[CH_30] = 1e3, -1e2, 30.0
    z = (ratio * std + std * r.standard_normal((count, C))).astype(F32)
    z[:, CH_CONST] = 0.5
    z[:, CH_NEG] = 1.5
    if not bf16:
        z[:, CH_NEG] = neg_var_column(FIN_COUNTS[-1])[:count] if count == FIN_COUNTS[-1] else neg_var_column(FIN_COUNTS[-1])[-1]
    if bf16:
        z = bf16_round32(z)
    gamma = (r.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 1, -1.0, 1.0)).astype(F32)
    gamma[CH_ZERO_GAMMA] = 0.0
    beta = r.uniform(-0.5, 0.5, C).astype(F32)
    out = {"z": z, "gamma": gamma, "beta": beta, "gstat": exact_sums(z), "count": count, "C": C}
    for a in (z, gamma, beta, out["gstat"]):
        a.setflags(write=False)
    return out


def finalize_ref64(gstat, count, gamma, beta, run_mean=None, run_var=None):
    """k_bn_finalize in float64 from the sums it is given.  -> dict of float64 values and, next to each, its bound (absolute):

    saved = mean | rstd: each ONE rounding of a float64 expression; compared in ulps by the caller (1 ulp: a contracted fp64 fma may flip it).
    sc = tr[0] = gamma * rstd: rstd rounded, the product rounded: 2 roundings of sc             -> 2 ulp32(sc)
    sh = tr[1] = beta - float(mean) * sc: on the product P = mean * sc: mean rounded, the 2 of sc, the product rounded (not if hipcc contracts
         beta - mean * sc into an fma: one fewer), and the subtraction rounded; beta and P can cancel, so the last one is taken of |beta| + |P|,
         never of the difference                                                                  -> 4 ulp32(P) + ulp32(|beta| + |P|)
    run' = (1 - mom) * run + mom * float(x), x = mean | unbiased var: on a = (1 - mom) run: 1 - mom rounded, the product rounded; on b = mom x:
         x rounded, the product rounded; the sum rounded (an fma saves one product rounding)     -> 2 ulp32(a) + 2 ulp32(b) + ulp32(|a| + |b|)
    """
    C = gamma.size
    g, b = gamma.astype(np.float64), beta.astype(np.float64)
    mean = gstat[0] / count
    var_raw = gstat[1] / count - mean * mean
    var = np.maximum(var_raw, 0.0)
    rstd = 1.0 / np.sqrt(var + EPS)
    sc = g * rstd
    P = mean * sc
    out = {"mean": mean, "var_raw": var_raw, "var": var, "rstd": rstd, "sc": sc, "sh": b - P,
           "sc_bound": 2 * ulp32(sc), "sh_bound": 4 * ulp32(P) + ulp32(np.abs(b) + np.abs(P))}
    if run_mean is not None:
        unb = var * count / (count - 1) if count > 1 else var
        for name, old, x in (("run_mean", run_mean, mean), ("run_var", run_var, unb)):
            a_, b_ = (1.0 - MOM) * np.asarray(old, F32).astype(np.float64), MOM * x
            out[name] = a_ + b_
            out[name + "_bound"] = 2 * ulp32(a_) + 2 * ulp32(b_) + ulp32(np.abs(a_) + np.abs(b_))
        out["unb"] = unb
    assert out["sc"].shape == (C,)
    return out


def finalize_emul(gstat, count, gamma, beta, run_mean=None, run_var=None, fused=False):
    """k_bn_finalize as written: float64 up to the casts, float32 behind them.  fused: beta - mean * sc and the running-statistics sums as
    fused multiply-adds (what hipcc may contract).  -> tr0, tr1, saved_mean, saved_rstd (, run_mean, run_var), all float32"""
    mean = gstat[0] / count
    var = np.maximum(gstat[1] / count - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + EPS)).astype(F32)
    sc = gamma.astype(F32) * rstd
    m32 = mean.astype(F32)
    sh = fma32(-m32, sc, beta) if fused else beta.astype(F32) - m32 * sc
    res = [sc, sh, m32, rstd]
    if run_mean is not None:
        unb = var * count / (count - 1) if count > 1 else var
        omm, mom = F32(1) - F32(MOM), F32(MOM)
        for old, x in ((run_mean, mean), (run_var, unb)):
            old, x32 = np.asarray(old, F32), x.astype(F32)
            res.append(fma32(np.full_like(old, omm), old, mom * x32) if fused else omm * old + mom * x32)
    assert all(a.dtype == F32 for a in res)
    return res


# ocrs_bn_finalize_parts: integer-valued float32 partials [nparts][C][sum | sum of squares]; every total is an integer below 2^24, exact in any order
PARTS_CASES = [(nparts, C) for nparts in (1, 7, 300) for C in (8, 32)]


@functools.lru_cache(maxsize=None)
def parts_case(nparts, C):
    r = np.random.RandomState(77 * nparts + C)
    parts = np.stack([r.randint(-4, 5, (nparts, C)), r.randint(20, 41, (nparts, C))], axis=2).astype(F32)
    count = 8 * nparts
    gamma = (r.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 2, -1.0, 1.0)).astype(F32)
    beta = r.uniform(-0.5, 0.5, C).astype(F32)
    tot = parts.astype(np.float64).sum(0)  # [C][2]
    assert float(np.abs(parts).sum(0).max()) < 2 ** 24
    return {"parts": parts, "count": count, "gamma": gamma, "beta": beta, "gstat": np.ascontiguousarray(tot.T)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the BatchNorm backward as a chain: statistics -> window forward -> reductions -> coefficients -> dz
# ---------------------------------------------------------------------------------------------------------------------------------------

CHAIN_CASES = [(2, 8, 12, 64, 2, 2), (2, 9, 13, 8, 2, 2), (3, 9, 7, 128, 2, 1), (2, 5, 9, 128, 1, 1)]  # (N, H, W, C, PH, PW)
AVG_CHAIN = (3, 5, 26, 128)                                                                              # (N, H, W, C)
# Seeds are chosen, not drawn: in float64 no pre-activation within SIGN_MARGIN of zero, no window whose two largest activations are closer than
# that (tests/test_bnstat_host.py asserts zero such elements).  The first salt, searched upwards from 0, at which that holds.
CHAIN_SALT = {((3, 9, 7, 128, 2, 1), "bf16"): 1}
BF16_OFF_BY_ONE_SHARE = 0.01


def _nchw(a):
    return torch.from_numpy(np.array(a)).double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def chain_case(dims, dname, salt=None, avg=False):
    """-> dict z [N][H][W][C] float32 (stored values), gy (pooled resolution NHWC; avg: gseq [W][N][C] float32), gamma, beta.  Per channel
    mean / std in [-2, 2] and std in [0.5, 2]; channel 5 has mean / std = 30: there B z + C cancels."""
    if avg:
        N, H, W, C = dims
        PH = PW = 1
    else:
        N, H, W, C, PH, PW = dims
    salt = CHAIN_SALT.get((dims, dname), 0) if salt is None else salt
    r = np.random.RandomState((sum(d * 31 ** i for i, d in enumerate(dims)) + (5 if dname == "bf16" else 0) + 1009 * salt) % (2 ** 31))
    std = r.uniform(0.5, 2.0, C)
    ratio = r.uniform(-2.0, 2.0, C)
    ratio[CH_30] = 30.0
    z = (ratio * std + std * r.standard_normal((N, H, W, C))).astype(F32)
    gamma = (r.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 3 == 1, -1.0, 1.0)).astype(F32)
    beta = r.uniform(-0.5, 0.5, C).astype(F32)
    gy = r.standard_normal((W, N, C) if avg else (N, H // PH, W // PW, C)).astype(F32)
    if dname == "bf16":
        z = bf16_round32(z)
        if not avg:
            gy = bf16_round32(gy)
    out = {"dims": dims, "dname": dname, "z": z, "gy": gy, "gamma": gamma, "beta": beta, "avg": avg, "count": N * H * W,
           "gstat": exact_sums(z.reshape(-1, C))}
    for a in (z, gy, gamma, beta, out["gstat"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def chain_reference(dims, dname, salt=None, avg=False):
    """float64 autograd of BatchNorm(train) -> ReLU -> max_pool2d((PH, PW)) (avg: BatchNorm(train) -> avg_pool2d((4, 1)) -> permute) on the stored
    z and gy.  -> dict (NHWC float64): out, dz, dgamma, dbeta, ghat (the gradient at the BatchNorm output), zhat, the terms A, B, Cc of
    dz = A ghat + B z + Cc, unit = 2^-24 (|A ghat| + |B z| + |Cc|) per element, close = the number of sign / maximum decisions inside SIGN_MARGIN"""
    case = chain_case(dims, dname, salt, avg)
    C = case["gamma"].size
    z = _nchw(case["z"]).requires_grad_(True)
    gamma = torch.from_numpy(case["gamma"].copy()).double().requires_grad_(True)
    beta = torch.from_numpy(case["beta"].copy()).double().requires_grad_(True)
    a = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    if avg:
        out = F.avg_pool2d(a, (4, 1))[:, :, 0, :].permute(2, 0, 1)  # [W][N][C]
        gout = torch.from_numpy(case["gy"].copy()).double()
        close = 0
    else:
        PH, PW = dims[4], dims[5]
        y = torch.relu(a)
        out = pool(y, PH, PW)  # the gradient goes to the FIRST maximum, stated explicitly
        assert torch.equal(out.detach(), F.max_pool2d(y.detach(), (PH, PW)))
        gout = _nchw(case["gy"])
        close = int((a.detach().abs() < SIGN_MARGIN).sum())
        if PH * PW > 1:
            # two EQUAL largest activations are no near-tie: they come from equal stored z (bf16 storage has many), every arithmetic maps them
            # to equal values and both sides take the first
            top = windows(y.detach(), PH, PW).sort(-1, descending=True).values
            close += int(((top[..., 0] > 0) & (top[..., 0] != top[..., 1]) & (top[..., 0] - top[..., 1] < SIGN_MARGIN)).sum())
    dz, ghat, dgamma, dbeta = torch.autograd.grad(out, [z, a, gamma, beta], grad_outputs=gout)
    zd = z.detach()
    cnt = case["count"]
    mean = zd.mean((0, 2, 3))
    var =((zd - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    rstd = 1.0 / torch.sqrt(var + EPS)
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    zhat = (zd - v(mean)) * v(rstd)
    m1, m2 = ghat.sum((0, 2, 3)) / cnt, (ghat * zhat).sum((0, 2, 3)) / cnt
    A = gamma.detach() * rstd
    B = -A * rstd * m2
    Cc = A * (-m1 + mean * rstd * m2)
    dz_formula = v(A) * ghat + v(B) * zd + v(Cc)
    assert float((dz_formula - dz).abs().max()) <= 1e-12 * float(dz.abs().max()), "the formulas the kernels implement ARE autograd's dz"
    unit = U * ((v(A) * ghat).abs() + (v(B) * zd).abs() + v(Cc).abs())
    res = {"out": out.detach().numpy() if avg else _nhwc(out), "dz": _nhwc(dz), "dgamma": dgamma.numpy(), "dbeta": dbeta.numpy(),
           "ghat": _nhwc(ghat), "zhat": _nhwc(zhat), "unit": _nhwc(unit), "A": A.numpy(), "B": B.numpy(), "Cc": Cc.numpy(),
           "mean": mean.numpy(), "rstd": rstd.numpy(), "close": close}
    for a_ in res.values():
        if isinstance(a_, np.ndarray):
            a_.setflags(write=False)
    return res


def ew_grid(items):
    g = (items + 255) // 256
    return max(1, min(g, NUM_CU * 8))


def reduce_plan(case):
    """How ocrs_rec_bn_reduce / ocrs_avgpool_bn_reduce spread the pooled pixels (avg: the columns): a thread keeps one channel group, a block of
    256 threads holds 256 / (C / 8) consecutive pixels per group, the grid is ew_grid capped at 4 per CU.  -> (pixels per block, pixels per
    thread, chain): chain = the longest float32 add chain of one channel's sum before the fp64 atomics (per-thread adds + the block's)."""
    dims = case["dims"]
    C = case["gamma"].size
    CG = C // 8
    pix = dims[0] * dims[2] if case["avg"] else dims[0] * (dims[1] // dims[4]) * (dims[2] // dims[5])
    grid = min(ew_grid(pix * CG), 4 * NUM_CU)
    per_block = 256 // CG
    per_thread = -(-pix // (grid * per_block))
    return per_block, per_thread, per_thread + per_block


def block_sums(terms, per_block):
    """[pixels][C] float32 per-thread values -> float64 [C]: float32 sums of `per_block` consecutive pixels in order, starting from 0 (the fixed
    order of group_sums_to_gsum), then float64 across the blocks (the fp64 atomics: exact, any order)"""
    P, C = terms.shape
    nb = -(-P // per_block)
    t = np.zeros((nb * per_block, C), F32)
    t[:P] = terms
    t = t.reshape(nb, per_block, C)
    acc = np.zeros((nb, C), F32)
    for i in range(per_block):
        acc = acc + t[:, i]
    assert acc.dtype == F32
    return acc.astype(np.float64).sum(0)


def bwd_finalize_emul(gsum, count, gamma, saved_mean, saved_rstd):
    """k_bn_bwd_finalize (and bn_fin_coef): float64 from the float32 saved statistics, one rounding per output.  -> coef [3][C], dgamma, dbeta"""
    s1, s2 = gsum
    m1, m2 = s1 / count, s2 / count
    mean, rstd = saved_mean.astype(np.float64), saved_rstd.astype(np.float64)
    A = gamma.astype(np.float64) * rstd
    coef = np.stack([A, -A * rstd * m2, A * (-m1 + mean * rstd * m2)]).astype(F32)
    return coef, s2.astype(F32), s1.astype(F32)


def chain_emul(dims, dname, salt=None, avg=False):
    """The kernels' stated arithmetic on the CPU in float32: coefficients rounded to float32, the fmaf nests of k_act_pool_fwd / k_rec_bn_reduce /
    k_dz_apply (k_avgpool_*), float32 per-thread and per-block sums folded in float64.  reduce_plan's one-pixel-per-thread layout is asserted.
    -> dict out, gsum [2][C] float64, coef, dgamma, dbeta, dz (float32; bf16 case: the float32 value of the stored bf16)"""
    case = chain_case(dims, dname, salt, avg)
    z, gy, gamma, beta, C = case["z"], case["gy"], case["gamma"], case["beta"], case["gamma"].size
    sc, sh, mu, rs = finalize_emul(case["gstat"], case["count"], gamma, beta)
    per_block, per_thread, _ = reduce_plan(case)
    assert per_thread == 1, "block_sums states the order for one pixel per thread"
    store = bf16_round32 if dname == "bf16" else (lambda t: t)
    if avg:
        N, H, W, _ = dims
        s = ((z[:, 0] + z[:, 1]) + z[:, 2]) + z[:, 3]                       # [N][W][C], the kernel's sequential float32 sum
        out = fma32(s * F32(0.25), sc, sh).transpose(1, 0, 2)                # [W][N][C]
        g = gy.transpose(1, 0, 2)                                            # [N][W][C]
        zs = np.zeros_like(s)
        for h in range(4):
            zs = zs + (z[:, h] - mu) * rs
        t1, t2 = g.reshape(-1, C), fma32(g * F32(0.25), zs, np.zeros_like(zs)).reshape(-1, C)
        gh = np.zeros_like(z)
        gh[:, :4] = (g * F32(0.25))[:, None]
    else:
        N, H, W, _, PH, PW = dims
        Hp, Wp = H // PH, W // PW
        zw = z[:, :Hp * PH, :Wp * PW].reshape(N, Hp, PH, Wp, PW, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp, Wp, PH * PW, C)
        y = np.maximum(fma32(zw, sc, sh), F32(0))
        k = y.argmax(3)                                                       # the FIRST maximum
        best = np.take_along_axis(y, k[:, :, :, None], 3)[:, :, :, 0]
        bz = np.take_along_axis(zw, k[:, :, :, None], 3)[:, :, :, 0]
        out = store(best)
        ghp = np.where(best > 0, gy, F32(0))
        t1, t2 = ghp.reshape(-1, C), fma32(ghp, (bz - mu) * rs, np.zeros_like(ghp)).reshape(-1, C)
        ghw = np.where(np.arange(PH * PW)[None, None, None, :, None] == k[:, :, :, None], ghp[:, :, :, None], F32(0))
        gh = np.zeros_like(z)
        gh[:, :Hp * PH, :Wp * PW] = ghw.reshape(N, Hp, Wp, PH, PW, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, Hp * PH, Wp * PW, C)
    gsum = np.stack([block_sums(t1, per_block), block_sums(t2, per_block)])
    coef, dgamma, dbeta = bwd_finalize_emul(gsum, case["count"], gamma, mu, rs)
    dz = store(fma32(coef[0], gh, fma32(coef[1], z, coef[2])))
    assert dz.dtype == F32 and out.dtype == F32
    return {"out": out, "tr": (sc, sh), "saved": (mu, rs), "gsum": gsum, "coef": coef, "dgamma": dgamma, "dbeta": dbeta, "dz": dz}


def dz_units(dz, ref):
    """the largest |dz - float64| per element in the element's own unit 2^-24 (|A ghat| + |B z| + |C|)"""
    return float((np.abs(np.asarray(dz, np.float64) - ref["dz"]) / ref["unit"]).max())


def bf16_offsets(dz, ref):
    """stored bf16 dz against the float64 dz rounded to bf16 -> (largest distance in bf16 ulps of the reference, share of unequal elements)"""
    want = bf16_from64(ref["dz"])
    d = np.abs(np.asarray(dz, np.float64) - want) / ulp_bf16(want)
    return float(d.max()), float((d != 0).mean())


def gsum_bounds(case, ref):
    """Absolute bounds on the kernel's gsum = [sum ghat | sum ghat zhat] against float64 (dgamma / dbeta are one float32 rounding of them: the caller
    adds one ulp).  ghat is exact (stored values).  L = reduce_plan's chain: every add of the chain rounds a partial sum no larger than sum |t|.
    sum ghat:       L 2^-24 sum |ghat|
    sum ghat zhat:  per term t = ghat (z - mu) rs: mu is the ROUNDED mean (moves zhat by 2^-24 |mean| rstd: 30 units in the mean / std = 30 channel),
                    z - mu rounded, rs rounded and up to one ulp off (2), the product rounded: 4 roundings of |t|; then the chain.
                    2^-24 (sum |ghat| (|mean| rstd + 4 |zhat|) + L sum |ghat zhat|)"""
    _, _, L = reduce_plan(case)
    gh, zh = np.abs(ref["ghat"]), np.abs(ref["zhat"])
    ax = (0, 1, 2)
    e1 = L * U * gh.sum(ax)
    e2 = U * ((gh * (np.abs(ref["mean"]) * ref["rstd"] + 4 * zh)).sum(ax) + L * (gh * zh).sum(ax))
    return e1, e2


def identities(case, ref, dz, bound):
    """The two sums the coefficient formulas exist for, per channel, of a dz given as NHWC: sum dz = 0 and sum dz zhat = -B count eps rstd
    (= A m2 count eps rstd^2: zero but for eps, since sum zhat^2 = count var / (var + eps)).  -> the two distances from those values, each divided
    by the per-element `bound` summed over the channel (the second weighted with |zhat|), plus the float64 reference's own residual"""
    ax = (0, 1, 2)
    d = np.asarray(dz, np.float64)
    want1 = -ref["B"] * case["count"] * EPS * ref["rstd"]
    r0 = np.abs(ref["dz"].sum(ax))
    r1 = np.abs((ref["dz"] * ref["zhat"]).sum(ax) - want1)
    e0 = np.abs(d.sum(ax)) / (bound.sum(ax) + r0)
    e1 = np.abs((d * ref["zhat"]).sum(ax) - want1) / ((bound * np.abs(ref["zhat"])).sum(ax) + r1)
    return float(e0.max()), float(e1.max()), float(r0.max()), float((r1 / np.maximum(np.abs(want1), 1e-300)).max())


def act_out_bound(case):
    """pooled y = max over the window of max(fmaf(z, sc, sh), 0): per element sc's two roundings on |z sc|, sh within its own bound, one rounding of
    the result; a maximum moves by no more than its largest member does"""
    N, H, W, C, PH, PW = case["dims"]
    fin = finalize_ref64(case["gstat"], case["count"], case["gamma"], case["beta"])
    zs = np.abs(case["z"].astype(np.float64) * fin["sc"])
    b = 2 * U * zs + fin["sh_bound"] + ulp32(zs + np.abs(fin["sh"]))
    return _nhwc(windows(torch.from_numpy(b).permute(0, 3, 1, 2), PH, PW).max(-1).values)


def avg_out_bound(case, ref):
    """seq = fmaf(s / 4, sc, sh): s a float32 sum of four (3 roundings of at most sum |z|), / 4 exact, sc two roundings, sh within its own bound,
    the fmaf one rounding of the result"""
    fin = finalize_ref64(case["gstat"], case["count"], case["gamma"], case["beta"])
    za = np.abs(case["z"][:, :4].astype(np.float64)).sum(1).transpose(1, 0, 2) * 0.25  # [W][N][C]
    zm = np.abs(case["z"][:, :4].astype(np.float64).sum(1)).transpose(1, 0, 2) * 0.25
    return U * (3 * za + 2 * zm) * np.abs(fin["sc"]) + fin["sh_bound"] + ulp32(zm * np.abs(fin["sc"]) + np.abs(fin["sh"]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. ocrs_col_sum
# ---------------------------------------------------------------------------------------------------------------------------------------

COL_ROWS = (1, 3, 16, 17, 4099, 14337, 16389, 40000)
COL4_SHAPES = ((8, 8), (128, 132), (1536, 1536))       # (C, ld) of k_col_sum4 (C % 4 == 0, ld % 4 == 0, 16-byte aligned rows)
COL1_SHAPES = ((97, 128, 0), (100, 101, 0), (128, 128, 1))  # (C, ld, pointer offset in elements) of the fallback k_col_sum: C % 4, ld % 4, the alignment
COL_WIDE_MAX_ROWS = 4099


def col4_plan(rows):
    """k_col_sum4's launch for `rows`: grid g4 = min(ceil(rows / 16), 2 per CU), a thread starts at row r0 = 4 block + phase < rstep = 4 g4 and walks
    its rows in three loops.  -> (g4, {loops that some thread enters}, the most loop iterations of one thread)

    At 256 CUs g4 = 512 and rstep = 2048 from rows = 8177 on:
      14337: the 8-row loop needs r0 + 7 * 2048 < 14337: r0 = 0 only; every other thread runs the 4-row loop once and the tail up to three times
      16389: every thread runs the 8-row loop once (r0 + 14336 < 16389); r0 < 5 then have ONE row left, r0 + 16384: the 1-row tail, no 4-row loop
      40000: the 8-row loop twice (to r0 + 32768); r0 < 1088 the 4-row loop (r0 + 32768 + 6144 < 40000), the others three tail rows
    and at 4099 (g4 = 257, rstep = 1028) the 4-row loop for r0 < 1015 and three tail rows for the rest."""
    g4 = max(1, min(-(-rows // 16), 2 * NUM_CU))
    rstep = 4 * g4
    used, most = set(), 0
    for r0 in range(rstep):
        r, it = r0, 0
        while r + 7 * rstep < rows:
            r += 8 * rstep
            used.add(8)
            it += 1
        while r + 3 * rstep < rows:
            r += 4 * rstep
            used.add(4)
            it += 1
        while r < rows:
            r += rstep
            used.add(1)
            it += 1
        most = max(most, it)
    return g4, used, most


def col_chain(rows, vec4, deferred=False):
    """the longest float32 add chain between an element and out[c]: the tree of a loop step (3), the thread's running sum (one add per loop
    iteration), the block's phases (2; fallback: 1), then one atomic add per block onto out (deferred: k_reduce_multi's 8 chains of
    ceil(nb / 8) adds, two 3-deep trees and the += onto out)"""
    if vec4:
        nb, _, most = col4_plan(rows)
        inner = 3 + most + 2
    else:
        nb = max(1, min((rows + 1) // 2, 1024))
        inner = -(-rows // (2 * nb)) + 1
    return inner + (-(-nb // 8) + 3 + 3 + 1 if deferred else nb)


@functools.lru_cache(maxsize=None)
def col_ints(rows, ld, seed=0):
    """[rows][ld] integers in [-2, 2] (float32): every partial sum is an integer below 2^24"""
    a = np.random.RandomState(rows * 7 + ld + seed).randint(-2, 3, (rows, ld)).astype(F32)
    assert 2 * rows < 2 ** 24
    a.setflags(write=False)
    return a


def col_prefill(C):
    return (0.25 * (np.arange(C) % 5)).astype(F32)  # multiples of 0.25: adds exactly to an integer sum below 2^22


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. ocrs_fold64_multi
# ---------------------------------------------------------------------------------------------------------------------------------------

FOLD_TABLE = ((5, 3, 0), (9, 11, 1), (20, 30, 63), (100, 200, 64), (300, 400, 65), (500, 1000, 1000))  # (dst offset, src offset, n)
FOLD_DST, FOLD_SRC = 1600, 2100

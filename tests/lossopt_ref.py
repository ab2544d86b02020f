"""Float64 references, CPU emulations and the cases of the loss / optimiser kernel tests (csrc/loss_optim.hip and the fused k_head_bwd_loss of
csrc/det_head.hip), stated once for tests/test_lossopt_host.py (CPU: proves what the GPU test rests on) and tests/test_lossopt_gpu.py.

Balanced BCE.  The kernel's tie rule is deterministic (every tie at the k-th largest loss is weighted need / ties), so given the per-pixel loss
the kernel itself stored, the whole selection -- counts, k, threshold bits, need, ties, frac, 1/(2k) and the weight of every pixel -- has exactly
one right answer: `select_ref` computes it on the float32 bit patterns.  Only two things are compared with a tolerance, each counted in float32
ulps of a float64 value: the per-pixel loss (one logf per term) and the gradient (a chain of correctly rounded operations).

Adam / clip.  One step at a time in float64 from the kernel's own float32 state of the step before, so errors do not compound.
"""
import functools
import struct

import numpy as np

F32 = np.float32
GOUT = 2.5

# ---------------------------------------------------------------------------------------------------------------------------------------
# float32 ulps
# ---------------------------------------------------------------------------------------------------------------------------------------


def ulp32(x):
    """float32 spacing at the magnitude of the float64 value(s) x (2^-149 below the normal range)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)  # |x| = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


def ulps(got, want):
    """|got - want| in float32 ulps of `want` (float64)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / ulp32(want)


def logf(x):
    """float32 log as float32(log(float64(x))): within 0.5 + 2^-29 ulps of the true value (numpy's own float32 log is a SIMD routine several
    ulps off)."""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, dtype=F32).astype(np.float64)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the per-pixel loss
# ---------------------------------------------------------------------------------------------------------------------------------------


def classes(target):
    t = np.asarray(target, dtype=F32)
    return np.where(t > F32(0.5), 1, np.where(t < F32(0.5), 2, 0)).astype(np.uint8)


def lpx64(pred, target):
    """-> (l float64 [P], cls u8 [P]): class on the raw target, BCE on the clamped one, both logs clamped at -100."""
    p, t0 = np.asarray(pred, dtype=F32).astype(np.float64), np.asarray(target, dtype=F32).astype(np.float64)
    t = np.clip(t0, 0.0, 1.0)
    with np.errstate(divide="ignore"):
        a, b = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
    return -(t * a + (1.0 - t) * b), classes(target)


def lpx32_emul(pred, target):
    """k_bce_fwd's arithmetic, operation for operation, in numpy float32 (every numpy float32 operation is correctly rounded; no contraction:
    with 0 / 1 targets one product of t * A + (1 - t) * B is a signed zero and a fused multiply-add gives the same bits)."""
    p, t0 = np.asarray(pred, dtype=F32), np.asarray(target, dtype=F32)
    one = F32(1)
    t = np.minimum(np.maximum(t0, F32(0)), one)
    a = np.maximum(logf(p), F32(-100))
    u = one - p
    with np.errstate(divide="ignore", invalid="ignore"):
        l1p = np.where(u <= 0, F32(-np.inf), logf(np.where(u <= 0, one, u)) - ((u - one) + p) / np.where(u <= 0, one, u)).astype(F32)
    b = np.maximum(l1p, F32(-100))
    l = -(t * a + (one - t) * b)
    assert l.dtype == F32
    return l, classes(target)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------------------------


def keys_of(lpx_f32):
    l = np.ascontiguousarray(lpx_f32, dtype=F32)
    return l.view(np.uint32) & np.uint32(0x7FFFFFFF)


def select_ref(lpx_f32, cls):
    """The balanced top-k selection on float32 bit patterns (key = bits & 0x7fffffff; -0.0 has key 0).  -> dict with
    cnt (2), k, and for k > 0: prefix / need / ties (2 each), frac (float64 need / ties), sum_gt (2, float64), loss (float64),
    weight (float64 [P]: 1 above the class threshold, need / ties on it, 0 below it and for class 0).  k == 0: loss NaN, weight 0."""
    key = keys_of(lpx_f32)
    cls = np.asarray(cls)
    cnt = [int((cls == 1).sum()), int((cls == 2).sum())]
    k = min(cnt)
    out = {"cnt": cnt, "k": k, "weight": np.zeros(key.shape, np.float64)}
    if k == 0:
        out["loss"] = float("nan")
        return out
    out.update(prefix=[], need=[], ties=[], frac=[], sum_gt=[])
    tot = 0.0
    for c in (1, 2):
        sel = cls == c
        kc = key[sel]
        thr = int(np.partition(kc, kc.size - k)[kc.size - k])  # k-th largest
        gt, eq = kc > thr, kc == thr
        ties, need = int(eq.sum()), k - int(gt.sum())
        assert 1 <= need <= ties
        sum_gt = float(kc[gt].view(F32).astype(np.float64).sum())
        w = np.where(gt, 1.0, np.where(eq, need / ties, 0.0))
        out["weight"][sel] = w
        out["prefix"].append(thr)
        out["need"].append(need)
        out["ties"].append(ties)
        out["frac"].append(need / ties)
        out["sum_gt"].append(sum_gt)
        tot += sum_gt + need * float(np.uint32(thr).view(F32))
    out["loss"] = tot / (2.0 * k)
    return out


def radix_emul(lpx_f32, cls, k):
    """The kernel's 3-pass MSB radix select (11 / 10 / 10 bits), every histogram scanned from its top bin until the running count reaches
    `need`.  -> per class (prefix, need, ties, [bins used in pass 0, bins used inside the prefix in pass 1, distinct keys in the last bucket])."""
    key = keys_of(lpx_f32)
    res = []
    for c in (1, 2):
        kc = key[np.asarray(cls) == c]
        prefix, need, ties, used = 0, k, 0, []
        for shift, bits in ((20, 11), (10, 10), (0, 10)):
            inb = kc if shift == 20 else kc[(kc >> np.uint32(shift + bits)) == prefix]
            h = np.bincount(((inb >> np.uint32(shift)) & np.uint32((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
            used.append(int((h > 0).sum()))
            run = 0
            for b in range((1 << bits) - 1, -1, -1):
                if run + int(h[b]) >= need:
                    prefix, need, ties = (prefix << bits) | b, need - run, int(h[b])
                    break
                run += int(h[b])
            else:
                raise AssertionError("the histogram holds fewer than `need` elements")
        res.append((prefix, need, ties, used))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------------
# the gradient
# ---------------------------------------------------------------------------------------------------------------------------------------

# k_bce_bwd:  ((gout * inv2k) * wgt) * (p - t) / max((1 - p) * p, 1e-12), every operation correctly rounded.  GRAD_ULPS = 6 float32 ulps of the
# float64 value: one per operation of the chain -- gout * inv2k, * wgt, p - t, the two of (1 - p) * p, and the divide taken together with the last
# multiply.  A chain of n roundings errs by 0.5 * m_r * sum(1 / m_i) ulps of its result (m: the mantissas in [1, 2) of the result and of each
# rounded value), between n / 4 and n.  Counting every rounding, inv2k and frac themselves included, gives nine, but with targets of 0 or 1 the
# two of p - t and 1 - p never count: either both are exact (t = 0 and p >= 0.5, the selected negatives) or they are the same value, which
# cancels in the quotient (t = 1: (p - 1) / ((1 - p) p) = -1 / p); and off the ties wgt = 1 costs nothing.  That leaves five roundings for a
# pixel above the threshold and seven for a tie, and seven ulps only if all seven mantissas sit at 1 and the result's at 2.  The cases are
# fixed: tests/test_lossopt_host.py evaluates the same correctly rounded operations on every one of them and asserts GRAD_ULPS (largest: 3.09
# ulps, on big).
GRAD_ULPS = 6.0


def grad64(pred, target, weight, k, gout=GOUT):
    """gout / (2k) * weight * (p - t) / max(p (1 - p), 1e-12) in float64; zero when k == 0."""
    p = np.asarray(pred, dtype=F32).astype(np.float64)
    t = np.clip(np.asarray(target, dtype=F32).astype(np.float64), 0.0, 1.0)
    if k == 0:
        return np.zeros_like(p)
    return gout / (2.0 * k) * np.asarray(weight, np.float64) * (p - t) / np.maximum(p * (1.0 - p), 1e-12)


def grad32_emul(pred, target, lpx_f32, cls, sel, gout=GOUT):
    """k_bce_bwd in numpy float32 from the decoded-state values a correct forward leaves (`sel` = select_ref's result)."""
    p, t0 = np.asarray(pred, dtype=F32), np.asarray(target, dtype=F32)
    if sel["k"] == 0:
        return np.zeros_like(p)
    key, cls = keys_of(lpx_f32), np.asarray(cls)
    inv2k = F32(1.0 / (2.0 * sel["k"]))
    s = F32(gout) * inv2k
    wgt = np.zeros(p.shape, F32)
    for c in (1, 2):
        thr, frac = np.uint32(sel["prefix"][c - 1]), F32(sel["frac"][c - 1])
        wgt = np.where(cls == c, np.where(key > thr, F32(1), np.where(key == thr, frac, F32(0))), wgt).astype(F32)
    t = np.minimum(np.maximum(t0, F32(0)), F32(1))
    g = (s * wgt) * (p - t) / np.maximum((F32(1) - p) * p, F32(1e-12))
    assert g.dtype == F32
    return np.where(wgt == 0, F32(0), g)


# ---------------------------------------------------------------------------------------------------------------------------------------
# LossState (csrc/loss_state.h)
# ---------------------------------------------------------------------------------------------------------------------------------------

LOSS_STATE_FMT = "<2Q Q 2I 2Q 2Q 2d f 2f f".replace(" ", "")  # cnt | k | prefix | need | ties | sum_gt | loss | frac | inv2k
LOSS_STATE_BYTES = 96
LOSS_STATE_OFFSETS = {"cnt": 0, "k": 16, "prefix": 24, "need": 32, "ties": 48, "sum_gt": 64, "loss": 80, "frac": 84, "inv2k": 92}


def decode_loss_state(raw: bytes):
    assert len(raw) == LOSS_STATE_BYTES == struct.calcsize(LOSS_STATE_FMT)
    v = struct.unpack(LOSS_STATE_FMT, raw)
    # the two float32 fields that must match bit for bit are also returned as raw words
    return {"cnt": list(v[0:2]), "k": v[2], "prefix": list(v[3:5]), "need": list(v[5:7]), "ties": list(v[7:9]), "sum_gt": list(v[9:11]),
            "loss": v[11], "frac": list(v[12:14]), "inv2k": v[14], "loss_bits": struct.unpack_from("<I", raw, 80)[0]}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loss cases
# ---------------------------------------------------------------------------------------------------------------------------------------

LOSS_CASES = ("plateau", "saturated", "k0", "narrow", "zero", "k1", "wide", "big")  # GPU order: k0 directly follows the tie-heavy saturated
TIE_CASES = ("plateau", "saturated", "k1", "big")   # the tie rule must be visible in the gradient
HEAD_CASES = ("plateau", "saturated", "k1")          # fused head backward (first P - P % 4 pixels)
BIG_P = 4 * 1024 * 1024 + 259


def _shuffled(seed, pred, target):
    perm = np.random.RandomState(seed).permutation(pred.size)
    return pred[perm].astype(F32), target[perm].astype(F32)


def _to_tail(pred, target, where):
    """Swap the first pixel of the mask `where` with the last one: the < 4 tail pixels are visited by separate code in every kernel, and only a tail
    pixel that IS selected (weight > 0) makes a dropped tail visit of the select passes change the result."""
    i, j = int(np.flatnonzero(where)[0]), pred.size - 1
    pred[[i, j]], target[[i, j]] = pred[[j, i]], target[[j, i]]


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> (pred float32 [P], target float32 [P]), read-only.  Every recipe but wide and big (whose recipes are positional) is shuffled with a
    fixed permutation.  Where P % 4 != 0 a SELECTED pixel is put into the tail (saturated has two by its permutation; wide keeps the recipe of
    test_balanced_bce as it is)."""
    r = np.random.RandomState({"plateau": 11, "saturated": 12, "narrow": 13, "zero": 14, "k1": 15, "k0": 16, "wide": 17, "big": 18}[name])
    u = lambda lo, hi, n: r.uniform(lo, hi, n)  # noqa: E731
    if name == "plateau":
        pred = np.concatenate([np.full(120, 0.02), np.full(180, 0.35), np.full(100, 0.9), np.full(500, 0.75), u(0.01, 0.5, 1000)])
        target = np.concatenate([np.ones(300), np.zeros(1600)])
        pred, target = _shuffled(1, pred, target)
    elif name == "saturated":
        pred = np.concatenate([np.zeros(50), u(0.1, 0.9, 150), np.ones(400), u(0.1, 0.9, 1403)])
        target = np.concatenate([np.ones(200), np.zeros(1803)])
        target[60], target[700] = 1.2, -0.3
        pred, target = _shuffled(2, pred, target)
        target[::53] = 0.5
    elif name == "narrow":
        pred = np.concatenate([0.5 + np.arange(4096) * 2.0 ** -24, u(0.1, 0.9, 1000)])
        target = np.concatenate([np.zeros(4096), np.ones(1000)])
        pred, target = _shuffled(3, pred, target)
    elif name == "zero":
        pred = np.concatenate([np.ones(64), u(0.5, 1.0, 36), u(0.0, 0.5, 333)])
        target = np.concatenate([np.ones(100), np.zeros(333)])
        pred, target = _shuffled(4, pred, target)
        _to_tail(pred, target, (target == 1) & (pred < 1))       # a positive above the threshold (key 0)
    elif name == "k1":
        pred = np.concatenate([[0.3], np.full(3, 0.97), u(0.01, 0.9, 997)])
        target = np.concatenate([[1.0], np.zeros(1000)])
        pred, target = _shuffled(5, pred, target)
        _to_tail(pred, target, (target == 0) & (pred == F32(0.97)))  # one of the three ties
    elif name == "k0":
        pred, target = _shuffled(6, u(0.05, 0.95, 400), np.zeros(400))
    elif name == "wide":  # tests/test_det_ops_gpu.py::test_balanced_bce at (3, 1, 33, 47), ppos 0.1
        import torch

        g = torch.Generator().manual_seed(int(0.1 * 10) + 33)
        logits = 6 * torch.randn((3, 1, 33, 47), generator=g)
        logits.view(-1)[::97] = 40.0
        logits.view(-1)[5::89] = -40.0
        tgt = (torch.rand((3, 1, 33, 47), generator=g) < 0.1).float()
        tgt.view(-1)[::53] = 0.5
        tgt.view(-1)[7::61] = 1.2
        pred, target = torch.sigmoid(logits).view(-1).numpy().astype(F32), tgt.view(-1).numpy().astype(F32)
    elif name == "big":
        pred = (1.0 / (1.0 + np.exp(-6.0 * r.standard_normal(BIG_P)))).astype(F32)
        target = (r.uniform(0, 1, BIG_P) < 0.07).astype(F32)
        pred[::97] = 1.0
        pred[5::89] = 0.0
        pred[-2:], target[-2:] = (0.0, 1.0), (1.0, 0.0)            # the tail holds a selected pixel of either class (both at the clamp)
    else:
        raise KeyError(name)
    pred, target = np.ascontiguousarray(pred, dtype=F32), np.ascontiguousarray(target, dtype=F32)
    pred.setflags(write=False)
    target.setflags(write=False)
    return pred, target


@functools.lru_cache(maxsize=None)
def head_case(name):
    """The first P - P % 4 pixels of a loss case (ocrs_head_bwd_loss needs P % 4 == 0)."""
    pred, target = loss_case(name)
    n = pred.size - pred.size % 4
    return pred[:n], target[:n]


# ---------------------------------------------------------------------------------------------------------------------------------------
# Adam and clip_grad_norm_
# ---------------------------------------------------------------------------------------------------------------------------------------

OPT_CHUNK = 2048
# (name, shape, gradient kind): the sizes on and around one chunk, a 2-d tensor, an all-zero gradient, gradients of magnitude 1e4
OPT_TENSORS = (("n1", (1,), "randn"), ("n2047", (2047,), "randn"), ("n2048", (2048,), "randn"), ("n2049", (2049,), "randn"),
               ("n4096", (4096,), "randn"), ("n4097", (4097,), "randn"), ("n10241", (5 * 2048 + 1,), "randn"), ("m33x5", (33, 5), "randn"),
               ("zero_grad", (300,), "zero"), ("grad_1e4", (257,), "1e4"))
OPT_STEPS = (1, 2, 3, 1000)        # the far step: state["step"] = 999 in front of the call
OPT_GRAD_SCALE = (0.1, 10.0, 0.1, 1.0)  # per step, as test_adam_and_clip_match_torch alternates small and large gradients
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
MAX_NORM = 4.0

M_ULPS, V_ULPS, P_REL = 3.0, 4.0, 8.0 * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def opt_params():
    r = np.random.RandomState(21)
    out = tuple(r.standard_normal(s).astype(F32) for _, s, _ in OPT_TENSORS)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def opt_grads(step_index):
    r = np.random.RandomState(100 + step_index)
    out = []
    for _, s, kind in OPT_TENSORS:
        if kind == "zero":
            g = np.zeros(s, F32)
        elif kind == "1e4":
            g = (1e4 * r.choice([-1.0, 1.0], s) * r.uniform(0.5, 1.5, s)).astype(F32)
        else:
            g = (OPT_GRAD_SCALE[step_index] * r.standard_normal(s)).astype(F32)
            # the elements a chunk loop can lose or visit twice -- the last one and the first of every further chunk -- are never small
            edge = sorted({g.size - 1, *range(OPT_CHUNK, g.size, OPT_CHUNK)})
            g.reshape(-1)[edge] = F32(1.5 * OPT_GRAD_SCALE[step_index]) * np.where(np.arange(len(edge)) % 2, F32(-1), F32(1))
        g.setflags(write=False)
        out.append(g)
    return tuple(out)


def norm64(grads):
    return float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)))


# clip_grad_norm_: the norm within NORM_REL of float64 -- per 2048-element chunk a float32 chain of 8 fused multiply-adds per thread and a 256-way
# tree (about 16 roundings of 2^-24 on a sum of squares, halved by the square root: 5e-7), then double accumulation.
NORM_REL = 1e-6
# Gradient sets (indices into OPT_TENSORS).  In the whole table the 257 gradients of 1e4 ARE the norm: any other tensor could be left out
# unnoticed.  So every other tensor is also taken alone, and the table once without that one.
CLIP_SETS = {**{name: (i,) for i, (name, _, kind) in enumerate(OPT_TENSORS) if kind == "randn"},
             "no_1e4": tuple(i for i, (_, _, kind) in enumerate(OPT_TENSORS) if kind != "1e4"),
             "table": tuple(range(len(OPT_TENSORS)))}


def clip_max_norm_below(norm):
    """A max_norm below `norm` that float32 holds exactly: the power of two at most half of it."""
    return float(2.0 ** (np.floor(np.log2(norm)) - 1))


def adam_ref64(p, g, m, v, step, coef=1.0):
    """One Adam step in float64 from float32 p, g, m, v (the state the kernel left) on the gradient g * coef.  The moment updates use the
    betas as the C ABI receives them -- float32: 1 - float32(0.999) differs from 0.001 by 1.3e-5 relative, hundreds of ulps of v -- ; the bias
    corrections, lr and eps are the exact doubles (each enters the update once, linearly: half an ulp, counted in P_REL).
    -> dict m, v, p, update (float64), m_scale (the largest term of the lerp, see adam_bounds)."""
    b1, b2 = float(F32(BETAS[0])), float(F32(BETAS[1]))
    p, g, m, v = (np.asarray(a, dtype=F32).astype(np.float64) for a in (p, g, m, v))
    g = g * float(coef)
    m1 = m + (g - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * g * g
    step_size = LR / (1.0 - BETAS[0] ** step)
    bc2_sqrt = np.sqrt(1.0 - BETAS[1] ** step)
    upd = step_size * (m1 / (np.sqrt(v1) / bc2_sqrt + EPS))
    return {"m": m1, "v": v1, "p": p - upd, "update": upd, "m_scale": np.maximum(np.abs(m1), np.maximum(np.abs(m), (1.0 - b1) * np.abs(g)))}


def adam_bounds(ref):
    """Per-element absolute bounds on (m, v, p) against adam_ref64.

    v: V_ULPS = 4 float32 ulps of v (v * b2, (1 - b2) * g, * g, the sum: four roundings of positive terms, 2^-24 relative each).  A scaled gradient
    g * coef adds its own rounding twice, through the square; the same 4 is kept for it: the float32 emulation stays below 2.7 ulps in every variant.
    m: M_ULPS = 3 ulps (g - m, * (1 - b1), + m) of the LARGEST TERM of the lerp, max(|m'|, |m|, (1 - b1) |g|), not of m' itself: m + (g - m) (1 - b1)
    cancels whenever the gradient changes sign, and the three roundings are relative to the terms, not to the difference (the host test shows
    that ulps of m' alone do not hold for the float32 emulation).
    p: ulp(p) + 8 * 2^-24 * |update|: the rounding of the subtraction plus eight relative roundings inside the update."""
    m_b = M_ULPS * ulp32(ref["m_scale"])
    v_b = V_ULPS * ulp32(ref["v"])
    p_b = ulp32(ref["p"]) + P_REL * np.abs(ref["update"])
    return m_b, v_b, p_b


def adam32_emul(p, g, m, v, step, coef=None, fused=False):
    """k_multi_adam in numpy float32; k_multi_adam_dev computes the same values (its float32 step counter is exact up to 2^24 and its bias
    corrections are the same double powers, rounded to float32 once).  fused = the contraction hipcc applies by default (a * b + c as one fused
    multiply-add, emulated through float64: the product of two float32 is exact there)."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    b1, b2, eps, one = F32(BETAS[0]), F32(BETAS[1]), F32(EPS), F32(1)
    step_size = F32(LR / (1.0 - BETAS[0] ** step))
    bc2_sqrt = F32(np.sqrt(1.0 - BETAS[1] ** step))
    fma = (lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F32)) if fused else (lambda a, b, c: a * b + c)
    gi = g * (F32(coef) if coef is not None else one)
    mi = fma(gi - m, one - b1, m)
    vi = fma(v, b2, (one - b2) * gi * gi) if fused else v * b2 + (one - b2) * gi * gi
    denom = np.sqrt(vi) / bc2_sqrt + eps
    q = mi / denom
    pn = fma(q, -step_size, p) if fused else p - step_size * q
    assert mi.dtype == vi.dtype == pn.dtype == F32
    return pn, mi, vi


# ---------------------------------------------------------------------------------------------------------------------------------------
# shared, computed once
# ---------------------------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def loss_reference(name, head=False):
    """-> dict: pred, target, l64, cls, l32 (the float32 emulation), interior (0 < l64 < 100), E_lpx (largest distance of l32 from l64 over the
    interior, in float32 ulps of l64), sel (select_ref on l32).  Read-only; shared by every test that needs it."""
    pred, target = head_case(name) if head else loss_case(name)
    l64, cls = lpx64(pred, target)
    l32, cls32 = lpx32_emul(pred, target)
    assert np.array_equal(cls, cls32)
    interior = (l64 > 0) & (l64 < 100)
    e = float(ulps(l32[interior], l64[interior]).max())
    for a in (l64, cls, l32, interior):
        a.setflags(write=False)
    return {"pred": pred, "target": target, "l64": l64, "cls": cls, "l32": l32, "interior": interior, "E_lpx": e, "sel": select_ref(l32, cls)}

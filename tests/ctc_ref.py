"""Float64 references, float32 emulations, cases and bounds of the tests of csrc/rec_seq.hip: log-softmax forward / backward, the CTC alpha /
beta recursions with the 2^-30 fixed-point occupancy sums and the gradient (all three forms: k_ctc_alpha + k_ctc_beta_grad, k_ctc_ab +
k_ctc_grad, the fp16-lattice variant), the greedy arg-max and collapse.  Stated once for tests/test_ctc_host.py (CPU: proves what the GPU
test rests on) and tests/test_ctc_gpu.py.

CPU only: nothing here imports the GPU package.

Units.  u = 2^-24: one float32 rounding moves a value by at most u of its magnitude.

Why the CTC bounds are per sample and scale with the lattice.  alpha and beta are log-masses of magnitude up to several hundred (A_n, B_n: the
largest finite |alpha|, |beta| of the float64 lattice of sample n); the recursion rounds each of them once per time step at that magnitude
(the fused multiply-add that ends lse3, and the addition of the emission), so the error of a lattice value -- and of nll_n -- is a multiple of
u A_n that no choice of transcendental can avoid, and a fixed relative tolerance is either blind at nll = 3 or wrong at nll = 1200.

  nll_n       |nll - nll64| <= K_NLL * u * A_n * sqrt(T_n).  A count gives T_n: every step adds at most two roundings of u A_n to a state, and
              lse3 passes the errors of its arguments on with weights that sum to 1, so they add up at most linearly.  The square root is
              MEASURED, NOT DERIVED: against u A_n T_n the emulation's ratio falls from 0.27 (T_n <= 37) to 0.03 (T_n = 140) -- the roundings
              do not line up --, against u A_n sqrt(T_n) it stays between 0.33 and 0.67 over all cases, so that form is the one that is
              equally sharp at every length.  Samples with T_n = 0 have unit 0: nll is exactly 0 or +inf.
  grad[t,n,c] |g - g64| <= K_GRAD * scale_n * [ u * (occ64(t,c) * (A_n + B_n + |nll64|) + p64(t,c)) + 2^-30 * states(c) ]
              occ64 = the per-class occupancy sum_s gamma_t(s), p64 = exp(lp), states(c) = the lattice states of class c (each contributes one
              rounding to the 2^-30 grid), scale_n = gout / (N max(L_n, 1)).  The occupancy is exp(alpha + beta + nll - lp): its relative
              error is the absolute error of that exponent, which is what the first term states.  For an infeasible sample (nll = +inf) the
              kernels write exp(lp) * scale (the documented departure from ATen's NaN); occ64 = 0 there and the unit is scale * u * p.
  rows t >= T_n, and every row of a sample with T_n = 0: the unit is 0 -- exactly 0 is the only value inside it.

The constants: the largest ratio the float32 emulation reaches against the unit over every case and SEEDS_PER_CASE seeds of it, times two (the
hardware exp2 / log2 / expf may differ from numpy's by an ulp or two, contraction moves single roundings).  tests/test_ctc_host.py asserts that
the emulation stays within HALF of every bound, which reproduces that measurement; the measured ratios stand next to the constants.
"""
import functools
import math

import numpy as np
import torch

from tests.bnstat_ref import bf16_from64, fma32, ulp_bf16  # noqa: F401  (re-exported for the tests)

F32 = np.float32
U = 2.0 ** -24
NINF = -np.inf
FIX = 2.0 ** 30
L2E = F32(1.4426950408889634)
LN2 = F32(0.6931471805599453)

SEEDS_PER_CASE = 9  # the case's own seed and 8 further ones

# ---------------------------------------------------------------------------------------------------------------------------------------
# The constants (2 x the emulation's largest ratio; tests/test_ctc_host.py::test_emulation_stays_within_half_of_every_bound re-measures them)
# ---------------------------------------------------------------------------------------------------------------------------------------
K_NLL = 1.34        # emulation: 0.667 (mixed); peaked4 0.62, single_path 0.54, edges 0.43 .. 0.48, infeasible 0.41, wide 0.35, peaked 0.33
K_GRAD = 8.0        # emulation: 3.99 (mixed); peaked4 3.91, peaked 3.85, wide 3.57, single_path 3.08, infeasible 2.70, edges 1.79 .. 2.55
K_GRAD_H16 = 2840.0  # emulation with the fp16 storage: 1419.6 (edges_c2); single_path 1141, edges_n1 713, wide 654, edges_c5 589, infeasible 581,
#                      peaked 486, edges_len 327, mixed 319, peaked4 296.  The fp16 rounding of alpha - rowmax is 2^-11 of a distance of up to a
#                      few units, against u (A + B + |nll|): hundreds of units, and more where the lattice is small.  The nll of the fp16 variant
#                      is the fp32 recursion's own (same bits): K_NLL.


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------

def ext_labels(target):
    """labels -> the extended sequence blank, l0, blank, l1, ..., blank"""
    target = np.asarray(target, dtype=np.int64).reshape(-1)
    ext = np.zeros(2 * len(target) + 1, dtype=np.int64)
    ext[1::2] = target
    return ext


def skip_into(ext):
    """[S] bool: the transition s-2 -> s is allowed (s a label that differs from the label before it)"""
    ok = np.zeros(len(ext), dtype=bool)
    ok[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    return ok


def _right(a, k, fill=NINF):
    out = np.full_like(a, fill)
    if k < len(a):
        out[k:] = a[: len(a) - k]
    return out


def _left(a, k, fill=NINF):
    out = np.full_like(a, fill)
    if k < len(a):
        out[: len(a) - k] = a[k:]
    return out


def onehot_states(ext, C):
    m = np.zeros((len(ext), C))
    m[np.arange(len(ext)), ext] = 1.0
    return m


def log_softmax64(x):
    """float64 log-softmax over the last axis; -inf entries stay -inf"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def log_softmax_bwd64(lp, g):
    lp, g = np.asarray(lp, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return g - np.exp(lp) * g.sum(-1, keepdims=True)


def ctc_sample64(lp, target, Ti):
    """One sample in float64, vectorised over the states.  lp (T, C) -> dict nll, alpha (Ti, S), beta (Ti, S), occ (T, C) per-class
    occupancy, grad (T, C) UNSCALED gradient in the ATen convention exp(lp) - occ (rows t >= Ti are 0; an infeasible sample has occ = 0: the
    kernels' finite gradient), A, B the largest finite |alpha|, |beta|."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    ext = ext_labels(target)
    S = len(ext)
    occ = np.zeros((T, C))
    grad = np.zeros((T, C))
    alpha = np.full((Ti, S), NINF)
    beta = np.full((Ti, S), NINF)
    if Ti == 0:
        return dict(nll=0.0 if S == 1 else np.inf, alpha=alpha, beta=beta, occ=occ, grad=grad, A=0.0, B=0.0, ext=ext)
    em = lp[:Ti][:, ext]
    into = skip_into(ext)
    outof = _left(into, 2, False)
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha[0, :2] = em[0, :2]
        for t in range(1, Ti):
            a = alpha[t - 1]
            v = np.logaddexp(np.logaddexp(a, _right(a, 1)), np.where(into, _right(a, 2), NINF))
            alpha[t] = v + em[t]
        beta[Ti - 1, max(S - 2, 0):] = em[Ti - 1, max(S - 2, 0):]
        for t in range(Ti - 2, -1, -1):
            b = beta[t + 1]
            v = np.logaddexp(np.logaddexp(b, _left(b, 1)), np.where(outof, _left(b, 2), NINF))
            beta[t] = v + em[t]
        ll = np.logaddexp(alpha[Ti - 1, S - 1], alpha[Ti - 1, S - 2]) if S > 1 else alpha[Ti - 1, 0]
        nll = -float(ll)
        ab = alpha + beta
        live = np.isfinite(ab) & np.isfinite(nll)
        gamma = np.where(live, np.exp(np.where(live, ab - em + nll, 0.0)), 0.0)
    occ[:Ti] = gamma @ onehot_states(ext, C)
    grad[:Ti] = np.exp(lp[:Ti]) - occ[:Ti]
    fin = lambda z: float(np.abs(z[np.isfinite(z)]).max()) if np.isfinite(z).any() else 0.0
    return dict(nll=nll, alpha=alpha, beta=beta, occ=occ, grad=grad, A=fin(alpha), B=fin(beta), ext=ext)


def ctc_batch64(case, gout=1.0):
    """-> dict nll (N,), grad (T, N, C) with the 1/(N max(L,1)) scale, loss (the 'mean' reduction), nll_unit (N,), grad_unit (T, N, C): the
    units of the bounds in the module docstring (without K_NLL / K_GRAD), feasible (N,) bool"""
    lp, tg, il, tl = case["lp"], case["targets"], case["il"], case["tl"]
    T, N, C = lp.shape
    nll = np.zeros(N)
    grad = np.zeros((T, N, C))
    nll_unit = np.zeros(N)
    grad_unit = np.zeros((T, N, C))
    for n in range(N):
        L, Ti = int(tl[n]), int(il[n])
        r = ctc_sample64(lp[:, n].astype(np.float64), tg[n, :L], Ti)
        scale = gout / (N * max(L, 1))
        nll[n] = r["nll"]
        grad[:, n] = r["grad"] * scale
        nll_unit[n] = U * r["A"] * math.sqrt(Ti)
        states = np.bincount(r["ext"], minlength=C).astype(np.float64)
        mag = r["A"] + r["B"] + (abs(r["nll"]) if np.isfinite(r["nll"]) else 0.0)
        p = np.exp(lp[:Ti, n].astype(np.float64))
        grad_unit[:Ti, n] = abs(scale) * (U * (r["occ"][:Ti] * mag + p) + states[None, :] / FIX)
        if not np.isfinite(r["nll"]):
            grad_unit[:Ti, n] = abs(scale) * U * p
    loss = float(np.mean(nll / np.maximum(np.asarray(tl, dtype=np.float64), 1.0)))
    return dict(nll=nll, grad=grad, loss=loss, nll_unit=nll_unit, grad_unit=grad_unit, feasible=np.isfinite(nll))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. float32 emulation of the kernels' written arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------

def lse3_32(a, b, c):
    """lse3 of rec_seq.hip: exp2 / log2 with the kernel's association, the closing fused multiply-add"""
    m = np.maximum(np.maximum(a, b), c)
    dead = m == NINF
    ms = np.where(dead, F32(0), m)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.exp2((a - ms) * L2E) + np.exp2((b - ms) * L2E) + np.exp2((c - ms) * L2E)
        r = fma32(np.log2(np.where(dead, F32(1), s)), LN2, ms)
    return np.where(dead, F32(NINF), r).astype(F32)


def lse2_32(a, b):
    a, b = F32(a), F32(b)
    m = max(a, b)
    if m == NINF:
        return F32(NINF)
    d = F32(0) if a == b else -abs(F32(a - b))
    return F32(m + np.log1p(np.exp(F32(d), dtype=F32), dtype=F32))


MUTANTS = ("skip_repeat", "skip_blank", "last_only", "scale_noclamp", "row_Tn", "beta_last_only", "occ_shift")


def ctc_sample32(lp, target, Ti, N, gout=1.0, h16=False, mutant=None):
    """One sample as the kernels compute it, float32 throughout.  lp (T, C) float32 -> (nll float32, grad (T, C) float32 with the scale).
    h16: the alpha lattice goes through the fp16-relative-to-row-maximum storage on its way to the gradient.
    mutant: one of MUTANTS -- a wrong kernel, for the host test's proof that the bounds see it."""
    lp = np.asarray(lp, dtype=F32)
    T, C = lp.shape
    ext = ext_labels(target)
    S, L = len(ext), len(ext) // 2
    grad = np.zeros((T, C), dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = F32(gout) / (F32(N) * F32(L if mutant == "scale_noclamp" else max(L, 1)))
    if mutant == "row_Tn" and 0 <= Ti < T:
        grad[Ti] = np.exp(lp[Ti]) * scale
    if Ti <= 0:
        return F32(0.0 if L == 0 else np.inf), grad
    em = lp[:Ti][:, ext]
    into = skip_into(ext)
    if mutant == "skip_repeat":
        into[2:] = ext[2:] != 0
    if mutant == "skip_blank":
        into[2:] |= ext[2:] == 0
    outof = _left(into, 2, False)
    ninf = F32(NINF)
    alpha = np.full((Ti, S), ninf, dtype=F32)
    alpha[0, :2] = em[0, :2]
    for t in range(1, Ti):
        a = alpha[t - 1]
        alpha[t] = lse3_32(a, _right(a, 1, ninf), np.where(into, _right(a, 2, ninf), ninf)) + em[t]
    nll = F32(-lse2_32(alpha[Ti - 1, S - 1], alpha[Ti - 1, S - 2] if (S > 1 and mutant != "last_only") else ninf))
    beta = np.full((Ti, S), ninf, dtype=F32)
    first = S - 1 if mutant == "beta_last_only" else max(S - 2, 0)
    beta[Ti - 1, first:] = em[Ti - 1, first:]
    for t in range(Ti - 2, -1, -1):
        b = beta[t + 1]
        beta[t] = lse3_32(b, _left(b, 1, ninf), np.where(outof, _left(b, 2, ninf), ninf)) + em[t]
    if h16:  # store_row of k_ctc_alpha<true>, read back as k_ctc_beta_grad<true> does
        rm = alpha.max(1, keepdims=True)
        with np.errstate(invalid="ignore"):
            d = np.where((alpha == ninf) | (rm == ninf), F32(-65504), np.maximum(alpha - rm, F32(-65504))).astype(np.float16).astype(F32)
            alpha_r = np.where(d <= F32(-65504), ninf, d + rm).astype(F32)
    else:
        alpha_r = alpha
    with np.errstate(invalid="ignore", over="ignore"):
        ab = alpha_r + beta
        live = ab != ninf
        g = np.minimum(np.exp(np.where(live, (ab + nll) - em, ninf).astype(F32)), F32(2))
        fixed = np.where(live, np.floor((g * F32(FIX) + F32(0.5)).astype(F32)), 0).astype(np.int64)
    cls = ext.copy()
    if mutant == "occ_shift":
        cls[:-1] = ext[1:]
    hot = np.zeros((S, C), dtype=np.int64)
    hot[np.arange(S), cls] = 1
    occ = (fixed @ hot).astype(F32) * F32(1.0 / FIX)
    with np.errstate(invalid="ignore", over="ignore"):
        grad[:Ti] = (np.exp(lp[:Ti]) - occ) * scale
    return nll, grad


def ctc_batch32(case, gout=1.0, h16=False, mutant=None):
    lp, tg, il, tl = case["lp"], case["targets"], case["il"], case["tl"]
    T, N, C = lp.shape
    nll = np.zeros(N, dtype=F32)
    grad = np.zeros((T, N, C), dtype=F32)
    for n in range(N):
        nll[n], grad[:, n] = ctc_sample32(lp[:, n], tg[n, : int(tl[n])], int(il[n]), N, gout, h16, mutant)
    return nll, grad


def ctc_ratios(nll, grad, ref):
    """the largest |error| / unit per sample: (nll ratios (N,), gradient ratios (N,)).  Nothing is left out: an element whose unit is 0 must be
    equal to the reference (ratio 0), anything else -- NaN included -- is inf; +inf nll must be +inf."""
    nll = np.asarray(nll, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)

    def ratio(err, unit):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(unit > 0, err / unit, np.where(err == 0, 0.0, np.inf))
        return np.where(np.isnan(r), np.inf, r)

    with np.errstate(invalid="ignore"):
        e = np.where(np.isinf(ref["nll"]), np.where(nll == ref["nll"], 0.0, np.inf), np.abs(nll - ref["nll"]))
    rn = ratio(e, np.where(np.isinf(ref["nll"]), 0.0, ref["nll_unit"]))
    rg = ratio(np.abs(grad - ref["grad"]), ref["grad_unit"]).max(axis=(0, 2))
    return rn, rg


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. cases
# ---------------------------------------------------------------------------------------------------------------------------------------

def _lp32(logits):
    """float32 log-probs of float64 logits: THE input of the CTC kernels and (widened) of the reference"""
    return log_softmax64(logits).astype(F32)


def make_case(name, seed, logits, tg, il, tl, **kw):
    c = dict(name=name, seed=seed, lp=_lp32(logits), targets=np.asarray(tg, dtype=np.int32), il=np.asarray(il, dtype=np.int64),
             tl=np.asarray(tl, dtype=np.int64), **kw)
    for k in ("lp", "targets", "il", "tl"):
        c[k].setflags(write=False)
    return c


def _mixed(seed):
    """the batch of test_rec_gpu.py::test_log_softmax_and_ctc_match_torch (its seed is 4)"""
    g = torch.Generator().manual_seed(seed)
    T, N, C, Lpad = 37, 9, 97, 64
    logits = 3 * torch.randn(T, N, C, generator=g)
    tl = [0, 1, 5, 12, 18, 3, 7, 9, 2]
    il = [37, 5, 20, 37, 37, 10, 30, 25, 4]
    tg = torch.zeros(N, Lpad, dtype=torch.int32)
    for i in range(N):
        tg[i, : tl[i]] = torch.randint(1, C, (tl[i],), generator=g)
    tg[3, 1] = tg[3, 0]
    tg[4, 2:6] = tg[4, 2]
    return make_case("mixed", seed, logits.double().numpy(), tg.numpy(), il, tl)


def labels_no_repeat(r, L, C):
    out = []
    for _ in range(L):
        c = int(r.randint(1, C))
        while out and c == out[-1] and C > 2:
            c = int(r.randint(1, C))
        out.append(c)
    return out


def _peaked(seed, bonus, name):
    r = np.random.RandomState(seed)
    T, N, C, Lmax = 101, 8, 97, 40
    tl = r.randint(1, Lmax + 1, N)
    tl[0], tl[1] = Lmax, 1
    il = np.array([r.randint(2 * L + 1, T + 1) for L in tl])
    il[0], il[2] = T, 2 * tl[2] + 1
    logits = r.randn(T, N, C)
    tg = np.zeros((N, Lmax), dtype=np.int32)
    for n in range(N):
        L, Ti = int(tl[n]), int(il[n])
        tg[n, :L] = r.randint(1, C, L)
        path = np.zeros(Ti, dtype=np.int64)  # one alignment: label k alone on an even frame, blanks everywhere else
        path[2 * np.sort(r.choice(Ti // 2, L, replace=False))] = tg[n, :L]
        logits[np.arange(Ti), n, path] += bonus
    return make_case(name, seed, logits, tg, il, tl)


def _single_path(seed):
    r = np.random.RandomState(seed)
    T, N, C = 12, 4, 30
    logits = 3 * r.randn(T, N, C)
    tg = np.zeros((N, T), dtype=np.int32)
    tg[0, :12] = labels_no_repeat(r, 12, C)
    tg[1, :7] = labels_no_repeat(r, 7, C)
    row = labels_no_repeat(r, 5, C)
    tg[2, :6] = row[:2] + [row[1]] + row[2:]  # a b b c d e in 7 frames: the one spare frame is the blank between the two b
    return make_case("single_path", seed, logits, tg, [12, 7, 7, 12], [12, 7, 6, 0])


def _edges_len(seed):
    r = np.random.RandomState(seed)
    T, N, C = 3, 4, 5
    tg = r.randint(1, C, (N, 2))
    return make_case("edges_len", seed, 3 * r.randn(T, N, C), tg, [1, 1, 0, 0], [0, 1, 0, 1])


def _edges_n1(seed):
    r = np.random.RandomState(seed)
    return make_case("edges_n1", seed, 3 * r.randn(6, 1, 5), r.randint(1, 5, (1, 3)), [6], [2])


def _edges_c2(seed):
    r = np.random.RandomState(seed)
    return make_case("edges_c2", seed, 3 * r.randn(7, 3, 2), np.ones((3, 3)), [7, 4, 5], [0, 2, 3])  # one class: every neighbour repeats


def _edges_c5(seed):
    r = np.random.RandomState(seed)
    tg = r.randint(1, 5, (3, 4))
    tg[1, 1] = tg[1, 0]
    return make_case("edges_c5", seed, 3 * r.randn(9, 3, 5), tg, [9, 6, 1], [4, 2, 1])


def _infeasible(seed, feasible=False):
    """sample 1: labels 3, 3, 5 need four frames and have three (`feasible`: the same batch with four)"""
    r = np.random.RandomState(seed)
    tg = r.randint(1, 8, (3, 3))
    tg[1] = [3, 3, 5]
    return make_case("infeasible", seed, 3 * r.randn(6, 3, 8), tg, [6, 4 if feasible else 3, 5], [2, 3, 1])


def _wide(seed):
    r = np.random.RandomState(seed)
    T, N, C = 140, 2, 23
    tg = np.zeros((N, 130), dtype=np.int32)
    tg[0] = labels_no_repeat(r, 130, C)
    tg[0, 127] = tg[0, 126]  # a repeated pair on the far side of the thread 255 / 256 seam (states 253 .. 257)
    tg[0, 40] = tg[0, 39]
    tg[1, :60] = labels_no_repeat(r, 60, C)
    return make_case("wide", seed, 1.5 * r.randn(T, N, C), tg, [140, 125], [130, 60])


_BUILD = {
    "mixed": (_mixed, 4),
    "peaked": (lambda s: _peaked(s, 8.0, "peaked"), 21),
    "peaked4": (lambda s: _peaked(s, 4.0, "peaked4"), 22),
    "single_path": (_single_path, 23),
    "edges_len": (_edges_len, 24),
    "edges_n1": (_edges_n1, 25),
    "edges_c2": (_edges_c2, 26),
    "edges_c5": (_edges_c5, 27),
    "infeasible": (_infeasible, 28),
    "wide": (_wide, 29),
}
CASES = tuple(_BUILD)
INFEASIBLE = {"edges_len": (3,), "infeasible": (1,)}  # the samples whose nll is +inf; every other sample of every case is feasible


@functools.lru_cache(maxsize=None)
def case(name, k=0):
    """case `name`, its k-th seed (0: the case's own)"""
    fn, seed = _BUILD[name]
    return fn(seed + 1000 * k)


@functools.lru_cache(maxsize=None)
def case_ref(name, k=0):
    return ctc_batch64(case(name, k))


@functools.lru_cache(maxsize=None)
def infeasible_made_feasible():
    return _infeasible(_BUILD["infeasible"][1], feasible=True)


def sequential_nll32(lp, target, Ti):
    """-sum_t lp[t, ext] along the ONE alignment of a single-path sample, added in float32 in time order: label k on frame k, or the blank
    between a repeated pair on its frame; L = 0: blanks"""
    lp = np.asarray(lp, dtype=F32)
    target = [int(v) for v in target]
    if len(target) == 0:
        path = [0] * Ti
    else:
        path = []
        for k, c in enumerate(target):
            if k and c == target[k - 1]:
                path.append(0)
            path.append(c)
        assert len(path) == Ti
    acc = lp[0, path[0]]
    for t in range(1, Ti):
        acc = F32(acc + lp[t, path[t]])
    return F32(-acc), path


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. log-softmax: cases, emulation, bounds
# ---------------------------------------------------------------------------------------------------------------------------------------
# Forward, as written: m = max x; s = sum_c expf(x_c - m) (per lane ceil(C / 16) additions, then a 4-level tree); lz = m + logf(s);
# out = x - lz.  Roundings, each <= u of the value it produces (expf / logf: 1 ulp = 2 u):
#   x_c - m          u |x_c - m| on the exponent of term c: moves log s by u W, W = sum_c p_c |x_c - m| (p = softmax)
#   expf             2 u relative on every term        -> 2 u on log s
#   the additions    (ceil(C / 16) + 4) u relative     -> NSUM u on log s
#   logf             2 u |log s|
#   m + logf(s)      u |lz|
#   x - lz           u |out|
# so |out - out64| <= u (|out64| + |lz64| + 2 |log s64| + W + 2 + NSUM)  =: LSM_FWD unit, constant 1.  -inf entries come out -inf exactly.
# Backward, as written: S = sum_c g_c (same order); d = g - expf(lp) * S.  expf 2 u, the product u, the sum NSUM u of sum |g|, the
# subtraction u |d| (a contracted multiply-add drops the product's):
#   |d - d64| <= u (|d64| + 3 p |S64| + NSUM p sum|g|)  =: LSM_BWD unit, constant 1.  bf16 output: + half a bf16 ulp of d64.
# Both units are complete counts: the emulation cannot leave them, and it comes close -- forward 0.65 of the unit (a row with -inf entries,
# C = 16), backward 0.99 (p ~ 1e-6 and d just above a power of two, where the closing rounding alone is u |d|).  The bound is K_LSM = 2 units,
# the rule of every bound here: the emulation stays within half of it (0.33 / 0.50), the other half is the hardware's.
K_LSM = 2.0

LSM_ROWS = (1, 15, 16, 17, 333)
LSM_C = (1, 2, 15, 16, 17, 97, 200)
LSM_KINDS = ("randn", "peak80", "const", "shift1000", "neginf")
LSM_PAD = 1e30


def nsum(C):
    return (C + 15) // 16 + 4


@functools.lru_cache(maxsize=None)
def lsm_case(rows, C, bf16):
    """-> dict x (rows, C) float32 (bf16-exact if bf16), kind (rows,) index into LSM_KINDS, g (rows, C) float32"""
    r = np.random.RandomState(7 * rows + 1000 * C + (1 if bf16 else 0))
    x = (3 * r.randn(rows, C)).astype(F32)
    kind = (np.arange(rows) + r.randint(5)) % 5
    for i in range(rows):
        k = LSM_KINDS[kind[i]]
        if k == "peak80":
            x[i] = r.randn(C)
            x[i, r.randint(C)] += 80
        elif k == "const":
            x[i] = F32(r.randn())
        elif k == "shift1000":
            x[i] += 1000
        elif k == "neginf" and C >= 2:
            x[i, r.choice(C, max(1, C // 3), replace=False)] = NINF
    if bf16:
        x = torch.from_numpy(x).bfloat16().float().numpy()
    g = r.randn(rows, C).astype(F32)
    x.setflags(write=False)
    g.setflags(write=False)
    return dict(x=x, kind=kind, g=g)


def lsm_fwd_ref(x):
    """-> (out64, unit): float64 log-softmax of the float32 / bf16 values and the forward bound per element (inf entries: unit 0, must be equal)"""
    x = np.asarray(x, dtype=np.float64)
    C = x.shape[-1]
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(x - m)
        s = e.sum(-1, keepdims=True)
        W = (e / s * np.where(np.isfinite(x), np.abs(x - m), 0.0)).sum(-1, keepdims=True)
        lz = m + np.log(s)
        out = x - lz
        unit = U * (np.abs(out) + np.abs(lz) + 2 * np.abs(np.log(s)) + W + 2 + nsum(C))
    return out, np.where(np.isfinite(out), unit, 0.0)


def lsm_bwd_ref(lp, g):
    """from the kernel's OWN float32 log-probs -> (d64, unit)"""
    lp, g = np.asarray(lp, dtype=np.float64), np.asarray(g, dtype=np.float64)
    C = lp.shape[-1]
    p = np.exp(lp)
    S = g.sum(-1, keepdims=True)
    d = g - p * S
    return d, U * (np.abs(d) + 3 * p * np.abs(S) + nsum(C) * p * np.abs(g).sum(-1, keepdims=True))


def _lane_sum32(v):
    """(rows, C) float32 -> (rows,): 16 lanes add their strided columns in order, then quad16_sum's butterfly"""
    rows, C = v.shape
    lanes = np.zeros((rows, 16), dtype=F32)
    for c in range(C):
        lanes[:, c % 16] = lanes[:, c % 16] + v[:, c]
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    return lanes[:, 0].astype(F32)


def lsm_fwd32(x):
    x = np.asarray(x, dtype=F32)
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = _lane_sum32(np.exp(x - m))
        lz = (m[:, 0] + np.log(s)).astype(F32)
        return (x - lz[:, None]).astype(F32)


def lsm_bwd32(lp, g):
    lp, g = np.asarray(lp, dtype=F32), np.asarray(g, dtype=F32)
    S = _lane_sum32(g)
    return (g - (np.exp(lp) * S[:, None]).astype(F32)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. greedy decode
# ---------------------------------------------------------------------------------------------------------------------------------------

def first_argmax(lp):
    """(T, N, C) -> (N, T) int64: the FIRST maximum of every row"""
    return np.argmax(np.asarray(lp), axis=-1).T


def collapse(amax_row, Ti):
    """drop repeats (compare with the previous class BEFORE the blank test), then blanks"""
    out, prev = [], -1
    for c in (int(v) for v in amax_row[: max(Ti, 0)]):
        if c == prev:
            continue
        prev = c
        if c != 0:
            out.append(c)
    return out


def plant_argmax(r, want, C):
    """(N, T) class indices -> (T, N, C) float32 log-probs whose first maximum is `want`"""
    N, T = want.shape
    lp = r.randn(T, N, C).astype(F32)
    idx = np.asarray(want).T
    np.put_along_axis(lp, idx[:, :, None], lp.max(-1, keepdims=True) + F32(1), axis=-1)
    return lp

"""The block backward as training runs it: inside a deferral window (ocrs_bwd_defer_begin .. ocrs_bwd_defer_flush; _DetRun._backward opens one whenever
there is no gradient bucketer and no capture), compared with the in-line launches the op tests pin, and with float64.  tests/defer_ref.py states the
references, the bounds (each with its derivation) and the cases once; tests/test_defer_host.py proves on the CPU what these tests rest on.

  a  bf16 matrix-core and row-streaming families (mm_bwd_fin in both forms, mm_bwd_fin_head, mm_bwd_fin_xu, mm_bwd_fin_xu_c1): the weight gradients are
     untouched before the flush and every output is bit-identical to the in-line run after it; the producers' sums, read back as increments of a
     pre-filled gsum, lie within the window bound (in line: the chain bound) of the float64 conversion of the launch's own partials; the partials lie
     within 2^-8 of the float64 sums over the kernel's own stored gradient; the scratch is left zeroed; three windows over one scratch give the same bytes
  b  the fp32 row-streaming family (rs32_bwd direct and pooled, rs32_bwd_head, rs32_convt_dgrad with sums, convt_bwd_parts' weight half): every output,
     the fp64 sums included, bit-identical between window and in-line
  c  the tile route (pw_bwd_fin with each of its kernels, then dw_bwd): dWpw queued by k_pwb and k_pw_bwd2 (the first of the two launches of the
     32 | 32 concat and the generic k_pw_bwd reduce in line); dw_bwd reduces in line when it produces sums, is queued when not
  d  the integer recipe of tests/exact_ref.py (conv0, ConvTranspose) once more inside a window: dW and db EQUAL to float64 after the flush
  e  the window's fallbacks: a scratch with one share for two launches, begin(None, 0), a full queue
  f  DetectionModel's default backward (window) against the in-line route, fp32 (bit-identical) and bf16 (against the float64 oracle gradients)

Worst fractions of the derived bounds, measured on an MI355X (a record, not a bound):
  mm_bwd_fin, 100 cases       gsum: window 0.062 of the window bound, in line 0.188 of the chain bound; partials 0.867 of the 2^-8 bound at (1, 5, 7),
                              0.115 from (2, 21, 37) up
  mm_bwd_fin_head             window 0.055, in line 0.117, partials 0.441
  mm_bwd_fin_xu / _xu_c1      window 0.052, in line 0.126, partials 0.110 (_xu)
  one share, two launches     first launch 0.021 of the window bound, second 0.099 of the chain bound
  rs32_bwd / rs32_bwd_head / rs32_convt_dgrad   0.026 / 0.014 / 0.008 of the fp32-accumulation bound
  bf16 model                  err(window) / (1.25 err(in line) + floor) at most 0.800 (in_conv.seq.0.seq.2.weight)
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import defer_ref as D
from tests import exact_ref as X
from tests.test_bnstat_gpu import padded, untouched
from tests.test_det_ops_gpu import MM_CASES, make_run, nchw, nhwc, rand_tr
from tests.test_exact_gpu import PW_KERNEL, rec_run, same

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _window_closed_at_teardown():
    """a failed assertion can never leave the library in window mode for later test files (flushing a closed window is a no-op)"""
    yield
    from ocrs_models_amd._lib import lib

    lib().bwd_defer_flush()
    torch.cuda.synchronize()


def test_case_tables_are_the_suites(dev):
    assert tuple(MM_CASES) == D.MM_CASES


def pattern(t, k=7):
    """a non-zero pattern of small dyadic values in the shape / dtype of t"""
    n = t.numel()
    return ((torch.arange(n, dtype=torch.float64) % k - (k // 2) + 0.125) * 0.25).to(t.dtype).view(t.shape).to(t.device)


def mk(pfx, cin, cout, P, Bf, g, dev):
    P[f"{pfx}.seq.0.weight"] = (torch.randn(cin, 1, 3, 3, generator=g) / 3).to(dev)
    P[f"{pfx}.seq.1.weight"] = (torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)).to(dev)
    P[f"{pfx}.seq.2.weight"] = (1 + 0.1 * torch.randn(cout, generator=g)).to(dev)
    P[f"{pfx}.seq.2.bias"] = (0.1 * torch.randn(cout, generator=g)).to(dev)
    Bf[f"{pfx}.seq.2.running_mean"] = torch.zeros(cout, device=dev)
    Bf[f"{pfx}.seq.2.running_var"] = torch.ones(cout, device=dev)
    Bf[f"{pfx}.seq.2.num_batches_tracked"] = torch.zeros((), dtype=torch.int64, device=dev)


class Chain:
    """Producers A (and B) -> block C, forward run ONCE; backward() runs C's backward on those stored tensors, in line or inside a window, with
    fresh pre-filled gradients and sums each time.  kind: "fin" (ocrs_mm_bwd_fin / ocrs_rs32_bwd), "head" (the gradient formed from gl: *_bwd_head),
    "xu" / "xu_c1" (A is the first block, C reads its u plane: ocrs_mm_bwd_fin_xu / _xu_c1)."""

    def __init__(self, dev, dtype, C0, Ca, Cb, Cc, shape, pooled, two, kind="fin", fuse=True):
        from ocrs_models_amd._lib import ptr
        from ocrs_models_amd.models import _Act

        self.dev, self.dtype, self.kind, self.pooled = dev, dtype, kind, pooled
        self.Ca, self.Cb, self.Cc, self.shape = Ca, Cb, Cc, shape
        N, H, W = shape
        g = torch.Generator().manual_seed(X.seed_of(61, C0, Ca, Cb, Cc, shape, pooled, two))
        P, Bf = {}, {}
        first = kind in ("xu", "xu_c1")
        if first:
            mk("A", 1, 8, P, Bf, g, dev)
            P["A.seq.1.weight"] = torch.randn(8, 1, 1, 1, generator=g).to(dev)
        else:
            mk("A", C0, Ca, P, Bf, g, dev)
        if Cb:
            mk("B", C0, Cb, P, Bf, g, dev)
        mk("C", Ca + Cb, Cc, P, Bf, g, dev)
        P["C.seq.2.weight"][1] *= -1  # a negative BatchNorm weight: the ReLU mask flips with the sign of gamma
        P["A.seq.2.weight"][2] = 0.0  # tra[0][2] = gamma * rstd is exactly 0: the conversion's sc == 0 rule
        if kind == "head":
            P["out_conv.0.weight"] = torch.randn(1, 8, 1, 1, generator=g).to(dev)
        self.P = P
        run = self.run = make_run(dev, dtype, N, P, Bf)
        run.fuse_bn_bwd = fuse
        L = self.L = run.L
        if first:
            img = (torch.rand(N, 1, H, W, generator=g) - 0.5).to(dev)
            run.x = img
            run.c1_noz = kind == "xu_c1"
            a = run.block_c1("A", img, H, W)
            assert a.u is not None and (a.t is None) == (kind == "xu_c1") and (run.recs["A"].fsum is not None) == (kind == "xu_c1")
            b = None
        else:
            x0 = _Act(nhwc(torch.randn(N, C0, H, W, generator=g).to(dev), dtype), rand_tr(C0, dev, g), C0, H, W)
            a = run.block("A", x0, None, Ca)
            b = run.block("B", x0, None, Cb) if Cb else None
        assert float(a.tr[0, 2]) == 0.0
        self.a, self.b = a, b
        self.out = run.block("C", a, b, Cc, pool=bool(pooled))
        r = self.rec = run.recs["C"]
        gh, gw = (H // 2, W // 2) if pooled else (H, W)
        if kind == "head":
            self.g1, self.g2 = (0.1 * torch.randn(N, H, W, generator=g)).to(dev), None
            self.gsumC = (0.01 * N * H * W * torch.randn(2 * Cc, generator=g, dtype=torch.float64)).to(dev)
        else:
            self.g1 = nhwc(torch.randn(N, Cc, gh, gw, generator=g).to(dev), dtype)
            self.g2 = nhwc(torch.randn(N, Cc, gh, gw, generator=g).to(dev), dtype) if two else None
            # C's own BatchNorm-backward sums, once: both variants derive their dz coefficients from the same bytes
            self.gsumC = torch.zeros(2 * Cc, dtype=torch.float64, device=dev)
            L.bn_bwd_reduce(ptr(self.g1), ptr(self.g2), pooled, ptr(r.z), ptr(r.tr), ptr(r.saved), ptr(self.gsumC), Cc, N, H, W, run.dt)
        self.pre = {"A": (3.0 + 0.37 * torch.arange(2 * Ca, dtype=torch.float64)).to(dev)}
        if Cb:
            self.pre["B"] = (-2.0 + 0.23 * torch.arange(2 * Cb, dtype=torch.float64)).to(dev)
        self.gkeys = [f"C.seq.{k}" for k in ("0.weight", "1.weight", "2.weight", "2.bias")]
        self.fill = {k: pattern(P[k]) for k in self.gkeys}
        torch.cuda.synchronize()

    def route(self):
        return self.run.bwd_route(self.rec, self.pooled, True)

    def backward(self, scratch=None, window=False, null_scratch=False):
        """-> (results after the flush, snapshot before the flush (window only)); everything on the CPU"""
        from ocrs_models_amd._lib import ptr

        run, L = self.run, self.L
        run.G = {k: (self.fill[k].clone() if k in self.fill else torch.zeros_like(v)) for k, v in self.P.items()}
        run.fused = {"C": self.gsumC.clone(), **{k: v.clone() for k, v in self.pre.items()}}
        if not run.fuse_bn_bwd:
            run.fused = {"C": self.gsumC.clone()}
        run._keep_ws, run._c1acc = [], None
        run._head_gl = self.g1 if self.kind == "head" else None
        before = None
        if window:
            L.bwd_defer_begin(None if null_scratch else ptr(scratch), 0 if null_scratch else scratch.numel())
        try:
            gxa, gxb = run.block_bwd("C", self.g1, self.g2, self.pooled)
            if window:
                torch.cuda.synchronize()
                before = self.collect(gxa, gxb)
        finally:
            if window:
                L.bwd_defer_flush()
        torch.cuda.synchronize()
        res = self.collect(gxa, gxb)
        run._keep_ws, run._c1acc, run._head_gl = None, None, None
        return res, before

    def collect(self, gxa, gxb):
        run = self.run
        res = {"gxa": gxa, "gxb": gxb, "c1acc": run._c1acc, "fusedA": run.fused.get("A"), "fusedB": run.fused.get("B"), "ws": run._keep_ws}
        res.update({k: run.G[k] for k in self.gkeys})
        return {k: ([w.cpu().clone() for w in v] if isinstance(v, list) else v.cpu().clone()) for k, v in res.items() if v is not None}


def equal_outputs(got, want, keys, what):
    for k in keys:
        if k in want or k in got:
            assert k in got and k in want and torch.equal(got[k], want[k]), f"{what}: {k}"


OUT_KEYS = ("gxa", "gxb", "c1acc", "C.seq.0.weight", "C.seq.1.weight", "C.seq.2.weight", "C.seq.2.bias")


def tie_reference(gx, x, tr):
    """float64 sums over the kernel's own stored gradient gx and stored input x [N][H][W][C]: sum gx [x~ > lo], sum gx x~ [x~ > lo] and the sums of
    their absolute terms.  (x * sc + sh is exact in float64 for a bf16 x and fp32 sc, sh up to the last add, so its sign is the sign the kernel's fmaf
    sees.)"""
    gx, x, tr = gx.double().numpy(), x.double().numpy(), tr.double().numpy()
    pre = x * tr[0] + tr[1]
    xt = np.maximum(pre, tr[2])
    m = (xt > tr[2]) * gx
    ax = (0, 1, 2)
    return m.sum(ax), (m * xt).sum(ax), np.abs(m).sum(ax), np.abs(m * xt).sum(ax)


def frac(got, want, bound):
    got, want, bound = (np.asarray(v, np.float64) for v in (got, want, bound))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(got - want) / bound
    return float(np.max(np.where(bound > 0, f, np.where(got == want, 0.0, np.inf))))


def launches(cs, nb):
    """[(offset of the launch's partials in ws, Cin, Ca, sources)]: one launch, or one per source of the 32 | 32 split"""
    if (cs.Ca, cs.Cb) == (32, 32):
        return [(0, 32, 32, ["A"]), (D.split_stride(nb, cs.Cc), 32, 32, ["B"])]
    return [(0, cs.Ca + cs.Cb, cs.Ca, ["A"] + (["B"] if cs.Cb else []))]


def check_sums(cs, nb, res, bound_fn, what, only=None):
    """the increments of the producers' pre-filled gsum against the float64 conversion of the launch's own partials -> worst fraction of the bound
    (only: the launches of these sources)"""
    worst = 0.0
    ws = res["ws"][-1].numpy()
    src = {"A": cs.a, "B": cs.b}
    for off, Cin, Ca, names in launches(cs, nb):
        if only is not None and names != only:
            continue
        T1, T2, A1, A2 = D.sums_from_partials(ws[off:], nb, Cin, cs.Cc)
        tr = [src[n].tr.cpu().numpy() for n in names]
        saved = [cs.run.recs[n].saved.cpu().numpy() for n in names]
        pre = [cs.pre[n].cpu().numpy().reshape(2, -1) for n in names]
        want = D.convert(T1, T2, tr, saved, Ca)
        bound = D.convert_bound(bound_fn(nb, A1), bound_fn(nb, A2), T1, T2, tr, saved, Ca, pre)
        for n, w, b, p in zip(names, want, bound, pre):
            inc = res["fused" + n].numpy().reshape(2, -1) - p
            f = frac(inc, w, b)
            assert f <= 1.0, f"{what}: gsum of {n}: {f:.3g}x the bound"
            assert float(src[n].tr[0, 2]) != 0.0 or inc[1, 2] == 0.0, "a channel with scale 0 gets nothing in the second row"
            worst = max(worst, f)
    return worst


def check_tie(cs, nb, res):
    """the partials against the operation -> worst fraction of the 2^-8 bound (None: the entry point stores no input gradient)"""
    if "gxa" not in res:
        return None
    ws = res["ws"][-1].numpy()
    worst = 0.0
    gx = {"A": res["gxa"], "B": res.get("gxb")}
    src = {"A": cs.a, "B": cs.b}
    for off, Cin, Ca, names in launches(cs, nb):
        T1, T2, _, _ = D.sums_from_partials(ws[off:], nb, Cin, cs.Cc)
        c0 = 0
        for n in names:
            C = src[n].C
            r1, r2, a1, a2 = tie_reference(gx[n].float(), src[n].t.float().cpu(), src[n].tr.cpu())
            f1, f2 = frac(T1[c0:c0 + C], r1, D.tie_bound(a1)), frac(T2[c0:c0 + C], r2, D.tie_bound(a2))
            assert f1 <= 1.0 and f2 <= 1.0, f"partials of {n}: S1 {f1:.3g}x, S2 {f2:.3g}x the 2^-8 bound"
            worst = max(worst, f1, f2)
            c0 += C
    return worst


def window_against_inline(cs, nb, name):
    """section (a) for one built chain"""
    dev = cs.dev
    scratch = torch.zeros(2048, dtype=torch.float64, device=dev)
    inline, _ = cs.backward()
    assert not torch.equal(inline["C.seq.1.weight"], cs.fill["C.seq.1.weight"].cpu())
    wins = []
    for rep in range(3):  # (the second and third window reuse the scratch the one before left)
        res, before = cs.backward(scratch, window=True)
        assert not bool(scratch.any()), f"window {rep}: the scratch is not left zeroed"
        for k in ("C.seq.0.weight", "C.seq.1.weight"):
            assert torch.equal(before[k], cs.fill[k].cpu()), f"{k} was written before the flush: the reduction was not queued"
        equal_outputs(before, res, ("gxa", "gxb", "c1acc", "C.seq.2.weight", "C.seq.2.bias", "fusedA", "fusedB"), "complete before the flush")
        wins.append(res)
    for res in wins[1:]:
        equal_outputs(res, wins[0], OUT_KEYS + ("fusedA", "fusedB"), "three windows, different bytes")
    equal_outputs(wins[0], inline, OUT_KEYS, "window vs in line")
    for off, Cin, _, _ in launches(cs, nb):  # (the workspace behind the partials is never written, or holds the scratch lines of border tiles)
        n = nb * D.ne_of(Cin, cs.Cc)
        assert torch.equal(wins[0]["ws"][-1][off:off + n], inline["ws"][-1][off:off + n]), "the partials differ between the variants"
    fw = check_sums(cs, nb, wins[0], D.window_sum_bound, "window")
    fi = check_sums(cs, nb, inline, D.inline_sum_bound, "in line")
    ft = check_tie(cs, nb, inline)
    print(f"{name} nb={nb}: gsum within {fw:.3f} of the window bound, in line {fi:.3f} of the chain bound; partials "
          + (f"{ft:.3f} of the 2^-8 bound" if ft is not None else "not tied (no stored input gradient)"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. bf16 matrix-core and row-streaming families
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0,Ca,Cb,Cc,shape,pooled,two", D.block_cases(), ids=_ids)
def test_mm_bwd_fin_window_against_inline_and_float64(dev, C0, Ca, Cb, Cc, shape, pooled, two):
    """ocrs_mm_bwd_fin: k_mm_bwd (direct and pooled, whole and border-cut tiles, the two launches of the 32 | 32 split) and, for 8 -> 16 channels
    unpooled, k_rs_bwd"""
    cs = Chain(dev, BF16, C0, Ca, Cb, Cc, shape, pooled, two)
    nb = int(cs.L.mm_bwd_nparts(Ca, Cb, Cc, pooled, two, *shape))
    assert nb == D.nb_table()[(C0, Ca, Cb, Cc, shape, pooled, two)] and cs.route() == "mm" and cs.L.mm_bwd_supported(Ca, Cb, Cc, cs.run.dt)
    assert cs.a.u is None
    window_against_inline(cs, nb, f"mm_bwd_fin{' (k_rs_bwd)' if D.rs_form(Ca, Cb, Cc, pooled) else ''} {Ca}|{Cb}->{Cc} {_ids(shape)} pooled={pooled} g2={two}")


@pytest.mark.parametrize("shape", D.SHAPES, ids=_ids)
def test_mm_bwd_fin_head_window_against_inline_and_float64(dev, shape):
    """ocrs_mm_bwd_fin_head (k_rs_bwd<HEAD>): the block in front of out_conv, its gradient formed from gl inside the launch"""
    cs = Chain(dev, BF16, 8, 8, 0, 8, shape, 0, 0, kind="head")
    nb = int(cs.L.mm_bwd_nparts(8, 0, 8, 0, 0, *shape))
    assert nb == D.nb_of(8, 0, 8, 0, *shape) and cs.route() == "mm" and cs.L.mm_bwd_head_supported(8, 0, 8, *shape, cs.run.dt)
    window_against_inline(cs, nb, f"mm_bwd_fin_head {_ids(shape)}")


@pytest.mark.parametrize("two", [0, 1])
@pytest.mark.parametrize("kind", ["xu", "xu_c1"])
def test_mm_bwd_fin_xu_window_against_inline_and_float64(dev, kind, two):
    """ocrs_mm_bwd_fin_xu / ocrs_mm_bwd_fin_xu_c1 (k_rs_bwd<XU>, <C1>): the block behind the first block, its input rebuilt from the u plane; _c1
    stores no input gradient (its partials are tied to the operation through _xu, the same loop) and accumulates c1acc"""
    shape = D.XU_SHAPE
    cs = Chain(dev, BF16, 1, 8, 0, 8, shape, 0, two, kind=kind)
    nb = int(cs.L.mm_bwd_nparts(8, 0, 8, 0, two, *shape))
    assert nb == D.nb_of(8, 0, 8, 0, *shape) == 2 and cs.route() == "mm" and cs.L.mm_bwd_head_supported(8, 0, 8, *shape, cs.run.dt)
    inline, _ = cs.backward()
    assert ("c1acc" in inline) == (kind == "xu_c1") and ("gxa" in inline) == (kind == "xu")
    window_against_inline(cs, nb, f"mm_bwd_fin_{kind} g2={two}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# e. the window's fallbacks on block kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_scratch_with_one_share_for_two_launches(dev):
    """a scratch of exactly 16 Cin + 2 doubles and the two launches of the 32 | 32 split: the first takes the share and behaves as in (a); the second
    finds none and is complete -- sums and its columns of the weight gradients -- BEFORE the flush, with the in-line run's bytes"""
    C0, Ca, Cb, Cc, shape = 16, 32, 32, 32, (2, 21, 37)
    cs = Chain(dev, BF16, C0, Ca, Cb, Cc, shape, 0, 1)
    nb = int(cs.L.mm_bwd_nparts(Ca, Cb, Cc, 0, 1, *shape))
    scratch = torch.zeros(16 * 32 + 2, dtype=torch.float64, device=dev)
    inline, _ = cs.backward()
    res, before = cs.backward(scratch, window=True)
    assert not bool(scratch.any())
    fill_pw, fill_dw = cs.fill["C.seq.1.weight"].cpu(), cs.fill["C.seq.0.weight"].cpu()
    assert torch.equal(before["C.seq.1.weight"][:, :32], fill_pw[:, :32]) and torch.equal(before["C.seq.0.weight"][:32], fill_dw[:32]), "first launch: queued"
    assert torch.equal(before["C.seq.1.weight"][:, 32:], inline["C.seq.1.weight"][:, 32:]), "second launch: dWpw complete before the flush"
    assert torch.equal(before["C.seq.0.weight"][32:], inline["C.seq.0.weight"][32:]), "second launch: dWdw complete before the flush"
    assert torch.equal(before["fusedB"], inline["fusedB"]), "second launch: the sums of k_mm_bwd_reduce, bit for bit"
    equal_outputs(res, inline, OUT_KEYS + ("fusedB",), "after the flush")
    f = check_sums(cs, nb, res, D.window_sum_bound, "first launch (window)", only=["A"])
    fb = check_sums(cs, nb, res, D.inline_sum_bound, "second launch (in line)", only=["B"])
    print(f"one share, two launches: first launch's gsum within {f:.3f} of the window bound, the second's {fb:.3f} of the chain bound")


def test_window_without_scratch(dev):
    """begin(None, 0): a launch that wants sums runs k_mm_bwd_reduce in line (complete before the flush, the in-line bytes); one that wants none is queued"""
    for fuse in (True, False):
        cs = Chain(dev, BF16, 8, 16, 0, 16, (2, 21, 37), 0, 1, fuse=fuse)
        inline, _ = cs.backward()
        res, before = cs.backward(window=True, null_scratch=True)
        assert ("fusedA" in inline) == fuse
        keys = OUT_KEYS + ("fusedA",)
        equal_outputs(res, inline, keys, "after the flush")
        if fuse:
            equal_outputs(before, inline, keys, "a launch with sums and no scratch is complete before the flush")
        else:
            for k in ("C.seq.0.weight", "C.seq.1.weight"):
                assert torch.equal(before[k], cs.fill[k].cpu()), f"{k}: a launch without sums is queued"


def test_fifty_block_backwards_in_one_window(dev):
    """50 block backwards at the nb == 1 shape onto 50 gradient buffers in one window: the queue holds 48, calls 49 and 50 reduce at once.  All 50 equal
    the in-line bytes, the padding around the buffers is untouched, and the producers' sums took 50 increments"""
    from ocrs_models_amd._lib import ptr

    C0, Ca, Cb, Cc, shape = 8, 8, 8, 8, (1, 5, 7)
    cs = Chain(dev, BF16, C0, Ca, Cb, Cc, shape, 0, 0)
    run, L = cs.run, cs.L
    assert int(L.mm_bwd_nparts(Ca, Cb, Cc, 0, 0, *shape)) == 1
    npw, ndw = Cc * 16, 16 * 9
    scratch = torch.zeros(50 * (16 * 16 + 2), dtype=torch.float64, device=dev)
    out = {}
    for window in (False, True):
        pw_buf, pw = padded(50 * npw, dev, fill=pattern(torch.empty(50 * npw)))
        dw_buf, dw = padded(50 * ndw, dev, fill=pattern(torch.empty(50 * ndw)))
        run.fused = {k: v.clone() for k, v in cs.pre.items()}
        run._keep_ws = []
        gx = []
        if window:
            L.bwd_defer_begin(ptr(scratch), scratch.numel())
        try:
            for i in range(50):
                run.G = {k: torch.zeros_like(v) for k, v in cs.P.items()}
                run.G["C.seq.1.weight"] = pw[i * npw:(i + 1) * npw].view(Cc, 16, 1, 1)
                run.G["C.seq.0.weight"] = dw[i * ndw:(i + 1) * ndw].view(16, 1, 3, 3)
                run.fused["C"] = cs.gsumC.clone()
                gx.append(run.block_bwd("C", cs.g1, None, 0))
        finally:
            if window:
                L.bwd_defer_flush()
        torch.cuda.synchronize()
        assert untouched(pw_buf, 50 * npw) and untouched(dw_buf, 50 * ndw), "written outside the gradient buffers"
        out[window] = (pw.cpu().clone(), dw.cpu().clone(), [(a.cpu(), b.cpu()) for a, b in gx], {k: v.cpu().clone() for k, v in run.fused.items()},
                       run._keep_ws[0].cpu().numpy())
        run._keep_ws = None
    assert not bool(scratch.any())
    for i in range(50):
        assert torch.equal(out[True][0][i * npw:(i + 1) * npw], out[False][0][i * npw:(i + 1) * npw]), f"dWpw of call {i + 1}"
        assert torch.equal(out[True][1][i * ndw:(i + 1) * ndw], out[False][1][i * ndw:(i + 1) * ndw]), f"dWdw of call {i + 1}"
        assert torch.equal(out[True][2][i][0], out[False][2][0][0]) and torch.equal(out[True][2][i][1], out[False][2][0][1])
    assert not torch.equal(out[True][0], pattern(torch.empty(50 * npw)))
    # 50 equal increments: 50 times the bound of one, with the += rounding at the final magnitude.  (At nb == 1 the in-line chain adds its one partial
    # to zeros, which is exact: the window bound holds for the in-line run too.)
    T1, T2, A1, A2 = D.sums_from_partials(out[True][4], 1, 16, Cc)
    tr, saved = [cs.a.tr.cpu().numpy(), cs.b.tr.cpu().numpy()], [run.recs[n].saved.cpu().numpy() for n in "AB"]
    want = D.convert(T1, T2, tr, saved, Ca)
    pre = [cs.pre[n].cpu().numpy().reshape(2, -1) for n in "AB"]
    big = [np.abs(p) + 50 * np.abs(w) for p, w in zip(pre, want)]
    bound = D.convert_bound(D.window_sum_bound(1, A1), D.window_sum_bound(1, A2), T1, T2, tr, saved, Ca, big)
    for n, w, b, p in zip("AB", want, bound, pre):
        for window in (False, True):
            assert frac(out[window][3][n].numpy().reshape(2, -1) - p, 50 * w, 50 * b) <= 1.0, (n, window)


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. the fp32 row-streaming family
# ---------------------------------------------------------------------------------------------------------------------------------------
def rs32_sums_check(cs, res, name):
    """the fp64 sums against float64 over the kernel's own fp32 gx.  Every workgroup sums its terms in fp32 and hands ONE fp32 partial per channel to the
    fp64 atomics: whatever the order inside the workgroup, n terms summed in fp32 are within (n - 1) 2^-24 of sum |terms|, n <= N H W here; the terms
    themselves (gx x~, x~ = fmaf(x, sc, sh)) carry two more roundings.  -> worst fraction of (N H W + 2) 2^-24 sum |terms|, through the conversion"""
    N, H, W = cs.shape
    worst = 0.0
    src = {"A": cs.a, "B": cs.b}
    for n, key in (("A", "gxa"), ("B", "gxb")):
        if src[n] is None or "fused" + n not in res:
            continue
        r1, r2, a1, a2 = tie_reference(res[key], src[n].t.cpu(), src[n].tr.cpu())
        tr, saved, pre = [src[n].tr.cpu().numpy()], [cs.run.recs[n].saved.cpu().numpy()], [cs.pre[n].cpu().numpy().reshape(2, -1)]
        u = (N * H * W + 2) * D.U32
        want = D.convert(r1, r2, tr, saved, src[n].C)[0]
        bound = D.convert_bound(u * a1, u * a2, r1, r2, tr, saved, src[n].C, pre)[0]
        f = frac(res["fused" + n].numpy().reshape(2, -1) - pre[0], want, bound)
        assert f <= 1.0, f"{name}: gsum of {n}: {f:.3g}x the bound"
        worst = max(worst, f)
    return worst


def rs32_window_against_inline(cs, name):
    scratch = torch.zeros(2048, dtype=torch.float64, device=cs.dev)
    inline, _ = cs.backward()
    wins = []
    for rep in range(2):
        res, before = cs.backward(scratch, window=True)
        assert not bool(scratch.any()), "the scratch is not left zeroed"
        for k in ("C.seq.0.weight", "C.seq.1.weight"):
            assert torch.equal(before[k], cs.fill[k].cpu()), f"{k} was written before the flush"
        equal_outputs(before, res, ("gxa", "gxb", "C.seq.2.weight", "C.seq.2.bias", "fusedA", "fusedB"), "complete before the flush")
        equal_outputs(res, inline, OUT_KEYS + ("fusedA", "fusedB"), "window vs in line")
        wins.append(res)
    f = rs32_sums_check(cs, inline, name)
    print(f"{name}: gsum within {f:.4f} of the fp32-accumulation bound")


# (C0, Ca, Cb, Cc, pooled): k_rs32_bwd with one source (8 -> 8: two strips per wave) and two, the two passes of 16 | 16, k_rs32_bwdx (16 -> 32), and the
# pooled k_rs32_bwdp at its four channel shapes (the concat and wide shapes have no pooled form: they run tiled, section c)
RS32_CASES = ([(8, 8, 0, 8, 0), (8, 8, 0, 16, 0), (8, 16, 0, 8, 0), (8, 16, 0, 16, 0), (8, 8, 8, 16, 0), (16, 16, 16, 16, 0), (8, 16, 0, 32, 0)]
              + [(8, 8, 0, 8, 1), (8, 8, 0, 16, 1), (8, 16, 0, 8, 1), (8, 16, 0, 16, 1)])


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 21, 37)], ids=_ids)
@pytest.mark.parametrize("C0,Ca,Cb,Cc,pooled", RS32_CASES)
def test_rs32_bwd_window_is_bit_identical_to_inline(dev, C0, Ca, Cb, Cc, pooled, shape):
    """ocrs_rs32_bwd: the last-workgroup state comes from the window's scratch instead of the file's own buffer, the weight gradients are queued"""
    cs = Chain(dev, F32, C0, Ca, Cb, Cc, shape, pooled, 1)
    assert cs.L.rs32_bwd_supported(Ca, Cb, Cc, pooled, cs.run.dt) and cs.route() == "rs32"
    rs32_window_against_inline(cs, f"rs32_bwd {Ca}|{Cb}->{Cc} {_ids(shape)} pooled={pooled}")


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 21, 37)], ids=_ids)
def test_rs32_bwd_head_window_is_bit_identical_to_inline(dev, shape):
    cs = Chain(dev, F32, 8, 8, 0, 8, shape, 0, 0, kind="head")
    assert cs.route() == "rs32" and cs.L.rs32_bwd_head_supported(8, 0, 8, cs.run.dt)
    rs32_window_against_inline(cs, f"rs32_bwd_head {_ids(shape)}")


@pytest.mark.parametrize("dims", [(16, 8, 6, 9, 12, 19), (32, 16, 5, 7, 11, 14), (16, 8, 40, 37, 81, 75)], ids=_ids)
def test_rs32_convt_window_is_bit_identical_to_inline(dev, dims):
    """ocrs_rs32_convt_dgrad with the producer's sums, and the weight / bias half of ocrs_convt_bwd_parts (k_rs32_ctw through det_rs32_ctw_launch): dx and
    the fp64 sums bit-identical, dW / dbias untouched before the flush and complete after it, dbias64 left as given"""
    from ocrs_models_amd._lib import ptr

    Cup, Cout, h, w, H, W = dims
    N = 2
    g = torch.Generator().manual_seed(X.seed_of(62, dims))
    run = make_run(dev, F32, N, {}, {})
    L = run.L
    assert L.rs32_convt_dgrad_supported(Cup, Cout, run.dt) and L.convt_bwd_splittable(Cup, Cout, run.dt)
    xs, tr = nhwc(torch.randn(N, Cup, h, w, generator=g).to(dev), F32), rand_tr(Cup, dev, g)
    Wt = (torch.randn(Cup, Cout, 3, 3, generator=g) / math.sqrt(2.25 * Cup)).to(dev)
    gy = nhwc(torch.randn(N, Cout, H, W, generator=g).to(dev), F32)
    saved = torch.stack([0.1 * torch.randn(Cup, generator=g), 1 + 0.2 * torch.rand(Cup, generator=g)]).to(dev)
    wpk_d = run.pack(Wt, 0, 9 * Cout, Cup, Cout, 1, 9, 9 * Cout)
    pre = (1.0 + 0.3 * torch.arange(2 * Cup, dtype=torch.float64)).to(dev)
    scratch = torch.zeros(1024, dtype=torch.float64, device=dev)
    out = {}
    for window in (False, True, True):
        dx = torch.full((N, h, w, Cup), float("nan"), device=dev)
        dW, db = pattern(Wt), pattern(torch.empty(Cout, device=dev))
        db64 = pattern(torch.empty(Cout, dtype=torch.float64, device=dev))
        gsum = pre.clone()
        ws = torch.empty(L.convt_bwd_ws_floats(Cup, Cout, N, h, w, run.dt), device=dev)
        if window:
            L.bwd_defer_begin(ptr(scratch), scratch.numel())
        try:
            L.convt_bwd_parts(ptr(xs), ptr(tr), ptr(gy), ptr(wpk_d), ptr(dx), ptr(dW), ptr(db), ptr(db64), ptr(ws), None, None, Cup, Cout, N, h, w, H, W, 2, run.dt)
            L.rs32_convt_dgrad(ptr(gy), ptr(Wt), ptr(dx), ptr(xs), ptr(tr), ptr(saved), ptr(gsum), Cup, Cout, N, h, w, H, W)
            if window:
                torch.cuda.synchronize()
                assert torch.equal(dW, pattern(Wt)) and torch.equal(db, pattern(db)), "dW / dbias written before the flush"
                before = (dx.cpu().clone(), gsum.cpu().clone())
        finally:
            if window:
                L.bwd_defer_flush()
        torch.cuda.synchronize()
        assert torch.equal(db64, pattern(db64)), "dbias64 is left as given"
        assert not bool(scratch.any())
        res = (dx.cpu(), gsum.cpu(), dW.cpu(), db.cpu())
        if window:
            assert torch.equal(before[0], res[0]) and torch.equal(before[1], res[1])
            for name, a, b in zip(("dx", "gsum", "dW", "dbias"), res, out[False]):
                assert torch.equal(a, b), name
        else:
            out[False] = res
            assert not torch.equal(res[2], pattern(Wt).cpu())
    dxc, gs = out[False][0], out[False][1]
    r1, r2, a1, a2 = tie_reference(dxc, xs.cpu(), tr.cpu())
    u = (N * h * w + 2) * D.U32
    trn, svn, pren = [tr.cpu().numpy()], [saved.cpu().numpy()], [pre.cpu().numpy().reshape(2, -1)]
    f = frac(gs.numpy().reshape(2, -1) - pren[0], D.convert(r1, r2, trn, svn, Cup)[0], D.convert_bound(u * a1, u * a2, r1, r2, trn, svn, Cup, pren)[0])
    assert f <= 1.0, f
    print(f"rs32_convt_dgrad {_ids(dims)}: gsum within {f:.4f} of the fp32-accumulation bound")


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. the tile route
# ---------------------------------------------------------------------------------------------------------------------------------------
TILE_CASES = [("k_pwb", "bf16", (32, 64, 0, 64)), ("k_pwb", "bf16", (16, 32, 0, 64)), ("k_pw_bwd2", "bf16", (8, 16, 0, 16)), ("k_pw_bwd2 x2", "bf16", (16, 32, 32, 32)),
              ("k_pw_bwd", "fp32", (32, 64, 0, 64)), ("k_pw_bwd", "fp32", (8, 8, 8, 16))]


@pytest.mark.parametrize("fuse", [True, False], ids=["sums", "nosums"])
@pytest.mark.parametrize("pooled", [0, 1])
@pytest.mark.parametrize("kernel,dname,chans", TILE_CASES, ids=_ids)
def test_tile_route_window_against_inline(dev, kernel, dname, chans, pooled, fuse):
    """ocrs_pw_bwd_fin (k_pwb, k_pw_bwd2 once and once per source of the 32 | 32 concat, the generic k_pw_bwd) followed by ocrs_dw_bwd: dWpw is queued
    (of the two launches of the 32 | 32 concat only the second's half: they share a workspace; the generic kernel's not at all); dw_bwd with producer sums reduces in line (dWdw and
    the sums complete before the flush), without sums it is queued.  Everything equals the in-line run bit for bit: this route has no sum that
    changes order."""
    dtype = {"fp32": F32, "bf16": BF16}[dname]
    C0, Ca, Cb, Cc = chans
    shape = (2, 11, 15)
    cs = Chain(dev, dtype, C0, Ca, Cb, Cc, shape, pooled, 1, fuse=fuse)
    cs.run.use_mm = not kernel.startswith("k_pw_bwd2")  # (k_pw_bwd2 takes the matrix-core shapes and runs where those kernels are off)
    if dname == "fp32" and cs.route() != "tile":
        cs.run.use_rs32 = False
    assert cs.route() == "tile" and cs.L.pw_bwd_kernel(Ca, Cb, Cc, cs.run.dt) == PW_KERNEL[kernel]
    scratch = torch.zeros(2048, dtype=torch.float64, device=dev)
    inline, _ = cs.backward()
    for rep in range(2):
        res, before = cs.backward(scratch, window=True)
        assert not bool(scratch.any())
        pw, fill_pw = before["C.seq.1.weight"], cs.fill["C.seq.1.weight"].cpu()
        if kernel == "k_pw_bwd2 x2":
            # the two launches share one workspace: the first reduces its partials at once (queued, both reductions would read the second launch's at
            # the flush -- what this case found), the second is queued
            assert torch.equal(pw[:, :32], inline["C.seq.1.weight"][:, :32]) and torch.equal(pw[:, 32:], fill_pw[:, 32:]), "dWpw before the flush"
        elif kernel == "k_pw_bwd":
            # launch_pw_bwd (csrc/det_bwd.hip) launches k_wgrad_partials_reduce itself, not through det_wgrad_reduce_launch: the generic kernel's dWpw
            # is never queued -- complete before the flush, with the in-line bytes
            assert torch.equal(pw, inline["C.seq.1.weight"]), "dWpw of the generic kernel is reduced in line"
        else:
            assert torch.equal(pw, fill_pw), "dWpw was written before the flush"
        if fuse:
            assert torch.equal(before["C.seq.0.weight"], inline["C.seq.0.weight"]), "dw_bwd with sums reduces in line"
        else:
            assert torch.equal(before["C.seq.0.weight"], cs.fill["C.seq.0.weight"].cpu()), "dw_bwd without sums is queued"
        assert ("fusedA" in inline) == fuse
        equal_outputs(before, inline, ("gxa", "gxb", "C.seq.2.weight", "C.seq.2.bias", "fusedA", "fusedB"), "complete before the flush")
        equal_outputs(res, inline, OUT_KEYS + ("fusedA", "fusedB"), "window vs in line")


# ---------------------------------------------------------------------------------------------------------------------------------------
# d. linear kernels on the integer recipe, in a window
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", X.CONV0_SHAPES, ids=_ids)
def test_conv0_backward_in_a_window_is_bit_exact(dev, dname, shape):
    """the backward of test_conv0_bit_exact_with_tied_maxima between begin(None, 0) (as the recogniser opens it) and flush: dW and db EQUAL to float64"""
    from ocrs_models_amd._lib import ptr

    dtype = {"fp32": F32, "bf16": BF16}[dname]
    N, H, W = shape
    case = X.conv0_case(X.seed_of(6, shape), *shape)
    ref = X.conv0_reference(case)
    r = rec_run(dev, dtype, N, H, W)
    img, w, b = case["img"].to(dev), case["w"].to(dev), case["b"].to(dev)
    gy = nhwc(case["gy"], dtype).to(dev)
    dW, db = torch.zeros_like(w), torch.zeros_like(b)
    r.L.bwd_defer_begin(None, 0)
    try:
        r.L.conv0_bwd(ptr(img), ptr(w), ptr(b), ptr(gy), ptr(dW), ptr(db), N, H, W, r.dt)
    finally:
        r.L.bwd_defer_flush()
    torch.cuda.synchronize()
    assert same(dW, ref["dW"]), "dW"
    assert same(db, ref["db"]), "db"


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", X.CONVT_CASES, ids=_ids)
def test_conv_transpose_backward_in_a_window_is_bit_exact(dev, dname, dims):
    """the backward of test_conv_transpose_bit_exact inside a window: dx, dW and db EQUAL to float64 after the flush"""
    from ocrs_models_amd._lib import ptr

    dtype = {"fp32": F32, "bf16": BF16}[dname]
    Cup, Cout, h, w, H, W = dims
    N = 2
    case = X.convt_case(X.seed_of(4, dims), *dims)
    ref = X.convt_reference(case)
    run = make_run(dev, dtype, N, {}, {})
    L = run.L
    xs, tr, Wt, bias = nhwc(case["x"], dtype).to(dev), case["tr"].to(dev), case["W"].to(dev), case["b"].to(dev)
    gy = nhwc(case["gy"], dtype).to(dev)
    dx = run.empty(N, h, w, Cup)
    dW, db = torch.zeros_like(Wt), torch.zeros_like(bias)
    ws = torch.empty(L.convt_bwd_ws_floats(Cup, Cout, N, h, w, run.dt), device=dev)
    db64 = torch.zeros(Cout, dtype=torch.float64, device=dev)
    scratch = torch.zeros(1024, dtype=torch.float64, device=dev)
    L.bwd_defer_begin(ptr(scratch), scratch.numel())
    try:
        L.convt_bwd(ptr(xs), ptr(tr), ptr(gy), ptr(run.pack(Wt, 0, 9 * Cout, Cup, Cout, 1, 9, 9 * Cout)), ptr(dx), ptr(dW), ptr(db), ptr(db64), ptr(ws), None, None,
                    Cup, Cout, N, h, w, H, W, run.dt)
    finally:
        L.bwd_defer_flush()
    torch.cuda.synchronize()
    assert same(nchw(dx).cpu().double(), ref["dx"]), "dgrad"
    assert same(dW, ref["dW"]), "wgrad"
    assert same(db.double() + db64, ref["db"]), "dbias"
    assert not bool(scratch.any())


# ---------------------------------------------------------------------------------------------------------------------------------------
# f. the model
# ---------------------------------------------------------------------------------------------------------------------------------------
class _NoBucketer:
    """stands in for a gradient bucketer: with one attached _DetRun._backward opens no window and runs every second stage in line"""

    def ready(self, flat, lo, hi):
        pass

    def finish(self, flat):
        pass


@functools.lru_cache(maxsize=None)
def _model_case():
    from oracle import detection as odet
    from oracle import losses as olosses
    from oracle.params import detection_specs, make_state

    seed, B, H, W = 41, 2, 64, 96
    r = np.random.RandomState(seed)
    x = torch.from_numpy(r.uniform(-0.5, 0.5, (B, 1, H, W)).astype(np.float32))
    mask = torch.from_numpy((r.uniform(0, 1, (B, 1, H, W)) > 0.85).astype(np.float32))
    P64, Bf64 = make_state(detection_specs(), seed, torch.float64)
    loss = olosses.balanced_bce(odet.forward(P64, Bf64, x.double(), True), mask.double())
    grads = torch.autograd.grad(loss, list(P64.values()))
    return seed, x, mask, dict(zip(P64, (g.detach() for g in grads)))


def _model_grads(dev, seed, x, mask, bf16, inline):
    import ocrs_models_amd as oa
    from oracle.params import detection_specs, make_state, state_dict_from

    specs = detection_specs()
    P, Bf = make_state(specs, seed)
    m = oa.DetectionModel(act_dtype=BF16 if bf16 else None)
    m.load_state_dict(state_dict_from(P, Bf, specs))
    m = m.to(dev)
    m.train()
    if inline:
        m._grad_bucketer = _NoBucketer()
    try:
        loss = oa.balanced_cross_entropy_loss(m(x.to(dev)), mask.to(dev))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        if inline:
            del m._grad_bucketer
    return {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_model_backward_window_against_inline(dev, dname):
    """DetectionModel at 2 x 1 x 64 x 96: the default backward (window) against the in-line route.  fp32: every parameter gradient bit-identical
    (nothing on that route sums in a different order).  bf16: the window's exact sums and the in-line chain sums differ in the last bits of gsum, which
    moves bf16 roundings downstream; both are compared with the float64 oracle gradients of the same step and, per parameter,
    err(window) <= 1.25 err(in-line) + 1e-6 |ref|_max (the in-line route is what the op tests pin; 25 % for run-to-run rounding flips)."""
    seed, x, mask, ref = _model_case()
    bf16 = dname == "bf16"
    w1, w2 = _model_grads(dev, seed, x, mask, bf16, False), _model_grads(dev, seed, x, mask, bf16, False)
    diff = [k for k in w1 if not torch.equal(w1[k], w2[k])]
    assert not diff, f"two default runs differ in {diff[:4]} ({len(diff)} tensors): {dname} is checked at the op level only"
    il = _model_grads(dev, seed, x, mask, bf16, True)
    if not bf16:
        diff = [k for k in w1 if not torch.equal(w1[k], il[k])]
        assert not diff, f"window and in-line route differ in {diff[:4]} ({len(diff)} tensors)"
        return
    worst = (0.0, None)
    for k in w1:
        r = ref[k].reshape(w1[k].shape)
        ew, ei = float((w1[k].double() - r).abs().max()), float((il[k].double() - r).abs().max())
        floor = 1e-6 * float(r.abs().max())
        print(f"{k}: max |err| vs float64: window {ew:.3e}, in line {ei:.3e}")
        assert ew <= 1.25 * ei + floor, (k, ew, ei)
        worst = max(worst, (ew / (1.25 * ei + floor), k))
    print(f"bf16 model: worst err(window) / (1.25 err(in line) + floor) = {worst[0]:.3f} at {worst[1]}")

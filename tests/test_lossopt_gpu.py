"""The detection loss and the optimiser kernels (csrc/loss_optim.hip, and k_head_bwd_loss of csrc/det_head.hip, which restates the loss
backward) against float64 on the CPU.  tests/lossopt_ref.py states the references and the cases once; tests/test_lossopt_host.py proves on the
CPU what these tests rest on (each case's property, that select_ref states the radix select's rule, that the tie rule is visible, the bounds).

Balanced BCE, through the C ABI as losses.py calls it, every case with 16-byte aligned tensors (the VEC = 4 kernels) and -- all but big -- once
more one float into a larger buffer (the VEC = 1 kernels), on ONE state and ONE histogram workspace for the whole module:

  * cls exact; lpx exactly 0 / 100 where float64 says so, elsewhere within E_lpx + 3 ulps (E_lpx: the float32 formula's own distance from
    float64, per case, measured by the host test; 3: the OpenCL bound of log, the build passes no fast-math flag).  Measured on an MI355X,
    the same aligned and one float in (a record, not a bound; every run prints its own figure): plateau 1.900, saturated 2.065, k0 2.072,
    narrow 2.027, zero 2.093, k1 1.971, wide 2.177, big 2.494 ulps against bounds of 3.50 (narrow) to 4.44 (big);
  * from the kernel's OWN lpx the selection is exact: cnt, k, prefix, need, ties, frac and inv2k equal select_ref, sum_gt to 1e-12, the loss
    to one float32 ulp, loss_out == state.loss bit for bit;
  * every pixel's gradient weight: exactly zero where the reference weight is zero, elsewhere gpred within GRAD_ULPS of grad64 with the
    reference weight -- one tie weighted 1 instead of need / ties is 10^6 bounds away;
  * k0 (run directly after the tie-heavy saturated case on the same workspace): NaN, k = 0, a zero gradient;
  * a second run gives the same bytes.

The fused head backward (ocrs_head_bwd_loss) must give gl bit-identical to ocrs_balanced_bce_bwd + ocrs_head_bwd_gl and within
GRAD_ULPS + 2 ulps of grad64 * p (1 - p).

Adam (through ocrs_models_amd.optim) one step at a time against float64 from the kernel's own previous state: tensors on and around the
2048-element chunk, steps 1, 2, 3 and 1000, plain / grad_scale = clip coefficient / capturable.  clip_grad_norm_: norm, coefficient and scaled
gradients on each chunk-edge tensor alone, on the table without its 1e4 gradients and on the whole table.
"""
import numpy as np
import pytest
import torch

from tests import lossopt_ref as R

pytestmark = pytest.mark.gpu

def dev_f32(a, dev, offset=0):
    """numpy float32 [n] -> device tensor; offset = 1: a view starting one float into a larger buffer (data_ptr() % 16 == 4)."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=dev)
    v = buf[offset:offset + a.size]
    v.copy_(torch.from_numpy(np.array(a)))
    assert v.data_ptr() % 16 == 4 * offset
    return v


def empty_f32(n, dev, offset=0):
    v = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=dev)[offset:offset + n]
    assert v.data_ptr() % 16 == 4 * offset
    return v


@pytest.fixture(scope="module")
def ws(dev):
    """ONE LossState and ONE histogram workspace for every loss call of this module: state left by one call must not reach the next."""
    from ocrs_models_amd._lib import lib

    L = lib()
    assert L.loss_state_bytes() == R.LOSS_STATE_BYTES == 96
    return {"state": torch.full((L.loss_state_bytes(),), 0xA5, dtype=torch.uint8, device=dev),
            "hist": torch.full((L.loss_hist_bytes(),), 0xA5, dtype=torch.uint8, device=dev)}


def run_loss(dev, ws, pred_np, target_np, offset):
    """forward + backward through the C ABI -> dict of CPU results"""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    P = pred_np.size
    pred, target = dev_f32(pred_np, dev, offset), dev_f32(target_np, dev, offset)
    lpx, gpred = empty_f32(P, dev, offset), empty_f32(P, dev, offset)
    cls = torch.full((P,), 7, dtype=torch.uint8, device=dev)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    gout = torch.full((1,), R.GOUT, dtype=torch.float32, device=dev)
    L.balanced_bce_fwd(ptr(pred), ptr(target), ptr(lpx), ptr(cls), ptr(ws["state"]), ptr(ws["hist"]), ptr(loss), P)
    L.balanced_bce_bwd(ptr(pred), ptr(target), ptr(lpx), ptr(cls), ptr(ws["state"]), ptr(gout), ptr(gpred), P)
    torch.cuda.synchronize()
    raw = bytes(ws["state"].cpu().numpy().tobytes())
    return {"raw": raw, "state": R.decode_loss_state(raw), "lpx": lpx.cpu().numpy(), "cls": cls.cpu().numpy(), "gpred": gpred.cpu().numpy(),
            "loss_bits": int(loss.cpu().numpy().view(np.uint32)), "dev": (pred, target, lpx, cls, gout)}


def check_loss(name, ref, out, tag):
    pred, target = ref["pred"], ref["target"]
    st = out["state"]
    # the class map and the per-pixel loss
    assert np.array_equal(out["cls"], ref["cls"])
    lpx, l64, mid = out["lpx"], ref["l64"], ref["interior"]
    assert np.array_equal(lpx[~mid].astype(np.float64), l64[~mid]), "zeros and the clamp at 100 are exact"
    worst = float(R.ulps(lpx[mid], l64[mid]).max())
    print(f"lpx {name} {tag}: {worst:.3f} float32 ulps from float64 (bound {ref['E_lpx']:.3f} + 3)")
    assert worst <= ref["E_lpx"] + 3.0
    # the selection, from the kernel's own lpx
    sel = R.select_ref(lpx, out["cls"])
    assert st["cnt"] == sel["cnt"] and st["k"] == sel["k"]
    assert out["loss_bits"] == st["loss_bits"], "loss_out is state.loss"
    if sel["k"] == 0:
        assert np.isnan(st["loss"])
        assert st["need"] == [0, 0] and st["ties"] == [0, 0] and st["frac"] == [0.0, 0.0] and st["inv2k"] == 0.0, "state of an earlier call"
        assert not out["gpred"].any(), "k == 0: a zero gradient (-0 allowed)"
        return
    assert st["prefix"] == sel["prefix"] and st["need"] == sel["need"] and st["ties"] == sel["ties"]
    assert [np.float32(f) for f in st["frac"]] == [np.float32(n / t) for n, t in zip(sel["need"], sel["ties"])]
    assert np.float32(st["inv2k"]) == np.float32(1.0 / (2.0 * sel["k"]))
    for c in range(2):
        assert abs(st["sum_gt"][c] - sel["sum_gt"][c]) <= 1e-12 * abs(sel["sum_gt"][c]), (c, st["sum_gt"], sel["sum_gt"])
    want = float(np.float32(sel["loss"]))
    assert abs(st["loss"] - want) <= float(np.spacing(np.float32(abs(want)))), (st["loss"], sel["loss"])
    # the weight of every pixel
    g = out["gpred"].astype(np.float64)
    w = sel["weight"]
    assert not g[w == 0].any(), "a pixel below the threshold (or of class 0) received a gradient"
    g64 = R.grad64(pred, target, w, sel["k"])
    g1 = R.grad64(pred, target, np.ones_like(w), sel["k"])
    err = np.abs(g - g64) / R.ulp32(g64)
    i = int(err.argmax())
    assert err[i] <= R.GRAD_ULPS, (f"pixel {i}: gpred {g[i]!r}, reference {g64[i]!r} ({err[i]:.1f} ulps); recovered weight "
                                   f"{g[i] / g1[i] if g1[i] else 0.0!r}, reference weight {w[i]!r}")
    print(f"gpred {name} {tag}: {float(err.max()):.2f} float32 ulps from grad64")


LOSS_RUNS = [(n, o) for n in R.LOSS_CASES for o in (0, 1) if not (n == "big" and o == 1)]


@pytest.mark.parametrize("name,offset", LOSS_RUNS, ids=[f"{n}-{'vec4' if o == 0 else 'vec1'}" for n, o in LOSS_RUNS])
def test_balanced_bce_exact(dev, ws, name, offset):
    ref = R.loss_reference(name)
    if name == "k0":
        # directly after a tie-heavy call on the same workspace: its ties, frac, need and prefix must not reach this one
        sat = R.loss_reference("saturated")
        prev = run_loss(dev, ws, sat["pred"], sat["target"], offset)
        assert prev["state"]["ties"][1] > prev["state"]["need"][1] > 0
    out = run_loss(dev, ws, ref["pred"], ref["target"], offset)
    check_loss(name, ref, out, "vec4" if offset == 0 else "vec1")
    again = run_loss(dev, ws, ref["pred"], ref["target"], offset)
    assert again["raw"] == out["raw"], "the state of a second run differs"
    assert np.array_equal(again["lpx"].view(np.uint32), out["lpx"].view(np.uint32))
    assert np.array_equal(again["gpred"].view(np.uint32), out["gpred"].view(np.uint32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", R.HEAD_CASES)
def test_fused_head_backward_restates_the_loss_backward(dev, ws, name, dtype):
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    ref = R.loss_reference(name, True)
    P = ref["pred"].size
    assert P % 4 == 0
    out = run_loss(dev, ws, ref["pred"], ref["target"], 0)
    pred, target, lpx, cls, gout = out["dev"]
    g = torch.Generator().manual_seed(31 + P)
    z = torch.randn(P, 8, generator=g).to(dev).to(dtype)
    tr = torch.zeros(3, 8)  # the load transform of the block in front of the head: x~ = max(z * scale + shift, lo)
    tr[0] = 1.0 + 0.3 * torch.randn(8, generator=g)
    tr[0, ::5] *= -1
    tr[1] = 0.2 * torch.randn(8, generator=g)
    tr = tr.to(dev)
    w = torch.randn(8, generator=g).to(dev)
    saved = torch.stack([0.1 * torch.randn(8, generator=g), 1 + 0.2 * torch.rand(8, generator=g)]).to(dev)
    dt = 1 if dtype == torch.bfloat16 else 0
    res = []
    for fused in (False, True):
        gl = torch.full((P,), float("nan"), device=dev)
        acc = torch.zeros(9, dtype=torch.float64, device=dev)
        gsum = torch.zeros(16, dtype=torch.float64, device=dev)
        if fused:
            L.head_bwd_loss(ptr(z), ptr(tr), ptr(w), ptr(pred), ptr(target), ptr(lpx), ptr(cls), ptr(ws["state"]), ptr(gout), ptr(gl), ptr(acc),
                            ptr(saved), ptr(gsum), P, dt)
        else:
            gpred = torch.empty(P, device=dev)
            L.balanced_bce_bwd(ptr(pred), ptr(target), ptr(lpx), ptr(cls), ptr(ws["state"]), ptr(gout), ptr(gpred), P)
            L.head_bwd_gl(ptr(z), ptr(tr), ptr(w), ptr(pred), ptr(gpred), ptr(gl), ptr(acc), ptr(saved), ptr(gsum), P, dt)
        torch.cuda.synchronize()
        res.append((gl.cpu(), acc.cpu(), gsum.cpu()))
    (gl_a, acc_a, gs_a), (gl_b, acc_b, gs_b) = res
    assert torch.equal(gl_a, gl_b), "k_head_bwd_loss does not restate k_bce_bwd + k_head_bwd operation for operation"
    sel = R.select_ref(out["lpx"], out["cls"])
    p = ref["pred"].astype(np.float64)
    want = R.grad64(ref["pred"], ref["target"], sel["weight"], sel["k"]) * (p * (1.0 - p))
    got = gl_b.numpy().astype(np.float64)
    assert not got[sel["weight"] == 0].any()
    err = np.abs(got - want) / R.ulp32(want)
    assert err.max() <= R.GRAD_ULPS + 2.0, (int(err.argmax()), float(err.max()))
    assert np.abs(got).max() > 0
    # acc64 (dw[8] | db) and gsum (sum ghat[8] | sum ghat * zhat[8]): float32 block sums added in another order.  Per ENTRY, relative to the sum
    # of the absolute values of what the entry adds up (an entry may cancel to far below its terms; a float32 running sum errs relative to those)
    zf, trc, wc, sv = z.float().cpu().double(), tr.cpu().double(), w.cpu().double(), saved.cpu().double()
    gl64 = gl_b.double().unsqueeze(1)
    pre = zf * trc[0] + trc[1]
    gh = torch.where(pre > 0, gl64 * wc, torch.zeros_like(pre))
    scale_acc = torch.cat([(gl64 * torch.maximum(pre, trc[2])).abs().sum(0), gl64.abs().sum(0)])
    scale_gs = torch.cat([gh.abs().sum(0), (gh * (zf - sv[0])).abs().sum(0) * sv[1].abs()])
    for a, b, scale in ((acc_a, acc_b, scale_acc), (gs_a, gs_b, scale_gs)):
        assert bool(((a - b).abs() <= 1e-6 * scale).all()), ((a - b).abs() / scale).tolist()
        assert float(a.abs().max()) > 0  # (single entries may be exactly zero: k1 has three pixels with a gradient, and x~ is clamped at 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Adam and clip_grad_norm_
# ---------------------------------------------------------------------------------------------------------------------------------------


def set_grads(ps, grads_np, dev):
    for p, g in zip(ps, grads_np):
        p.grad = torch.from_numpy(np.array(g)).to(dev)


def host(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


@pytest.mark.parametrize("variant", ["plain", "grad_scale", "capturable"])
def test_adam_steps_against_float64(dev, variant):
    import ocrs_models_amd as oa
    from ocrs_models_amd._lib import lib

    assert lib().opt_chunk() == R.OPT_CHUNK
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dev)) for a in R.opt_params()]
    opt = oa.optim.Adam(ps, lr=R.LR, betas=R.BETAS, eps=R.EPS, capturable=variant == "capturable")
    for si, step in enumerate(R.OPT_STEPS):
        grads = R.opt_grads(si)
        set_grads(ps, grads, dev)
        if si == 0:
            p0, m0, v0 = host(ps), [np.zeros_like(g) for g in grads], [np.zeros_like(g) for g in grads]
        else:
            p0, m0, v0 = host(ps), host([opt.state[p]["exp_avg"] for p in ps]), host([opt.state[p]["exp_avg_sq"] for p in ps])
        if step != si + 1:  # the far step
            for p in ps:
                opt.state[p]["step"] = step - 1
            opt._dev_step = {}  # (as load_state_dict does: the device counter restarts from the restored step)
        coef = 1.0
        if variant == "grad_scale":
            norm, coef_t = oa.optim.clip_grad_norm_(ps, R.MAX_NORM, scale_in_place=False)
            opt.grad_scale = coef_t
            coef = float(coef_t.item())
            assert coef < 1.0
        opt.step()
        torch.cuda.synchronize()
        for p, g in zip(ps, grads):
            assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), g.view(np.uint32)), "the step changed a gradient"
        assert all(opt.state[p]["step"] == step for p in ps)
        if variant == "capturable":
            assert float(opt._dev_step[0].item()) == float(step), "the device step counter must read t after step t"
        p1, m1, v1 = host(ps), host([opt.state[p]["exp_avg"] for p in ps]), host([opt.state[p]["exp_avg_sq"] for p in ps])
        for i, (name, _, _) in enumerate(R.OPT_TENSORS):
            ref = R.adam_ref64(p0[i], grads[i], m0[i], v0[i], step, coef)
            m_b, v_b, p_b = R.adam_bounds(ref)
            for what, got, want, bound in (("m", m1[i], ref["m"], m_b), ("v", v1[i], ref["v"], v_b), ("p", p1[i], ref["p"], p_b)):
                err = np.abs(got.astype(np.float64) - want) / bound
                j = int(err.argmax())
                assert err.flat[j] <= 1.0, f"{variant} step {step} {name} {what}[{j}]: {got.flat[j]!r} vs {want.flat[j]!r}, {err.flat[j]:.1f}x the bound"


@pytest.mark.parametrize("set_name", list(R.CLIP_SETS))
def test_clip_grad_norm_against_float64(dev, set_name):
    """Every gradient set of R.CLIP_SETS: each chunk-edge tensor ALONE and the table without the 1e4 gradients (in the whole table that one tensor
    is the norm, and a dropped or doubled chunk-edge element elsewhere moves it by less than the bound: the host test shows both), below and
    above max_norm."""
    import ocrs_models_amd as oa

    idx = R.CLIP_SETS[set_name]
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(R.opt_params()[i])).to(dev)) for i in idx]
    for si in range(2):
        grads = [R.opt_grads(si)[i] for i in idx]
        n64 = R.norm64(grads)
        assert n64 > 0
        # below max_norm: coef exactly 1, the gradients untouched
        set_grads(ps, grads, dev)
        norm, coef = oa.optim.clip_grad_norm_(ps, 1e9, scale_in_place=False)
        assert abs(float(norm.item()) - n64) <= R.NORM_REL * n64, (float(norm.item()), n64)
        assert float(coef.item()) == 1.0
        norm = oa.optim.clip_grad_norm_(ps, 1e9)
        assert abs(float(norm.item()) - n64) <= R.NORM_REL * n64
        for p, g in zip(ps, grads):
            assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), g.view(np.uint32))
        # above it
        max_norm = R.clip_max_norm_below(n64)
        norm, coef = oa.optim.clip_grad_norm_(ps, max_norm, scale_in_place=False)
        n32, c32 = norm.cpu().numpy().astype(np.float32), coef.cpu().numpy().astype(np.float32)[0]
        assert abs(float(n32) - n64) <= R.NORM_REL * n64, (float(n32), n64)
        want = max_norm / (float(n32) + 1e-6)
        assert want < 1.0 and abs(float(c32) - want) <= 2 * R.ulp32(want), (c32, want)
        for p, g in zip(ps, grads):
            assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), g.view(np.uint32)), "scale_in_place=False changed a gradient"
        norm2 = oa.optim.clip_grad_norm_(ps, max_norm)
        assert norm2.cpu().numpy().astype(np.float32).view(np.uint32) == n32.view(np.uint32)
        for p, g in zip(ps, grads):
            want_g = g.astype(np.float64) * float(c32)
            assert (np.abs(p.grad.cpu().numpy().astype(np.float64) - want_g) <= R.ulp32(want_g)).all()


def test_clip_grad_norm_table_follows_the_gradient_size(dev):
    """Gradients of different sizes at the SAME address, one call after the other -- what the caching allocator does with a freed gradient: the
    pointer table cached for the first must not serve the next (it did: the norm of n4096 came out as that of its first 2049 elements whenever
    the allocator happened to reuse the address)."""
    import ocrs_models_amd as oa

    g = R.opt_grads(0)[4]
    buf = torch.from_numpy(np.array(g)).to(dev)
    for n in (2048, 4096, 2049, 1):
        p = torch.nn.Parameter(torch.zeros(n, device=dev))
        p.grad = buf[:n]
        assert p.grad.data_ptr() == buf.data_ptr()
        norm = oa.optim.clip_grad_norm_([p], 1e9)
        n64 = R.norm64([g[:n]])
        assert abs(float(norm.item()) - n64) <= R.NORM_REL * n64, (n, float(norm.item()), n64)

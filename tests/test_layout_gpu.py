"""Layout model on the GPU: every new kernel against tests/layout_ref.py in float64 on the kernel's own inputs, the whole model against
the reference's goldens (tests/golden/layout.npz) and against layout_ref at the real size, dropout with the kernels' own masks, the
batch-axis quirk, the split-bf16 mode, bit-reproducibility and the train / test loops.

Bounds: exact-fp32 ops <= 5e-6 forward and <= 2e-5 gradients relative to the tensor's maximum; model outputs and loss
<= 1e-4 relative; gradients err(HIP, fp64) <= 2 * err(reference fp32, fp64) + 2e-4 per tensor."""
from __future__ import annotations

import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_ref as lr  # noqa: E402
from golden_util import GOLDEN_DIR, compare_to_golden, golden_vs_golden, load_npz  # noqa: E402

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 5e-6, 2e-5


def _dev():
    return torch.device("cuda:0")


def _oa():
    import ocrs_models_amd as oa

    return oa


def _L():
    from ocrs_models_amd._lib import lib

    return lib()


def ptr(t):
    return None if t is None else t.data_ptr()


def relmax(a, b):
    """max |a - b| relative to the comparand's maximum"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def rell2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _model(seed, p=0.0, train=True, return_probs=False):
    m = _oa().LayoutModel(return_probs=return_probs)
    m.load_state_dict(lr.fill_params(seed))
    m = m.to(_dev())
    m.dropout_p = p
    return m.train() if train else m.eval()


def _meta():
    with open(os.path.join(GOLDEN_DIR, "layout_meta.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("case", list(lr.CASES))
def test_embedding(case):
    c = lr.CASES[case]
    boxes, _ = lr.make_inputs(c["N"], c["W"], c["seed"])
    from ocrs_models_amd.layout import _rates

    out = torch.empty(c["N"] * c["W"], 256, device=_dev())
    bd = boxes.to(_dev())
    _L().layout_embed(ptr(bd), ptr(_rates(_dev())), ptr(out), c["N"] * c["W"])
    ref = lr.embed64(boxes).reshape(-1, 256)
    diff = (out.cpu().double() - ref).abs()
    err, at = float(diff.max()), int(diff.argmax())
    print(f"embedding {case}: max abs err {err:.3e} at row {at // 256} column {at % 256}: {float(out.reshape(-1)[at]):.7f} vs {float(ref.reshape(-1)[at]):.7f}, "
          f"box {boxes.reshape(-1, 4)[at // 256].tolist()}")
    assert err <= 1e-6


def _attn_masks(S, W, p, seed, site):
    from ocrs_models_amd.layout import dropout_mask

    return dropout_mask((W * 4, S, S), p, seed, site // 4, site % 4).cpu()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("W", [1, 7, 500])
@pytest.mark.parametrize("S", [1, 2, 5, 16, 63, 64, 65, 128])
def test_attention(S, W, p):
    g = torch.Generator().manual_seed(1000 * S + W)
    qkv = torch.randn(S, W, 768, generator=g)
    dout = torch.randn(S, W, 256, generator=g)
    seed, site = 123456789 + S, 9
    d = _dev()
    out = torch.full((S, W, 256), float("nan"), device=d)
    dqkv = torch.full((S, W, 768), float("nan"), device=d)
    qd, dd = qkv.to(d), dout.to(d)
    _L().layout_attn_fwd(ptr(qd), ptr(out), S, W, p, seed, site)
    _L().layout_attn_bwd(ptr(qd), ptr(dd), ptr(dqkv), S, W, p, seed, site)
    mask = _attn_masks(S, W, p, seed, site) if p > 0 else None
    q64 = qkv.double().requires_grad_(True)
    ref = lr.attention(q64[..., :256], q64[..., 256:512], q64[..., 512:], mask, p)
    (gref,) = torch.autograd.grad(ref, q64, dout.double())
    e_f = relmax(out, ref)
    e_b = [relmax(dqkv[..., i * 256:(i + 1) * 256], gref[..., i * 256:(i + 1) * 256]) for i in range(3)]
    print(f"attention S={S} W={W} p={p}: fwd {e_f:.2e} dq/dk/dv {e_b[0]:.2e} {e_b[1]:.2e} {e_b[2]:.2e}")
    assert e_f <= FWD_TOL
    assert max(e_b) <= GRAD_TOL


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1, 7, 800, 32000])
def test_residual_dropout_layernorm(rows, p):
    from ocrs_models_amd.layout import dropout_mask

    g = torch.Generator().manual_seed(rows)
    x, a, dy1, dy2 = (torch.randn(rows, 256, generator=g) for _ in range(4))
    x = x * 2 + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    d, L = _dev(), _L()
    seed, site = 42, 7
    xd, ad, gd, bd, d1, d2 = (t.to(d) for t in (x, a, gamma, beta, dy1, dy2))
    y, stat = torch.empty(rows, 256, device=d), torch.empty(rows, 2, device=d)
    L.layout_ln_fwd(ptr(xd), ptr(ad), ptr(gd), ptr(bd), ptr(y), ptr(stat), rows, 1e-5, p, seed, site)
    ds, da = torch.empty(rows, 256, device=d), (torch.empty(rows, 256, device=d) if p > 0 else None)
    dg, db = torch.empty(256, device=d), torch.empty(256, device=d)
    ws = torch.empty(L.layout_ln_bwd_ws_floats(rows), device=d)
    L.layout_ln_bwd(ptr(d1), ptr(d2), ptr(xd), ptr(ad), ptr(stat), ptr(gd), ptr(ds), ptr(da), ptr(dg), ptr(db), ptr(ws), rows, p, seed, site)
    x64, a64, g64, b64 = (t.double().requires_grad_(True) for t in (x, a, gamma, beta))
    m = dropout_mask((rows, 256), p, seed, site // 4, site % 4).cpu().double() / (1 - p) if p > 0 else 1.0
    ref = lr.layer_norm(x64 + a64 * m, g64, b64)
    rx, ra, rg, rb = torch.autograd.grad(ref, (x64, a64, g64, b64), (dy1 + dy2).double())
    errs = dict(y=relmax(y, ref), dx=relmax(ds, rx), da=relmax(da if p > 0 else ds, ra), dgamma=relmax(dg, rg), dbeta=relmax(db, rb))
    print(f"res+drop+LN rows={rows} p={p}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["y"] <= FWD_TOL
    assert max(errs["dx"], errs["da"], errs["dgamma"], errs["dbeta"]) <= GRAD_TOL


def _loss_case(kind, rows):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows // 50 or 1, 50 if rows >= 50 else rows, 2, generator=g) * 3
    t = (torch.rand(x.shape, generator=g) < 0.08).float()
    if kind == "all_negative":
        x = -x.abs() - 0.1
    elif kind == "saturated":
        x = torch.where(torch.rand(x.shape, generator=g) < 0.5, 80.0, -80.0)
    return x, t


@pytest.mark.parametrize("kind", ["random", "all_negative", "saturated"])
@pytest.mark.parametrize("rows", [7, 800, 32000])
def test_loss_head(kind, rows):
    x, t = _loss_case(kind, rows)
    tl = _oa().train_layout
    d = _dev()
    counts = torch.zeros(6, dtype=torch.int64, device=d)
    xd = x.to(d).requires_grad_(True)
    loss = tl.weighted_loss()(xd, t.to(d), counts)
    loss.backward()
    x64 = x.double().requires_grad_(True)
    ref = lr.weighted_loss(x64, t.double())
    (gref,) = torch.autograd.grad(ref, x64)
    e_l, e_g = abs(loss.item() - ref.item()) / abs(ref.item()), relmax(xd.grad, gref)
    print(f"loss {kind} rows={x.shape[0] * x.shape[1]}: loss {e_l:.2e} dlogits {e_g:.2e} counts {counts.tolist()}")
    assert e_l <= FWD_TOL and e_g <= GRAD_TOL
    want = lr.counts(torch.sigmoid(x), t)
    assert counts.tolist() == want
    stats = tl.LayoutAccuracyStats()
    stats.update_counts(counts)
    got, exp = list(stats.stats_dict().values()), lr.ratios(want)
    for a, b in zip(got, exp):
        assert (math.isnan(a) and math.isnan(b)) or a == b, (got, exp)
    if kind == "all_negative":
        assert math.isnan(got[0]) and math.isnan(got[2])  # 0 / 0 precision, as the reference


# ---------------------------------------------------------------------------------------------------------------------- model level
def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _step(m, boxes, target, opt=None):
    tl = _oa().train_layout
    if opt is not None:
        opt.zero_grad()
    else:
        m.zero_grad()
    pred = m(boxes)
    loss = tl.weighted_loss()(pred, target)
    loss.backward()
    if opt is not None:
        opt.step()
    return pred.detach(), loss.detach()


@pytest.mark.parametrize("case", list(lr.CASES))
def test_model_against_goldens(case):
    c, G = lr.CASES[case], load_npz("layout.npz")
    boxes, target = lr.make_inputs(c["N"], c["W"], c["seed"])
    bd, td = boxes.to(_dev()), target.to(_dev())
    with torch.no_grad():
        pe = _model(c["seed"], train=False)(bd)
    e = compare_to_golden(G, f"{case}/f64/pred", pe, 0)
    print(f"{case} eval forward rel {e:.2e}")
    assert e <= 1e-4
    m = _model(c["seed"], p=0.0)
    opt = _oa().optim.Adam(m.parameters(), lr=3e-4)
    for step in range(3):
        pred, loss = _step(m, bd, td, opt)
        if step == 0:
            e = compare_to_golden(G, f"{case}/f64/pred", pred, 0)
            el = abs(loss.item() - float(G[f"{case}/f64/loss"])) / abs(float(G[f"{case}/f64/loss"]))
            print(f"{case} train forward rel {e:.2e} loss rel {el:.2e}")
            assert e <= 1e-4 and el <= 1e-4
            worst = 0.0
            for k, g in _grads(m).items():
                eh = compare_to_golden(G, f"{case}/f64/grad/{k}", g, 0)
                er = golden_vs_golden(G, f"{case}/f32/grad/{k}", f"{case}/f64/grad/{k}")
                worst = max(worst, eh)
                assert eh <= 2 * er + 2e-4, (k, eh, er)
            print(f"{case} worst gradient rel err vs fp64 {worst:.2e}")
        if step in (0, 2):
            worst, GS = 0.0, load_npz("layout_state.npz")
            for k, v in m.state_dict().items():
                # the oracle tests' bound for parameters after Adam steps (tests/test_oracle_golden.py, 2e-4): an Adam update is
                # lr * m / (sqrt(v) + eps), sign-like where |g| ~ eps, so fp32 rounding of such a gradient moves the element by up to lr
                e = compare_to_golden(GS, f"{case}/f32/state{step + 1}/{k}", v, 0)
                worst = max(worst, e)
                assert e <= 2e-4, (k, step, e)
            print(f"{case} parameters after {step + 1} Adam step(s): worst rel {worst:.2e}")


def test_model_full_size():
    N, W, seed = 64, 500, 41
    boxes, target = lr.make_inputs(N, W, seed)
    m = _model(seed, p=0.0)
    pred, loss = _step(m, boxes.to(_dev()), target.to(_dev()))
    P = {k: v.requires_grad_(True) for k, v in lr.fill_params(seed, torch.float64).items()}
    ref = lr.forward(P, boxes)
    rl = lr.weighted_loss(ref, target.double())
    gref = torch.autograd.grad(rl, list(P.values()))
    e, el = rell2(pred, ref), abs(loss.item() - rl.item()) / abs(rl.item())
    print(f"full size forward rel {e:.2e} loss rel {el:.2e}")
    assert e <= 1e-4 and el <= 1e-4
    worst = max(rell2(g, r) for g, r in zip(_grads(m).values(), gref))
    print(f"full size worst gradient rel {worst:.2e}")
    assert worst <= 2e-4


def _all_masks(N, W, p, seed):
    from ocrs_models_amd.layout import dropout_mask

    R, out = N * W, {}
    for i in range(lr.LAYERS):
        for site, shape in ((0, (W * 4, N, N)), (1, (R, 256)), (2, (R, 1024)), (3, (R, 256))):
            out[(i, site)] = dropout_mask(shape, p, seed, i, site).cpu()
    return out


def test_dropout_on():
    c = lr.CASES["lay1"]
    N, W, p = c["N"], c["W"], 0.1
    boxes, target = lr.make_inputs(N, W, c["seed"])
    bd, td = boxes.to(_dev()), target.to(_dev())
    m = _model(c["seed"], p=p)
    torch.manual_seed(5)
    pred, loss = _step(m, bd, td)
    grads, seed = _grads(m), m.last_seed
    masks = _all_masks(N, W, p, seed)
    P = {k: v.requires_grad_(True) for k, v in lr.fill_params(c["seed"], torch.float64).items()}
    ref = lr.forward(P, boxes, masks, p)
    rl = lr.weighted_loss(ref, target.double())
    gref = torch.autograd.grad(rl, list(P.values()))
    e, el = rell2(pred, ref), abs(loss.item() - rl.item()) / abs(rl.item())
    worst = max(rell2(g, r) for g, r in zip(grads.values(), gref))
    print(f"dropout on: forward rel {e:.2e} loss rel {el:.2e} worst gradient rel {worst:.2e}")
    assert e <= 1e-4 and el <= 1e-4 and worst <= 2e-4
    for key, mk in masks.items():  # keep rate within 4 standard deviations of 0.9
        n = mk.numel()
        rate = float(mk.double().mean())
        assert abs(rate - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), (key, rate, n)
    assert not torch.equal(masks[(0, 1)], masks[(0, 3)]) and not torch.equal(masks[(0, 1)], masks[(1, 1)])
    assert not torch.equal(masks[(0, 1)], _all_masks(N, W, p, seed + 1)[(0, 1)])
    torch.manual_seed(5)
    pred2, loss2 = _step(m, bd, td)  # same seed -> the same step, bit for bit
    assert m.last_seed == seed and torch.equal(pred, pred2) and torch.equal(loss, loss2)
    for k, g in _grads(m).items():
        assert torch.equal(g, grads[k]), k
    torch.manual_seed(6)
    pred3, _ = _step(m, bd, td)
    assert not torch.equal(pred, pred3)


def test_batch_axis_quirk():
    c = lr.CASES["lay3"]
    boxes, _ = lr.make_inputs(c["N"], c["W"], c["seed"])
    m = _model(c["seed"], train=False)
    with torch.no_grad():
        y0 = m(boxes.to(_dev()))
        b2 = boxes.clone()
        b2[0, 0] += 37.0
        y1 = m(b2.to(_dev()))
    diff = (y0 != y1).any(-1).cpu()  # (N, W)
    assert diff[:, 0].all(), "the word with the same index on the other pages must change"
    assert not diff[:, 1:].any(), "no other word may change, bit for bit"


def test_autocast_x3():
    case = "lay1"
    c, G = lr.CASES[case], load_npz("layout.npz")
    boxes, target = lr.make_inputs(c["N"], c["W"], c["seed"])
    m = _model(c["seed"], p=0.0)
    m.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = m(boxes.to(_dev()))
    loss = _oa().train_layout.weighted_loss()(pred, target.to(_dev()))
    loss.backward()
    ratios = {}
    for key, t in [("pred", pred)] + [(f"grad/{k}", g) for k, g in _grads(m).items()]:
        mine = compare_to_golden(G, f"{case}/f32/{key}", t, 0)
        refd = golden_vs_golden(G, f"{case}/bf16/{key}", f"{case}/f32/{key}")
        ratios[key] = mine / refd
    worst = max(ratios, key=ratios.get)
    print(f"x3 mode: worst distance ratio {ratios[worst]:.4f} ({worst}); predictions {ratios['pred']:.4f}")
    assert ratios[worst] <= 0.05, (worst, ratios[worst])


def test_reproducible():
    c = lr.CASES["lay1"]
    boxes, target = lr.make_inputs(c["N"], c["W"], c["seed"])
    bd, td = boxes.to(_dev()), target.to(_dev())
    runs = []
    for _ in range(2):
        m = _model(c["seed"], p=0.1)
        torch.manual_seed(11)
        pred, loss = _step(m, bd, td)
        runs.append((pred, loss, _grads(m)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_train_and_test_loops():
    c = lr.CASES["lay1"]
    tl = _oa().train_layout
    batches = [lr.make_inputs(c["N"], c["W"], 80 + i) for i in range(3)]  # (seeds whose comparand probabilities all stay > 1e-4 away from 0.5)
    m = _model(c["seed"], p=0.0)
    opt = tl.make_optimizer(m)
    P = lr.fill_params(c["seed"], torch.float64)
    # comparand: the same loops on layout_ref (Adam re-stated in layout_ref.adam_steps' arithmetic, one update per batch)
    P = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    mom = {k: torch.zeros_like(v) for k, v in P.items()}
    sq = {k: torch.zeros_like(v) for k, v in P.items()}
    t = 0
    for epoch in range(2):
        mean_loss, stats = tl.train(epoch, _dev(), batches, m, opt)
        assert isinstance(stats._sums, torch.Tensor) and stats._sums.is_cuda
        ref_stats, tot = lr.Stats(), 0.0
        for boxes, target in batches:
            pred = lr.forward(P, boxes)
            loss = lr.weighted_loss(pred, target.double())
            grads = torch.autograd.grad(loss, list(P.values()))
            prob = torch.sigmoid(pred.detach())
            assert float((prob - 0.5).abs().min()) > 1e-5, "choose other seeds: a comparand probability lies within 1e-5 of 0.5"
            ref_stats.update(prob, target)
            tot += loss.item()
            t += 1
            with torch.no_grad():
                for (k, v), g in zip(P.items(), grads):
                    mom[k].mul_(0.9).add_(g, alpha=0.1)
                    sq[k].mul_(0.999).addcmul_(g, g, value=0.001)
                    v.addcdiv_(mom[k], (sq[k].sqrt() / math.sqrt(1 - 0.999**t)).add_(1e-8), value=-3e-4 / (1 - 0.9**t))
        e = abs(mean_loss - tot / 3) / abs(tot / 3)
        print(f"train() epoch {epoch}: mean loss rel {e:.2e}; {stats.summary()}")
        assert e <= 1e-4
        got, exp = list(stats.stats_dict().values()), ref_stats.means()
        for a, b in zip(got, exp):
            assert (math.isnan(a) and math.isnan(b)) or a == b, (got, exp)
    val_loss, vstats = tl.test(_dev(), batches, m)
    ref_stats, tot = lr.Stats(), 0.0
    with torch.no_grad():
        for boxes, target in batches:
            prob = torch.sigmoid(lr.forward(P, boxes))
            assert float((prob - 0.5).abs().min()) > 1e-5
            tot += lr.weighted_loss(prob, target.double()).item()  # (the logits loss on probabilities, as the reference's test())
            ref_stats.update(prob, target)
    e = abs(val_loss - tot / 3) / abs(tot / 3)
    print(f"test(): mean loss rel {e:.2e}; {vstats.summary()}")
    assert e <= 1e-4
    for a, b in zip(vstats.stats_dict().values(), ref_stats.means()):
        assert (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("case", list(lr.CASES))
def test_aten_graph_matches_hip(case):
    c = lr.CASES[case]
    boxes, _ = lr.make_inputs(c["N"], c["W"], c["seed"])
    m = _oa().LayoutModel()
    m.load_state_dict(lr.fill_params(c["seed"]))
    with torch.no_grad():
        ya = _oa().export.AtenGraph(m.eval())(boxes)
        yh = m.to(_dev())(boxes.to(_dev()))
    e = rell2(yh, ya)
    print(f"AtenGraph vs HIP {case}: {e:.2e}")
    assert e <= 1e-4


def test_limits_and_refusals():
    oa = _oa()
    m = _model(31, train=False)
    with pytest.raises(RuntimeError, match="128"):
        m(torch.zeros(129, 3, 4, device=_dev()))
    m.train()
    m.dropout_p = 0.1
    with pytest.raises(RuntimeError, match="dropout"):
        oa.graph.GraphedTrainStep(m, oa.optim.Adam(m.parameters(), capturable=True), oa.train_layout.weighted_loss(),
                                  torch.zeros(2, 3, 4, device=_dev()), torch.zeros(2, 3, 2, device=_dev()))
    mp = _model(31, train=False, return_probs=True)
    boxes, _ = lr.make_inputs(5, 33, 33)
    with torch.no_grad():
        assert rell2(mp(boxes.to(_dev())), torch.sigmoid(m.eval()(boxes.to(_dev())))) <= 1e-6

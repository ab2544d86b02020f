"""Edge cases and size-independent properties on the GPU: ragged / odd batch shapes, the full BASELINE tile size,
directional-derivative (finite difference) checks of the analytic gradients, run-to-run stability."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _det(seed, dev, dtype=None):
    import ocrs_models_amd as oa
    from oracle.params import detection_specs, make_state, state_dict_from

    specs = detection_specs()
    P, Bf = make_state(specs, seed)
    m = oa.DetectionModel(act_dtype=dtype).to(dev)
    m.load_state_dict(state_dict_from(P, Bf, specs))
    return m, P, Bf


def _rec(seed, dev):
    import ocrs_models_amd as oa
    from oracle.params import make_state, recognition_specs, state_dict_from

    specs = recognition_specs()
    P, Bf = make_state(specs, seed)
    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
    m.load_state_dict(state_dict_from(P, Bf, specs))
    return m, P, Bf


def test_detection_full_tile_1024_forward_and_loss(dev):
    """BASELINE tile size (1x1x1024x1024, fp32 parity mode) against the CPU oracle: prediction and balanced-BCE loss."""
    import ocrs_models_amd as oa
    from oracle import detection as odet
    from oracle import losses as olosses

    torch.set_num_threads(16)
    m, P, Bf = _det(41, dev)
    m.train()
    r = np.random.RandomState(41)
    x = torch.from_numpy(r.uniform(-0.5, 0.5, (1, 1, 1024, 1024)).astype(np.float32))
    mask = torch.from_numpy((r.uniform(0, 1, (1, 1, 1024, 1024)) > 0.9).astype(np.float32))
    with torch.no_grad():
        pred_o = odet.forward(P, Bf, x, True)
        loss_o = olosses.balanced_bce(pred_o, mask)
    with torch.no_grad():
        pred = m(x.to(dev))
        loss = oa.balanced_cross_entropy_loss(pred, mask.to(dev))
    assert rel(pred, pred_o) < 1e-4
    assert abs(loss.item() - loss_o.item()) < 1e-4 * abs(loss_o.item())
    sd = m.state_dict()
    for k, v in Bf.items():
        if not k.endswith("num_batches_tracked"):
            assert rel(sd[k], v) < 1e-4, k


def test_detection_directional_derivative(dev):
    """Size-independent property: (L(w + e*d) - L(w - e*d)) / 2e == <grad, d> for a random direction d (plain mean BCE on the
    prediction so the loss is smooth; fp32 parity mode, eval-mode BN would hide the batch-stat path, so train mode is used)."""
    m, _, _ = _det(43, dev)
    m.train()
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 1, 96, 128, generator=g) - 0.5).to(dev)
    t = (torch.rand(2, 1, 96, 128, generator=g) > 0.7).float().to(dev)
    # direction restricted to the last block + head: perturbing all 622k parameters of a 26-layer ReLU/max-pool/BatchNorm net crosses
    # so many kinks that the finite difference itself is off by 10-25 % (measured: -0.137 / -0.162 at eps 2e-3 / 1e-4 vs analytic
    # -0.182); the full-network gradients are checked against the oracle's autograd in test_det_model_gpu.py instead
    params = [p for k, p in m.named_parameters() if k.startswith("out_conv") or k.startswith("up.0.contract.seq.1")]

    def loss_fn():
        p = m(x)
        return -(t * torch.log(p.clamp_min(1e-6)) + (1 - t) * torch.log((1 - p).clamp_min(1e-6))).mean()

    loss = loss_fn()
    loss.backward()
    grads = [p.grad.clone() for p in params]
    d = [torch.randn(p.shape, generator=g).to(dev) * p.detach().abs().mean() for p in params]
    analytic = sum(float((gg.double() * dd.double()).sum()) for gg, dd in zip(grads, d))
    eps = 1e-3
    with torch.no_grad():
        for p, dd in zip(params, d):
            p.add_(eps * dd)
        lp = loss_fn().item()
        for p, dd in zip(params, d):
            p.sub_(2 * eps * dd)
        lm = loss_fn().item()
    numeric = (lp - lm) / (2 * eps)
    assert abs(numeric - analytic) < 0.03 * abs(analytic) + 1e-4, (numeric, analytic)


@pytest.mark.parametrize("B,W", [(1, 64), (5, 100), (17, 36), (3, 256)])
def test_recognition_odd_batches_and_widths(dev, B, W):
    """batch sizes that are not multiples of the 16-column GRU tile / 64-pixel GEMM tile, several crop widths; ragged CTC lengths,
    an empty target and a target with repeated labels."""
    import ocrs_models_amd as oa
    from oracle import ctc as octc
    from oracle import recognition as orec

    m, P, Bf = _rec(50 + B, dev)
    m.train()
    r = np.random.RandomState(B * 1000 + W)
    x = torch.from_numpy(r.uniform(-0.5, 0.5, (B, 1, 64, W)).astype(np.float32))
    T = W // 4 + 1
    il = torch.tensor([max(1, (W // 4) - (i % 3)) for i in range(B)])
    tl = torch.tensor([min(int(il[i]) // 2, i % 7) for i in range(B)])
    tg = torch.zeros(B, 64, dtype=torch.int32)
    for i in range(B):
        tg[i, : tl[i]] = torch.from_numpy(r.randint(1, 97, size=int(tl[i])).astype(np.int32))
        if tl[i] >= 2 and 2 * int(tl[i]) <= int(il[i]):
            tg[i, 1] = tg[i, 0]
    lp = m(x.to(dev))
    assert lp.shape == (T, B, 97)
    loss = oa.CTCLoss()(lp, tg.to(dev), il, tl)
    loss.backward()
    lp_o = orec.forward(P, Bf, x, True)
    loss_o = octc.ctc_loss_torch(lp_o, tg, il.tolist(), tl.tolist())
    grads_o = torch.autograd.grad(loss_o, list(P.values()))
    assert rel(lp, lp_o) < 1e-4
    assert abs(loss.item() - loss_o.item()) < 1e-4 * abs(loss_o.item()) + 1e-6
    errs = [rel(p.grad, go) for (k, p), go in zip(m.named_parameters(), grads_o)]
    assert max(errs) < 5e-3 and float(np.median(errs)) < 2e-4, (max(errs), float(np.median(errs)))
    dec, amax = oa.text.greedy_decode_batch(lp.detach(), il.tolist())
    assert torch.equal(amax.cpu().long(), lp_o.detach().argmax(-1).T)


def test_detection_odd_batch_bf16_runs_and_is_stable(dev):
    """bf16 throughput mode, batch 3, non-square odd size: two identical runs agree BIT FOR BIT (prediction, loss, every gradient), no NaN."""
    import ocrs_models_amd as oa

    m, _, _ = _det(47, dev, torch.bfloat16)
    m.train()
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(3, 1, 200, 152, generator=g) - 0.5).to(dev)
    t = (torch.rand(3, 1, 200, 152, generator=g) > 0.9).float().to(dev)
    outs = []
    for _ in range(2):
        m.zero_grad()
        import copy
        sd = copy.deepcopy(m.state_dict())
        pred = m(x)
        loss = oa.balanced_cross_entropy_loss(pred, t)
        loss.backward()
        outs.append((pred.detach().clone(), loss.item(), [p.grad.clone() for p in m.parameters()]))
        m.load_state_dict(sd)  # undo the running-stat update
    assert torch.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1])
    # Two identical runs are bit-identical: the statistics and every weight-gradient flush are fixed-order sums (per-wave LDS slots, per-block
    # partials reduced by a single writer per element); the remaining cross-block accumulations are fp64 sums of fp32 partials, which are
    # exact -- hence order-independent -- for partials of comparable magnitude ("Reproducibility")
    assert torch.equal(outs[1][0], outs[0][0])
    assert outs[1][1] == outs[0][1]
    for a, b in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (3, 65, 127), (2, 200, 72), (1, 129, 513)])
def test_awkward_shapes_two_train_steps_fp32_vs_bf16(B, H, W):
    """Minimum size (deepest level 1x1), odd sizes (floor pooling + ConvTranspose crops at every level), extreme aspect ratios: two full
    train steps in both storage modes give finite predictions / gradients, and the bf16 loss stays within 5 % of the fp32 one
    (measured 1e-4; the tile / halo / prefetch logic of every kernel sees partial tiles here)."""
    import ocrs_models_amd as oa

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 1000 + H + W)
    x = (torch.rand(B, 1, H, W, generator=g) - 0.5).to(dev)
    m = (torch.rand(B, 1, H, W, generator=g) > 0.9).float().to(dev)
    losses = []
    for dt in (torch.float32, torch.bfloat16):
        torch.manual_seed(1)
        net = oa.DetectionModel(act_dtype=dt).to(dev)
        opt = oa.optim.Adam(net.parameters())
        for _ in range(2):
            pred = net(x)
            loss = oa.balanced_cross_entropy_loss(pred, m)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(pred).all() and torch.isfinite(loss)
        assert all(torch.isfinite(p.grad).all().item() for p in net.parameters())
        losses.append(float(loss.detach()))
    assert abs(losses[0] - losses[1]) < 0.05 * abs(losses[0]) + 1e-3, losses


def test_rank_one_ends_of_the_network_are_bit_identical_to_the_stored_paths(dev, monkeypatch):
    """Round 5: the two single-channel ends of the U-Net travel in compact form -- the first block's output as its u plane (2 B per pixel; in_conv.seq.1's
    backward rebuilds x = round(wexp[c] * u)), out_conv's input gradient as gl = dL/dlogit (4 B per pixel; the last block's backward forms round(gl * w[c]))
    -- and the first block's backward rebuilds z from its recomputed depthwise output.  With the switches off the 16-byte-per-pixel tensors are
    read instead: prediction, loss and EVERY parameter gradient of a bf16 train step must be identical bit for bit (sizes with whole and with cut
    strips / row blocks)."""
    import copy

    import ocrs_models_amd as oa
    from ocrs_models_amd.models import _DetRun

    for (B, H, W) in [(2, 128, 192), (1, 66, 64)]:
        m, _, _ = _det(48, dev, torch.bfloat16)
        m.train()
        g = torch.Generator().manual_seed(3)
        x = (torch.rand(B, 1, H, W, generator=g) - 0.5).to(dev)
        t = (torch.rand(B, 1, H, W, generator=g) > 0.9).float().to(dev)
        sd = copy.deepcopy(m.state_dict())
        outs = []
        for c1u, noz, hgl, fuse in ((1, 1, 1, 0), (0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, 1)):
            # (c1_noz: the first block does not store its 8-channel output at all -- in_conv.seq.1's forward reads the u plane too;
            #  c1_fuse, the last variant: the first block's weight gradient from sums accumulated by in_conv.seq.1's backward -- see below)
            for k, v in (("c1_u", c1u), ("c1_noz", noz), ("head_gl", hgl), ("c1_fuse", fuse)):
                monkeypatch.setattr(_DetRun, k, bool(v))
            m.load_state_dict(sd)
            m.zero_grad()
            pred = m(x)
            loss = oa.balanced_cross_entropy_loss(pred, t)
            loss.backward()
            torch.cuda.synchronize()
            outs.append((pred.detach().clone(), loss.item(), {k: p.grad.clone() for k, p in m.named_parameters()}))
        for o in outs[1:-1]:
            assert torch.equal(o[0], outs[0][0]) and o[1] == outs[0][1]
            for k in o[2]:
                assert torch.equal(o[2][k], outs[0][2][k]), k
        # the fused first-block backward (k_rs_bwd<..., C1> + k_c1_bwd_fin): everything but the first block's two weight gradients is bit-identical;
        # those are formed from sums (unrounded z1 = wexp u in the two forward-only terms, fp64 combination) instead of per pixel: the depthwise
        # gradient agrees to 1e-4, the pointwise one -- analytically ~0 in front of a BatchNorm, pure rounding noise -- to 1e-4 of the depthwise norm
        o = outs[-1]
        assert torch.equal(o[0], outs[0][0]) and o[1] == outs[0][1]
        fused_keys = ("in_conv.seq.0.seq.0.weight", "in_conv.seq.0.seq.1.weight")
        for k in o[2]:
            if k not in fused_keys:
                assert torch.equal(o[2][k], outs[0][2][k]), k
        ref0 = outs[0][2][fused_keys[0]].double()
        assert float((o[2][fused_keys[0]].double() - ref0).norm() / ref0.norm()) < 1e-4
        assert float((o[2][fused_keys[1]].double() - outs[0][2][fused_keys[1]].double()).abs().max()) < 1e-4 * float(ref0.norm())

"""Layout model, host side (no GPU): tests/layout_ref.py against the reference's goldens (oracle policy of DESIGN.md section 2: fp32 <= 2e-5,
fp64 <= 1e-10, statistics and scalar helpers exact), state-dict layout, checkpoint round trip, refusals, and the exportable ATen graph."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_ref as lr  # noqa: E402
from golden_util import GOLDEN_DIR, _sample_idx, compare_to_golden, load_npz  # noqa: E402

import ocrs_models_amd as oa  # noqa: E402


def _meta():
    with open(os.path.join(GOLDEN_DIR, "layout_meta.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(lr.CASES))
def test_embedding_bit_equal(case):
    c, G = lr.CASES[case], load_npz("layout.npz")
    boxes, _ = lr.make_inputs(c["N"], c["W"], c["seed"])
    for e in (lr.embed(boxes), oa.layout.encode_bbox_positions_aten(boxes)):
        flat = e.reshape(-1).numpy()
        if f"{case}/f32/embed|full" in G.files:
            assert np.array_equal(flat, G[f"{case}/f32/embed|full"].reshape(-1))
        else:
            assert flat.size == int(G[f"{case}/f32/embed|size"])
            assert np.array_equal(flat[_sample_idx(flat.size)], G[f"{case}/f32/embed|samples"])
            assert compare_to_golden(G, f"{case}/f32/embed", e, 0) <= 1e-7
    assert torch.equal(lr.angle_rates(), oa.layout.angle_rates())


@pytest.mark.parametrize("tag,dtype,tol", [("f32", torch.float32, 2e-5), ("f64", torch.float64, 1e-10)])
@pytest.mark.parametrize("case", list(lr.CASES))
def test_layout_ref_against_goldens(case, tag, dtype, tol):
    c, G, GS = lr.CASES[case], load_npz("layout.npz"), load_npz("layout_state.npz")
    boxes, target = lr.make_inputs(c["N"], c["W"], c["seed"])
    P = {k: v.requires_grad_(True) for k, v in lr.fill_params(c["seed"], dtype).items()}
    pred = lr.forward(P, boxes)
    loss = lr.weighted_loss(pred, target.to(dtype))
    grads = torch.autograd.grad(loss, list(P.values()))
    assert compare_to_golden(G, f"{case}/{tag}/pred", pred, tol) <= tol
    gl = float(G[f"{case}/{tag}/loss"])
    assert abs(loss.item() - gl) <= tol * abs(gl)
    for k, g in zip(P, grads):
        e = compare_to_golden(G, f"{case}/{tag}/grad/{k}", g, tol)
        assert e <= tol, (k, e)
    tloss = lr.weighted_loss(torch.sigmoid(pred.detach()), target.to(dtype)).item()  # test()'s loss on probabilities
    gt = float(G[f"{case}/{tag}/test_loss"])
    assert abs(tloss - gt) <= tol * abs(gt)
    if tag == "f32":
        meta = _meta()
        prob = torch.clamp(torch.sigmoid(pred.detach()), 0.0, 1.0)
        assert float((prob - 0.5).abs().min()) > 1e-5  # (no borderline decision in these cases)
        st = lr.Stats()
        st.update(prob, target)
        for a, b in zip(st.means(), meta[f"{case}/stats"].values()):
            assert (math.isnan(a) and math.isnan(b)) or a == b
        # parameters after Adam steps: the bound the oracle tests use for them (tests/test_oracle_golden.py: 2e-4) -- a first Adam step is
        # lr * g / (|g| + eps), sign-like where |g| ~ eps = 1e-8, so fp32 rounding of such a gradient moves the parameter by up to lr
        for steps in (1, 3):
            Q = lr.adam_steps(lr.fill_params(c["seed"], dtype), boxes, target, steps)
            for k, v in Q.items():
                e = compare_to_golden(GS, f"{case}/f32/state{steps}/{k}", v, 0)
                assert e <= 2e-4, (k, steps, e)


def test_scalar_helpers_exact():
    meta, tl = _meta(), oa.train_layout
    for e, v in meta["lr_scale_for_epoch"]:
        assert tl.lr_scale_for_epoch(e) == v
    for p, r, f in meta["f1_score"]:
        assert tl.f1_score(p, r) == f
    assert all(meta["stats_no_positives_are_nan"])
    pr = tl.precision_recall(torch.tensor([True, False, True, True]), torch.tensor([True, True, False, True]))
    assert pr == (float(np.float32(2) / np.float32(3)), float(np.float32(2) / np.float32(3)))
    pr = tl.precision_recall(torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool))
    assert math.isnan(pr[0]) and math.isnan(pr[1])


def test_state_dict_layout_and_init():
    meta = _meta()
    torch.manual_seed(0)
    m = oa.LayoutModel()
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state_keys"]
    assert len(sd) == 74 and sum(p.numel() for p in m.parameters()) == meta["n_params"] == 4739074
    assert [k for k, _ in lr.param_specs()] == list(sd)
    assert m.dropout_p == 0.1 and m.return_probs is False and m.d_embed == 256
    # default initialisation scheme: the stock containers' (xavier in-projection, zero attention biases, unit LayerNorm gains)
    assert float(sd["encode.layers.0.self_attn.in_proj_bias"].abs().max()) == 0.0
    assert torch.equal(sd["encode.layers.3.norm1.weight"], torch.ones(256))
    bound = math.sqrt(6 / (768 + 256))
    assert float(sd["encode.layers.0.self_attn.in_proj_weight"].abs().max()) <= bound


def test_checkpoint_round_trip(tmp_path):
    m = oa.LayoutModel()
    m.load_state_dict(lr.fill_params(3))
    opt = torch.optim.Adam(m.parameters(), lr=3e-4)
    path = str(tmp_path / "text-layout-checkpoint.pt")
    oa.checkpoint.save_checkpoint(path, m, opt, epoch=7)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert list(raw["model_state"]) == [k for k, _ in lr.param_specs()] and raw["epoch"] == 7  # the reference's checkpoint format
    m2 = oa.LayoutModel()
    ck = oa.checkpoint.load_checkpoint(path, m2, torch.optim.Adam(m2.parameters(), lr=3e-4), torch.device("cpu"))
    assert ck["epoch"] == 7
    for (k, a), b in zip(m.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k


def test_refusals():
    m = oa.LayoutModel()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 3, 4))
    with pytest.raises(NotImplementedError, match="mlp"):
        oa.LayoutModel(pos_embedding="mlp")
    with pytest.raises(RuntimeError):
        oa.train_layout.weighted_loss()(torch.zeros(2, 3, 2), torch.zeros(2, 3, 2))
    with pytest.raises(RuntimeError, match="eval"):
        oa.export.AtenGraph(m.train())(torch.zeros(2, 3, 4))


@pytest.mark.parametrize("case", list(lr.CASES))
def test_aten_graph_equals_layout_ref(case):
    c = lr.CASES[case]
    boxes, _ = lr.make_inputs(c["N"], c["W"], c["seed"])
    m = oa.LayoutModel()
    m.load_state_dict(lr.fill_params(c["seed"]))
    with torch.no_grad():
        y = oa.export.AtenGraph(m.eval())(boxes)
        ref = lr.forward(lr.fill_params(c["seed"]), boxes)
    assert tuple(y.shape) == (c["N"], c["W"], 2)
    assert float((y - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    mp = oa.LayoutModel(return_probs=True)
    mp.load_state_dict(lr.fill_params(c["seed"]))
    with torch.no_grad():
        assert float((oa.export.AtenGraph(mp.eval())(boxes) - torch.sigmoid(ref)).abs().max()) <= 1e-5

"""What tests/test_lossopt_gpu.py rests on, proved on the CPU for every case it uses (tests/lossopt_ref.py states the cases once):

  * every loss case has the property it was built for (a plateau of ties cut by need, a threshold at the clamp, a class inside one pass-0 bin,
    a threshold at key 0, k = 1, k = 0, the 4-deep load loop and all 1024 block partials);
  * an emulation of the kernel's 11 / 10 / 10-bit radix select, histograms scanned from the top bin, lands on the same (prefix, need, ties) as
    select_ref's plain k-th-largest rule -- the reference states the kernel's rule;
  * the tie rule can be seen: weighting every tie 1 moves a pixel of plateau, saturated, k1 and big by more than 1000x the per-pixel bound;
  * the float32 emulation of the per-pixel loss lies E_lpx ulps from float64 (measured here: plateau 0.97, saturated 0.96, k0 0.93, narrow 0.50,
    zero 0.97, k1 0.99, wide 1.32, big 1.44; zeros and the clamp at 100 are exact), and the emulated gradient within GRAD_ULPS = 6 of grad64
    (measured maximum 3.09, on big);
  * a numpy-float32 emulation of k_multi_adam, with and without the fused multiply-adds hipcc contracts by default, stays inside the Adam bounds.
"""
import numpy as np
import pytest

from tests import lossopt_ref as R

# 0 < lpx64 < 100: the largest distance the float32 formula itself (correctly rounded logs) can be from float64, over all cases; two logf of
# 0.5 ulp, the log1p correction (a subtract, a divide, a subtract) and the negated sum: below 2 ulps
E_LPX_CEIL = 2.0


@pytest.mark.parametrize("name", R.LOSS_CASES)
def test_loss_case_properties(name):
    ref = R.loss_reference(name)
    pred, target, cls, sel = ref["pred"], ref["target"], ref["cls"], ref["sel"]
    P = pred.size
    key = R.keys_of(ref["l32"])
    if name == "plateau":
        assert P == 1900 and sel["cnt"] == [300, 1600] and sel["k"] == 300
        assert sel["need"] == [180, 200] and sel["ties"] == [180, 500] and sel["frac"] == [1.0, 0.4]
    elif name == "saturated":
        assert P == 2003 and P % 4 == 3
        assert (target == np.float32(1.2)).sum() == 1 and (target == np.float32(-0.3)).sum() == 1 and (cls == 0).sum() == len(range(0, P, 53))
        assert sel["prefix"][1] == int(np.float32(100.0).view(np.uint32)) and sel["ties"][1] > sel["need"][1] and sel["sum_gt"][1] == 0.0
        assert ((ref["l32"] == 100) & (cls == 1)).sum() >= 40  # the positive clamp (p = 0) is hit as well
    elif name == "narrow":
        used = R.radix_emul(ref["l32"], cls, sel["k"])[1][3]
        assert P == 5096 and used[0] == 1 and used[1] <= 16 and used[2] >= 256, used
    elif name == "zero":
        assert P == 433 and P % 4 == 1 and sel["k"] == 100
        assert sel["prefix"][0] == 0 and sel["need"][0] == sel["ties"][0] == 64
        assert (np.signbit(ref["l32"]) & (ref["l32"] == 0) & (cls == 1)).sum() == 64  # l = -0.0: its key must be 0, not 0x80000000
    elif name == "k1":
        assert P == 1001 and sel["cnt"] == [1, 1000] and sel["k"] == 1 and sel["need"][1] == 1 and sel["ties"][1] == 3
    elif name == "k0":
        assert P == 400 and sel["cnt"] == [0, 400] and sel["k"] == 0 and np.isnan(sel["loss"]) and not sel["weight"].any()
    elif name == "wide":
        assert P == 3 * 33 * 47 and sel["k"] > 0
    elif name == "big":
        assert P == R.BIG_P and P % 4 == 3 and P // 4 > 3 * 1024 * 256  # k_select_hist<4>'s 4-deep loop runs in every block
        assert (P + 3) // 4 // 256 >= 1024 and sel["k"] > 0             # 1024 blocks: k_select_scan reduces 1024 partials
        assert min(sel["ties"][1], sel["need"][1]) >= 1 and sel["ties"][1] > sel["need"][1]
    if P % 4 and name != "wide":
        # a selected pixel among the last P % 4: the tail code of the select passes cannot be dropped unnoticed
        assert sel["k"] == 0 or sel["weight"][P - P % 4:].max() > 0
    # zeros and the clamp are exact in the float32 formula; elsewhere it is E_lpx ulps from float64
    out = ~ref["interior"]
    assert np.array_equal(ref["l32"][out].astype(np.float64), ref["l64"][out])
    assert set(np.unique(ref["l64"][out])) <= {0.0, 50.0, 100.0}  # (50: target 0.5 on a saturated prediction)
    print(f"{name}: E_lpx = {ref['E_lpx']:.3f} float32 ulps")
    assert ref["E_lpx"] <= E_LPX_CEIL
    assert key.max() < 0x7F800000  # every loss is finite


@pytest.mark.parametrize("name,head", [(n, False) for n in R.LOSS_CASES] + [(n, True) for n in R.HEAD_CASES])
def test_radix_select_is_the_kth_largest(name, head):
    ref = R.loss_reference(name, head)
    sel = ref["sel"]
    if sel["k"] == 0:
        return
    for c, (prefix, need, ties, _) in enumerate(R.radix_emul(ref["l32"], ref["cls"], sel["k"])):
        assert (prefix, need, ties) == (sel["prefix"][c], sel["need"][c], sel["ties"][c]), (name, c)
    # the loss equals the mean of the 2k largest values, whatever subset of the ties is taken
    l, tot = ref["l32"].astype(np.float64), 0.0
    for c in (1, 2):
        tot += np.sort(l[ref["cls"] == c])[-sel["k"]:].sum()
    assert abs(sel["loss"] - tot / (2 * sel["k"])) <= 1e-12 * abs(sel["loss"])


def test_head_cases_keep_their_property():
    for name in R.HEAD_CASES:
        ref, full = R.loss_reference(name, True), R.loss_reference(name)
        assert ref["pred"].size % 4 == 0 and ref["sel"]["k"] > 0
        assert ref["sel"]["ties"][1] > ref["sel"]["need"][1], name  # still a fractional tie weight in the negative class
        assert ref["sel"]["k"] == full["sel"]["k"] or name == "saturated"


@pytest.mark.parametrize("name", R.LOSS_CASES)
def test_gradient_emulation_and_tie_rule(name):
    ref = R.loss_reference(name)
    sel = ref["sel"]
    g64 = R.grad64(ref["pred"], ref["target"], sel["weight"], sel["k"])
    g32 = R.grad32_emul(ref["pred"], ref["target"], ref["l32"], ref["cls"], sel)
    if sel["k"] == 0:
        assert not g64.any() and not g32.any()
        return
    assert np.array_equal(g32 == 0, g64 == 0)
    worst = float(R.ulps(g32, g64).max())
    print(f"{name}: emulated gradient within {worst:.2f} float32 ulps of grad64")
    assert worst <= R.GRAD_ULPS
    # every tie weighted 1 (frac applied as 1, or the oracle's "take them all")
    w1, key = sel["weight"].copy(), R.keys_of(ref["l32"])
    for c in (1, 2):
        w1[(ref["cls"] == c) & (key == sel["prefix"][c - 1])] = 1.0
    moved = float((np.abs(R.grad64(ref["pred"], ref["target"], w1, sel["k"]) - g64) / (R.GRAD_ULPS * R.ulp32(g64))).max())
    if name in R.TIE_CASES:
        assert moved > 1000.0, (name, moved)


def test_loss_state_layout():
    import struct

    assert struct.calcsize(R.LOSS_STATE_FMT) == R.LOSS_STATE_BYTES == 96
    raw = struct.pack(R.LOSS_STATE_FMT, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0)
    for field, off, fmt, want in (("cnt", 0, "<2Q", (1, 2)), ("k", 16, "<Q", (3,)), ("prefix", 24, "<2I", (4, 5)), ("need", 32, "<2Q", (6, 7)),
                                  ("ties", 48, "<2Q", (8, 9)), ("sum_gt", 64, "<2d", (10.0, 11.0)), ("loss", 80, "<f", (12.0,)),
                                  ("frac", 84, "<2f", (13.0, 14.0)), ("inv2k", 92, "<f", (15.0,))):
        assert R.LOSS_STATE_OFFSETS[field] == off and struct.unpack_from(fmt, raw, off) == want, field
    d = R.decode_loss_state(raw)
    assert d["cnt"] == [1, 2] and d["k"] == 3 and d["prefix"] == [4, 5] and d["need"] == [6, 7] and d["ties"] == [8, 9]
    assert d["sum_gt"] == [10.0, 11.0] and d["loss"] == 12.0 and d["frac"] == [13.0, 14.0] and d["inv2k"] == 15.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------------


def test_opt_table_covers_the_chunk_edges():
    sizes = [int(np.prod(s)) for _, s, _ in R.OPT_TENSORS]
    for n in (1, R.OPT_CHUNK - 1, R.OPT_CHUNK, R.OPT_CHUNK + 1, 2 * R.OPT_CHUNK, 2 * R.OPT_CHUNK + 1, 5 * R.OPT_CHUNK + 1, 165):
        assert n in sizes
    g = R.opt_grads(0)
    kinds = [k for _, _, k in R.OPT_TENSORS]
    assert not g[kinds.index("zero")].any() and np.abs(g[kinds.index("1e4")]).min() >= 5e3
    # the clip cases of the GPU test: below a huge max_norm, far above MAX_NORM
    assert R.norm64(g) > 10 * R.MAX_NORM


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "contracted"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "grad_scale"])
def test_adam_emulation_stays_inside_the_bounds(scaled, fused):
    ps = [a.copy() for a in R.opt_params()]
    ms, vs = [np.zeros_like(a) for a in ps], [np.zeros_like(a) for a in ps]
    m_in_own_ulps = 0.0
    for si, step in enumerate(R.OPT_STEPS):
        gs = R.opt_grads(si)
        coef = np.float32(min(1.0, R.MAX_NORM / (R.norm64(gs) + 1e-6))) if scaled else None
        for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
            pn, mn, vn = R.adam32_emul(p, g, m, v, step, coef, fused)
            ref = R.adam_ref64(p, g, m, v, step, 1.0 if coef is None else float(coef))
            m_b, v_b, p_b = R.adam_bounds(ref)
            assert (np.abs(mn - ref["m"]) <= m_b).all(), (step, R.OPT_TENSORS[i][0])
            assert (np.abs(vn - ref["v"]) <= v_b).all(), (step, R.OPT_TENSORS[i][0])
            assert (np.abs(pn - ref["p"]) <= p_b).all(), (step, R.OPT_TENSORS[i][0])
            m_in_own_ulps = max(m_in_own_ulps, float(R.ulps(mn, ref["m"]).max()))
            ps[i], ms[i], vs[i] = pn, mn, vn
    # why m is bounded in ulps of the lerp's largest term: in ulps of m' itself the emulation is hundreds off wherever the lerp cancels
    assert m_in_own_ulps > 20 * R.M_ULPS


def test_clip_sets_see_the_chunk_edges():
    """What the norm bound of the GPU test can see.  In the whole table it cannot see a chunk-edge element, a whole chunk, or (first gradient set) any
    tensor but the 1e4 one; taken alone, every tensor's last element, its first element past a chunk (summed twice by a chunk loop running one
    too far) and each of its chunks move the norm by more than NORM_REL."""
    names = [n for n, _, _ in R.OPT_TENSORS]
    for si in range(2):
        grads = R.opt_grads(si)
        full = R.norm64(grads)

        def moved(idx, i, keep, twice=None):
            """relative change of the set's norm when tensor i keeps only the mask `keep` (or counts element `twice` twice)"""
            gs = [grads[j].reshape(-1) for j in idx]
            n0 = R.norm64(gs)
            g = gs[idx.index(i)]
            gs[idx.index(i)] = np.concatenate([g, g[twice:twice + 1]]) if twice is not None else g[keep]
            return abs(R.norm64(gs) - n0) / n0

        table, no1e4 = R.CLIP_SETS["table"], R.CLIP_SETS["no_1e4"]
        i2049, i10241 = names.index("n2049"), names.index("n10241")
        last = lambda n: np.arange(n) < n - 1  # noqa: E731
        # the whole table is blind to these
        assert moved(table, i2049, last(2049)) < R.NORM_REL
        assert moved(table, i10241, np.arange(10241) >= 2048) < (R.NORM_REL if si == 0 else 1e-5)
        if si == 0:
            assert abs(R.norm64([grads[names.index("grad_1e4")]]) - full) / full < R.NORM_REL
        # without the 1e4 gradients: a chunk of n10241 and the element past the first chunk of n2049 are seen
        assert moved(no1e4, i10241, np.arange(10241) >= 2048) > 100 * R.NORM_REL
        assert moved(no1e4, i2049, last(2049)) > R.NORM_REL and moved(no1e4, i2049, None, twice=2048) > R.NORM_REL
        # alone: every chunk, the last element, and every element just past a chunk
        for name, idx in R.CLIP_SETS.items():
            if len(idx) != 1 or name == "n1":
                continue
            n = grads[idx[0]].size
            assert moved(idx, idx[0], last(n)) > R.NORM_REL, (si, name)
            for c0 in range(0, n, R.OPT_CHUNK):
                inside = (np.arange(n) >= c0) & (np.arange(n) < c0 + R.OPT_CHUNK)
                assert moved(idx, idx[0], ~inside) > R.NORM_REL, (si, name, c0)
                if 0 < c0:
                    assert moved(idx, idx[0], None, twice=c0) > R.NORM_REL, (si, name, c0)
        assert R.clip_max_norm_below(full) <= full / 2 and np.float32(R.clip_max_norm_below(full)) == R.clip_max_norm_below(full)


def test_adam_bounds_can_fail():
    """An element updated twice (a chunk loop running one element too far) and a step taken with the wrong bias correction leave the bounds."""
    p, g = R.opt_params()[3], R.opt_grads(0)[3]
    z = np.zeros_like(p)
    ref = R.adam_ref64(p, g, z, z, 1)
    m_b, v_b, p_b = R.adam_bounds(ref)
    p1, m1, v1 = R.adam32_emul(p, g, z, z, 1)
    p2, m2, v2 = R.adam32_emul(p1, g, m1, v1, 1)
    assert (np.abs(m2 - ref["m"]) > 1000 * m_b).any() and (np.abs(v2 - ref["v"]) > 1000 * v_b).any() and (np.abs(p2 - ref["p"]) > 1000 * p_b).any()
    p3, _, _ = R.adam32_emul(p, g, z, z, 2)
    assert (np.abs(p3 - ref["p"]) > 1000 * p_b).any()

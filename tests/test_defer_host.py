"""What tests/test_defer_gpu.py rests on, proved on the CPU (tests/defer_ref.py states the references, the bounds and the cases):

  * on synthetic partials a float32 emulation of det_column_sum's order lies inside the in-line bound and the float64 replica sum inside the window
    bound, before and after the conversion;
  * each planted fault -- one partial dropped, replica 7 of 8 dropped, S1 and S2 swapped, a's channels credited to b, the scale-0 rule ignored --
    leaves the window bound by at least FAULT_FACTOR, and one dropped tile leaves the 2^-8 bound that ties the partials to the operation;
  * the case tables hold an nb of every class, and restate ocrs_mm_bwd_nparts (which needs no GPU) exactly."""
import numpy as np
import pytest

from tests import defer_ref as D

FAULT_FACTOR = 1e6  # the window bound is ~1e-14 of the sums; every fault below moves a sum by more than 1e-8 of them
NBS = (1, 2, 7, 8, 9, 16, 63, 64, 65, 72, 96, 121, 512)


def _tr_saved(C, seed, zero=None):
    r = np.random.RandomState(seed)
    tr = np.stack([(1.0 + 0.3 * r.standard_normal(C)) * np.where(np.arange(C) % 5, 1, -1), 0.2 * r.standard_normal(C), np.zeros(C)]).astype(np.float32)
    if zero is not None:
        tr[0, zero] = 0.0
    saved = np.stack([0.1 * r.standard_normal(C), 1.0 + 0.2 * r.uniform(size=C)]).astype(np.float32)
    return tr, saved


def _worst(got, want, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.abs(np.asarray(got) - want) / bound
    return float(np.nanmax(np.where(bound > 0, f, np.where(np.asarray(got) == want, 0.0, np.inf))))


def _setup(nb, Ca, Cb, seed=0):
    Cin = Ca + Cb
    p = D.synthetic_partials(nb, Cin, seed)
    tra, sva = _tr_saved(Ca, 11 + seed, zero=1)
    tr, saved = [tra], [sva]
    if Cb:
        trb, svb = _tr_saved(Cb, 12 + seed)
        tr.append(trb)
        saved.append(svb)
    p64 = p.astype(np.float64)
    T1, T2, A1, A2 = p64[..., 0].sum(0), p64[..., 1].sum(0), np.abs(p64[..., 0]).sum(0), np.abs(p64[..., 1]).sum(0)
    pre = [np.zeros((2, c)) for c in ((Ca, Cb) if Cb else (Ca,))]
    return p, tr, saved, (T1, T2, A1, A2), pre


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("Ca,Cb", [(8, 0), (16, 16), (32, 0)])
def test_both_second_stages_lie_inside_their_bounds(nb, Ca, Cb):
    p, tr, saved, (T1, T2, A1, A2), pre = _setup(nb, Ca, Cb)
    want = D.convert(T1, T2, tr, saved, Ca)
    s32 = D.column_sum32(p).astype(np.float64)
    s64 = D.window_sum64(p)
    for name, got, bound in (("in-line", s32, D.inline_sum_bound), ("window", s64, D.window_sum_bound)):
        d1, d2 = bound(nb, A1), bound(nb, A2)
        assert (np.abs(got[:, 0] - T1) <= d1).all() and (np.abs(got[:, 1] - T2) <= d2).all(), name
        inc = D.convert(got[:, 0], got[:, 1], tr, saved, Ca)
        cb = D.convert_bound(d1, d2, T1, T2, tr, saved, Ca, pre)
        for i, w, b in zip(inc, want, cb):
            assert _worst(i, w, b) <= 1.0, name
        assert inc[0][1, 1] == 0.0 and inc[0][0, 1] != 0.0, "the channel with scale 0 gets nothing in the second row"
    # the in-line bound is not vacuous: fp32 chain sums do differ from the exact ones once there are a few partials, by more than the window allows
    if nb >= 16:
        assert _worst(s32[:, 0], T1, D.window_sum_bound(nb, A1)) > 1e3


def test_chain_adds_is_det_column_sums_chain():
    """ceil(nb / 8) + 3 + 3, read off bnstat_ref.col_chain"""
    for nb in NBS:
        assert D.chain_adds(nb) == -(-nb // 8) + 6


def test_column_sum32_is_exact_on_integers_and_order_sensitive_on_floats():
    for nb in NBS:
        ints = np.random.RandomState(nb).randint(-4, 5, (nb, 5)).astype(np.float32)
        assert np.array_equal(D.column_sum32(ints), ints.sum(0))
    p = D.synthetic_partials(96, 8)[..., 0]
    assert not np.array_equal(D.column_sum32(p), D.column_sum32(p[np.random.RandomState(0).permutation(96)]))


FAULTS = ("partial dropped", "slot 7 dropped", "S1 and S2 swapped", "a credited to b", "scale-0 rule ignored")


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("nb", [n for n in NBS if n >= 8])
def test_each_planted_fault_leaves_the_window_bound(nb, fault):
    Ca, Cb = 16, 16
    p, tr, saved, (T1, T2, A1, A2), pre = _setup(nb, Ca, Cb, seed=3)
    want = D.convert(T1, T2, tr, saved, Ca)
    bound = D.convert_bound(D.window_sum_bound(nb, A1), D.window_sum_bound(nb, A2), T1, T2, tr, saved, Ca, pre)
    s = D.window_sum64(p)
    if fault == "partial dropped":
        s = D.window_sum64(p[:-1])
    elif fault == "slot 7 dropped":
        s = D.window_sum64(p, drop_slot=7)
    elif fault == "S1 and S2 swapped":
        s = s[:, ::-1]
    if fault == "a credited to b":
        got = D.convert(s[:, 0], s[:, 1], tr, saved, Ca)[::-1]
    else:
        got = D.convert(s[:, 0], s[:, 1], tr, saved, Ca, zero_rule=fault != "scale-0 rule ignored")
    worst = max(_worst(g, w, b) for g, w, b in zip(got, want, bound))
    assert worst >= FAULT_FACTOR, f"{fault} at nb = {nb}: only {worst:.3g}x the bound"
    if fault == "scale-0 rule ignored":  # (the fault is in the one channel the rule exists for)
        assert not np.isfinite(got[0][1, 1]) and want[0][1, 1] == 0.0


@pytest.mark.parametrize("shape,share", [((1, 5, 7), 1.0), ((2, 21, 37), 0.6), ((2, 37, 53), 0.3), ((4, 64, 96), 0.0)])
def test_one_dropped_tile_leaves_the_tie_bound(shape, share):
    """The partials are tied to the operation at 2^-8 of the absolute sum.  The gradient that flows into a BatchNorm has mean ~0 per channel, so the terms
    are modelled as mean-0 normals, half of them masked by the ReLU.  A dropped whole tile (32 x 8 pixels, the smallest the kernels use; the whole image
    where that is smaller) moves a channel's sum by ~sqrt(pixels of the tile / 2), against a bound of 2^-8 * 0.8 * (pixels of the batch / 2): out of the
    bound for every channel at (1, 5, 7), for most at (2, 21, 37) (16 sd against 2.4), for a good part at (2, 37, 53) (against 6.1) -- and for none at
    (4, 64, 96) (against 38), which is in the tables for the unrolled part of the in-line chain, not for this: a tile loop that drops a tile drops it
    at every shape."""
    N, H, W = shape
    r = np.random.RandomState(H)
    x = r.standard_normal((32, N, H, W)) * (r.uniform(size=(32, N, H, W)) < 0.5)
    full, A = x.sum((1, 2, 3)), np.abs(x).sum((1, 2, 3))
    x[:, 0, :8, :32] = 0.0
    frac = np.abs(x.sum((1, 2, 3)) - full) / D.tie_bound(A)
    assert (frac > 1.0).mean() >= share, f"{shape}: {(frac > 1.0).mean():.2f} of the channels leave the bound"
    if share == 0.0:
        assert frac.max() < 1.0


def test_case_tables_hold_every_class_of_nb():
    table = D.nb_table()
    assert len(table) == len(D.block_cases()) == len(set(D.block_cases()))
    assert {D.nb_class(nb) for nb in table.values()} == {1, 2, 3, 4}
    # the tile kernel in every class, its pooled form too; the row-streaming form (at most 8 workgroups below (4, 96, 128)) in the first two
    for pooled in (0, 1):
        assert {D.nb_class(nb) for c, nb in table.items() if c[5] == pooled and not D.rs_form(c[1], c[2], c[3], pooled)} == {1, 2, 3, 4}
    assert {D.nb_class(nb) for c, nb in table.items() if D.rs_form(c[1], c[2], c[3], c[5])} == {1, 2}
    assert any(c[1:3] == (32, 32) and D.nb_class(nb) == 4 for c, nb in table.items()), "the two launches of the 32 | 32 split with wrapped replicas"
    assert all(n <= 4 and h <= 96 and w <= 128 for (n, h, w) in D.SHAPES) and D.XU_SHAPE == (1, 2, 192)  # (the one shape the u-plane route needs)
    assert (2, 21, 37) in D.SHAPES and D.nb_of(8, 0, 8, 0, *D.XU_SHAPE) == 2


def test_nb_table_restates_the_query():
    """ocrs_mm_bwd_nparts is host arithmetic: the restatement in defer_ref.nb_of is checked here as well as on the GPU"""
    from ocrs_models_amd._lib import lib

    L = lib()
    for c, nb in D.nb_table().items():
        C0, Ca, Cb, Cc, (N, H, W), pooled, two = c
        assert L.mm_bwd_nparts(Ca, Cb, Cc, pooled, two, N, H, W) == nb, c
    for shape in D.SHAPES + (D.XU_SHAPE, (4, 96, 128), (3, 45, 64)):
        for pooled in (0, 1):
            assert L.mm_bwd_nparts(8, 0, 8, pooled, 0, *shape) == D.nb_of(8, 0, 8, pooled, *shape), shape
    assert L.mm_bwd_nparts(8, 0, 32, 0, 0, 2, 21, 37) == 0 and L.mm_bwd_nparts(8, 0, 8, 0, 0, 2, 1, 37) == 0  # unsupported: no launch, no partials

"""CPU: what tests/test_ctc_gpu.py rests on (tests/ctc_ref.py).

* the float64 reference is the oracle's: brute-force enumeration on tiny cases, oracle.ctc.ctc_alpha_beta_np per sample, and
  torch.nn.functional.ctc_loss(reduction="none") in float64 on every feasible sample of every case, each to <= 1e-10;
* the float32 emulation of the kernels' written arithmetic stays within HALF of every bound on every case and seed (the measurement that
  fixed the constants: the bound is twice the emulation's largest ratio), with and without the fp16 lattice storage;
* on single_path the emulated nll IS the sequential float32 sum of the one alignment and the float64 gradient is exp(lp) - onehot;
* every wrong kernel of ctc_ref.MUTANTS leaves a per-sample bound on at least one case.

What the earlier criterion (whole-batch gradient relL2 < 1e-4 and mean loss within 1e-5 relative, on `mixed`, the only case the suite had)
says about the same mutants -- printed by test_mutants_exceed_a_per_sample_bound, recorded here as information:

    mutant           gradient relL2   mean loss rel.   earlier criterion    per-sample bounds (worst ratio / bound, first case that sees it)
    skip_repeat      7.7e-03          2.5e-04          fails                4.8e+05 x bound on mixed
    skip_blank       3.4e-02          1.4e-03          fails                2.9e+05 x bound on mixed
    last_only        7.6e-01          1.6e-02          fails                2.6e+07 x bound on mixed
    scale_noclamp    inf              6.4e-08          fails                inf (the L = 0 sample)
    row_Tn           6.9e-02          6.4e-08          fails                inf (a row that must be 0)
    beta_last_only   3.4e-01          6.4e-08          fails                2.1e+04 x bound on mixed
    occ_shift        5.0e-01          6.4e-08          fails                5.3e+07 x bound on mixed

So on `mixed` the earlier criterion, had it been applied to these mutants, would have refused all seven: that batch has short samples, an empty
target and repeated labels, and each mutant moves the whole-batch norm by 0.8 % or more.  What it could not see is smaller: the per-sample
bounds are four to seven orders of magnitude closer to the kernels than 1e-4 of a batch norm (a wrong transition confined to the T_n = 4
sample of `mixed` moves the batch norm by its 3 % share of it), nll[n] itself, the exact zeros, and everything outside that one batch.
"""
import itertools

import numpy as np
import pytest
import torch

from oracle.ctc import ctc_alpha_beta_np, ctc_brute_force
from tests import ctc_ref as R


def test_reference_matches_brute_force_on_tiny_cases():
    r = np.random.RandomState(0)
    for T, C, target in [(1, 3, []), (1, 3, [2]), (3, 3, [1]), (4, 3, [1, 1]), (4, 3, [1, 2]), (5, 3, [2, 2, 1]), (5, 4, [1, 2, 3]), (4, 2, [1, 1]),
                         (3, 3, [1, 1]), (5, 3, [])]:
        lp = R.log_softmax64(2 * r.randn(T, C))
        want = ctc_brute_force(lp, target)
        got = R.ctc_sample64(lp, target, T)["nll"]
        if np.isinf(want):
            assert got == np.inf, (T, C, target)
        else:
            assert abs(got - want) <= 1e-10, (T, C, target, got, want)


@pytest.mark.parametrize("name", R.CASES)
def test_reference_matches_the_oracle_and_torch_float64(name):
    c, ref = R.case(name), R.case_ref(name)
    T, N, C = c["lp"].shape
    lp64 = torch.from_numpy(c["lp"].astype(np.float64)).requires_grad_(True)
    Lp = max(1, int(c["tl"].max()))
    per = torch.nn.functional.ctc_loss(lp64, torch.from_numpy(c["targets"][:, :Lp].astype(np.int64)), torch.from_numpy(np.array(c["il"])),
                                       torch.from_numpy(np.array(c["tl"])), reduction="none")
    feas = ref["feasible"]
    assert [n for n in range(N) if not feas[n]] == list(R.INFEASIBLE.get(name, ()))  # feasibility is as stated
    scale = torch.from_numpy(np.where(feas, 1.0 / (N * np.maximum(c["tl"], 1)), 0.0))
    (per * scale)[torch.from_numpy(feas)].sum().backward()
    for n in range(N):
        L, Ti = int(c["tl"][n]), int(c["il"][n])
        nll, a, b, g = ctc_alpha_beta_np(c["lp"][:, n].astype(np.float64), c["targets"][n, :L], Ti)
        if not feas[n]:
            assert nll == np.inf and ref["nll"][n] == np.inf and per[n].item() == np.inf
            continue
        assert abs(nll - ref["nll"][n]) <= 1e-10 and abs(per[n].item() - ref["nll"][n]) <= 1e-10, (name, n)
        assert np.abs(g / (N * max(L, 1)) - ref["grad"][:, n]).max() <= 1e-10, (name, n)
        assert np.abs(lp64.grad[:, n].numpy() - ref["grad"][:, n]).max() <= 1e-10, (name, n)
        assert np.all(ref["grad"][Ti:, n] == 0)
    # the properties the cases are there for
    if name == "peaked":
        for k in range(R.SEEDS_PER_CASE):
            assert R.case_ref(name, k)["nll"].max() < 10, k
    if name == "wide":
        assert 2 * int(c["tl"].max()) + 1 > 256
    if name == "mixed":
        assert list(c["il"]) == [37, 5, 20, 37, 37, 10, 30, 25, 4] and list(c["tl"]) == [0, 1, 5, 12, 18, 3, 7, 9, 2]
        assert c["targets"][3, 1] == c["targets"][3, 0] and len(set(c["targets"][4, 2:6])) == 1
    if name == "edges_len":
        assert list(ref["nll"][2:]) == [0.0, np.inf]


def test_emulation_stays_within_half_of_every_bound():
    """the measurement behind K_NLL, K_GRAD, K_GRAD_H16: per case the largest ratio over SEEDS_PER_CASE seeds"""
    worst = {}
    for name, k, h16 in itertools.product(R.CASES, range(R.SEEDS_PER_CASE), (False, True)):
        nll, grad = R.ctc_batch32(R.case(name, k), h16=h16)
        rn, rg = R.ctc_ratios(nll, grad, R.case_ref(name, k))
        w = worst.setdefault((name, h16), [0.0, 0.0])
        w[0], w[1] = max(w[0], rn.max()), max(w[1], rg.max())
    for (name, h16), (rn, rg) in worst.items():
        print(f"{name:12s} {'fp16' if h16 else 'fp32'} lattice: nll {rn:.3f} (bound {R.K_NLL}), gradient {rg:.2f} (bound {R.K_GRAD_H16 if h16 else R.K_GRAD})")
    for (name, h16), (rn, rg) in worst.items():
        assert rn <= 0.5 * R.K_NLL, (name, h16, rn)
        assert rg <= 0.5 * (R.K_GRAD_H16 if h16 else R.K_GRAD), (name, h16, rg)
    # and the constants are the measurement, not something wider: twice the largest ratio, rounded up by at most a tenth
    assert max(w[0] for w in worst.values()) >= 0.9 * 0.5 * R.K_NLL
    assert max(w[1] for (n, h), w in worst.items() if not h) >= 0.9 * 0.5 * R.K_GRAD
    assert max(w[1] for (n, h), w in worst.items() if h) >= 0.9 * 0.5 * R.K_GRAD_H16


def test_single_path_is_a_sequential_sum():
    for k in range(R.SEEDS_PER_CASE):
        c, ref = R.case("single_path", k), R.case_ref("single_path", k)
        nll, _ = R.ctc_batch32(c)
        T, N, C = c["lp"].shape
        for n in range(N):
            L, Ti = int(c["tl"][n]), int(c["il"][n])
            want, path = R.sequential_nll32(c["lp"][:, n], c["targets"][n, :L], Ti)
            assert nll[n].tobytes() == want.tobytes(), (k, n)
            onehot = np.zeros((T, C))
            onehot[np.arange(Ti), path] = 1.0
            g = np.exp(c["lp"][:, n].astype(np.float64)) - onehot
            g[Ti:] = 0
            assert np.abs(ref["grad"][:, n] - g / (N * max(L, 1))).max() <= 1e-12, (k, n)


def test_mutants_exceed_a_per_sample_bound():
    mixed, mref = R.case("mixed"), R.case_ref("mixed")
    rows = []
    for mutant in R.MUTANTS:
        seen = None
        for name in R.CASES:
            nll, grad = R.ctc_batch32(R.case(name), mutant=mutant)
            rn, rg = R.ctc_ratios(nll, grad, R.case_ref(name))
            over = max((rn / R.K_NLL).max(), (rg / R.K_GRAD).max())
            if over > 1 and seen is None:
                seen = (name, over)
        nll, grad = R.ctc_batch32(mixed, mutant=mutant)
        with np.errstate(invalid="ignore"):
            l2 = np.linalg.norm(grad.astype(np.float64) - mref["grad"]) / np.linalg.norm(mref["grad"])
            loss = float(np.mean(nll.astype(np.float64) / np.maximum(mixed["tl"], 1)))
        dl = abs(loss - mref["loss"]) / abs(mref["loss"])
        old = "passes" if (l2 < 1e-4 and dl < 1e-5) else "fails"
        rows.append((mutant, l2, dl, old, seen))
    print("mutant           gradient relL2   mean loss rel.   earlier criterion    per-sample bounds")
    for mutant, l2, dl, old, seen in rows:
        print(f"{mutant:16s} {l2:<16.1e} {dl:<16.1e} {old:20s} " + (f"{seen[1]:.3g} x bound on {seen[0]}" if seen else "NOT SEEN"))
    for mutant, _, _, _, seen in rows:
        assert seen is not None, mutant


@pytest.mark.parametrize("bf16", [False, True])
def test_log_softmax_emulation_within_half_of_the_counted_bounds(bf16):
    wf = wb = 0.0
    for rows, C in itertools.product(R.LSM_ROWS, R.LSM_C):
        c = R.lsm_case(rows, C, bf16)
        out64, unit = R.lsm_fwd_ref(c["x"])
        out32 = R.lsm_fwd32(c["x"])
        inf = ~np.isfinite(out64)
        assert np.array_equal(out32[inf], out64[inf].astype(np.float32))
        assert np.isfinite(out32[~inf]).all()
        wf = max(wf, float((np.abs(out32[~inf].astype(np.float64) - out64[~inf]) / unit[~inf]).max()))
        const = c["kind"] == R.LSM_KINDS.index("const")
        assert np.abs(out64[const] + np.log(C)).max(initial=0) <= 1e-12  # a constant row: -log C
        lp = np.where(inf, -np.inf, out32)
        d64, bunit = R.lsm_bwd_ref(lp, c["g"])
        wb = max(wb, float((np.abs(R.lsm_bwd32(lp, c["g"]).astype(np.float64) - d64) / bunit).max()))
    print(f"log-softmax emulation ({'bf16' if bf16 else 'fp32'} input): forward {wf:.3f}, backward {wb:.3f} of the counted units (bound {R.K_LSM})")
    assert wf <= 0.5 * R.K_LSM and wb <= 0.5 * R.K_LSM


def test_greedy_reference_rules():
    from oracle.text import greedy_collapse

    assert R.collapse([1, 1, 0, 1, 2, 2], 6) == [1, 1, 2] == greedy_collapse([1, 1, 0, 1, 2, 2])
    assert R.collapse([0, 0, 0], 3) == [] and R.collapse([3, 3], 0) == [] and R.collapse([3, 3], 1) == [3]
    lp = np.zeros((1, 1, 5), dtype=np.float32)
    assert R.first_argmax(lp)[0, 0] == 0
    r = np.random.RandomState(1)
    want = r.randint(0, 5, (3, 7))
    assert np.array_equal(R.first_argmax(R.plant_argmax(r, want, 5)), want)

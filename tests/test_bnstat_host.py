"""What tests/test_bnstat_gpu.py rests on, proved on the CPU for every case it uses (tests/bnstat_ref.py states the cases once):

  * every statistics case has the channels it was built for: an exactly zero variance, a float64 variance below zero in front of the clamp
    (count = 351), |mean| / std of 1e3, both signs of gamma and a zero;
  * the float32 emulation of k_bn_finalize, plain and with the multiply-adds fused, lies inside every stated bound, twice in a row; the biased
    variance in run_var would not;
  * every chain case has NO pre-activation within SIGN_MARGIN of zero and no window whose two largest activations are closer than that (equal
    ones, from equal stored values, excepted); the reduce kernels' launches give one pixel per thread, as the emulation's summation order assumes;
  * the emulation's dz in the per-element unit (printed), its bf16 form within one bf16 ulp of the rounded float64 dz on at most 1 % of the
    elements, its dgamma / dbeta inside the derived bounds; a coefficient with a term or a factor missing moves dz far outside twice that;
  * the column-sum row counts reach the loops they are there for; the fold table's rows do not overlap.
"""
import numpy as np
import pytest

from tests import bnstat_ref as R
from tests.lossopt_ref import ulp32, ulps

_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("count", R.FIN_COUNTS)
@pytest.mark.parametrize("C", R.FIN_C)
def test_finalize_cases(C, count, bf16):
    case = R.fin_case(C, count, bf16)
    z, gamma, beta, gstat = case["z"], case["gamma"], case["beta"], case["gstat"]
    if bf16:
        assert np.array_equal(R.bf16_round32(z), z)
    assert (gamma > 0).any() and (gamma < 0).any() and gamma[R.CH_ZERO_GAMMA] == 0
    rm = np.full(C, R.FIN_PREFILL[0], np.float32)
    rv = np.full(C, R.FIN_PREFILL[1], np.float32)
    ref = R.finalize_ref64(gstat, count, gamma, beta, rm, rv)
    assert ref["var_raw"][R.CH_CONST] == 0.0
    assert np.float32(ref["rstd"][R.CH_CONST]) == np.float32(1.0 / np.sqrt(R.EPS))
    if count == R.FIN_COUNTS[-1]:
        if not bf16:  # (bf16-exact values cannot have it: see neg_var_column)
            assert ref["var_raw"][R.CH_NEG] < 0, "the clamp is not exercised"
            assert np.float32(ref["rstd"][R.CH_NEG]) == np.float32(1.0 / np.sqrt(R.EPS))
        ratio = np.abs(ref["mean"]) * ref["rstd"]
        assert ratio[R.CH_1E3] > (300 if bf16 else 800)  # (bf16 storage of 1000 std +- std adds its own spread)
        assert ratio[R.CH_1E2] > 80 and ratio[R.CH_30] > 24
    if count < R.FIN_COUNTS[-1] or bf16:
        assert ref["var_raw"][R.CH_NEG] == 0.0
    if count == 1:
        assert not ref["var"].any() and not ref["unb"].any()  # one value per channel: variance zero, and count - 1 = 0 is not divided by
    for fused in (False, True):
        old_m, old_v = rm, rv
        for call in range(2):  # the running statistics chain: the second call starts from the first one's float32 results
            r = R.finalize_ref64(gstat, count, gamma, beta, old_m, old_v)
            sc, sh, mu, rs, nm, nv = R.finalize_emul(gstat, count, gamma, beta, old_m, old_v, fused)
            assert ulps(mu, r["mean"]).max() <= 0.5 and ulps(rs, r["rstd"]).max() <= 0.5
            for name, got, want, bound in (("sc", sc, r["sc"], r["sc_bound"]), ("sh", sh, r["sh"], r["sh_bound"]),
                                           ("run_mean", nm, r["run_mean"], r["run_mean_bound"]), ("run_var", nv, r["run_var"], r["run_var_bound"])):
                err = np.abs(got.astype(np.float64) - want) / bound
                assert err.max() <= 1.0, (name, fused, call, int(err.argmax()), float(err.max()))
            old_m, old_v = nm, nv
    if count > 1:
        # trial (a): the biased variance in run_var
        biased = (1.0 - R.MOM) * rv.astype(np.float64) + R.MOM * ref["var"]
        moved = np.abs(biased - ref["run_var"]) / ref["run_var_bound"]
        assert np.median(moved) > 100, float(np.median(moved))


@pytest.mark.parametrize("nparts,C", R.PARTS_CASES)
def test_parts_totals_are_exact(nparts, C):
    case = R.parts_case(nparts, C)
    p = case["parts"]
    assert np.array_equal(p, np.rint(p)) and float(np.abs(p).sum(0).max()) < 2 ** 24
    assert np.array_equal(p.sum(0, dtype=np.float32).astype(np.float64).T, case["gstat"])
    ref = R.finalize_ref64(case["gstat"], case["count"], case["gamma"], case["beta"])
    assert (ref["var_raw"] > 1.0).all()


CHAIN_RUNS = [(d, n, False) for d in R.CHAIN_CASES for n in ("fp32", "bf16")] + [(R.AVG_CHAIN, n, True) for n in ("fp32", "bf16")]


@pytest.mark.parametrize("dims,dname,avg", CHAIN_RUNS, ids=[f"{_ids(d)}-{n}" for d, n, _ in CHAIN_RUNS])
def test_chain_cases(dims, dname, avg):
    case = R.chain_case(dims, dname, None, avg)
    ref = R.chain_reference(dims, dname, None, avg)
    C = case["gamma"].size
    assert ref["close"] == 0, "a sign or maximum decision inside SIGN_MARGIN: choose another salt"
    ratio = np.abs(ref["mean"]) * ref["rstd"]
    assert ratio[R.CH_30] > 20 and np.delete(ratio, R.CH_30).max() < 4
    per_block, per_thread, chain = R.reduce_plan(case)
    assert per_thread == 1 and per_block == 256 // (C // 8) and chain == per_block + 1
    emul = R.chain_emul(dims, dname, None, avg)
    if dname == "fp32":
        e = R.dz_units(emul["dz"], ref)
        print(f"chain {_ids(dims)} fp32: emulated dz {e:.2f} units from float64")
        # trials (b) and (c): C without its mean rstd m2 term, B with one rstd missing -- in float64, nothing else changed
        v = lambda t: t.reshape(1, 1, 1, C)  # noqa: E731
        z = case["z"].astype(np.float64)
        m2 = -ref["B"] / (ref["A"] * ref["rstd"])
        for name, B, Cc in (("b", ref["B"], ref["Cc"] - ref["A"] * ref["mean"] * ref["rstd"] * m2), ("c", ref["B"] / ref["rstd"] * 1.0, ref["Cc"])):
            wrong = v(ref["A"]) * ref["ghat"] + v(B) * z + v(Cc)
            moved = np.abs(wrong - ref["dz"]) / ref["unit"]
            if name == "c":
                moved = moved[..., np.abs(ref["rstd"] - 1) > 0.05]  # (a channel with rstd = 1 would not notice)
            assert moved.max() > 100 * e, (name, float(moved.max()), e)
    else:
        worst, share = R.bf16_offsets(emul["dz"], ref)
        print(f"chain {_ids(dims)} bf16: emulated dz at most {worst:.0f} bf16 ulp off, {share:.5f} of the elements unequal")
        assert worst <= 1.0 and share <= R.BF16_OFF_BY_ONE_SHARE
    # sum dz = 0 and sum dz zhat = -B count eps rstd hold for the float64 dz itself (the second is not zero: eps) and, within the summed
    # per-element bound, for the emulation
    bound = 2.0 * e * ref["unit"] if dname == "fp32" else 1.5 * R.ulp_bf16(R.bf16_from64(ref["dz"]))
    i0, i1, r0, r1 = R.identities(case, ref, emul["dz"], bound)
    assert r0 <= 1e-10 and r1 <= 1e-6 and i0 <= 1.0 and i1 <= 1.0, (i0, i1, r0, r1)
    e1, e2 = R.gsum_bounds(case, ref)
    assert (np.abs(emul["dbeta"].astype(np.float64) - ref["dbeta"]) <= e1 + ulp32(ref["dbeta"])).all()
    assert (np.abs(emul["dgamma"].astype(np.float64) - ref["dgamma"]) <= e2 + ulp32(ref["dgamma"])).all()
    if avg:
        assert (np.abs(emul["out"].astype(np.float64) - ref["out"]) <= R.avg_out_bound(case, ref)).all()


def test_column_sum_rows_reach_their_loops():
    plans = {rows: R.col4_plan(rows) for rows in R.COL_ROWS}
    assert [plans[r][0] for r in R.COL_ROWS] == [1, 1, 1, 2, 257, 512, 512, 512]
    assert plans[4099][1] == {4, 1} and plans[14337][1] == {8, 4, 1} and plans[16389][1] == {8, 1} and plans[40000][1] == {8, 4, 1}
    assert plans[17][1] == {1} and plans[16][1] == {4}  # 16 rows, one block: every phase's four rows in one 4-row step
    for C, ld in R.COL4_SHAPES:
        assert C % 4 == 0 and ld % 4 == 0 and ld >= C
    for C, ld, off in R.COL1_SHAPES:
        assert C % 4 or ld % 4 or off  # each fails exactly one test of the launcher's
        assert sum([C % 4 != 0, ld % 4 != 0, off != 0]) >= 1 and ld >= C
    assert R.COL1_SHAPES[2][:2] == (128, 128)
    assert R.col_chain(40000, True) == 3 + 5 + 2 + 512 and R.col_chain(40000, False) == 20 + 1 + 1024


def test_fold_table_rows_do_not_overlap():
    assert [n for _, _, n in R.FOLD_TABLE] == [0, 1, 63, 64, 65, 1000]
    assert all(d > 0 and s > 0 and d != s for d, s, _ in R.FOLD_TABLE)
    hit = np.zeros(R.FOLD_DST, int)
    for d, s, n in R.FOLD_TABLE:
        assert d + n <= R.FOLD_DST and s + n <= R.FOLD_SRC
        hit[d:d + n] += 1
    assert hit.max() == 1 and hit.sum() < R.FOLD_DST

"""What tests/test_defer_gpu.py compares the block backward inside a deferral window against (ocrs_bwd_defer_begin .. ocrs_bwd_defer_flush), in
numpy float64, stated once; tests/test_defer_host.py proves on the CPU that the bounds hold for the arithmetic they are derived from and that
each planted fault leaves them.

The partials (include/ocrs_hip.h at ocrs_mm_bwd_nparts): a launch of the matrix-core / row-streaming block backward leaves nb per-block partials
in its workspace, partial b at ws[b * ne], ne = Cout * Cin + 11 * Cin:  [Cout][Cin] dWpw | [Cin][9] dWdw | [Cin][S1 | S2] interleaved.

The two second stages of the producers' sums S1 = sum ghat', S2 = sum ghat' x~:
  in line (no window)  k_mm_bwd_reduce (csrc/det_mm.hip): fp32 column sums in det_column_sum's order (csrc/common.h), then the conversion in fp64
  window               BwdLast (csrc/det_common.h): every workgroup adds its fp32 partial, widened, into one of 8 fp64 replicas (bwd_last_add); the
                       last workgroup sums the 8 replicas and converts (bwd_last_finish)
Both convert with   gsum[0][c] += S1,   gsum[1][c] += rstd * ((S2 - sh * S1) / sc - mean * S1)   if sc != 0   (sc | sh: the source's load transform,
mean | rstd: its saved statistics), per source of a concat."""
import numpy as np

from tests import bnstat_ref as R

U32, U64 = 2.0 ** -24, 2.0 ** -53
SLOTS = 8  # BWD_LAST_SLOTS
NUM_CU = R.NUM_CU


def ne_of(Cin, Cout):
    return Cout * Cin + 11 * Cin


def split_stride(nb, Cout):
    """floats between the two launches' partials of a 32 | 32 concat (mm_bwd_impl: each launch has its partials and 1024 floats of scratch lines per block)"""
    return nb * (Cout * 32 + 11 * 32 + 1024)


def partials(ws, nb, Cin, Cout):
    """-> float64 [nb][Cin][2] (S1 | S2) of the nb partials at the head of ws"""
    ne = ne_of(Cin, Cout)
    p = np.asarray(ws, dtype=np.float32)[:nb * ne].reshape(nb, ne)
    return p[:, Cout * Cin + 9 * Cin:].reshape(nb, Cin, 2).astype(np.float64)


def sums_from_partials(ws, nb, Cin, Cout):
    """-> T1[c], T2[c] (float64 sums over the nb partials: nb <= 768 fp32 values of 24 bits each, so float64 adds them to within nb * 2^-53 of their
    absolute sum -- three orders below every bound here) and A1[c], A2[c] (sums of absolute values)"""
    p = partials(ws, nb, Cin, Cout)
    return p[..., 0].sum(0), p[..., 1].sum(0), np.abs(p[..., 0]).sum(0), np.abs(p[..., 1]).sum(0)


def weight_partials(ws, nb, Cin, Cout):
    """-> float64 [nb][Cout * Cin + 9 * Cin]: the weight-gradient columns of the partials"""
    ne = ne_of(Cin, Cout)
    return np.asarray(ws, dtype=np.float32)[:nb * ne].reshape(nb, ne)[:, :Cout * Cin + 9 * Cin].astype(np.float64)


def _per_source(T, Ca):
    return [T[:Ca]] + ([T[Ca:]] if Ca < T.size else [])


def convert(T1, T2, tr, saved, Ca, zero_rule=True):
    """bwd_last_finish / k_mm_bwd_reduce in float64.  T1, T2 [Cin]; tr, saved: per source [3][Cs], [2][Cs] (a list: a, then b when Ca < Cin).
    -> per source the [2][Cs] increments of gsum; a channel with scale exactly 0 gets nothing in the second row (zero_rule=False: the planted fault)"""
    out = []
    for S1, S2, t, sv in zip(_per_source(T1, Ca), _per_source(T2, Ca), tr, saved):
        t, sv = np.asarray(t, np.float64), np.asarray(sv, np.float64)
        sc, sh, mean, rstd = t[0], t[1], sv[0], sv[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            second = rstd * ((S2 - sh * S1) / sc - mean * S1)
        if zero_rule:
            second = np.where(sc != 0.0, second, 0.0)
        out.append(np.stack([S1, second]))
    return out


def chain_adds(nb):
    """fp32 additions between a partial and the column sum in det_column_sum: a chain of ceil(nb / 8), 3 to combine the chains' accumulators, 3 through
    the LDS tree.  bnstat_ref.col_chain states exactly this for k_reduce_multi (the same function); it is read off there as the difference of its
    deferred and atomic forms at rows = 2 nb (scalar kernel: nb blocks, the same inner chain in both), less the final += onto out (here in fp64)."""
    assert 1 <= nb <= 1024
    return R.col_chain(2 * nb, False, True) - R.col_chain(2 * nb, False, False) + nb - 1


def inline_sum_bound(nb, A):
    """every add of the chain rounds a partial sum of at most A = sum |partial| to fp32"""
    return chain_adds(nb) * U32 * A


def window_sum_bound(nb, A):
    """the widening float -> double is exact; nb atomic adds into the replicas and 8 adds over the replicas each round a partial sum of at most A to
    fp64 (bwd_last_add / bwd_last_finish)"""
    return (nb + SLOTS) * U64 * A


def convert_bound(d1, d2, T1, T2, tr, saved, Ca, prefill):
    """errors d1, d2 [Cin] of S1, S2 through the conversion, per source [2][Cs]:
        row 0:  d1
        row 1:  |rstd| (d2 + |sh| d1) / |sc| + |rstd mean| d1
    plus 8 fp64 ulps (2^-53 relative each) of the terms of the evaluation -- S1; |rstd| (|S2| + |sh S1|) / |sc| + |rstd mean S1| (five operations) --
    and of |prefill| + |increment|: the += onto gsum rounds at that magnitude, and so does the test's subtraction of the prefill.  prefill: per
    source [2][Cs]."""
    out = []
    for D1, D2, S1, S2, t, sv, pre in zip(_per_source(d1, Ca), _per_source(d2, Ca), _per_source(T1, Ca), _per_source(T2, Ca), tr, saved, prefill):
        t, sv, pre = np.asarray(t, np.float64), np.asarray(sv, np.float64), np.abs(np.asarray(pre, np.float64))
        sc, sh, mean, rstd = np.abs(t[0]), np.abs(t[1]), np.abs(sv[0]), np.abs(sv[1])
        live = sc != 0.0
        scs = np.where(live, sc, 1.0)
        b1 = np.where(live, rstd * (D2 + sh * D1) / scs + rstd * mean * D1, 0.0)
        mag1 = np.where(live, rstd * (np.abs(S2) + sh * np.abs(S1)) / scs + rstd * mean * np.abs(S1), 0.0)
        out.append(np.stack([D1 + 8 * U64 * (2 * pre[0] + np.abs(S1)), b1 + 8 * U64 * (2 * pre[1] + mag1)]))
    return out


def column_sum32(p):
    """det_column_sum in numpy float32: p [nb][...] -> [...].  Thread `chain` k owns partials k, k + 8, ...; it walks them 64 at a time into eight
    accumulators (a[u] takes k + 8 u + 64 j) and the rest in turn (a[u & 7]); ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), then the same tree over the chains"""
    p = np.asarray(p, np.float32)
    nb = p.shape[0]
    tree = lambda v: ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))  # noqa: E731
    red = []
    for chain in range(8):
        a = [np.zeros(p.shape[1:], np.float32) for _ in range(8)]
        b = chain
        while b + 56 < nb:
            for u in range(8):
                a[u] = a[u] + p[b + 8 * u]
            b += 64
        u = 0
        while b < nb:
            a[u & 7] = a[u & 7] + p[b]
            b += 8
            u += 1
        red.append(tree(a))
    return tree(red)


def window_sum64(p, drop_slot=None):
    """BwdLast in numpy: workgroup b adds into replica b & 7, the last one sums the replicas (drop_slot: the planted fault of a missed replica)"""
    p = np.asarray(p, np.float32).astype(np.float64)
    slots = [p[k::SLOTS].sum(0) for k in range(SLOTS)]
    return sum(s for k, s in enumerate(slots) if k != drop_slot)


def tie_bound(abs_sum):
    """|T - float64 sum over the kernel's own stored tensors| <= 2^-8 * sum |terms|: one bf16 rounding (2^-9 relative) of each stored element, doubled.
    What the two kernels sum (csrc/det_mm.hip at `t1[i] += gh`, csrc/det_rs.hip:20-23):
      k_mm_bwd  S1: the STORED (rounded) dx~ where x~ > 0 -- the reference's terms exactly, summed in fp32;  S2: sum_{tap, o} Weff G_tap = the sum of the
                UNROUNDED dx~ times the bf16 x~ of the staged tile (0 where the ReLU clamps)
      k_rs_bwd  both from the weight-gradient GEMM: the unrounded dx~ times the 0 / 1 mask (S1), times the bf16 x~ (S2)
    so each term differs from the reference's by the rounding of dx~ to its stored value (2^-9) and, in S2, that of x~ to bf16 (2^-9): 2^-8 in all.  The
    fp32 accumulation (2^-24 per add) is four orders below."""
    return 2.0 ** -8 * np.asarray(abs_sum, np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launch arithmetic, restated (csrc/det_mm.hip mm_grid / mm_bwd_th, csrc/det_rs.hip rs_bwd_supported / rs_geometry, csrc/common.h persistent_grid)
# ---------------------------------------------------------------------------------------------------------------------------------------
def rs_form(Ca, Cb, Cout, pooled):
    """the launch runs the row-streaming kernel k_rs_bwd (8 -> 8 and 8 -> 16 channels, unpooled; an 8-channel concat only as 8 | 8 -- none here)"""
    return not pooled and Ca + Cb == 8 and Cout in (8, 16) and Cb == 0


def _round8(g):
    return g & ~7 if g >= 8 else max(g, 1)


def nb_of(Ca, Cb, Cout, pooled, N, H, W):
    """ocrs_mm_bwd_nparts"""
    if rs_form(Ca, Cb, Cout, pooled):
        njobs = N * -(-((H + 1) // 2) // 32) * -(-W // 30)
        return _round8(min((njobs + 3) // 4, NUM_CU * (3 if Cout == 8 else 2)))
    Cin = 32 if (Ca, Cb) == (32, 32) else Ca + Cb
    th = 8 if (Cin == 32 or Cout == 32 or (Cin == 16 and Cout == 16 and not pooled)) else 12
    p = 1 if pooled else 0
    return _round8(min(N * -(-(W + p) // 32) * -(-(H + p) // th), 2 * NUM_CU))


def nb_class(nb):
    """1: the only workgroup is also the last; 2: not every replica is used; 3: the replicas wrap; 4: the unrolled part of the in-line chain runs"""
    return 1 if nb == 1 else 2 if nb <= 8 else 3 if nb <= 64 else 4


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
# (C0, Ca, Cb, Cc) as MM_CASES of tests/test_det_ops_gpu.py (asserted equal there): producers A (and B) C0 -> Ca (Cb), the block under test Ca | Cb -> Cc
MM_CASES = ((8, 8, 8, 8), (8, 8, 0, 16), (8, 16, 0, 8), (8, 16, 0, 16), (8, 8, 8, 16), (16, 16, 16, 16), (8, 16, 0, 32), (16, 32, 0, 32), (16, 32, 32, 32),
            (16, 32, 0, 16))
# (1, 5, 7): one tile; (2, 21, 37): the suite's usual, tiles cut by the border on both axes; (2, 37, 53): 16 workgroups, cut on both axes;
# (4, 64, 96): 72 or 96 workgroups of the tile kernel
SHAPES = ((1, 5, 7), (2, 21, 37), (2, 37, 53), (4, 64, 96))
XU_SHAPE = (1, 2, 192)  # the first block writes its u plane only for whole 64-column x 2-row units


def block_cases():
    """(C0, Ca, Cb, Cc, shape, pooled, two_grads): every channel set at every shape, direct and pooled; at the usual shape with one and with two gradient
    tensors, elsewhere two where pooled (the form of the model's down path) and one where direct"""
    out = []
    for chans in MM_CASES:
        for shape in SHAPES:
            for pooled in (0, 1):
                for two in ((0, 1) if shape == (2, 21, 37) else (pooled,)):
                    out.append((*chans, shape, pooled, two))
    return out


def nb_table():
    """{case: nb}: what the GPU tests assert equal to ocrs_mm_bwd_nparts"""
    return {c: nb_of(c[1], c[2], c[3], c[5], *c[4]) for c in block_cases()}


def synthetic_partials(nb, Cin, seed=0, tiles=None):
    """fp32 partials [nb][Cin][2] shaped like a launch's: every workgroup's share is the sum of `tiles` per-tile values of mixed sign (mean 0.3, sd 1:
    the S1 / S2 of a few hundred pixels), so the totals do not cancel"""
    r = np.random.RandomState(1000 * nb + Cin + seed)
    return (0.3 + r.standard_normal((nb, Cin, 2))).astype(np.float32) * np.float32(tiles or 1)

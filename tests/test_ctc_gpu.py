"""csrc/rec_seq.hip through the C ABI against the float64 references of tests/ctc_ref.py: per-sample nll and every gradient element of the
three CTC forms inside bounds that scale with each sample's lattice (derivation and measured constants: ctc_ref.py; what they rest on:
tests/test_ctc_host.py), exact zeros, exact equalities between the forms and the states-per-thread instantiations, device-side lengths
beyond the tensor extents inside guarded views, both dtypes of the log-softmax kernels element by element, and the greedy decode's
first-maximum and collapse rules.  Every test prints the largest ratio it reached before it asserts.

Measured on an MI355X, largest ratio per case (nll of K_NLL = 1.34 units | gradient of K_GRAD = 8 units | fp16-lattice gradient of
K_GRAD_H16 = 2840 units); the two fp32 forms are bit-identical, so they share a column:

    mixed        0.413 | 2.75 | 193      edges_len    0.000 | 0.81 | 0.81
    peaked       0.073 | 2.24 | 203      edges_n1     0.148 | 0.76 | 254
    peaked4      0.621 | 2.63 | 296      edges_c2     0.482 | 1.58 | 777
    single_path  0.543 | 2.16 | 613      edges_c5     0.174 | 1.55 | 406
    infeasible   0.049 | 1.80 | 293      wide         0.348 | 2.34 | 624   (the same at Smax = 261, 769, 2049)

log-softmax: forward 0.61 (fp32 input) / 0.65 (bf16 input), backward 0.99 (fp32 output) of the K_LSM = 2 counted units -- the emulation's
own figures to the digit; exp2(0) = 1 and log2(1) = 0 are exact on the hardware (single_path holds bit for bit)."""
import numpy as np
import pytest
import torch

from tests import ctc_ref as R

pytestmark = pytest.mark.gpu

FORMS = ("sep", "ab", "h16")  # ocrs_ctc_fwd + _bwd, ocrs_ctc_fwd_ab + ocrs_ctc_grad_ab, ocrs_ctc_fwd_h16 + ocrs_ctc_bwd_h16
GUARD = 4096   # bytes of sentinel on either side of a guarded view
SENTINEL = 0xA5


class Guarded:
    """device buffers as views in the middle of larger sentinel-filled allocations: a write outside a view lands in the guard, where
    check() sees it, and not in someone else's memory"""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def __call__(self, shape, dtype, fill):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.uint8, device=self.dev)
        view = raw[GUARD:GUARD + n].view(dtype).reshape(shape)
        view.fill_(fill)
        self.bufs.append((raw, n))
        return view

    def check(self):
        for raw, n in self.bufs:
            assert bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[GUARD + n:] == SENTINEL).all())


def plain(dev):
    return lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device=dev)


def run_ctc(dev, form, c, Smax=None, gout=1.0, il=None, tl=None, alloc=None):
    """one forward + backward of a form through the C ABI -> nll (N,), loss (), grad (T, N, C) as float32 numpy.  Every output and workspace is
    NaN before the launch: a value the kernels do not write, or a lattice entry they read without having written it, shows."""
    from ocrs_models_amd._lib import lib, ptr

    L = lib()
    alloc = alloc or plain(dev)
    T, N, C = c["lp"].shape
    Lpad = c["targets"].shape[1]
    Smax = Smax or 2 * int(c["tl"].max()) + 1
    lp = torch.from_numpy(np.array(c["lp"])).to(dev)
    tg = torch.from_numpy(np.array(c["targets"])).to(dev)
    ild = torch.tensor(np.array(c["il"] if il is None else il), dtype=torch.int64).to(dev)
    tld = torch.tensor(np.array(c["tl"] if tl is None else tl), dtype=torch.int64).to(dev)
    nan = float("nan")
    nll, loss, grad = alloc((N,), torch.float32, nan), alloc((1,), torch.float32, nan), alloc((T, N, C), torch.float32, nan)
    g = torch.tensor([gout], dtype=torch.float32, device=dev)
    dims = (T, N, C, Lpad, Smax)
    if form == "sep":
        alpha = alloc((N, T, Smax), torch.float32, nan)
        L.ctc_fwd(ptr(lp), ptr(tg), ptr(ild), ptr(tld), ptr(alpha), ptr(nll), ptr(loss), *dims)
        L.ctc_bwd(ptr(lp), ptr(tg), ptr(ild), ptr(tld), ptr(alpha), ptr(nll), ptr(g), ptr(grad), *dims)
    elif form == "ab":
        alpha, beta = alloc((N, T, Smax), torch.float32, nan), alloc((N, T, Smax), torch.float32, nan)
        L.ctc_fwd_ab(ptr(lp), ptr(tg), ptr(ild), ptr(tld), ptr(alpha), ptr(beta), ptr(nll), ptr(loss), *dims)
        L.ctc_grad_ab(ptr(lp), ptr(tg), ptr(ild), ptr(tld), ptr(alpha), ptr(beta), ptr(nll), ptr(g), ptr(grad), *dims)
    else:
        alpha, rowmax = alloc((N, T, Smax), torch.float16, nan), alloc((N, T), torch.float32, nan)
        L.ctc_fwd_h16(ptr(lp), ptr(tg), ptr(ild), ptr(tld), ptr(alpha), ptr(rowmax), ptr(nll), ptr(loss), *dims)
        L.ctc_bwd_h16(ptr(lp), ptr(tg), ptr(ild), ptr(tld), ptr(alpha), ptr(rowmax), ptr(nll), ptr(g), ptr(grad), *dims)
    torch.cuda.synchronize()
    return nll.cpu().numpy(), float(loss.cpu()[0]), grad.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def check_against_float64(name, form, c, ref, nll, loss, grad, tag=""):
    """every sample's nll and every gradient element against their bounds; +inf where the reference has it; exact zeros; the mean loss"""
    T, N, C = c["lp"].shape
    rn, rg = R.ctc_ratios(nll, grad, ref)
    kg = R.K_GRAD_H16 if form == "h16" else R.K_GRAD
    print(f"ctc {name}{tag} [{form}]: nll {rn.max():.3f} of {R.K_NLL} units, gradient {rg.max():.2f} of {kg} units")
    assert np.array_equal(np.isinf(nll), np.isinf(ref["nll"])) and not np.isnan(nll).any() and (nll[np.isinf(nll)] > 0).all()
    assert (rn <= R.K_NLL).all(), (name, form, rn)
    assert np.isfinite(grad).all()
    assert (rg <= kg).all(), (name, form, rg)
    for n in range(N):
        assert not grad[max(int(c["il"][n]), 0):, n].any(), (name, form, n)  # rows t >= T_n: exactly 0
    per = ref["nll"] / np.maximum(c["tl"], 1)
    if np.isinf(per).any():
        assert loss == np.inf
    else:
        # k_ctc_reduce: a division per sample, a 6-level wave tree, 3 additions, the division by N: 12 roundings of the mean magnitude
        bound = float(np.mean(R.K_NLL * ref["nll_unit"] / np.maximum(c["tl"], 1))) + 12 * R.U * float(np.mean(np.abs(per)))
        assert abs(loss - ref["loss"]) <= bound, (name, form, loss, ref["loss"], bound)


@pytest.mark.parametrize("name", R.CASES)
def test_ctc_three_forms_per_sample_against_float64(dev, name):
    c, ref = R.case(name), R.case_ref(name)
    T, N, C = c["lp"].shape
    out = {form: run_ctc(dev, form, c) for form in FORMS}
    for form in FORMS:
        check_against_float64(name, form, c, ref, *out[form])
    assert same_bits(out["sep"][0], out["ab"][0]) and same_bits(out["sep"][0], out["h16"][0])  # nll: the same recursion in all three
    assert same_bits(out["sep"][2], out["ab"][2])                                            # gradient: the two fp32 forms
    assert out["sep"][1] == out["ab"][1] == out["h16"][1]
    for form in FORMS:
        for gout in (2.0, 0.5):  # the upstream gradient is one exact factor
            _, _, g = run_ctc(dev, form, c, gout=gout)
            assert same_bits(g, out[form][2] * np.float32(gout)), (form, gout)
    if name == "single_path":
        # one alignment: every lse3 on it sees (x, -inf, -inf) and must return x -- exp2(0) = 1 and log2(1) = 0 exactly on the hardware --, so
        # nll is the float32 sum of the path's log-probs in time order, bit for bit
        for n in range(N):
            want, _ = R.sequential_nll32(c["lp"][:, n], c["targets"][n, : int(c["tl"][n])], int(c["il"][n]))
            assert out["sep"][0][n].tobytes() == want.tobytes(), (n, out["sep"][0][n], want)
    if name == "infeasible":
        bad = R.INFEASIBLE[name][0]
        Ti = int(c["il"][bad])
        want = np.exp(c["lp"][:Ti, bad].astype(np.float64)) / (N * int(c["tl"][bad]))  # the documented departure from ATen's NaN
        for form in FORMS:
            nll, loss, grad = out[form]
            assert loss == np.inf and nll[bad] == np.inf
            assert (np.abs(grad[:Ti, bad] - want) <= R.K_GRAD * R.U * want).all() and not grad[Ti:, bad].any()
        # (the fp16 form has no lattice entry to round here: its exp(lp) * scale is the fp32 form's)
        assert same_bits(out["h16"][2][:, bad], out["sep"][2][:, bad])
        twin = R.infeasible_made_feasible()
        others = [n for n in range(N) if n != bad]
        for form in FORMS:
            nll2, loss2, _ = run_ctc(dev, form, twin)
            assert np.isfinite(nll2).all() and np.isfinite(loss2)
            assert same_bits(nll2[others], out[form][0][others])  # a sample beside an infeasible one does not feel it


def test_ctc_wide_lattice_states_per_thread(dev):
    """S = 261 > 256 states: more than one state per thread and the thread 255 / 256 seam; Smax = 261, 769 and 2049 select the 3-, 8- and
    16-states-per-thread instantiations of every kernel, which must agree bit for bit"""
    c, ref = R.case("wide"), R.case_ref("wide")
    for form in FORMS:
        outs = {}
        for Smax in (261, 769, 2049):
            outs[Smax] = run_ctc(dev, form, c, Smax=Smax)
            check_against_float64("wide", form, c, ref, *outs[Smax], tag=f" Smax={Smax}")
        for Smax in (769, 2049):
            assert same_bits(outs[Smax][0], outs[261][0]) and same_bits(outs[Smax][2], outs[261][2]) and outs[Smax][1] == outs[261][1], (form, Smax)


@pytest.mark.parametrize("name", ["mixed", "peaked"])
@pytest.mark.parametrize("h16", [False, True])
def test_ctcloss_with_device_lengths_equals_host_lengths(dev, name, h16):
    """CTCLoss takes lengths that live on the device, sizes the lattice from the padding instead of the real lengths (no sync), and the
    kernels clamp: loss and gradient are those of the host-length call, bit for bit"""
    import ocrs_models_amd as oa

    c = R.case(name)
    lp = torch.from_numpy(np.array(c["lp"])).to(dev)
    tg = torch.from_numpy(np.array(c["targets"])).to(dev)
    il, tl = torch.from_numpy(np.array(c["il"])), torch.from_numpy(np.array(c["tl"]))
    fn = oa.CTCLoss(lattice_dtype=torch.float16 if h16 else torch.float32)
    res = []
    for lengths in ((il, tl), (il.to(dev), tl.to(dev)), (il.to(dev), tl)):
        x = lp.clone().requires_grad_(True)
        loss = fn(x, tg, *lengths)
        loss.backward()
        res.append((loss.detach().clone(), x.grad.clone()))
    assert torch.isfinite(res[0][0]) and torch.isfinite(res[0][1]).all()
    for other in res[1:]:
        assert torch.equal(other[0], res[0][0]) and torch.equal(other[1], res[0][1])


@pytest.mark.parametrize("form", FORMS)
def test_ctc_device_lengths_beyond_the_extents_are_clamped(dev, form):
    """T_n > T, L_n > Lpad, 2 L_n + 1 > Smax and negative lengths through the C ABI: the result -- nll, mean loss, gradient -- is that of the
    call with the clamped lengths, and nothing is written outside alpha, beta / rowmax, nll, loss or grad, which are views inside guards"""
    r = np.random.RandomState(41)
    T, N, C, Lpad, Smax = 9, 6, 5, 4, 7  # Smax = 7 holds L <= 3 < Lpad
    tg = np.array([R.labels_no_repeat(r, Lpad, C) for _ in range(N)])
    c = R.make_case("clamp", 41, 3 * r.randn(T, N, C), tg, [9, 9, 0, 5, 9, 7], [2, 3, 0, 0, 3, 3])
    raw_il, raw_tl = [12, 9, -3, 5, 100, 7], [2, 9, -1, -2, 4, 3]
    assert list(np.clip(raw_il, 0, T)) == list(c["il"]) and list(np.minimum(np.clip(raw_tl, 0, Lpad), (Smax - 1) // 2)) == list(c["tl"])
    ref = R.ctc_batch64(c)
    want = run_ctc(dev, form, c, Smax=Smax)
    check_against_float64("clamp", form, c, ref, *want)
    assert np.isfinite(want[1])
    guard = Guarded(dev)
    got = run_ctc(dev, form, c, Smax=Smax, il=raw_il, tl=raw_tl, alloc=guard)
    guard.check()
    assert same_bits(got[0], want[0]) and same_bits(got[2], want[2]) and got[1] == want[1], (got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# log-softmax
# ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", [0, 1])
def test_log_softmax_forward_backward_every_element(dev, dtype, padded):
    """k_log_softmax<float / bf16> and k_log_softmax_bwd<float / bf16> (dtype 1 is exported and used by nothing else): every element within
    K_LSM counted units of float64; pad columns that hold 1e30 influence nothing and come back 0 from the backward"""
    from ocrs_models_amd._lib import lib, ptr

    tdt = torch.bfloat16 if dtype else torch.float32
    worst_f = worst_b = 0.0
    for rows in R.LSM_ROWS:
        for C in R.LSM_C:
            c = R.lsm_case(rows, C, bool(dtype))
            ld = (C + 31) // 32 * 32 if padded else C
            x = torch.full((rows, ld), R.LSM_PAD, dtype=tdt, device=dev)
            x[:, :C] = torch.from_numpy(np.array(c["x"])).to(dev).to(tdt)
            assert torch.equal(x[:, :C].float().cpu(), torch.from_numpy(np.array(c["x"])))  # (bf16 cases are bf16-exact)
            out = torch.full((rows, C), float("nan"), device=dev)
            lib().log_softmax_fwd(ptr(x), ptr(out), rows, C, ld, dtype)
            lp = out.cpu().numpy()
            out64, unit = R.lsm_fwd_ref(c["x"])
            inf = np.isinf(out64)
            assert not np.isnan(lp).any() and np.array_equal(lp == -np.inf, inf), (rows, C)
            if (~inf).any():
                rf = float((np.abs(lp[~inf].astype(np.float64) - out64[~inf]) / unit[~inf]).max())
                worst_f = max(worst_f, rf)
                assert rf <= R.K_LSM, (rows, C, rf)
            # backward from the kernel's own log-probs
            g = torch.from_numpy(np.array(c["g"])).to(dev)
            dl = torch.full((rows, ld), float("nan"), dtype=tdt, device=dev)
            lib().log_softmax_bwd(ptr(out), ptr(g), ptr(dl), rows, C, ld, dtype)
            d = dl.float().cpu().numpy().astype(np.float64)
            assert not d[:, C:].any() and not np.isnan(d).any(), (rows, C)  # pad columns: exactly 0
            d64, bunit = R.lsm_bwd_ref(lp, c["g"])
            err = np.abs(d[:, :C] - d64)
            if dtype:
                err = np.maximum(err - 0.5 * R.ulp_bf16(d64), 0.0)  # the stored value: + half a bf16 ulp of the float64 one
            rb = float((err / bunit).max())
            worst_b = max(worst_b, rb)
            assert rb <= R.K_LSM, (rows, C, rb)
    print(f"log-softmax dtype {dtype} {'ld = C up to 32' if padded else 'ld = C'}: forward {worst_f:.3f}, backward {worst_b:.3f} of {R.K_LSM} units")


# ---------------------------------------------------------------------------------------------------------------------------------------
# greedy decode
# ---------------------------------------------------------------------------------------------------------------------------------------

def decode(dev, lp, il):
    from ocrs_models_amd._lib import lib, ptr

    T, N, C = lp.shape
    lpd = torch.from_numpy(lp).to(dev)
    ild = torch.tensor(list(il), dtype=torch.int64).to(dev)
    amax = torch.full((N, T), -7, dtype=torch.int32, device=dev)
    labels = torch.full((N, T), -7, dtype=torch.int32, device=dev)
    lens = torch.full((N,), -7, dtype=torch.int32, device=dev)
    lib().ctc_greedy_decode(ptr(lpd), ptr(ild), ptr(amax), ptr(labels), ptr(lens), T, N, C)
    torch.cuda.synchronize()
    return amax.cpu().numpy(), labels.cpu().numpy(), lens.cpu().numpy()


@pytest.mark.parametrize("C", [1, 5, 16, 17, 97])
def test_argmax_is_the_first_maximum(dev, C):
    r = np.random.RandomState(C)
    T, N = (117, 1) if C == 97 else (7, 5)  # 117 / 35 rows: no multiple of the 16 rows of a block
    lp = r.randn(T, N, C).astype(np.float32)
    rows = lp.reshape(T * N, C)
    k = 0
    if C == 97:
        for cls in range(C):  # the maximum on every class in turn: every lane, every trip of the strided loop
            rows[k, cls] = 9
            k += 1
    planted = []
    for a, b in [(1, 3), (2, 4), (0, C - 1), (0, 16), (5, 21), (3, 19), (64, 80), (80, 96)]:  # ties across lanes, and c / c + 16 in ONE lane
        if a < b < C:
            rows[k, a] = rows[k, b] = 9
            planted.append((k, a))
            k += 1
    rows[k] = 0.25  # a constant row: class 0
    planted.append((k, 0))
    k += 1
    for only in sorted({0, C // 2, C - 1}):  # -inf but for one entry
        rows[k] = -np.inf
        rows[k, only] = -3
        planted.append((k, only))
        k += 1
    if C > 1:
        rows[k] = -np.inf  # and a tie of two among -inf
        rows[k, [C - 2, C - 1]] = -1
        planted.append((k, C - 2))
        k += 1
    assert k <= T * N
    want = R.first_argmax(lp)
    for row, cls in planted:
        assert want[row % N, row // N] == cls
    amax, _, _ = decode(dev, lp, [T] * N)
    assert np.array_equal(amax, want)


@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_collapse_rule_lengths_and_untouched_tail(dev, N):
    from oracle.text import greedy_collapse

    r = np.random.RandomState(N)
    T, C = 9, 5
    want = r.randint(0, 3, (N, T))  # classes 0..2: plenty of repeats and blanks
    want[0] = [1, 1, 0, 1, 2, 2, 0, 0, 0]  # "a a blank a b b"
    il = [(0, 1, T, T + 5, 4, T)[n % 6] for n in range(N)]
    il[0] = 6
    if N > 1:
        want[1], il[1] = 0, T  # an all-blank row
    lp = R.plant_argmax(r, want, C)
    amax, labels, lens = decode(dev, lp, il)
    assert np.array_equal(amax, want)
    for n in range(N):
        exp = greedy_collapse(want[n, : min(il[n], T)].tolist())
        assert exp == R.collapse(want[n], min(il[n], T))
        assert lens[n] == len(exp) and labels[n, : len(exp)].tolist() == exp, n
        assert (labels[n, len(exp):] == -7).all(), n  # beyond lens[n]: untouched
    assert labels[0, :3].tolist() == [1, 1, 2] and lens[0] == 3
    if N > 1:
        assert lens[1] == 0

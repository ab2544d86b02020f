"""Device character error rate (csrc/rec_cer.hip) against the CPU oracle and against the host RecognitionAccuracyStats.
Integers only: every comparison in this file is exact equality."""
import numpy as np
import pytest
import torch

from oracle import text as otext
from tests.golden_util import REC_CASE, load_meta, load_npz, rec_samples

pytestmark = pytest.mark.gpu

A_LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 500, 2047)
B_LENS = (0, 1, 63, 64, 65, 101, 500, 2048)
SAME_LENS = (0, 1, 64, 65, 129, 2047)  # identical sequences


def _pairs(r, K):
    """every (m, n) of A_LENS x B_LENS with labels in [1, K], plus identical pairs"""
    out = [(r.randint(1, K + 1, size=m), r.randint(1, K + 1, size=n)) for m in A_LENS for n in B_LENS]
    for m in SAME_LENS:
        a = r.randint(1, K + 1, size=m)
        out.append((a, a.copy()))
    return out


def _pack(r, rows, pitch):
    """label rows -> (N, pitch) int32 with NON-ZERO garbage beyond each length, lengths"""
    M = r.randint(1, 97, size=(len(rows), pitch)).astype(np.int32)
    for i, row in enumerate(rows):
        M[i, : len(row)] = row
    return torch.from_numpy(M), [len(row) for row in rows]


@pytest.mark.parametrize("K", [2, 96])
def test_edit_distance_matches_oracle(dev, K):
    import ocrs_models_amd as oa

    r = np.random.RandomState(100 + K)
    pairs = _pairs(r, K)
    assert (0, 0) in [(len(a), len(b)) for a, b in pairs] and len(pairs) == len(A_LENS) * len(B_LENS) + len(SAME_LENS)
    a, a_len = _pack(r, [p[0] for p in pairs], 2047 + 9)   # pitches larger than every length
    b, b_len = _pack(r, [p[1] for p in pairs], 2048 + 40)
    got = oa.text.edit_distance_device(a.to(dev), a_len, b.to(dev), torch.tensor(b_len))
    assert got.dtype == torch.int32 and got.is_cuda
    want = [otext.levenshtein(x.tolist(), y.tolist()) for x, y in pairs]
    got = got.cpu().tolist()
    bad = [(len(x), len(y), g, w) for (x, y), g, w in zip(pairs, got, want) if g != w]
    print(f"K={K}: {len(pairs)} pairs, {len(bad)} differ")
    assert not bad, bad[:10]
    # the same pairs with the roles swapped (long rows <-> many passes) and device-side lengths
    got = oa.text.edit_distance_device(b.to(dev), torch.tensor(b_len).to(dev), a.to(dev), torch.tensor(a_len).to(dev)).cpu().tolist()
    assert got == want


def test_edit_distance_codes_table_merges_ids(dev):
    import ocrs_models_amd as oa

    r = np.random.RandomState(7)
    codes = [0, 1, 1, 3]  # ids 1 and 2 are the same character
    rows_a = [r.randint(1, 4, size=m) for m in (0, 1, 5, 64, 65, 130, 300)]
    rows_b = [r.randint(1, 4, size=n) for n in (3, 1, 0, 65, 64, 129, 301)]
    a, a_len = _pack(r, rows_a, 320)
    b, b_len = _pack(r, rows_b, 333)
    got = oa.text.edit_distance_device(a.to(dev), a_len, b.to(dev), b_len, codes=torch.tensor(codes, dtype=torch.int32, device=dev)).cpu().tolist()
    want = [otext.levenshtein([codes[v] for v in x], [codes[v] for v in y]) for x, y in zip(rows_a, rows_b)]
    plain = [otext.levenshtein(x.tolist(), y.tolist()) for x, y in zip(rows_a, rows_b)]
    assert got == want and want != plain
    assert oa.text.edit_distance_device(a.to(dev), a_len, b.to(dev), b_len).cpu().tolist() == plain


def test_golden_batch_counters_and_distances(dev):
    import ocrs_models_amd as oa

    G, meta = load_npz("rec.npz"), load_meta()
    batch = oa.text.collate_samples(rec_samples(REC_CASE))
    il = batch["image_width"].div(4, rounding_mode="floor")
    lp = torch.from_numpy(G["rec1/f32/log_probs"]).to(dev)
    stats = oa.text.DeviceRecognitionAccuracyStats()
    stats.update(batch["text_seq"], batch["text_len"].tolist(), lp, il.tolist())
    assert stats.char_errors == meta["rec1/f32/char_errors"] and stats.total_chars == meta["rec1/f32/total_chars"]
    targets = [otext.decode_labels(row) for row in batch["text_seq"].numpy()]
    want = [otext.levenshtein(t, d) for t, d in zip(targets, meta["rec1/f32/decoded"])]
    assert stats.last_dist.cpu().tolist() == want
    assert stats.char_error_rate() == meta["rec1/f32/char_errors"] / meta["rec1/f32/total_chars"]
    assert stats.stats_dict() == {"char_error_rate": stats.char_error_rate()}


def _random_batch(r, T, N, C, Lpad):
    """log-probs with boosted blanks and forced repeats; input lengths with 0, 1 and values above T; targets with interior zeros and
    target_lengths that differ from the non-zero count"""
    x = r.randn(T, N, C).astype(np.float32)
    x[..., 0] += 2.5 * (r.uniform(size=(T, N)) < 0.3)
    rep = r.uniform(size=(T, N)) < 0.3
    for t in range(1, T):
        x[t][rep[t]] = x[t - 1][rep[t]]
    lp = torch.from_numpy(x).log_softmax(-1)
    il = r.randint(0, T + 20, size=N)
    il[:4] = (0, 1, T, T + 7)
    tg = r.randint(1, C, size=(N, Lpad)).astype(np.int32)
    tg[r.uniform(size=(N, Lpad)) < 0.5] = 0  # zeros anywhere in the padded row
    tg[0] = 0
    tl = r.randint(0, Lpad + 1, size=N)
    return lp, il.tolist(), torch.from_numpy(tg), tl.tolist()


def test_device_stats_equal_host_stats(dev):
    import ocrs_models_amd as oa

    r = np.random.RandomState(5)
    host, device = oa.text.RecognitionAccuracyStats(), oa.text.DeviceRecognitionAccuracyStats()
    for i in range(3):
        lp, il, tg, tl = _random_batch(r, 101, 256, 97, 64)
        lp = lp.to(dev)
        host.update(tg, tl, lp, il)
        if i == 1:  # device-resident targets and length tensors
            device.update(tg.to(dev), torch.tensor(tl).to(dev), lp, torch.tensor(il).to(dev))
        else:
            device.update(tg, tl, lp, il)
        assert (tg.numpy() > 0).sum() != sum(tl)
    print("host", host.char_errors, host.total_chars, "device", device.char_errors, device.total_chars)
    assert host.char_errors > 0 and host.total_chars > 0
    assert device.char_errors == host.char_errors and device.total_chars == host.total_chars
    assert device.char_error_rate() == host.char_error_rate()


def test_duplicate_character_alphabet(dev):
    import ocrs_models_amd as oa

    r = np.random.RandomState(9)
    host, device = oa.text.RecognitionAccuracyStats("aab"), oa.text.DeviceRecognitionAccuracyStats("aab")
    plain = oa.text.DeviceRecognitionAccuracyStats("abc")
    lp, il, tg, tl = _random_batch(r, 80, 64, 4, 70)
    lp = lp.to(dev)
    for s in (host, device, plain):
        s.update(tg, tl, lp, il)
    assert device.char_errors == host.char_errors and device.total_chars == host.total_chars
    assert plain.char_errors > device.char_errors  # the table matters on this batch


def test_update_is_graph_capturable(dev):
    import ocrs_models_amd as oa

    r = np.random.RandomState(11)
    batches = [_random_batch(r, 101, 64, 97, 64) for _ in range(3)]
    _, il, tg, tl = batches[0]
    tg_d, tl_d, il_d = tg.to(dev), torch.tensor(tl).to(dev), torch.tensor(il).to(dev)
    host, device = oa.text.RecognitionAccuracyStats(), oa.text.DeviceRecognitionAccuracyStats()
    static_lp = batches[0][0].to(dev)
    device.update(tg_d, tl_d, static_lp, il_d)  # (creates the counters outside the capture)
    host.update(tg, tl, static_lp, il)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a device-to-host copy or a synchronisation inside the update would raise here
        device.update(tg_d, tl_d, static_lp, il_d)
    for lp, _, _, _ in batches[1:]:
        static_lp.copy_(lp.to(dev))
        graph.replay()
        host.update(tg, tl, static_lp, il)
    assert device.char_errors == host.char_errors and device.total_chars == host.total_chars and host.char_errors > 0


def _rec_batches(seed, n):
    import ocrs_models_amd as oa

    r = np.random.RandomState(seed)
    out = []
    for k in range(n):
        samples = []
        for w, L in ((72, 5), (128, 12), (200, 20), (256, 9)):
            seq = r.randint(1, 97, size=L).astype(np.int32)
            img = r.uniform(-0.5, 0.5, (1, 64, w)).astype(np.float32)
            samples.append({"image": torch.from_numpy(img), "text_seq": torch.from_numpy(seq)})
        out.append(oa.text.collate_samples(samples))
    return out


def _model(dev):
    import ocrs_models_amd as oa
    from oracle.params import make_state, recognition_specs, state_dict_from

    specs = recognition_specs()
    P, Bf = make_state(specs, 31)
    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    m.load_state_dict(state_dict_from(P, Bf, specs))
    return m.to(dev)


def test_train_and_test_loops_host_vs_device(dev):
    from ocrs_models_amd import text, train_rec

    res = {}
    for mode in ("host", "device"):
        m = _model(dev)
        opt = train_rec.make_optimizer(m)
        loss, stats = train_rec.train(0, dev, _rec_batches(41, 3), m, opt, stats=mode)
        vloss, vstats = train_rec.test(dev, _rec_batches(42, 2), m, preview=0, stats=mode)
        assert type(stats) is type(vstats) is (text.DeviceRecognitionAccuracyStats if mode == "device" else text.RecognitionAccuracyStats)
        res[mode] = (loss, vloss, stats.char_errors, stats.total_chars, vstats.char_errors, vstats.total_chars,
                     [p.detach().cpu().clone() for p in m.parameters()])
    h, d = res["host"], res["device"]
    print("host", h[:6], "device", d[:6])
    assert h[:6] == d[:6] and h[3] > 0
    assert all(torch.equal(a, b) for a, b in zip(h[6], d[6]))
    # the default is the host class
    m = _model(dev)
    assert type(train_rec.test(dev, _rec_batches(42, 1), m, preview=0)[1]) is text.RecognitionAccuracyStats


def test_non_finite_loss_raises_the_same_exception(dev, monkeypatch):
    """A step whose loss is NaN: the host mode raises inside that step, the device mode counts it and raises the same exception when the
    epoch ends.  (The loss is poisoned behind the CTC kernel, so the test does not depend on how a kernel propagates NaN inputs.)"""
    import ocrs_models_amd as oa
    from ocrs_models_amd import train_rec

    class PoisonedCTC(oa.CTCLoss):
        calls, poison = 0, float("nan")

        def forward(self, *args):
            loss = super().forward(*args)
            PoisonedCTC.calls += 1
            return loss + PoisonedCTC.poison if PoisonedCTC.calls == 2 else loss

    monkeypatch.setattr(train_rec, "CTCLoss", PoisonedCTC)
    msgs = {}
    for mode, poison, steps_run in (("host", float("nan"), 2), ("device", float("nan"), 3), ("device-inf", float("inf"), 3)):
        PoisonedCTC.calls, PoisonedCTC.poison = 0, poison
        m = _model(dev)
        opt = train_rec.make_optimizer(m)
        with pytest.raises(Exception) as ei:
            train_rec.train(0, dev, _rec_batches(43, 3), m, opt, stats=mode.split("-")[0])
        assert type(ei.value) is Exception and PoisonedCTC.calls == steps_run
        msgs[mode] = str(ei.value)
    assert set(msgs.values()) == {"Training produced invalid loss. Check input and target lengths are compatible with CTC loss"}
    # a clean epoch does not raise
    PoisonedCTC.calls = 10
    m = _model(dev)
    train_rec.train(0, dev, _rec_batches(43, 2), m, train_rec.make_optimizer(m), stats="device")

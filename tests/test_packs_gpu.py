"""The per-step weight-fragment pack table (ocrs_models_amd/packs.py) of the three model drivers: every row a run lists is found again by
the same row, holds the bytes a single ocrs_pack_frags of that row writes, and the table lives on the module until a parameter moves."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _params(m):
    return {k: p.detach() for k, p in m.named_parameters()}


def _det(dev, dtype):
    import ocrs_models_amd as oa
    from ocrs_models_amd.models import _DetRun

    m = oa.DetectionModel().to(dev)

    def run():
        r = _DetRun(_params(m), dict(m.named_buffers()), dev, dtype, 2, mod=m)
        return r, r.pack_rows, r.prepack
    return m, "up.0.up.weight", run


def _rec(dev, dtype, train):
    import ocrs_models_amd as oa
    from ocrs_models_amd.recognition import _RecRun

    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
    m._gru_flatten()

    def run():
        r = _RecRun(_params(m), dict(m.named_buffers()), dev, dtype, 2, 64, 64, train=train, mod=m)
        return r, r.pack_rows, r.prepack
    return m, "conv.3.weight", run


def _layout(dev, x3, need_dgrad):
    import ocrs_models_amd as oa
    from ocrs_models_amd.layout import _LayoutRun

    m = oa.LayoutModel().to(dev)
    boxes = torch.zeros(1, 2, 4, device=dev)

    def run():
        P = _params(m)
        r = _LayoutRun(m, boxes, list(P), list(P.values()), need_dgrad, x3, 0.0, 0)
        return r, lambda: r.pack_rows(need_dgrad), lambda: r.prepack(need_dgrad)
    return m, "encode.layers.1.linear1.weight", run


CASES = {"det-bf16": (_det, BF16), "det-fp32": (_det, F32),
         "rec-fp32-train": (_rec, F32, True), "rec-fp32-eval": (_rec, F32, False),
         "rec-bf16-x3-train": (_rec, BF16, True), "rec-bf16-x3-eval": (_rec, BF16, False),
         "rec-bf16-nox3-train": (_rec, BF16, True), "rec-bf16-nox3-eval": (_rec, BF16, False),
         "layout-x3-dgrad": (_layout, True, True), "layout-x3": (_layout, True, False),
         "layout-parity-dgrad": (_layout, False, True), "layout-parity": (_layout, False, False)}


def _check(run):
    """prepack a fresh run; every row of pack_rows() is in the table and byte-equal to its own single pack"""
    from ocrs_models_amd.packs import pack_one

    r, pack_rows, prepack = run()
    prepack()
    rows = pack_rows()
    assert rows and len({row.key() for row in rows}) == len(rows)
    for row in rows:
        hit = r.packs.get(row)
        assert hit is not None, row[1:]
        assert torch.equal(hit, pack_one(row, r.dev)), row[1:]
    return r.packs


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_a_detection_step_takes_every_pack_from_the_table(dev, dtype, monkeypatch):
    """A lookup that misses the table packs its own copy each step and computes the same numbers: only the launch count shows it.  One train
    step at 2 x 64 x 64: one ocrs_pack_frags_multi, no single ocrs_pack_frags."""
    import ocrs_models_amd as oa
    from ocrs_models_amd._lib import lib

    torch.manual_seed(5)
    m = oa.DetectionModel(act_dtype=dtype).to(dev).train()
    x = torch.rand(2, 1, 64, 64, device=dev) - 0.5
    mask = (torch.rand(2, 1, 64, 64, device=dev) > 0.9).float()
    rec = {"pack_frags": [], "pack_frags_multi": []}
    monkeypatch.setattr(lib(), "timing", rec)
    oa.balanced_cross_entropy_loss(m(x), mask).backward()
    torch.cuda.synchronize()
    assert len(rec["pack_frags_multi"]) == 1 and not rec["pack_frags"]


@pytest.mark.parametrize("case", list(CASES))
def test_every_listed_row_is_in_the_table_with_the_bytes_of_a_single_pack(dev, case, monkeypatch):
    make, *args = CASES[case]
    monkeypatch.setenv("OCRS_GRU_X3", "0" if "nox3" in case else "1")
    torch.manual_seed(11)
    m, moved, run = make(dev, *args)
    table = _check(run)
    assert _check(run).buf is table.buf  # unchanged parameters: the cached table, packed again into the same buffer
    p = dict(m.named_parameters())[moved]
    p.data = p.data.clone()
    rebuilt = _check(run)
    assert rebuilt is not table and rebuilt.buf is not table.buf

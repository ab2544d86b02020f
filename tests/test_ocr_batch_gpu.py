"""Page batches on the GPU (inference.detect_words_batch, find_lines_pages, rectify_crops_pages, ocr_pages and the kernels of the C
ABI section "page batches") against the single-page path, which tests/test_ocr_gpu.py and tests/test_lines_gpu.py pin.

Every comparison is ``torch.equal`` / ``==`` with one exception: the batched eval forward against the single one
(test_batched_forward_against_single_forward), bounded by 1e-4, the project's output parity bound for the fp32 path.  That is why the driver
tests start from the batch's own ``probs``.  For B > 1 the recognised strings are compared with hand-chained POOLED batches, never with
per-page ``ocr_lines``: a crop's chunk, and so the padded width the BiGRU runs over, depends on the other pages' crops."""
import numpy as np
import pytest
import torch

from tests import lines_ref as LR
from tests import ocr_ref as R
from tests.test_lines_gpu import _count_waits, _golden_state, bar_page, dot_page

pytestmark = pytest.mark.gpu

SIZE = (160, 120)  # detection size of the driver tests
PAGE_SIZES = [(320, 240), (200, 160), (256, 384), (97, 131)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def det_model(dev):
    import ocrs_models_amd as oa

    m = oa.DetectionModel()
    m.load_state_dict(_golden_state("det"))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def rec_model(dev):
    import ocrs_models_amd as oa

    m = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET)
    m.load_state_dict(_golden_state("rec"))
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def pages(dev):
    """the four fixture pages; the all-white one sits in the middle of the batch (it has no words under BlankAware, see there)"""
    return [dot_page(320, 240).to(dev), torch.full((1, 200, 160), 255, dtype=torch.uint8, device=dev), dot_page(256, 384, step=20, size=7).to(dev),
            dot_page(97, 131).to(dev)]


class NeverCalled(torch.nn.Module):
    def forward(self, x):
        raise AssertionError("the recogniser must not run for a batch without words")


class BlankAware(torch.nn.Module):
    """The golden detector, with the probabilities of a page that has no contrast set to 0.  The golden weights are not trained: on the
    all-white fixture page they report several hundred components (351 at this size), so on their own no page of the batch would be without
    words.  The rule is per page and does not look at the batch, so the single-page functions run with this module are still the comparand."""

    def __init__(self, det):
        super().__init__()
        self.det = det

    def forward(self, x):
        flat = x.flatten(1)
        keep = (flat.amax(1) - flat.amin(1)) > 1e-3
        return self.det(x) * keep.to(x.dtype)[:, None, None, None]


class PaintedBatch(torch.nn.Module):
    """a detector that returns fixed probability maps (B,1,h,w), whatever the pages"""

    def __init__(self, probs):
        super().__init__()
        self.probs = probs

    def forward(self, x):
        assert tuple(x.shape) == (self.probs.shape[0], 1, *self.probs.shape[-2:])
        return self.probs[:, None]


def _sizes_d(sizes, dev):
    return torch.tensor(sizes, dtype=torch.int32, device=dev)


def _dirty_allocator(nbytes, dev):
    """leave a freed block of 0xFF bytes of this size in the caching allocator, so that an output that is allocated next and not fully written
    shows it"""
    t = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)
    del t


# ------------------------------------------------------------------ 1. masks ------------------------------------------------------------
def _check_canvas(dev, prob, sizes, canvas, threshold=0.5):
    from ocrs_models_amd import inference as inf

    B = len(sizes)
    _dirty_allocator(B * canvas[0] * canvas[1], dev)
    got = inf.binarize_resize_pages(prob, _sizes_d(sizes, dev), canvas, threshold)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, *canvas)
    inside = torch.zeros_like(got, dtype=torch.bool)
    for p, (H, W) in enumerate(sizes):
        assert torch.equal(got[p, :H, :W], inf.binarize_resize(prob[p], (H, W), threshold)), p
        inside[p, :H, :W] = True
    assert int(got[~inside].max().item() if (~inside).any() else 0) == 0  # every byte outside the regions
    return got


def test_masks_of_all_pages_equal_each_pages_own_mask(dev):
    g = torch.Generator().manual_seed(3)
    prob = torch.rand(4, 37, 29, generator=g)
    prob[:, ::5, ::3] = 0.5  # values on the threshold are background (strict >)
    prob = prob.to(dev)
    canvas = (max(h for h, _ in PAGE_SIZES), max(w for _, w in PAGE_SIZES))
    got = _check_canvas(dev, prob, PAGE_SIZES, canvas)
    assert 0 < int(got.sum()) < got.numel()
    _check_canvas(dev, prob, PAGE_SIZES, (333, 401), 0.8125)  # a canvas larger than every page, odd on both axes
    # B = 1 without padding; 97 * 131 is no multiple of 16: the tail of the last lane
    _check_canvas(dev, prob[3:], PAGE_SIZES[3:], PAGE_SIZES[3])
    _check_canvas(dev, prob[:1], PAGE_SIZES[:1], PAGE_SIZES[0])
    # rows shorter than a lane's 16 bytes: one lane crosses several rows and a page boundary
    _check_canvas(dev, prob[:3], [(3, 5), (5, 7), (1, 1)], (5, 7))


# ------------------------------------------------------------------ 2. quads through the padded canvas -------------------------------------
def _bar_probs(dev):
    """hand-made bars on a 40 x 30 probability grid, a different number per page and none on page 1"""
    prob = np.zeros((4, 40, 30), np.float32)
    bars = {0: [(2 + 7 * c, 2 + 4 * r) for r in range(5) for c in range(4)], 1: [], 2: [(3 + 9 * c, 5 + 6 * r) for r in range(3) for c in range(3)],
            3: [(1, 1), (12, 20), (20, 33)]}
    for p, bs in bars.items():
        for x, y in bs:
            prob[p, y:y + 2, x:x + 5] = 0.9
    return torch.from_numpy(prob).to(dev), [len(b) for b in bars.values()]


def test_quads_through_the_padded_canvas_equal_each_pages_own(dev):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.postprocess import extract_cc_quads_device

    prob, want_counts = _bar_probs(dev)
    canvas = _check_canvas(dev, prob, PAGE_SIZES, (320, 384))
    flat, page_of_word, word_offs, counts = inf.cc_quads_pages(canvas)
    quads = inf.expand_quads(flat, 3.0)
    assert counts == want_counts and counts[1] == 0
    offs = word_offs.tolist()
    assert offs == [0] + np.cumsum(counts).tolist() and tuple(quads.shape) == (offs[-1], 4, 2)
    assert page_of_word.dtype == torch.int32 and page_of_word.tolist() == [p for p, c in enumerate(counts) for _ in range(c)]
    for p, (H, W) in enumerate(PAGE_SIZES):
        own = inf.expand_quads(extract_cc_quads_device(inf.binarize_resize(prob[p], (H, W))), 3.0)
        assert torch.equal(quads[offs[p]:offs[p + 1]], own), p
    # expansion before the gather (with counts) gives the same bytes as on the flat rows: one lane per quad either way
    raw = torch.zeros(4, 32, 4, 2, device=dev)
    for p in range(4):
        raw[p, :counts[p]] = flat[offs[p]:offs[p + 1]]
    ncomp = torch.tensor(counts, dtype=torch.int32, device=dev)
    before, _, offs2, counts2 = inf.gather_page_quads(inf.expand_quads(raw, 3.0, ncomp), ncomp)
    assert torch.equal(before, quads) and offs2.tolist() == offs and counts2 == counts


# ------------------------------------------------------------------ 3. lines ------------------------------------------------------------
def _flat(dev, per_page):
    """per-page numpy quads -> (flat device quads, page_of_word, word_offs, host offsets)"""
    offs = [0] + np.cumsum([len(q) for q in per_page]).tolist()
    quads = torch.from_numpy(np.concatenate([np.asarray(q, np.float32).reshape(-1, 4, 2) for q in per_page])).to(dev)
    pow_ = torch.tensor([p for p, q in enumerate(per_page) for _ in range(len(q))], dtype=torch.int32, device=dev)
    return quads, pow_, torch.tensor(offs, dtype=torch.int32, device=dev), offs


def _valid(tl, n):
    """the defined part of a TextLines of find_lines_pages as host bytes"""
    L = int(tl.n_lines.item())
    return {"n_lines": L, "quads": tl.quads[:L].cpu().numpy().tobytes(), "line_offsets": tl.line_offsets[:L + 1].tolist(),
            "line_of_word": tl.line_of_word[:n].tolist(), "word_order": tl.word_order[:n].tolist(), "next_word": tl.next_word[:n].tolist(),
            "line_page_offs": tl.line_page_offs.tolist(), "page_of_line": tl.page_of_line[:L].tolist()}


def _check_pages_equal_single(dev, per_page):
    """every output of find_lines_pages, page by page, against find_lines on that page's words alone, after shifting the indices"""
    from ocrs_models_amd import inference as inf

    quads, pow_, word_offs, offs = _flat(dev, per_page)
    tl = inf.find_lines_pages(quads, pow_, word_offs)
    n, L = offs[-1], int(tl.n_lines.item())
    lpo = tl.line_page_offs.tolist()
    assert len(lpo) == len(per_page) + 1 and lpo[0] == 0 and lpo[-1] == L
    loffs = tl.line_offsets[:L + 1].tolist()
    assert loffs[0] == 0 and loffs[L] == n
    for p in range(len(per_page)):
        w0, w1, l0, l1 = offs[p], offs[p + 1], lpo[p], lpo[p + 1]
        own = inf.find_lines(quads[w0:w1].contiguous())
        Lp = int(own.n_lines.item()) if w1 > w0 else 0
        assert l1 - l0 == Lp, p
        nw = own.next_word[:w1 - w0]
        assert torch.equal(tl.next_word[w0:w1], torch.where(nw < 0, nw, nw + w0)), p
        assert torch.equal(tl.line_of_word[w0:w1], own.line_of_word[:w1 - w0] + l0), p
        assert torch.equal(tl.word_order[w0:w1], own.word_order[:w1 - w0] + w0), p  # a page's lines hold exactly its words
        assert torch.equal(tl.line_offsets[l0:l1 + 1], own.line_offsets[:Lp + 1] + w0) if w1 > w0 else loffs[l0] == w0, p
        assert tl.quads[l0:l1].cpu().numpy().tobytes() == own.quads[:Lp].cpu().numpy().tobytes(), p
        assert tl.page_of_line[l0:l1].tolist() == [p] * Lp
    return quads, pow_, word_offs, offs, tl


def test_lines_do_not_cross_the_seam_between_pages(dev):
    from ocrs_models_amd import inference as inf

    a, b = LR.box(0, 0, 40, 14), LR.box(50, 0, 40, 14)  # the same baseline, 10 apart: within max_gap * 14
    quads, pow_, word_offs, _ = _flat(dev, [a[None], b[None]])
    one = inf.find_lines(quads)
    assert one.next_word.tolist() == [1, -1] and int(one.n_lines) == 1  # the single-page rule on the concatenation links them
    tl = inf.find_lines_pages(quads, pow_, word_offs)
    assert tl.next_word.tolist() == [-1, -1] and int(tl.n_lines) == 2
    assert tl.line_page_offs.tolist() == [0, 1, 2] and tl.page_of_line.tolist() == [0, 1] and tl.line_of_word.tolist() == [0, 1]
    assert torch.equal(tl.quads, quads)
    # line order is by page first: page 1's word lies above page 0's and still comes second
    quads2, pow2, offs2, _ = _flat(dev, [LR.box(0, 500, 40, 14)[None], LR.box(0, 0, 40, 14)[None]])
    tl2 = inf.find_lines_pages(quads2, pow2, offs2)
    assert tl2.line_of_word.tolist() == [0, 1] and tl2.page_of_line.tolist() == [0, 1]
    assert int(inf.find_lines(quads2).line_of_word[0]) == 1  # (the single-page order would put it second)


def _three_pages():
    return [LR.grid_case(9, 7, seed=3), LR.grid_case(12, 20, seed=5), LR.rotated_case()]


def test_lines_per_page_equal_find_lines_of_each_page(dev):
    per_page = _three_pages()
    assert all(len(q) < 300 for q in per_page)
    *_, tl = _check_pages_equal_single(dev, per_page)
    assert tl.line_page_offs.tolist()[:3] == [0, 9, 21]
    # pages without words at the start, in the middle and at the end own no lines and change nothing
    empty = np.zeros((0, 4, 2), np.float32)
    _check_pages_equal_single(dev, [empty, per_page[0], empty, empty, per_page[2], empty])
    _check_pages_equal_single(dev, [per_page[2]])  # B = 1 is find_lines
    # a page boundary inside a tile of 256 and a page of exactly one tile
    _check_pages_equal_single(dev, [LR.grid_case(16, 16, seed=1), LR.grid_case(1, 1), LR.grid_case(23, 23, seed=2)[:257]])


def test_lines_of_more_than_2048_words(dev):
    """both ranking paths of §14: the batches above run in one workgroup's LDS (fewer than 2048 words in total); here the total is above it
    with every page below, and then one page is above it on its own"""
    pages_ = [LR.grid_case(30, 30, seed=s) for s in (1, 2, 3)]
    assert sum(len(q) for q in pages_) > 2048 and all(len(q) < 2048 for q in pages_)
    _check_pages_equal_single(dev, pages_)
    big = LR.grid_case(42, 50, seed=9)
    assert len(big) > 2048
    _check_pages_equal_single(dev, [LR.grid_case(9, 7, seed=3), big])


def test_lines_pages_two_runs_give_identical_bytes(dev):
    from ocrs_models_amd import inference as inf

    for per_page in (_three_pages(), [LR.grid_case(30, 30, seed=s) for s in (1, 2, 3)], [LR.case_accept_tie()[0], LR.case_accept_tie()[0]]):
        quads, pow_, word_offs, offs = _flat(dev, per_page)
        a = _valid(inf.find_lines_pages(quads, pow_, word_offs), offs[-1])
        b = _valid(inf.find_lines_pages(quads, pow_, word_offs), offs[-1])
        assert a == b


def test_find_lines_pages_makes_no_host_sync(dev):
    from ocrs_models_amd import inference as inf

    cases = [_flat(dev, _three_pages()), _flat(dev, [LR.grid_case(30, 30, seed=s) for s in (1, 2, 3)])]
    want = [inf.find_lines_pages(q, pw, wo) for q, pw, wo, _ in cases]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [inf.find_lines_pages(q, pw, wo) for q, pw, wo, _ in cases]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for g, w, c in zip(got, want, cases):
        assert _valid(g, c[3][-1]) == _valid(w, c[3][-1])


# ------------------------------------------------------------------ 4. crops ------------------------------------------------------------
def _gradient_page(H, W, k, dev):
    y, x = np.mgrid[0:H, 0:W]
    return torch.from_numpy(((x * 0.37 + y * 0.61 + 40 * k) % 256).astype(np.uint8))[None].to(dev)


@pytest.fixture(scope="module")
def crop_case(dev):
    """the three-page batch of the lines test on smooth-gradient pages of three sizes; the line stage's output for it"""
    from ocrs_models_amd import inference as inf

    quads, pow_, word_offs, offs = _flat(dev, _three_pages())
    pgs = [_gradient_page(400, 380, 0, dev), _gradient_page(500, 1010, 1, dev), _gradient_page(2400, 3000, 2, dev)]
    tl = inf.find_lines_pages(quads, pow_, word_offs)
    return {"pages": pgs, "store": inf.pack_pages(pgs), "quads": quads, "page_of_word": pow_, "offs": offs, "lines": tl,
            "lpo": tl.line_page_offs.tolist(), "L": int(tl.n_lines.item())}


def _crops_of(packed, table):
    return [packed[int(o):int(o) + int(h) * int(w)].view(int(h), int(w)) for h, w, _, o in table[:, :4].tolist()]


def _own_crops(case, quads, offs):
    """every crop from the single-page path: rectify_crops of page p on the rows offs[p]:offs[p + 1]"""
    from ocrs_models_amd import inference as inf

    crops = []
    for p, page in enumerate(case["pages"]):
        q = quads[offs[p]:offs[p + 1]].contiguous()
        plan = inf.crop_plan(q)
        crops += _crops_of(inf.rectify_crops(page, q, plan), plan.table.cpu())
    return crops


def test_pack_pages_layout(dev, crop_case):
    packed, page_offs, page_sizes = crop_case["store"]
    sizes = [tuple(p.shape[1:]) for p in crop_case["pages"]]
    assert packed.dtype == torch.uint8 and packed.numel() == sum(h * w for h, w in sizes)
    assert page_offs.dtype == torch.int64 and page_offs.tolist() == [0] + np.cumsum([h * w for h, w in sizes]).tolist()[:-1]
    assert page_sizes.dtype == torch.int32 and [tuple(r) for r in page_sizes.tolist()] == sizes
    for p, o, (h, w) in zip(crop_case["pages"], page_offs.tolist(), sizes):
        assert torch.equal(packed[o:o + h * w].view(1, h, w), p)


def test_crops_from_many_pages_equal_each_pages_own_crops(dev, crop_case):
    from ocrs_models_amd import inference as inf

    c = crop_case
    for quads, page_of, offs, count in ((c["lines"].quads, c["lines"].page_of_line, c["lpo"], c["lines"].n_lines), (c["quads"], c["page_of_word"], c["offs"], None)):
        plan = inf.crop_plan(quads, count=count)
        n = plan.host()[0]
        assert n == offs[-1]
        packed = inf.rectify_crops_pages(*c["store"], quads, page_of, plan)
        got, want = _crops_of(packed, plan.table[:n].cpu()), _own_crops(c, quads, offs)
        assert len(got) == len(want) == n
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(g, w), i
    with pytest.raises(RuntimeError):
        inf.rectify_crops_pages(*c["store"], c["quads"], c["page_of_word"].long(), inf.crop_plan(c["quads"]))


@pytest.mark.parametrize("max_batch", [256, 5])
def test_pooled_batches_hold_every_crop_of_every_page(dev, crop_case, max_batch):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import input_pipeline as ip

    c = crop_case
    tl, L = c["lines"], c["L"]
    plan = inf.crop_plan(tl.quads, count=tl.n_lines)
    packed = inf.rectify_crops_pages(*c["store"], tl.quads, tl.page_of_line, plan)
    batches, widths, perm = inf.crops_to_batches(packed, plan, max_batch)
    crops = _own_crops(c, tl.quads, c["lpo"])  # the single-page crops, in flat order
    assert len(crops) == L > 2 * 5
    order, chunks, ows = R.batching([tuple(x.shape) for x in crops], max_batch, 64)  # order = sorted by (ow, flat index)
    assert order == sorted(range(L), key=lambda i: (ows[i], i))
    assert len(batches) == len(chunks) == len(widths) and [order[p] for p in perm] == list(range(L))
    assert len({tl.page_of_line[i].item() for i in order[:chunks[0][1]]}) > 1 or max_batch < 256  # one chunk mixes the pages' crops
    for (p0, cnt, wpad), b, iw in zip(chunks, batches, widths):
        assert tuple(b.shape) == (cnt, 1, 64, wpad)
        assert iw.tolist() == [ows[i] for i in order[p0:p0 + cnt]]
        for slot, i in enumerate(order[p0:p0 + cnt]):
            alone = ip.resize_line(crops[i][None].contiguous())
            assert alone.shape[-1] == ows[i]
            assert torch.equal(b[slot, :, :, :ows[i]], alone)
            assert (b[slot, :, :, ows[i]:] == 0.0).all()


# ------------------------------------------------------------------ 5. the driver, stage by stage -------------------------------------------
@pytest.fixture(scope="module")
def det_blank(det_model):
    return BlankAware(det_model).eval()


@pytest.fixture(scope="module")
def det_batch(det_blank, pages):
    from ocrs_models_amd import inference as inf

    return inf.detect_words_batch(det_blank, pages, size=SIZE)


def test_detect_words_batch_equals_the_stages_chained_from_its_probs(dev, pages, det_batch):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.postprocess import extract_cc_quads_device

    det = det_batch
    assert set(det) == {"probs", "text_masks", "quads", "page_of_word", "word_offs", "counts"}
    assert tuple(det["probs"].shape) == (4, *SIZE) and det["probs"].dtype == torch.float32
    assert tuple(det["text_masks"].shape) == (4, 320, 384) and det["text_masks"].dtype == torch.uint8
    counts, offs = det["counts"], det["word_offs"].tolist()
    print(f"fixture pages: words per page {counts}")
    assert isinstance(counts, list) and offs == [0] + np.cumsum(counts).tolist() and tuple(det["quads"].shape) == (offs[-1], 4, 2)
    assert det["page_of_word"].tolist() == [p for p, c in enumerate(counts) for _ in range(c)]
    inside = torch.zeros_like(det["text_masks"], dtype=torch.bool)
    for p, (H, W) in enumerate(PAGE_SIZES):
        mask = inf.binarize_resize(det["probs"][p], (H, W), 0.5)
        assert torch.equal(det["text_masks"][p, :H, :W], mask), p
        inside[p, :H, :W] = True
        own = inf.expand_quads(extract_cc_quads_device(mask), inf.SHRINK_DISTANCE)
        assert counts[p] == own.shape[0] and torch.equal(det["quads"][offs[p]:offs[p + 1]], own), p
    assert int(det["text_masks"][~inside].max()) == 0
    assert counts[0] > 0 and counts[2] > 0 and counts[3] > 0 and counts[1] == 0  # the white page in the middle has no words


def _pooled_by_hand(rec_model, pages, det, lines, max_batch=256):
    """the strings of the batch from the single-page functions: per-page find_lines / crop_plan / rectify_crops on the batch's own quads, the
    crops placed in a pooled plan's packed buffer, then crops_to_batches and recognize_crops.  -> (per-page results, pooled plan)"""
    from ocrs_models_amd import inference as inf

    offs = det["word_offs"].tolist()
    per_page, crop_quads = [], []
    for p, page in enumerate(pages):
        q = det["quads"][offs[p]:offs[p + 1]].contiguous()
        if lines and len(q):
            tl = inf.find_lines(q)
            L = int(tl.n_lines.item())
            order, lo = tl.word_order.tolist(), tl.line_offsets[:L + 1].tolist()
            per_page.append([{"quad": tl.quads[l].tolist(), "words": [q[i].tolist() for i in order[lo[l]:lo[l + 1]]]} for l in range(L)])
            crop_quads.append(tl.quads[:L])
        else:
            per_page.append([{"quad": r} for r in q.tolist()])
            crop_quads.append(q)
    flat = torch.cat(crop_quads).contiguous()
    pooled = inf.crop_plan(flat)
    packed = torch.zeros(pooled.host()[1], dtype=torch.float32, device=flat.device)
    table, i = pooled.table.cpu().tolist(), 0
    for page, q in zip(pages, crop_quads):
        if len(q):
            plan = inf.crop_plan(q.contiguous())
            own = inf.rectify_crops(page, q.contiguous(), plan)
            for h, w, _, o, *_ in plan.table.cpu().tolist():
                assert table[i][:2] == [h, w]
                packed[table[i][3]:table[i][3] + h * w] = own[o:o + h * w]
                i += 1
    texts = inf.recognize_crops(rec_model, inf.crops_to_batches(packed, pooled, max_batch))
    it = iter(texts)
    return [[{**r, "text": next(it)} for r in rs] for rs in per_page], pooled


@pytest.mark.parametrize("lines", [True, False])
def test_ocr_pages_equals_the_single_page_functions_in_pooled_order(dev, det_blank, rec_model, pages, det_batch, lines):
    from ocrs_models_amd import inference as inf

    max_batch = 256 if lines else 100
    want, pooled = _pooled_by_hand(rec_model, pages, det_batch, lines, max_batch)
    got = inf.ocr_pages(det_blank, rec_model, pages, lines=lines, size=SIZE, max_batch=max_batch)
    assert isinstance(got, list) and len(got) == len(pages) and got[1] == []  # page order; the empty page in the middle
    print(f"ocr_pages(lines={lines}): entries per page {[len(g) for g in got]}, pooled crops {pooled.host()[0]}")
    if not lines:
        assert [len(g) for g in got] == det_batch["counts"] and pooled.host()[0] > max_batch  # more than one chunk
    for p, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), p
        for a, b in zip(g, w):
            assert set(a) == ({"quad", "text", "words"} if lines else {"quad", "text"})
            assert a == b, p


def test_ocr_pages_of_one_page_is_the_single_page_driver(dev, det_model, det_blank, rec_model, pages):
    """one page gives the same chunks either way, so quads AND strings must match exactly"""
    from ocrs_models_amd import inference as inf

    for det, page in ((det_model, pages[0]), (det_model, pages[3]), (det_model, pages[1]), (det_blank, pages[1])):
        assert inf.ocr_pages(det, rec_model, [page], size=SIZE) == [inf.ocr_lines(det, rec_model, page, size=SIZE)]
        assert inf.ocr_pages(det, rec_model, [page], lines=False, size=SIZE) == [inf.ocr_page(det, rec_model, page, size=SIZE)]
    assert len(inf.ocr_pages(det_model, rec_model, [pages[0]], size=SIZE)[0]) > 0
    assert inf.ocr_pages(det_blank, rec_model, [pages[1]], size=SIZE) == [[]]


# ------------------------------------------------------------------ 6. batched forward against single forward -----------------------------
def test_batched_forward_against_single_forward(dev, det_model, pages, det_batch):
    """the one comparison that is not exact: whether the eval forward gives the same bits at B = 4 as at B = 1 is measured here, not assumed.
    Bound: 1e-4, the output parity bound of the fp32 path.  (DESIGN.md §15 records the printed maximum.)"""
    from ocrs_models_amd import inference as inf

    raw = inf.detect_words_batch(det_model, pages, size=SIZE)  # the golden detector itself: the white page has components too
    print(f"golden detector: words per page {raw['counts']}")
    keep = torch.tensor([1.0, 0.0, 1.0, 1.0], device=dev)[:, None, None]
    assert torch.equal(det_batch["probs"], raw["probs"] * keep)
    worst = 0.0
    for p, page in enumerate(pages):
        single = inf.detect_words(det_model, page, size=SIZE)["probs"]
        d = float((raw["probs"][p] - single).abs().max())
        print(f"page {p}: max |probs(B=4) - probs(B=1)| = {d:.3e}")
        worst = max(worst, d)
    print(f"batched forward against single forward: max difference {worst:.3e}, bound 1e-4")
    assert worst <= 1e-4


# ------------------------------------------------------------------ 7. waits ------------------------------------------------------------
def test_ocr_pages_waits_no_more_often_than_one_ocr_lines_call(dev, rec_model):
    from ocrs_models_amd import inference as inf

    size = (230, 340)
    pgs, probs = [], []
    for rows in (5, 3, 4, 2):
        bars = [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(rows) for c in range(6)]
        page, det = bar_page(*size, bars, dev)
        pgs.append(page), probs.append(det.probs)
    det_one, det_all = bar_page(*size, [(15 + 52 * c, 18 + 40 * r + (c % 3), 40, 12) for r in range(5) for c in range(6)], dev)[1], PaintedBatch(torch.stack(probs)).eval()
    for _ in range(2):  # (first calls allocate pinned memory, which may wait)
        inf.ocr_lines(det_one, rec_model, pgs[0], size=size), inf.ocr_pages(det_all, rec_model, pgs, size=size)
    one, n_one, what_one = _count_waits(lambda: inf.ocr_lines(det_one, rec_model, pgs[0], size=size))
    four, n_four, what_four = _count_waits(lambda: inf.ocr_pages(det_all, rec_model, pgs, size=size))
    print(f"host waits: one ocr_lines call {n_one} {what_one}, ocr_pages of four pages {n_four} {what_four}")
    assert len(one) == 5 and [len(g) for g in four] == [5, 3, 4, 2] and all(len(l["words"]) == 6 for g in four for l in g)
    assert n_one >= 3 and n_four <= n_one
    words, n_words, _ = _count_waits(lambda: inf.ocr_pages(det_all, rec_model, pgs, lines=False, size=size))
    assert [len(g) for g in words] == [30, 18, 24, 12] and n_words <= n_one


# ------------------------------------------------------------------ 8. edge cases ----------------------------------------------------------
def test_no_pages_and_blank_pages(dev, det_model):
    from ocrs_models_amd import inference as inf

    class NoDetector(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("nothing may be launched for an empty batch")

    assert inf.ocr_pages(NoDetector().eval(), NeverCalled().eval(), []) == []
    blank = [torch.full((1, 200, 160), 255, dtype=torch.uint8, device=dev), torch.full((1, 64, 96), 255, dtype=torch.uint8, device=dev)]
    for lines in (True, False):
        assert inf.ocr_pages(det_model, NeverCalled().eval(), blank, lines=lines, size=(128, 96), threshold=1.0) == [[], []]
    det = inf.detect_words_batch(det_model, blank, size=(128, 96), threshold=1.0)
    assert det["counts"] == [0, 0] and det["word_offs"].tolist() == [0, 0, 0] and tuple(det["quads"].shape) == (0, 4, 2)
    assert det["page_of_word"].numel() == 0 and int(det["text_masks"].sum()) == 0
    tl = inf.find_lines_pages(det["quads"], det["page_of_word"], det["word_offs"])
    assert tl.n_lines.tolist() == [0] and tl.line_page_offs.tolist() == [0, 0, 0] and tl.page_of_line.numel() == 0


def test_argument_errors(dev, det_model, rec_model, pages):
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf

    page = pages[3]
    for bad in ([page.float()], [page[0]], [page, page.cpu()], [page, page[:, :0]]):  # dtype, not (1,H,W), another device, no pixels
        with pytest.raises(RuntimeError):
            inf.ocr_pages(det_model, rec_model, bad, size=SIZE)
        with pytest.raises(RuntimeError):
            inf.detect_words_batch(det_model, bad, size=SIZE)
    with pytest.raises(RuntimeError):
        inf.detect_words_batch(det_model, [], size=SIZE)
    training = oa.DetectionModel().to(dev)
    training.train()
    with pytest.raises(RuntimeError):
        inf.ocr_pages(training, rec_model, [page], size=SIZE)
    rec_training = oa.RecognitionModel(oa.text.DEFAULT_ALPHABET).to(dev)
    rec_training.train()
    with pytest.raises(RuntimeError):
        inf.ocr_pages(det_model, rec_training, [page], size=SIZE)
    # a canvas ocrs_cc_quads cannot take is refused before anything runs, as extract_cc_quads_device refuses a mask
    from ocrs_models_amd._lib import lib

    assert lib().cc_quads_ws_bytes(2, 70000, 70000) <= 0
    with pytest.raises(ValueError):
        inf._cc_quads_pages_sizes(2, 70000, 70000)
    quads, pow_, word_offs, _ = _flat(dev, [LR.grid_case(2, 2)])
    for args in ((quads.double(), pow_, word_offs), (quads, pow_.long(), word_offs), (quads, pow_, word_offs.long()), (quads, pow_[:2], word_offs),
                 (quads.cpu(), pow_, word_offs)):
        with pytest.raises(RuntimeError):
            inf.find_lines_pages(*args)

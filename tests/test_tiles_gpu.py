"""Tiled detection on the GPU (inference.tile_batch, binarize_resize_tiles, the tile= argument of the detection drivers and
the kernels of the C ABI section "tiles") against the untiled stages, which tests/test_ocr_gpu.py and tests/test_ocr_batch_gpu.py pin, and
against the numpy restatement in tests/tiles_ref.py.

Every comparison is ``torch.equal`` / ``==`` with one exception: the eval forward over the tiles one at a time against all of them in one
chunk (test_forward_chunks_of_one_tile_against_one_chunk), bounded by 1e-4, the project's output parity bound for the fp32 path -- the bound
and the reason of test_ocr_batch_gpu.py::test_batched_forward_against_single_forward.  That is why the driver tests start from the call's own
``probs``."""
import numpy as np
import pytest
import torch

from tests import tiles_ref as TR
from tests.test_lines_gpu import _count_waits, _golden_state, dot_page
from tests.test_ocr_batch_gpu import BlankAware

pytestmark = pytest.mark.gpu

SIZE = (160, 120)   # detection size of the driver tests
TILE = (200, 150)   # 2 x 2 tiles on the 320 x 240 page (default overlap (25, 18))


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
def page(dev):
    return dot_page(320, 240).to(dev)


def _dirty_allocator(dev, *nbytes):
    """leave freed blocks of 0xFF bytes (fp32 NaN) of these sizes in the caching allocator, so that an output or a workspace that is allocated
    next and not fully written shows it"""
    blocks = [torch.full((n,), 255, dtype=torch.uint8, device=dev) for n in nbytes]
    del blocks


# ------------------------------------------------------------------ 1. the tile batch -----------------------------------------------------
@pytest.mark.parametrize("size", [(40, 30), (80, 60)])  # shrinking and enlarging the 64 x 48 windows
def test_every_tile_equals_the_resize_of_its_window(dev, size):
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd import input_pipeline as ip

    g = torch.Generator().manual_seed(11)
    sizes = [(97, 131), (64, 48), (20, 30)]  # two pages no larger than the tile: windows of three sizes in one call
    pages = [torch.randint(0, 256, (1, H, W), dtype=torch.uint8, generator=g).to(dev) for H, W in sizes]
    plans = [inf.tile_plan(H, W, (64, 48), (16, 12)) for H, W in sizes]
    assert [len(p.windows) for p in plans] == [8, 1, 1]
    tables, store = inf.tile_tables(plans, dev), inf.pack_pages(pages)
    T = tables.tiles.shape[0]
    assert T == 10 and tables.max_th == 64 and tables.tiles.cpu().tolist() == [[b, *w] for b, p in enumerate(plans) for w in p.windows]
    _dirty_allocator(dev, T * size[0] * size[1] * 4, T * tables.max_th * size[1] * 4)
    got = inf.tile_batch(*store, tables.tiles, tables.max_th, size)
    assert tuple(got.shape) == (T, 1, *size) and got.dtype == torch.float32
    t = 0
    for pg, plan in zip(pages, plans):
        for y0, x0, th, tw in plan.windows:
            want = ip.resize(ip.transform_image(pg[:, y0:y0 + th, x0:x0 + tw].clone()), size)
            assert torch.equal(got[t], want), (t, y0, x0, th, tw)
            t += 1
    assert t == T and not bool(torch.isnan(got).any())


# ------------------------------------------------------------------ 2. composition ------------------------------------------------------------
def _random_probs(T, h, w, dev, seed, threshold=0.5):
    g = torch.Generator().manual_seed(seed)
    prob = torch.rand(T, h, w, generator=g)
    prob[:, ::3, ::2] = threshold  # values on the threshold are background (strict >)
    return prob.to(dev)


@pytest.mark.parametrize("sizes,canvas,tile,overlap,threshold", [
    ([(97, 131), (64, 48), (20, 30)], (97, 131), (40, 30), (10, 8), 0.5),   # canvas width 131; 3 x 6, 2 x 2 and 1 x 1 tiles
    ([(50, 33), (20, 30), (7, 5), (50, 17)], (50, 33), (16, 12), (4, 3), 0.8125),  # canvas width 33; a page narrower than a lane
    ([(37, 29)], (41, 35), (9, 7), (8, 6), 0.5),                            # a canvas larger than its page; strides of one pixel
    ([(320, 7), (7, 7)], (320, 7), (5, 7), (0, 0), 0.5),                     # 64 tile rows, the bound of an axis; rows shorter than a lane
])
def test_composed_canvas_equals_the_restated_rule(dev, sizes, canvas, tile, overlap, threshold):
    from ocrs_models_amd import inference as inf

    plans = [inf.tile_plan(H, W, tile, overlap) for H, W in sizes]
    tables = inf.tile_tables(plans, dev)
    T = tables.tiles.shape[0]
    prob = _random_probs(T, 13, 11, dev, 3, threshold)
    _dirty_allocator(dev, len(sizes) * canvas[0] * canvas[1])
    got = inf.binarize_resize_tiles(prob, tables, canvas, threshold)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(sizes), *canvas)
    want = TR.compose_pages(prob.cpu().numpy(), sizes, tile, overlap, canvas, threshold)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert 0 < int(got.sum()) < sum(H * W for H, W in sizes)
    assert T > len(sizes) and tables.tile_offs.cpu().tolist() == [0] + np.cumsum([len(p.windows) for p in plans]).tolist()


def test_one_tile_per_page_gives_the_bytes_of_the_untiled_canvas(dev):
    from ocrs_models_amd import inference as inf

    for sizes, canvas in (([(97, 131), (64, 48), (20, 30)], (97, 131)), ([(50, 33), (3, 5), (1, 1)], (50, 33)), ([(97, 131)], (97, 131))):
        tables = inf.tile_tables([inf.tile_plan(H, W, (97, 131)) for H, W in sizes], dev)
        assert tables.tiles.shape[0] == len(sizes) and tables.max_axis == 1
        prob = _random_probs(len(sizes), 37, 29, dev, 4)
        _dirty_allocator(dev, len(sizes) * canvas[0] * canvas[1])
        got = inf.binarize_resize_tiles(prob, tables, canvas)
        assert torch.equal(got, inf.binarize_resize_pages(prob, tables.page_sizes, canvas))
        assert 0 < int(got.sum()) < got.numel()


# ------------------------------------------------------------------ 3. the seam ---------------------------------------------------------------
def test_a_word_across_a_seam_stays_one_component(dev):
    """size == tile: the nearest map is the identity, so tiles painted with their own windows of an image must compose to that image"""
    from ocrs_models_amd import inference as inf
    from ocrs_models_amd.postprocess import extract_cc_quads_device

    H, W, tile, overlap = 90, 70, (40, 30), (10, 8)
    plan = inf.tile_plan(H, W, tile, overlap)
    assert plan.rows.cuts == [32, 57, 89] and plan.cols.cuts == [24, 44, 69] and len(plan.windows) == 9
    img = np.zeros((H, W), np.float32)
    bars = [(slice(10, 15), slice(5, 65)),   # across both column cuts
            (slice(20, 86), slice(50, 55)),  # across both row cuts
            (slice(28, 38), slice(20, 30)),  # across the first row cut and the first column cut at once
            (slice(70, 76), slice(5, 16))]   # inside one tile's own ground
    for ys, xs in bars:
        img[ys, xs] = 1.0
    prob = torch.from_numpy(np.stack([img[y0:y0 + th, x0:x0 + tw] for y0, x0, th, tw in plan.windows])).to(dev)
    assert tuple(prob.shape) == (9, *tile)
    mask = inf.binarize_resize_tiles(prob, inf.tile_tables([plan], dev), (H, W))[0]
    assert torch.equal(mask.cpu(), torch.from_numpy(img.astype(np.uint8)))
    quads = extract_cc_quads_device(mask)
    assert quads.shape[0] == len(bars)  # one component per bar, not one per tile
    # each tile labelled on its own sees more pieces than there are bars
    assert sum(extract_cc_quads_device(p.clone()).shape[0] for p in prob) > len(bars)


# ------------------------------------------------------------------ 4. the drivers ------------------------------------------------------------
def _stages_from_probs(inf, probs, H, W, tile, threshold=0.5):
    from ocrs_models_amd.postprocess import extract_cc_quads_device

    mask = torch.from_numpy(TR.compose_page(probs.cpu().numpy(), H, W, tile, (tile[0] // 8, tile[1] // 8), threshold)).to(probs.device)
    return mask, inf.expand_quads(extract_cc_quads_device(mask), inf.SHRINK_DISTANCE)


def test_detect_words_tiled_equals_the_stages_chained_from_its_probs(dev, det_model, page):
    from ocrs_models_amd import inference as inf

    det = inf.detect_words(det_model, page, size=SIZE, tile=TILE)
    assert set(det) == {"probs", "text_mask", "quads", "n", "tiles"}
    plan = inf.tile_plan(320, 240, TILE)
    assert len(plan.windows) == 4 and det["tiles"].cpu().tolist() == [[0, *w] for w in plan.windows]
    assert tuple(det["probs"].shape) == (4, *SIZE) and det["probs"].dtype == torch.float32
    mask, quads = _stages_from_probs(inf, det["probs"], 320, 240, TILE)
    assert tuple(det["text_mask"].shape) == (320, 240) and torch.equal(det["text_mask"], mask)
    assert det["n"] == quads.shape[0] > 0 and torch.equal(det["quads"], quads)
    print(f"golden detector, 2 x 2 tiles: {det['n']} words; untiled {inf.detect_words(det_model, page, size=SIZE)['n']}")
    # the probabilities are the forward of the tile images in one chunk
    store = inf.pack_pages([page])
    imgs = inf.tile_batch(*store, det["tiles"], 200, SIZE)
    with torch.inference_mode():
        assert torch.equal(det_model(imgs)[:, 0], det["probs"])


@pytest.mark.parametrize("tile", [(320, 240), (400, 300)])
def test_a_tile_as_large_as_the_page_is_the_untiled_call(dev, det_model, page, tile):
    from ocrs_models_amd import inference as inf

    want, got = inf.detect_words(det_model, page, size=SIZE), inf.detect_words(det_model, page, size=SIZE, tile=tile)
    assert tuple(got["probs"].shape) == (1, *SIZE) and torch.equal(got["probs"][0], want["probs"])
    assert torch.equal(got["text_mask"], want["text_mask"]) and torch.equal(got["quads"], want["quads"]) and got["n"] == want["n"] > 0


@pytest.fixture(scope="module")
def batch_pages(dev, page):
    """the white page sits in the middle of the batch (it has no words under BlankAware, see there)"""
    return [page, torch.full((1, 200, 160), 255, dtype=torch.uint8, device=dev), dot_page(97, 131).to(dev)]


def test_detect_words_batch_tiled_equals_per_page_composition_from_its_probs(dev, det_model, batch_pages):
    from ocrs_models_amd import inference as inf

    det = inf.detect_words_batch(BlankAware(det_model).eval(), batch_pages, size=SIZE, tile=TILE)
    assert set(det) == {"probs", "text_masks", "quads", "page_of_word", "word_offs", "counts", "tiles", "tile_offs"}
    sizes = [(320, 240), (200, 160), (97, 131)]
    plans = [inf.tile_plan(H, W, TILE) for H, W in sizes]
    toffs = det["tile_offs"].cpu().tolist()
    assert toffs == [0, 4, 6, 7] and det["tile_offs"].dtype == torch.int32
    assert det["tiles"].cpu().tolist() == [[b, *w] for b, p in enumerate(plans) for w in p.windows]
    assert tuple(det["probs"].shape) == (7, *SIZE) and tuple(det["text_masks"].shape) == (3, 320, 240)
    counts, offs = det["counts"], det["word_offs"].tolist()
    assert offs == [0] + np.cumsum(counts).tolist() and tuple(det["quads"].shape) == (offs[-1], 4, 2)
    inside = torch.zeros_like(det["text_masks"], dtype=torch.bool)
    for p, (H, W) in enumerate(sizes):
        mask, own = _stages_from_probs(inf, det["probs"][toffs[p]:toffs[p + 1]], H, W, TILE)
        assert torch.equal(det["text_masks"][p, :H, :W], mask), p
        inside[p, :H, :W] = True
        assert counts[p] == own.shape[0] and torch.equal(det["quads"][offs[p]:offs[p + 1]], own), p
    assert int(det["text_masks"][~inside].max()) == 0
    assert counts[0] > 0 and counts[2] > 0 and counts[1] == 0  # the white page in the middle has no words
    assert det["page_of_word"].tolist() == [p for p, c in enumerate(counts) for _ in range(c)]


def test_ocr_drivers_tiled_equal_the_stages_after_tiled_detection(dev, det_model, rec_model, page):
    from ocrs_models_amd import inference as inf

    det = inf.detect_words(det_model, page, size=SIZE, tile=TILE)
    lines = inf.ocr_lines(det_model, rec_model, page, size=SIZE, tile=TILE)
    assert len(lines) > 0 and lines == inf.read_lines(rec_model, page, det["quads"])
    assert inf.ocr_pages(det_model, rec_model, [page], size=SIZE, tile=TILE) == [lines]
    words = inf.ocr_page(det_model, rec_model, page, size=SIZE, tile=TILE)
    assert len(words) == det["n"] and [w["quad"] for w in words] == det["quads"].tolist()
    assert inf.ocr_pages(det_model, rec_model, [page], lines=False, size=SIZE, tile=TILE) == [words]
    # an explicit overlap and chunk size travel through every driver
    kw = dict(size=SIZE, tile=TILE, overlap=(40, 30), tile_batch=3)
    det2 = inf.detect_words(det_model, page, **kw)
    assert det2["tiles"].cpu().tolist() == [[0, *w] for w in inf.tile_plan(320, 240, TILE, (40, 30)).windows]
    assert [w["quad"] for w in inf.ocr_page(det_model, rec_model, page, **kw)] == det2["quads"].tolist()


class SameForEveryImage(torch.nn.Module):
    """a detector that paints the same few bars for every image it is given, so the number of words, and with it the number of recognition
    chunks whose labels are waited for, is small with and without tiles"""

    def __init__(self, dev):
        super().__init__()
        probs = torch.zeros(SIZE)
        for r in range(3):
            for c in range(2):
                probs[20 + 45 * r:28 + 45 * r, 12 + 55 * c:47 + 55 * c] = 0.9
        self.probs = probs.to(dev)

    def forward(self, x):
        return self.probs.expand(x.shape[0], 1, *SIZE)


def test_tiled_calls_wait_as_often_as_untiled_calls(dev, rec_model, page, batch_pages):
    from ocrs_models_amd import inference as inf

    det = SameForEveryImage(dev).eval()
    legs = {"detect_words": lambda **kw: inf.detect_words(det, page, size=SIZE, **kw),
            "detect_words_batch": lambda **kw: inf.detect_words_batch(det, batch_pages, size=SIZE, **kw),
            "ocr_lines": lambda **kw: inf.ocr_lines(det, rec_model, page, size=SIZE, **kw),
            "ocr_pages": lambda **kw: inf.ocr_pages(det, rec_model, batch_pages, size=SIZE, **kw)}
    assert inf.detect_words(det, page, size=SIZE)["n"] == 6 and 6 < inf.detect_words(det, page, size=SIZE, tile=TILE)["n"] <= 24
    for name, fn in legs.items():
        for _ in range(2):  # (first calls allocate pinned memory, which may wait)
            fn(), fn(tile=TILE)
        _, n_plain, what_plain = _count_waits(fn)
        _, n_tiled, what_tiled = _count_waits(lambda: fn(tile=TILE))
        print(f"host waits of {name}: untiled {n_plain} {what_plain}, tiled {n_tiled} {what_tiled}")
        assert n_tiled == n_plain >= 1, name


def test_eval_detection_with_tiles_writes_its_files(dev, tmp_path):
    """the entry point in this process (its argument parsing and pictures; the detection itself is the driver tested above)"""
    import ocrs_models_amd as oa
    from ocrs_models_amd import eval_detection
    from ocrs_models_amd.checkpoint import save_checkpoint
    from PIL import Image

    det = oa.DetectionModel()
    det.load_state_dict(_golden_state("det"))
    save_checkpoint(str(tmp_path / "det.pt"), det, oa.optim.Adam(det.parameters()), 0)
    Image.fromarray(dot_page(640, 480)[0].numpy()).save(tmp_path / "page.png")
    base = [str(tmp_path / "det.pt"), str(tmp_path / "page.png"), str(tmp_path / "out")]
    eval_detection.main(base + ["--tile", "400", "300", "--tile-overlap", "40", "30"])  # 2 x 2 tiles
    for name, size in (("input", (600, 800)), ("text-regions", (480, 640)), ("text-probs", (1200, 1600)), ("text-words", (480, 640))):
        assert Image.open(tmp_path / f"out-{name}.png").size == size, name  # (PIL: width, height)
    for bad in (["--tile-overlap", "4", "4"], ["--tile", "400", "300", "--tile-overlap", "400", "0"], ["--tile", "0", "300"]):
        with pytest.raises(SystemExit):
            eval_detection.main(base + bad)


# ------------------------------------------------------------------ 5. forward chunks -----------------------------------------------------
def test_forward_chunks_of_one_tile_against_one_chunk(dev, det_model, page):
    """the one comparison that is not exact: whether the eval forward gives the same bits for a tile alone as for the four tiles in one
    chunk is measured here, not assumed.  Bound: 1e-4, the output parity bound of the fp32 path.  (DESIGN.md §20 records the printed maximum.)"""
    from ocrs_models_amd import inference as inf

    one = inf.detect_words(det_model, page, size=SIZE, tile=TILE, tile_batch=1)["probs"]
    pooled = inf.detect_words(det_model, page, size=SIZE, tile=TILE, tile_batch=16)["probs"]
    assert one.shape == pooled.shape == (4, *SIZE)
    worst = float((one - pooled).abs().max())
    print(f"forward chunks: max |probs(tile_batch=1) - probs(tile_batch=16)| = {worst:.3e}, bound 1e-4")
    assert worst <= 1e-4
    # chunks that do not divide the tile count: 3 + 1
    three = inf.detect_words(det_model, page, size=SIZE, tile=TILE, tile_batch=3)["probs"]
    assert float((three - pooled).abs().max()) <= 1e-4


# ------------------------------------------------------------------ 6. determinism and arguments ----------------------------------------------
def test_two_runs_give_identical_bytes(dev, det_model, batch_pages):
    from ocrs_models_amd import inference as inf

    a = inf.detect_words_batch(det_model, batch_pages, size=SIZE, tile=TILE)
    _dirty_allocator(dev, 7 * SIZE[0] * SIZE[1] * 4, 3 * 320 * 240)
    b = inf.detect_words_batch(det_model, batch_pages, size=SIZE, tile=TILE)
    for key in ("probs", "text_masks", "quads", "page_of_word", "word_offs", "tiles", "tile_offs"):
        assert torch.equal(a[key], b[key]), key
    assert a["counts"] == b["counts"]


def test_argument_errors(dev, det_model, rec_model, page):
    import ocrs_models_amd as oa
    from ocrs_models_amd import inference as inf

    training = oa.DetectionModel().to(dev)
    training.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        inf.detect_words(training, page, size=SIZE, tile=TILE)
    with pytest.raises(RuntimeError, match="eval mode"):
        inf.detect_words_batch(training, [page], size=SIZE, tile=TILE)
    for bad in (dict(tile=TILE, overlap=TILE), dict(tile=TILE, overlap=(0, 150)), dict(tile=(0, 150)), dict(tile=(200.0, 150)),
                dict(tile=TILE, tile_batch=0), dict(tile=TILE, tile_batch=2.0),
                dict(tile=(1, 240), overlap=0),    # 320 tile rows: more than TILES_AXIS_MAX along one axis
                dict(tile=(320, 3), overlap=0)):   # 80 tile columns
        with pytest.raises(RuntimeError):
            inf.detect_words(det_model, page, size=SIZE, **bad)
        with pytest.raises(RuntimeError):
            inf.detect_words_batch(det_model, [page], size=SIZE, **bad)
        with pytest.raises(RuntimeError):
            inf.ocr_pages(det_model, rec_model, [page], size=SIZE, **bad)
    assert inf.TILES_AXIS_MAX == 64
    with pytest.raises(RuntimeError):
        inf.detect_words(det_model, page.cpu(), size=SIZE, tile=TILE)
    with pytest.raises(RuntimeError):
        inf.detect_words_batch(det_model, [page.cpu()], size=SIZE, tile=TILE)
    tables = inf.tile_tables([inf.tile_plan(320, 240, TILE)], dev)
    with pytest.raises(RuntimeError):
        inf.binarize_resize_tiles(torch.zeros(3, 8, 8, device=dev), tables, (320, 240))  # one map per tile: 4
    with pytest.raises(RuntimeError):
        inf.tile_batch(*inf.pack_pages([page]), tables.tiles.float(), 200, SIZE)

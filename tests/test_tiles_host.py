"""CPU-only checks of tiled detection: ``inference.tile_plan`` against the numpy restatement in tests/tiles_ref.py and against
the properties the rule promises, the argument checks that need no GPU, and the C ABI section "tiles"."""
import ctypes

import numpy as np
import pytest
import torch

from ocrs_models_amd import _lib
from ocrs_models_amd import inference as inf
from tests import tiles_ref as TR

NEW = ["ocrs_tile_batch_ws_floats", "ocrs_tile_batch", "ocrs_binarize_resize_tiles"]


def _overlaps(T):
    return sorted({0, 1, T // 2, T - 1} & set(range(T)))


@pytest.mark.parametrize("T", [1, 7, 16, 64])
def test_tile_plan_against_the_restated_rule_and_its_properties(T):
    seen_counts = set()
    for V in _overlaps(T):
        for L in range(1, 201):
            ref = TR.axis_plan(L, T, V)
            TR.check_axis(L, T, V, *ref)
            # the same axis as rows of one plan and as columns of another, against an axis that has one tile
            a, b = inf.tile_plan(L, 5, (T, 9), (V, 0)), inf.tile_plan(3, L, (4, T), (1, V))
            for got in (a.rows, b.cols):
                assert (got.starts, got.lengths, got.cuts) == ref, (L, T, V)
            assert (a.cols.starts, a.cols.lengths, a.cols.cuts) == ([0], [5], [4]) and (b.rows.starts, b.rows.lengths, b.rows.cuts) == ([0], [3], [2])
            # every coordinate has exactly one owner, and the owner's tile covers it
            owners = [TR.owner(ref[2], v) for v in range(L)]
            assert owners == sorted(owners) and set(owners) == set(range(len(ref[0])))
            assert all(ref[0][o] <= v < ref[0][o] + ref[1][o] for v, o in enumerate(owners))
            seen_counts.add(len(ref[0]))
    assert 1 in seen_counts and (T == 64 or max(seen_counts) > 3)


def test_one_tile_when_the_page_fits():
    for L, T in ((1, 1), (5, 5), (5, 64), (64, 64), (199, 200)):
        for V in _overlaps(T):
            assert TR.axis_plan(L, T, V) == ([0], [L], [L - 1])
    p = inf.tile_plan(97, 131, (200, 150))
    assert (p.H, p.W) == (97, 131) and p.windows == [(0, 0, 97, 131)]
    assert inf.tile_plan(97, 131, (97, 131), (96, 130)).windows == [(0, 0, 97, 131)]
    # one pixel more than the tile: two tiles, one pixel apart
    q = inf.tile_plan(98, 131, (97, 131), 0)
    assert q.windows == [(0, 0, 97, 131), (1, 0, 97, 131)] and q.rows.cuts == [48, 97]


def test_windows_are_the_row_major_product_and_the_default_overlap():
    p = inf.tile_plan(3508, 2480, (1600, 1200))  # a 300 dpi A4 scan: overlap (200, 150) by default
    assert p.rows.starts == [0, 954, 1908] and p.cols.starts == [0, 640, 1280]
    assert p.rows.cuts == [1276, 2230, 3507] and p.cols.cuts == [919, 1559, 2479]
    assert p.windows == [(y0, x0, 1600, 1200) for y0 in p.rows.starts for x0 in p.cols.starts] and len(p.windows) == 9
    assert p == inf.tile_plan(3508, 2480, (1600, 1200), (200, 150))
    assert inf.tile_plan(100, 100, 40, 8) == inf.tile_plan(100, 100, (40, 40), (8, 8))  # an int stands for both axes
    ref = TR.windows(90, 70, (40, 30), (10, 8))
    assert inf.tile_plan(90, 70, (40, 30), (10, 8)).windows == ref[2]


def test_argument_errors():
    for bad in (dict(tile=(0, 10)), dict(tile=(10, -1)), dict(tile=(10.0, 10)), dict(tile=(10, 10, 10)), dict(tile="big"), dict(tile=(True, 10)),
                dict(tile=(10, 10), overlap=(10, 0)), dict(tile=(10, 10), overlap=(0, 12)), dict(tile=(10, 10), overlap=(-1, 0)),
                dict(tile=(10, 10), overlap=(0.5, 0)), dict(tile=(10, 10), overlap=(1, 2, 3))):
        with pytest.raises(RuntimeError, match="tile_plan"):
            inf.tile_plan(50, 50, **bad)
    for H, W in ((0, 5), (5, 0), (5.0, 5)):
        with pytest.raises(RuntimeError, match="tile_plan"):
            inf.tile_plan(H, W, (4, 4))
    with pytest.raises(RuntimeError, match="tile_tables"):
        inf.tile_tables([], "cpu")
    with pytest.raises(RuntimeError, match="at most 64"):  # 65 tiles along the rows; refused before any device is touched
        inf.tile_tables([inf.tile_plan(65, 4, (1, 4), 0)], "cpu")
    assert len(inf.tile_plan(64, 4, (1, 4), 0).windows) == inf.TILES_AXIS_MAX == 64


def test_tiled_functions_have_no_cpu_path():
    page = torch.zeros(1, 8, 8, dtype=torch.uint8)
    ident = torch.nn.Identity().eval()
    for fn, args, kw in ((inf.detect_words, (ident, page), dict(tile=(4, 4))), (inf.detect_words_batch, (ident, [page]), dict(tile=(4, 4))),
                         (inf.ocr_pages, (ident, None, [page]), dict(tile=(4, 4))),
                         (inf.tile_batch, (torch.zeros(64, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.tensor([[8, 8]], dtype=torch.int32),
                                           torch.zeros(1, 5, dtype=torch.int32), 8, (4, 4)), {}),
                         (inf.binarize_resize_tiles, (torch.zeros(1, 4, 4), None, (8, 8)), {})):
        with pytest.raises(RuntimeError):
            fn(*args, **kw)
    import ocrs_models_amd as oa

    for name in ("tile_plan", "tile_tables", "tile_batch", "binarize_resize_tiles", "TilePlan", "TileTables"):
        assert getattr(oa, name) is getattr(inf, name)


def test_the_tiles_section_is_declared_and_exported():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(dll, name), name
    assert _lib.SIGNATURES["ocrs_tile_batch_ws_floats"] == ("l", "iii")
    assert _lib.ARG_NAMES["ocrs_tile_batch"][:8] == ["pages", "pages_bytes", "page_offs", "page_sizes", "B", "tiles", "T", "max_th"]
    assert _lib.ARG_NAMES["ocrs_binarize_resize_tiles"][4:11] == ["tiles", "tile_offs", "page_sizes", "grids", "row_cuts", "col_cuts", "max_axis"]
    assert "#define OCRS_TILES_AXIS_MAX 64" in open(_lib.HEADER_PATH).read()


def test_workspace_query_answers_without_a_gpu():
    L = _lib.lib()
    assert L.tile_batch_ws_floats(9, 1600, 600) == 9 * 1600 * 600
    assert L.tile_batch_ws_floats(65535, 65535, 800) == 65535 * 65535 * 800  # beyond 32 bits
    assert L.tile_batch_ws_floats(0, 10, 10) == 0 and L.tile_batch_ws_floats(3, 0, 10) == 0 and L.tile_batch_ws_floats(3, 10, -1) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    raw = _lib.lib()._dll
    f = ctypes.c_float(0.5)
    assert raw.ocrs_tile_batch(None, 0, None, None, 0, None, 0, 8, None, 0, None, 4, 4, None) == 0      # no tiles: nothing to launch
    assert raw.ocrs_tile_batch(None, 0, None, None, 1, None, 1, 8, None, 0, None, 4, 4, None) == 1      # tiles but no buffers
    assert raw.ocrs_tile_batch(None, 0, None, None, 0, None, 0, 0, None, 0, None, 4, 4, None) == 1      # max_th < 1
    assert raw.ocrs_tile_batch(None, 0, None, None, 0, None, 70000, 8, None, 0, None, 4, 4, None) == 1  # T beyond the grid
    assert raw.ocrs_binarize_resize_tiles(None, 1, 4, 4, None, None, None, None, None, None, 1, None, 0, 8, 8, f, None) == 0   # no pages
    assert raw.ocrs_binarize_resize_tiles(None, 1, 4, 4, None, None, None, None, None, None, 65, None, 0, 8, 8, f, None) == 1  # beyond the bound
    assert raw.ocrs_binarize_resize_tiles(None, 1, 4, 4, None, None, None, None, None, None, 0, None, 0, 8, 8, f, None) == 1
    assert raw.ocrs_binarize_resize_tiles(None, 1, 4, 4, None, None, None, None, None, None, 64, None, 1, 8, 8, f, None) == 1  # pages but no buffers


def test_reference_composition_of_one_tile_is_the_plain_nearest_resize():
    """tiles_ref against the untiled rule it generalises (restated here, float32): one tile covering the page"""
    g = np.random.default_rng(5)
    probs = g.random((1, 13, 11), dtype=np.float32)
    H, W = 37, 29
    ys = np.minimum(np.floor(np.arange(H, dtype=np.float32) * (np.float32(13) / np.float32(H))).astype(int), 12)
    xs = np.minimum(np.floor(np.arange(W, dtype=np.float32) * (np.float32(11) / np.float32(W))).astype(int), 10)
    want = (probs[0][np.ix_(ys, xs)] > np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(TR.compose_page(probs, H, W, (64, 64), (8, 8)), want)

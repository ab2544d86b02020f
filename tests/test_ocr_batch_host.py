"""CPU-only checks of the page-batch path: the pure-Python halves of ``ocr_pages`` -- the chunk layout from a pooled histogram of
output widths and the split of the flat results by page -- against hand-made numbers, the new C ABI section, and the argument checks that
need no GPU."""
import ctypes

import pytest
import torch

from ocrs_models_amd import _lib
from ocrs_models_amd import inference as inf

NEW = ["ocrs_binarize_resize_pages", "ocrs_gather_page_quads", "ocrs_text_lines_pages_ws_bytes", "ocrs_line_links_pages", "ocrs_line_rank_pages",
       "ocrs_line_order_pages", "ocrs_line_quads_pages", "ocrs_rectify_crops_pages"]


def _hist(widths):
    h = [0] * 801
    for w in widths:
        h[w] += 1
    return h


def test_chunks_of_a_pooled_histogram():
    """three pages' crops pooled: page 0 has widths 40, 40, 200; page 1 none; page 2 has 64, 130, 130, 640.  In (width, flat index) order:
    40 40 64 130 130 200 640."""
    pooled = _hist([40, 40, 200] + [] + [64, 130, 130, 640])
    assert inf.plan_chunks(pooled, 256, 64) == [(0, 7, 704)]                              # one chunk, padded to the batch's widest crop
    assert inf.plan_chunks(pooled, 3, 64) == [(0, 3, 128), (3, 3, 256), (6, 1, 704)]      # round_up(64, 64) = 128: an exact multiple gets a unit more
    assert inf.plan_chunks(pooled, 5, 4) == [(0, 5, 132), (5, 2, 644)]
    # pooling is what changes a crop's padded width: page 0 alone pads its 40s to 256 with its own 200; pooled at 3 per chunk they get 128
    assert inf.plan_chunks(_hist([40, 40, 200]), 3, 64) == [(0, 3, 256)]
    assert inf.plan_chunks(_hist([]), 256, 64) == []


def test_split_by_page():
    lines = [f"l{i}" for i in range(6)]
    assert inf.split_by_page(lines, [0, 2, 2, 5, 6]) == [["l0", "l1"], [], ["l2", "l3", "l4"], ["l5"]]  # an empty page in the middle
    assert inf.split_by_page([], [0, 0, 0]) == [[], []]
    assert inf.split_by_page(lines, [0, 6]) == [lines]
    for bad in ([0, 3, 2, 6], [0, 2, 5], [1, 3, 6]):  # not ascending, not to the end, not from 0
        with pytest.raises(RuntimeError):
            inf.split_by_page(lines, bad)


def test_the_page_batch_section_is_declared_and_exported():
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(dll, name), name
    assert _lib.SIGNATURES["ocrs_text_lines_pages_ws_bytes"] == ("l", "li")
    assert _lib.ARG_NAMES["ocrs_rectify_crops_pages"][:5] == ["pages", "pages_bytes", "page_offs", "page_sizes", "B"]
    assert _lib.ARG_NAMES["ocrs_line_order_pages"][7:9] == ["line_page_offs", "page_of_line"]


def test_workspace_size_of_the_paged_line_stage():
    L = _lib.lib()
    for cap, B in ((1, 1), (300, 4), (2049, 16), (5000, 1000)):
        got, single = L.text_lines_pages_ws_bytes(cap, B), L.text_lines_ws_bytes(cap)
        assert got % 16 == 0 and got >= single + 2 * 4 * (B + 1)  # the single-page layout first, then two per-page tables
        assert got <= single + 2 * 4 * (B + 1) + 32
    assert L.text_lines_pages_ws_bytes(0, 4) == 0 and L.text_lines_pages_ws_bytes(10, 0) == 0 and L.text_lines_pages_ws_bytes((1 << 24) + 1, 1) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    raw = L._dll
    assert raw.ocrs_binarize_resize_pages(None, None, None, 2, 0, 5, 8, 8, ctypes.c_float(0.5), None) == 1
    assert raw.ocrs_gather_page_quads(None, None, 70000, 4, None, None, None, 0, None) == 1
    assert raw.ocrs_line_links_pages(None, None, 2, -1, ctypes.c_float(2.0), ctypes.c_float(0.9), None, None, 0, None) == 1
    assert raw.ocrs_line_links_pages(None, None, 2, 0, ctypes.c_float(2.0), ctypes.c_float(0.9), None, None, 0, None) == 0  # no words: nothing to launch
    assert raw.ocrs_rectify_crops_pages(None, -1, None, None, 1, None, None, None, None, 1, None, 0, None) == 1
    assert raw.ocrs_rectify_crops_pages(None, 0, None, None, 0, None, None, None, None, 0, None, 0, None) == 0  # no tiles: nothing to launch


def test_batch_functions_have_no_cpu_path():
    page = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for fn, args in ((inf.detect_words_batch, (torch.nn.Identity().eval(), [page])), (inf.ocr_pages, (torch.nn.Identity().eval(), None, [page])),
                     (inf.pack_pages, ([page],)), (inf.find_lines_pages, (torch.zeros(1, 4, 2), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)))):
        with pytest.raises(RuntimeError):
            fn(*args)
    assert inf.ocr_pages(None, None, []) == []
    import ocrs_models_amd as oa

    for name in ("detect_words_batch", "find_lines_pages", "rectify_crops_pages", "ocr_pages"):
        assert getattr(oa, name) is getattr(inf, name)

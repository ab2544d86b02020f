"""CPU-only: tests/chars_ref.py, the numpy restatement of the character rule that tests/test_chars_gpu.py compares the kernels
of csrc/char_spans.hip with, pinned on cases worked out by hand."""
import numpy as np

from tests import chars_ref as R
from tests.lines_ref import box


def _lp(classes, C=3, values=None):
    """(T,1,C) log-probs whose arg-max at step t is classes[t], with value values[t] there and -9 elsewhere"""
    T = len(classes)
    lp = np.full((T, 1, C), -9.0, dtype=np.float32)
    for t, c in enumerate(classes):
        lp[t, 0, c] = -0.125 * (t + 1) if values is None else values[t]
    return lp


def test_runs_blanks_and_repeats():
    lp = _lp([1, 1, 0, 1, 2, 2])  # a a _ a b b
    (r,) = R.decode_spans(lp, [6])
    assert r["labels"] == [1, 1, 2] and r["t0"] == [0, 3, 4] and r["t1"] == [1, 3, 5]
    assert r["peak"].dtype == np.float32 and r["peak"].tolist() == [-0.125, -0.5, -0.625]  # the largest of the run, a copy of an input value
    assert r["labels"] == R.collapse([1, 1, 0, 1, 2, 2])
    (r,) = R.decode_spans(_lp([1, 0, 1]), [3])
    assert r["labels"] == [1, 1] and r["t0"] == [0, 2] and r["t1"] == [0, 2]  # a, blank, a: two characters
    (r,) = R.decode_spans(_lp([1, 1]), [2])
    assert r["labels"] == [1] and (r["t0"], r["t1"]) == ([0], [1])           # a, a: one
    (r,) = R.decode_spans(_lp([2, 2, 2, 1], values=[-3.0, -1.0, -2.0, -0.5]), [4])
    assert r["peak"].tolist() == [-1.0, -0.5]                                 # the peak need not be at either end of the run


def test_input_length_cuts_the_last_run():
    lp = _lp([1, 1, 0, 1, 2, 2])
    (r,) = R.decode_spans(lp, [5])
    assert r["labels"] == [1, 1, 2] and r["t1"] == [1, 3, 4] and r["peak"].tolist() == [-0.125, -0.5, -0.625]
    (r,) = R.decode_spans(lp, [4])
    assert r["labels"] == [1, 1] and r["t1"] == [1, 3]
    assert R.decode_spans(lp, [0])[0]["labels"] == [] and R.decode_spans(lp, [-3])[0]["labels"] == []
    (r,) = R.decode_spans(lp, [11])  # longer than T: T
    assert r["t1"] == [1, 3, 5]


def test_ties_take_the_first_class():
    lp = np.zeros((4, 1, 3), dtype=np.float32)  # every class equal: blank
    assert R.decode_spans(lp, [4])[0]["labels"] == []
    lp[:, 0, 0] = -1.0                           # classes 1 and 2 tie: 1
    (r,) = R.decode_spans(lp, [4])
    assert r["labels"] == [1] and (r["t0"], r["t1"]) == ([0], [3]) and r["peak"].tolist() == [0.0]


def test_extent_and_clamping_at_both_crop_ends():
    # ow = 10: step 0 starts two columns left of the crop, step 3 ends four right of it
    a0, a1 = R.char_extent([0, 1, 2], [0, 1, 3], 10)
    assert a0.tolist() == [0, 2, 6] and a1.tolist() == [2, 6, 10]
    # a 40 x 16 crop frame resized to ow = 10: columns are 4 page pixels wide; the quad spans the crop's height
    q = box(100, 50, 40, 16)
    b = R.char_boxes(q, 10, [0, 1, 2], [0, 1, 3])
    assert b["s0"].tolist() == [0.0, 8.0, 24.0] and b["s1"].tolist() == [8.0, 24.0, 40.0] and b["centre"].tolist() == [4.0, 16.0, 32.0]
    assert b["quads"].dtype == np.float32
    assert b["quads"][1].tolist() == [[108.0, 50.0], [124.0, 50.0], [124.0, 66.0], [108.0, 66.0]]
    assert b["quads"][0][0].tolist() == [100.0, 50.0] and b["quads"][2][2].tolist() == [140.0, 66.0]  # the crop's own corners
    # a vertical crop: u = (0, 1), v = (-1, 0), the origin is the top right corner
    v = R.char_boxes(box(100, 50, 16, 40), 10, [1], [1])
    assert v["quads"][0].tolist() == [[116.0, 58.0], [116.0, 74.0], [100.0, 74.0], [100.0, 58.0]]
    assert R.char_boxes(q, 10, [1], [1], np.float64)["quads"].dtype == np.float64


LINE = box(0, 0, 256, 64)  # ow = 256 below: a column is a page pixel, so s = a and the centre of steps t0..t1 is 2 (t0 + t1)


def _centres(ts):
    b = R.char_boxes(LINE, 256, [t for t, _ in ts], [t for _, t in ts])
    return b["centre"]


def test_a_centre_on_a_boundary_goes_to_the_later_word():
    words = [box(0, 0, 100, 64), box(120, 0, 136, 64)]
    wb = R.word_bounds(LINE, words)
    assert wb["lo"].tolist() == [0.0, 120.0] and wb["hi"].tolist() == [100.0, 256.0] and wb["b"].tolist() == [110.0] and wb["B"].tolist() == [110.0]
    c = _centres([(10, 12), (27, 27), (27, 28), (40, 41)])
    assert c.tolist() == [44.0, 108.0, 110.0, 162.0]
    assert R.word_ranges(wb["B"], c, [5, 6, 7, 8], 1).tolist() == [[0, 2], [2, 4]]
    r = R.line_words(LINE, words, 256, [10, 27, 27, 40], [12, 27, 28, 41], [5, 6, 7, 8], 1)
    assert r["ranges"].tolist() == [[0, 2], [2, 4]] and r["margin"] == 0.0


def test_the_running_maximum_mends_boundaries_that_fall_back():
    # the second word lies inside the first: b = [125, 90] -> B = [125, 125]; it gets no character, the third word those from 125 on
    words = [box(0, 0, 150, 64), box(100, 0, 20, 64), box(60, 0, 140, 64)]
    wb = R.word_bounds(LINE, words)
    assert wb["b"].tolist() == [125.0, 90.0] and wb["B"].tolist() == [125.0, 125.0]
    c = _centres([(5, 5), (25, 25), (30, 30), (31, 32), (40, 40)])
    assert c.tolist() == [20.0, 100.0, 120.0, 126.0, 160.0]
    assert R.word_ranges(wb["B"], c, [5, 5, 5, 5, 5], 1).tolist() == [[0, 3], [3, 3], [3, 5]]  # an empty word is (e, e)


def test_trimming_keeps_inner_spaces_and_empties_an_all_space_range():
    words = [box(0, 0, 60, 64), box(80, 0, 60, 64), box(160, 0, 96, 64)]
    wb = R.word_bounds(LINE, words)
    assert wb["B"].tolist() == [70.0, 150.0]
    c = _centres([(2, 2), (5, 5), (8, 8), (15, 15), (20, 20), (25, 25), (30, 30), (35, 35), (45, 45), (50, 50)])
    assert c.tolist() == [8.0, 20.0, 32.0, 60.0, 80.0, 100.0, 120.0, 140.0, 180.0, 200.0]
    sp = 1
    # word 0: ' a b' + ' ' -> the leading and the trailing space go, the inner one stays; word 1: all spaces; word 2: untouched
    labels = [sp, 7, sp, 8, sp, sp, sp, sp, 9, 9]
    assert R.word_ranges(wb["B"], c, labels, sp).tolist() == [[1, 4], [8, 8], [8, 10]]
    labels = [sp, 7, sp, 8, sp, 3, sp, sp, 9, sp]
    assert R.word_ranges(wb["B"], c, labels, sp).tolist() == [[1, 4], [5, 6], [8, 9]]
    assert R.word_ranges(wb["B"], c, labels, -1).tolist() == [[0, 4], [4, 8], [8, 10]]  # an alphabet without a space: nothing is trimmed
    # a one-word line gets every character, trimmed; a line without characters gives every word (0, 0)
    assert R.word_ranges(np.zeros(0, np.float32), c, labels, sp).tolist() == [[1, 9]]
    assert R.word_ranges(wb["B"], np.zeros(0, np.float32), [], sp).tolist() == [[0, 0], [0, 0], [0, 0]]


def test_space_label():
    from ocrs_models_amd.text import DEFAULT_ALPHABET

    assert R.space_label(DEFAULT_ALPHABET) == 1 and R.space_label("abc") == -1 and R.space_label("ab c") == 3

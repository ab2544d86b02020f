"""The mixed-directions rule on the host: the numpy restatement tests/directions_ref.py on hand-made cases, the package's host
half (``mixed_results``) and the argument errors, which must come before any device use.  No GPU."""
import numpy as np
import pytest
import torch

from tests import directions_ref as D
from tests import orient_ref as O


def box(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float32)


NAN = np.float32(np.nan)


def test_the_axis_of_hand_made_quads():
    diag = np.array([[0, 0], [16, 16], [14, 18], [-2, 2]], np.float32)            # long side (16, 16): exactly 45 degrees
    steeper = np.array([[0, 0], [16, 17], [14, 19], [-2, 2]], np.float32)         # (16, 17)
    flatter = np.array([[0, 0], [17, 16], [15, 18], [-2, 2]], np.float32)
    up_left = np.array([[0, 0], [-16, -17], [-14, -19], [2, -2]], np.float32)     # the signs of L do not matter
    cases = [(box(0, 0, 40, 10), False), (box(0, 0, 10, 40), True), (diag, False), (steeper, True), (flatter, False), (up_left, True),
             (np.roll(box(0, 0, 10, 40), 1, axis=0), True),                       # the long side is c1->c2 or c0->c1: the same answer
             (box(0, 0, 10, 10), False), (np.roll(box(0, 0, 10, 10), 1, axis=0), False),  # equal sides: the one with the larger |x|, so upright
             (box(5, 5, 0, 0), False),                                            # a point: L = (0, 0), 0 > 0 fails
             (box(0, 0, 0, 30), True), (box(0, 0, 30, 0), False)]                 # zero area, non-zero length: the segment decides
    got = D.sideways(np.stack([q for q, _ in cases]))
    assert got.tolist() == [want for _, want in cases]


def test_a_nan_anywhere_is_upright():
    tall = box(0, 0, 10, 40)
    assert D.sideways(tall[None]).tolist() == [True]
    for corner in range(4):
        for axis in range(2):
            q = tall.copy()
            q[corner, axis] = NAN
            assert D.sideways(q[None]).tolist() == [False], (corner, axis)  # also where the sides that decide are finite (corner 0 or 3)
    assert D.sideways(np.full((1, 4, 2), NAN, np.float32)).tolist() == [False]


def test_the_split_is_stable_and_turns_by_the_table():
    H, W = 301, 517
    quads = np.stack([box(10, 10, 40, 10), box(100, 20, 10, 40), box(20, 50, 40, 10), box(200, 30.5, 10, 40), box(300, 5, 9, 70), box(30, 90, 40, 10)])
    got = D.axis_split(quads, H, W)
    assert got["word_offs"].tolist() == [0, 3, 6] and got["page_of_word"].tolist() == [0, 0, 0, 1, 1, 1]
    assert got["source_index"].tolist() == [0, 2, 5, 1, 3, 4]  # each page in input order
    assert np.array_equal(got["quads"][:3], quads[[0, 2, 5]])
    for row, src in zip(got["quads"][3:], quads[[1, 3, 4]]):  # (x, y) -> (y, (W-1) - x): the inverse of k = 1 of the orientation table
        assert row.tolist() == [[float(y), float(W - 1 - x)] for x, y in src.tolist()]
        back = np.stack(O.turn_point(row[:, 0].astype(np.float64), row[:, 1].astype(np.float64), 1, H, W), axis=1)
        assert np.array_equal(back, src.astype(np.float64))
    assert got["quads"].dtype == np.float32
    # a vertical word is a horizontal word of the turned page: the split of the turned rows finds nothing sideways
    assert not D.sideways(got["quads"][3:]).any()
    part = D.axis_split(quads, H, W, count=4)
    assert part["word_offs"].tolist() == [0, 2, 4] and part["source_index"].tolist() == [0, 2, 1, 3]
    assert D.axis_split(quads, H, W, count=0)["word_offs"].tolist() == [0, 0, 0] and D.axis_split(quads, H, W, count=99)["word_offs"].tolist() == [0, 3, 6]
    assert D.axis_split(quads[[0, 2]], H, W)["word_offs"].tolist() == [0, 2, 2] and D.axis_split(quads[[1]], H, W)["word_offs"].tolist() == [0, 0, 1]


def test_the_flip_of_a_valid_span():
    batch = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 1, 3, 5) + 1
    got = D.flip_crops(batch, [3, 5])
    assert got[0, 0].tolist() == [[13, 12, 11, 4, 5], [8, 7, 6, 9, 10], [3, 2, 1, 14, 15]]  # columns 3 and 4 are pad: untouched, not zeroed
    assert np.array_equal(got[1, 0], batch[1, 0, ::-1, ::-1])
    assert np.array_equal(D.flip_crops(got, [3, 5]), batch)  # twice is the identity
    assert np.array_equal(D.flip_crops(batch, [3, 5], [0, 0]), batch)
    only = D.flip_crops(batch, [3, 5], [0, 1])
    assert np.array_equal(only[0], batch[0]) and np.array_equal(only[1], got[1])
    assert np.array_equal(D.flip_crops(batch, [0, 1]), np.concatenate([batch[:1], np.concatenate([batch[1:, :, ::-1, :1], batch[1:, :, :, 1:]], axis=3)]))
    assert np.array_equal(D.flip_crops(batch, [9, -2])[0, 0], batch[0, 0, ::-1, ::-1])  # widths are clamped to the batch


def test_the_flag_rule():
    s_plain = [-1.0, -1.0, -1.0, -1.0, np.nan, -1.0, np.nan, -2.0]
    s_flip = [-0.5, -1.0, -1.5, -0.5, -0.5, np.nan, np.nan, np.nextafter(-2.0, 0.0)]
    probe = [1, 1, 1, 0, 1, 1, 1, 1]
    assert D.flip_flags(s_plain, s_flip, probe).tolist() == [1, 0, 0, 0, 0, 0, 0, 1]  # larger; equal; smaller; unprobed; NaN either side; one ulp
    assert D.flip_flags(s_plain, s_flip, [7] * 8).tolist() == [1, 0, 0, 1, 0, 0, 0, 1]  # any non-zero mask probes
    assert [D.direction(False, False), D.direction(False, True), D.direction(True, False), D.direction(True, True)] == [0, 0, 1, 3]


def _line(x, n, block=None, spine=False):
    """a line of n words running along x from x, as the line stage finds it on its (virtual) page"""
    words = [box(x + 10.0 * k, 20, 8, 4).tolist() for k in range(n)]
    d = {"quad": box(x, 20, 10 * n - 2, 4).tolist(), "text": f"t{x}", "words": words}
    if spine:
        d["spine"] = [pt for k in range(n) for pt in ([x + 10.0 * k, 22.0], [x + 10.0 * k + 8, 22.0])]
        d["height"] = 4.0
    d["log_prob"] = -1.5
    if block is not None:
        d["block"] = block
    return d


def test_mixed_results_keys_reversal_and_block_offset():
    from ocrs_models_amd import inference as inf

    H, W = 100, 200
    flat = [_line(0, 2, 0, True), _line(10, 1, 0, True), _line(20, 3, 1, True), _line(30, 3, 0, True), _line(40, 2, 0, True), _line(50, 2, 1, True)]
    # reading order: position k holds line line_at[k]; the flags and scores are per LINE
    line_at = [1, 0, 2, 4, 3, 5]
    flags, scores = [0, 0, 0, 0, 1, 0], [[-9.0, -9.5]] * 3 + [[-1.0, -2.0], [-3.0, -2.0], [-4.0, -4.0]]
    got = inf.mixed_results(flat, [0, 3, 6], line_at, flags, scores, H, W)
    assert [g["direction"] for g in got] == [0, 0, 0, 3, 1, 1]
    assert [g["direction_scores"] for g in got] == [None, None, None, [-3.0, -2.0], [-1.0, -2.0], [-4.0, -4.0]]
    assert [g["block"] for g in got] == [0, 0, 1, 2, 2, 3]  # page 1's blocks count on from page 0's two
    assert all(list(g) == ["quad", "text", "words", "spine", "height", "log_prob", "direction", "direction_scores", "block"] for g in got)
    assert got[:3] == [{**{k: v for k, v in f.items() if k != "block"}, "direction": 0, "direction_scores": None, "block": f["block"]} for f in flat[:3]]
    for g, f in zip(got[3:], flat[3:]):
        turned = O.turn_results([f], 1, H, W)[0]
        assert g["quad"] == turned["quad"] and g["text"] == f["text"] and g["height"] == f["height"] and "turns" not in g
        if g["direction"] == 3:  # reads upwards: the last word first, every word from its former right edge
            assert g["words"] == turned["words"][::-1] and g["spine"] == turned["spine"][::-1]
            ys = [pt[1] for pt in g["spine"]]
            assert ys == sorted(ys, reverse=True)
        else:
            assert g["words"] == turned["words"] and g["spine"] == turned["spine"]
    # without reading order: no "block", the keys at the end; a page without upright lines; a page without sideways ones
    plain = [{k: v for k, v in _line(0, 2).items()}, _line(30, 2)]
    got = inf.mixed_results(plain, [0, 1, 2], [0, 1], [0, 1], [[0.0, 0.0], [-2.0, -1.0]], H, W)
    assert [list(g) for g in got] == [["quad", "text", "words", "log_prob", "direction", "direction_scores"]] * 2
    assert [g["direction"] for g in got] == [0, 3] and got[1]["words"] == O.turn_results(plain[1:], 1, H, W)[0]["words"][::-1]
    only_side = inf.mixed_results([_line(30, 2, 0), _line(40, 2, 1)], [0, 0, 2], [0, 1], [0, 0], [[-1.0, -1.0]] * 2, H, W)
    assert [g["block"] for g in only_side] == [0, 1] and [g["direction"] for g in only_side] == [1, 1]
    only_up = inf.mixed_results([_line(30, 2, 0), _line(40, 2, 1)], [0, 2, 2], [0, 1], [0, 0], [[-1.0, -1.0]] * 2, H, W)
    assert [g["block"] for g in only_up] == [0, 1] and [g["direction_scores"] for g in only_up] == [None, None]
    assert inf.mixed_results([], [0, 0, 0], [], [], [], H, W) == []


@pytest.mark.parametrize("bad", ["Mixed", "vertical", True, 1, 0, ["mixed"], ("mixed",), b"mixed"])
def test_a_bad_directions_value_is_refused_before_any_device_use(bad):
    from ocrs_models_amd import inference as inf

    page = torch.zeros(1, 40, 30, dtype=torch.uint8)
    quads = torch.zeros(3, 4, 2)
    for call in (lambda: inf.ocr_lines(None, None, page, directions=bad), lambda: inf.read_lines(None, page, quads, directions=bad),
                 lambda: inf.ocr_lines(None, None, page, directions=bad, orientation=1), lambda: inf.read_lines(None, page, quads, directions=bad, rectify="chain")):
        with pytest.raises(RuntimeError, match="directions must be None or"):
            call()


def test_mixed_with_chars_is_refused_before_any_device_use():
    from ocrs_models_amd import inference as inf

    page = torch.zeros(1, 40, 30, dtype=torch.uint8)
    quads = torch.zeros(3, 4, 2)
    for call in (lambda: inf.ocr_lines(None, None, page, directions="mixed", chars=True), lambda: inf.read_lines(None, page, quads, directions="mixed", chars=True),
                 lambda: inf.ocr_lines(None, None, page, directions="mixed", chars=True, beam_width=4)):
        with pytest.raises(RuntimeError, match="does not go with chars"):
            call()
    # the other keywords' errors still come first or alike; a valid call on a CPU page fails at the device check, not silently
    with pytest.raises(RuntimeError, match="rectify"):
        inf.read_lines(None, page, quads, directions="mixed", rectify="spline")
    with pytest.raises(RuntimeError, match="orientation"):
        inf.read_lines(None, page, quads, directions="mixed", orientation=7)
    with pytest.raises(RuntimeError):
        inf.read_lines(None, page, quads, directions="mixed")
    with pytest.raises(RuntimeError):
        inf.ocr_lines(None, None, page, directions="mixed")


def test_device_functions_have_no_cpu_path():
    from ocrs_models_amd import inference as inf

    for call in (lambda: inf.split_by_axis(torch.zeros(2, 4, 2), 10, 10), lambda: inf.flip_crops(torch.zeros(1, 1, 8, 4), torch.tensor([4])),
                 lambda: inf.flip_flags(torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(RuntimeError):
            call()

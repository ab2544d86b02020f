"""The orientation rules on the CPU: the numpy restatement (tests/orient_ref.py) against np.rot90 and hand-worked cases, the package's host half
(``turn_results``, the argument checks that come before any device use) against the restatement.  DESIGN.md §22."""
import numpy as np
import pytest
import torch

from tests import ocr_ref as R
from tests import orient_ref as O

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 8), (6, 6)]


def box(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=np.float32)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_table_is_where_rot90_moves_a_marked_pixel(k):
    for H, W in SHAPES:
        assert O.turn_shape(H, W, k) == np.rot90(np.zeros((H, W)), k).shape
        for Y in range(H):
            for X in range(W):
                page = np.zeros((H, W), dtype=np.uint8)
                page[Y, X] = 1
                (y,), (x,) = np.nonzero(np.rot90(page, k))  # where the pixel sits on the turned page
                assert O.turn_point(int(x), int(y), k, H, W) == (X, Y)
                assert O.turn_point(X, Y, k, H, W, inverse=True) == (int(x), int(y))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_the_table_round_trips_and_keeps_corner_order(k):
    H, W = 37, 52
    r = np.random.RandomState(k)
    for dtype in (np.float64, np.float32):
        q = (r.randint(-20, 140, (50, 4, 2)) * 0.5).astype(dtype)  # integers and half-integers: every subtraction is exact
        there = O.turn_quads(q, k, H, W, dtype=dtype)
        assert there.dtype == dtype and np.array_equal(O.turn_quads(there, k, H, W, inverse=True, dtype=dtype), q)
        assert np.array_equal(O.turn_quads(O.turn_quads(q, k, H, W, inverse=True, dtype=dtype), k, H, W, dtype=dtype), q)
    quad = R.rotated_rect(20.0, 15.0, 12.0, 4.0, 25).astype(np.float64)
    turned = O.turn_quads(quad, k, H, W, inverse=True)

    def area(p):  # signed: the winding
        return 0.5 * float(np.sum(p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]))

    assert abs(area(turned) - area(quad)) < 1e-9  # a proper rotation: no mirror
    for j in range(4):  # corner j -> corner j, side lengths kept
        assert abs(np.linalg.norm(turned[(j + 1) % 4] - turned[j]) - np.linalg.norm(quad[(j + 1) % 4] - quad[j])) < 1e-9
    # four quarter turns are the identity: turning by k then by 4 - k
    back = O.turn_quads(turned, (4 - k) % 4, *O.turn_shape(H, W, k), inverse=True)
    assert np.allclose(back, quad, atol=1e-12)


def test_turn_results_maps_the_coordinate_keys_only():
    from ocrs_models_amd import inference as inf

    d = {"quad": box(2, 3, 10, 4).tolist(), "text": "ab", "words": [box(2, 3, 4, 4).tolist(), box(8, 3, 4, 4).tolist()], "spine": [[2.0, 5.0], [6.0, 5.0]],
         "height": 4.0, "char_quads": [box(2, 3, 2, 4).tolist(), box(8.5, 3, 2, 4).tolist()], "char_log_probs": [-0.5, -0.25], "log_prob": -1.0,
         "word_chars": [[0, 1], [1, 2]], "word_texts": ["a", "b"], "block": 0}
    empty = {"quad": box(0, 0, 1, 1).tolist(), "text": "", "char_quads": [], "char_log_probs": []}
    H, W = 30, 40
    for k in range(4):
        got = inf.turn_results([d, empty], k, H, W)
        assert got == O.turn_results([d, empty], k, H, W)
        assert list(got[0]) == [*d, "turns"] and got[0]["turns"] == k and got[1]["char_quads"] == []
        for key in d:
            if key not in O.COORD_KEYS:
                assert got[0][key] == d[key]
        assert got[0]["quad"] == O.turn_quads(np.array(d["quad"]), k, H, W).tolist()
        assert got[0]["words"] == O.turn_quads(np.array(d["words"]), k, H, W).tolist()
    assert inf.turn_results([d], 0, H, W)[0]["quad"] == d["quad"]
    assert inf.turn_results([d], 1, H, W)[0]["quad"][0] == [W - 1 - 3.0, 2.0]
    assert inf.turn_shape(3, 5, 1) == (5, 3) and inf.turn_shape(3, 5, 2) == (3, 5)


def test_votes_and_picks_on_hand_made_quads():
    quads = np.stack([
        box(0, 0, 30, 10),     # 0: horizontal, length 30
        box(0, 20, 10, 40),    # 1: vertical, length 40
        box(50, 0, 15, 10),    # 2: aspect exactly 1.5: votes, horizontal 15
        box(50, 20, 14.5, 10), # 3: aspect just below 1.5: no vote
        box(80, 0, 10, 10),    # 4: a square: no vote
        box(0, 70, 30, 0),     # 5: zero area: no vote (short side 0)
        box(5, 5, 0, 0),       # 6: a point: no vote
        box(0, 80, 30, 10),    # 7: as long as quad 0: the tie goes to the smaller index
        R.rotated_rect(100.0, 100.0, 20.0, 5.0, 30),   # 8: 30 degrees: horizontal, 20
        R.rotated_rect(100.0, 150.0, 50.0, 5.0, 80),   # 9: steep: vertical, 50
    ])
    v = O.votes(quads, 1.5, 4)
    assert v["voter"].tolist() == [True, True, True, False, False, False, False, True, True, True]
    assert v["voters"] == 6 and v["K"] == 4 and v["picks"] == [9, 1, 0, 7]
    lng, _, horiz = O.long_sides(quads)
    assert horiz[[0, 1, 2, 7, 8, 9]].tolist() == [True, False, True, True, True, False] and abs(float(lng[8]) - 20.0) < 1e-5
    assert v["V"] == 40.0 + float(lng[9]) and abs(v["H"] - (30.0 + 15.0 + 30.0 + float(lng[8]))) < 1e-12
    more = O.votes(quads, 1.5, 64)
    assert more["K"] == 6 and more["picks"] == [9, 1, 0, 7, 8, 2] + [-1] * 58 and (more["H"], more["V"]) == (v["H"], v["V"])
    assert O.votes(quads[:0])["voters"] == 0 and O.votes(quads[:0], sample=3)["picks"] == [-1, -1, -1]
    # exactly 45 degrees with exact coordinates: |x| == |y| counts as horizontal; a hair steeper does not
    diag = np.array([[0, 0], [16, 16], [14, 18], [-2, 2]], dtype=np.float32)
    steeper = np.array([[0, 0], [16, 17], [14, 19], [-2, 2]], dtype=np.float32)
    assert O.long_sides(diag[None])[2].tolist() == [True] and O.long_sides(steeper[None])[2].tolist() == [False]
    # the tie rule of the sides: a square votes for nobody, but its long side is the one with the larger |x|
    assert O.long_sides(box(0, 0, 10, 10)[None])[2].tolist() == [True] and O.long_sides(np.roll(box(0, 0, 10, 10), 1, axis=0)[None])[2].tolist() == [True]
    # min_aspect reaches the rule
    assert O.votes(quads, 1.0, 64)["voters"] == 8 and O.votes(quads, 3.5, 64)["voters"] == 3


def test_path_confidence_and_the_decision():
    lp = np.log(np.array([[[0.5, 0.25, 0.25], [0.1, 0.1, 0.8]], [[0.25, 0.5, 0.25], [1 / 3, 1 / 3, 1 / 3]]]))  # (T=2, B=2, C=3)
    got = O.path_confidence(lp, [2, 1])
    assert np.allclose(got, [np.log(0.5), np.log(0.8)], atol=1e-15)
    assert O.decide(10.0, 10.0, {0: -1.0, 2: -1.0}.get) == {"a": 0, "scores": (-1.0, -1.0), "turns": 0}  # both comparisons are strict
    assert O.decide(10.0, 10.5, {1: -1.0, 3: -0.5}.get)["turns"] == 3 and O.decide(10.0, 10.5, {1: -0.5, 3: -1.0}.get)["turns"] == 1
    assert O.decide(11.0, 10.5, {0: -2.0, 2: -0.5}.get)["turns"] == 2
    assert O.mean_in_order([1.0, 2.0, 4.5]) == 2.5


BAD = [True, False, 4, -1, "upright", 1.0, [0], (1,)]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_a_bad_orientation_is_refused_before_any_device_use(bad):
    """the page is a CPU tensor and the models are None: anything that got past the argument check would fail differently"""
    from ocrs_models_amd import inference as inf

    page = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: inf.ocr_page(None, None, page, orientation=bad), lambda: inf.ocr_lines(None, None, page, orientation=bad)):
        with pytest.raises(RuntimeError, match="orientation"):
            call()
    if not isinstance(bad, (list, tuple)):
        with pytest.raises(RuntimeError, match="orientation"):
            inf.ocr_pages(None, None, [page], orientation=bad)
        with pytest.raises(RuntimeError, match="orientation"):
            inf.ocr_pages(None, None, [page, page], orientation=[0, bad])
        with pytest.raises(RuntimeError, match="orientation"):
            inf.turn_page(page, bad)
        with pytest.raises(RuntimeError, match="orientation"):
            inf.turn_quads(torch.zeros(1, 4, 2), bad, 8, 8)
    for who in (inf.read_words, inf.read_lines):
        with pytest.raises(RuntimeError, match="orientation"):
            who(None, page, torch.zeros(1, 4, 2), orientation=bad)


def test_orientation_lists_need_one_entry_per_page():
    from ocrs_models_amd import inference as inf

    page = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for pages, bad in (([page, page], [0]), ([page], [0, 1]), ([], [0]), ([page], [])):
        with pytest.raises(RuntimeError, match="one entry per page"):
            inf.ocr_pages(None, None, pages, orientation=bad)
    with pytest.raises(RuntimeError, match="orientation"):  # "auto" needs a detector: the read_* halves take the caller's int only
        inf.read_lines(None, page, torch.zeros(1, 4, 2), orientation="auto")
    assert inf.ocr_pages(None, None, [], orientation="auto") == [] and inf.ocr_pages(None, None, [], orientation=[]) == []


def test_device_functions_have_no_cpu_path():
    from ocrs_models_amd import inference as inf

    page = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        inf.turn_page(page, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        inf.turn_page(page, 0)  # (k = 0 returns its input, but only a page the other turns would take)
    with pytest.raises(RuntimeError, match="GPU"):
        inf.turn_quads(torch.zeros(1, 4, 2), 1, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        inf.orientation_votes(torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        inf.path_confidence(torch.zeros(2, 1, 3), torch.ones(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        inf.ocr_page(None, None, page, orientation=1)

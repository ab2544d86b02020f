"""CPU only: pins tests/lines_ref.py, the numpy restatement of the text-line rule, on hand-made cases.  The GPU tests
(tests/test_lines_gpu.py) compare csrc/text_lines.hip against this restatement, so what it means is fixed here first."""
import numpy as np
import pytest

from tests import lines_ref as R


def lines_of(quads, **kw):
    return R.find_lines(quads, **kw)["lines"]


def test_a_row_breaks_at_a_wide_gap():
    quads, want = R.case_row_gap_row()
    r = R.find_lines(quads)
    assert r["lines"] == want == [[0, 1, 2], [3, 4]]
    assert r["next_word"].tolist() == [1, 2, -1, 4, -1]
    assert r["line_of_word"].tolist() == [0, 0, 0, 1, 1] and r["word_order"].tolist() == [0, 1, 2, 3, 4] and r["line_offsets"].tolist() == [0, 3, 5]
    # the line quad of axis-aligned words is their bounding box, first corner top left, clockwise
    assert r["quads"][0].tolist() == [[0, 0], [220, 0], [220, 20], [0, 20]] and r["quads"][1].tolist() == [[300, 0], [440, 0], [440, 20], [300, 20]]
    # the gap of 4 h is what breaks it: the same five words 1 h apart are one line
    assert lines_of(np.stack(R.row_of_words(0, 0, 5))) == [[0, 1, 2, 3, 4]]
    # and max_gap is the parameter that decides: 4 h links with max_gap = 4
    assert lines_of(quads, max_gap=4.0) == [[0, 1, 2, 3, 4]]


def test_two_words_choose_one_successor_and_the_nearer_wins():
    quads, want = R.case_competing()
    r = R.find_lines(quads)
    assert r["lines"] == want == [[0], [1, 2]]
    assert r["next_word"].tolist() == [-1, 2, -1]
    f = R.word_frames(quads)
    p0, p1 = (R.pair_terms(f, i, R.MAX_GAP, R.MIN_COS, np.float32) for i in (0, 1))
    assert R.candidates(p0).tolist() == [False, False, True] and R.candidates(p1).tolist() == [False, False, True]  # both chose word 2
    assert p0["s"][2] == 90 and p1["s"][2] == 70


def test_equal_s_is_decided_by_the_index():
    quads, want = R.case_accept_tie()  # two choosers at the same s: the smaller k is accepted
    assert lines_of(quads) == want == [[0, 2], [1]]
    r = R.find_lines(quads[[1, 0, 2]])  # the other word has index 0 now, and wins; it lies lower, so its line sorts second
    assert r["next_word"].tolist() == [2, -1, -1] and r["lines"] == [[1], [0, 2]]
    for swap in (False, True):  # two candidates at the same s: the smaller j is chosen
        quads, want = R.case_choice_tie(swap)
        r = R.find_lines(quads)
        assert r["lines"] == want and r["next_word"].tolist() == [-1, -1, 0]


def test_a_vertical_stack_of_wide_words_never_links():
    quads = np.stack([R.box(0, 30 * k, 60, 20) for k in range(4)])
    f = R.word_frames(quads)
    assert f["ux"].tolist() == [1.0] * 4 and f["uy"].tolist() == [0.0] * 4
    r = R.find_lines(quads)
    assert r["lines"] == [[0], [1], [2], [3]] and (r["next_word"] == -1).all()
    assert np.array_equal(r["quads"], quads)  # one-word lines are the words' quads


def test_a_stack_of_tall_boxes_links_downward():
    quads = np.stack([R.box(0, 80 * k, 20, 60) for k in range(4)])
    f = R.word_frames(quads)
    assert f["ux"].tolist() == [0.0] * 4 and f["uy"].tolist() == [1.0] * 4 and f["lng"].tolist() == [60.0] * 4
    r = R.find_lines(quads[::-1])  # given bottom-up: the links still run down the page (d.x == 0 and d.y > 0)
    assert r["lines"] == [[3, 2, 1, 0]] and r["next_word"].tolist() == [-1, 0, 1, 2]
    # corners (minU,minV), (maxU,minV), (maxU,maxV), (minU,maxV) with u = (0, 1), v = (-1, 0)
    assert r["quads"][0].tolist() == [[20, 0], [20, 300], [0, 300], [0, 0]]


@pytest.mark.parametrize("case", ["grid", "rotated", "random"])
def test_every_word_is_in_exactly_one_line(case):
    if case == "grid":
        quads = R.grid_case(7, 9, seed=3)
    elif case == "rotated":
        quads = R.rotated_case()
    else:
        r = np.random.RandomState(5)
        quads = np.stack([R.rotated_rect(r.uniform(0, 900), r.uniform(0, 500), r.uniform(20, 90), r.uniform(8, 30), r.uniform(-90, 90)) for _ in range(150)])
    n = len(quads)
    r = R.find_lines(quads)
    assert sorted(r["word_order"].tolist()) == list(range(n))
    assert sorted(i for c in r["lines"] for i in c) == list(range(n))
    assert r["line_offsets"][0] == 0 and r["line_offsets"][-1] == n and len(r["line_offsets"]) == r["n_lines"] + 1
    for l, c in enumerate(r["lines"]):
        assert r["word_order"][r["line_offsets"][l]:r["line_offsets"][l + 1]].tolist() == c and (r["line_of_word"][c] == l).all()
    nxt = r["next_word"]
    linked = nxt[nxt >= 0]
    assert len(set(linked.tolist())) == len(linked)  # in-degree <= 1 (out-degree <= 1 by construction)
    f = R.word_frames(quads)
    keys = [(f["cy"][c[0]], f["cx"][c[0]], c[0]) for c in r["lines"]]
    assert keys == sorted(keys)


def test_shuffling_the_words_keeps_the_set_of_lines():
    quads = R.rotated_case()  # no ties: decision_margin says so
    assert R.decision_margin(quads) > 1.0
    base = R.find_lines(quads)

    def as_sets(q, r):
        return {frozenset(q[i].tobytes() for i in c) for c in r["lines"]}

    want = as_sets(quads, base)
    for seed in range(3):
        perm = np.random.RandomState(seed).permutation(len(quads))
        got = R.find_lines(quads[perm])
        assert as_sets(quads[perm], got) == want
        # and the lines come in the same order with the same quads (multi-word quads differ only in the order of a sum: not here, chain order)
        assert np.array_equal(got["quads"], base["quads"])


def test_float32_and_float64_agree_on_the_integer_lattice():
    for quads in (R.grid_case(6, 11, seed=1), np.stack([R.box(0, 80 * k, 20, 60) for k in range(5)]), R.case_competing()[0], R.case_row_gap_row()[0]):
        a, b = R.find_lines(quads, dtype=np.float32), R.find_lines(quads, dtype=np.float64)
        for k in ("next_word", "line_of_word", "word_order", "line_offsets"):
            assert np.array_equal(a[k], b[k]), k
        assert a["quads"].dtype == np.float32 and b["quads"].dtype == np.float64 and np.array_equal(a["quads"].astype(np.float64), b["quads"])


def test_rotated_case_is_away_from_every_threshold():
    """the construction the GPU test relies on: float32 and float64 take the same decisions, with at least a pixel to spare"""
    quads = R.rotated_case()
    assert R.decision_margin(quads) > 1.0
    a, b = R.find_lines(quads, dtype=np.float32), R.find_lines(quads, dtype=np.float64)
    assert a["lines"] == b["lines"] and max(len(c) for c in b["lines"]) == 7 and sum(len(c) == 1 for c in b["lines"]) == 10
    err = np.abs(a["quads"].astype(np.float64) - b["quads"]).max()
    assert err <= 8 * R.ulp32(np.abs(b["quads"]).max())

"""The numpy restatement of the reading-order rule (tests/reading_ref.py) pinned on hand-made cases, without a GPU."""
import numpy as np
import pytest

from tests import reading_ref as RR


def _read(quads, **kw):
    r32, r64 = RR.reading_order(quads, dtype=np.float32, **kw), RR.reading_order(quads, dtype=np.float64, **kw)
    # integer boxes: the float32 and float64 forms agree in everything
    assert r32["line_order"].tolist() == r64["line_order"].tolist() and r32["new_block"].tolist() == r64["new_block"].tolist()
    assert np.array_equal(r32["before"], r64["before"]) and r32["forced"] == r64["forced"]
    assert r32["ext"]["yc"].dtype == np.float32 and r64["ext"]["yc"].dtype == np.float64
    assert sorted(r32["line_order"].tolist()) == list(range(len(quads)))
    return r32


def test_two_columns_read_column_by_column():
    quads, names, want = RR.case_two_columns()
    # the fixture: handed over as find_lines orders lines, the columns interleave
    assert names[:5] == ["H1", "B0", "A0", "B1", "A1"] and names[10:13] == ["H2", "D0", "C0"] and names != want
    r = _read(quads)
    assert [names[i] for i in r["line_order"]] == want
    assert want == ["H1"] + [f"A{k}" for k in range(4)] + [f"B{k}" for k in range(5)] + ["H2"] + [f"C{k}" for k in range(3)] + [f"D{k}" for k in range(3)]
    assert r["forced"] == 0
    # blocks at block_gap = 1: the heading stands alone (gap 24 > 20), a column is a block, H2 follows B4 at exactly 20 <= 20
    starts = [n for n, f in zip(want, r["new_block"]) if f]
    assert starts == ["H1", "A0", "B0", "C0", "D0"]
    assert RR.blocks_of(r["line_order"], r["new_block"]) == [0] + [1] * 4 + [2] * 6 + [3] * 3 + [4] * 3


def test_three_columns_read_column_by_column():
    quads, names, want = RR.case_three_columns()
    assert names[:4] == ["P0", "Q0", "R0", "P1"]
    r = _read(quads)
    assert [names[i] for i in r["line_order"]] == want == [f"P{k}" for k in range(5)] + [f"Q{k}" for k in range(3)] + [f"R{k}" for k in range(6)]
    assert r["forced"] == 0
    assert [n for n, f in zip(want, r["new_block"]) if f] == ["P0", "Q0", "R0"]


def test_a_cycle_forces_an_emission():
    quads = RR.case_cycle()
    e = RR.extents(quads)
    assert e["x0"].tolist() == [c[0] for c in RR.CYCLE] and e["x1"].tolist() == [c[1] for c in RR.CYCLE] and e["yc"].tolist() == [c[2] for c in RR.CYCLE]
    r = _read(quads)
    assert r["forced"] >= 1
    assert r["line_order"].tolist() == RR.CYCLE_ORDER
    # lines 2 and 3 are free; after them every remaining line has a remaining line before it
    rest = r["before"][[0, 1, 4, 5, 6, 7]][:, [0, 1, 4, 5, 6, 7]]
    assert not r["before"][:, 2].any() and rest.any(0).all()


def test_one_line():
    r = _read(RR.xyxy(5, 7, 90, 21)[None])
    assert r["line_order"].tolist() == [0] and r["new_block"].tolist() == [1] and r["before"].tolist() == [[False]] and r["forced"] == 0


def test_one_row_of_five_reads_left_to_right():
    quads = np.stack([RR.xyxy(100 * k, 3 * ((k * 2) % 5), 100 * k + 80, 3 * ((k * 2) % 5) + 20) for k in range(5)])[[3, 0, 4, 2, 1]]
    r = _read(quads)
    assert [int(quads[i, 0, 0]) for i in r["line_order"]] == [0, 100, 200, 300, 400]
    assert r["new_block"].tolist() == [1] * 5 and r["forced"] == 0  # no two overlap: rule 1 never holds


def test_equal_yc_takes_the_index_tie_break():
    a, b = RR.xyxy(0, 10, 100, 30), RR.xyxy(50, 5, 150, 35)  # both yc = 20
    for quads, first in ((np.stack([a, b]), 0), (np.stack([b, a]), 0)):
        r = _read(quads)
        assert r["line_order"].tolist() == [first, 1 - first]
        assert r["before"].tolist() == [[False, True], [False, False]]
    assert RR.decision_margin(np.stack([a, b])) == 0.0


@pytest.mark.parametrize("gap,flags", [(20, [1, 0]), (21, [1, 1]), (19, [1, 0])])
def test_block_flags_just_inside_and_outside_the_gap(gap, flags):
    """two lines 20 high, one below the other: block_gap * max(sht) = 20 at the default"""
    quads = np.stack([RR.xyxy(0, 0, 200, 20), RR.xyxy(10, 20 + gap, 150, 40 + gap)])
    assert _read(quads)["new_block"].tolist() == flags
    assert _read(quads, block_gap=1.05)["new_block"].tolist() == [1, 0]
    assert _read(quads, block_gap=0.9)["new_block"].tolist() == [1, 1]


def test_blocks_need_rule_one():
    """the next line of the order lies to the right, not below: a new block whatever the gap"""
    quads = np.stack([RR.xyxy(0, 0, 100, 20), RR.xyxy(120, 4, 220, 24)])
    r = _read(quads, block_gap=100.0)
    assert r["line_order"].tolist() == [0, 1] and r["new_block"].tolist() == [1, 1]


def test_a_blocker_keeps_the_columns_of_two_sections_apart():
    """A | B above a heading that spans both, C | D below it: A is before B, but not before D (the heading blocks rule 2), so the order is
    A, B, heading, C, D and not A, C, ..."""
    quads = np.stack([RR.xyxy(0, 4, 100, 24), RR.xyxy(120, 0, 220, 20), RR.xyxy(0, 40, 220, 60), RR.xyxy(120, 80, 220, 100), RR.xyxy(0, 84, 100, 104)])
    r = _read(quads)
    assert r["before"][0, 1] and not r["before"][0, 3] and not r["before"][4, 1] and r["before"][4, 3]
    assert r["line_order"].tolist() == [0, 1, 2, 4, 3]


def test_pages_are_never_related():
    q1, _, _ = RR.case_two_columns()
    q2 = RR.case_cycle()
    quads, offs = np.concatenate([q1, q2, q1]), [0, len(q1), len(q1), len(q1) + len(q2), 2 * len(q1) + len(q2)]
    r = RR.reading_order(quads, offs)
    one, two = RR.reading_order(q1), RR.reading_order(q2)
    a, b = len(q1), len(q1) + len(q2)
    assert r["line_order"].tolist() == one["line_order"].tolist() + (two["line_order"] + a).tolist() + (one["line_order"] + b).tolist()
    assert r["new_block"].tolist() == one["new_block"].tolist() + two["new_block"].tolist() + one["new_block"].tolist()
    assert not r["before"][:a, a:].any() and not r["before"][a:, :a].any() and not r["before"][a:b, b:].any() and not r["before"][b:, :b].any()
    assert np.array_equal(r["before"][a:b, a:b], two["before"])
    assert RR.blocks_of(r["line_order"], r["new_block"], offs)[a] == 0


def test_peel_of_a_hand_made_matrix():
    """a 3-cycle 0 -> 1 -> 2 -> 0, then a chain 3 -> 4 -> 5 hanging off 2: line 0 is forced, which frees 1, then 2, then the chain"""
    before = np.zeros((6, 6), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5)):
        before[a, b] = True
    order, forced = RR.peel(before, [0, 6])
    assert order.tolist() == [0, 1, 2, 3, 4, 5] and forced == 1
    # the same graph with the indices mirrored, 5 -> 4 -> 3 -> 5 and 3 -> 2 -> 1 -> 0: the chain now hangs below the cycle, nothing is free
    # until 3 is emitted, and the smallest index is forced four times
    order, forced = RR.peel(before[::-1, ::-1], [0, 6])
    assert order.tolist() == [0, 1, 2, 3, 5, 4] and forced == 4


def test_pack_bits_layout():
    before = np.zeros((40, 40), dtype=bool)
    before[1, 0] = before[1, 31] = before[2, 32] = before[39, 39] = True
    w = RR.pack_bits(before, 70)
    assert w.shape == (70, 3) and w.dtype == np.uint32
    assert w[1].tolist() == [0x80000001, 0, 0] and w[2].tolist() == [0, 1, 0] and w[39].tolist() == [0, 1 << 7, 0] and int(w.sum()) == 0x80000001 + 1 + 128


def test_decision_margin_reports_the_nearest_threshold():
    quads, _, _ = RR.case_two_columns()
    assert RR.decision_margin(quads) == 0.0                 # H2 follows B4 at exactly block_gap * 20
    assert RR.decision_margin(quads, block_gap=0.7) == 4.0  # A_k and B_k: yc 4 apart; every gap is at least 4 from 14
    shifted = quads.copy()
    shifted[1, :, 1] += 3.25                                # B0 now 0.75 above A0
    assert RR.decision_margin(shifted, block_gap=0.7) == 0.75
    near = np.stack([RR.xyxy(0, 0, 100, 20), RR.xyxy(100.5, 40, 200, 60)])
    assert RR.decision_margin(near) == 0.5                  # the overlap test: 0.5 from touching


def test_the_wide_cases_of_the_gpu_tests():
    """what tests/test_reading_gpu.py relies on: three or four columns read column by column, and the spanning lines do block"""
    for n, cols, kw in ((257, 3, {}), (513, 3, {})):
        q = RR.columns_case(n, cols, **kw)
        r = RR.reading_order(q)
        xs = q[r["line_order"], 0, 0]
        assert r["forced"] == 0 and (np.diff(xs) >= 0).all() and int(r["new_block"].sum()) == cols
    plain, spanned = RR.columns_case(120, 4, h=4, row_pitch=7), RR.columns_case(120, 4, h=4, row_pitch=7, headers=(10, 20))
    assert len(spanned) == 122
    r0, r1 = RR.reading_order(plain), RR.reading_order(spanned)
    assert (np.diff(plain[r0["line_order"], 0, 0]) >= 0).all() and not (np.diff(spanned[r1["line_order"], 0, 0]) >= 0).all()
    assert r1["before"].sum() < RR.reading_order(np.concatenate([plain, spanned[:0]]))["before"].sum() + 2 * 121  # pairs across a spanning line are gone


def test_page_text_joins_lines_and_blocks():
    from ocrs_models_amd.inference import page_text

    lines = [{"text": t, "block": b} for t, b in (("Heading", 0), ("left one", 1), ("left two", 1), ("right one", 2))]
    assert page_text(lines) == "Heading\n\nleft one\nleft two\n\nright one"
    assert page_text([{"text": "a"}, {"text": "b"}]) == "a\nb" and page_text([]) == "" and page_text(lines[:1]) == "Heading"

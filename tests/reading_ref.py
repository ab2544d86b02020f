"""CPU restatement of the reading-order rule in plain numpy, for the tests of csrc/reading_order.hip.  Written once with a
dtype parameter: in float32 every operation is the kernel's, in the kernel's order, with one rounding each; in float64 it is the comparand
for inputs whose comparisons are away from their thresholds.  Nothing here calls the package's kernels.

The rule.  Input: the line quads (L,4,2) float32 of one page in line order (``find_lines``' own: top to bottom), or of several pages with
``offs`` (B+1,), the lines of page p at offs[p]:offs[p+1].  Every relation holds between lines of one page only; indices are flat.

* Page axis.  u_l, lng_l, sht_l of every line by §14's word-frame rule applied to the line quad (``lines_ref.word_frames``).
  U = normalise(sum of lng_l * u_l), the sum started at 0 and taken one line after the other in line order; a zero sum gives (1, 0).
  V = (-U.y, U.x).
* Extents.  The four corners projected on U and V: x0 / x1 = min / max along U, y0 / y1 = min / max along V,
  yc = 0.25 * ((p0 + p1) + (p2 + p3)) of the V projections.
* ov(a, b): min(x1a, x1b) > max(x0a, x0b).
* before(a, b), a != b.  (1) If ov(a, b): yc_a < yc_b, or yc_a == yc_b and a < b.  (2) Otherwise, if x1a <= x0b: true unless a blocker c
  exists, a line c not in {a, b} with min(yc_a, yc_b) < yc_c < max(yc_a, yc_b), ov(c, a) and ov(c, b).  (3) Otherwise false.
* Order.  Repeatedly emit the smallest-index line that is not emitted and has no unemitted line before it; if there is none (a cycle), the
  smallest-index unemitted line (a forced emission).
* Blocks.  Position k starts a new block unless, for p at k - 1 and q at k, rule 1 gives before(p, q) and
  y0_q - y1_p <= block_gap * max(sht_p, sht_q).  The first position of a page starts a block.
"""
from __future__ import annotations

import numpy as np

from tests import lines_ref as LR

BLOCK_GAP = 1.0


# ------------------------------------------------------------------ the rule -------------------------------------------------------------
def page_axis(f: dict, lo: int, hi: int, T):
    """U of the lines lo:hi: the direction sum in line order"""
    sx, sy = T(0), T(0)
    for l in range(lo, hi):
        sx, sy = sx + f["lng"][l] * f["ux"][l], sy + f["lng"][l] * f["uy"][l]
    norm = np.sqrt(sx * sx + sy * sy)
    return (sx / norm, sy / norm) if norm > 0 else (T(1), T(0))


def extents(quads, offs=None, dtype=np.float32) -> dict:
    """x0, x1, y0, y1, yc, sht (L,) in ``dtype`` and the page axes (B,2)"""
    T = dtype
    q32 = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    L = len(q32)
    offs = [0, L] if offs is None else [int(o) for o in offs]
    f = LR.word_frames(q32, T)
    q = q32.astype(T)
    e = {k: np.zeros(L, dtype=T) for k in ("x0", "x1", "y0", "y1", "yc")}
    axes = np.zeros((len(offs) - 1, 2), dtype=T)
    for p, (lo, hi) in enumerate(zip(offs, offs[1:])):
        ux, uy = page_axis(f, lo, hi, T)
        vx, vy = -uy, ux
        axes[p] = ux, uy
        x, y = q[lo:hi, :, 0], q[lo:hi, :, 1]
        pu, pv = x * ux + y * uy, x * vx + y * vy
        e["x0"][lo:hi], e["x1"][lo:hi], e["y0"][lo:hi], e["y1"][lo:hi] = pu.min(1), pu.max(1), pv.min(1), pv.max(1)
        e["yc"][lo:hi] = T(0.25) * ((pv[:, 0] + pv[:, 1]) + (pv[:, 2] + pv[:, 3]))
    e["sht"], e["axes"], e["offs"] = f["sht"], axes, offs
    return e


def ov(e: dict, a, b):
    return np.minimum(e["x1"][a], e["x1"][b]) > np.maximum(e["x0"][a], e["x0"][b])


def rule1(e: dict, a: int, b: int) -> bool:
    return bool(ov(e, a, b)) and bool(e["yc"][a] < e["yc"][b] or (e["yc"][a] == e["yc"][b] and a < b))


def relation(e: dict) -> np.ndarray:
    """before (L,L) bool, row a, column b.  One row at a time over all b.  The blockers of row a are looked for among the lines c with
    ov(c, a) and x1c > x1a only: ov(c, b) with a left of b needs x1c > x0b >= x1a, comparisons of the same stored numbers, so no other c can
    block and the result is the plain rule's."""
    L = len(e["yc"])
    x0, x1, yc = e["x0"], e["x1"], e["yc"]
    before = np.zeros((L, L), dtype=bool)
    for lo, hi in zip(e["offs"], e["offs"][1:]):
        idx = np.arange(lo, hi)
        for a in range(lo, hi):
            ovab = ov(e, a, idx)
            first = ovab & ((yc[a] < yc[idx]) | ((yc[a] == yc[idx]) & (a < idx)))
            left = ~ovab & (x1[a] <= x0[idx])
            ylo, yhi = np.minimum(yc[a], yc[idx]), np.maximum(yc[a], yc[idx])
            blocked = np.zeros(hi - lo, dtype=bool)
            for c in idx[ovab & (x1[idx] > x1[a]) & (idx != a)]:
                blocked |= (idx != c) & (ylo < yc[c]) & (yc[c] < yhi) & ov(e, c, idx)
            before[a, lo:hi] = first | (left & ~blocked)
            before[a, a] = False
    return before


def peel(before: np.ndarray, offs) -> tuple[np.ndarray, int]:
    """(line_order (L,), number of forced emissions) from any relation matrix.  deg[j] counts the unemitted lines before line j."""
    L = before.shape[0]
    order, forced = np.full(L, -1), 0
    for lo, hi in zip(offs, offs[1:]):
        left = np.ones(hi - lo, dtype=bool)
        sub = before[lo:hi, lo:hi].astype(np.int64)
        deg = sub.sum(0)
        for k in range(lo, hi):
            free = left & (deg == 0)
            if not free.any():
                free, forced = left, forced + 1
            i = int(np.argmax(free))
            order[k], left[i] = lo + i, False
            deg -= sub[i]
    return order, forced


def block_flags(e: dict, order, block_gap=BLOCK_GAP, dtype=np.float32) -> np.ndarray:
    T = dtype
    flags = np.ones(len(order), dtype=np.int32)
    for lo, hi in zip(e["offs"], e["offs"][1:]):
        for k in range(lo + 1, hi):
            p, q = int(order[k - 1]), int(order[k])
            near = e["y0"][q] - e["y1"][p] <= T(block_gap) * max(e["sht"][p], e["sht"][q])
            flags[k] = 0 if (rule1(e, p, q) and near) else 1
    return flags


def reading_order(quads, offs=None, block_gap=BLOCK_GAP, dtype=np.float32) -> dict:
    """line_order (L,), new_block (L,), before (L,L) bool, forced, ext"""
    e = extents(quads, offs, dtype)
    before = relation(e)
    order, forced = peel(before, e["offs"])
    return {"line_order": order, "new_block": block_flags(e, order, block_gap, dtype), "before": before, "forced": forced, "ext": e}


def pack_bits(before: np.ndarray, cap: int | None = None) -> np.ndarray:
    """the kernel's layout: (cap, ceil(cap / 32)) uint32, bit (b & 31) of word [a][b >> 5]"""
    L = before.shape[0]
    cap = L if cap is None else cap
    out = np.zeros((cap, (cap + 31) // 32), dtype=np.uint32)
    a, b = np.nonzero(before)
    np.bitwise_or.at(out, (a, b >> 5), (np.uint32(1) << (b & 31).astype(np.uint32)))
    return out


def blocks_of(order, flags, offs=None) -> list:
    """the block number of every position, counted from 0 per page"""
    offs = [0, len(order)] if offs is None else list(offs)
    out = []
    for lo, hi in zip(offs, offs[1:]):
        n = -1
        for k in range(lo, hi):
            n += int(flags[k] != 0 or k == lo)
            out.append(n)
    return out


def decision_margin(quads, offs=None, block_gap=BLOCK_GAP) -> float:
    """How far (in pixels, float64) the input keeps every comparison of the rule from its threshold: for every pair of lines of a page the
    overlap min(x1) - max(x0) from 0 (for a pair without overlap that is also the left-of test x1a <= x0b) and yc_a from yc_b (rule 1 and
    the two tests of every blocker); for every two neighbours of the order that rule 1 joins, the gap from block_gap * the taller height.
    Lines with equal yc (the index tie-break) give 0."""
    r = reading_order(quads, offs, block_gap, np.float64)
    e, worst = r["ext"], np.inf
    for lo, hi in zip(e["offs"], e["offs"][1:]):
        for a in range(lo, hi):
            for b in range(a + 1, hi):
                worst = min(worst, abs(min(e["x1"][a], e["x1"][b]) - max(e["x0"][a], e["x0"][b])), abs(e["yc"][a] - e["yc"][b]))
        for k in range(lo + 1, hi):
            p, q = int(r["line_order"][k - 1]), int(r["line_order"][k])
            if rule1(e, p, q):
                worst = min(worst, abs(block_gap * max(e["sht"][p], e["sht"][q]) - (e["y0"][q] - e["y1"][p])))
    return float(worst)


# ------------------------------------------------------------------ cases ----------------------------------------------------------------
def xyxy(x0, y0, x1, y1) -> np.ndarray:
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float32)


def sort_lines(quads, names=None):
    """the order ``find_lines`` gives lines: by (centre y, centre x)"""
    c = quads.mean(1)
    idx = sorted(range(len(quads)), key=lambda i: (c[i, 1], c[i, 0], i))
    return quads[idx], (None if names is None else [names[i] for i in idx])


def two_column_boxes():
    """the named boxes of the two-column page, in the order they are read"""
    named = [("H1", (0, 0, 400, 20))]
    named += [(f"A{k}", (0, 44 + 30 * k, 180, 64 + 30 * k)) for k in range(4)]
    named += [(f"B{k}", (220, 40 + 30 * k, 400, 60 + 30 * k)) for k in range(5)]
    named += [("H2", (0, 200, 400, 220))]
    named += [(f"C{k}", (0, 244 + 30 * k, 180, 264 + 30 * k)) for k in range(3)]
    named += [(f"D{k}", (220, 240 + 30 * k, 400, 260 + 30 * k)) for k in range(3)]
    return named


def case_two_columns():
    """(quads sorted by (centre y, centre x), their names, the names in reading order)"""
    named = two_column_boxes()
    quads, names = sort_lines(np.stack([xyxy(*b) for _, b in named]), [n for n, _ in named])
    return quads, names, [n for n, _ in named]


def case_three_columns():
    """columns at x = 0 / 200 / 400 with 5 / 3 / 6 lines 160 wide and 14 high at a pitch of 24, column c 10 * c lower, the last line of each
    column 70 wide"""
    named = []
    for c, (x, n) in enumerate(((0, 5), (200, 3), (400, 6))):
        for k in range(n):
            y = 10 * c + 24 * k
            named.append((f"{'PQR'[c]}{k}", (x, y, x + (70 if k == n - 1 else 160), y + 14)))
    quads, names = sort_lines(np.stack([xyxy(*b) for _, b in named]), [n for n, _ in named])
    return quads, names, [n for n, _ in named]


CYCLE = [(112, 168, 8), (104, 120, 12), (0, 64, 32), (56, 72, 68), (152, 192, 120), (96, 160, 144), (40, 104, 156), (80, 96, 232)]
CYCLE_ORDER = [2, 3, 0, 1, 4, 5, 6, 7]


def case_cycle():
    return np.stack([xyxy(x0, yc - 2, x1, yc + 2) for x0, x1, yc in CYCLE])


def columns_case(n, cols, w=40, h=10, col_pitch=60, row_pitch=16, step=3, headers=()):
    """n one-word lines in ``cols`` columns, column c ``step * c`` lower, plus one line across all columns in the row gap above each row of
    ``headers`` (they are what blocks rule 2 between the columns); sorted as find_lines sorts; all corners integers below 4096"""
    per = -(-n // cols)
    boxes = [xyxy(col_pitch * (i // per), step * (i // per) + row_pitch * (i % per), col_pitch * (i // per) + w, step * (i // per) + row_pitch * (i % per) + h)
             for i in range(n)]
    boxes += [xyxy(0, row_pitch * r - 2, col_pitch * (cols - 1) + w, row_pitch * r - 1) for r in headers]
    q, _ = sort_lines(np.stack(boxes))
    assert q.min() >= 0 and q.max() < 4096
    return q

"""Host restatement of the detection datasets' items (ocrs_models/datasets/hiertext.py:22-130, ddi100.py:34-107, datasets/util.py:54-110)
up to the transform: ``shrink_polygon`` is the project's shrink rule in float64, operation by operation, in the order csrc/page_data.hip
mirrors; ``page_mask`` is ``generate_mask`` with it, PIL doing the fill (and the conversion of the float vertices); ``write_hiertext_tree``
and ``write_ddi_tree`` build small dataset directories with PIL and pickle."""
from __future__ import annotations

import gzip
import json
import math
import os
import pickle
import random

import numpy as np
from PIL import Image, ImageDraw

MITRE_LIMIT_DEN = (25.0, 2.0)  # a mitre longer than 5 dist: sqrt(2 / (1 + cos)) > 5  <=>  (1 + cos) * 25 < 2
MAX_COORD = 1048576.0


def dedupe(poly) -> list:
    w = []
    for x, y in poly:
        x, y = int(x), int(y)
        if w and w[-1] == (x, y):
            continue
        w.append((x, y))
    while len(w) > 1 and w[-1] == w[0]:
        w.pop()
    return w


def _normal(w, s: int, i: int):
    """Edge i's integer direction and its unit normal pointing into the polygon, s * (-dy, dx) / len; exact for an axis-aligned edge."""
    (x0, y0), (x1, y1) = w[i], w[(i + 1) % len(w)]
    dx, dy = x1 - x0, y1 - y0
    if dx == 0:
        return dx, dy, float(-s if dy > 0 else s), 0.0
    if dy == 0:
        return dx, dy, 0.0, float(s if dx > 0 else -s)
    length = math.sqrt(float(dx * dx + dy * dy))
    return dx, dy, float(-s * dy) / length, float(s * dx) / length


def _corner(w, s: int, dist: float, i: int):
    """The output points of vertex i: None (anti-parallel edges), one mitre point or two bevel points."""
    dx0, dy0, n0x, n0y = _normal(w, s, (i - 1) % len(w))
    dx1, dy1, n1x, n1y = _normal(w, s, i)
    vx, vy = float(w[i][0]), float(w[i][1])
    cr = dx0 * dy1 - dy0 * dx1
    if cr == 0:
        if dx0 * dx1 + dy0 * dy1 <= 0:
            return None
        return [(vx + dist * n1x, vy + dist * n1y)]
    c = n0x * n1x + n0y * n1y
    den = 1.0 + c
    if s * cr < 0 and den * MITRE_LIMIT_DEN[0] < MITRE_LIMIT_DEN[1]:
        return [(vx + dist * n0x, vy + dist * n0y), (vx + dist * n1x, vy + dist * n1y)]
    if dx0 == 0 or dx1 == 0:  # a vertical edge fixes x exactly; the other edge's line gives y
        (ax, _), (ox, oy) = ((n0x, n0y), (n1x, n1y)) if dx0 == 0 else ((n1x, n1y), (n0x, n0y))
        tx = dist * ax
        return [(vx + tx, vy + (dist - ox * tx) / oy)]
    if dy0 == 0 or dy1 == 0:  # a horizontal edge fixes y exactly
        (_, ay), (ox, oy) = ((n0x, n0y), (n1x, n1y)) if dy0 == 0 else ((n1x, n1y), (n0x, n0y))
        ty = dist * ay
        return [(vx + (dist - oy * ty) / ox, vy + ty)]
    mm = dist / den
    return [(vx + mm * (n0x + n1x), vy + mm * (n0y + n1y))]


def shrink_polygon(poly, dist: float) -> list:
    """The shrunk ring as float (x, y) tuples, [] when the polygon is skipped (DESIGN.md section 13 has the rule in words)."""
    if dist == 0.0:
        return [(float(x), float(y)) for x, y in poly]
    w = dedupe(poly)
    m = len(w)
    area2 = sum(w[i][0] * w[(i + 1) % m][1] - w[(i + 1) % m][0] * w[i][1] for i in range(m))
    if m < 3 or area2 == 0:
        return []
    s = 1 if area2 > 0 else -1
    out, first = [], []
    for i in range(m):
        pts = _corner(w, s, dist, i)
        if pts is None:
            return []
        first.append(len(out))
        out += pts
    for i in range(m):
        j = (i + 1) % m
        ax, ay = out[(first[j] if j else len(out)) - 1]
        bx, by = out[first[j]]
        dot = (bx - ax) * float(w[j][0] - w[i][0]) + (by - ay) * float(w[j][1] - w[i][1])
        if not dot > 0.0:
            return []
    acc = 0.0
    for k in range(len(out)):
        j = (k + 1) % len(out)
        acc += out[k][0] * out[j][1] - out[j][0] * out[k][1]
        if not abs(out[k][0]) <= MAX_COORD or not abs(out[k][1]) <= MAX_COORD:
            return []
    if not acc * float(s) > 0.0:
        return []
    return out


def page_mask(w: int, h: int, polys, dist: float = 3.0) -> np.ndarray:
    """generate_mask(w, h, polys, dist) of datasets/util.py:78-110 as a (h, w) uint8 0/1 array: PIL is given the float vertices."""
    im = Image.new("1", (w, h), 0)
    draw = ImageDraw.Draw(im)
    for poly in polys:
        shrunk = shrink_polygon(poly, dist) if dist != 0.0 else [tuple(p) for p in poly]
        if not shrunk:
            continue
        draw.polygon(shrunk, fill="white", outline=None)
    return np.array(im, dtype=np.uint8)


# ---- polygon families ------------------------------------------------------------------------------------------------------------
def ring(n: int, cx: float, cy: float, rx: float, ry: float):
    """n distinct integer vertices around an ellipse."""
    pts = []
    for k in range(n):
        a = 2 * math.pi * k / n
        p = (int(round(cx + rx * math.cos(a))), int(round(cy + ry * math.sin(a))))
        if not pts or (p != pts[-1] and p != pts[0]):
            pts.append(p)
    return pts


def shrink_cases() -> list:
    """[(name, polygon)]: the families the device shrink is held to."""
    r = random.Random(31)
    rect = [(10, 10), (40, 10), (40, 30), (10, 30)]
    ell = [(0, 0), (60, 0), (60, 20), (20, 20), (20, 50), (0, 50)]
    needle = [(0, 0), (100, 0), (100, 60), (52, 60), (50, 8), (48, 60), (0, 60)]  # a reflex vertex past the mitre limit
    blunt = [(0, 0), (100, 0), (100, 60), (70, 60), (50, 40), (30, 60), (0, 60)]  # a reflex vertex below it
    cases = [("rect", rect), ("rect-rev", rect[::-1]), ("rect-closed", rect + [rect[0]]), ("rect-dups", [rect[0], rect[0], rect[1], rect[2], rect[2], rect[3]]),
             ("thin", [(0, 0), (50, 0), (50, 6), (0, 6)]), ("thinner", [(0, 0), (50, 0), (50, 4), (0, 4)]), ("just", [(0, 0), (50, 0), (50, 7), (0, 7)]),
             ("diamond", [(50, 20), (80, 50), (50, 80), (20, 50)]), ("ell", ell), ("ell-rev", ell[::-1]), ("needle", needle),
             ("needle-rev", needle[::-1]), ("blunt", blunt), ("blunt-rev", blunt[::-1]), ("zero-area", [(0, 0), (10, 10), (20, 20)]),
             ("spike", [(0, 0), (40, 0), (40, 20), (20, 20), (20, 40), (20, 20), (0, 20)]),  # anti-parallel neighbours
             ("two", [(0, 0), (9, 9)]), ("collinear", [(0, 0), (20, 0), (40, 0), (40, 30), (0, 30)]),
             ("sheared", [(10, 10), (70, 14), (78, 40), (18, 36)]), ("rotated", [(30, 5), (90, 35), (80, 55), (20, 25)]),
             ("sliver", [(0, 0), (100, 3), (100, 5)]), ("outside", [(-30, -20), (25, -18), (24, 12), (-31, 10)]),
             ("ring512", ring(512, 4000, 3000, 3900, 2900))]
    for k in range(200):  # random convex quads: a jittered rectangle
        x0, y0, bw, bh = r.randint(-20, 150), r.randint(-20, 110), r.randint(4, 70), r.randint(4, 40)
        q = [(x0 + r.randint(-2, 2), y0 + r.randint(-2, 2)), (x0 + bw + r.randint(-2, 2), y0 + r.randint(-2, 2)),
             (x0 + bw + r.randint(-2, 2), y0 + bh + r.randint(-2, 2)), (x0 + r.randint(-2, 2), y0 + bh + r.randint(-2, 2))]
        cases.append((f"quad{k}", q if k % 2 else q[::-1]))
    return cases


def grid_words(w: int, h: int, n: int, seed: int) -> list:
    """n word-like quads on a (w, h) page, some sticking out of it."""
    r = random.Random(seed)
    out = []
    for _ in range(n):
        bw, bh = r.randint(8, max(9, w // 4)), r.randint(7, max(8, h // 5))
        x0, y0 = r.randint(-6, w - 2), r.randint(-6, h - 2)
        out.append([(x0 + r.randint(-1, 1), y0 + r.randint(-1, 1)), (x0 + bw, y0 + r.randint(-1, 1)), (x0 + bw + r.randint(-1, 1), y0 + bh),
                    (x0, y0 + bh + r.randint(-1, 1))])
    return out


def dense_words() -> list:
    """153 polygons that all touch rows 16 .. 31 of a (200, 64) page, so that band's slice of the store takes three 64-lane passes: four
    tiers of 38 narrow quads (2 px wide once shrunk, 5 px apart, every other tier moved by 2 px so that overlapping tiers stay apart) whose
    row ranges are staggered, and a 24-vertex ring whose first row sorts it behind the first two tiers, into the second pass, among quads."""
    tiers = [(2, 24), (12, 36), (22, 46), (27, 52)]
    out = [[(x, y0 + (k + t) % 2), (x + 7, y0 + (k % 3) % 2), (x + 7, y1 - (k + t) % 2), (x, y1)] for t, (y0, y1) in enumerate(tiers)
           for k, x in enumerate(range(2 + 2 * (t % 2), 192, 5))]
    assert len(out) == 152
    return out[:76] + [ring(24, 100, 30, 60, 10)] + out[76:]


def mask_pages() -> list:
    """[(name, (w, h), polygons)] of the page-mask test: pages of different sizes for one batch."""
    many =[[(x, y), (x + 11, y), (x + 11, y + 8), (x, y + 8)] for y in range(2, 140, 10) for x in range(3, 190, 14)][:150]
    assert len(many) == 150
    return [("empty", (40, 30), []),
            ("one", (57, 33), [[(5, 4), (50, 6), (51, 28), (4, 26)]]),
            ("overlap", (90, 70), [[(5, 5), (60, 5), (60, 40), (5, 40)], [(30, 20), (85, 22), (84, 65), (29, 60)], [(10, 30), (50, 30), (50, 60), (10, 60)]]),
            ("shared-rows", (160, 48), [[(x, 6 + (x % 3)), (x + 20, 7), (x + 21, 40), (x, 39)] for x in range(2, 150, 24)]),
            ("outside", (64, 48), [[(-20, -10), (30, -8), (31, 20), (-19, 18)], [(40, 30), (90, 31), (91, 70), (41, 69)], [(-50, -50), (-10, -50), (-10, -10), (-50, -10)],
                                   [(70, 5), (120, 5), (120, 30), (70, 30)], [(-10, 20), (80, 22), (79, 36), (-11, 34)]]),
            ("all-skipped", (50, 40), [[(5, 5), (45, 5), (45, 10), (5, 10)], [(0, 0), (10, 10), (20, 20)], [(3, 3), (9, 9)]]),
            ("many", (200, 150), many),
            ("concave", (120, 90), [[(5, 5), (110, 5), (110, 80), (62, 80), (60, 20), (58, 80), (5, 80)], ring(40, 60, 45, 30, 22)]),
            ("words", (131, 77), grid_words(131, 77, 40, 7)),
            ("dense", (200, 64), dense_words())]


def page_pixels(w: int, h: int, seed: int) -> np.ndarray:
    r = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    return (96 + 64 * np.sin(x / 5.0) * np.cos(y / 7.0) + r.randint(0, 60, (h, w))).clip(0, 255).astype(np.uint8)


# ---- dataset trees ---------------------------------------------------------------------------------------------------------------
HIERTEXT_PAGES = {"page_a": (97, 61), "page_b": (160, 120), "page_c": (40, 33), "page_d": (120, 90), "page_e": (64, 48)}  # image_id -> (w, h)


def hiertext_annotations() -> list:
    """One annotation per page: paragraphs -> lines -> words, with vertices; the word order is the test's subject."""
    anns = []
    for k, (name, (w, h)) in enumerate(HIERTEXT_PAGES.items()):
        words = grid_words(w, h, 5 + 2 * k, 40 + k)
        word = lambda q, t: {"vertices": [list(v) for v in q], "text": t, "legible": True, "handwritten": False, "vertical": False}  # noqa: E731
        lines = [{"vertices": [list(v) for v in words[i]], "text": f"l{i}", "legible": True, "vertical": False, "handwritten": False,
                  "words": [word(q, f"w{i}") for q in words[i:i + 2]]} for i in range(0, len(words), 2)]
        anns.append({"image_id": name, "image_width": w, "image_height": h, "paragraphs": [{"vertices": [], "legible": True, "lines": lines[:1]},
                                                                                         {"vertices": [], "legible": True, "lines": lines[1:]}]})
    return anns


def annotation_words(ann: dict) -> list:
    return [[tuple(v) for v in word["vertices"]] for para in ann["paragraphs"] for line in para["lines"] for word in line["words"]]


def write_hiertext_tree(root, split: str = "train", seed: int = 1) -> list:
    """gt/{split}.jsonl.gz + {split}/*.jpg (quality 95).  Returns [(image_id, word polygons)] in file order."""
    os.makedirs(os.path.join(root, "gt"), exist_ok=True)
    os.makedirs(os.path.join(root, split), exist_ok=True)
    for k, (name, (w, h)) in enumerate(HIERTEXT_PAGES.items()):
        px = page_pixels(w, h, seed + k)
        Image.fromarray(np.stack([px, 255 - px, px // 2], axis=-1), "RGB").save(os.path.join(root, split, name + ".jpg"), quality=95)
    anns = hiertext_annotations()
    with gzip.open(os.path.join(root, "gt", split + ".jsonl.gz"), "wt") as f:
        json.dump({"annotations": anns}, f)
    return [(a["image_id"], annotation_words(a)) for a in anns]


DDI_PAGES = [(f"{k:03d}.png", (50 + 9 * k, 40 + 5 * k)) for k in range(20)]  # file -> (w, h)


def write_ddi_tree(root, seed: int = 3) -> list:
    """gen_imgs/*.png (grey) + gen_boxes/*.pickle (a list of {"box": (4, 2) int array, "text"}).  Returns [(file, word quads)] sorted."""
    os.makedirs(os.path.join(root, "gen_imgs"), exist_ok=True)
    os.makedirs(os.path.join(root, "gen_boxes"), exist_ok=True)
    out = []
    for k, (name, (w, h)) in enumerate(DDI_PAGES):
        Image.fromarray(page_pixels(w, h, seed + k), "L").save(os.path.join(root, "gen_imgs", name))
        quads = grid_words(w, h, 3 + k % 4, 70 + k)
        with open(os.path.join(root, "gen_boxes", os.path.splitext(name)[0] + ".pickle"), "wb") as f:
            pickle.dump([{"box": np.array(q, dtype=np.int64), "text": f"w{i}"} for i, q in enumerate(quads)], f)
        out.append((name, quads))
    return out


def read_gray(path: str) -> np.ndarray:
    with Image.open(path) as im:
        if im.format == "JPEG":
            im.draft("L", im.size)
        return np.array(im.convert("L"), dtype=np.uint8)

"""Host restatement of the reference's HierTextRecognition item (ocrs_models/datasets/hiertext.py:238-274) up to the un-resized masked crop:
PIL for the mask, torch CPU for the rest.  ``polygon_mask`` restates PIL's polygon fill itself (the helper csrc/line_data.hip was ported
from; tests/test_hiertext_host.py pins it to the installed PIL), ``polygon_cases`` are the polygon families both tests use, and
``write_tree`` builds a small HierText directory with PIL."""
from __future__ import annotations

import gzip
import json
import math
import os
import random

import numpy as np
import torch
from PIL import Image, ImageDraw

f32 = np.float32


def pil_mask(w: int, h: int, poly) -> np.ndarray:
    """generate_mask(w, h, [poly], shrink_dist=0.0) of datasets/util.py:78-110 as a (h, w) uint8 0/1 array."""
    im = Image.new("1", (w, h), 0)
    ImageDraw.Draw(im).polygon([tuple(p) for p in poly], fill="white", outline=None)
    return np.array(im, dtype=np.uint8)


def _round_up(f) -> int:
    f = f32(f)
    return int(math.floor(f + f32(0.5))) if f >= 0 else -int(math.floor(abs(f) + f32(0.5)))


def _round_down(f) -> int:
    f = f32(f)
    return int(math.ceil(f - f32(0.5))) if f >= 0 else -int(math.ceil(abs(f) - f32(0.5)))


def polygon_mask(w: int, h: int, poly) -> np.ndarray:
    """PIL's ImageDraw.polygon(poly, fill, outline=None) on a mode "1" image, rule by rule, in fp32 as PIL computes it:
    horizontal edges are their own hline; on each row every other edge crossing it gives x = (y - y0) * dx + x0, twice where the edge ends on
    an inner row; where two edges leaning the same way share a vertex, the row is extended to the pixel beside the next row's span;
    the sorted crossings are filled in pairs from ROUND_UP to ROUND_DOWN, each span starting after the previous one."""
    v = [(int(x), int(y)) for x, y in poly]
    out = np.zeros((h, w), np.uint8)

    def hline(x0, y, x1):
        if 0 <= y < h and x0 < w and x1 >= 0:
            out[y, max(x0, 0):min(x1, w - 1) + 1] = 1

    edges = [(v[i], v[i + 1]) for i in range(len(v) - 1)] + ([(v[-1], v[0])] if v[-1] != v[0] else [])
    ymin, ymax, tab = h - 1, 0, []
    for (x0, y0), (x1, y1) in edges:
        ymin, ymax = min(ymin, y0, y1), max(ymax, y0, y1)
        if y0 == y1:
            hline(min(x0, x1), y0, max(x0, x1))
        else:
            tab.append((x0, y0, min(y0, y1), max(y0, y1), f32(x1 - x0) / f32(y1 - y0), x1, y1))
    ymin, ymax = max(ymin, 0), min(ymax, h)

    def at(e, y):
        return f32(f32(y - e[1]) * e[4]) + f32(e[0])

    def vertex_x(e, y):
        """the integer x of the edge's vertex on row y, None where the edge only passes through the row"""
        return e[0] if y == e[1] else (e[5] if y == e[6] else None)

    for y in range(ymin, ymax + 1):
        xx = []
        for i, cur in enumerate(tab):
            if not cur[2] <= y <= cur[3]:
                continue
            xx.append(at(cur, y))
            if y == cur[3] and y < ymax:
                xx.append(xx[-1])
            elif cur[4] != 0 and vertex_x(cur, y) is not None:
                # a corner is two edges that share a VERTEX (their fp32 crossings need not agree: the far end of an edge is rounded)
                cx = vertex_x(cur, y)
                for oth in tab[:i]:
                    if (cur[4] > 0) != (oth[4] > 0) or oth[4] == 0:
                        continue
                    if not ((y == cur[2] and y == oth[2]) or (y == cur[3] and y == oth[3])) or vertex_x(oth, y) != cx:
                        continue
                    off = -1 if y == ymax else 1
                    a, b = at(cur, y + off), at(oth, y + off)
                    if (cur[4] > 0) == (off == 1):
                        xx[-1] = f32(max(cx, _round_up(min(a, b)) - 1))
                    else:
                        xx[-1] = f32(min(cx, _round_up(f32(max(a, b) + f32(1)))))
                    break
        xx.sort()
        x_pos = int(xx[0]) if xx else 0
        for i in range(1, len(xx), 2):
            x_end = _round_down(xx[i])
            if x_end < x_pos:
                continue
            x_start = max(_round_up(xx[i - 1]), x_pos)
            if x_end < x_start:
                continue
            hline(x_start, y, x_end)
            x_pos = x_end + 1
    return out


# ---- polygon families ---------------------------------------------------------------------------------------------------------
CANVASES = [(1, 1), (1, 40), (40, 1), (67, 13), (300, 41), (801, 23), (24, 10), (130, 64)]  # (w, h)


def _band(r: random.Random, w: int, h: int, n: int, out: int, concave: bool):
    """x-monotone band: a top chain left to right, a bottom chain right to left."""
    k = n // 2
    xs = sorted(r.randint(-out, w + out) for _ in range(k))
    xs2 = sorted((r.randint(-out, w + out) for _ in range(n - k)), reverse=True)
    if concave:
        top = [(x, r.randint(-out, max(-out, h // 2))) for x in xs]
        bot = [(x, r.randint(h // 2, h + out)) for x in xs2]
        # the two chains may touch but not share a vertex: a polygon that passes twice through one vertex is not simple
        bot = [q for q in bot if q not in top] or [(xs2[0], h + out)]
    else:  # convex: the chains bend one way only (a parabola-like top and bottom)
        mid = (h - 1) / 2
        top = [(x, int(round(mid * ((2 * (x / max(w, 1)) - 1) ** 2)))) for x in xs]
        bot = [(x, h - int(round(mid * ((2 * (x / max(w, 1)) - 1) ** 2)))) for x in xs2]
    return top + bot


def _quad(r: random.Random, w: int, h: int, out: int):
    pts = [(0, 0), (w, 0), (w, h), (0, h)]
    return [(min(max(x + r.randint(-3, 3), -out), w + out), min(max(y + r.randint(-3, 3), -out), h + out)) for x, y in pts]


def _rect(r: random.Random, w: int, h: int, out: int):
    x0, x1 = sorted((r.randint(-out, w + out), r.randint(-out, w + out)))
    y0, y1 = sorted((r.randint(-out, h + out), r.randint(-out, h + out)))
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


SEEDS = (20, 21, 22, 23)


def all_polygon_cases():
    return [c for seed in SEEDS for c in polygon_cases(seed)]


def polygon_cases(seed: int = 20, per_family: int = 24):
    """[(family, w, h, polygon)]: fixed seeds, no self-intersecting polygons."""
    r = random.Random(seed)
    cases = []
    for k in range(per_family):
        w, h = CANVASES[k % len(CANVASES)]
        for out in (0, 3):
            tag = "+out" if out else ""
            cases.append(("rect" + tag, w, h, _rect(r, w, h, out)))
            cases.append(("quad" + tag, w, h, _quad(r, w, h, out)))
            cases.append(("band-concave" + tag, w, h, _band(r, w, h, r.randint(4, 16), out, True)))
            cases.append(("band-convex" + tag, w, h, _band(r, w, h, r.randint(4, 16), out, False)))
        # the reference's own geometry: the canvas is the polygon's bounding box, so the largest coordinate equals the canvas size
        p = _band(r, w + 8, h + 8, r.randint(4, 12), 0, True)
        mx, my = min(x for x, _ in p), min(y for _, y in p)
        p = [(x - mx, y - my) for x, y in p]
        bw, bh = max(x for x, _ in p), max(y for _, y in p)
        if bw > 0 and bh > 0:
            cases.append(("bbox", bw, bh, p))
        for _ in range(4):  # more of it, on canvases of their own: these are the shapes HierText lines have
            cw, ch = r.randint(12, 400), r.randint(10, 64)
            p = _band(r, cw, ch, r.randint(4, 14), 0, True)
            mx, my = min(x for x, _ in p), min(y for _, y in p)
            p = [(x - mx, y - my) for x, y in p]
            bw, bh = max(x for x, _ in p), max(y for _, y in p)
            if bw > 0 and bh > 0:
                cases.append(("bbox", bw, bh, p))
        q = _quad(r, w, h, 3)
        cases.append(("repeated", w, h, [q[0], q[0], q[1], q[2], q[2], q[2], q[3]]))
        cases.append(("closed", w, h, q + [q[0]]))
        cases.append(("flat-top-bottom", w, h, [(0, 0), (w // 3, 0), (w, 0), (w - r.randint(0, 3), h), (w // 2, h), (r.randint(0, 3), h)]))
        cases.append(("two-points", w, h, [(r.randint(0, w), r.randint(0, h)), (r.randint(0, w), r.randint(0, h))]))
    return cases


# ---- the reference's item --------------------------------------------------------------------------------------------------------
def line_box(vertices):
    """hiertext.py:248-253"""
    xs, ys = [v[0] for v in vertices], [v[1] for v in vertices]
    min_x = max(0, min(xs))
    max_x = max(min_x, max(xs))
    min_y = max(0, min(ys))
    max_y = max(min_y, max(ys))
    return min_x, min_y, max_x, max_y


def read_gray(path: str) -> np.ndarray:
    with Image.open(path) as im:
        if im.format == "JPEG":
            im.draft("L", im.size)
        return np.array(im.convert("L"), dtype=np.uint8)


def line_crop(page: np.ndarray, box) -> np.ndarray:
    """hiertext.py:217-222: clamp to size - 1, exclusive slice"""
    ph, pw = page.shape
    min_x, min_y, max_x, max_y = box
    c = lambda v, hi: max(0, min(v, hi))  # noqa: E731
    return page[c(min_y, ph - 1):c(max_y, ph - 1), c(min_x, pw - 1):c(max_x, pw - 1)]


def item(page: np.ndarray, vertices):
    """(crop uint8 (1, h, w), mask uint8 (1, h, w), masked crop fp32 (1, h, w)) of hiertext.py:256-274 (the PNG cache is lossless)."""
    box = line_box(vertices)
    crop = torch.from_numpy(np.ascontiguousarray(line_crop(page, box)))[None]
    _, h, w = crop.shape
    mask = torch.from_numpy(pil_mask(w, h, [(x - box[0], y - box[1]) for x, y in vertices]))[None]
    img = crop.float() / 255.0 - 0.5
    m = mask.float()
    return crop, mask, torch.full(img.shape, -0.5) * (1.0 - m) + img * m


def _line(vertices, text, legible=True, vertical=False, handwritten=False, word_vertices=None):
    return {"vertices": [list(v) for v in vertices], "text": text, "legible": legible, "vertical": vertical, "handwritten": handwritten,
            "words": [{"vertices": [list(v) for v in (word_vertices or vertices)], "text": text}]}


PAGES = {"page_a": (97, 61), "page_b": (160, 120), "page_c": (33, 40)}  # image_id -> (width, height)


def tree_lines():
    """[(image_id, line dict, kept by the filter)] of the test tree, in file order."""
    return [
        ("page_a", _line([(5, 4), (60, 6), (61, 22), (4, 20)], "Hello"), True),
        ("page_a", _line([(10, 30), (96, 28), (97, 61), (9, 58)], "border box"), True),          # max on the page border: the clamp quirk
        ("page_a", _line([(40, 2), (50, 2), (50, 30), (40, 30)], "tall"), False),                 # aspect < 1
        ("page_b", _line([(12, 10), (80, 8), (150, 14), (149, 40), (78, 36), (11, 38)], "six point band"), True),
        ("page_b", _line([(-4, 50), (120, 48), (170, 56), (168, 90), (118, 80), (-3, 84)], "sticks out"), True),  # polygon outside the page
        ("page_b", _line([(20, 95), (140, 96), (139, 118), (21, 117)], "aa"), True),
        ("page_b", _line([(30, 60), (52, 60), (52, 72), (30, 72)], "this text is far too long for it"), True),  # infeasible for the CTC loss
        ("page_b", _line([(100, 100), (108, 100), (108, 108), (100, 108)], "tiny"), False),       # < 10 x 10
        ("page_c", _line([(2, 3), (30, 5), (31, 18), (1, 17)], "C1"), True),
        ("page_c", _line([(3, 20), (33, 21), (32, 39), (2, 38)], "c€~"), True),
        ("page_c", _line([(0, 0), (33, 0), (33, 12), (0, 12)], "Top"), True),
        ("page_c", _line([(4, 22), (30, 22), (30, 36), (4, 36)], "nope", legible=False), False),
    ]


def write_tree(root, split: str = "train", seed: int = 1, lines=None) -> list:
    """gt/{split}.jsonl.gz + {split}/*.jpg (quality 95).  Returns the kept (image_id, vertices, text) in file order."""
    r = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "gt"), exist_ok=True)
    os.makedirs(os.path.join(root, split), exist_ok=True)
    for name, (w, h) in PAGES.items():
        y, x = np.mgrid[0:h, 0:w]
        px = (96 + 64 * np.sin(x / 5.0) * np.cos(y / 7.0) + r.randint(0, 60, (h, w))).clip(0, 255).astype(np.uint8)
        Image.fromarray(np.stack([px, 255 - px, px // 2], axis=-1), "RGB").save(os.path.join(root, split, name + ".jpg"), quality=95)
    lines = tree_lines() if lines is None else lines
    anns = []
    for name in PAGES:
        mine = [ln for pid, ln, _ in lines if pid == name]
        anns.append({"image_id": name, "paragraphs": [{"lines": mine[:2]}, {"lines": mine[2:]}]})
    with gzip.open(os.path.join(root, "gt", split + ".jsonl.gz"), "wt") as f:
        json.dump({"annotations": anns}, f)
    return [(pid, [tuple(v) for v in ln["vertices"]], ln["text"]) for pid, ln, kept in lines if kept]

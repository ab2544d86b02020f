"""Which kernel the detection backward routes a shape to, and how much workspace it asks for (CPU: plain host arithmetic, no kernel runs).

The route and size queries -- ocrs_pw_bwd_kernel, ocrs_pw_bwd_ws_floats, ocrs_dw_bwd_ws_floats, ocrs_convt_bwd_ws_floats,
ocrs_convt_bwd_stats_supported, ocrs_convt_bwd_splittable -- decide what `models.py` launches and allocates.  They are pinned here, for both
dtypes, to the values the library returned BEFORE the detection sources were split by kernel family and the pointwise-backward route was stated
once (`pw_bwd_route`, csrc/det_bwd.hip): a refactor of that code must not move a single number.

Shapes: every DepthwiseConv block (Ca, Cb, Cout) and every ConvTranspose (Cup, Cout) of DetectionModel's layer table, at the resolution of its
level; every (Cin, Cout) pair of PW_BWD_COMBOS plus one pair outside it, (8, 32), which must stay unrouted (0).  Sizes: N = 2 at 64 x 64
(few tiles: the grids sit below their caps) and N = 32 at 1024 x 1024 (the caps bind).

tests/golden/det_routes.json is a list of [query, [arguments], value]; it was written by running this file as a script against the library of
the commit before the split (`cases()` below enumerates the calls, `__main__` prints them with the values the loaded library returns):

    python tests/test_det_routes_host.py > tests/golden/det_routes.json
"""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det_routes.json")
SIZES = ((2, 64, 64), (32, 1024, 1024))
PW_BWD_COMBOS = ((8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 128),
                 (128, 64), (64, 32), (32, 16), (16, 8))
OUTSIDE = (8, 32)


def model_shapes():
    """(level, Ca, Cb, Cout) of every DepthwiseConv block behind the first one, and (level of the input, Cup, Cout) of every ConvTranspose"""
    from ocrs_models_amd.models import DEPTH_SCALE as d

    blocks = [(0, d[0], 0, d[0])]  # in_conv's second block (the first, 1 -> 8, has its own kernels)
    convts = []
    for i in range(len(d) - 1):
        blocks += [(i + 1, d[i], 0, d[i + 1]), (i + 1, d[i + 1], 0, d[i + 1])]  # down[i]; its input is already pooled to level i + 1
        blocks += [(i, d[i], d[i], d[i]), (i, d[i], 0, d[i])]  # up[i].contract: cat(upsampled | cross), then the second block
        convts.append((i + 1, d[i + 1], d[i]))
    return blocks, convts


def cases():
    blocks, convts = model_shapes()
    out = []
    for N, H, W in SIZES:
        pw = [(lv, Ca, Cb, Co) for lv, Ca, Cb, Co in blocks] + [(0, ci, 0, co) for ci, co in PW_BWD_COMBOS + (OUTSIDE,)]
        for lv, Ca, Cb, Co in pw:
            h, w = max(H >> lv, 1), max(W >> lv, 1)
            for dt in (0, 1):
                out.append(("pw_bwd_kernel", (Ca, Cb, Co, dt)))
            out.append(("pw_bwd_ws_floats", (Ca + Cb, Co, N, h, w)))
            out.append(("dw_bwd_ws_floats", (Ca + Cb, N, h, w)))
        for lv, Cup, Co in convts:
            h, w = max(H >> lv, 1), max(W >> lv, 1)
            for dt in (0, 1):
                out.append(("convt_bwd_ws_floats", (Cup, Co, N, h, w, dt)))
                out.append(("convt_bwd_stats_supported", (Cup, Co, dt)))
                out.append(("convt_bwd_splittable", (Cup, Co, dt)))
    return sorted(set(out))


def _answers():
    from ocrs_models_amd._lib import lib

    L = lib()
    return [[q, list(a), int(getattr(L, q)(*a))] for q, a in cases()]


def test_golden_covers_every_case():
    golden = json.load(open(GOLDEN))
    assert [(q, tuple(a)) for q, a, _ in golden] == cases()


def test_routes_and_workspace_sizes_match_the_recorded_ones():
    golden = json.load(open(GOLDEN))
    got = _answers()
    wrong = [(g, r) for g, r in zip(got, golden) if g != r]
    assert not wrong, wrong[:10]
    routes = {tuple(a): v for q, a, v in golden if q == "pw_bwd_kernel"}
    assert routes[(OUTSIDE[0], 0, OUTSIDE[1], 0)] == 0 and routes[(OUTSIDE[0], 0, OUTSIDE[1], 1)] == 0  # outside PW_BWD_COMBOS: no kernel
    assert set(routes.values()) == {0, 1, 2, 3, 4}  # every route is exercised, the 32 | 32 concat (3) included


if __name__ == "__main__":
    print(json.dumps(_answers(), separators=(",", ":")).replace("],[", "],\n["))

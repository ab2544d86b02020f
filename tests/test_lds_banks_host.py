"""The bf16 LDS pixel pitch rule (csrc/common.h: lds_pitch_bf16) against the gfx950 bank model of tools/lds_banks.py: the MFMA fragment reads and
the transpose reads of every tile the detection net stages must cost their ideal number of LDS cycles."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lds_banks", os.path.join(ROOT, "tools", "lds_banks.py"))
lb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lb)


@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_padded_tiles_are_conflict_free(c):
    p = lb.lds_pitch(c)
    assert p == c + 16
    assert lb.fragment_read(p) == lb.IDEAL["fragment_read"] == 4
    assert lb.transpose_read(p) == lb.IDEAL["transpose_read"] == 2


@pytest.mark.parametrize("c", [8, 16])
def test_narrow_tiles_are_ideal_unpadded(c):
    p = lb.lds_pitch(c)
    assert p == c
    assert lb.fragment_read(p) == 4
    assert lb.transpose_read(p) == 2


@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_model_tells_the_pitches_apart(c):
    # the 16-byte pad (and a 48-byte one) costs every read twice its cycles under the real lane groups: the model is not vacuous
    for p in (c + 8, c + 24):
        assert lb.fragment_read(p) == 8
        assert lb.transpose_read(p) == 4


def test_lane_groups_cover_the_wave():
    for groups in (lb.B128_GROUPS, lb.TR_GROUPS, lb.W64_GROUPS):
        assert sorted(l for g in groups for l in g) == list(range(64))
    assert all(len(g) == 16 for g in lb.B128_GROUPS)


def test_rule_matches_common_h():
    src = open(os.path.join(ROOT, "ocrs_models_amd", "csrc", "common.h")).read()
    m = re.search(r"constexpr\s+int\s+lds_pitch_bf16\(int c\)\s*\{\s*return\s+c\s*<=\s*(\d+)\s*\?\s*c\s*:\s*c\s*\+\s*(\d+)\s*;\s*\}", src)
    assert m, "lds_pitch_bf16 is not of the form `c <= A ? c : c + B` in common.h"
    widest_unpadded, pad = int(m.group(1)), int(m.group(2))
    assert (widest_unpadded, pad) == (16, 16)
    for c in (8, 16, 32, 64, 128, 256):
        assert (c if c <= widest_unpadded else c + pad) == lb.lds_pitch(c)


def test_stats_epilogue_read_is_two_way_at_the_padded_pitch():
    # the price of the pad, pinned: k_mm_bwd's ds_read_b64 of x~ (8 per tile and wave) is ideal at C + 8 and takes twice its cycles at C + 16
    assert lb.quad_read(32 + 8) == lb.IDEAL["quad_read"] == 2
    assert lb.quad_read(lb.lds_pitch(32)) == 4


def test_commit_store_is_not_ideal_at_either_pitch():
    assert lb.commit_write(32 + 8, 32) == 12 and lb.commit_write(lb.lds_pitch(32), 32) == 8 and lb.IDEAL["commit_write"] == 4

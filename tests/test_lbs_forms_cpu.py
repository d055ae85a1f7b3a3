"""The frame counts of tests/test_gpu_frame_counts.py reach every kernel form the host can pick, and tests/lbs_forms.py
answers like the host's selection rules (smalify_amd/csrc/smalfit_plan.h, called through tests/host_plan_shim.cpp; no GPU
needed)."""
import os
import re

import pytest

from tests import host_plan
from tests import lbs_forms as lf

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smalify_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def plan():
    return host_plan.load()


def test_the_rules_are_the_hosts(plan):
    # skin_form and padded_verts: every frame count up to 300, vertex counts around the block size and the models'
    for V in (1, 64, 255, 256, 257, 1000, 2048, 3072, 3073, lf.NUM_VERTS, 4096, 4097, 8192, 20000):
        assert plan.padded_verts(V) == lf.padded_verts(V), V
        for M in range(1, 301):
            assert plan.skin_form(M, V) == lf.skin_form(M, V), (M, V)
    assert {plan.skin_form(M, V) for M in (4, 5, 300) for V in (64, 20000)} == {"plain", "split", "wide"}


def test_the_chunks_are_the_kernels():
    bwd, plan_h = _src("kernels_lbs_backward.inc"), _src("smalfit_plan.h")     # (the launch's constants and grid: the plan header)
    tiles = re.search(r"constexpr int PBM_SPLITS = \d+, PBM_TILES = (\d+);", plan_h)
    assert tiles and int(tiles.group(1)) == lf.PBM_TILES
    assert ("mid_pb_ids(int M) { return 10 * PBM_SPLITS * (((M + 15) / 16 + PBM_TILES - 1) / PBM_TILES); }" in plan_h)
    assert "const int nft = (M + 15) / 16, t0 = tchunk * PBM_TILES, nt = min(PBM_TILES, nft - t0);" in bwd


def test_rule_boundaries():
    assert lf.padded_verts() == 4096
    assert [lf.skin_form(M) for M in (1, 4, 5, 48, 49, 64, 65)] == ["plain", "plain", "split", "split", "wide", "wide", "wide"]
    assert [lf.pose_blend_chunks(M) for M in (1, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]


def test_frame_lists_reach_every_form():
    forms = {lf.skin_form(M) for M in lf.LBS_FRAMES}
    assert forms == {"plain", "split", "wide"}
    assert {lf.pose_blend_chunks(M) for M in lf.LBS_FRAMES} == {1, 2, 3}
    for form in ("split", "wide"):             # the matrix-core forms with full and with ragged 16-frame tiles
        ms = [M for M in lf.LBS_FRAMES if lf.skin_form(M) == form]
        assert any(lf.ragged_tile(M) for M in ms) and any(not lf.ragged_tile(M) for M in ms), form
    assert any(lf.skin_form(M) == "wide" and lf.ragged_tile(M) and lf.pose_blend_chunks(M) == 1 for M in lf.LBS_FRAMES)
    assert any(M % 8 for M in lf.LBS_FRAMES if M > 8)
    assert [lf.skin_form(M) for M in lf.ONE_PER_FORM] == ["plain", "split", "wide"]
    assert {lf.skin_form(M) for M in lf.FIT_FRAMES} == {"split", "wide"}
    assert {lf.pose_blend_chunks(M) for M in lf.FIT_FRAMES} == {1, 2, 3}


def test_prefix_pairs_share_their_forms():
    for M1, M2 in lf.PREFIX_PAIRS:
        assert M1 < M2 and lf.same_forms(M1, M2), (M1, M2)
    assert {lf.skin_form(M1) for M1, _ in lf.PREFIX_PAIRS} == {"plain", "split", "wide"}
    assert not lf.same_forms(48, 49) and not lf.same_forms(64, 65)


def test_beta_counts_reach_both_groups_and_the_limit():
    nb = lf.BETA_COUNTS
    assert min(nb) == 1 and max(nb) == 41                        # 41 = every direction of the model (NBall)
    assert 20 in nb and 21 in nb                                 # the shipped count and the first past it
    assert any(20 < b <= 32 for b in nb) and any(b > 32 for b in nb)   # dbeta_block's first and second group of 32

"""tests/fold_forms.py answers like the functions smalfit_fit_run decides with (smalify_amd/csrc/smalfit_plan.h, called through
tests/host_plan_shim.cpp), and the case lists of tests/test_gpu_fold_step.py reach every branch of the folded optimiser step
(no GPU needed)."""
import itertools
import os
import random
import re

import pytest

from smalify_amd import _lib
from tests import fold_forms as ff
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
    """run_loop for every combination of the flags, 1 to 8 iterations"""
    for K in range(1, 9):
        for graph, profiled, default_stream, accepted in itertools.product((False, True), repeat=4):
            want = ff.path(K, graph, profiled, default_stream, accepted)
            assert plan.path(K, graph, profiled, default_stream, accepted) == want, (K, graph, profiled, default_stream, accepted)


def _same_plan(plan, M, mode, offsets, ranges, gao):
    want = ff.plan_fold(M, mode, offsets, ranges, gao)
    got = plan.plan_fold(M, mode, offsets, ranges, gao)
    assert got == want, (M, mode, offsets, ranges, gao, got, want)
    return got


def test_plan_fold_is_the_hosts_on_the_case_lists(plan):
    seen = set()
    for name, why in ff.REFUSED:
        for mode in (1, 2):
            for M in ff.FRAMES:
                r = ff.refused_layout(name, M, mode)
                got = _same_plan(plan, M, mode, r["offsets"], r["ranges"], r["grad_at_offset"])[2]
                assert got == why or (M == 1 and name == "half_of_joint_rotations" and got is None)    # (half of one frame's rows: all of them)
                seen.add(why)
    for mode in (0, 1, 2):
        for M in ff.FRAMES:
            for order in (None, ff.TENSORS[::-1]):
                offs, _ = ff.layout(M, mode, order=order)
                for names, want in ff.trainable_sets(mode).values():
                    ok, train, _ = _same_plan(plan, M, mode, {k: o for k, (o, _) in offs.items()}, ff.merged_ranges(offs, names),
                                              {k: k in want for k in offs})
                    assert ok and {k for k in train if train[k]} == set(names)
    al = ff.ALIASED_LAYOUT
    seen.add(_same_plan(plan, al["M"], al["logscale_mode"], al["offsets"], al["ranges"], al["grad_at_offset"])[2])
    assert seen == {"cut", "gradient", "extra"}
    # what the restatement leaves out: independent images and a missing tensor are not folded
    offs, _ = ff.layout(4, 2)
    o = {k: v[0] for k, v in offs.items()}
    every = dict.fromkeys(offs, True)
    assert plan.plan_fold(4, 2, o, ff.merged_ranges(offs, ff.TENSORS), every)[0]
    assert plan.plan_fold(4, 2, o, ff.merged_ranges(offs, ff.TENSORS), every, subject_frames=1) == (False, dict.fromkeys(ff.TENSORS, False), "nothing")
    assert not plan.plan_fold(4, 2, {k: v for k, v in o.items() if k != "trans"}, [(0, 20)], every)[0]
    assert plan.plan_fold(0, 1, o, [(0, 20)], every) == ff.plan_fold(0, 1, o, [(0, 20)], every)


def test_plan_fold_is_the_hosts_on_random_layouts(plan):
    """tensors overlapping, padded and outside the buffer, 0 to 4 ranges drawn around the tensors' ends: every reason and the
    acceptance are met, and the restatement answers like the host each time"""
    rs = random.Random(20260)
    seen = {}
    for _ in range(6000):
        M, mode = rs.choice((1, 2, 3, 5)), rs.choice((0, 1, 2))
        cnt = ff.counts(M, mode)
        kind = rs.random()
        if kind < 0.5:                                     # a tidy buffer in a random order, sometimes padded
            offs, size = ff.layout(M, mode, order=rs.sample(ff.TENSORS, 5), pad=rs.choice((0, 0, 0, 3)))
            offsets = {k: o for k, (o, _) in offs.items()}
        else:                                              # anywhere: overlaps, gaps, negative offsets
            size = sum(cnt.values())
            offsets = {k: rs.randrange(-30, size) for k in ff.TENSORS if not (k == "log_beta_scales" and mode == 0)}
        if rs.random() < 0.15:
            offsets[rs.choice(list(offsets))] = -(1 << 20) + rs.randrange(64)         # a tensor in a buffer of its own
        if rs.random() < 0.15 and "trans" in offsets:
            offsets["trans"] = offsets["global_rotation"] + rs.choice((0, 1, -1))      # two tensors on the same floats
        names = [k for k in offsets if offsets[k] >= 0 and rs.random() < 0.6]          # (a range begins inside the buffer)
        if rs.random() < 0.6:
            ranges = ff.merged_ranges({k: (offsets[k], cnt[k]) for k in names}, names)[:4]
        else:
            ends = sorted({max(offsets[k] + d, 0) for k in offsets for d in (0, cnt[k], cnt[k] // 2, 1)} | {0, size})
            ranges = []
            for _ in range(rs.randrange(0, 5)):
                b, e = sorted((rs.choice(ends), rs.choice(ends)))
                ranges.append((b, e))
        if ranges and rs.random() < 0.1:
            b, e = ranges[-1]
            ranges[-1] = (b, e + rs.choice((1, 5)))
        gao = {k: rs.random() < 0.9 for k in offsets}
        ok, train, why = _same_plan(plan, M, mode, offsets, ranges, gao)
        seen[why] = seen.get(why, 0) + 1
    assert set(seen) == {None, "cut", "gradient", "alias", "nothing", "extra"} and min(seen.values()) >= 20, seen


def test_the_routes_are_the_hosts(plan):
    for K in range(1, 13):
        assert plan.shared_travel(K) == ff.shared_travel(K), K
        for trained in (True, False):
            assert plan.restore_slot(K, trained) == ff.restore_slot(K, trained), (K, trained)
        assert plan.prior_slot(K - 1) == ff.prior_slot(K - 1)
    for window in (1, 2, 3, 4, 8):
        for offset in range(0, 20):
            for M in range(1, 20):
                assert plan.prior_windows(window, offset, M) == ff.prior_windows(window, offset, M), (window, offset, M)
    # which tensors travel: the betas, and the limb scales when one set serves every frame
    assert [[plan.tensor_is_shared(k, mode) for k in range(5)] for mode in (0, 1, 2)] == \
        [[True, False, False, False, False], [True, True, False, False, False], [True, False, False, False, False]]
    assert plan.SHARED_SLOT_FLOATS == 3 * 32 and ff.NUM_BETAS + 6 <= 32


def test_the_sizes_are_the_hosts(plan):
    assert plan.BETA_GROUPS == ff.BETA_GROUPS
    for V in (1, 255, 256, 257, lf.NUM_VERTS, 4096, 4097):
        Vp = plan.padded_verts(V)
        assert Vp == lf.padded_verts(V)
        assert plan.nblk_beta(Vp) * plan.BETA_GROUPS == ff.column_partials(V)
        for M in (1, 5, 64):
            # shared betas: column blocks x one shape set x kBetaGroups frame groups; per frame: x M sets x one group
            assert plan.dbeta_grid(True, Vp, True, M) == (plan.nblk_beta(Vp), 1, ff.BETA_GROUPS)
            assert plan.dbeta_grid(True, Vp, False, M) == (plan.nblk_beta(Vp), M, 1)
            assert plan.dbeta_grid(False, Vp, True, M)[0] == 0
            # the head launch: M pose blocks, Vp / 256 shape blocks per shape set, the prior's block(s); the step kernel's launch
            # is the shared-shape one
            assert plan.head_blocks(M, Vp, False, "none") == M + Vp // 256
            assert plan.head_blocks(M, Vp, False, "shared") == M + Vp // 256 + 1
            assert plan.head_blocks(M, Vp, True, "none") == M + Vp // 256 * M
            assert plan.head_blocks(M, Vp, True, "per_frame") == M + Vp // 256 * M + (M + plan.HEAD_PRIOR_FRAMES - 1) // plan.HEAD_PRIOR_FRAMES
    fwd = _src("kernels_lbs_forward.inc")
    assert "constexpr int kPriorFrames = %d;" % plan.HEAD_PRIOR_FRAMES in fwd


def test_adam_ranges_are_packed_or_refused(plan):
    def adam(ranges, **kw):
        a = _lib.AdamArgs()
        a.param, a.grad, a.exp_avg, a.exp_avg_sq = 0x1000, 0x2000, 0x3000, 0x4000
        a.num_segments = len(ranges)
        for q, (b, e) in enumerate(ranges[:4]):
            a.seg_begin[q], a.seg_end[q] = b, e
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert plan.pack_adam_segments(adam([(0, 20), (26, 242)])) == (None, (2, [0, 26, 0, 0], [0, 20, 236, 236, 236]))
    assert plan.pack_adam_segments(adam([])) == (None, (0, [0, 0, 0, 0], [0, 0, 0, 0, 0]))
    assert plan.pack_adam_segments(adam([(5, 5), (1, 2), (3, 4), (0, 9)]))[1] == (4, [5, 1, 3, 0], [0, 0, 1, 2, 11])
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert plan.pack_adam_segments(adam([(0, 1)], **{field: None}))[0] == "smalfit adam: null buffer"
    assert plan.pack_adam_segments(adam([(0, 1)], num_segments=5))[0] == "smalfit adam: at most 4 segments"
    assert plan.pack_adam_segments(adam([(0, 1)], num_segments=-1))[0] == "smalfit adam: at most 4 segments"
    assert plan.pack_adam_segments(adam([(-1, 1)]))[0] == "smalfit adam: bad segment"
    assert plan.pack_adam_segments(adam([(0, 4), (3, 2)]))[0] == "smalfit adam: bad segment"


def test_the_step_kernels_sums_are_the_kernels():
    fwd = _src("kernels_lbs_forward.inc")
    assert "constexpr int kAsmFr = %d, kAsmPa = %d, kAsmLs = %d;" % (ff.ASM_FR, ff.ASM_PA, ff.ASM_LS) in fwd
    assert "constexpr int kPendingNb = %d;" % ff.NUM_BETAS in fwd
    for line in (
            "slice = min(t / 20, %d)" % (ff.BETA_SLICES - 1),
            "for (int n0 = nlo + slice; n0 < nhi; n0 += %d * kAsmFr) {" % ff.BETA_SLICES,
            "for (int k0 = slice; k0 < nparts; k0 += %d * kAsmPa) {" % ff.BETA_SLICES,
            "nparts = a.nblk_beta * a.ngrp_beta;",
            "for (int n0 = sl; n0 < a.M; n0 += %d * kAsmLs) {" % ff.LS_SLICES,
            "else if (!p.ls.train) o.ls.p = a.logscale[(size_t)n * a.ls_stride + min(t, 5)];",
            "idx = idx_pre; tv0 = tv_pend; mv = mv_pre; acc = jt_pre;"):
        assert line in fwd, "the step kernel's sums changed (%s): update tests/fold_forms.py" % line
    internal = _src("smalfit_internal.h")
    assert re.search(r"struct PendingTensor \{\s*int train;[^\n]*\n\s*const float \*p_in, \*m_in, \*v_in;\s*float \*p, \*m, \*v, \*g;\s*\};", internal)
    assert "PendingTensor betas, ls, grot, jrot, trans;" in internal


def test_path_boundaries():
    assert ff.path(1, False, False, True, True) == "plain"                 # nothing pending in a call of one iteration
    assert ff.path(2, False, False, True, True) == "folded"
    assert ff.path(2, False, False, True, False) == "plain"
    assert ff.path(7, False, True, True, True) == "plain"                  # a profiled run keeps the plain chain
    assert ff.path(7, True, False, False, True) == "graph"
    assert ff.path(7, True, False, True, True) == "folded"                 # graph switch on, default stream
    assert ff.path(7, True, False, True, False) == "plain"
    assert ff.path(7, True, True, False, True) == "plain"
    assert ff.path(1, True, False, False, True) == "plain"
    assert [ff.head_step_launches(K, False, False, True, True) for K in (1, 2, 3, 7)] == [0, 1, 2, 6]
    assert ff.head_step_launches(7, False, False, True, False) == 0


def _fitter_plan(M, mode, names, want=None, ranges=None):
    offs, _ = ff.layout(M, mode)
    want = (names if ranges is None else ff.TENSORS) if want is None else want
    return ff.plan_fold(M, mode, {k: o for k, (o, _) in offs.items()}, ff.merged_ranges(offs, names) if ranges is None else ranges,
                        {k: k in want for k in offs})


def test_plan_fold_boundaries():
    # FusedFitter's layout with stage 0's names: one range, two tensors
    offs, size = ff.layout(2, 1)
    assert offs == {"betas": (0, 20), "log_beta_scales": (20, 6), "joint_rotations": (26, 204), "global_rotation": (230, 6), "trans": (236, 6)}
    assert ff.merged_ranges(offs, ("global_rotation", "trans")) == [(230, 242)] and size == 242
    ok, train, why = _fitter_plan(2, 1, ("global_rotation", "trans"))
    assert ok and why is None and [k for k in ff.TENSORS if train[k]] == ["global_rotation", "trans"]
    # the same layout with one frame of the joint rotations in a range
    ok, train, why = _fitter_plan(2, 1, (), ranges=[(26, 26 + 102)])
    assert not ok and why == "cut" and not any(train.values())
    assert _fitter_plan(2, 1, (), ranges=[(26, 26 + 204)])[0]
    assert _fitter_plan(2, 1, (), ranges=[(26, 26 + 205)])[2] == "cut"          # one float of the global rotations
    assert _fitter_plan(2, 1, (), ranges=[(25, 26 + 204)])[2] == "cut"          # one float of the limb scales
    # all but the limb scales: two ranges with a gap
    ok, train, _ = _fitter_plan(2, 1, ("betas", "joint_rotations", "global_rotation", "trans"))
    assert ok and not train["log_beta_scales"] and sum(train.values()) == 4
    assert ff.merged_ranges(offs, ("betas", "joint_rotations", "global_rotation", "trans")) == [(0, 20), (26, 242)]
    # per-frame limb scales count M * 6; without limb scales the tensor does not exist
    assert ff.layout(3, 2)[0]["log_beta_scales"] == (20, 18) and "log_beta_scales" not in ff.layout(3, 0)[0]
    assert _fitter_plan(3, 2, ("log_beta_scales",)) == (True, dict.fromkeys(ff.TENSORS, False) | {"log_beta_scales": True}, None)
    # a trained tensor whose gradient is not asked for; an untrained one whose gradient is
    assert _fitter_plan(2, 1, ("betas", "trans"), want=("betas",))[2] == "gradient"
    assert _fitter_plan(2, 1, ("trans",), want=ff.TENSORS)[0]
    # no range at all; a range over floats of no tensor; two ranges over the same tensor
    assert _fitter_plan(2, 1, ())[2] == "nothing"
    assert _fitter_plan(2, 1, (), ranges=[(242, 250)])[2] == "nothing"
    assert _fitter_plan(2, 1, (), ranges=[(0, 20), (0, 20)])[2] == "extra"
    # two trained tensors on the same floats
    o = {k: v[0] for k, v in offs.items()}
    o["trans"] = o["global_rotation"]
    assert ff.plan_fold(2, 1, o, [(0, 236)], dict.fromkeys(ff.TENSORS, True))[2] == "alias"
    # the one kind of layout where 'cut' decides alone (see plan_fold's docstring)
    al = ff.ALIASED_LAYOUT
    assert ff.plan_fold(al["M"], al["logscale_mode"], al["offsets"], al["ranges"], al["grad_at_offset"])[2] == "cut"
    uncut = dict(al["offsets"], betas=-1000)
    assert ff.plan_fold(al["M"], al["logscale_mode"], uncut, al["ranges"], al["grad_at_offset"])[0]


def test_shared_travel_boundaries():
    assert ff.shared_travel(1) == [] and ff.restore_slot(1) is None
    assert ff.shared_travel(2) == [("caller", 1)] and ff.restore_slot(2) == 1          # K = 2 restores
    assert ff.restore_slot(2, shared_trained=False) is None
    assert ff.shared_travel(3) == [("caller", 1), (1, "caller")] and ff.restore_slot(3) is None      # home from slot 1
    assert ff.shared_travel(4) == [("caller", 1), (1, 0), (0, "caller")]               # K = 4 ends from slot 0
    assert ff.shared_travel(7)[-1] == (1, "caller") and ff.shared_travel(6)[-1] == (0, "caller")
    for K in range(2, 12):
        tr = ff.shared_travel(K)
        assert len(tr) == K - 1 and all(r != w for r, w in tr)
        assert all(tr[i][1] == tr[i + 1][0] for i in range(K - 2))                     # a step reads what its predecessor wrote
        assert (tr[-1][1] == "caller") != (ff.restore_slot(K) is not None)             # the parameters get home exactly once
        assert ff.restore_slot(K) in (None, tr[-1][1])
    assert [ff.prior_slot(it) for it in range(4)] == [0, 1, 0, 1]
    assert ff.prior_windows(4, 0, 8) == 2 and ff.prior_windows(4, 5, 2) == 0 and ff.prior_windows(4, 3, 8) == 2
    assert ff.prior_windows(4, 4, 1) == 1 and ff.prior_windows(4, 0, 1) == 1


def test_batch_boundaries():
    assert [ff.frame_batches(M) for M in (1, 96, 97, 192, 193)] == [1, 1, 2, 2, 3]
    assert [ff.scale_batches(M) for M in (1, 128, 129)] == [1, 1, 2]
    assert [ff.empty_slices(M) for M in (1, 11, 12, 31, 32)] == [(11, 31), (1, 21), (0, 20), (0, 1), (0, 0)]
    # the 3889-vertex model's column-block partials are EXACTLY one batch: the second-batch branch of asm_beta_slices
    # (k0 + 12 * kAsmPa < nparts) runs for no model this suite builds.  A larger model or another kBetaGroups makes this fail
    # and so names the gap instead of hiding it
    assert lf.padded_verts() == 4096 and ff.column_partials() == 48 * 8 == 384 == ff.BETA_SLICES * ff.ASM_PA
    assert ff.partial_batches() == 1 and ff.partial_batches(4097) == 2


def test_case_lists_reach_every_branch():
    fr = ff.FRAMES
    for lo, hi in ((4, 5), (11, 12), (31, 32), (96, 97), (128, 129)):
        assert lo in fr and hi in fr, (lo, hi)
    assert 1 in fr
    assert {lf.skin_form(M) for M in fr} == {"plain", "split", "wide"}
    assert {ff.frame_batches(M) for M in fr} == {1, 2} and {ff.scale_batches(M) for M in fr} == {1, 2}
    assert {ff.empty_slices(M)[0] > 0 for M in fr} == {True, False} and {ff.empty_slices(M)[1] > 0 for M in fr} == {True, False}
    assert len({ff.step_kernel_forms(M) for M in fr}) >= 7
    # K: restore | home from slot 1 | home from slot 0 | odd >= 5 | even >= 6; the frame cases take both parities
    assert {2, 3, 4} <= set(ff.ALL_KS) and any(K >= 5 and K % 2 for K in ff.ALL_KS) and any(K >= 6 and K % 2 == 0 for K in ff.ALL_KS)
    assert set(ff.KS) <= set(ff.ALL_KS) and {2, 3, 4} <= set(ff.KS)
    assert {ff.shared_travel(K)[-1][0] for K in ff.FRAME_KS} == {0, 1}
    # every train flag alone and absent, in each mode where the tensor exists; every set is accepted
    for mode in (0, 1, 2):
        sets = ff.trainable_sets(mode)
        every = [k for k in ff.TENSORS if not (k == "log_beta_scales" and mode == 0)]
        for k in every:
            assert sets["only_" + k][0] == (k,)
            assert any(k not in names for names, _ in sets.values())
        assert ("only_log_beta_scales" in sets) == (mode != 0)
        assert set(sets["all"][0]) == set(every)
        assert any(set(want) > set(names) for names, want in sets.values())
        if mode:
            assert set(sets["all_but_scales"][0]) == set(every) - {"log_beta_scales"}
            assert len(ff.merged_ranges(ff.layout(8, mode)[0], sets["all_but_scales"][0])) == 2      # two ranges with a gap
        for name, (names, want) in sets.items():
            ok, train, why = _fitter_plan(8, mode, names, want)
            assert ok and {k for k in train if train[k]} == set(names), (mode, name, why)
            # ... in another order in the buffer too
            offs, _ = ff.layout(8, mode, order=ff.TENSORS[::-1])
            assert ff.plan_fold(8, mode, {k: o for k, (o, _) in offs.items()}, ff.merged_ranges(offs, names), {k: k in want for k in offs})[0]
    # every refusal the host can give to tensors that do not alias
    reasons = set()
    for name, why in ff.REFUSED:
        for mode in (1, 2):
            r = ff.refused_layout(name, 8, mode)
            ok, train, got = ff.plan_fold(8, mode, r["offsets"], r["ranges"], r["grad_at_offset"])
            assert not ok and got == why and not any(train.values()), (name, mode, got)
            assert all(0 <= b < en <= r["size"] for b, en in r["ranges"]), name          # the plain chain stays inside the buffers
        reasons.add(why)
    assert reasons == {"cut", "gradient", "extra"}
    # 'cut' layouts also fail 'extra' (no case where it decides alone without aliasing)
    for name, why in ff.REFUSED:
        if why == "cut":
            r = ff.refused_layout(name, 8)
            offs = r["offs"]
            whole = [k for k in offs if any(b <= offs[k][0] and offs[k][0] + offs[k][1] <= en for b, en in r["ranges"])]
            assert sum(offs[k][1] for k in whole) != sum(en - b for b, en in r["ranges"])

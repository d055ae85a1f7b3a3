"""tests/fold_forms.py still restates what smalfit_fit_run decides on the host, and the case lists of
tests/test_gpu_fold_step.py reach every branch of the folded optimiser step (no GPU needed)."""
import os
import re

from tests import fold_forms as ff
from tests import lbs_forms as lf

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smalify_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_rules_are_the_hosts():
    launch = _src("smalfit_launch.inc")
    # the two conditions at the top of smalfit_fit_run, in this order, and the plain chain behind them
    m = re.search(r"if \(e->use_graph && !e->prof_on && iterations >= 2 && st != nullptr\) \{.*?"
                  r"if \(iterations >= 2 && !e->prof_on && plan_fold\(a, o, sg, plan\)\) \{.*?"
                  r"for \(int it = 0; it < iterations; \+\+it\) \{\s*const int t = o->step \+ it \+ 1;\s*"
                  r"if \(smalfit_fit_eval\(e, stream, a\)\) return 1;\s*if \(launch_adam_segments\(st, sg, o, t, t == 1\)\) return 1;",
                  launch, re.S)
    assert m, "smalfit_fit_run's choice of loop changed: update tests/fold_forms.py"
    # plan_fold, line by line
    for line in (
            "const float* ptr[5] = {a->betas, a->logscale_mode ? a->log_beta_scales : nullptr, a->global_rotation, a->joint_rotations, a->trans};",
            "const float* gptr[5] = {a->g_betas, a->g_log_beta_scales, a->g_global_rotation, a->g_joint_rotations, a->g_trans};",
            "const long long cnt[5] = {20, a->logscale_mode == 1 ? 6 : (long long)M * 6, (long long)M * 3, (long long)M * 102, (long long)M * 3};",
            "if (!ptr[k]) continue;",
            "if (b <= lo[k] && lo[k] + cnt[k] <= en) inside = true;",
            "else if (lo[k] < en && b < lo[k] + cnt[k]) touches = true;",
            "if (touches) return false;",
            "if (!inside) continue;",
            "if (gptr[k] != o->grad + lo[k]) return false;",
            "if (plan.train[j] && lo[j] < lo[k] + cnt[k] && lo[k] < lo[j] + cnt[j]) return false;",
            "return covered > 0 && covered == sg.off[sg.nseg];"):
        assert line in launch, "plan_fold changed (%s): update tests/fold_forms.py" % line
    # where the shared parameters travel, the restore launch, the prior's slot, the number of head-step launches
    for line in (
            "fold.pending = it ? &ps : nullptr; fold.prior_slot = it & 1; fold.assemble = last; fold.args_out = &g;",
            "if (k == 0 || (k == 1 && ls_shared)) {",
            "float* dst = e->shstate + ((it + 1) & 1) * 96 + at;",
            "const float* src = e->shstate + (it & 1) * 96 + at;",
            "if (it) { T.p_in = src; T.m_in = src + 32; T.v_in = src + 64; }",
            "if (!(it && it + 2 == iterations)) { T.p = dst; T.m = dst + 32; T.v = dst + 64; }",
            "const bool ls_shared = a->logscale_mode == 1, shared_trained = plan.train[0] || (plan.train[1] && ls_shared);",
            "if (shared_trained && iterations == 2) {",
            "shared_state_restore_kernel<<<1, 64, 0, st>>>(e->shstate + ((iterations - 1) & 1) * 96, o->param, o->exp_avg, o->exp_avg_sq,",
            "if (ex && ex->pending) lbs_head_step_kernel<<<M + h.nshape + (prior ? 1 : 0), 256, 0, st>>>(m, h, *ex->pending);",
            "const int w0 = (win.offset + win.window - 1) / win.window, w1 = (win.offset + M + win.window - 1) / win.window;",
            "ex.prior_w = a->w_betas * (float)(w1 - w0);",
            "static constexpr int kBetaGroups = %d;" % ff.BETA_GROUPS,
            "e->nblk_beta = (3 * model->Vp + 255) / 256;",
            "g.ngrp_beta = kBetaGroups;"):
        assert line in launch, "smalfit_fit_run changed (%s): update tests/fold_forms.py" % line
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

"""The pose maths on the device at the edges of its value range (-m gpu): the fused evaluation (Engine.fit_eval), the
stand-alone operators of the C ABI and the drop-in wrappers against the float64 oracle on the cases of tests/value_forms.py
(tests/test_value_forms_cpu.py proves on the host which regime each case is in).

Bounds: every deviation within the project's existing bar for the quantity, or YARD = 2 x the float32 ORACLE's own deviation
on the same inputs where that is larger (value_forms.bound; the yardstick is computed here, on the CPU), and -- with
tests/golden/hip_value_forms_measured.json present -- within RATCHET = 3 x what these kernels measured when the file was
written (floors 1e-6 on values, 1e-5 on gradients).  Every number is printed past the capture next to the float32 oracle's;
SMALFIT_WRITE_VALUE_MEASURED=<path> writes them.  `Exactly zero` and the sentinel padding round every output buffer are
equalities."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_cases as pc  # noqa: E402
from tests import value_forms as vf    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_value_forms_measured.json")
EPS32 = float(np.finfo(np.float32).eps)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


class Padded:
    """an output buffer with vf.PAD sentinel floats on each side: .t is the part handed to the library"""

    def __init__(self, *shape, fill=None):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * vf.PAD,), vf.SENTINEL, device="cuda", dtype=torch.float32)
        self.t = self.whole[vf.PAD:vf.PAD + n].view(*shape)
        if fill is not None:
            self.t.copy_(dev(fill).view(*shape))

    def intact(self):
        w = self.whole.cpu().numpy().view(np.uint32)
        s = np.array([vf.SENTINEL], np.float32).view(np.uint32)[0]
        return bool((w[:vf.PAD] == s).all() and (w[-vf.PAD:] == s).all())

    def np(self):
        return host(self.t)


def ptr(t):
    from smalify_amd import engine as eng
    return eng._ptr(t)


def stream():
    from smalify_amd import engine as eng
    return eng._stream()


class Table:
    """the printed table of one test, its bound and ratchet checks, and the record of what was measured"""

    def __init__(self, title):
        self.title, self.lines, self.bad, self.measured = title, [], [], {}
        self.recorded = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}

    def add(self, key, err, yard, kind, gradient):
        limit = vf.bound(kind, yard)
        line = "%-52s hip %.2e  (f32 oracle %.2e)  bound %.1e" % (key, err, yard, limit)
        self.lines.append(line)
        self.measured[key] = max(self.measured.get(key, 0.0), float(err))
        if not err <= limit:
            self.bad.append(line)
        floor = vf.FLOOR_GRAD if gradient else vf.FLOOR_VALUE
        if key in self.recorded and err > max(vf.RATCHET * self.recorded[key], floor):
            self.bad.append(line + "   [ratchet: %.1f x the recorded %.2e]" % (err / max(self.recorded[key], 1e-300), self.recorded[key]))

    def close(self, capsys):
        with capsys.disabled():
            print("\n[%s: HIP vs float64 oracle]\n" % self.title + "\n".join(self.lines))
        path = os.environ.get("SMALFIT_WRITE_VALUE_MEASURED")
        if path:
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc.update(self.measured)
            json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        assert not self.bad, "\n".join(self.bad)
        assert self.recorded, "tests/golden/hip_value_forms_measured.json is missing: run this file with SMALFIT_WRITE_VALUE_MEASURED=<path> on a GPU box and commit the result"


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


@pytest.fixture(scope="module")
def cases():
    return vf.fused_cases()


@pytest.fixture(scope="module")
def engine():
    e, _, _ = pc.get_engine(8, vf.S)
    e.clear_joint_limits()
    return e


# ------------------------------------------------------------------------------------------------
# A. fused evaluation
# ------------------------------------------------------------------------------------------------
def _hip_eval(e, case, weights=None, w_temp=None, tj=None, vis=None):
    """(losses (9,), {tensor: gradient}) of one smalfit_fit_eval on `case`, every output inside sentinel padding"""
    d = {k: dev(v) for k, v in case["params"].items()}
    losses = Padded(9)
    grads = {k: Padded(*case["params"][k].shape) for k in vf.PARAMS}
    if case["limits"] is not None:
        e.set_joint_limits(*case["limits"])
    try:
        e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
                   joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=dev(case["tj"] if tj is None else tj),
                   target_visibility=dev(case["vis"] if vis is None else vis), target_sil=None,
                   weights=case["weights"] if weights is None else weights, w_temp=case["w_temp"] if w_temp is None else w_temp,
                   window=vf.WINDOW, losses=losses.t, grads={k: g.t for k, g in grads.items()}, want=vf.PARAMS)
        assert e.status() == 0
    finally:
        if case["limits"] is not None:
            e.clear_joint_limits()              # the engine is shared
    assert losses.intact() and all(g.intact() for g in grads.values()), "a write outside an output buffer"
    l = losses.np()
    g = {k: v.np() for k, v in grads.items()}
    assert np.isfinite(l).all() and all(np.isfinite(v).all() for v in g.values())
    return l, g


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", vf.FUSED_NAMES)
def test_fused_evaluation_at_value_edges(name, cases, engine, capsys):
    c = cases[name]
    t64, g64 = vf.oracle_eval(c)
    t32, g32 = vf.oracle_eval(c, torch.float32)
    l, g = _hip_eval(engine, c)
    table = Table("fit_eval / " + name)
    hip, yard = vf.fused_deviations(l, g, t64, g64), vf.fused_deviations(t32, g32, t64, g64)
    assert set(hip) >= set(yard), sorted(set(yard) - set(hip))        # a quantity the oracle has is one the device reports
    for q, (err, kind) in hip.items():
        table.add("%s/%s" % (name, q), err, yard[q][0] if q in yard else float("nan"), kind, q.startswith("grad"))
    # ---- equalities ------------------------------------------------------------------------------------
    if name == "one_frame":
        assert not l[5:8].any(), l[5:8]                                # no pair of frames: the temporal losses are exactly 0.0
        l0, g0 = _hip_eval(engine, c, w_temp=0.0)
        assert _same_bits(l, l0) and all(_same_bits(g[k], g0[k]) for k in vf.PARAMS), "a temporal share in a one-frame gradient"
    if name.startswith("weights_off/"):
        col = name.split("/")[1]
        slots = vf.LOSS_NAMES if col == "all" else vf.WEIGHT_SLOTS[col]
        for s in slots:
            assert l[vf.LOSS_NAMES.index(s)] == 0.0, (s, l)
        if col == "all":
            assert all(not v.any() for v in g.values())
    if name == "visibility":
        # what an invisible target holds must not leak, and any non-zero visibility means visible
        tj2 = c["tj"].copy()
        tj2[c["vis"] == 0] = 7.0
        l2, g2 = _hip_eval(engine, c, tj=tj2, vis=(c["vis"] != 0).astype(np.float32))
        assert _same_bits(l, l2) and all(_same_bits(g[k], g2[k]) for k in vf.PARAMS)
        assert l[0] > 1e3                                              # the far-off visible target is in the loss
    if name == "limits":
        # closed form of the limit term's share of d/d joint_rotations: slope x w / (102 B_n), slope 0 AT a limit (the kernel's
        # documented convention, where autograd's torch.max splits the tie) and inside, +-1 outside, one ulp included
        _, kinds, _, _ = vf.limit_placement()
        w0 = c["weights"].copy()
        w0[4] = 0.0
        l0, g0 = _hip_eval(engine, c, weights=w0)
        assert l0[8] == 0.0 and l[8] > 0
        share = g["joint_rotations"] - g0["joint_rotations"]
        slope = np.zeros(kinds.shape)
        x, (lo, hi) = c["params"]["joint_rotations"], c["limits"]
        slope[x > hi], slope[x < lo] = 1.0, -1.0
        bn = np.array([2.0, 2.0, 1.0])[:, None, None]
        want = slope * vf.W_LIMIT / (102.0 * bn)
        flat = (kinds == 0) | (kinds == 1) | (kinds == 2) | (kinds == 4) | (kinds == 7)
        assert (slope[flat] == 0).all() and (np.abs(slope[(kinds == 3) | (kinds == 5) | (kinds == 6)]) == 1).all()
        assert _same_bits(g["joint_rotations"][flat], g0["joint_rotations"][flat]), "the limit term has a slope at or inside a limit"
        # outside: the share enters one float32 sum whose partial sums are of the size of the tensor's largest entries
        tol = 16 * EPS32 * (np.abs(g0["joint_rotations"]).max() + np.abs(want))
        assert (np.abs(share - want) <= tol).all(), float((np.abs(share - want) - tol).max())
    table.close(capsys)


# ------------------------------------------------------------------------------------------------
# B. stand-alone operators through the C ABI
# ------------------------------------------------------------------------------------------------
def _lib():
    from smalify_amd import _lib as L
    return L.load()


def _rodrigues(th, G):
    n = len(th)
    R, dth = Padded(n, 3, 3), Padded(n, 3)
    t, g = dev(th), dev(G)
    assert _lib().smalfit_rodrigues(stream(), n, ptr(t), ptr(R.t)) == 0
    assert _lib().smalfit_rodrigues_backward(stream(), n, ptr(t), ptr(g), ptr(dth.t)) == 0
    torch.cuda.synchronize()
    assert R.intact() and dth.intact(), "a write outside an output buffer"
    return R.np(), dth.np()


def test_rodrigues_per_magnitude(capsys):
    """smalfit_rodrigues / _backward: 256 rows per (magnitude, direction kind), scored per magnitude and never pooled -- the
    adjoint's 1 - cos(a) loses up to 4e-5 relative in the band 1e-4 .. 1e-3 rad, which one rel-L2 over mixed rows hides"""
    sweep = vf.rodrigues_sweep()
    R, dth = _rodrigues(np.concatenate([s[2] for s in sweep]), np.concatenate([s[3] for s in sweep]))
    assert np.isfinite(R).all() and np.isfinite(dth).all()
    table = Table("smalfit_rodrigues")
    n = vf.RODRIGUES_ROWS
    for i, (m, kind, th, G) in enumerate(sweep):
        (fwd, bwd, skew), (yf, yb, ys), d64 = vf.rodrigues_deviations(R[i * n:(i + 1) * n], dth[i * n:(i + 1) * n], th, G)
        table.add("rodrigues/%s/%s/fwd_maxabs" % (vf.magnitude_label(m), kind), fwd, yf, "rodrigues_fwd", False)
        table.add("rodrigues/%s/%s/fwd_skew_rel" % (vf.magnitude_label(m), kind), skew, ys, "rodrigues_skew", False)
        table.add("rodrigues/%s/%s/bwd_rel" % (vf.magnitude_label(m), kind), bwd, yb, "rodrigues_bwd", True)
        if m == 0.0:
            assert np.abs(dth[i * n:(i + 1) * n] - d64).max() < 1e-5          # theta = 0: the generators, finite
    for count in vf.RODRIGUES_COUNTS:
        th, G = vf.rodrigues_count_case(count)
        Rc, dc = _rodrigues(th, G)
        (fwd, bwd, skew), (yf, yb, ys), _ = vf.rodrigues_deviations(Rc, dc, th, G)
        table.add("rodrigues/count%d/fwd_maxabs" % count, fwd, yf, "rodrigues_fwd", False)
        table.add("rodrigues/count%d/fwd_skew_rel" % count, skew, ys, "rodrigues_skew", False)
        table.add("rodrigues/count%d/bwd_rel" % count, bwd, yb, "rodrigues_bwd", True)
    table.close(capsys)


def test_global_rigid_transformation_at_value_edges(synth_model, capsys):
    parents = np.ascontiguousarray(synth_model.parents, np.int32)
    table = Table("smalfit_global_rigid_transformation")
    lib = _lib()
    for scale in vf.CHAIN_SCALES:
        for count in vf.CHAIN_COUNTS:
            c = vf.chain_case(count, scale)
            Rs, Js, ls = dev(c["Rs"]), dev(c["Js"]), None if c["ls"] is None else dev(c["ls"])
            out = {"newJ": Padded(count, 35, 3), "A": Padded(count, 35, 4, 4), "dRs": Padded(count, 35, 3, 3), "dJs": Padded(count, 35, 3)}
            if ls is not None:
                out["dls"] = Padded(count, 6)
            scratch = Padded(count * 840)
            dnewJ, dA = dev(c["dnewJ"]), dev(c["dA"])
            assert lib.smalfit_global_rigid_transformation(stream(), count, ptr(Rs), ptr(Js), parents.ctypes.data, ptr(ls), ptr(out["newJ"].t),
                                                           ptr(out["A"].t)) == 0
            assert lib.smalfit_global_rigid_transformation_backward(stream(), count, ptr(Rs), ptr(Js), parents.ctypes.data, ptr(ls),
                                                                    ptr(dnewJ), ptr(dA), ptr(scratch.t), ptr(out["dRs"].t),
                                                                    ptr(out["dJs"].t), ptr(out["dls"].t) if ls is not None else None) == 0
            torch.cuda.synchronize()
            assert scratch.intact() and all(o.intact() for o in out.values()), "a write outside an output buffer"
            r64, r32 = vf.chain_oracle(c, parents), vf.chain_oracle(c, parents, torch.float32)
            for k in r64:
                got = out[k].np()
                assert np.isfinite(got).all()
                table.add("chain/scale_%s/count%d/%s" % ("none" if scale is None else "%g" % scale, count, k), vf.rel(got, r64[k]),
                          vf.rel(r32[k], r64[k]), "chain", k.startswith("d"))
            assert (out["A"].np()[:, :, 3, :] == np.array([0, 0, 0, 1.0])).all()
    table.close(capsys)


def test_projection_at_every_depth(engine, capsys):
    """forward through smalfit_render_forward with sil = NULL, backward through smalfit_project_points_backward, points at
    z_view 1, 0.1, 0.05 and -0.05 (behind the camera plane), scored per depth"""
    table = Table("projection")
    lib = _lib()
    for frames, P in vf.PROJECT_SHAPES:
        pts, g, which = vf.project_case(frames, P)
        p, gd = dev(pts), dev(g)
        proj, dp = Padded(frames, P, 2), Padded(frames, P, 3)
        assert lib.smalfit_render_forward(engine.handle, stream(), frames, ptr(p), ptr(p), P, None, ptr(proj.t)) == 0
        assert lib.smalfit_project_points_backward(stream(), frames * P, vf.S, ptr(p), ptr(gd), ptr(dp.t)) == 0
        assert engine.status() == 0
        assert proj.intact() and dp.intact(), "a write outside an output buffer"
        p64, d64 = vf.project_oracle(pts, g)
        p32, d32 = vf.project_oracle(pts, g, torch.float32)
        n = frames * P
        for k, zv in enumerate(vf.PROJECT_DEPTHS):
            sel = which == k
            if not sel.any():
                continue
            for tag, got, r64, r32 in (("proj", proj.np().reshape(n, 2), p64.reshape(n, 2), p32.reshape(n, 2)),
                                       ("dpoints", dp.np().reshape(n, 3), d64.reshape(n, 3), d32.reshape(n, 3))):
                assert np.isfinite(got).all()
                table.add("project/M%d_P%d/zv_%g/%s" % (frames, P, zv, tag), vf.rel(got[sel], r64[sel]), vf.rel(r32[sel], r64[sel]), "camera",
                          tag == "dpoints")
    table.close(capsys)


def _prior(e, x, dout):
    N = len(x)
    out, dx = Padded(N, 105), Padded(N, 105)
    xd, dd = dev(x), dev(dout)
    assert e.lib.smalfit_pose_prior(e.handle, stream(), N, ptr(xd), ptr(out.t)) == 0
    assert e.lib.smalfit_pose_prior_backward(e.handle, stream(), N, ptr(xd), ptr(dd), ptr(dx.t)) == 0
    assert e.status() == 0
    assert out.intact() and dx.intact(), "a write outside an output buffer"
    return out.np(), dx.np()


def _walking_prior(tmp_path):
    from smalify_amd import model_io
    path = tmp_path / "walking_prior.pkl"
    with gzip.open(os.path.join(HERE, "golden", "reference_priors", "walking_toy_symmetric_pose_prior_with_cov_35parts.pkl.gz"), "rb") as f:
        path.write_bytes(f.read())
    return model_io.load_pose_prior(str(path))


def test_pose_prior_at_value_edges(engine, synth_model, tmp_path, capsys):
    from smalify_amd import engine as eng, synthetic
    table = Table("smalfit_pose_prior")
    synth = synthetic.synthetic_pose_prior()
    assert (np.asarray(synth[2]) == 0).any() and (np.asarray(synth[2]) != 0).any()          # the mask has zero entries
    real_engine = eng.Engine(pc.get_model()[2], 3, 16)
    real = _walking_prior(tmp_path)
    real_engine.set_pose_prior(*real)
    for tag, e, prior, counts in (("synthetic", engine, synth, vf.PRIOR_COUNTS), ("walking", real_engine, real, (3,))):
        mean = np.asarray(prior[1], np.float32)
        for N in counts:
            x, dout = vf.prior_case(N, mean)
            out, dx = _prior(e, x, dout)
            o64, d64 = vf.prior_oracle(x, dout, prior)
            o32, d32 = vf.prior_oracle(x, dout, prior, torch.float32)
            table.add("prior/%s/N%d/out" % (tag, N), vf.rel(out, o64), vf.rel(o32, o64), "term", False)
            table.add("prior/%s/N%d/dx" % (tag, N), vf.rel(dx, d64), vf.rel(d32, d64), "grad", True)
            masked = np.asarray(prior[2]) == 0
            assert not out[:, masked].any()                                                 # a masked column is exactly zero
            # x = mean exactly: the output and the gradient are exactly zero whatever comes from upstream
            out, dx = _prior(e, np.tile(mean, (N, 1)), dout)
            assert not out.any() and not dx.any(), (tag, N)
    table.close(capsys)


def _temporal(e, g, j, t, gm, rm, w_temp, want_trans=True):
    N = len(g)
    losses, gg, gj, gt = Padded(3), Padded(N, 3), Padded(N, 34, 3), Padded(N, 3)
    gd, jd, td = dev(g), dev(j), dev(t)                     # held: a pointer does not keep its tensor alive
    gmd, rmd = None if gm is None else dev(gm), None if rm is None else dev(rm)
    assert e.lib.smalfit_temporal(e.handle, stream(), N, float(w_temp), ptr(gd), ptr(jd), ptr(td), ptr(gmd), ptr(rmd), ptr(losses.t), ptr(gg.t), ptr(gj.t), ptr(gt.t) if want_trans else None) == 0
    assert e.status() == 0
    assert all(o.intact() for o in (losses, gg, gj, gt)), "a write outside an output buffer"
    if not want_trans:
        assert (gt.np() == vf.SENTINEL).all()
    return losses.np(), gg.np(), gj.np(), gt.np()


def test_temporal_at_value_edges(engine, capsys):
    table = Table("smalfit_temporal")
    for N in (1, 2, 3, engine.max_frames):
        for masked in (False, True):
            for identical in ((False, True) if N == 3 else (False,)):
                g, j, t, gm, rm = vf.temporal_case(N, identical)
                if not masked:
                    gm = rm = None
                got = _temporal(engine, g, j, t, gm, rm, vf.W_TEMP)
                r64 = vf.temporal_oracle(g, j, t, gm, rm, vf.W_TEMP)
                r32 = vf.temporal_oracle(g, j, t, gm, rm, vf.W_TEMP, torch.float32)
                tag = "temporal/N%d/%s%s" % (N, "masked" if masked else "nomask", "/identical" if identical else "")
                if N == 1:
                    assert all(not a.any() for a in got), tag                      # no pair: exactly zero losses and gradients
                    continue
                scale = r64[0].sum()
                for i, nme in enumerate(("joint", "global", "trans")):
                    table.add(tag + "/loss_" + nme, abs(got[0][i] - r64[0][i]) / max(abs(r64[0][i]), 1e-3 * scale),
                              abs(r32[0][i] - r64[0][i]) / max(abs(r64[0][i]), 1e-3 * scale), "term", False)
                for i, nme in ((1, "global_rotation"), (2, "joint_rotations"), (3, "trans")):
                    table.add(tag + "/d" + nme, vf.rel(got[i], r64[i]), vf.rel(r32[i], r64[i]), "grad", True)
                if masked:
                    assert not got[1][:, gm == 0].any() and not got[2][:, rm == 0].any()     # a masked parameter has no gradient
                if identical:
                    assert all(not a[0].any() for a in got[1:]), tag                # frame 0's only neighbour is its twin
                # g_trans = NULL: the other outputs keep their bits
                again = _temporal(engine, g, j, t, gm, rm, vf.W_TEMP, want_trans=False)
                assert all(_same_bits(a, b) for a, b in zip(got[:3], again[:3])), tag
    # two identical frames and nothing else: every difference is exactly zero
    g, j, t, _, _ = vf.temporal_case(2, identical=True)
    got = _temporal(engine, g, j, t, None, None, vf.W_TEMP)
    assert all(not a.any() for a in got)
    table.close(capsys)


@pytest.mark.parametrize("t", vf.ADAM_STEPS)
def test_adam_step_at_value_edges(t, capsys):
    table = Table("smalfit_adam_step / t = %d" % t)
    lr, b1, b2, eps = vf.ADAM_HYPER
    for count in vf.ADAM_COUNTS:
        p, g, m, v, zero = vf.adam_case(count, t)
        want = vf.adam_reference(p, g, m, v, t)
        P, Mo, V, gd = Padded(count, fill=p), Padded(count, fill=m), Padded(count, fill=v), dev(g)
        assert _lib().smalfit_adam_step(stream(), count, ptr(P.t), ptr(gd), ptr(Mo.t), ptr(V.t), lr, b1, b2, eps, t) == 0
        torch.cuda.synchronize()
        assert P.intact() and Mo.intact() and V.intact(), "a write outside a buffer"
        for nme, got, ref in zip(("param", "exp_avg", "exp_avg_sq"), (P, Mo, V), want):
            assert np.isfinite(got.np()).all()
            table.add("adam_step/t%d/count%d/%s" % (t, count, nme), vf.rel(got.np(), ref), float("nan"), "adam", False)
        assert _same_bits(P.np()[zero], p[zero]), "a zero gradient on zero moments moved the parameter"
    table.close(capsys)


@pytest.mark.parametrize("step", [t - 1 for t in vf.ADAM_STEPS])
def test_adam_segments_at_value_edges(step, capsys):
    """smalfit_adam_segments over 1 to 4 ranges, one of them empty: the ranges against the float64 replica, every float outside
    them untouched; at step 0 the moments are taken as zero and not read (they hold stale values here)"""
    from smalify_amd import engine as eng
    table = Table("smalfit_adam_segments / step = %d" % step)
    lr, b1, b2, eps = vf.ADAM_HYPER
    n = vf.ADAM_FLAT
    for segs in vf.ADAM_SEGMENT_SETS:
        p, g, m, v, zero = vf.adam_case(n, step + 1, seed=113 + len(segs))
        if step == 0:
            rs = np.random.RandomState(7)
            m_in, v_in = rs.randn(n).astype(np.float32), rs.rand(n).astype(np.float32)       # stale: must not be read
        else:
            m_in, v_in = m, v
        inside = np.zeros(n, bool)
        for b, e_ in segs:
            inside[b:e_] = True
        want = vf.adam_reference(p, g, m, v, step + 1)
        P, Mo, V = Padded(n, fill=p), Padded(n, fill=m_in), Padded(n, fill=v_in)
        gd = dev(g)
        a = eng.make_adam_args(P.t, gd, Mo.t, V.t, list(segs), lr, step=step, beta1=b1, beta2=b2, eps=eps)
        assert _lib().smalfit_adam_segments(stream(), C.byref(a)) == 0
        torch.cuda.synchronize()
        assert P.intact() and Mo.intact() and V.intact(), "a write outside a buffer"
        for nme, got, ref, before in zip(("param", "exp_avg", "exp_avg_sq"), (P, Mo, V), want, (p, m_in, v_in)):
            table.add("adam_segments/step%d/%dseg/%s" % (step, len(segs), nme), vf.rel(got.np()[inside], ref[inside]), float("nan"), "adam", False)
            assert _same_bits(got.np()[~inside], before[~inside]), "a float outside the ranges changed"
        assert _same_bits(P.np()[zero & inside], p[zero & inside])
    table.close(capsys)


# ------------------------------------------------------------------------------------------------
# C. the drop-in wrappers with awkward tensors
# ------------------------------------------------------------------------------------------------
def _awkward(a, kind):
    """a tensor of the values of `a` (float32 numpy) that is a leaf requiring grad: contiguous float32, a non-contiguous float32
    view's base (strided slice of a wider buffer, or a transposed buffer), or float64"""
    t = torch.from_numpy(a).cuda()
    if kind == "plain":
        leaf = t.clone().requires_grad_(True)
        return leaf, leaf
    if kind == "float64":
        leaf = t.double().requires_grad_(True)
        return leaf, leaf
    if kind == "strided":
        wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device="cuda")
        wide[..., ::2] = t
        leaf = wide.requires_grad_(True)
        view = leaf[..., ::2]
    else:
        leaf = t.transpose(0, -1).contiguous().requires_grad_(True)
        view = leaf.transpose(0, -1)
    assert not view.is_contiguous()
    return leaf, view


def _leaf_grad(leaf, kind):
    g = leaf.grad
    if kind == "strided":
        return g[..., ::2].float().cpu().numpy()
    if kind == "transposed":
        return g.transpose(0, -1).float().cpu().numpy()
    return g.float().cpu().numpy()


def _awkward_upstream(w, kind):
    """the upstream gradient `w` as the grad_output autograd hands the wrapper: non-contiguous for the view kinds"""
    t = torch.from_numpy(w).cuda()
    if kind in ("strided", "transposed"):
        t = t.transpose(0, -1).contiguous().transpose(0, -1)
        assert not t.is_contiguous()
    return t


@pytest.mark.parametrize("kind", ["strided", "transposed", "float64"])
def test_wrappers_take_awkward_tensors(kind, synth_model):
    """batch_rodrigues, batch_global_rigid_transformation, Renderer (points branch) and SMAL.__call__: inputs given as
    non-contiguous views or as float64, and gradients arriving through a non-contiguous grad_output, give the bits of the
    contiguous float32 call"""
    from smalify_amd.smal_model.batch_lbs import batch_global_rigid_transformation, batch_rodrigues
    from smalify_amd.smal_model.smal_torch import SMAL
    from smalify_amd.smal_fitter.p3d_renderer import Renderer
    rs = np.random.RandomState(127)
    n = 5
    smal = SMAL("cuda", shape_family_id=1, model_data=synth_model)
    renderer = Renderer(16, "cuda", model=smal.device_model)
    c = vf.chain_case(n, 0.3)
    inputs = {
        "rodrigues": [(0.7 * rs.randn(37, 3)).astype(np.float32)],
        "chain": [c["Rs"], c["Js"], c["ls"]],
        "project": [np.concatenate([0.3 * rs.randn(n, 25, 2), 1.0 + 0.5 * rs.rand(n, 25, 1)], 2).astype(np.float32)],
        "smal": [(0.5 * rs.randn(n, 20)).astype(np.float32), (0.3 * rs.randn(n, 35, 3)).astype(np.float32), (0.2 * rs.randn(n, 6)).astype(np.float32)],
    }
    verts0 = torch.from_numpy(rs.randn(n, smal.size[0], 3).astype(np.float32) * 0.1).cuda()

    def call(op, xs):
        if op == "rodrigues":
            return [batch_rodrigues(xs[0])]
        if op == "chain":
            return list(batch_global_rigid_transformation(xs[0], xs[1], synth_model.parents, betas_logscale=xs[2]))
        if op == "project":
            return [renderer(verts0, xs[0], None)[1]]
        return list(smal(xs[0], xs[1], betas_logscale=xs[2])[:2])

    for op, arrays in inputs.items():
        results = {}
        ups = None
        for k in ("plain", kind):
            pairs = [_awkward(a, k) for a in arrays]
            outs = call(op, [v for _, v in pairs])
            if ups is None:
                ups = [rs.randn(*o.shape).astype(np.float32) for o in outs]
            assert all(o.dtype == torch.float32 for o in outs)
            torch.autograd.backward(outs, grad_tensors=[_awkward_upstream(w, k) for w in ups])
            results[k] = ([o.detach().cpu().numpy() for o in outs], [_leaf_grad(leaf, k) for leaf, _ in pairs])
        for a, b in zip(results["plain"][0] + results["plain"][1], results[kind][0] + results[kind][1]):
            assert a.shape == b.shape and _same_bits(a, b), (op, kind)

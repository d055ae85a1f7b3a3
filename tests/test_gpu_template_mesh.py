"""The rasteriser and the 3-D kernels on the reference's SMAL template mesh (-m gpu): tests/golden/smal_template_mesh.npz in the
views of tests/template_cases.py (tests/test_template_cases_cpu.py proves on the host what each view reaches -- hundreds of
candidates on a pixel in ordinary views, the 1024 caps crossed by sliver faces at near-equal depths, faces at the cull threshold,
mask and list hand-off in one frame -- and that the ambiguity rule is enough).

  a  loose     every view, all pixels, the project's bars for SMAL poses (tests/test_gpu_parity.py::test_renderer): silhouette
               max-abs 2e-3, fewer than 5e-3 of the pixels off by more than 1e-4, d/d verts rel-L2 1e-2
  b  tight     the views the rule can keep: silhouette on the kept pixels, d/d verts (rel-L2 and the worst vertex row over the
               largest) with the upstream weights zeroed on the pixels left out; bound = max(floor, YARD x the float32 ORACLE's own
               deviation on the same pixels), floors 1e-5; RATCHET x tests/golden/hip_template_measured.json
               (SMALFIT_WRITE_TEMPLATE_MEASURED=<path> writes it)
  c  stale depth cache, d frame independence, e fit_eval's silhouette term, f fit_metrics' coverage
  g  the template as the one target mesh of the 3-D kernels: mesh_score, the sampler, the surface term

Every number is printed past the capture."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import smal_oracle as so                  # noqa: E402
from smalify_amd import engine as eng                 # noqa: E402
from smalify_amd import synthetic                     # noqa: E402
from tests import metrics_cases as mc                 # noqa: E402
from tests import raster_forms as rf                  # noqa: E402
from tests import template_cases as tc                # noqa: E402
from tests import test_gpu_raster_forms as grf        # noqa: E402
from tests import value_forms as vf                   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_template_measured.json")
LOOSE_SIL, LOOSE_SHARE, LOOSE_GRAD = 2e-3, 5e-3, 1e-2        # tests/test_gpu_parity.py::test_renderer
TIGHT_SIL, TIGHT_GRAD = tc.SIL_BAR, vf.FLOOR_GRAD            # the floors of the tight comparison
MAX_FRAMES = 3
W_SIL = 100.0


class Table:
    """the printed table of one test, its bound and ratchet checks, and the record of what was measured (the layout and the
    rule of tests/test_gpu_value_forms.py: Table, on a file of its own)"""

    def __init__(self, title):
        self.title, self.lines, self.bad, self.measured = title, [], [], {}
        self.recorded = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}

    def add(self, key, err, bar, gradient, yard=None, floor=None):
        """floor: of the ratchet, for a quantity that is no relative deviation (ulp(L): 1, as tests/test_gpu_mesh_score.py)"""
        limit = bar if yard is None else max(bar, vf.YARD * yard)
        line = "%-44s hip %.2e  %s bound %.1e" % (key, err, "" if yard is None else "(f32 oracle %.2e) " % yard, limit)
        self.lines.append(line)
        self.measured[key] = max(self.measured.get(key, 0.0), float(err))
        if not err <= limit:
            self.bad.append(line)
        floor = floor if floor is not None else (vf.FLOOR_GRAD if gradient else vf.FLOOR_VALUE)
        if key in self.recorded and err > max(vf.RATCHET * self.recorded[key], floor):
            self.bad.append(line + "   [ratchet: %.1f x the recorded %.2e]" % (err / max(self.recorded[key], 1e-300), self.recorded[key]))

    def note(self, text):
        self.lines.append(text)

    def close(self, capsys):
        with capsys.disabled():
            print("\n[%s: HIP vs float64 oracle]\n" % self.title + "\n".join(self.lines))
        path = os.environ.get("SMALFIT_WRITE_TEMPLATE_MEASURED")
        if path:
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc.update(self.measured)
            json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        assert not self.bad, "\n".join(self.bad)
        assert self.recorded, "tests/golden/hip_template_measured.json is missing: run this file with SMALFIT_WRITE_TEMPLATE_MEASURED=<path> on a GPU box and commit the result"
        missing = [k for k in self.measured if k not in self.recorded]
        assert not missing, "not in tests/golden/hip_template_measured.json: %s" % missing


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


_CTX = {}


def _engine(S, tag=0):
    """an engine of MAX_FRAMES frames at S^2 on the rigid template model, priors set (fit_eval wants them)"""
    if "dm" not in _CTX:
        _CTX["dm"] = eng.DeviceModel(tc.model_data())
    if (S, tag) not in _CTX:
        e = eng.Engine(_CTX["dm"], MAX_FRAMES, S)
        e.set_pose_prior(*synthetic.synthetic_pose_prior())
        e.set_shape_prior(*synthetic.synthetic_shape_prior())
        _CTX[(S, tag)] = e
    return _CTX[(S, tag)]


def _verts(vid):
    return tc.world(vid).astype(np.float32)


def _hip(e, vids, weights):
    """(sil (n,S,S), d/d template verts (n,3889,3)) float64 of one cold call on the views `vids`"""
    e.reset_raster_cache()
    v = grf._pad([_verts(x) for x in vids])
    sil, _ = e.render_forward(v)
    dv = e.render_backward(v, sil, torch.from_numpy(np.stack(weights).astype(np.float32)).cuda())
    assert e.status() == 0
    return sil.double().cpu().numpy(), dv.double().cpu().numpy()[:, grf.SLOTS[:tc.V]]


# ---- a. loose, all pixels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vid", tc.VIEW_IDS)
def test_loose_on_all_pixels(vid, capsys):
    sil_o, dv_o = tc.oracle(vid)
    sil, dv = _hip(_engine(tc.size(vid)), [vid], [tc.upstream(vid)])
    d = np.abs(sil[0] - sil_o)
    es, share, eg = float(d.max()), float((d > 1e-4).mean()), tc.rel(dv[0], dv_o)
    with capsys.disabled():
        print("\n[loose %-15s sil %.2e (<%.0e)  share off by > 1e-4 %.2e (<%.0e)  dverts %.2e (<%.0e)]"
              % (vid, es, LOOSE_SIL, share, LOOSE_SHARE, eg, LOOSE_GRAD))
    assert es < LOOSE_SIL and share < LOOSE_SHARE and eg < LOOSE_GRAD
    assert np.all(sil[0][sil_o == 0.0] == 0.0)                           # pixels no face reaches: exactly 0
    # the vertices whose faces lie in pixels past the K cut and past the 1024 caps, on their own (nothing is left out here)
    a = tc.analysis(vid)
    for name, cap in (("> K", tc.K), ("> 1024", rf.CAND_CAP)):
        rows = a.vertices_of_pixels(a.count > cap)
        assert (len(rows) > 0) == bool((a.count > cap).any())
        if len(rows):
            part = tc.rel(dv[0][rows], dv_o[rows])
            with capsys.disabled():
                print("      %4d vertices of %s pixels: dverts %.2e (<%.0e)" % (len(rows), name, part, LOOSE_GRAD))
            assert part < LOOSE_GRAD


# ---- b. tight, on what the rule keeps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("vid", tc.TIGHT_IDS)
def test_tight_on_kept_pixels(vid, capsys):
    a = tc.analysis(vid)
    keep, gkeep = ~a.image(a.sil_excluded), ~a.image(a.grad_excluded)
    w = tc.upstream(vid) * gkeep
    sil_o, _ = tc.oracle(vid)
    sil_32, _ = tc.oracle(vid, "float32")
    _, dv_o = tc.oracle(vid, "float64", gkeep)
    _, dv_32 = tc.oracle(vid, "float32", gkeep)
    sil, dv = _hip(_engine(a.S), [vid], [w])
    sil, dv = sil[0], dv[0]
    table = Table("template %s: %d covered pixels, %.1f %% / %.1f %% left out" % ((vid, int(a.covered.sum())) + tuple(100 * s for s in a.shares())))
    table.add("%s sil, kept pixels" % vid, float(np.abs(sil - sil_o)[keep].max()), TIGHT_SIL, False, float(np.abs(sil_32 - sil_o)[keep].max()))
    table.add("%s dverts rel-L2" % vid, tc.rel(dv, dv_o), TIGHT_GRAD, True, tc.rel(dv_32, dv_o))
    table.add("%s dverts worst row / largest" % vid, tc.worst_row(dv, dv_o), TIGHT_GRAD, True, tc.worst_row(dv_32, dv_o))
    # the vertices whose faces lie in pixels past the K cut, and past the 1024 caps: lines of their own, at the project's bar
    for name, cap in (("> K", tc.K), ("> 1024", rf.CAND_CAP)):
        rows = a.vertices_of_pixels((a.count > cap) & ~a.grad_excluded)
        if len(rows):
            table.add("%s dverts rel-L2, %d vertices of %s pixels" % (vid, len(rows), name), tc.rel(dv[rows], dv_o[rows]), LOOSE_GRAD, True,
                      tc.rel(dv_32[rows], dv_o[rows]))
        else:
            table.note("%s: no kept pixel with %s candidates" % (vid, name))
    never = a.never_near()
    assert len(never) and np.all(dv[never] == 0.0) and np.all(dv_o[never] == 0.0), int(np.sum(dv[never] != 0.0))
    assert np.all(sil[sil_o == 0.0] == 0.0)
    table.close(capsys)


# ---- c ... e: the rigid template model through fit_eval ------------------------------------------------------------------------
ZERO = dict(log_beta_scales=np.zeros(6, np.float32), joint_rotations=np.zeros((1, 34, 3), np.float32))
WEIGHTS = [0.0, W_SIL, 0.0, 0.0, 0.0, 0.0]
WANT = ("trans", "global_rotation", "betas")
# d rotation, d trans of the target's view: turned a little, moved sideways and 0.15 towards the camera -- the target is some 6 %
# larger than the render, so that d/d betas[0] (the scale) is a sum of one sign and not the remainder of a cancellation
DISPLACED = (np.array([0.02, -0.015, 0.01], np.float32), np.array([0.03, 0.0, 0.15], np.float32))


def _params(vid, d_rot=None, d_trans=None):
    rv, t = tc.pose_of(vid)
    if d_rot is not None:
        rv, t = rv + d_rot, t + d_trans
    return dict(ZERO, betas=np.zeros(20, np.float32), global_rotation=rv[None].astype(np.float32), trans=t[None].astype(np.float32))


def _problem(S, tsil):
    pp, sp = synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior()
    if "om" not in _CTX:
        _CTX["om"] = so.OracleModel(tc.model_data())
    return so.FitProblem(_CTX["om"], S, np.zeros((1, 25, 2), np.float32), np.zeros((1, 25), np.float32), tsil[None], pp[0], pp[1], pp[2],
                         sp[0], sp[1], 1, use_unity_prior=True)


def _target(vid):
    """the thresholded float64 oracle silhouette of the view turned and moved by DISPLACED"""
    key = ("target", vid)
    if key not in _CTX:
        p = {k: torch.from_numpy(x).double() for k, x in _params(vid, *DISPLACED).items()}
        om = _problem(tc.size(vid), np.zeros((tc.size(vid),) * 2, np.float32)).m
        theta = torch.cat([p["global_rotation"][:, None], p["joint_rotations"]], 1)
        with torch.no_grad():
            v, _, _, _ = so.smal_forward(om, p["betas"][None], theta, p["log_beta_scales"][None])
            sil = so.soft_silhouette(v + p["trans"][:, None], om.faces, tc.size(vid))[0].numpy()
        _CTX[key] = (sil > 0.5).astype(np.float32)
    return _CTX[key]


def _fit_eval(e, params, tsil):
    d = {k: torch.from_numpy(x).cuda() for k, x in params.items()}
    losses, grads = e.fit_eval(**d, target_joints=torch.zeros(1, 25, 2, device="cuda"), target_visibility=torch.zeros(1, 25, device="cuda"),
                               target_sil=tsil, weights=WEIGHTS, w_temp=0.0, window=1, want=WANT)
    assert e.status() == 0
    return losses.cpu().numpy().copy(), {k: g.cpu().numpy().copy() for k, g in grads.items()}


@pytest.mark.parametrize("vid", ("init_far-64", "native_far-64"))
def test_fit_eval_silhouette_term(vid, capsys):
    S = tc.size(vid)
    tsil = _target(vid)
    assert 0.02 < tsil.mean() < 0.5
    params = _params(vid)
    _, sums, g_o = so.loss_and_grads(_problem(S, tsil), {k: torch.from_numpy(x).double() for k, x in params.items()}, WEIGHTS, 0.0, WANT)
    e = _engine(S)
    e.reset_raster_cache()
    losses, grads = _fit_eval(e, params, torch.from_numpy(tsil[None]).cuda())
    e.reset_raster_cache()
    losses_u8, grads_u8 = _fit_eval(e, params, torch.from_numpy((tsil[None] * 255).astype(np.uint8)).cuda())
    assert losses.tobytes() == losses_u8.tobytes() and all(grads[k].tobytes() == grads_u8[k].tobytes() for k in WANT)
    total = abs(float(losses[4]) - sums["sil_reproj"]) / abs(sums["sil_reproj"])
    lines = ["fit %-15s sil loss %.6f rel %.2e (<1e-4)" % (vid, sums["sil_reproj"], total)]
    errs = {"trans": tc.rel(grads["trans"].astype(np.float64), g_o["trans"].numpy()),
            "global_rotation": tc.rel(grads["global_rotation"].astype(np.float64), g_o["global_rotation"].numpy()),
            "betas[0]": abs(float(grads["betas"].reshape(-1)[0]) - float(g_o["betas"][0])) / abs(float(g_o["betas"][0]))}
    lines += ["    d/d %-16s %.2e (<2e-3)" % kv for kv in errs.items()]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert float(losses.sum()) == float(losses[4]) and sums["sil_reproj"] > 0.1
    assert total < 1e-4
    assert all(v < 2e-3 for v in errs.values()), errs


@pytest.mark.parametrize("vid", ("init_far-64", "native_far-64"))
def test_a_stale_depth_cache_never_changes_results(vid, capsys):
    """the pose drifts over 4 small steps: engine A keeps its cached depth bounds, engine B forgets them before every call"""
    S = tc.size(vid)
    tsil = torch.from_numpy(_target(vid)[None]).cuda()
    e_a, e_b = _engine(S), _engine(S, tag=1)
    rs = np.random.RandomState(3)
    params = _params(vid)
    e_a.reset_raster_cache()
    loss_rel, grad_rel = 0.0, 0.0
    for step in range(6):
        if step >= 2:                                  # steps 0 and 1: the same pose, fresh and then fully cached
            params = dict(params, global_rotation=params["global_rotation"] + (0.004 * rs.randn(1, 3)).astype(np.float32),
                          trans=params["trans"] + (0.003 * rs.randn(1, 3)).astype(np.float32))
        la, ga = _fit_eval(e_a, params, tsil)
        e_b.reset_raster_cache()
        lb, gb = _fit_eval(e_b, params, tsil)
        loss_rel = max(loss_rel, abs(float(la.sum()) - float(lb.sum())) / abs(float(lb.sum())))
        grad_rel = max([grad_rel] + [tc.rel(ga[k].astype(np.float64), gb[k].astype(np.float64)) for k in WANT])
    with capsys.disabled():
        print("\n[stale cache %-15s loss %.2e (<2e-6)  gradients %.2e (<2e-5)]" % (vid, loss_rel, grad_rel))
    assert loss_rel < 2e-6 and grad_rel < 2e-5


# ---- d. frames -----------------------------------------------------------------------------------------------------------
def test_frames_are_independent_bit_for_bit():
    vids = ("init_far-64", "native_far-64", "init_tilt-64")
    e = _engine(64)

    def run(idx):
        e.reset_raster_cache()
        v = grf._pad([_verts(vids[i]) for i in idx])
        sil, _ = e.render_forward(v)
        e.reset_raster_cache()
        dv = e.render_backward(v, sil, torch.from_numpy(np.stack([tc.upstream(vids[i]) for i in idx])).cuda())
        assert e.status() == 0
        return sil.cpu().numpy(), dv.cpu().numpy()

    singles = [run([i]) for i in range(3)]
    for _ in range(2):                                                   # two identical calls: identical bits
        sil, dv = run([0, 1, 2])
        for i in range(3):
            assert np.array_equal(sil[i], singles[i][0][0]), i
            assert np.array_equal(dv[i], singles[i][1][0]), i
    sil, dv = run([2, 0])                                                # another order, another frame count
    assert np.array_equal(sil[0], singles[2][0][0]) and np.array_equal(dv[1], singles[0][1][0])
    assert len({s[0].tobytes() for s in singles}) == 3


# ---- f. fit_metrics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vid", tc.VIEW_IDS)
def test_fit_metrics_coverage(vid, capsys):
    a = tc.analysis(vid)
    S = a.S
    mask, free = a.image(a.mask), a.image(a.mask_excluded)
    target = np.roll(mask, 3, axis=-1)
    e = _engine(S)
    v = grf._pad([_verts(vid)])
    got = None
    for tgt in (target.astype(np.float32), target.astype(np.uint8) * 255):
        out = e.fit_metrics(v, torch.from_numpy(tgt[None]).cuda(), want_mask=True)
        assert e.status() == 0
        out = {k: x.cpu().numpy() for k, x in out.items()}
        assert got is None or all(out[k].tobytes() == got[k].tobytes() for k in got)
        got = out
    m = got["mask"][0].astype(bool)
    differ = m != mask
    with capsys.disabled():
        print("\n[metrics %-15s covered %d, undecided %d, differing %d]" % (vid, int(mask.sum()), int(free.sum()), int(differ.sum())))
    assert not (differ & ~free).any(), int((differ & ~free).sum())
    assert got["sil_counts"][0].tolist() == mc.counts(m, target).tolist()
    lo, hi = mc.counts(mask & ~free, target), mc.counts(mask | free, target)
    want = mc.counts(mask, target)
    c = got["sil_counts"][0].astype(np.int64)
    assert (lo[:3] <= c[:3]).all() and (c[:3] <= hi[:3]).all() and c[3] == want[3]
    if not free.any():
        assert c.tolist() == want.tolist()
    assert 0 < want[0] < want[2] < want[1]


# ---- g. the template as the one target mesh of the 3-D kernels ----------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _targets():
    if "targets" not in _CTX:
        tv, tf = tc.target_mesh()
        _CTX["targets"] = eng.MeshTargets([tv], [tf])
    return _CTX["targets"]


def test_mesh_score_both_directions(capsys):
    """the bent template (the template's own topology: every scanned triangle is one of its 7774, in both roles) against the
    template: float64 brute force on the same float32 inputs, in ulp(L); the bar of tests/test_gpu_mesh_score.py -- 4 x the host
    shim's recorded worst"""
    from tests import mesh_score_cases as msc
    tv, tf = tc.target_mesh()
    fit = tc.bent_template()[None]
    S = 3000
    obj = eng.MeshObjective(tc.V, tf, 1, S)
    tg = _targets()
    pts = tg.sample(S, 17, 0)
    o = obj.score(_t(fit), tg, pts, (0.01, 0.05))
    torch.cuda.synchronize()
    p = pts.cpu().numpy()
    want0 = msc.surface_dist_culled(fit[0], tv, tf)
    want1 = msc.surface_dist_culled(p[0], fit[0], tf)
    assert want0.mean() > 3e-3 and want1.mean() > 3e-3                                    # not a fit
    shim = json.load(open(os.path.join(HERE, "golden", "hip_mesh_score_measured.json")))["shim/near_surface_ulp"]
    bar = msc.DEVICE_FACTOR_OVER_SHIM * shim
    table = Table("mesh_score, template against the bent template (ulp(L))")
    for key, got, want, L in (("mesh_score vert_dist ulp(L)", o["vert_dist"], want0, msc.ulp_l(fit, tv)),
                              ("mesh_score point_dist ulp(L)", o["point_dist"], want1, msc.ulp_l(p, fit))):
        got = got.cpu().numpy()[0]
        assert np.isfinite(got).all()
        table.add(key, msc.deviation_ulp(got, want, L), bar, False, floor=1.0)
    s = o["sums"].cpu().numpy()[0]
    for d, k in enumerate(("vert_dist", "point_dist")):
        got = o[k].cpu().numpy()[0].astype(np.float64)
        assert abs(s[d, 0] - got.sum()) <= len(got) * 2.0 ** -24 * got.sum() and s[d, 2] == got.max()
    table.close(capsys)


def _shim_sample(shim, S, seed, it):
    import ctypes as C
    tv, tf = tc.target_mesh()
    v, f = np.ascontiguousarray(tv, np.float32), np.ascontiguousarray(tf, np.int32)
    want, chosen = np.zeros((S, 3), np.float32), np.zeros(S, np.int32)
    assert shim.hm3_sample(len(v), v.ctypes.data_as(C.c_void_p), len(f), f.ctypes.data_as(C.c_void_p), S, C.c_ulonglong(seed), it, 0,
                           want.ctypes.data_as(C.c_void_p), chosen.ctypes.data_as(C.c_void_p)) == 0
    return want, chosen


def test_sampler_is_the_host_shim_bit_for_bit():
    from tests import host_shim
    seed, it, S = (5 << 32) | 23, 3, 4096
    p = _targets().sample(S, seed=seed, iteration=it)
    torch.cuda.synchronize()
    want, _ = _shim_sample(host_shim.mesh3d(), S, seed, it)
    got = p.cpu().numpy()[0]
    assert got.shape == (S, 3)
    differ = got.view(np.int32) != want.view(np.int32)
    assert not differ.any(), (int(differ.sum()), float(np.abs(got - want).max()))


def test_sampler_draws_faces_by_area(capsys):
    """200 000 points in one launch: the faces the draw picked (the host shim's, on the same counters; the points agree) in 64
    bins of equal face count by area, each within 5 binomial standard deviations of the share its faces' threshold intervals hold"""
    from tests import host_shim
    seed, it, S = (9 << 32) | 41, 1, 200_000
    p = _targets().sample(S, seed=seed, iteration=it)
    torch.cuda.synchronize()
    want, chosen = _shim_sample(host_shim.mesh3d(), S, seed, it)
    got = p.cpu().numpy()[0]
    assert float(np.abs(got - want).max()) < 1e-6                       # the same draw: `chosen` names the device's faces
    tv, tf = tc.target_mesh()
    thr, share, area = tc.sampler_intervals(tv, tf)
    assert abs(share.sum() - 1.0) < 1e-12 and np.abs(share - area / area.sum()).max() < 2.0 ** -31
    counts = np.bincount(chosen, minlength=tc.F)
    assert not counts[share == 0.0].any()                               # an empty interval is never drawn
    order = np.argsort(area, kind="stable")
    worst, lines = 0.0, []
    for b, ids in enumerate(np.array_split(order, 64)):
        q = float(share[ids].sum())
        n, sd = int(counts[ids].sum()), float(np.sqrt(S * q * (1.0 - q)))
        worst = max(worst, abs(n - S * q) / sd)
        lines.append("bin %2d: %4d faces, share %.3e, drawn %6d, expected %9.1f, %+.2f sd" % (b, len(ids), q, n, S * q, (n - S * q) / sd))
    with capsys.disabled():
        print("\n[sampler: 200000 points over 64 area quantiles, worst %.2f sd (<5); smallest interval %.0f of 2^32]\n" % (worst, (share * 2.0 ** 32).min())
              + "\n".join(lines[:3] + ["..."] + lines[-3:]))
    assert worst < 5.0


def test_surface_term_against_the_template(capsys):
    """a strip of 256 vertices scattered about the template's surface: its vertices scan the template's 7774 triangles, 256 points
    sampled on the template scan the strip; the checks and bars of tests/test_gpu_surface_term.py"""
    from tests import test_gpu_surface_term as gst
    tv, tf = tc.target_mesh()
    fv, ff = tc.small_fit(256)
    pts = _targets().sample(256, 29, 2).cpu().numpy()
    with capsys.disabled():
        print()
        o, _ = gst._surface(fv[None], ff, [(tv, tf)], pts, 1.0, 0.5, max_points=256)
        gst._check_call("template", o, fv[None], ff, [(tv, tf)], pts, 1.0, 0.5)
    assert o["losses"][2] > 0

"""The gated point-to-surface term on the device (mesh3d_surface_near / hit <ROLE, GATED>, mesh3d_vertex_normal, the sampler's
normals, behind MeshObjective.surface(gates=), smalfit_fit3d_step_gated and Stage(surface_gates=); the definitions are this
project's, include/smalfit.h) (-m gpu).  Every mesh is tens to about a thousand triangles.

  gates open    gate = NULL, a block with every gate off, and a block that only asks for the masks equal the ungated call bit for
                bit, stand-alone and over three steps; kept = (S, V)
  closed forms  the plate with a hole, two plates wound in opposite ways, no compatible face at all, truncation on the cube
  branches      queries in 3, 63, 64, 65, 130 and scanned triangles in 1, 2, 511, 512, 513, 1027 in both roles; one slice against
                16; a ragged batch of 1-, 513- and 7-face targets against the one-mesh calls; each gate alone and all together
  oracle        posed stand-in pieces with patches removed against tests/surface_gate_cases.py in float64: the kept masks equal
                at every unflagged query, the faces the oracle's or a tie with them (faces_equivalent: a closest point on an edge
                two faces share ties in exact arithmetic, and rounding picks), |r| within DELTA_ULP ulp(L), kept = the masks'
                popcount, rows within (count + 16) 2^-24 over the kept, dverts within the float32 summation bound of the
                returned correspondences, vert_normals against float64 on the same float32 vertices
  sampler       the points of smalfit_mesh_targets_sample bit for bit, the normals of the faces they lie on
  the step      fused against unfused with the gates on; 30 Adam steps on a target with a third of its faces removed against the
                float64 loop (4 x the float32 yardstick, 3 x tests/golden/hip_surface_gate_measured.json;
                SMALFIT_WRITE_SURFACE_GATE_MEASURED=<path> writes it)
  refusals      leave every output alone

Every figure is printed before it is judged.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib                        # noqa: E402
from smalify_amd import engine as eng               # noqa: E402
from tests import host_surface_gate as hg           # noqa: E402
from tests import mesh3d_cases as m3                # noqa: E402
from tests import mesh_score_cases as mc            # noqa: E402
from tests import surface_gate_cases as gc          # noqa: E402
from tests import surface_term_cases as sc          # noqa: E402

MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_surface_gate_measured.json")
DEV = "cuda"
ULP = 2.0 ** -23
RATCHET = 3.0


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _targets(targets):
    return eng.MeshTargets([t[0] for t in targets], [t[1] for t in targets]) if targets is not None else None


def _surface(fit, faces, targets, points, normals=None, gates=None, w_ps=1.0, w_vs=1.0, max_points=130, objective=None):
    """fit (N,V,3); targets: list of N (verts, faces) or None; points / normals (N,S,3) or None -> host dict"""
    N, V = fit.shape[:2]
    obj = objective or eng.MeshObjective(V, faces, N, max_points)
    o = obj.surface(_t(fit), _targets(targets), None if points is None else _t(points), w_ps, w_vs, correspondences=True, gates=gates,
                    point_normals=None if normals is None else _t(normals))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype.itemsize == 4 else a


def _same_bits(a, b, what="", keys=None):
    for k in keys or a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _record(key, value):
    path = os.environ.get("SMALFIT_WRITE_SURFACE_GATE_MEASURED")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[key] = max(value, doc.get(key, 0.0))
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    return bool(path)


def _ratchet(key, device):
    """a measured device deviation stays within 3 x what tests/golden/hip_surface_gate_measured.json recorded"""
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    print("%-28s device %.3e   recorded %s" % (key, device, rec.get(key)))
    if _record(key, device):
        return
    assert key in rec, "tests/golden/hip_surface_gate_measured.json has no %s: run this file with " \
        "SMALFIT_WRITE_SURFACE_GATE_MEASURED=<path> on a GPU box and commit the result" % key
    assert device <= RATCHET * rec[key], (key, device, rec[key])


UNGATED_KEYS = ("losses", "rows", "dverts", "dtrans", "point_face", "point_bary", "point_residual", "vert_face", "vert_bary", "vert_residual")


def _soup_problem(F, S, seed, N=1, V=None):
    """N ribbons of V vertices (F + 2 unless given) against N soups of F faces, S points near each soup with random unit normals"""
    V = V or F + 2
    fit = np.stack([mc.ribbon(V, seed=seed + 7 * n)[0] for n in range(N)])
    faces = mc.ribbon(V, seed=0)[1]
    targets = [mc.soup(F, seed=seed + 100 + n) for n in range(N)]
    pts = np.stack([mc.points_near(targets[n][0], targets[n][1], S, seed=seed + 200 + n, sigma=0.05) for n in range(N)])
    nrm = np.random.RandomState(seed + 300).randn(N, S, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    return fit, faces, targets, pts, nrm


SOUP_GATES = dict(max_dist_point=0.2, max_dist_vert=0.3, min_cos_point=0.0, min_cos_vert=-0.2, reject_boundary=True)


# ---- against the float64 oracle ------------------------------------------------------------------------------------------------
def _check_direction(tag, q, u, sv, sf, want, face, kept, bary, resid, min_cos):
    L_ulp = mc.ulp_l(q, sv)
    delta = gc.DELTA_ULP * L_ulp
    share = want["flagged"].mean()
    assert share <= gc.FLAG_CAP, (tag, "the oracle flags too many", share)
    ok = ~want["flagged"]
    assert np.array_equal(kept.astype(bool)[ok], want["kept"][ok]), (tag, "kept masks", np.nonzero(kept.astype(bool) != want["kept"])[0][:5])
    assert np.array_equal(face >= 0, kept.astype(bool)), (tag, "face -1 exactly where dropped")
    assert (face < len(sf)).all(), tag
    assert gc.faces_equivalent(q, u, sv, sf, face, want, min_cos, delta)[ok].all(), (tag, "faces")
    both = ok & want["kept"]
    dev = 0.0
    if both.any():
        dev = float(np.abs(np.linalg.norm(resid.astype(np.float64), axis=1) - np.sqrt(want["d2"]))[both].max() / L_ulp)
    dropped = ~kept.astype(bool)
    assert (resid[dropped] == 0).all() and (bary[dropped] == 0).all(), (tag, "a dropped query is all zero")
    print("%-40s |r| %6.2f ulp(L)  kept %d/%d  flagged %d  faces other than the oracle's %d" %
          (tag, dev, kept.sum(), len(kept), want["flagged"].sum(), ((face != want["face"]) & ok).sum()))
    assert dev <= gc.DELTA_ULP, tag
    return dev


def _check_call(tag, o, fit, faces, targets, pts, nrm, gates, w_ps=1.0, w_vs=1.0):
    """everything one gated call returned against the float64 oracle, then the assembly from the returned correspondences"""
    N, V = fit.shape[:2]
    g = dict(gc.open_gates(), **gates)
    worst = 0.0
    want = np.zeros((N, V, 3))
    count = np.zeros((N, V))
    largest = 1e-300
    rows = np.zeros((N, 2))
    for n in range(N):
        L_ulp = mc.ulp_l(fit[n], targets[n][0]) if targets is not None else mc.ulp_l(fit[n], pts[n])
        w = gc.gated_term(fit[n:n + 1], faces, None if targets is None else targets[n:n + 1], None if pts is None else pts[n:n + 1],
                          None if nrm is None else nrm[n:n + 1], w_ps, w_vs, g, delta=gc.DELTA_ULP * L_ulp)
        if w_ps > 0:
            S = pts.shape[1]
            worst = max(worst, _check_direction("%s/mesh%d/points" % (tag, n), pts[n], None if nrm is None else nrm[n], fit[n], faces,
                                                w["point"][0], o["point_face"][n], o["point_kept"][n], o["point_bary"][n],
                                                o["point_residual"][n], g["min_cos_point"]))
            assert o["kept"][n, 0] == o["point_kept"][n].sum(), tag
            r = o["point_residual"][n].astype(np.float64)
            rows[n, 0] = (r * r).sum()
            corners = np.asarray(faces)[np.maximum(o["point_face"][n], 0)]
            for i in range(3):
                c = -w_ps * 2.0 / (N * S) * o["point_bary"][n][:, i:i + 1].astype(np.float64) * r
                np.add.at(want[n], corners[:, i], c)
                np.add.at(count[n], corners[:, i], 1)
                largest = max(largest, np.abs(c).max())
        else:
            assert o["kept"][n, 0] == 0
        if w_vs > 0:
            u = None
            if g["min_cos_vert"] > -1:
                u = o["vert_normals"][n]
                vn = gc.vertex_normals(fit[n], faces)
                # the unit normal of a float32 sum of deg cross products: (deg + 8) ulp x the cancellation of the sum
                nf = np.linalg.norm(gc.face_normals(fit[n], faces), axis=1)
                tot = np.zeros(V)
                np.add.at(tot, np.asarray(faces).ravel(), np.repeat(nf, 3))
                deg = np.bincount(np.asarray(faces).ravel(), minlength=V)
                s = np.zeros((V, 3))
                for k in range(3):
                    np.add.at(s, np.asarray(faces)[:, k], gc.face_normals(fit[n], faces))
                cancel = tot / np.maximum(np.linalg.norm(s, axis=1), 1e-300)
                err = np.abs(u - vn).max(1)
                bound = (deg + 8) * ULP * np.maximum(cancel, 1.0)
                print("%-40s vert_normals off by %.2e of the bound at worst (%.2e absolute)" % (tag, (err / bound).max(), err.max()))
                assert (err <= bound).all(), (tag, "vert_normals")
                _ratchet("vert_normals", float(err.max()))
            worst = max(worst, _check_direction("%s/mesh%d/verts" % (tag, n), fit[n], u, targets[n][0], targets[n][1], w["vert"][0],
                                                o["vert_face"][n], o["vert_kept"][n], o["vert_bary"][n], o["vert_residual"][n],
                                                g["min_cos_vert"]))
            assert o["kept"][n, 1] == o["vert_kept"][n].sum(), tag
            r = o["vert_residual"][n].astype(np.float64)
            rows[n, 1] = (r * r).sum()
            c = w_vs * 2.0 / (N * V) * r
            want[n] += c
            count[n] += 1
            largest = max(largest, np.abs(c).max())
        else:
            assert o["kept"][n, 1] == 0
    bound = (count + 2)[:, :, None] * ULP * largest
    err = np.abs(o["dverts"] - want)
    print("%-40s dverts off by %.2e of the bound at worst" % (tag, (err / bound).max()))
    assert (err <= bound).all(), tag
    for n in range(N):
        for d in (0, 1):
            cnt = int(o["kept"][n, d])
            assert abs(o["rows"][n, d] - rows[n, d]) <= (cnt + 16) * 2.0 ** -24 * rows[n, d] + 1e-45, (tag, n, d, o["rows"][n, d], rows[n, d])
    # the denominators stay N S and N V
    dev_rows = o["rows"].astype(np.float64)
    L_ps = dev_rows[:, 0].sum() / (N * pts.shape[1]) if w_ps > 0 else 0.0
    L_vs = dev_rows[:, 1].sum() / (N * V) if w_vs > 0 else 0.0
    rel = (N + 1) * 2.0 ** -24
    assert abs(o["losses"][0] - L_ps) <= rel * L_ps and abs(o["losses"][1] - L_vs) <= rel * L_vs, (tag, o["losses"], L_ps, L_vs)
    return worst


# ---- gates open ------------------------------------------------------------------------------------------------------------------
def _raw_gated(obj, tg, verts, pts, gate):
    """smalfit_mesh_surface_eval_gated with the required outputs only -> host dict; gate: a SurfaceGateArgs, None, or "plain" for
    smalfit_mesh_surface_eval"""
    lib = _lib.load()
    N, V, S = verts.shape[0], verts.shape[1], pts.shape[1]
    a = _lib.SurfaceTermArgs()
    a.num_meshes, a.w_point_surface, a.w_vert_surface = N, 1.0, 0.5
    a.verts, a.points, a.num_points = verts.data_ptr(), pts.data_ptr(), S
    out = dict(losses=torch.zeros(3, device=DEV), rows=torch.zeros(N, 2, device=DEV), dverts=torch.zeros(N, V, 3, device=DEV),
               dtrans=torch.zeros(N, 3, device=DEV))
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    if isinstance(gate, str):
        rc = _lib.resolve(lib, "smalfit_mesh_surface_eval")(obj.handle, tg.handle, eng._stream(), C.byref(a))
    else:
        out["kept"] = torch.full((N, 2), -7, dtype=torch.int32, device=DEV)
        if gate is not None:
            gate.kept = out["kept"].data_ptr()
        rc = _lib.resolve(lib, "smalfit_mesh_surface_eval_gated")(obj.handle, tg.handle, eng._stream(), C.byref(a),
                                                                  C.byref(gate) if gate is not None else None)
    assert rc == 0, lib.smalfit_last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_open_gates_are_the_ungated_call_bit_for_bit():
    fit, faces, targets, pts, nrm = _soup_problem(70, 70, seed=3, N=2)
    V = fit.shape[1]
    obj = eng.MeshObjective(V, faces, 2, 130)
    tg = _targets(targets)
    verts, dp = _t(fit), _t(pts)
    plain = _raw_gated(obj, tg, verts, dp, "plain")
    null = _raw_gated(obj, tg, verts, dp, None)
    off = _raw_gated(obj, tg, verts, dp, _lib.SurfaceGateArgs())
    assert np.abs(plain["dverts"]).max() > 0
    _same_bits(plain, null, "gate = NULL")
    _same_bits(plain, off, "every gate off", keys=plain)
    assert (null["kept"] == -7).all()                                 # (no block, nothing to write into)
    assert off["kept"].tolist() == [[70, V]] * 2
    wide = _lib.SurfaceGateArgs()                                     # switched on, never biting: the gated kernels, the same bits
    wide.max_dist_point = wide.max_dist_vert = 1e6
    on = _raw_gated(obj, tg, verts, dp, wide)
    _same_bits(plain, on, "gates that drop nothing", keys=plain)
    assert on["kept"].tolist() == [[70, V]] * 2
    # through the binding: the masks asked for, every gate off
    a = _surface(fit, faces, targets, pts, objective=obj)
    b = _surface(fit, faces, targets, pts, gates={}, objective=obj)
    _same_bits(a, b, "masks only", keys=UNGATED_KEYS)
    assert b["kept"].tolist() == [[70, V]] * 2 and (b["point_kept"] == 1).all() and (b["vert_kept"] == 1).all()
    assert "vert_normals" not in b


_PARAMS = ("betas", "global_rot", "joint_rot", "trans", "deform_verts")


def _three_steps(how):
    """three iterations of the default scheme with the surface term on through smalfit_fit3d_step_surface, smalfit_fit3d_step_gated
    with gate = NULL and with a block whose gates are all off"""
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = m3.fitter_problem(2, seed=6)
    stage = Stage(3, "default", fit, targets, lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=11,
                  loss_weights=dict(w_point_surface=1.0, w_vert_surface=1.0))
    e = fit._engine()
    plain, gated = _lib.resolve(e.lib, "smalfit_fit3d_step_surface"), _lib.resolve(e.lib, "smalfit_fit3d_step_gated")
    kept = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
    losses, terms = [], []
    for it in range(3):
        a = stage._step_args()
        for name in ("betas", "log_beta_scales") + _PARAMS[1:]:
            setattr(a, name, getattr(fit, name).data_ptr())
        a.weights = (C.c_float * 4)(*stage._weights())
        a.iteration, a.adam_t = it, it + 1
        sf = stage._surface_block()
        sf.w_point_surface, sf.w_vert_surface = 1.0, 1.0
        tg = stage.target_meshes._dev.handle
        if how == "surface":
            rc = plain(e.handle, stage._objective.handle, tg, eng._stream(), C.byref(a), C.byref(sf))
        elif how == "null":
            rc = gated(e.handle, stage._objective.handle, tg, eng._stream(), C.byref(a), C.byref(sf), None)
        else:
            g = _lib.SurfaceGateArgs()
            g.kept = kept.data_ptr()
            rc = gated(e.handle, stage._objective.handle, tg, eng._stream(), C.byref(a), C.byref(sf), C.byref(g))
        assert rc == 0, e.lib.smalfit_last_error()
        losses.append(stage._buffers["losses"].clone())
        terms.append(stage._step_losses.clone())
    torch.cuda.synchronize()
    state = {k: getattr(fit, k).detach().cpu().numpy().copy() for k in _PARAMS}
    for k, st in stage._adam.items():
        state["m_" + k], state["v_" + k] = st["m"].cpu().numpy().copy(), st["v"].cpu().numpy().copy()
    state["losses"], state["terms"] = torch.stack(losses).cpu().numpy(), torch.stack(terms).cpu().numpy()
    state["points"] = stage._points.cpu().numpy().copy()
    return state, kept.cpu().numpy(), stage.n_verts


def test_three_steps_with_open_gates_are_the_steps_of_before():
    base, _, _ = _three_steps("surface")
    assert np.abs(base["m_trans"]).max() > 0 and (base["terms"][:, 2] > 0).all()
    null, kept, _ = _three_steps("null")
    _same_bits(base, null, "gate = NULL")
    assert (kept == -7).all()
    off, kept, V = _three_steps("off")
    _same_bits(base, off, "every gate off")
    assert kept.tolist() == [[3000, V]] * 2


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_plate_with_a_hole_and_the_boundary_rule():
    tv, tf = gc.plate(4, hole=((1, 1),))
    over_hole = [(0.5, 0.5, 0.05), (0.45, 0.52, 0.03), (0.55, 0.4, 0.08)]
    over_plate = [(0.15, 0.2, 0.05), (0.8, 0.9, 0.02), (0.2, 0.85, 0.07)]
    fit = np.array(over_hole + over_plate, np.float32)[None]
    faces = np.array([(0, 1, 2), (3, 4, 5)], np.int32)
    for order in sc.CORNER_ORDERS:
        targets = [(tv, tf[:, list(order)])]
        o = _surface(fit, faces, targets, None, gates=dict(reject_boundary=True), w_ps=0.0)
        assert o["vert_kept"][0].tolist() == [0, 0, 0, 1, 1, 1], order
        assert o["kept"].tolist() == [[0, 3]] and (o["vert_face"][0][:3] == -1).all() and (o["vert_face"][0][3:] >= 0).all()
        assert (o["vert_residual"][0][:3] == 0).all() and (o["dverts"][0][:3] == 0).all()
        # over the plate: the plane, the residual (h / |n|^2) n is the height along z (a product and a quotient: 4 ulp)
        assert np.abs(o["vert_residual"][0][3:, 2] - fit[0, 3:, 2]).max() <= 4 * ULP * 0.1 and (o["vert_residual"][0][3:, :2] == 0).all()
        assert abs(o["rows"][0, 1] - (fit[0, 3:, 2].astype(np.float64) ** 2).sum()) <= 4 * 2.0 ** -24 * o["rows"][0, 1]
        free = _surface(fit, faces, targets, None, gates={}, w_ps=0.0)
        assert free["vert_kept"][0].tolist() == [1] * 6 and (np.abs(free["vert_residual"][0][:3]).max(1) > 0).all()


def _two_plates():
    """the near plate at z = 0.1 faces up, the far one at z = 0 faces down; -> (verts (1,V,3), faces, faces of the near plate)"""
    nv, nf = gc.plate(3, hole=(), z=0.1)
    fv, ff = gc.plate(3, hole=(), z=0.0, flip=True)
    return np.concatenate([nv, fv])[None], np.concatenate([nf, ff + len(nv)]).astype(np.int32), len(nf)


def test_two_plates_wound_in_opposite_ways():
    fit, faces, near = _two_plates()
    pts = np.array([[(0.4, 0.6, 0.11), (0.7, 0.2, 0.11)]], np.float32)
    nrm = np.array([[(0, 0, -1), (0, 0, -1)]], np.float32)            # agree with the far plate
    o = _surface(fit, faces, None, pts, nrm, gates=dict(min_cos_point=-1.0), w_vs=0.0)
    assert (o["point_face"][0] < near).all() and (o["point_face"][0] >= 0).all()
    d = np.float32(0.11) - np.float32(0.1)
    assert np.abs(o["point_residual"][0][:, 2] - d).max() <= 2 * ULP * 0.11
    o = _surface(fit, faces, None, pts, nrm, gates=dict(min_cos_point=0.5), w_vs=0.0)
    assert (o["point_face"][0] >= near).all() and o["kept"].tolist() == [[2, 0]]
    # the far plate's distance and nothing of the near one's: (h / |n|^2) n with n = (0, 0, -|n|) up to the rounding of its
    # cross product -- 4 ulp of the distance
    assert np.abs(o["point_residual"][0] - np.array([(0, 0, 0.11)] * 2)).max() <= 4 * ULP * 0.11
    assert abs(o["rows"][0, 0] - 2 * 0.11 ** 2) <= 4 * 2.0 ** -24 * o["rows"][0, 0]
    # the same normals turned round: the near plate, also under the test
    o = _surface(fit, faces, None, pts, -nrm, gates=dict(min_cos_point=0.5), w_vs=0.0)
    assert (o["point_face"][0] < near).all() and (o["point_face"][0] >= 0).all()


def test_no_compatible_face_drops_the_query():
    fit, faces, near = _two_plates()
    pts = np.array([[(0.4, 0.6, 0.11), (0.7, 0.2, 0.3), (0.1, 0.1, -0.2)]], np.float32)
    nrm = np.array([[(1, 0, 0), (0, 1, 0), (0.6, 0.8, 0)]], np.float32)   # perpendicular to both plates: 0 < c |c|
    o = _surface(fit, faces, None, pts, nrm, gates=dict(min_cos_point=0.5), w_vs=0.0)
    assert (o["point_face"] == -1).all() and (o["point_kept"] == 0).all() and o["kept"].tolist() == [[0, 0]]
    for k in ("point_residual", "point_bary", "rows", "losses", "dverts", "dtrans"):
        assert (o[k] == 0).all(), k
    # compatible exactly when c <= 0
    o = _surface(fit, faces, None, pts, nrm, gates=dict(min_cos_point=0.0), w_vs=0.0)
    assert (o["point_kept"] == 1).all()


def test_truncation_on_the_cube_in_closed_form():
    shifts = [np.array(s, np.float32) for s in ((0.25, 0.5, -0.125), (0.0625, 0.03125, 0.09375), (-0.5, 0.25, 1.5))]
    N = len(shifts)
    fit = np.repeat(mc.CUBE_VERTS[None], N, 0)
    targets = [(mc.CUBE_VERTS + s, mc.CUBE_FACES) for s in shifts]
    d = np.stack([mc.box_surface_dist(mc.CUBE_VERTS, s, s + 1.0) for s in shifts])
    vals = np.unique(d)
    gap = np.argmax(np.diff(vals))
    tau = float(np.float32(0.5 * (vals[gap] + vals[gap + 1])))
    assert np.abs(d - tau).min() > 1e-3 and (d < tau).any() and (d > tau).any()           # none is placed at tau
    o = _surface(fit, mc.CUBE_FACES, targets, None, gates=dict(max_dist_vert=tau), w_ps=0.0, max_points=8)
    print("tau %g distances %s" % (tau, np.round(d, 4).tolist()))
    assert np.array_equal(o["vert_kept"].astype(bool), d < tau)
    assert o["kept"][:, 1].tolist() == (d < tau).sum(1).tolist() and (o["kept"][:, 0] == 0).all()
    got = np.linalg.norm(o["vert_residual"].astype(np.float64), axis=2)
    assert np.abs(got - np.where(d < tau, d, 0.0)).max() <= gc.DELTA_ULP * mc.ulp_l(fit, *[t[0] for t in targets])
    L_vs = (np.where(d < tau, d, 0.0) ** 2).sum() / (N * 8)                                 # the denominator stays N V
    assert abs(o["losses"][1] - L_vs) <= 1e-6 * L_vs


# ---- branches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", (3, 63, 64, 65, 130))
def test_query_counts(Q):
    fit, faces, targets, pts, nrm = _soup_problem(70, Q, seed=Q, V=Q)
    o = _surface(fit, faces, targets, pts, nrm, gates=SOUP_GATES)
    _ratchet("residual_ulp", _check_call("Q=%d" % Q, o, fit, faces, targets, pts, nrm, SOUP_GATES))


@pytest.mark.parametrize("direction", ("verts", "points"))
@pytest.mark.parametrize("F0", (1, 2, 511, 512, 513, 1027))
def test_scanned_counts(F0, direction):
    if direction == "verts":
        fit, faces, targets, _, _ = _soup_problem(F0, 1, seed=F0, V=65)
        o = _surface(fit, faces, targets, None, gates=SOUP_GATES, w_ps=0.0)
        dev = _check_call("F=%d/verts" % F0, o, fit, faces, targets, None, None, SOUP_GATES, w_ps=0.0)
    else:
        point_gates = {k: v for k, v in SOUP_GATES.items() if k.endswith("_point")}     # (a vertex gate without targets is refused)
        fit, faces, _, _, _ = _soup_problem(5, 1, seed=F0, V=F0 + 2)
        pts = mc.points_near(fit[0], faces, 65, seed=F0 + 11, sigma=0.05)[None]       # (a draw under which the oracle alone flags at most 1 of 65)
        nrm = np.random.RandomState(F0).randn(1, 65, 3)
        nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
        o = _surface(fit, faces, None, pts, nrm, gates=point_gates, w_vs=0.0)
        dev = _check_call("F=%d/points" % F0, o, fit, faces, None, pts, nrm, point_gates, w_vs=0.0)
    _ratchet("residual_ulp", dev)


def test_one_slice_and_sixteen_slices_give_the_same_bits():
    """1027 scanned triangles: one mesh is scanned in 16 slices, a batch of 520 copies in one"""
    from tests import host_surface_term as hs
    fit, faces, targets, pts, nrm = _soup_problem(1027, 64, seed=9)
    V = fit.shape[1]
    assert hs.near_grid(V, 1027, 1)[2] == 16 and hs.near_grid(64, 1027, 1)[2] == 16
    N = 520
    assert hs.near_grid(V, 1027, N)[2] == 1 and hs.near_grid(64, 1027, N)[2] == 1
    one = _surface(fit, faces, targets, pts, nrm, gates=SOUP_GATES)
    many = _surface(np.repeat(fit, N, 0), faces, targets * N, np.repeat(pts, N, 0), np.repeat(nrm, N, 0), gates=SOUP_GATES)
    keys = ("rows", "kept", "point_face", "point_bary", "point_residual", "point_kept", "vert_face", "vert_bary", "vert_residual",
            "vert_kept", "vert_normals")
    for n in (0, N - 1):
        _same_bits({k: one[k][0] for k in keys}, {k: many[k][n] for k in keys}, "mesh %d" % n)
    assert 0 < one["kept"][0, 0] < 64 and 0 < one["kept"][0, 1] < V


def test_ragged_batch_equals_the_one_mesh_calls():
    counts = (1, 513, 7)
    fit, faces, _, _, nrm = _soup_problem(40, 70, seed=21, N=3)
    targets = [mc.soup(F, seed=400 + F) for F in counts]
    pts = np.stack([mc.points_near(fit[n], faces, 70, seed=50 + n, sigma=0.05) for n in range(3)])
    obj = eng.MeshObjective(fit.shape[1], faces, 3, 130)
    whole = _surface(fit, faces, targets, pts, nrm, gates=SOUP_GATES, objective=obj)
    keys = ("rows", "kept", "point_face", "point_bary", "point_residual", "point_kept", "vert_face", "vert_bary", "vert_residual",
            "vert_kept", "vert_normals")
    for n in range(3):
        one = _surface(fit[n:n + 1], faces, targets[n:n + 1], pts[n:n + 1], nrm[n:n + 1], gates=SOUP_GATES, objective=obj)
        _same_bits({k: one[k][0] for k in keys}, {k: whole[k][n] for k in keys}, "mesh %d" % n)
    assert (whole["vert_face"][0] <= 0).all() and whole["vert_face"][1].max() > 7


# ---- against the oracle on the stand-in pieces ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {seed: gc.oracle_scene(seed) for seed in gc.ORACLE_SEEDS}


@pytest.mark.parametrize("gates", gc.EACH_GATE, ids=["+".join(sorted(g)) for g in gc.EACH_GATE])
def test_each_gate_alone_and_all_together_against_the_oracle(scenes, gates):
    worst = 0.0
    for seed, s in scenes.items():
        o = _surface(s["fit"], s["faces"], s["targets"], s["points"], s["point_normals"], gates=gates)
        worst = max(worst, _check_call("piece %d" % seed, o, s["fit"], s["faces"], s["targets"], s["points"], s["point_normals"], gates))
    _ratchet("residual_ulp", worst)


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def test_sampler_with_normals():
    pieces = [gc.remove_patch(*gc.standin_piece(300, seed), 0.2, seed) for seed in (0, 1)]
    pieces.append(gc.fan_of_three())
    tg = _targets(pieces)
    for it in (0, 5):
        plain = tg.sample(130, 77, it).cpu().numpy()
        p, n = tg.sample_normals(130, 77, it)
        p, n = p.cpu().numpy(), n.cpu().numpy()
        assert np.array_equal(_bits(plain), _bits(p))
        for m, (tv, tf) in enumerate(pieces):
            near = sc.nearest(p[m], tv, tf)
            assert np.sqrt(near["d2"]).max() <= gc.DELTA_ULP * mc.ulp_l(tv)
            want = gc.face_unit_normals(tv, tf)
            # the face a point lies on is its nearest; on an edge two faces share, either's normal
            err = np.abs(n[m] - want[near["face"]]).max(1)
            edge = err > 8 * 2.0 ** -24
            if edge.any():
                alt = np.abs(want[None] - n[m][edge][:, None]).max(2).min(1)
                assert (alt <= 8 * 2.0 ** -24).all()
            assert edge.mean() <= 0.05
            assert np.abs(np.linalg.norm(n[m].astype(np.float64), axis=1) - 1).max() <= 4 * 2.0 ** -24
    assert np.array_equal(hg.face_unit_normals(*pieces[2]).shape, (3, 3))


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
STEP_GATES = dict(max_dist_point=0.2, max_dist_vert=0.2, min_cos_point=0.2, min_cos_vert=0.2, reject_boundary=True)


def _partial_targets(targets, share=1.0 / 3.0):
    from smalify_amd.fitter_3d import TargetMeshes
    return TargetMeshes(targets.verts, [gc.remove_patch(v, f, share, 3 + n)[1] for n, (v, f) in enumerate(zip(targets.verts, targets.faces))])


def test_fused_and_unfused_gated_steps_agree():
    from smalify_amd.fitter_3d import Stage
    results = []
    for fused in (True, False):
        md, fit, targets = m3.fitter_problem(2, seed=6)
        stage = Stage(4, "default", fit, _partial_targets(targets), lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=11,
                      loss_weights=dict(w_point_surface=2.0, w_vert_surface=1.5), surface_gates=STEP_GATES)
        assert stage.gates_on and stage.last_surface_kept is None
        losses, terms, kept = [], [], []
        for it in range(4):
            losses.append((stage.step(it) if fused else stage.step_unfused(it)).clone())
            terms.append(stage.last_surface_terms.clone())
            kept.append(stage.last_surface_kept.clone())
        torch.cuda.synchronize()
        results.append((torch.stack(losses).cpu().numpy(), torch.stack(terms).cpu().numpy(), torch.stack(kept).cpu().numpy(),
                        {k: getattr(fit, k).detach().cpu().numpy().copy() for k in _PARAMS}, stage.last_points.cpu().numpy().copy(),
                        stage.n_verts))
    (la, ta, ka, pa, xa, V), (lb, tb, kb, pb, xb, _) = results
    print("fused %s\nunfused %s\nkept %s" % (la, lb, ka[-1].tolist()))
    assert np.array_equal(xa, xb)
    assert ka.shape == (4, 2, 2) and (ka[:, :, 0] < 3000).all() and (ka[:, :, 1] < V).all() and (ka > 0).all()       # the gates bite
    assert np.array_equal(ka[0], kb[0])
    assert np.abs(ka.astype(np.int64) - kb).max() <= 3                       # (parameters 1e-6 apart may move a query across a gate)
    assert (ta[:, 2] > 0).all() and np.abs(ta - tb).max() <= 1e-6 * np.abs(tb).max()
    assert np.abs(la - lb).max() <= 1e-6 * np.abs(lb).max()                  # the bar of the fused-versus-unfused fit3d test
    for k in pa:
        assert m3.rel(pa[k], pb[k]) < 1e-6 or np.array_equal(pa[k], pb[k]), k


DESCENT_GATES = dict(max_dist_point=0.75, max_dist_vert=0.75, reject_boundary=True)


def _numpy_descent(dtype, lr, steps, fit0, faces, targets, pts):
    v = fit0.astype(dtype).copy()
    m, s = np.zeros_like(v), np.zeros_like(v)
    b1, b2, eps = dtype(0.9), dtype(0.999), dtype(1e-8)
    terms = []
    for t in range(1, steps + 1):
        o = gc.gated_term(v, faces, [(targets[0][0].astype(dtype), targets[0][1])], pts.astype(dtype), None, 1.0, 1.0, DESCENT_GATES, dtype=dtype)
        terms.append(float(o["term"]))
        g = o["dverts"]
        m = b1 * m + (dtype(1) - b1) * g
        s = b2 * s + (dtype(1) - b2) * g * g
        step = dtype(lr) / dtype(1 - 0.9 ** t)
        v = v - step * m / (np.sqrt(s) / dtype(np.sqrt(1 - 0.999 ** t)) + eps)
    return np.array(terms), o["kept"]


def test_descent_on_a_partial_target_follows_the_float64_loop():
    """the cube towards its shifted copy with a third of the copy's faces (its two x sides) removed.  A hard gate makes the loss
    jump when a query changes sides; the learning rate is the first under which the float64 loop decreases all the way"""
    steps = 30
    fit0 = mc.CUBE_VERTS[None].copy()
    targets = [(mc.CUBE_VERTS + mc.CUBE_SHIFT, mc.CUBE_FACES[4:])]
    pts = mc.points_near(targets[0][0], targets[0][1], 64, seed=4, sigma=0.0)[None]
    lr = next((c for c in (0.05, 0.02, 0.01, 0.005)
               if (np.diff(_numpy_descent(np.float64, c, steps, fit0, mc.CUBE_FACES, targets, pts)[0]) < 0).all()), None)
    assert lr is not None, "no candidate learning rate makes the float64 loop decrease"
    t64, k64 = _numpy_descent(np.float64, lr, steps, fit0, mc.CUBE_FACES, targets, pts)
    t32, _ = _numpy_descent(np.float32, lr, steps, fit0, mc.CUBE_FACES, targets, pts)
    assert 0 < k64[0, 1] < 8
    obj = eng.MeshObjective(8, mc.CUBE_FACES, 1, 64)
    tg = _targets(targets)
    v, dp = _t(fit0), _t(pts)
    m, s = torch.zeros_like(v), torch.zeros_like(v)
    got = []
    for t in range(1, steps + 1):
        o = obj.surface(v, tg, dp, 1.0, 1.0, gates=DESCENT_GATES)
        got.append(o["losses"][2].clone())
        eng.adam_step(v, o["dverts"], m, s, lr, t, beta1=0.9, beta2=0.999, eps=1e-8)
    torch.cuda.synchronize()
    got = torch.stack(got).cpu().numpy().astype(np.float64)
    device, yardstick = float(np.abs(got - t64).max()), float(np.abs(t32 - t64).max())
    print("lr %g kept %s\nfloat64 %s\ndevice  %s\ndevice off %.3e, float32 yardstick off %.3e" % (lr, k64.tolist(), t64, got, device, yardstick))
    assert np.isfinite(device) and device <= sc.WHOLE_GRADIENT_FACTOR * yardstick
    _ratchet("descent", device)
    assert got[-1] < got[0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    fit, faces, targets, pts, nrm = _soup_problem(40, 70, seed=2, N=2)
    N, V, S = 2, fit.shape[1], 70
    obj = eng.MeshObjective(V, faces, sc.MAX_MESHES, sc.MAX_POINTS)
    tg = _targets(targets)
    verts, dp, dn = _t(fit), _t(pts), _t(nrm)
    lib = _lib.load()
    fn = _lib.resolve(lib, "smalfit_mesh_surface_eval_gated")
    f32 = dict(losses=(3,), rows=(N, 2), dverts=(N, V, 3), dtrans=(N, 3), point_bary=(N, S, 3), vert_bary=(N, V, 3),
               point_residual=(N, S, 3), vert_residual=(N, V, 3))
    out = {k: torch.full(s, -7.0, device=DEV) for k, s in f32.items()}
    out["point_face"] = torch.full((N, S), -7, dtype=torch.int32, device=DEV)
    out["vert_face"] = torch.full((N, V), -7, dtype=torch.int32, device=DEV)
    gout = dict(kept=torch.full((N, 2), -7, dtype=torch.int32, device=DEV), point_kept=torch.full((N, S), 7, dtype=torch.uint8, device=DEV),
                vert_kept=torch.full((N, V), 7, dtype=torch.uint8, device=DEV), vert_normals=torch.full((N, V, 3), -7.0, device=DEV))

    def blocks():
        a = sc.valid_args(N=N, S=S)
        a.verts, a.points = verts.data_ptr(), dp.data_ptr()
        for k, v in out.items():
            setattr(a, k, v.data_ptr())
        a.step_total = None
        g = gc.valid_gate()
        g.point_normals = dn.data_ptr()
        for k, v in gout.items():
            setattr(g, k, v.data_ptr())
        return a, g
    tried = 0
    for name, cg, ct, facts, text in gc.REFUSALS:
        if facts.get("step"):
            continue
        a, g = blocks()
        cg(g)
        ct(a)
        t = None if facts.get("targets") is False else tg
        assert fn(obj.handle, t.handle if t else None, eng._stream(), C.byref(a), C.byref(g)) != 0, name
        assert lib.smalfit_last_error().decode() == "smalfit_mesh_surface_eval_gated: " + text, name
        tried += 1
    assert tried >= 13
    # a fault of the term's own block is named as before, under the gated call's name
    a, g = blocks()
    a.losses = None
    assert fn(obj.handle, tg.handle, eng._stream(), C.byref(a), C.byref(g)) != 0
    assert lib.smalfit_last_error().decode() == "smalfit_mesh_surface_eval_gated: losses missing"
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == -7).all(), k
    for k, v in gout.items():
        assert (v == (7 if v.dtype == torch.uint8 else -7)).all(), k
    a, g = blocks()
    assert fn(obj.handle, tg.handle, eng._stream(), C.byref(a), C.byref(g)) == 0, lib.smalfit_last_error()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert not (v == -7).all(), k
    for k, v in gout.items():
        assert not (v == (7 if v.dtype == torch.uint8 else -7)).any(), k
    with pytest.raises(KeyError, match="unknown surface gate"):
        obj.surface(verts, tg, dp, 1.0, 1.0, gates=dict(max_dist=1.0))


def test_stage_refuses_unknown_gates_and_reports_kept():
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = m3.fitter_problem(2, seed=6)
    with pytest.raises(KeyError, match="unknown surface gate"):
        Stage(2, "init", fit, targets, surface_gates=dict(min_cos=0.5))
    stage = Stage(2, "init", fit, _partial_targets(targets), loss_weights=dict(w_vert_surface=1.0), lr=0.05, seed=2,
                  surface_gates=dict(reject_boundary=True))
    stage.step(0)
    kept = stage.last_surface_kept.cpu().numpy()
    assert kept.shape == (2, 2) and (kept[:, 0] == 0).all() and (kept[:, 1] > 0).all() and (kept[:, 1] < stage.n_verts).all()

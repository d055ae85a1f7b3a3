"""GPU tests of the 3D mesh objective and the fused fit3d step at every branch of their kernels.

The cases of tests/mesh3d_forms.py (checked by tests/test_mesh3d_forms_cpu.py to reach every chamfer form of both roles,
the 64/256 grid edges and every topology branch) run through eng.MeshObjective against the float64 reference of the same
module, mesh by mesh.  Designed ties must resolve to the lowest index.  Some results must hold bit for bit: a repeated
call, a larger capacity, the other meshes of a batch when one mesh changes, a chamfer-off call after a chamfer-on call
with more points, and a negative weight against a zero one.  The sampler runs on zero-area, one-face and ragged target
meshes against the host shim.  smalfit_fit3d_step runs every scheme against the oracle loop and the component calls, and
1 to 41 shape parameters with caller-supplied points: after Adam's first step the first moments hold (1 - beta1) g, so
they expose the fused step's gradients.

Bars (those of tests/test_gpu_fit3d.py): loss terms 2e-5 relative, d/d verts 2e-4 rel-L2 per mesh, d/d trans
2e-4 max|g| + 1e-7, LBS-level gradients 5e-4 rel-L2, stage-loop loss 1e-4 per iteration and parameters 1e-4, sampler
1e-6.  The worst value of each is printed at the end of the module."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mesh3d_oracle as mo  # noqa: E402
from oracle import smal_oracle as so  # noqa: E402
from smalify_amd import _lib  # noqa: E402
from smalify_amd import engine as eng  # noqa: E402
from tests import host_shim  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402
from tests import mesh3d_forms as mf  # noqa: E402

TERMS = ("chamfer", "edge", "normal", "laplacian")
WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print("\nworst measured:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def run(obj, c, weights=None, lbs=None, points=None):
    o = obj.eval(dev(c.lbs if lbs is None else lbs), dev(c.trans), dev(c.deform),
                 dev(c.points if points is None else points), c.weights if weights is None else weights)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def check_against_reference(c, o, ref):
    assert np.array_equal(o["verts"], c.verts)                  # same float32 additions as the compose kernel
    wc = max(c.weights[0], 0.0)
    for i, k in enumerate(TERMS):
        want = ref["terms"][i] if (i > 0 or wc > 0) else 0.0
        if want == 0.0:
            assert o["losses"][i] == 0.0, (k, o["losses"][i])   # P = 0, or chamfer off
        else:
            err = abs(o["losses"][i] - want) / abs(want)
            note("loss term (rel)", err)
            assert err <= 2e-5, (k, o["losses"][i], want)
    err = abs(o["losses"][4] - ref["total"]) / abs(ref["total"])
    note("loss total (rel)", err)
    assert err <= 2e-5
    for n in range(c.N):                                         # one wrong mesh cannot hide in the batch
        err = mc.rel(o["dverts"][n], ref["dverts"][n])
        note("dverts (rel-L2 per mesh)", err)
        assert err < 2e-4, ("mesh", n, err)
    gt = ref["dtrans"]
    err = np.abs(o["dtrans"] - gt).max()
    note("dtrans (fraction of its bar)", err / (2e-4 * np.abs(gt).max() + 1e-7))
    assert err <= 2e-4 * np.abs(gt).max() + 1e-7


# ---- objective against the float64 reference -----------------------------------------------------------------------
@pytest.mark.parametrize("name", mf.case_names())
def test_objective_matches_reference(name):
    c = mf.case(name)
    obj = eng.MeshObjective(c.V, c.faces, mf.MAX_MESHES, c.S)
    assert (obj.num_edges, obj.num_face_pairs) == (len(mo.unique_edges(c.faces)), c.P)
    o = run(obj, c)
    ref = mf.reference(o["verts"], c.points, c.faces, c.weights)
    check_against_reference(c, o, ref)
    for t in c.ties:                                              # designed ties: the lowest index wins
        rows = t.rows()
        err = mc.rel(o["dverts"][t.mesh, rows], ref["dverts"][t.mesh, rows])
        note("tied rows of dverts (rel-L2)", err)
        assert err < 2e-4, (t, err)


# ---- bit-exact invariants --------------------------------------------------------------------------------------------
def same_bits(a, b, keys=("losses", "verts", "dverts", "dtrans")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["ribbon_V1029_S5_N5", "ribbon_V257_S2048_N1", "hand_strip_fin_S63_N5"])
def test_repeated_call_has_the_same_bits(name):
    c = mf.case(name)
    obj = eng.MeshObjective(c.V, c.faces, mf.MAX_MESHES, c.S)
    same_bits(run(obj, c), run(obj, c))


@pytest.mark.parametrize("name", ["ribbon_V6_S3_N1", "ribbon_V65_S1024_N3", "ribbon_V255_S1025_N1",
                                  "ribbon_V257_S2048_N1", "hand_tetra_S4_N3"])
def test_capacity_changes_no_bit(name):
    c = mf.case(name)
    tight = eng.MeshObjective(c.V, c.faces, c.N, c.S)
    roomy = eng.MeshObjective(c.V, c.faces, c.N + 4, c.S + 1000)
    same_bits(run(tight, c), run(roomy, c))


@pytest.mark.parametrize("name,k", [("ribbon_V1029_S5_N5", 2), ("ribbon_V65_S1024_N3", 0), ("hand_fan_S65_N3", 1)])
def test_changing_one_mesh_leaves_the_others(name, k):
    c = mf.case(name)
    obj = eng.MeshObjective(c.V, c.faces, mf.MAX_MESHES, c.S)
    a = run(obj, c)
    lbs, pts = c.lbs.copy(), c.points.copy()
    lbs[k] += np.float32(0.125)
    pts[k] = pts[k, ::-1] * np.float32(1.5)
    b = run(obj, c, lbs=lbs, points=pts)
    others = [n for n in range(c.N) if n != k]
    assert not np.array_equal(a["dverts"][k], b["dverts"][k])
    for key in ("verts", "dverts", "dtrans"):
        assert np.array_equal(a[key][others], b[key][others]), key


@pytest.mark.parametrize("first,second", [("ribbon_V1024_S2053_N1", (0.0, 0.7, 0.3, 0.2)),
                                          ("ribbon_V65_S1024_N3", (-1.0, 0.7, 0.3, 0.2))])
def test_chamfer_off_after_chamfer_on_equals_a_fresh_objective(first, second):
    """the chamfer-off branch zeroes the chamfer gradient itself and the reduce ignores the stale chamfer partials"""
    c = mf.case(first)
    used = eng.MeshObjective(c.V, c.faces, mf.MAX_MESHES, c.S)
    run(used, c)
    fresh = eng.MeshObjective(c.V, c.faces, mf.MAX_MESHES, c.S)
    small = c.points[:, :3]
    a, b = run(used, c, weights=second, points=small), run(fresh, c, weights=second, points=small)
    same_bits(a, b)
    assert a["losses"][0] == 0.0
    ref = mf.reference(a["verts"], None, c.faces, second)
    check_against_reference(mf.Case(c.name, c.faces, c.lbs, c.trans, c.deform, small, second), a, ref)


@pytest.mark.parametrize("name,neg,zero", [("ribbon_V256_S1027_N3", (1.0, -0.7, 0.3, 0.2), (1.0, 0.0, 0.3, 0.2)),
                                           ("hand_book_S64_N1", (1.0, 0.7, -0.3, -0.2), (1.0, 0.7, 0.0, 0.0)),
                                           ("hand_collinear_S2_N1", (-2.0, 0.7, 0.3, 0.2), (0.0, 0.7, 0.3, 0.2))])
def test_negative_weight_equals_zero_weight(name, neg, zero):
    c = mf.case(name)
    obj = eng.MeshObjective(c.V, c.faces, mf.MAX_MESHES, c.S)
    same_bits(run(obj, c, weights=neg), run(obj, c, weights=zero))


# ---- sampler -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    return host_shim.mesh3d()


def sampler_meshes():
    """interior zero-area faces, trailing zero-area faces, one face, the stand-in -> (verts list, faces list, zero-area)"""
    md = mc.synthetic.synthetic_model(seed=0, shape_family_id=1)
    sv, sf = np.asarray(md.v_template, np.float32), np.asarray(md.faces, np.int32)
    rv, rf = mf.ribbon(40, seed=3)
    inner = rf.copy()
    inner[[4, 5, 17]] = [[0, 1, 1], [2, 2, 2], [3, 3, 5]]                    # repeated corners: zero area
    trail = np.concatenate([rf[:20], [[7, 7, 8], [9, 9, 9], [10, 10, 11]]]).astype(np.int32)
    one_v = np.array([[0.0, 0, 0], [1, 0, 0], [0.25, 0.75, 0.5]], np.float32)
    verts = [rv, rv, one_v, sv]
    faces = [inner, trail, np.array([[0, 1, 2]], np.int32), sf]
    zero = [[4, 5, 17], [20, 21, 22], [], []]
    return verts, faces, zero


@pytest.mark.parametrize("S", (1, 255, 256, 257, 3000))
def test_sampler_on_ragged_and_degenerate_targets(shim, S):
    verts, faces, zero = sampler_meshes()
    t = eng.MeshTargets(verts, faces)
    seed, it = (3 << 32) | 17, 5
    p = t.sample(S, seed=seed, iteration=it)
    torch.cuda.synchronize()
    got = p.cpu().numpy()
    assert got.shape == (4, S, 3)
    for n in range(4):
        v = np.ascontiguousarray(verts[n], np.float32)
        f = np.ascontiguousarray(faces[n], np.int32)
        want, chosen = np.zeros((S, 3), np.float32), np.zeros(S, np.int32)
        assert shim.hm3_sample(len(v), v.ctypes.data_as(C.c_void_p), len(f), f.ctypes.data_as(C.c_void_p), S,
                               C.c_ulonglong(seed), it, n, want.ctypes.data_as(C.c_void_p),
                               chosen.ctypes.data_as(C.c_void_p)) == 0
        assert not np.isin(chosen, zero[n]).any()
        err = np.abs(got[n] - want).max()
        note("sampler (abs)", err)
        assert err < 1e-6, (n, err)
    assert torch.equal(p, t.sample(S, seed=seed, iteration=it))


# ---- fused step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,lr,custom_lrs,iters", [("init", 0.05, None, 5), ("shape", 0.02, {"betas": 0.03}, 5),
                                                        ("pose", 0.01, {"joint_rot": 0.005}, 6)])
def test_stage_loop_follows_the_oracle_in_every_scheme(scheme, lr, custom_lrs, iters):
    trace, fit, params, names = mc.stage_loop_against_oracle(scheme, lr, custom_lrs, iters)
    note("stage loop loss (rel)", max(trace))
    assert max(trace) < 1e-4, trace
    for k in names:
        err = mc.rel(getattr(fit, k).detach().cpu().numpy(), params[k].numpy())
        note("stage loop parameters (rel-L2)", err)
        assert err < 1e-4, (k, err)
    for k in params:
        if k not in names:
            assert np.array_equal(getattr(fit, k).detach().cpu().numpy(), params[k].float().numpy()), k


@pytest.mark.parametrize("scheme,lr,iters", [("default", 0.02, 6), ("init", 0.05, 6), ("shape", 0.02, 6), ("pose", 0.02, 3),
                                             ("deform", 2e-4, 6)])
def test_fused_step_equals_the_component_calls_in_every_scheme(scheme, lr, iters):
    """as test_gpu_fit3d.py::test_fused_step_equals_the_component_calls.  The first step's gradients agree to the last
    bit or two and the losses of every step to 1e-7, but in the pose scheme Adam turns such a last-bit difference at a
    near-zero joint-rotation gradient into a step of ~lr: six steps part joint_rot by 1.6e-4 rel-L2, so it runs three (as
    the 57-mesh case of test_gpu_frame_counts.py does)"""
    (la, pa, xa), (lb, pb, xb) = mc.fused_and_component_runs(3, iters=iters, scheme=scheme, lr=lr)
    assert np.array_equal(xa, xb)
    err = np.abs(la - lb).max() / np.abs(lb).max()
    note("fused vs component loss (rel)", err)
    assert err <= 1e-6
    for k in pa:
        assert mc.rel(pa[k], pb[k]) < 1e-6 or np.array_equal(pa[k], pb[k]), (scheme, k)


_ENV = {}


def fit3d_env():
    """a fitter of 5 meshes (engine capacity 5) and an objective for 400 points, shared by the num_betas cases"""
    if not _ENV:
        md, fit, _ = mc.fitter_problem(5, seed=2)
        _ENV.update(md=md, fit=fit, om=so.OracleModel(md), obj=eng.MeshObjective(md.num_verts, md.faces, 5, 400))
    return _ENV


@pytest.mark.parametrize("nb", (1, 20, 21, 41))
@pytest.mark.parametrize("N", (1, 5))
def test_fused_step_gradients_at_every_beta_count(nb, N):
    """smalfit_fit3d_step with nb of the model's shape directions, caller-supplied points, points_out and verts_out;
    every parameter trained, Adam's first step: m = (1 - beta1) g"""
    env = fit3d_env()
    md, fit, om, obj = env["md"], env["fit"], env["om"], env["obj"]
    e = fit._engine()
    V, S = md.num_verts, 400
    rs = np.random.RandomState(100 * nb + N)
    host = dict(betas=0.5 * rs.randn(N, nb), log_beta_scales=0.05 * rs.randn(N, 6), global_rot=0.2 * rs.randn(N, 3),
                joint_rot=0.1 * rs.randn(N, 34, 3), trans=0.05 * rs.randn(N, 3), deform_verts=0.003 * rs.randn(N, V, 3))
    host = {k: v.astype(np.float32) for k, v in host.items()}
    pts = mc.objective_problem(N, S, seed=nb + N)[4]
    d = {k: dev(v) for k, v in host.items()}
    lr = 1e-3
    trained = ("betas", "global_rot", "joint_rot", "trans", "deform_verts")
    m = {k: torch.zeros_like(d[k]) for k in trained}
    v = {k: torch.zeros_like(d[k]) for k in trained}
    points, points_out = dev(pts), torch.full((N, S, 3), -7.0, device="cuda")
    losses, verts_out = torch.zeros(5, device="cuda"), torch.zeros((N, V, 3), device="cuda")
    weights = (1.0, 0.8, 0.02, 0.1)
    a = _lib.Fit3dArgs()
    a.num_meshes, a.num_betas, a.num_points = N, nb, S
    for k in host:
        setattr(a, k, d[k].data_ptr())
    for k in trained:
        setattr(a, "lr_" + k, lr)
        setattr(a, "m_" + k, m[k].data_ptr())
        setattr(a, "v_" + k, v[k].data_ptr())
    a.beta1, a.beta2, a.eps, a.adam_t = 0.9, 0.999, 1e-8, 1
    a.weights = (C.c_float * 4)(*weights)
    a.points, a.seed, a.iteration = points.data_ptr(), 0, 0
    a.points_out, a.losses, a.verts_out = points_out.data_ptr(), losses.data_ptr(), verts_out.data_ptr()
    assert e.lib.smalfit_fit3d_step(e.handle, obj.handle, None, eng._stream(), C.byref(a)) == 0, e.lib.smalfit_last_error()
    torch.cuda.synchronize()
    assert torch.equal(points_out, points)
    # oracle: SMAL3DFitter.forward with shapedirs[:nb], the objective, autograd in float64
    leaf = {k: torch.from_numpy(x).double().requires_grad_(k in trained) for k, x in host.items()}
    vo = mo.fitter_verts(om, leaf)
    total, _ = mo.objective(vo, torch.from_numpy(pts).double(), mo.unique_edges(md.faces), mo.face_pairs(md.faces),
                            dict(zip(mc.WEIGHT_KEYS, weights)))
    grads = dict(zip(trained, torch.autograd.grad(total, [leaf[k] for k in trained])))
    vo = vo.detach().numpy()
    got_v = verts_out.cpu().numpy()
    for n in range(N):
        err = mc.rel(got_v[n], vo[n])
        note("fused verts_out (rel-L2 per mesh)", err)
        assert err < 2e-5, (n, err)
    total = float(total.detach())
    err = abs(float(losses[4]) - total) / abs(total)
    note("fused loss total (rel)", err)
    assert err <= 2e-5
    one_minus_b1 = np.float32(1.0) - np.float32(0.9)
    for k in trained:
        g = m[k].cpu().numpy().astype(np.float64) / float(one_minus_b1)
        want = grads[k].numpy()
        if k == "trans":
            err = np.abs(g - want).max()
            note("fused dtrans (fraction of its bar)", err / (2e-4 * np.abs(want).max() + 1e-7))
            assert err <= 2e-4 * np.abs(want).max() + 1e-7, (k, err)
        elif k == "deform_verts":
            for n in range(N):
                err = mc.rel(g[n], want[n])
                note("fused dverts (rel-L2 per mesh)", err)
                assert err < 2e-4, (k, n, err)
        else:
            err = mc.rel(g, want)
            note("fused LBS gradients (rel-L2)", err)
            assert err < 5e-4, (k, err)
        # the parameter took the Adam step of its own moments
        mm, vv = m[k].cpu().numpy().astype(np.float64), v[k].cpu().numpy().astype(np.float64)
        step = lr / (1 - 0.9) * mm / (np.sqrt(vv) / np.sqrt(1 - 0.999) + 1e-8)
        assert np.abs(d[k].cpu().numpy() - (host[k] - step)).max() <= 1e-6, k

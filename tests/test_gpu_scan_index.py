"""The scan index on the device (mesh3d_surface_near_grid_kernel / mesh3d_surface_dist_grid_kernel of kernels_mesh3d.inc behind
smalfit_mesh_targets_build_index) (-m gpu).  Two handles of the same targets, one indexed and one not: every output of every call
is equal BIT FOR BIT -- there is no tolerance in this file and nothing under tests/golden/ belongs to it.

  surface   MeshObjective.surface with correspondences, V in 3, 4, 5, 65, 130 (queries per block, the last partial block) against
            targets of 1, 2, 7, 513 and 1280 faces, the query placements of tests/test_scan_index_cpu.py (NaN and +-inf among them);
            plain, each gate alone, all gates, and the robust block; a ragged batch of 1, 513 and 7 faces = the one-mesh calls
  score     MeshObjective.score: vert_dist, sums, within; a mesh against itself identically 0
  the step  three Stage.step calls in each spelling (plain, gated, partial, robust) against a posed stand-in target subdivided
            twice (124 k faces): parameters, Adam state and losses; scan_index=False = a Stage built without the argument
  books     index_stats = the shim's; build_index twice; refusals leave the handle usable; destroy / create rounds
  CLI       optimise.py --scan_index and the YAML key write the .npz contents of a run without, byte for byte
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib                        # noqa: E402
from smalify_amd import engine as eng               # noqa: E402
from tests import host_scan_index as hsi            # noqa: E402
from tests import mesh3d_cases as m3                # noqa: E402
from tests import mesh_score_cases as mc            # noqa: E402
from tests import scan_index_cases as sic           # noqa: E402

DEV = "cuda"


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


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same_bits(a, b, what=""):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, k)


def _handles(meshes, scale=0.0):
    """the same targets twice: -> (linear, indexed)"""
    v, f = [m[0] for m in meshes], [m[1] for m in meshes]
    return eng.MeshTargets(v, f), eng.MeshTargets(v, f).build_index(scale)


def _scale(F):
    return sic.PAIR_SCALE if F == 2 else 0.0


def _queries(mesh, V, F, seed=0):
    ix = hsi.Index(mesh[0], mesh[1], _scale(F))
    lo, hi = ix.box()
    return sic.placements(mesh[0], mesh[1], lo, hi, ix.cell_edge, V, seed)


GATES = {"plain": None,
         "compatibility": dict(min_cos_vert=0.0),
         "truncation": dict(max_dist_vert=0.3),
         "boundary": dict(reject_boundary=True),
         "all": dict(min_cos_vert=0.2, max_dist_vert=0.3, reject_boundary=True)}
ROBUST = dict(sigma_surface_vert=0.25)

_TARGETS = {}


def _target_handles(F):
    if F not in _TARGETS:
        mesh = sic.target(F)
        _TARGETS[F] = (mesh,) + _handles([mesh], _scale(F))
    return _TARGETS[F]


@pytest.mark.parametrize("V", sic.QUERY_COUNTS)
@pytest.mark.parametrize("F", sic.TARGET_FACES)
def test_surface_term_bit_for_bit(F, V):
    mesh, lin, idx = _target_handles(F)
    assert idx.has_index and not lin.has_index
    fit = _queries(mesh, V, F, seed=V)[None]
    obj = eng.MeshObjective(V, mc.ribbon(V, 1)[1], 1, 8)
    for name, gates in GATES.items():
        for robust in (None, ROBUST):
            a = _host(obj.surface(_t(fit), lin, None, 0.0, 1.0, correspondences=True, gates=gates, robust=robust))
            b = _host(obj.surface(_t(fit), idx, None, 0.0, 1.0, correspondences=True, gates=gates, robust=robust))
            _same_bits(a, b, (F, V, name, robust is not None))
            for k in ("vert_face", "vert_bary", "vert_residual", "losses", "rows", "dverts", "dtrans"):
                assert k in a
            if gates is not None:
                assert "vert_kept" in a and "kept" in a
            if robust is not None:
                assert "vert_weights" in a and "surface_weight_sums" in a
    if V >= 65 and F >= 7:
        plain = _host(obj.surface(_t(fit), idx, None, 0.0, 1.0, correspondences=True, gates=GATES["truncation"]))
        assert 0 < plain["kept"][0, 1] < V                                    # the truncation drops some and keeps some


def test_ragged_batch_is_the_one_mesh_calls():
    meshes = [sic.target(F) for F in (1, 513, 7)]
    V = 65
    fit = np.stack([_queries(m, V, len(m[1]), seed=3 + i) for i, m in enumerate(meshes)])
    faces = mc.ribbon(V, 1)[1]
    lin, idx = _handles(meshes)
    obj = eng.MeshObjective(V, faces, 3, 8)
    for gates in (None, GATES["all"]):
        a = _host(obj.surface(_t(fit), lin, None, 0.0, 1.0, correspondences=True, gates=gates, robust=ROBUST))
        b = _host(obj.surface(_t(fit), idx, None, 0.0, 1.0, correspondences=True, gates=gates, robust=ROBUST))
        _same_bits(a, b, "ragged")
        for n, m in enumerate(meshes):
            one = _host(obj.surface(_t(fit[n:n + 1]), eng.MeshTargets([m[0]], [m[1]]).build_index(), None, 0.0, 1.0,
                                    correspondences=True, gates=gates, robust=ROBUST))
            for k in ("vert_face", "vert_bary", "vert_residual", "rows", "vert_weights"):
                assert one[k][0].tobytes() == b[k][n].tobytes(), (n, k)
    st = idx.index_stats()
    assert [s["dims"] for s in st][0] == (1, 1, 1) and len(st) == 3


@pytest.mark.parametrize("F", sic.TARGET_FACES)
def test_score_bit_for_bit(F):
    mesh, lin, idx = _target_handles(F)
    for V in sic.QUERY_COUNTS:
        fit = _queries(mesh, V, F, seed=10 + V)
        if V >= 16:
            fit = fit[:-3].copy()                                              # (the score's sums of NaN rows compare as bits too, but keep them readable)
            fit = np.concatenate([fit, fit[:3]])
        obj = eng.MeshObjective(V, mc.ribbon(V, 1)[1], 1, 8)
        thr = (0.01, 0.1, 1.0)
        a = _host(obj.score(_t(fit[None]), lin, thresholds=thr))
        b = _host(obj.score(_t(fit[None]), idx, thresholds=thr))
        _same_bits(a, b, (F, V))
        assert set(a) >= {"vert_dist", "sums", "within"}


def test_score_of_a_mesh_against_itself_is_zero():
    v, f = mc.ribbon(130, 5)
    lin, idx = _handles([(v, f)])
    obj = eng.MeshObjective(130, f, 1, 8)
    o = _host(obj.score(_t(v[None]), idx, thresholds=(1e-6,)))
    assert (o["vert_dist"] == 0).all() and (o["sums"][0, 0] == 0).all() and o["within"][0, 0, 0] == 130
    _same_bits(o, _host(obj.score(_t(v[None]), lin, thresholds=(1e-6,))))


# ---- the step ----------------------------------------------------------------------------------------------------------------
SPELLINGS = {"plain": dict(loss_weights={"w_vert_surface": 1.0}),
             "gated": dict(loss_weights={"w_vert_surface": 1.0, "w_point_surface": 0.5},
                           surface_gates=dict(max_dist_vert=0.2, min_cos_vert=0.0, reject_boundary=True, max_dist_point=0.3)),
             "partial": dict(loss_weights={"w_vert_surface": 1.0},
                             surface_gates=dict(max_dist_vert=0.05),
                             chamfer_gates=dict(max_dist_point=0.3, max_dist_vert=0.3, min_cos_vert=0.0)),
             "robust": dict(loss_weights={"w_vert_surface": 1.0, "w_point_surface": 1.0}, surface_gates=dict(max_dist_vert=0.2),
                            robust=dict(sigma_surface_vert=0.1, sigma_surface_point=0.1, sigma_chamfer_point=0.2))}
_PARAMS = ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")


@pytest.fixture(scope="module")
def dense_targets():
    """a posed stand-in subdivided twice, 124 k faces: (linear TargetMeshes, TargetMeshes that Stage(scan_index=True) indexes)"""
    from smalify_amd.fitter_3d import TargetMeshes
    from smalify_amd.fitter_3d.utils import subdivide_mesh
    md = m3.synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf = m3.target_meshes_from_smal(md, 1, seed=7)
    v, f = subdivide_mesh(tv[0], tf, 2)
    assert len(f) == 7774 * 16
    return md, TargetMeshes([v], [f]), TargetMeshes([v], [f])


def _three_steps(md, targets, spelling, **kw):
    from smalify_amd.fitter_3d import SMAL3DFitter, Stage
    fit = SMAL3DFitter(batch_size=1, shape_family=-1, model_data=md, smal_data=m3.synthetic_smal_data())
    stage = Stage(3, "default", fit, targets, lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=4, **SPELLINGS[spelling], **kw)
    out = {}
    for it in range(3):
        out["total%d" % it] = stage.step(it).detach().clone().reshape(1)
        out["terms%d" % it] = stage.last_terms.detach().clone()
        out["surface%d" % it] = stage.last_surface_terms.detach().clone()
    for k in _PARAMS:
        out[k] = getattr(fit, k).detach().clone()
    for name, st in stage._adam.items():
        out["m_" + name], out["v_" + name] = st["m"].clone(), st["v"].clone()
    if stage.last_surface_kept is not None:
        out["kept"] = stage.last_surface_kept.clone()
    return _host(out), stage


@pytest.mark.parametrize("spelling", sorted(SPELLINGS))
def test_three_steps_bit_for_bit(dense_targets, spelling):
    md, lin, idx = dense_targets
    a, stage_a = _three_steps(md, lin, spelling, scan_index=False)
    b, stage_b = _three_steps(md, idx, spelling, scan_index=True)
    assert idx.has_index and not lin.has_index and stage_b.scan_index and not stage_a.scan_index
    _same_bits(a, b, spelling)
    assert np.isfinite(a["total2"]).all() and a["surface0"][1] > 0
    if spelling == "plain":
        c, _ = _three_steps(md, lin, spelling)
        _same_bits(a, c, "no argument")
    if spelling != "plain":
        assert 0 < a["kept"][0, 1] <= md.num_verts


def test_stage_metrics_with_the_index(dense_targets):
    md, lin, idx = dense_targets
    out = []
    for targets in (lin, idx.build_index()):
        _, stage = _three_steps(md, targets, "plain")
        m = stage.metrics(num_points=500, thresholds=(0.01, 0.05))
        out.append(m)
    assert repr(out[0]) == repr(out[1]) and "hausdorff" in repr(out[0])


# ---- bookkeeping -------------------------------------------------------------------------------------------------------------
def test_index_stats_are_the_shims():
    for F in sic.TARGET_FACES:
        mesh, lin, idx = _target_handles(F)
        assert idx.index_stats() == [hsi.Index(mesh[0], mesh[1], _scale(F)).stats()]
        with pytest.raises(eng.SmalfitError, match="the targets have no scan index"):
            lin.index_stats()
    meshes = [sic.oversize_target(), sic.flat_target()]
    t = eng.MeshTargets([m[0] for m in meshes], [m[1] for m in meshes]).build_index(1.5)
    assert t.index_stats() == [hsi.Index(m[0], m[1], 1.5).stats() for m in meshes]
    assert t.index_stats()[0]["oversize"] == 1 and t.index_stats()[1]["dims"][2] == 1


def test_build_twice_refusals_and_destroy_rounds():
    mesh = sic.target(513)
    V = 65
    fit = _t(_queries(mesh, V, 513, seed=2)[None])
    obj = eng.MeshObjective(V, mc.ribbon(V, 1)[1], 1, 8)
    lin, idx = _handles([mesh])
    want = _host(obj.surface(fit, lin, None, 0.0, 1.0, correspondences=True))
    stats = idx.index_stats()
    idx.build_index()                                                          # twice: the same grid again
    assert idx.index_stats() == stats
    _same_bits(want, _host(obj.surface(fit, idx, None, 0.0, 1.0, correspondences=True)))
    idx.build_index(3.0)                                                       # another grid, the same results
    assert idx.index_stats() != stats
    _same_bits(want, _host(obj.surface(fit, idx, None, 0.0, 1.0, correspondences=True)))
    # refusals leave the handle as it was
    kept = idx.index_stats()
    with pytest.raises(eng.SmalfitError, match="cell_scale must be finite and >= 0"):
        idx.build_index(-1.0)
    a = _lib.ScanIndexArgs()
    a.struct_size = 4
    assert _lib.resolve(idx.lib, "smalfit_mesh_targets_build_index")(idx.handle, C.byref(a)) == 1
    assert b"struct_size" in idx.lib.smalfit_last_error()
    assert _lib.resolve(idx.lib, "smalfit_mesh_targets_build_index")(idx.handle, None) == 1
    assert idx.index_stats() == kept
    _same_bits(want, _host(obj.surface(fit, idx, None, 0.0, 1.0, correspondences=True)))
    # a non-finite vertex no face uses: the targets are accepted, the index is refused, the linear scan still serves
    v = np.concatenate([mesh[0], np.float32([[np.nan, 0, 0]])])
    bad = eng.MeshTargets([v], [mesh[1]])
    with pytest.raises(eng.SmalfitError, match="scan index needs finite target vertices"):
        bad.build_index()
    assert not bad.has_index
    _same_bits(want, _host(obj.surface(fit, bad, None, 0.0, 1.0, correspondences=True)))
    # destroy with an index, create again: nothing a second round trips over
    for _ in range(3):
        t = eng.MeshTargets([mesh[0]], [mesh[1]]).build_index()
        _same_bits(want, _host(obj.surface(fit, t, None, 0.0, 1.0, correspondences=True)))
        del t


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_optimise_writes_the_same_bytes_with_the_index(tmp_path):
    from smalify_amd.fitter_3d import optimise
    md = m3.synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf = m3.target_meshes_from_smal(md, 1, seed=9)
    mesh_dir = tmp_path / "meshes"
    mesh_dir.mkdir()
    with open(mesh_dir / "m0.obj", "w") as fh:
        for p in tv[0] * 3.0 + 0.5:
            fh.write("v %.7f %.7f %.7f\n" % tuple(p))
        for f in tf:
            fh.write("f %d %d %d\n" % tuple(f + 1))
    stage = ("stages:\n  Stage0:\n    scheme: 'default'\n    nits: 5\n    lr: 0.02\n"
             "    loss_weights:\n      w_vert_surface: 1.0\n      w_point_surface: 0.5\n"
             "    surface_gates:\n      max_dist_vert: 0.3\n")
    got = {}
    for name, flag, key in (("without", [], ""), ("flag", ["--scan_index"], ""), ("yaml", [], "  scan_index: true\n")):
        cfg = tmp_path / (name + ".yaml")
        cfg.write_text(stage + "args:\n  results_dir: %s\n  shape_family_id: -1\n%s" % (tmp_path / name, key))
        args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--yaml_src", str(cfg), "--no_plots"] + flag)
        mgr = optimise.main(args, model_data=md, smal_data=m3.synthetic_smal_data())
        assert mgr.stages[0].target_meshes.has_index == (name != "without")
        z = np.load(tmp_path / name / "Stage0.npz", allow_pickle=True)
        got[name] = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}     # (the archive itself carries the time)
    assert got["without"] == got["flag"] == got["yaml"] and len(got["without"]["verts"][2]) == 3889 * 3 * 4

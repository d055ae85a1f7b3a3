"""Every call on the 3-D handle after every other on ONE MeshObjective (-m gpu): the mesh acts of tests/entry_order_cases.py.

fitter_3d shares one smalfit_mesh_objective among all stages of a fitter, and StageManager.run(metrics=True) alternates the step
spellings and smalfit_mesh_score on it.  The handle keeps work buffers (the composed vertices, first-candidate keys, the chamfer
gradient, per-mesh rows) and no cache: whatever ran before, a call gives the bits it gives on a brand-new objective.

  a  fresh    every act twice, each on a brand-new objective: bit for bit; one result is fresh[B]
  b  order    for every B, on one long-lived objective shared by the module: for every A in table order, A then B; B == fresh[B] byte
              for byte on every output
  c  stages   a SMAL3DFitter runs three Stages in a row on its one objective -- plain, partial + robust, plain -- with
              Stage.metrics() between them; the third stage's parameters, Adam state and losses equal those of a second fitter that
              starts from the first one's parameters at that point and runs the same stage as its first work on a new objective

V = 130 (three blocks of queries, the last partial) against targets of 7 and 513 faces and a ragged batch of 1 / 513 / 7, linear
and indexed targets, N = 1 and 3, S at the objective's capacity and at 1.  There is no tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import entry_order_cases as oc      # noqa: E402
from tests import mesh3d_cases as m3           # noqa: E402

_FRESH = {}
_SHARED = {}
_PARAMS = ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def _handles():
    if "handles" not in _SHARED:
        _SHARED["handles"] = oc.MeshHandles()
    return _SHARED["handles"]


def _differing(a, b):
    if set(a) != set(b):
        return "keys %s" % sorted(set(a) ^ set(b))
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return k
    return None


def _fresh(name):
    if name not in _FRESH:
        results = [oc.MESH_ACTS[name].fn(oc.new_objective(), _handles()) for _ in range(2)]
        k = _differing(results[0], results[1])
        assert k is None, "act %r is not reproducible on fresh objectives: %s" % (name, k)
        _FRESH[name] = results[0]
    return _FRESH[name]


@pytest.mark.parametrize("name", oc.MESH_NAMES)
def test_a_fresh_objectives_agree(name):
    r = _fresh(name)
    for k, v in r.items():
        if v.dtype == np.float32:
            assert not (v == np.float32(oc.SENTINEL)).any(), (name, k)
    if name.startswith("eval") and "chamfer off" not in name:
        assert r["losses"][0] > 0 and np.isfinite(r["losses"]).all()
    if name.startswith("surface"):
        assert np.isfinite(r["losses"]).all() and np.isfinite(r["dverts"]).all()
    if name.startswith("surface plain"):
        assert r["losses"][0] > 0 and r["losses"][1] > 0 and np.abs(r["dverts"]).max() > 0
    if "kept" in r and name.startswith("surface") and ("truncation" in name or "all gates" in name) and "S=70" in name:
        V, S = oc.MESH_V, oc.MESH_POINTS
        assert (r["kept"][:, 1] < V).any() or (r["kept"][:, 0] < S).any(), (name, r["kept"])      # a gate that gates


@pytest.mark.parametrize("name", oc.MESH_NAMES)
def test_b_after_any_act_the_bits_are_a_fresh_objectives(name):
    if "objective" not in _SHARED:
        _SHARED["objective"], _SHARED["history"] = oc.new_objective(), []
    obj, history, handles = _SHARED["objective"], _SHARED["history"], _handles()
    ref = _fresh(name)
    for after in oc.MESH_NAMES:
        oc.MESH_ACTS[after].fn(obj, handles)
        history.append(after)
        got = oc.MESH_ACTS[name].fn(obj, handles)
        history.append(name)
        k = _differing(got, ref)
        assert k is None, "%r after %r differs from a fresh objective's in %s\nlast acts: %s" % (name, after, k, history[-5:])


# ---- c. the fused step through three stages on the fitter's one objective -------------------------------------------------------
SPELLINGS = (dict(),
             dict(loss_weights={"w_vert_surface": 1.0, "w_point_surface": 1.0}, surface_gates=dict(max_dist_vert=0.2),
                  chamfer_gates=dict(max_dist_point=0.3, max_dist_vert=0.3, min_cos_vert=0.0),
                  robust=dict(sigma_surface_vert=0.1, sigma_surface_point=0.1, sigma_chamfer_point=0.2)),
             dict())
ITERATIONS = 3


def _stage(fit, targets, index):
    from smalify_amd.fitter_3d import Stage
    return Stage(ITERATIONS, "default", fit, targets, lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=4,
                 iteration_offset=index * ITERATIONS, **SPELLINGS[index])


def _run_stage(stage):
    out = {}
    for it in range(ITERATIONS):
        out["total%d" % it] = stage.step(it).detach().clone().reshape(1)
        out["terms%d" % it] = stage.last_terms.detach().clone()
    for k in _PARAMS:
        out[k] = getattr(stage.smal_3d_fitter, k).detach().clone()
    for name, st in stage._adam.items():
        out["m_" + name], out["v_" + name] = st["m"].clone(), st["v"].clone()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_c_a_third_stage_on_the_shared_objective_is_a_first_stage_on_a_new_one():
    md, first, targets = m3.fitter_problem(2, seed=6)
    thresholds = (0.01, 0.05)
    history = []
    for index in (0, 1):
        stage = _stage(first, targets, index)
        history.append(_run_stage(stage))
        stage.metrics(thresholds=thresholds, num_points=500)
    objective = first._mesh_objective
    start = {k: getattr(first, k).detach().clone() for k in _PARAMS}
    third = _run_stage(_stage(first, targets, 2))
    assert first._mesh_objective is objective                      # all of it ran on the one handle

    _, second, _ = m3.fitter_problem(2, seed=6)
    with torch.no_grad():
        for k in _PARAMS:
            getattr(second, k).copy_(start[k])
    alone = _run_stage(_stage(second, targets, 2))
    assert second._mesh_objective is not objective
    k = _differing(third, alone)
    assert k is None, "the third stage differs from the same stage on a new objective in %s" % k
    # the stages did what their spellings say: the fit moved, and the middle stage's total carries more than the four terms
    assert not np.array_equal(history[0]["betas"], history[1]["betas"]) and not np.array_equal(third["betas"], history[1]["betas"])
    assert np.isfinite(third["total2"]).all() and history[1]["total0"][0] != history[1]["terms0"][4]

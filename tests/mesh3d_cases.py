"""Problems and parity cases of the 3D mesh-fitting objective, shared by tests/test_mesh3d_cpu.py (host shim vs oracle),
tests/test_gpu_fit3d.py (HIP through the C-ABI vs oracle) and __graft_entry__/tools.  Nothing here asserts.
Oracle = oracle/mesh3d_oracle.py (test infrastructure)."""
from __future__ import annotations

import numpy as np
import torch

from oracle import mesh3d_oracle as mo
from oracle import smal_oracle as so
from smalify_amd import synthetic

WEIGHT_KEYS = ("w_chamfer", "w_edge", "w_normal", "w_laplacian")


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def objective_problem(N, S, seed, deform=True):
    """N noisy copies of the synthetic SMAL template against S target points from a perturbed, rescaled surface"""
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    rs = np.random.RandomState(seed)
    V = md.num_verts
    base = np.asarray(md.v_template, np.float32)
    lbs = (base[None] + 0.01 * rs.randn(N, V, 3)).astype(np.float32)
    trans = (0.05 * rs.randn(N, 3)).astype(np.float32)
    dfm = (0.003 * rs.randn(N, V, 3)).astype(np.float32) if deform else None
    idx = rs.randint(0, V, size=(N, S))
    pts = (1.1 * base[idx] + 0.02 * rs.randn(N, S, 3) + 0.03).astype(np.float32)
    return md, lbs, trans, dfm, pts


def oracle_objective(verts32, pts32, faces, weights):
    """oracle value and gradient at the float32 vertices -> (total, {term: value}, d total / d verts)"""
    edges, pairs = mo.unique_edges(faces), mo.face_pairs(faces)
    tv = torch.from_numpy(np.asarray(verts32)).double().requires_grad_(True)
    total, terms = mo.objective(tv, torch.from_numpy(np.asarray(pts32)).double(), edges, pairs, dict(zip(WEIGHT_KEYS, weights)))
    total.backward()
    return float(total.detach()), {k: float(v.detach()) for k, v in terms.items()}, tv.grad.numpy()


def target_meshes_from_smal(md, N, seed):
    """N posed + reshaped SMAL meshes (oracle LBS), centred and scaled like fitter_3d/utils.py:237-241 -> verts list, faces"""
    rs = np.random.RandomState(seed)
    om = so.OracleModel(md)
    beta = torch.from_numpy(0.5 * rs.randn(N, 20))
    theta = torch.from_numpy(0.12 * rs.randn(N, 35, 3))
    ls = torch.from_numpy(0.05 * rs.randn(N, 6))
    verts = so.smal_forward(om, beta, theta, ls)[0].numpy()
    out = []
    for v in verts:
        v = v - v.mean(0)
        out.append((v / np.abs(v).max()).astype(np.float32))
    return out, np.asarray(md.faces, np.int64)


def synthetic_smal_data(seed=0):
    return synthetic.synthetic_smal_dicts(seed=seed)[1]


def fitter_problem(N, seed=0):
    """SMAL3DFitter of N meshes (stand-in model, 20 betas) + N target meshes from the oracle's LBS -> (md, fitter, targets)"""
    from smalify_amd.fitter_3d import SMAL3DFitter, TargetMeshes
    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf = target_meshes_from_smal(md, N, seed=seed + 1)
    fit = SMAL3DFitter(batch_size=N, shape_family=-1, model_data=md, smal_data=synthetic_smal_data())
    return md, fit, TargetMeshes(tv, [tf] * N)


DEFAULT_CUSTOM_LRS = {"joint_rot": 0.004, "betas": 0.03}


def fused_and_component_runs(N, seed=6, iters=6, scheme="default", lr=0.02, custom_lrs=DEFAULT_CUSTOM_LRS):
    """`iters` Stage iterations of N meshes as one smalfit_fit3d_step each (Stage.step) and as the component calls
    (Stage.step_unfused), each from a fresh fitter -> [(losses (iters,), {parameter: values}, last sampled points)] x 2"""
    from smalify_amd.fitter_3d import Stage
    results = []
    for fused in (True, False):
        md, fit, targets = fitter_problem(N, seed=seed)
        stage = Stage(iters, scheme, fit, targets, lr=lr, custom_lrs=custom_lrs, seed=11)
        losses = []
        for it in range(iters):
            losses.append((stage.step(it) if fused else stage.step_unfused(it)).clone())
        torch.cuda.synchronize()
        results.append((torch.stack(losses).cpu().numpy(), {k: getattr(fit, k).detach().cpu().numpy().copy() for k in
                                                           ("betas", "global_rot", "joint_rot", "trans", "deform_verts")},
                        stage.last_points.cpu().numpy().copy()))
    return results


def stage_loop_against_oracle(scheme, lr, custom_lrs, iters, N=2, seed=0):
    """Stage.step x iters against the oracle: same sampled points, loss + autograd through the LBS oracle, torch-style
    Adam with betas (0.9, 0.999) and per-parameter learning rates -> (per-iteration relative loss errors, fitter,
    oracle parameters after the loop, names of the trained parameters)"""
    from smalify_amd.fitter_3d import SMALParamGroup, Stage
    md, fit, targets = fitter_problem(N, seed)
    weights = dict(w_chamfer=1.0, w_edge=0.8, w_normal=0.02, w_laplacian=0.01)
    stage = Stage(iters, scheme, fit, targets, loss_weights=weights, lr=lr, custom_lrs=custom_lrs, seed=5)
    om = so.OracleModel(md)
    edges, pairs = mo.unique_edges(md.faces), mo.face_pairs(md.faces)
    names = [n for n in SMALParamGroup.param_map[scheme] if n != "log_beta_scales"]      # frozen in the reference
    params = {k: getattr(fit, k).detach().cpu().double() for k in
              ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")}
    adam = mo.Adam({n: (custom_lrs or {}).get(n, lr) for n in names})
    trace = []
    for it in range(iters):
        loss = stage.step(it)
        pts = stage.last_points.cpu().double()
        leaf = {k: v.clone().requires_grad_(k in names) for k, v in params.items()}
        total, _ = mo.objective(mo.fitter_verts(om, leaf), pts, edges, pairs, weights)
        grads = dict(zip(names, torch.autograd.grad(total, [leaf[n] for n in names])))
        adam.step(params, grads)
        trace.append(abs(float(loss) - float(total.detach())) / abs(float(total.detach())))
    return trace, fit, params, names

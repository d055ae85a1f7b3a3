#!/usr/bin/env python3
"""Developer measurement (GPU box) of the 3D mesh-fitting loop: iterations/s of Stage.step for a
batch of N target meshes, "default" scheme (trainer.py:115), all four loss terms, 3000 target points per mesh, and the
share of each of the five C-ABI calls of a step (torch events on the launch stream, separate short run).

    python tools/fit3d_bench.py [--meshes 1 8 32] [--iters 300] [--surface [--gates]] [--chamfer-gates] [--robust]

    python tools/fit3d_bench.py --surface --target-subdiv K --scan-index [--gates] [--cell-scale X] [--near-warmup W]

Prints one JSON line per batch size.  --target-subdiv K subdivides every stand-in target K times by midpoint subdivision (7774 x
4^K faces: a dense scan).  --scan-index (with --surface) makes two handles of the same targets, one with the scan index and one
without, and times `--iters` steps on each in alternating runs of one process, three runs each, at two states: "far" = the
first steps of the stage from the template pose, "near" = the steps after --near-warmup steps of the same fit; one JSON line
per (batch size, state, handle) with the index's statistics and its build time beside the rates.  --surface adds the point-to-surface term both ways (w_point_surface = w_vert_surface = 1:
every step is smalfit_fit3d_step_surface) and two fields to the line; without it the run and the line are those of before.
--gates (with --surface) switches every gate of that term on (GATES below: every step is smalfit_fit3d_step_gated) and adds the
kept counts of the last step.  --chamfer-gates, alone or with the others, switches every gate of the chamfer term on (every step is
smalfit_fit3d_step_partial) and adds its kept counts.  --robust, alone or with the others, switches the Geman-McClure kernel on for
every data term that runs (ROBUST below: every step is smalfit_fit3d_step_robust) and adds the weight sums of the last step.  Synthetic SMAL-topology model and targets (posed copies of it), as bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def targets_for(md, N, seed):
    """posed copies of the template: cheap stand-ins with the SMAL face list (no oracle involved)"""
    rs = np.random.RandomState(seed)
    base = np.asarray(md.v_template, np.float32)
    out = []
    for _ in range(N):
        a = 0.3 * rs.randn()
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
        v = (base * (1.0 + 0.1 * rs.randn(3))) @ R.T + 0.01 * rs.randn(*base.shape)
        v = v - v.mean(0)
        out.append((v / np.abs(v).max()).astype(np.float32))
    return out


# every gate on, none of them tight on a complete target: the cost of the gated kernels, not of what they drop
GATES = dict(max_dist_point=0.5, max_dist_vert=0.5, min_cos_point=0.0, min_cos_vert=0.0, reject_boundary=True)


# every scale on, wide against a complete target (the targets fill [-1, 1]): the cost of the robust kernels, not of what they let go
ROBUST = dict(sigma_chamfer_point=0.5, sigma_chamfer_vert=0.5, sigma_surface_point=0.5, sigma_surface_vert=0.5)


def scan_index_runs(args, md, smal_data, N):
    """the indexed and the linear handle, alternating: -> the JSON lines of one batch size"""
    import torch
    from smalify_amd.fitter_3d import SMAL3DFitter, Stage, TargetMeshes
    from smalify_amd.fitter_3d.utils import subdivide_mesh
    meshes = [subdivide_mesh(v, np.asarray(md.faces), args.target_subdiv) for v in targets_for(md, N, seed=N)]
    handles = {"linear": TargetMeshes([m[0] for m in meshes], [m[1] for m in meshes]),
               "index": TargetMeshes([m[0] for m in meshes], [m[1] for m in meshes])}
    t0 = time.perf_counter()
    handles["index"].build_index(args.cell_scale)
    build_ms = 1e3 * (time.perf_counter() - t0)
    stats = handles["index"].index_stats()
    weights = {"w_point_surface": 1.0, "w_vert_surface": 1.0}
    times = {(st, h): [] for st in ("far", "near") for h in handles}
    final = {}
    for st, warm in (("far", 0), ("near", args.near_warmup)):
        for rep in range(3):
            for h, targets in handles.items():
                fit = SMAL3DFitter(batch_size=N, shape_family=-1, model_data=md, smal_data=smal_data)
                # (the warm-up runs on the indexed handle: the fit it reaches is the same to the bit, and it gets there sooner)
                stage = Stage(warm + args.iters, "default", fit, handles["index"] if warm else targets, lr=0.01,
                              custom_lrs={"joint_rot": 0.005}, loss_weights=weights, surface_gates=GATES if args.gates else None)
                for i in range(warm):
                    stage.step(i)
                stage.target_meshes = targets
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    stage.step(warm + i)
                torch.cuda.synchronize()
                times[(st, h)].append(1e3 * (time.perf_counter() - t0) / args.iters)
                final[(st, h)] = float(stage.last_terms[4])
                del stage, fit
    lines = []
    for (st, h), ms in times.items():
        line = {"meshes": N, "target_subdiv": args.target_subdiv, "target_faces": int(len(meshes[0][1])), "state": st, "handle": h,
                "iters": args.iters, "ms_per_iteration": ms, "final_total_loss": final[(st, h)], "gates": bool(args.gates)}
        if h == "index":
            line.update(cell_scale=args.cell_scale, build_ms=build_ms, index_stats=stats[0],
                        index_bytes=int(sum(x["bytes"] for x in stats)))
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--surface", action="store_true", help="add the point-to-surface term both ways to every step")
    ap.add_argument("--gates", action="store_true", help="with --surface: gate the term (truncation, compatibility, boundary)")
    ap.add_argument("--chamfer-gates", action="store_true", help="gate the chamfer term (truncation, compatibility, boundary)")
    ap.add_argument("--robust", action="store_true", help="the Geman-McClure kernel on every data term that runs")
    ap.add_argument("--target-subdiv", type=int, default=0, help="subdivide every target this many times (7774 x 4^K faces)")
    ap.add_argument("--scan-index", action="store_true", help="with --surface: the indexed handle against the linear one, alternating")
    ap.add_argument("--cell-scale", type=float, default=0.0, help="with --scan-index: the grid's cell scale (0: the library's own)")
    ap.add_argument("--near-warmup", type=int, default=300, help="with --scan-index: steps of the fit before the near state is timed")
    args = ap.parse_args()
    if args.gates and not args.surface:
        ap.error("--gates needs --surface")
    if args.scan_index and not args.surface:
        ap.error("--scan-index needs --surface")
    import torch
    from smalify_amd import synthetic
    from smalify_amd.fitter_3d import SMAL3DFitter, Stage, TargetMeshes

    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    smal_data = synthetic.synthetic_smal_dicts(seed=0)[1]
    from smalify_amd.fitter_3d.utils import subdivide_mesh
    for N in args.meshes:
        if args.scan_index:
            for line in scan_index_runs(args, md, smal_data, N):
                print(json.dumps(line), flush=True)
            continue
        fit = SMAL3DFitter(batch_size=N, shape_family=-1, model_data=md, smal_data=smal_data)
        tv = targets_for(md, N, seed=N)
        if args.target_subdiv:
            sub = [subdivide_mesh(v, np.asarray(md.faces), args.target_subdiv) for v in tv]
            targets = TargetMeshes([m[0] for m in sub], [m[1] for m in sub])
        else:
            targets = TargetMeshes(tv, [np.asarray(md.faces)] * N)
        weights = {"w_point_surface": 1.0, "w_vert_surface": 1.0} if args.surface else None
        stage = Stage(args.iters, "default", fit, targets, lr=0.01, custom_lrs={"joint_rot": 0.005}, loss_weights=weights,
                      surface_gates=GATES if args.gates else None, chamfer_gates=GATES if args.chamfer_gates else None,
                      **(dict(robust=ROBUST) if args.robust else {}))
        for i in range(10):
            stage.step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            stage.step(10 + i)
        t_issue = time.perf_counter() - t0          # host time to enqueue everything (the GPU runs behind)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # share of the calls of one step
        e = fit._engine()
        betas, ls, theta = fit.betas.detach().contiguous(), fit.log_beta_scales.detach().contiguous(), fit._pack_theta()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        acc = np.zeros(4)
        reps = 50
        for r in range(reps):
            ev[0].record()
            lbs = e.lbs_forward(betas, theta, ls, want_Rs=False, want_v_shaped=False)[0]
            ev[1].record()
            pts = targets.sample(3000, 0, r)
            ev[2].record()
            o = stage._objective.eval(lbs, fit.trans.detach(), fit.deform_verts.detach(), pts, stage._weights())
            ev[3].record()
            e.lbs_backward(betas, theta, ls, o["dverts"], None)
            ev[4].record()
            torch.cuda.synchronize()
            acc += [ev[k].elapsed_time(ev[k + 1]) for k in range(4)]
        sec = dict(zip(("lbs_forward", "sample", "objective", "lbs_backward"), (acc / reps).tolist()))
        V, S = md.num_verts, 3000
        line = {"meshes": N, "iterations_per_s": args.iters / dt, "ms_per_iteration": 1e3 * dt / args.iters,
                "mesh_iterations_per_s": N * args.iters / dt,
                "host_issue_ms_per_iteration": 1e3 * t_issue / args.iters, "section_ms": sec,
                "chamfer_point_pairs_per_s": 2.0 * N * V * S / (sec["objective"] * 1e-3),
                "final_total_loss": float(stage.last_terms[4])}
        if args.surface:
            line["surface"] = True
            line["final_surface_terms"] = [float(x) for x in stage.last_surface_terms]
        if args.gates:
            line["gates"] = GATES
            line["final_surface_kept"] = stage.last_surface_kept.cpu().tolist()
        if args.chamfer_gates:
            line["chamfer_gates"] = GATES
            line["final_chamfer_kept"] = stage.last_chamfer_kept.cpu().tolist()
        if args.robust:
            line["robust"] = ROBUST
            line["final_robust_weights"] = {k: (None if v is None else v.cpu().tolist()) for k, v in stage.last_robust_weights.items()}
        print(json.dumps(line))
        del stage, targets, fit


if __name__ == "__main__":
    main()

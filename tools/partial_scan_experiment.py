"""What the gates and the robust kernel buy on a partial scan: the stand-in fitted to a posed, reshaped copy of
itself with a contiguous third of the target's faces removed, as three stages (init 150, default 600, deform 300 iterations),
the surface weights 1 and 1 beside the four default weights, and `Stage.metrics()` against the COMPLETE target, which the fit never
saw.  One JSON line per column:

    off       no gate
    surface   the surface term's gates: reject_boundary, min_cos 0 and max_dist 0.1 both ways (f10's column)
    both      the same gates on the surface term and on the chamfer term (f11)
    robust    no gate; the Geman-McClure kernel on all four directions (f12), sigma = SIGMA below
    robust_both   the kernel on the matches both gate sets keep

    python tools/partial_scan_experiment.py [--columns off surface both robust robust_both] [--seed 6]

SIGMA = 0.05, half the gates' cap of 0.1, in every stage: a match at the cap keeps (1/5)^2 = 4 % of its pull, one at 3 sigma 1 %,
and a match within a fifth of sigma (0.01, twice the gated fits' mean distance) more than 92 %.  The robust columns add the share
of vertices whose weight is below 0.01 at the final parameters, beside f11's "no data term" share: for the chamfer match, for the
surface match, and for both at once (a dropped vertex counts with weight 0).

The problem is tests/mesh3d_cases.fitter_problem (one mesh), the patch tests/surface_gate_cases.remove_patch(share 1/3, seed 3)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GATES = dict(reject_boundary=True, min_cos_point=0.0, min_cos_vert=0.0, max_dist_point=0.1, max_dist_vert=0.1)
STAGES = (("init", 150, 0.05), ("default", 600, 0.02), ("deform", 300, 0.005))
SIGMA = 0.05
ROBUST = dict(sigma_chamfer_point=SIGMA, sigma_chamfer_vert=SIGMA, sigma_surface_point=SIGMA, sigma_surface_vert=SIGMA)
COLUMNS = dict(off=(None, None, None), surface=(GATES, None, None), both=(GATES, GATES, None), robust=(None, None, ROBUST),
               robust_both=(GATES, GATES, ROBUST))
LOW_WEIGHT = 0.01


def run(column, seed):
    import torch
    from smalify_amd.fitter_3d import Stage, TargetMeshes
    from tests import mesh3d_cases as m3
    from tests import surface_gate_cases as gc
    surface_gates, chamfer_gates, robust = COLUMNS[column]
    md, fit, complete = m3.fitter_problem(1, seed=seed)
    partial = TargetMeshes(complete.verts, [gc.remove_patch(v, f, 1.0 / 3.0, 3 + n)[1]
                                            for n, (v, f) in enumerate(zip(complete.verts, complete.faces))])
    done = 0
    kept = {}
    for name, nits, lr in STAGES:
        stage = Stage(nits, name, fit, partial, name=name, lr=lr, custom_lrs=m3.DEFAULT_CUSTOM_LRS if name == "default" else None,
                      loss_weights=dict(w_point_surface=1.0, w_vert_surface=1.0), seed=11, iteration_offset=done,
                      surface_gates=surface_gates, chamfer_gates=chamfer_gates, robust=robust)
        stage.run(plot=False, progress=False)
        done += nits
        if stage.last_surface_kept is not None:
            kept["surface_kept"] = stage.last_surface_kept.cpu().tolist()
        if stage.last_chamfer_kept is not None:
            kept["chamfer_kept"] = stage.last_chamfer_kept.cpu().tolist()
    if robust is not None:
        # the weights at the final parameters: one more evaluation (the component calls), then the surface term's per vertex
        kept["robust_weight_sums"] = {k: v.cpu().tolist() for k, v in stage.last_robust_weights.items()}
        stage.evaluate(done)
        wc = stage._buffers["vert_weights"]
        sf = stage._objective.surface(stage._buffers["verts"], partial, stage.last_points, 1.0, 1.0, gates=surface_gates,
                                      point_normals=stage._point_normals if surface_gates else None, robust=robust)
        ws = sf["vert_weights"]
        kept["low_weight_share"] = dict(chamfer=float((wc < LOW_WEIGHT).float().mean()), surface=float((ws < LOW_WEIGHT).float().mean()),
                                        both=float(((wc < LOW_WEIGHT) & (ws < LOW_WEIGHT)).float().mean()))
    torch.cuda.synchronize()
    # the score against the target with nothing removed
    judge = Stage(1, "init", fit, complete, seed=11)
    m = judge.metrics()
    batch = m["batch"]
    line = dict(column=column, seed=seed, verts=judge.n_verts, final_total_loss=float(stage.last_terms[4]), **kept)
    for k, v in batch.items():
        line[k] = v if not hasattr(v, "tolist") else v.tolist()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", nargs="+", default=list(COLUMNS), choices=list(COLUMNS))
    ap.add_argument("--seed", type=int, default=6)
    args = ap.parse_args()
    for column in args.columns:
        print(json.dumps(run(column, args.seed), default=float))


if __name__ == "__main__":
    main()

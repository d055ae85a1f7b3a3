"""What the gates buy on a partial scan: the stand-in fitted to a posed, reshaped copy of
itself with a contiguous third of the target's faces removed, as three stages (init 150, default 600, deform 300 iterations),
the surface weights 1 and 1 beside the four default weights, and `Stage.metrics()` against the COMPLETE target, which the fit never
saw.  One JSON line per column:

    off       no gate
    surface   the surface term's gates: reject_boundary, min_cos 0 and max_dist 0.1 both ways (f10's column)
    both      the same gates on the surface term and on the chamfer term (f11)

    python tools/partial_scan_experiment.py [--columns off surface both] [--seed 6]

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
COLUMNS = dict(off=(None, None), surface=(GATES, None), both=(GATES, GATES))


def run(column, seed):
    import torch
    from smalify_amd.fitter_3d import Stage, TargetMeshes
    from tests import mesh3d_cases as m3
    from tests import surface_gate_cases as gc
    surface_gates, chamfer_gates = COLUMNS[column]
    md, fit, complete = m3.fitter_problem(1, seed=seed)
    partial = TargetMeshes(complete.verts, [gc.remove_patch(v, f, 1.0 / 3.0, 3 + n)[1]
                                            for n, (v, f) in enumerate(zip(complete.verts, complete.faces))])
    done = 0
    kept = {}
    for name, nits, lr in STAGES:
        stage = Stage(nits, name, fit, partial, name=name, lr=lr, custom_lrs=m3.DEFAULT_CUSTOM_LRS if name == "default" else None,
                      loss_weights=dict(w_point_surface=1.0, w_vert_surface=1.0), seed=11, iteration_offset=done,
                      surface_gates=surface_gates, chamfer_gates=chamfer_gates)
        stage.run(plot=False, progress=False)
        done += nits
        if stage.last_surface_kept is not None:
            kept["surface_kept"] = stage.last_surface_kept.cpu().tolist()
        if stage.last_chamfer_kept is not None:
            kept["chamfer_kept"] = stage.last_chamfer_kept.cpu().tolist()
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

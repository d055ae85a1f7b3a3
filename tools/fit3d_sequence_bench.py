#!/usr/bin/env python3
"""Time a default-scheme Stage.step with and without the scan-sequence block (include/smalfit.h, "scan sequences"): one extra
launch, fit3d_sequence_kernel, between the betas assembly and Adam.  The method of tools/rigid_align_bench.py: device events round
a run of whole steps (no host synchronisation inside), warmed up, the median and the spread of the repeats.  Needs a GPU.

    python tools/fit3d_sequence_bench.py [--meshes 1 8 32] [--steps 50] [--repeats 7] [--vertex] [--plain-only | --only KIND]
                                         [--library FILE.so] [--label TEXT] [--out FILE.json]

Per batch size: "plain" = the stage without clip_lengths (the step of before), "sequence" = all meshes one clip, share_shape and
the three temporal weights on (at N = 1 the block couples nothing and launches nothing).  Both from the same start, alternating
repeat by repeat in one process.  --plain-only --library FILE.so times the plain step of another build of the library (the parent
commit's), the same way; that build need not export the sequence entry points.
--vertex adds a third stage to the alternation, "vertex" = the sequence stage with the velocity and acceleration terms on the posed
vertices on as well (two more launches, fit3d_sequence_vertex_kernel and its finish kernel, between the surface term and the LBS
adjoint; at N = 1 nothing is launched, at N = 2 only the velocity term applies); its extra time is taken against "sequence".
--only KIND times one of plain | sequence | vertex alone, a process of its own (with --library: another build's).
Synthetic SMAL-topology model and targets (posed copies of it), as tools/fit3d_bench.py; 3000 points per mesh, all four terms."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TEMPORAL = dict(w_temp_joint=1.0, w_temp_global=1.0, w_temp_trans=1.0)
TEMPORAL_VERTS = dict(w_temp_vert_vel=1.0, w_temp_vert_acc=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--steps", type=int, default=50, help="steps between the two events of one repeat")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--vertex", action="store_true", help="also time the sequence stage with the vertex terms on")
    ap.add_argument("--only", choices=("plain", "sequence", "vertex"), default=None, help="time this stage alone")
    ap.add_argument("--library", type=str, default=None, help="load this libsmalfit.so in place of the tree's")
    ap.add_argument("--label", type=str, default="branch")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from smalify_amd import _lib
    if args.library:
        _lib.LIB_PATH = os.path.abspath(args.library)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fit3d_sequence_bench needs a GPU: no time is reported without one")
    from smalify_amd import synthetic
    from smalify_amd.fitter_3d import SMAL3DFitter, Stage, TargetMeshes
    from tools.fit3d_bench import targets_for

    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    smal_data = synthetic.synthetic_smal_dicts(seed=0)[1]
    rows = []
    for N in args.meshes:
        targets = TargetMeshes(targets_for(md, N, seed=N), [np.asarray(md.faces)] * N)
        kinds = {"plain": {}, "sequence": dict(clip_lengths=(N,), temporal=TEMPORAL)}
        if args.vertex or args.only == "vertex":
            kinds["vertex"] = dict(clip_lengths=(N,), temporal=TEMPORAL, temporal_verts=TEMPORAL_VERTS)
        only = "plain" if args.plain_only else args.only
        if only:
            kinds = {only: kinds[only]}
        stages = {}
        for kind, kw in kinds.items():
            fit = SMAL3DFitter(batch_size=N, shape_family=-1, model_data=md, smal_data=smal_data)
            stages[kind] = Stage(10 ** 6, "default", fit, targets, lr=0.01, custom_lrs={"joint_rot": 0.005}, **kw)
            for i in range(10):
                stages[kind].step(i)
        torch.cuda.synchronize()
        us = {kind: [] for kind in kinds}
        done = 10
        for _ in range(args.repeats):
            for kind, stage in stages.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for i in range(args.steps):
                    stage.step(done + i)
                t1.record()
                torch.cuda.synchronize()
                us[kind].append(1e3 * t0.elapsed_time(t1) / args.steps)
            done += args.steps
        for kind in kinds:
            row = dict(label=args.label, meshes=N, step=kind, steps=args.steps, repeats=args.repeats,
                       step_us_median=float(np.median(us[kind])), step_us_min=float(min(us[kind])), step_us_max=float(max(us[kind])))
            if kind == "sequence":
                row["temporal_losses"] = [float(x) for x in stages[kind].last_temporal_losses]
                if "plain" in us:
                    row["extra_us_median"] = row["step_us_median"] - float(np.median(us["plain"]))
            if kind == "vertex":
                row["temporal_vertex_losses"] = [float(x) for x in stages[kind].last_temporal_vertex_losses]
                if "sequence" in us:
                    row["extra_us_median"] = row["step_us_median"] - float(np.median(us["sequence"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del stages, targets
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Developer measurement (GPU box) of smalfit_mesh_score: `--calls` calls of MeshObjective.score for a batch of `--meshes`
stand-in SMAL meshes against stand-in-sized targets (posed copies of the template, 7774 faces) with 3000 sampled points and
three thresholds.  Meant to run under `rocprofv3 --kernel-trace --stats` (no counters), one process per batch size:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o score -- python tools/mesh_score_profile.py --meshes 32

Prints one JSON line: the batch figures and the wall time per call (host timer around a synchronised loop)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=1)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--points", type=int, default=3000)
    args = ap.parse_args()
    import torch
    from smalify_amd import engine as eng, metrics, synthetic
    from tools.fit3d_bench import targets_for

    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    N, V = args.meshes, md.num_verts
    faces = np.asarray(md.faces, np.int32)
    base = np.asarray(md.v_template, np.float32)
    base = (base - base.mean(0)) / np.abs(base - base.mean(0)).max()
    rs = np.random.RandomState(1)
    verts = torch.from_numpy((base[None] + 0.005 * rs.randn(N, V, 3)).astype(np.float32)).cuda()
    targets = eng.MeshTargets(targets_for(md, N, seed=N), [faces] * N)
    objective = eng.MeshObjective(V, faces, N, args.points)
    points = targets.sample(args.points, 3, 0)
    thresholds = (0.01, 0.02, 0.05)
    o = objective.score(verts, targets, points, thresholds)          # warm-up: code objects loaded
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        o = objective.score(verts, targets, points, thresholds)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.calls
    s = metrics.summarise_mesh_score(o["sums"], o["within"], num_verts=V, num_points=args.points, thresholds=thresholds)
    print(json.dumps({"meshes": N, "calls": args.calls, "ms_per_call": 1e3 * dt,
                      "pair_tests_per_call": N * (V + args.points) * len(faces),
                      "summary": metrics.mesh_score_line(s, thresholds)}))


if __name__ == "__main__":
    main()

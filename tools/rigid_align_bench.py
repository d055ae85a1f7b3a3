"""Time one smalfit_rigid_align call at the 3-D fitter's own size: V = 3889 vertices, S = 3000 points, the 24 built-in starts,
30 iterations, one mesh and 32 meshes.  Device events around the whole call (the init, 31 rounds of two scans and a solve, the
pick -- rigid_align_launches of smalfit_plan.h counts them --, no host synchronisation in between), warmed up, the median and
the spread of the repeats.  Needs a GPU.

    python tools/rigid_align_bench.py [--meshes 1 32] [--iterations 30] [--repeats 7] [--trim_point F] [--trim_vert F] [--out FILE.json]

--trim_point / --trim_vert below 1 time smalfit_trimmed_rigid_align instead (a selection launch more per round;
rigid_trim_launches); the handle's first trimmed call, which allocates, is one of the warm-ups.

The points are a rigidly moved, sub-sampled copy of the vertices (a lopsided blob, seeded), so the call does what a user's does:
most starts settle elsewhere, the right one converges."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from smalify_amd import engine as eng  # noqa: E402


def problem(N, V, S, seed=0):
    rs = np.random.RandomState(seed)
    x = np.concatenate([rs.randn(N, V // 2, 3) * [0.45, 0.18, 0.12], rs.randn(N, V - V // 2, 3) * [0.10, 0.12, 0.08] + [0.75, 0.30, 0.10]], 1)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = np.deg2rad(160.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    p = x[:, rs.choice(V, S, replace=False)] @ R.T + [0.2, -0.1, 0.3]
    return torch.as_tensor(x, dtype=torch.float32).cuda().contiguous(), torch.as_tensor(p, dtype=torch.float32).cuda().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--verts", type=int, default=3889)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trim_point", type=float, default=1.0, help="fraction of the points every iteration keeps")
    ap.add_argument("--trim_vert", type=float, default=1.0, help="fraction of the vertices every iteration keeps")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rigid_align_bench needs a GPU: no time is reported without one")
    rows = []
    for N in args.meshes:
        x, p = problem(N, args.verts, args.points)
        al = eng.RigidAligner(N, args.verts, args.points, 24)
        out = {}
        trim = dict(trim_point=args.trim_point, trim_vert=args.trim_vert) if (args.trim_point, args.trim_vert) != (1.0, 1.0) else {}
        for _ in range(2):
            al.align(x, p, iterations=args.iterations, out=out, **trim)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            al.align(x, p, iterations=args.iterations, out=out, **trim)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        row = dict(meshes=N, verts=args.verts, points=args.points, starts=24, iterations=args.iterations,
                   call_ms_median=float(np.median(ms)), call_ms_min=float(min(ms)), call_ms_max=float(max(ms)),
                   per_iteration_ms=float(np.median(ms)) / (args.iterations + 1), **trim,
                   best=[int(b) for b in out["best"].cpu()], best_score=[float(s) for s in out["scores"].min(1).values.cpu()])
        rows.append(row)
        print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Developer measurement (GPU box): fitting a dataset of UNRELATED single images (the reference's StanfordExtra workload,
BASELINE config 1: one image, all four stages), in image-iterations per second of the reference schedule scaled to
--steps iterations the way bench.py scales it (150:400:600:800).

  (a) baseline   one image per fit: FusedFitter, N = 1, window 1 -- how such a dataset is fitted without batching; --repeats
                 runs, so that the run-to-run spread is known
  (b) batched    ImageBatchFitter at --images N (default 1 8 32 64): N images, each with its own shape, in one call

    python tools/image_batch_bench.py [--images 1 8 32 64] [--steps 390] [--size 256] [--repeats 3] [--only batched --images 64]

  (c) rows       what asking for one row of loss terms per image costs: one evaluation (stage-2 weights, the fitted state) with
                 and without losses_per_frame, mean of --row-evals evaluations each (the <true> band / select kernels and
                 frame_loss_rows_kernel against the plain ones)

Prints one JSON line per measurement (and appends them to --out when given).  Synthetic model; every image has its own
ground-truth shape, limb scales, pose and translation, its targets rendered by the engine itself (untimed)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARMUP = 40


def image_scenes(engine, torch, N, S):
    """N unrelated images: ground truth drawn per image -> (keypoints + noise, visibility, hard silhouette as float 0/1)"""
    from smalify_amd import synthetic
    sp = synthetic.synthetic_shape_prior()
    rs = np.random.RandomState(77)
    gts = []
    for n in range(N):
        g = synthetic.ground_truth_params(1, seed=4000 + n, mean_betas=sp[1][:20], mean_logscale=sp[1][20:26])
        g["betas"] = (np.asarray(g["betas"]) + 0.3 * rs.randn(20)).astype(np.float32)
        g["log_beta_scales"] = (np.asarray(g["log_beta_scales"]) + 0.1 * rs.randn(6)).astype(np.float32)
        g["trans"] = (np.asarray(g["trans"]) + np.array([0.0, 0.0, 0.4 * rs.rand()])).astype(np.float32)
        gts.append(g)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=engine.device, dtype=torch.float32).contiguous()  # noqa: E731
    shapes = dict(betas=(N, 20), log_beta_scales=(N, 6), global_rotation=(N, 3), joint_rotations=(N, 34, 3), trans=(N, 3))
    cat = lambda k: np.stack([np.asarray(g[k], np.float32).reshape(shapes[k][1:]) for g in gts])  # noqa: E731
    sil = torch.empty(N, S, S, device=engine.device)
    proj = torch.empty(N, 25, 2, device=engine.device)
    engine.fit_eval(betas=t(cat("betas")), log_beta_scales=t(cat("log_beta_scales")), global_rotation=t(cat("global_rotation")),
                    joint_rotations=t(cat("joint_rotations")), trans=t(cat("trans")), target_joints=None, target_visibility=None,
                    target_sil=None, weights=(0, 0, 0, 0, 0, 0), w_temp=0.0, window=1, temporal=False, want=(), sil_out=sil,
                    proj_out=proj, subject_frames=1)
    noise = rs.randn(N, 25, 2).astype(np.float32)
    vis = (rs.rand(N, 25) < 0.9).astype(np.float32)
    vis[:, [2, 5, 8, 11, 12, 23]] = 1.0
    return (proj + t(noise)).contiguous(), t(vis), (sil > 0.5).float().contiguous(), sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--steps", type=int, default=390)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=("baseline", "batched"), default=None)
    ap.add_argument("--row-evals", type=int, default=50)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import bench
    from smalify_amd import config, engine as eng, fitter as fit, image_batch, synthetic

    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    dm = eng.DeviceModel(md)
    W = np.array(config.OPT_WEIGHTS).T
    S = args.size

    def run(f, schedule):
        for stage_id, iters in enumerate(schedule):
            if iters:
                f.begin_stage(stage_id)
                f.run_iterations(W[stage_id][:6], float(W[stage_id][6]), float(W[stage_id][8]), stage_id, iters)

    def emit(doc):
        doc.update(image_size=S, steps=args.steps, schedule=bench.scaled_schedule(args.steps), kernel_source_sha=bench.kernel_source_sha(),
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(doc)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def measure(N, make, repeats):
        e = eng.Engine(dm, N, S)
        e.set_pose_prior(*synthetic.synthetic_pose_prior())
        sp = synthetic.synthetic_shape_prior()
        e.set_shape_prior(*sp)
        tj, vis, tsil, _ = image_scenes(e, torch, N, S)
        run(make(e, tj, vis, tsil, sp), bench.scaled_schedule(WARMUP))
        rates, final = [], None
        for _ in range(repeats):
            f = make(e, tj, vis, tsil, sp)
            e.reset_raster_cache()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(f, bench.scaled_schedule(args.steps))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert e.status() == 0
            rates.append(N * args.steps / dt)
            final = float(f.losses.sum())
        return rates, final, f

    def rows_cost(f, N):
        """us per evaluation without / with losses_per_frame at the fitted state (torch events on the launch stream)"""
        w = W[2][:6]
        out = {}
        for name, kw in (("plain", {}), ("rows", dict(losses_per_frame=f.losses_per_image))):
            for _ in range(5):
                f.evaluate(w, 0.0, 2, **kw)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.row_evals):
                f.evaluate(w, 0.0, 2, **kw)
            ev[1].record()
            torch.cuda.synchronize()
            out[name] = 1e3 * ev[0].elapsed_time(ev[1]) / args.row_evals
        emit({"path": "one evaluation with / without losses_per_frame (subject_frames = 1)", "images": N, "evaluations": args.row_evals,
              "us_per_evaluation_plain": out["plain"], "us_per_evaluation_with_rows": out["rows"],
              "rows_cost_us": out["rows"] - out["plain"]})

    if args.only != "batched":
        rates, final, _ = measure(1, lambda e, tj, vis, tsil, sp: fit.FusedFitter(e, tj, vis, tsil, 1, True, sp[1][:20], sp[1][20:26]), args.repeats)
        emit({"path": "baseline: FusedFitter, one image per fit (N = 1, window 1)", "images": 1,
              "image_iterations_per_s": float(np.median(rates)), "runs": rates,
              "spread_rel": float((max(rates) - min(rates)) / np.median(rates)), "us_per_iteration": 1e6 / float(np.median(rates)),
              "final_total_loss": final})
    if args.only != "baseline":
        for N in args.images:
            rates, final, f = measure(N, lambda e, tj, vis, tsil, sp: image_batch.ImageBatchFitter(e, tj, vis, tsil, True, sp[1][:20], sp[1][20:26]),
                                   args.repeats if N == 1 else 1)
            emit({"path": "ImageBatchFitter (subject_frames = 1)", "images": N, "image_iterations_per_s": float(np.median(rates)),
                  "runs": rates, "us_per_iteration": 1e6 * N / float(np.median(rates)), "final_total_loss_sum_over_images": final})
            rows_cost(f, N)


if __name__ == "__main__":
    main()

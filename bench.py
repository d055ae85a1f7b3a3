#!/usr/bin/env python3
"""Benchmark of the SMAL per-frame fitting hot path on MI355X.

metric  : fitter iterations/sec  (BASELINE.json) -- one iteration = one epoch of the reference loop
          (smal_fitter/optimize_to_joints.py:113-137): LBS + projection + soft-silhouette render + all
          losses + temporal term + full gradient + Adam step over the whole batch.
workload: synthetic BADJA-shape sequence, 64 frames, 256x256, WINDOW_SIZE 8, shape family 1 with the
          unity-style shape prior, synthetic SMAL-topology model (V=3889, F=7774); targets (keypoints + noise, visibility,
          hard silhouettes) rendered once by the float64 CPU oracle and committed as data (tests/golden/eval_targets_*.npz).  The K timed steps run
          the reference's 4-stage schedule (150:400:600:800 iterations, config.py:63-72) scaled to K
          iterations, each stage with its own weights / learning rate / fresh Adam state, one library
          call (smalfit_fit_run) per stage.  With --steps 1950 the timed region is exactly one complete fit.

timing  : W untimed warm-up steps, then EXACTLY K steps between (barrier +) torch.cuda.synchronize() on both
          sides, nothing synchronising in between (per-stage times come from HIP events on the launch stream).
          The warm-up is at least INTERNAL_WARMUP iterations whatever --warmup says (clocks, code objects, allocator;
          SMALFIT_BENCH_MIN_WARMUP overrides the floor for measurements of its effect);
          the JSON reports the real number.  `value` is COLD-HONEST: the rasteriser's per-pixel depth-bound cache is
          forgotten (smalfit_engine_reset_raster_cache) before the timed fit starts, so the fit pays its first exact
          K-nearest selection inside the timed region, exactly like a fit of a new sequence does -- and so is the host-side
          set-up of every stage's argument block (round 3 prebuilt the four blocks before the region).  `value_primed` is a
          second, separately timed run of the same K steps after ONE untimed silhouette evaluation of the initial state --
          what a K-step window in the middle of a long fit looks like.  Neither region carries instrumentation beyond five
          stream events at the stage boundaries; the per-section HIP events behind `roofline` / `section_ms` are recorded in a
          THIRD run of the same K steps (primed; every 8th iteration), because a profiled iteration costs ~60 us of event
          records and pipeline bubbles.
          `value_crop` (--full, scene=survey runs only; --no-crop skips it) is ONE complete 1950-iteration fit, timed the same way, of the
          crop-filling scene: the animal as large in the image as the reference's loaders deliver it (utils.py:5-36).  It does
          not scale with --steps: every fit starts from the reference's small initial mesh, so only a complete fit spends most
          of its iterations in that regime.

multi-GPU: `python bench.py --gpus N` launches N ranks itself (torch.distributed.run, one process per GPU, RCCL)
          when it is not already running under a launcher; under `python -m torch.distributed.run ... bench.py
          --gpus N` it is one of the ranks.  Frames are sharded contiguously across ranks (strong scaling: the
          64-frame sequence is BASELINE.json's config 4), see smalify_amd/distributed.py.

Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the cold K-step fit behind `value` / `ms_per_step` and prints the line.  `--full` adds
everything else the line can carry: `value_primed`, the profiled run behind `section_ms` / `roofline`, `value_crop` (scene=survey;
--no-crop skips it), and with one rank `cpu_baseline` and `final_loss_vs_ref` (--no-cpu-baseline skips them).
`--dump-outputs DIR` writes what the timed fit returns after its last step -- the fitted parameters and the loss terms -- as
float32 DIR/<name>.npy; the inputs are seeded, so two builds run with the same arguments can be compared output for output.

SMALFIT_BENCH_FORCE_DIST=1 (validation hook): run the sharded step with its all-gather even when the world is one
rank, so that the RCCL path can be exercised on a single-GPU box.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NUM_FRAMES = 64
IMAGE_SIZE = 256
WINDOW = 8
SCHEDULE_ITERS = (150, 400, 600, 800)
HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
INTERNAL_WARMUP = int(os.environ.get("SMALFIT_BENCH_MIN_WARMUP", "40"))           # minimum number of untimed iterations before the timed region
PROFILE_STRIDE = 8
PMC_SUMMARY = os.path.join("profiles", "r6_pmc_summary.json")              # rocprofv3 PMC passes of `bench.py --steps 39` (tools/pmc_sq.py)
PMC_SUMMARY_CROP = os.path.join("profiles", "r6_pmc_summary_crop.json")    # ... of `tools/crop_fit.py crop 0.3` (the crop-filling scene)
FULL_RATE_CYCLES = 2.0          # cycles a full-rate wave64 vector instruction occupies a SIMD (MI355X_MICROARCH.md: v_fma_f32 wave64 = 2)
NUM_SIMDS = 1024                # 256 CUs x 4
PEAK_CLOCK_GHZ = 2.4            # /opt/skills/guides/MI355X_MICROARCH.md: max clock 2400 MHz
ORACLE_TARGETS = {"survey": os.path.join("tests", "golden", "eval_targets_config3.npz"),
                  "crop": os.path.join("tests", "golden", "eval_targets_crop64.npz")}


def kernel_source_sha():
    """sha256 over the kernel sources: a PMC summary under profiles/ belongs to exactly one version of the kernels"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "smalify_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if os.path.isfile(os.path.join(d, f)) and f.endswith((".inc", ".h", ".hip")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def scaled_schedule(total):
    """split `total` iterations over the 4 stages in the reference's 150:400:600:800 proportion"""
    raw = [total * s / float(sum(SCHEDULE_ITERS)) for s in SCHEDULE_ITERS]
    its = [int(np.floor(r)) for r in raw]
    order = np.argsort([-(r - i) for r, i in zip(raw, its)])
    k = 0
    while sum(its) < total:
        its[order[k % 4]] += 1
        k += 1
    return its


TARGET_SOURCE = {}


def build_problem(engine, torch, scene):
    """ground-truth draw -> targets (data synthesis, untimed).  The targets of the two benchmark scenes were rendered ONCE by the
    float64 CPU oracle (tests/golden/make_oracle_eval.py targets config3 / crop64: projected keypoints + 1 px noise, visibility, hard
    silhouette = oracle soft silhouette > 0.5) and are committed as data (tests/golden/eval_targets_*.npz, 23 KB of packed bits): the
    benchmark input is produced independently of the kernels it times.  Only if such a file is missing are the targets rendered by
    the engine itself, as until round 4 (`data` says which)."""
    from smalify_amd import synthetic
    N, S = NUM_FRAMES, IMAGE_SIZE
    sp = synthetic.synthetic_shape_prior()
    gt = synthetic.ground_truth_params(N, seed=1234, mean_betas=sp[1][:20], mean_logscale=sp[1][20:26])
    if scene == "crop":           # animal fills the crop, as BADJA crops do (data_loader crop_to_silhouette)
        gt["trans"][:, 2] += 1.2
    dev = engine.device
    t = lambda a: torch.as_tensor(a, device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    path = os.path.join(ROOT, ORACLE_TARGETS[scene])
    if os.path.exists(path) and os.environ.get("SMALFIT_BENCH_ENGINE_TARGETS") != "1":
        z = np.load(path, allow_pickle=False)
        shape = tuple(int(x) for x in z["shape"])
        if shape == (N, S, S):
            tsil = np.unpackbits(z["tsil_bits"])[:N * S * S].reshape(shape).astype(np.float32)
            # the committed targets must belong to THIS ground-truth draw (they are data made offline; `gt`, the noise and the visibility
            # are re-drawn here): one untimed evaluation of the ground truth -- its projected keypoints + the seeded noise must be the
            # stored keypoints, its silhouette the stored one up to the few rim pixels float32 and float64 decide differently.  Stale
            # targets fail loudly instead of being fitted.
            sil = torch.empty(N, S, S, device=dev)
            proj = torch.empty(N, 25, 2, device=dev)
            engine.fit_eval(betas=t(gt["betas"]), log_beta_scales=t(gt["log_beta_scales"]), global_rotation=t(gt["global_rotation"]),
                            joint_rotations=t(gt["joint_rotations"]), trans=t(gt["trans"]), target_joints=None, target_visibility=None,
                            target_sil=None, weights=(0, 0, 0, 0, 0, 0), w_temp=0.0, window=WINDOW, want=(), sil_out=sil, proj_out=proj)
            noise, vis = synthetic.keypoint_noise_and_visibility(N)
            kp_err = float((proj + t(noise) - t(z["tj"])).abs().max())
            sil_diff = float(((sil > 0.5).float() - t(tsil)).abs().mean())
            vis_same = bool(np.array_equal(np.asarray(vis, np.float32), np.asarray(z["vis"], np.float32)))
            if kp_err > 0.05 or sil_diff > 2e-4 or not vis_same:
                raise RuntimeError("%s does not belong to today's ground-truth draw (keypoints off by %.3g px, %.3g of the silhouette pixels differ, "
                                   "visibility equal: %s): regenerate it with tests/golden/make_oracle_eval.py targets" % (ORACLE_TARGETS[scene], kp_err, sil_diff, vis_same))
            TARGET_SOURCE[scene] = "float64 CPU oracle (%s; checked against the ground-truth draw: keypoints within %.1e px, %.1e of the silhouette pixels differ)" % (
                ORACLE_TARGETS[scene], kp_err, sil_diff)
            return gt, t(z["tj"]), t(z["vis"]), t(tsil), sp
    TARGET_SOURCE[scene] = "the engine's own rasteriser (sil > 0.5)"
    sil = torch.empty(N, S, S, device=dev)
    proj = torch.empty(N, 25, 2, device=dev)
    engine.fit_eval(betas=t(gt["betas"]), log_beta_scales=t(gt["log_beta_scales"]),
                    global_rotation=t(gt["global_rotation"]), joint_rotations=t(gt["joint_rotations"]),
                    trans=t(gt["trans"]), target_joints=None, target_visibility=None, target_sil=None,
                    weights=(0, 0, 0, 0, 0, 0), w_temp=0.0, window=WINDOW, want=(), sil_out=sil, proj_out=proj)
    noise, vis = synthetic.keypoint_noise_and_visibility(N)
    target_joints = proj + t(noise)
    target_sil = (sil > 0.5).float()
    return gt, target_joints, t(vis), target_sil, sp


def cpu_baseline(md, pose_prior, shape_prior, target_joints, vis, target_sil, W):
    """BASELINE.md section 4's CPU leg: the oracle (CPU port of the same maths: torch float32, pair-list rasteriser --
    already far cheaper than pytorch3d's naive CPU rasteriser --, autograd backward, Adam) timed on the box's host cores
    for CPU_ITERS (>= 20) iterations of BOTH iteration types of the schedule:
      stage-0 type (keypoints + priors + temporal, no silhouette; 150 of the 1950 iterations)  on all 64 frames,
      stage-2 type (silhouette on; 1800 of the 1950 iterations) on the first `nf` frames, nf chosen from a 1-frame probe so
      that the leg costs about 20 s, extrapolated linearly to 64 frames (the cost is per frame).
    `value` = 1950 / (150 t0 + 1800 t2): the rate of the reference's schedule mix, the same mix the GPU value is quoted on.
    torch intra-op threads are capped at 16 (the oracle's tensors are small; more only add contention)."""
    import torch
    from oracle import smal_oracle as so
    from smalify_amd import model_io
    CPU_ITERS = 20
    ncores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(ncores)
    om = so.OracleModel(md, dtype=torch.float32)

    def iterations(nf, count, stage):
        w = W[stage]
        prob = so.FitProblem(om, IMAGE_SIZE, target_joints[:nf], vis[:nf], target_sil[:nf], pose_prior[0], pose_prior[1],
                             pose_prior[2], shape_prior[0], shape_prior[1], min(WINDOW, nf), True, dtype=torch.float32)
        params = dict(betas=torch.from_numpy(shape_prior[1][:20].copy()),
                      log_beta_scales=torch.from_numpy(shape_prior[1][20:26].copy()),
                      global_rotation=torch.from_numpy(np.tile(model_io.initial_global_rotation(), (nf, 1))).float(),
                      trans=torch.zeros(nf, 3), joint_rotations=torch.zeros(nf, 34, 3))
        names = so.trainable_names(stage)
        vis0 = so.stage0_visibility(prob.vis) if stage == 0 else None
        opt = so.Adam(so.PARAM_ORDER, lr=float(w[8]))
        t0 = time.perf_counter()
        for _ in range(count):
            total, sums, grads = so.loss_and_grads(prob, params, w[:6].copy(), float(w[6]), names, visibility=vis0)
            opt.step(params, grads)
            assert (sums.get("sil_reproj", 0.0) > 0.0) == (stage != 0), "wrong iteration type in the CPU baseline sample"
        return (time.perf_counter() - t0) / count

    iterations(NUM_FRAMES, 2, 0)                                  # untimed: allocator, thread pool
    t_stage0 = iterations(NUM_FRAMES, CPU_ITERS, 0)
    t1 = iterations(1, 1, 2)
    nf = int(max(1, min(NUM_FRAMES, 20.0 / (CPU_ITERS * max(t1, 1e-3)))))
    t_sil = iterations(nf, CPU_ITERS, 2)
    t_stage2 = t_sil * (NUM_FRAMES / nf)
    mix = sum(SCHEDULE_ITERS) / (SCHEDULE_ITERS[0] * t_stage0 + sum(SCHEDULE_ITERS[1:]) * t_stage2)
    return {"value": mix, "unit": "iterations/s", "cores": ncores, "kind": "port",
            "stage0_type_iterations_per_s": 1.0 / t_stage0, "stage2_type_iterations_per_s": 1.0 / t_stage2,
            "sample": "oracle (torch CPU float32 restatement, pair-list rasteriser), %d timed iterations per type incl. backward + "
                      "Adam: stage-0 type on all 64 frames %.3f s/iteration; stage-2 type on %d of 64 frames %.2f s/iteration "
                      "(1-frame probe %.2f s), extrapolated x%.1f; value = 1950 / (150 t0 + 1800 t2)"
                      % (CPU_ITERS, t_stage0, nf, t_sil, t1, NUM_FRAMES / nf)}


def final_loss_parity(torch):
    """The metric's second half ('final keypoint/sil loss vs ref') on BASELINE config 2's shape: 8 frames, 256 x 256,
    WINDOW_SIZE 8, the reference's FULL 150/400/600/800 schedule from the reference's initial state, HIP engine vs the
    oracle's float64 run of the same problem (tests/golden/oracle_config2_f64.npz, hours of CPU made offline by
    tests/golden/make_oracle_config2.py; asserted by tests/test_gpu_config2.py).  Over ~2000 Adam steps float32 arithmetic
    alone carries any implementation away from a float64 run, so the oracle's own float32 run (oracle_config2_f32.npz) is
    reported next to every number as the yardstick."""
    from tests import config2_case as c2
    from smalify_amd import config, engine as eng, fitter as fit, synthetic
    f64, f32 = c2.load_fixture("f64"), c2.load_fixture("f32")
    if f64 is None or not f64["complete"]:
        return {"error": "tests/golden/oracle_config2_f64.npz missing or incomplete"}
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    e = eng.Engine(eng.DeviceModel(md), c2.FRAMES, c2.IMAGE_SIZE)
    e.set_pose_prior(*synthetic.synthetic_pose_prior())
    e.set_shape_prior(*synthetic.synthetic_shape_prior())
    tg, start = f64["targets"], c2.initial_params()
    f = fit.FusedFitter(e, tg["tj"], tg["vis"], tg["tsil"].astype(np.float32), c2.WINDOW, True, start["betas"], start["log_beta_scales"])
    Wt = np.array(config.OPT_WEIGHTS).T
    for stage in range(4):
        f.begin_stage(stage)
        f.run_iterations(Wt[stage][:6], float(Wt[stage][6]), float(Wt[stage][8]), stage, c2.SCHEDULE[stage])
    hip = f.losses.cpu().numpy().astype(np.float64)[:8]
    ref = f64["trace"][-1]
    y = f32["trace"][-1] if (f32 is not None and f32["complete"]) else None

    def rel(a, b):
        a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))

    keep = {"frames": c2.FRAMES, "image_size": c2.IMAGE_SIZE, "window": c2.WINDOW, "schedule": list(c2.SCHEDULE),
            "reference": "oracle float64 (tests/golden/oracle_config2_f64.npz)", "status_bits": e.status(),
            "final_total_hip": float(hip.sum()), "final_total_ref": float(ref.sum()),
            "final_total_rel": abs(hip.sum() - ref.sum()) / abs(ref.sum()),
            "final_total_rel_f32_oracle": (abs(y.sum() - ref.sum()) / abs(ref.sum())) if y is not None else None}
    for name in ("joint", "sil_reproj"):
        i = c2.TERMS.index(name)
        keep["final_%s_hip" % name], keep["final_%s_ref" % name] = float(hip[i]), float(ref[i])
        keep["final_%s_rel" % name] = abs(hip[i] - ref[i]) / abs(ref[i])
        keep["final_%s_rel_f32_oracle" % name] = (abs(y[i] - ref[i]) / abs(ref[i])) if y is not None else None
    keep["param_rel_l2"] = {k: rel(f.p[k].cpu().numpy(), f64["final"][k]) for k in c2.PARAMS}
    if y is not None:
        keep["param_rel_l2_f32_oracle"] = {k: rel(f32["final"][k], f64["final"][k]) for k in c2.PARAMS}
    return keep


def dump_outputs(out_dir, base, losses, rank, world):
    """--dump-outputs: what the timed fit hands its caller after its last step -- the fitted parameters (the per-frame ones over
    all frames, gathered from the ranks) and the loss terms -- as float32 DIR/<name>.npy (about 30 KB; rank 0 writes)"""
    import torch.distributed as dist
    arrays = {k: v.detach().cpu().numpy() for k, v in base.p.items()}
    if world > 1:
        per_frame = [k for k, v in arrays.items() if v.ndim > 1]       # joint_rotations, global_rotation, trans (+ per-frame scales)
        parts = [None] * world
        dist.all_gather_object(parts, {k: arrays[k] for k in per_frame})
        for k in per_frame:
            arrays[k] = np.concatenate([p[k] for p in parts])
    arrays["losses"] = losses.detach().cpu().numpy()
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        for name, a in arrays.items():
            np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """not under a launcher and more than one GPU asked for: start one rank per GPU and relay rank 0's JSON line"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=390)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scene", default="survey", choices=["survey", "crop"])
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: value_primed, the profiled run behind section_ms / "
                         "roofline, value_crop (scene=survey), cpu_baseline and final_loss_vs_ref")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline and final_loss_vs_ref")
    ap.add_argument("--no-crop", action="store_true", help="with --full: skip the second timed scene (value_crop: one complete 1950-iteration fit, ~3 s)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the timed fit returns after its last step (fitted parameters, loss terms) to DIR/<name>.npy")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))

    # stdout must carry exactly one JSON line: libraries write there too (RCCL prints a version banner when the
    # communicator is created), so file descriptor 1 points at stderr for the whole run and the line goes to the saved one
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    from smalify_amd import config, distributed, engine as eng, fitter as fit, synthetic

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (smalify_amd has no CPU fallback)")
    if torch.cuda.device_count() < world // max(1, int(os.environ.get("SMALFIT_BENCH_RANKS_PER_GPU", "1"))):
        raise SystemExit("bench.py: %d rank(s) but only %d GPU(s) visible" % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank % torch.cuda.device_count())
    force_dist = os.environ.get("SMALFIT_BENCH_FORCE_DIST") == "1"
    use_dist = world > 1 or force_dist
    if use_dist:
        dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
        assert dist.get_world_size() == world

    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    dm = eng.DeviceModel(md)
    full_engine = eng.Engine(dm, NUM_FRAMES, IMAGE_SIZE)
    pose_prior = synthetic.synthetic_pose_prior()
    gt, tj, vis, tsil, shape_prior = build_problem(full_engine, torch, args.scene)
    # the second scene the line reports: the animal filling the crop, as the reference's loaders deliver it (utils.py:5-36
    # crop_to_silhouette, called at data_loader.py:48,117) -- `value_crop`; the headline stays BASELINE.md section 4's draw
    crop_targets = build_problem(full_engine, torch, "crop")[1:4] if args.full and args.scene == "survey" and not args.no_crop else None
    lo, hi = distributed.shard_range(NUM_FRAMES, rank, world, WINDOW)      # any contiguous split: the engine is told where it sits
    if world > 1:
        del full_engine
        torch.cuda.empty_cache()
        engine = eng.Engine(dm, hi - lo, IMAGE_SIZE)
    else:
        engine = full_engine
    engine.set_pose_prior(*pose_prior)
    engine.set_shape_prior(*shape_prior)

    def new_fitter(targets=None):
        tj_, vis_, tsil_ = (tj, vis, tsil) if targets is None else targets
        f = fit.FusedFitter(engine, tj_[lo:hi], vis_[lo:hi], tsil_[lo:hi], WINDOW, use_unity_prior=True,
                            mean_betas=shape_prior[1][:20], mean_log_scales=shape_prior[1][20:26],
                            frame_offset=lo, total_frames=NUM_FRAMES)
        return distributed.ShardedFitter(f, rank, world, always_exchange=force_dist) if use_dist else f

    W = np.array(config.OPT_WEIGHTS).T

    def run(fitter, iters_per_stage, events=None):
        """the stage loop of optimize_to_joints.py:90-137; unsharded: ONE library call per stage"""
        for stage_id, its in enumerate(iters_per_stage):
            if events is not None:
                events[stage_id].record()
            fitter.begin_stage(stage_id)
            if its == 0:
                continue
            w = W[stage_id]
            # one library call per stage either way: unsharded smalfit_fit_run; sharded smalfit_shard_run, which enqueues the
            # all-gather between the two halves of every iteration itself (RCCL on the kernels' stream)
            fitter.run_iterations(w[:6], float(w[6]), float(w[8]), stage_id, its)
        if events is not None:
            events[len(iters_per_stage)].record()

    def sync():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- the collective is proved BEFORE anything is timed (round 6; until then only afterwards): rank stamps through the very
    # function pointer the sharded loop hands to the library.  The native path (ncclAllGather called from C on torch's communicator)
    # has never met more than one rank on the builder's boxes: if its proof fails, every rank switches to the host callback
    # (torch.distributed's own all-gather) -- the verdict is agreed between the ranks -- and the line says so.
    collective_fallback = None
    if use_dist:
        probe = new_fitter()
        first = probe.prove_world()
        if not first["ok"] and first.get("collective") == "rccl":
            collective_fallback = first
            probe.use_host_collective()
            again = new_fitter().prove_world()
            if not again["ok"]:
                raise SystemExit("bench.py: neither the native nor the host collective spans %d distinct ranks: %r / %r" % (world, first, again))
        del probe

    # ---- warm-up (untimed) --------------------------------------------------------------------------------
    n_warm = max(args.warmup, INTERNAL_WARMUP)
    run(new_fitter(), scaled_schedule(n_warm))
    sched = scaled_schedule(args.steps)

    def timed(primed, sections=False, targets=None, schedule=None):
        """EXACTLY args.steps iterations of a fresh fit between two synchronisation points.  Everything a fit does per stage
        is inside the region, the ~100 us of host-side marshalling of each stage's argument block included (run_iterations
        builds it on first use; round 3 prebuilt the four blocks before the region)."""
        fitter = new_fitter(targets)
        base = fitter.fitter if use_dist else fitter
        base.e.reset_raster_cache()                                  # a new sequence: no depth bounds from the warm-up fit
        if primed:
            base.evaluate(W[1][:6], float(W[1][6]), 1, want=())      # silhouette of the initial state: primes the depth-bound cache
        sched_ = sched if schedule is None else schedule
        if sections:
            # HIP events on the launch stream around the sections of every 8th iteration (an event record costs ~5 us of
            # stream time and stalls the launch pipeline: kept out of the two regions the rates are quoted on)
            base.e.profile_begin(sum(sched_), PROFILE_STRIDE)
        stage_events = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        sync()
        t0 = time.perf_counter()
        run(fitter, sched_, stage_events)
        t_issued = time.perf_counter() - t0
        sync()
        elapsed = time.perf_counter() - t0
        if use_dist:
            tmax = torch.tensor([elapsed], device="cuda")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())
        stage_seconds = [stage_events[i].elapsed_time(stage_events[i + 1]) * 1e-3 for i in range(4)]
        return dict(elapsed=elapsed, t_issued=t_issued, stage_seconds=stage_seconds, sections=base.e.profile_end() if sections else None,
                    status=base.e.status(), fitter=fitter, base=base)

    cold = timed(primed=False)                       # -> value
    primed = profiled = crop_cold = crop_profiled = None
    if args.full:
        primed = timed(primed=True)                      # -> value_primed
        profiled = timed(primed=True, sections=True)     # -> section_ms / roofline (not a quoted rate)
        # -> value_crop: one COMPLETE fit (the reference's 150/400/600/800 iterations) on the crop-filling scene, timed the same way.
        # A K-step window cannot show this scene: every fit starts from the reference's initial state (translation 0: the animal a
        # third of the image wide), and only as it converges on its targets does the mesh grow to fill the crop -- the regime most of
        # a BADJA fit runs in.  K = 1950 is the shortest window that contains it as a real fit does.
        if crop_targets is not None:
            crop_cold = timed(primed=False, targets=crop_targets, schedule=list(SCHEDULE_ITERS))
            crop_profiled = timed(primed=False, sections=True, targets=crop_targets, schedule=list(SCHEDULE_ITERS))
    elapsed, t_issued, stage_seconds, status = (cold[k] for k in ("elapsed", "t_issued", "stage_seconds", "status"))
    for r in (primed, profiled, crop_cold, crop_profiled):
        if r is not None:
            status |= r["status"]
    fitter, base = cold["fitter"], cold["base"]
    losses = fitter.global_losses() if use_dist else base.losses
    final_losses = losses.cpu().numpy().tolist()
    import hashlib
    state_sha = hashlib.sha256(base.flat.cpu().numpy().tobytes() + base.losses.cpu().numpy().tobytes()).hexdigest()[:16]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, base, losses, rank, world)

    world_proof = None
    if use_dist:
        world_proof = fitter.prove_world()          # every rank takes part (a collective); rank 0 reports
        if not world_proof["ok"]:
            raise SystemExit("bench.py: the sharded loop's collective does not span %d distinct ranks: %r" % (world, world_proof))
    if rank == 0:
        V, F, S = md.num_verts, md.num_faces, IMAGE_SIZE
        nloc = hi - lo
        # Algorithmic bytes per launch of the two face sweeps: the
        # frame's projected vertices (12 V per frame) and the faces (12 F) in, the per-pixel sums / per-face adjoints
        # are intermediates.  The target silhouette belongs to the resolve kernel, which reads it.
        algo = {"raster_sweep": nloc * 12 * V + 12 * F, "raster_bwd": nloc * 12 * V + 12 * F + nloc * 24 * F,
                "raster_select": nloc * 12 * V + 12 * F, "raster_resolve": nloc * 4 * S * S}
        kernel_of = {"raster_sweep": "raster_sweep_kernel", "raster_select": "raster_select_kernel",
                     "raster_resolve": "raster_resolve_kernel", "raster_bwd": "raster_bwd_kernel"}
        def issue_and_traffic(kernel, launch_ms, algo, summary_path):
            """`roofline.issue`: how busy the vector ALUs were -- vector wave-instructions per launch (SQ_INSTS_VALU of the committed PMC
            summary) x the 2 cycles a full-rate wave64 instruction occupies a SIMD (/opt/skills/guides/MI355X_MICROARCH.md, "Per-instruction
            cycle constants": v_fma_f32 wave64 = 2 cycles) over the cycles 1024 SIMDs offer in the measured launch time at the 2.4 GHz peak
            clock.  A fraction by construction (round 5 reported a modelled issue cost per instruction instead, which read 1.1); what the
            half-rate instructions of the mix, dependency stalls and waits take is the distance to 1, and `wait_share_of_wave_cycles` says how
            much of it is waiting.  `traffic_ratio`: counter bytes / algorithmic bytes.  Recomputable by hand from the summary file."""
            out_i, traffic_, src = None, None, None
            try:
                pmc_ = json.load(open(os.path.join(ROOT, summary_path)))
                if pmc_.get("kernel_source_sha") != kernel_source_sha():
                    return None, None, summary_path + " is stale (made on other kernel sources): withheld"
                row = next(v for k_, v in pmc_.items() if isinstance(v, dict) and ("smalfit::" + kernel) in k_)   # (template kernels carry "void ...<args>")
                traffic_ = 1024.0 * (2.0 * row["FETCH_SIZE"] + row["WRITE_SIZE"])      # KiB; FETCH_SIZE x2: the guide's gfx950 correction
                cycles = NUM_SIMDS * PEAK_CLOCK_GHZ * 1e9 * launch_ms * 1e-3
                out_i = {"valu_insts_per_launch": row["SQ_INSTS_VALU"], "salu_insts_per_launch": row.get("SQ_INSTS_SALU"),
                         "full_rate_cycles_per_valu": FULL_RATE_CYCLES, "simds": NUM_SIMDS, "clock_ghz": PEAK_CLOCK_GHZ, "launch_ms": launch_ms,
                         "frac": row["SQ_INSTS_VALU"] * FULL_RATE_CYCLES / cycles,
                         "frac_definition": "valu_utilisation = valu_insts_per_launch x %g cycles / (simds x clock x launch time)" % FULL_RATE_CYCLES,
                         "achieved_cycles_per_valu": cycles / row["SQ_INSTS_VALU"],
                         "lds_bank_conflict_per_active": (row["SQ_LDS_BANK_CONFLICT"] / row["SQ_LDS_IDX_ACTIVE"]) if row.get("SQ_LDS_IDX_ACTIVE") else None,
                         "wait_share_of_wave_cycles": (row["SQ_WAIT_ANY"] / row["SQ_WAVE_CYCLES"]) if row.get("SQ_WAVE_CYCLES") else None,
                         "traffic_ratio": traffic_ / algo if algo else None}
                src = summary_path + " (rocprofv3 --pmc, separate passes per counter group; FETCH_SIZE doubled per MI355X_MICROARCH.md); kernel sources " + \
                    pmc_["kernel_source_sha"]
            except Exception as exc:
                src = "unavailable: %r" % (exc,)
            return out_i, traffic_, src

        ms_per_step = 1e3 * elapsed / args.steps
        out = {
            "metric": "fitter iterations/sec", "value": args.steps / elapsed, "unit": "iterations/s",
            "value_definition": "value: cold rasteriser cache (a fit of a new sequence, first exact K-nearest selection and the host-side "
                                "set-up of every stage's argument block inside the timed region)",
            "n_gpus": world, "steps": args.steps, "warmup": n_warm, "warmup_requested": args.warmup,
            "ms_per_step": ms_per_step, "host_issue_ms_per_step": 1e3 * t_issued / args.steps,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic; targets rendered by " + "; ".join("%s: %s" % kv for kv in sorted(TARGET_SOURCE.items())),
            "config": {"workload": "synthetic BADJA-shape sequence: %d frames, %dx%d, WINDOW_SIZE %d, shape family 1, "
                                   "reference 4-stage schedule scaled to %d iterations %s, scene=%s"
                                   % (NUM_FRAMES, S, S, WINDOW, args.steps, sched, args.scene),
                       "frames": NUM_FRAMES, "image_size": S, "window": WINDOW, "parallelism": "frames/%d" % world},
            "per_stage_iterations_per_s": {"stage%d" % i: (sched[i] / stage_seconds[i] if stage_seconds[i] > 0 and sched[i] else None)
                                           for i in range(len(sched))},
            "final_losses": dict(zip(eng.LOSS_NAMES, final_losses)), "status_bits": status,
            "final_state_sha256": state_sha, "kernel_source_sha": kernel_source_sha(),
        }
        if args.full:
            sec_ms = {k: (v[0] / v[1] if v[1] else None) for k, v in profiled["sections"].items()}
            # dominant kernel: whichever rasteriser kernel has the largest average launch time in this run (HIP events
            # around that kernel alone)
            cand = {k: sec_ms[k] for k in kernel_of if sec_ms.get(k)}
            dom_name = max(cand, key=cand.get) if cand else None
            dom = cand.get(dom_name) if dom_name else None
            algo_bytes = algo.get(dom_name)
            achieved = algo_bytes / (dom * 1e-3) / 1e9 if dom else None
            issue, traffic, traffic_source = issue_and_traffic(kernel_of.get(dom_name), dom, algo_bytes, PMC_SUMMARY_CROP if args.scene == "crop" else PMC_SUMMARY) if dom_name else (None, None, None)
            iter_bytes = 2 * 16442644 + NUM_FRAMES * (4 * S * S + 3324)            # 49.88 MB / iteration
            out["value_definition"] += ("; value_primed: same K steps timed again after one untimed silhouette evaluation of "
                                        "the initial state (a K-step window inside a long fit)")
            out.update({
                "value_primed": args.steps / primed["elapsed"], "ms_per_step_primed": 1e3 * primed["elapsed"] / args.steps,
                "per_stage_iterations_per_s_primed": {"stage%d" % i: (sched[i] / primed["stage_seconds"][i] if primed["stage_seconds"][i] > 0 and sched[i] else None)
                                                      for i in range(len(sched))},
                "roofline": {"bound": "hbm", "bound_note": "HBM is the contract's yardstick; this kernel is bound by vector issue and waits: see `issue`", "kernel": kernel_of.get(dom_name), "achieved": achieved, "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic,
                             "traffic_source": traffic_source, "algorithmic_bytes_per_launch": algo_bytes, "avg_launch_ms": dom,
                             "issue": issue,
                             # whole iteration, whole job: SURVEY.md section 8d's byte formula over the measured step, against N x peak
                             "iteration": {"algorithmic_bytes": iter_bytes, "achieved": iter_bytes / (ms_per_step * 1e-3) / 1e9,
                                           "frac": iter_bytes / (ms_per_step * 1e-3) / 1e9 / (HBM_PEAK_GBS * world)}},
                "section_ms": sec_ms, "section_ms_source": "third run of the same steps (primed, HIP events on every %dth iteration): %.1f it/s with the events in"
                                                         % (PROFILE_STRIDE, args.steps / profiled["elapsed"]),
            })
        if use_dist:
            out["world_proof"] = world_proof        # rank stamps gathered through the loop's own collective; ncclCommCount / ncclCommUserRank
            if collective_fallback is not None:
                out["world_proof"]["native_collective_failed"] = collective_fallback      # the host callback took over (see above)
            out["collective"] = fitter._collective()[3] + ": one all-gather of %d floats per rank and iteration, enqueued by smalfit_shard_run" % (base.num_shared() + 216)
        if crop_cold is not None:
            full = list(SCHEDULE_ITERS)
            out["value_crop"] = sum(full) / crop_cold["elapsed"]
            out["value_crop_definition"] = ("ONE complete fit, %d iterations in the reference's %s schedule whatever --steps says, cold cache, timed like "
                                            "`value`, on scene=crop: the ground-truth animal 1.2 units nearer the camera so that it fills the 256x256 "
                                            "crop as the reference's loaders deliver it (utils.py:5-36 crop_to_silhouette, data_loader.py:48,117); the fit "
                                            "starts from the reference's initial state like every fit, so only a complete fit spends its stages 2-3 on "
                                            "the large mesh" % (sum(full), full))
            out["ms_per_step_crop"] = 1e3 * crop_cold["elapsed"] / sum(full)
            out["per_stage_iterations_per_s_crop"] = {"stage%d" % i: full[i] / crop_cold["stage_seconds"][i] for i in range(4)}
            out["section_ms_crop"] = {k: (v[0] / v[1] if v[1] else None) for k, v in crop_profiled["sections"].items()}
            cc = {k: out["section_ms_crop"][k] for k in kernel_of if out["section_ms_crop"].get(k)}
            if cc:
                dk = max(cc, key=cc.get)
                ci, ct, cs = issue_and_traffic(kernel_of[dk], cc[dk], algo[dk], PMC_SUMMARY_CROP)
                ach = algo[dk] / (cc[dk] * 1e-3) / 1e9
                out["roofline_crop"] = {"bound": "hbm", "kernel": kernel_of[dk], "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                                        "traffic": ct, "traffic_source": cs, "algorithmic_bytes_per_launch": algo[dk], "avg_launch_ms": cc[dk], "issue": ci}
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(md, pose_prior, shape_prior, tj.cpu().numpy(), vis.cpu().numpy(), tsil.cpu().numpy(), W)
            out["final_loss_vs_ref"] = final_loss_parity(torch)
        line = json.dumps(out)
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:                       # the JSON line is the last thing this process writes
        sys.stdout.flush()
        sys.stderr.flush()
        os.write(json_fd, (line + "\n").encode())


if __name__ == "__main__":
    main()

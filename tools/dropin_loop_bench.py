#!/usr/bin/env python3
"""Developer measurement (GPU box): the reference's own stage loop (optimize_to_joints.py:90-137) over the drop-in
smalify_amd.smal_fitter.SMALFitter, on bench.py's headline workload -- 64 frames at 256^2, windows of 8, the targets of
tests/golden/eval_targets_config3.npz as bench.build_problem delivers them, the schedule scaled to --steps iterations the way
bench.py scales it (150:400:600:800).

The loop is the reference's: a new torch.optim.Adam(model.parameters(), lr, betas=(0.5, 0.999)) per stage, the stage-0 freeze and
torso visibility (in place), the CPU visibility tensor swapped in from stage 1 on, and per epoch zero_grad, one forward() per
window, get_temporal, backward, step.  Left out: the progress bar, whose description reads the loss on the host every epoch, and
the visualisation every VIS_FREQUENCY epochs.

  window   SMALFitter as it always was: one smalfit_fit_eval per window call
  epoch    SMALFitter(..., epoch_evaluation=True): one smalfit_fit_eval_windows per epoch, every window call served from it

    python tools/dropin_loop_bench.py [--modes window epoch] [--steps 390] [--repeats 3] [--out profiles/dropin_loop_bench.jsonl]
    python tools/dropin_loop_bench.py --rows-evals 200      (also: what the rows cost per evaluation at the fitted state)

--repeats runs per mode, the modes alternating inside one process after an untimed pass over every stage in every mode; host
clock around a region that ends in a device synchronise.  One JSON line per run (and per rows-cost measurement), appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WARMUP = 12       # untimed iterations per mode, spread over the four stages like the timed ones


def reference_loop(torch, config, model, data_visibility, schedule, window, sync):
    """optimize_to_joints.py:90-137 over `model`; -> seconds per stage (each ends in a device synchronise)"""
    dataset_size = model.num_images
    seconds = []
    for stage_id, weights in enumerate(np.array(config.OPT_WEIGHTS).T):
        opt_weight = weights[:6]
        w_temp = weights[6]
        epochs = schedule[stage_id]
        lr = weights[8]
        t0 = time.perf_counter()
        optimizer = torch.optim.Adam(model.parameters(), lr=lr, betas=(0.5, 0.999))
        if stage_id == 0:
            model.joint_rotations.requires_grad = False
            model.betas.requires_grad = False
            model.log_beta_scales.requires_grad = False
            target_visibility = model.target_visibility.clone()
            model.target_visibility *= 0
            model.target_visibility[:, config.TORSO_JOINTS] = target_visibility[:, config.TORSO_JOINTS]
        else:
            model.joint_rotations.requires_grad = True
            model.betas.requires_grad = True
            if config.ALLOW_LIMB_SCALING:
                model.log_beta_scales.requires_grad = True
            model.target_visibility = data_visibility.clone()
        for _epoch_id in range(epochs):
            acc_loss = 0
            optimizer.zero_grad()
            for j in range(0, dataset_size, window):
                batch_range = list(range(j, min(dataset_size, j + window)))
                loss, _losses = model(batch_range, opt_weight, stage_id)
                acc_loss += loss.mean()
            joint_loss, global_loss, trans_loss = model.get_temporal(w_temp)
            acc_loss = acc_loss + joint_loss + global_loss + trans_loss
            acc_loss.backward()
            optimizer.step()
        sync()
        seconds.append(time.perf_counter() - t0)
    return seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", choices=("window", "epoch"), default=["window", "epoch"])
    ap.add_argument("--steps", type=int, default=390)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows-evals", type=int, default=0, help="also time this many smalfit_fit_eval_windows / smalfit_fit_eval pairs at the fitted state")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--label", default=None, help="recorded in every line, e.g. which commit's sources ran")
    args = ap.parse_args()
    import torch
    import bench
    from smalify_amd import config, engine as eng, runtime, synthetic
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter

    N, S, window = bench.NUM_FRAMES, bench.IMAGE_SIZE, bench.WINDOW
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    pose_prior = synthetic.synthetic_pose_prior()
    # the targets (untimed), through an engine of their own
    scratch = eng.Engine(eng.DeviceModel(md), N, S)
    _gt, tj, vis, tsil, shape_prior = bench.build_problem(scratch, torch, "survey")
    del scratch
    data = (torch.zeros(N, 3, S, S), tsil.reshape(N, 1, S, S).cpu(), tj.cpu(), vis.cpu())
    schedule = bench.scaled_schedule(args.steps)

    def new_model(mode):
        kw = {"epoch_evaluation": True} if mode == "epoch" else {}
        return SMALFitter("cuda", data, window, 1, True, model_data=md, pose_prior_data=pose_prior,
                          shape_prior_data=(shape_prior[0], shape_prior[1]), **kw)

    def emit(doc):
        if args.label:
            doc["label"] = args.label
        doc.update(frames=N, image_size=S, window=window, steps=args.steps, schedule=schedule, kernel_source_sha=bench.kernel_source_sha(),
                   device=torch.cuda.get_device_name(0), targets=bench.TARGET_SOURCE.get("survey"))
        line = json.dumps(doc)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    sync = torch.cuda.synchronize
    for mode in args.modes:
        reference_loop(torch, config, new_model(mode), data[-1], bench.scaled_schedule(WARMUP), window, sync)
    last = {}
    for rep in range(args.repeats):
        for mode in args.modes:
            model = new_model(mode)
            engine = runtime.get_engine(model.smal_model.device_model, N, S)
            engine.reset_raster_cache()
            sync()
            seconds = reference_loop(torch, config, model, data[-1], schedule, window, sync)
            assert engine.status() == 0
            total = sum(seconds)
            evaluations = getattr(model, "engine_evaluations", None)
            with torch.no_grad():
                final = float(sum(model(list(range(j, min(N, j + window))), np.array(config.OPT_WEIGHTS).T[3][:6], 3)[0] for j in range(0, N, window)))
            emit({"path": "reference stage loop over the drop-in SMALFitter", "mode": mode, "repeat": rep,
                  "iterations_per_s": args.steps / total, "ms_per_epoch": 1e3 * total / args.steps,
                  "iterations_per_s_by_stage": [its / s if its else None for its, s in zip(schedule, seconds)],
                  "engine_evaluations": evaluations, "final_window_loss_sum": final})
            last[mode] = model

    if args.rows_evals:
        # what the rows cost: one evaluation of the whole sequence at the fitted state, stage-2 weights, with and without them
        model = last.get("epoch") or last.get("window") or new_model("window")
        e = runtime.get_engine(model.smal_model.device_model, N, S)
        kw = dict(betas=model.betas.detach(), log_beta_scales=model.log_beta_scales.detach(), global_rotation=model.global_rotation.detach(),
                  joint_rotations=model.joint_rotations.detach(), trans=model.trans.detach(), target_joints=model.target_joints,
                  target_visibility=model.target_visibility.to("cuda").float(), target_sil=model.sil_imgs.reshape(N, S, S),
                  weights=np.array(config.OPT_WEIGHTS).T[2][:6], w_temp=0.0, window=window, temporal=False)
        calls = {"plain": lambda: e.fit_eval(**kw), "windows": lambda: e.fit_eval_windows(**kw)}
        for _ in range(5):
            for call in calls.values():
                call()
        ms = {k: 0.0 for k in calls}
        for _ in range(args.rows_evals):                      # alternating, an event pair around every evaluation
            for name, call in calls.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                call()
                ev[1].record()
                ev[1].synchronize()
                ms[name] += ev[0].elapsed_time(ev[1])
        emit({"path": "one evaluation of the sequence: smalfit_fit_eval_windows against smalfit_fit_eval (alternating)",
              "evaluations": args.rows_evals, "us_per_evaluation_plain": 1e3 * ms["plain"] / args.rows_evals,
              "us_per_evaluation_with_window_rows": 1e3 * ms["windows"] / args.rows_evals,
              "window_rows_cost_us": 1e3 * (ms["windows"] - ms["plain"]) / args.rows_evals})


if __name__ == "__main__":
    main()

"""Drop-in for reference fitter_3d/optimise.py: fit SMAL to a directory of .obj meshes, stages from YAML or arguments.

    python -m smalify_amd.fitter_3d.optimise --mesh_dir <dir> [--yaml_src cfg.yaml] [--scheme default --lr 1e-3 --nits 100]

Same arguments and YAML layout (`stages: {name: {scheme, nits, lr, loss_weights, custom_lrs}}`, `args: {...}` overriding
the command line) as fitter_3d/optimise.py:18-90 and fitter_3d/example_cfg.yaml.  Beyond the reference, opt-in: --metrics,
--scan_index, --prealign (YAML `args: {prealign: true}`) with --prealign_trim_point / --prealign_trim_vert, and scan sequences:
--sequence (YAML `args: {sequence: true}`) or --clip_lengths L ... make the meshes clips of one animal each, with one shape per
clip and, per stage, `share_shape:`, a `temporal: {w_temp_joint, w_temp_global, w_temp_trans}` block and a
`temporal_verts: {w_temp_vert_vel, w_temp_vert_acc}` block (velocity and acceleration of the posed vertices).

The order of a sequence: with --sequence or --clip_lengths the .obj files are taken in ascending order of their file names (Python's
`sorted`: zero-pad the frame numbers), then every --frame_step'th of them; that is the batch order, and batch order within a clip
is temporal order.  Without either flag the files keep os.listdir's order, as in the reference, and the meshes stay unrelated."""
from __future__ import annotations

import argparse
import os

from .trainer import DEFAULT_METRIC_THRESHOLDS, SMAL3DFitter, SMALParamGroup, Stage, StageManager
from .utils import load_meshes


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--results_dir", type=str, default="fit3d_results", help="Directory in which results are stored")
    parser.add_argument("--mesh_dir", type=str, default="fitter_3d/example_meshes", help="Directory in which meshes are stored")
    parser.add_argument("--frame_step", type=int, default=1,
                        help="If directory is a sequence of animated frames, only take every nth frame")
    parser.add_argument("--shape_family_id", type=int, default=-1,
                        help="Shape family to use for optimisation (-1 to use default SMAL mesh)")
    parser.add_argument("--yaml_src", type=str, default=None, help="YAML source for experimental set-up")
    parser.add_argument("--scheme", type=str, default="default", choices=list(SMALParamGroup.param_map.keys()),
                        help="Optimisation scheme")
    parser.add_argument("--lr", type=float, default=1e-3)
    parser.add_argument("--nits", type=int, default=100)
    parser.add_argument("--seed", type=int, default=0, help="seed of the target-point sampler")
    parser.add_argument("--no_plots", action="store_true", help="skip the per-stage mesh figures")
    parser.add_argument("--metrics", action="store_true",
                        help="score the fit after every stage (exact point-to-surface distances both ways, per mesh) and write "
                             "metrics.json into results_dir")
    parser.add_argument("--metric_thresholds", type=float, nargs="+", default=list(DEFAULT_METRIC_THRESHOLDS),
                        help="distance thresholds of the F-score, in the units of the normalised targets (at most 8)")
    parser.add_argument("--scan_index", action="store_true",
                        help="build a grid over the target meshes for the vertex-to-surface scans (dense scan targets); the "
                             "results are bit for bit those without it")
    parser.add_argument("--prealign", action="store_true",
                        help="before the first stage, stand every SMAL mesh where its target stands: rigid multi-start ICP from the "
                             "24 rotations of the cube, folded into global_rot and trans; its report goes to prealign.json in results_dir")
    parser.add_argument("--prealign_iterations", type=int, default=30, help="ICP iterations of --prealign")
    parser.add_argument("--prealign_trim_point", type=float, default=None, metavar="F",
                        help="with --prealign: every ICP iteration keeps this fraction in (0, 1] of the drawn target points, those "
                             "nearest to the mesh (trimmed ICP: a scan with a floor or a stand in it)")
    parser.add_argument("--prealign_trim_vert", type=float, default=None, metavar="F",
                        help="with --prealign: every ICP iteration keeps this fraction in (0, 1] of the SMAL vertices, those nearest "
                             "to the target (trimmed ICP: a scan that shows part of the animal)")
    parser.add_argument("--sequence", action="store_true",
                        help="the meshes are ONE clip: scans of one animal moving, in ascending file-name order; one shape for all "
                             "of them, and the stages' temporal weights tie consecutive poses")
    parser.add_argument("--clip_lengths", type=int, nargs="+", default=None, metavar="L",
                        help="the meshes are several clips, in ascending file-name order: positive lengths that sum to the number "
                             "of meshes loaded (a length of 1 is an unrelated mesh)")
    return parser


def sequence_clip_lengths(args, num_meshes=None):
    """-> the clip lengths --sequence / --clip_lengths (or the YAML's args) ask for, None when neither is given.  num_meshes: the
    number of meshes loaded, needed for --sequence and checked against --clip_lengths when given"""
    lengths = getattr(args, "clip_lengths", None)
    sequence = bool(getattr(args, "sequence", False))
    if lengths is not None:
        lengths = [int(c) for c in lengths]
        if sequence and len(lengths) != 1:
            raise ValueError("--sequence makes all meshes one clip: give it or --clip_lengths, not both")
        if any(c <= 0 for c in lengths) or (num_meshes is not None and sum(lengths) != int(num_meshes)):
            raise ValueError("--clip_lengths %r: positive lengths with sum %s expected" % (lengths, num_meshes))
        return lengths
    if not sequence:
        return None
    return None if num_meshes is None else [int(num_meshes)]


def main(args, model_data=None, smal_data=None):
    stage_options = None
    if args.yaml_src is not None:
        import yaml
        try:
            with open(args.yaml_src) as infile:
                yaml_cfg = yaml.load(infile, Loader=yaml.FullLoader)
        except FileNotFoundError:
            raise FileNotFoundError(f"No YAML file found at {args.yaml_src}.")
        stage_options = yaml_cfg["stages"]
        for arg, val in (yaml_cfg.get("args") or {}).items():       # YAML args overwrite the command line
            setattr(args, arg, val)

    trims = {k: getattr(args, "prealign_" + k, None) for k in ("trim_point", "trim_vert")}
    if any(v is not None for v in trims.values()) and not getattr(args, "prealign", False):
        raise ValueError("--prealign_trim_point / --prealign_trim_vert trim the ICP of --prealign: give --prealign with them")
    trims = {k: float(v) for k, v in trims.items() if v is not None}
    is_sequence = bool(getattr(args, "sequence", False)) or getattr(args, "clip_lengths", None) is not None
    sequence_order = dict(sorting=sorted) if is_sequence else {}       # a sequence needs a defined order: ascending file names
    mesh_names, target_meshes = load_meshes(mesh_dir=args.mesh_dir, frame_step=args.frame_step,
                                            scan_index=bool(getattr(args, "scan_index", False)), **sequence_order)
    n_batch = len(target_meshes)
    clip_lengths = sequence_clip_lengths(args, n_batch) if is_sequence else None
    os.makedirs(args.results_dir, exist_ok=True)
    manager = StageManager(out_dir=args.results_dir, labels=mesh_names)
    smal_model = SMAL3DFitter(batch_size=n_batch, shape_family=args.shape_family_id, model_data=model_data,
                              smal_data=smal_data)
    if getattr(args, "prealign", False):
        # once, before any stage is built (a stage reads the fitter's vertices when it is constructed)
        import json
        from .trainer import rigid_prealign
        report = rigid_prealign(smal_model, target_meshes, iterations=int(getattr(args, "prealign_iterations", 30)),
                                seed=getattr(args, "seed", 0), **trims)
        names = [str(n) for n in mesh_names] if len(mesh_names) == len(report) else ["mesh_%d" % i for i in range(len(report))]
        with open(os.path.join(args.results_dir, "prealign.json"), "w") as fh:
            json.dump(dict(iterations=int(getattr(args, "prealign_iterations", 30)), starts=24,
                           meshes=[dict(name=nm, **row) for nm, row in zip(names, report)]), fh, indent=1)
    stage_kwargs = dict(target_meshes=target_meshes, smal_3d_fitter=smal_model, out_dir=args.results_dir,
                        mesh_names=mesh_names, seed=getattr(args, "seed", 0))
    if clip_lengths is not None:
        # one shape per clip from the first stage on (a stage that shares the shape refuses rows that differ within a clip)
        from .trainer import tie_shapes
        tie_shapes(smal_model, clip_lengths)
        stage_kwargs["clip_lengths"] = clip_lengths
    if stage_options is not None:
        for stage_name, kwargs in stage_options.items():
            manager.add_stage(Stage(name=stage_name, **kwargs, **stage_kwargs))
    else:
        print("No YAML provided. Loading from system args. ")
        manager.add_stage(Stage(scheme=args.scheme, nits=args.nits, lr=args.lr, **stage_kwargs))
    manager.run(plot=not getattr(args, "no_plots", False), metrics=getattr(args, "metrics", False),
                metric_thresholds=tuple(getattr(args, "metric_thresholds", DEFAULT_METRIC_THRESHOLDS)))
    return manager


if __name__ == "__main__":
    main(build_parser().parse_args())

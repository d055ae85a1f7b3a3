"""From the device's counts to the figures a fit is reported in: silhouette IoU and PCK.

`Engine.fit_metrics` (smalfit_fit_metrics) returns integer pixel counts and float32 keypoint distances per frame and forms no
quotient; `summarise` does, in float64 numpy.  The reference contains no evaluation code, so every definition here is THIS
PROJECT'S (include/smalfit.h words them):

    IoU        pixels in (hard render AND target) / pixels in (hard render OR target); nan for a frame where both are empty
    PCK@t      visible keypoints within t x sqrt(target silhouette pixels) of their target / visible keypoints; nan for a
               frame without a visible keypoint.  (The normaliser is the convention the BADJA / StanfordExtra results are
               recalled to use; no parity with anyone's evaluation script is claimed.)
    groups     PCK over a subset of the 25 keypoints -- this project's grouping, below
    sequence   the mean of the frames' IoU that are not nan; PCK micro-averaged: correct keypoints of all frames / visible
               keypoints of all frames (NOT the mean of the frames' PCK: a frame with two visible keypoints does not weigh
               as much as one with twenty)
"""
from __future__ import annotations

import json

import numpy as np

# the 25 annotated keypoints, in the order of the label list the loaders read (data_loader.py; config.CANONICAL_MODEL_JOINTS
# maps them to model joints)
KEYPOINT_NAMES = (
    "left_front_leg_paw", "left_front_leg_middle", "left_front_leg_top",
    "left_rear_leg_paw", "left_rear_leg_middle", "left_rear_leg_top",
    "right_front_leg_paw", "right_front_leg_middle", "right_front_leg_top",
    "right_rear_leg_paw", "right_rear_leg_middle", "right_rear_leg_top",
    "tail_start", "tail_end", "left_ear_base", "right_ear_base", "nose", "chin", "left_ear_tip", "right_ear_tip",
    "left_eye", "right_eye", "withers", "throat", "tail_mid")
NUM_KEYPOINTS = len(KEYPOINT_NAMES)


def _group_of(name):
    if "_leg_" in name:
        return "legs"
    if name.startswith("tail_"):
        return "tail"
    if "_ear_" in name:
        return "ears"
    if name in ("nose", "chin") or name.endswith("_eye"):
        return "face"
    return "torso"                     # withers, throat


# this project's grouping (no dataset prescribes one): legs 0-11, tail 12 13 24, ears 14 15 18 19, face 16 17 20 21, torso 22 23
KEYPOINT_GROUPS = {g: tuple(i for i, n in enumerate(KEYPOINT_NAMES) if _group_of(n) == g)
                   for g in ("legs", "tail", "ears", "face", "torso")}


def _ratio(num, den):
    """num / den in float64, nan where den == 0"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den > 0)
    return out


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)


def summarise(counts, dist=None, visibility=None, thresholds=()):
    """counts (M,4) = [intersection, union, rendered, target] pixels; dist (M,25) keypoint distances over sqrt(target pixels);
    visibility (M,25), visible where > 0; thresholds: the T values given to the device (compared as float32, like there).
    Device tensors or arrays.  -> dict:
        iou (M,)   intersection, union, rendered, target (M,) int64
        with keypoints: visible (M,), correct (M,T), pck (M,T), pck_groups {group: (M,T)}
        sequence: {iou, frames_with_iou, and with keypoints pck (T,), visible, pck_groups {group: (T,)}}"""
    c = _host(counts).astype(np.int64).reshape(-1, 4)
    out = dict(intersection=c[:, 0], union=c[:, 1], rendered=c[:, 2], target=c[:, 3], iou=_ratio(c[:, 0], c[:, 1]))
    scored = ~np.isnan(out["iou"])
    seq = dict(iou=float(out["iou"][scored].mean()) if scored.any() else float("nan"), frames_with_iou=int(scored.sum()))
    if dist is not None:
        d = _host(dist).astype(np.float64).reshape(len(c), NUM_KEYPOINTS)
        vis = _host(visibility).reshape(len(c), NUM_KEYPOINTS) > 0
        thr = np.asarray([np.float32(t) for t in thresholds], np.float64)
        ok = vis[:, :, None] & (d[:, :, None] <= thr[None, None, :])                  # (M,25,T); nan and inf are never within
        out["visible"], out["correct"] = vis.sum(1), ok.sum(1)
        out["pck"] = _ratio(out["correct"], out["visible"][:, None])
        out["pck_groups"] = {g: _ratio(ok[:, list(idx)].sum(1), vis[:, list(idx)].sum(1)[:, None]) for g, idx in KEYPOINT_GROUPS.items()}
        seq["visible"] = int(vis.sum())
        seq["pck"] = _ratio(ok.sum((0, 1)), vis.sum())
        seq["pck_groups"] = {g: _ratio(ok[:, list(idx)].sum((0, 1)), vis[:, list(idx)].sum()) for g, idx in KEYPOINT_GROUPS.items()}
    out["sequence"] = seq
    return out


def summarise_mesh_score(sums, within=None, *, num_verts, num_points=0, thresholds=()):
    """From MeshObjective.score (smalfit_mesh_score) to the figures a 3-D fit is reported in, float64, per mesh.
    sums (N,2,3) = per direction [sum d, sum d^2, max d] (0: fitted vertex -> target surface over num_verts vertices, 1: target
    point -> fitted surface over num_points points); within (N,2,T) = queries with d <= thresholds[t], or None.  Device
    tensors or arrays.  num_points = 0: direction 1 was not asked for -- every figure that needs it is nan.  -> dict:
        vert_mean, vert_rms, vert_max, point_mean, point_rms, point_max (N,)
        hausdorff (N,)    the larger of the two maxima
        chamfer_l2 (N,)   the sum of the two mean squared distances
        precision (N,T)   share of the fitted vertices within t;  recall (N,T)  share of the target points within t
        fscore (N,T)      their harmonic mean, 0 when both are 0
        batch: {meshes, the means over the meshes of the above (rms: root of the mean square; max, hausdorff: the maximum),
                worst_mesh: the index of the largest hausdorff (of vert_max for one direction)}"""
    s = _host(sums).astype(np.float64).reshape(-1, 2, 3)
    N, T = len(s), len(thresholds)
    w = np.zeros((N, 2, T), np.int64) if within is None else _host(within).astype(np.int64).reshape(N, 2, T)
    counts = np.array([float(num_verts), float(num_points)])
    out = {}
    for d, name in enumerate(("vert", "point")):
        out[name + "_mean"] = _ratio(s[:, d, 0], counts[d])
        out[name + "_rms"] = np.sqrt(_ratio(s[:, d, 1], counts[d]))
        out[name + "_max"] = s[:, d, 2] if counts[d] > 0 else np.full(N, np.nan)
    out["hausdorff"] = np.maximum(out["vert_max"], out["point_max"])          # nan without the second direction
    out["chamfer_l2"] = _ratio(s[:, 0, 1], counts[0]) + _ratio(s[:, 1, 1], counts[1])
    prec, rec = _ratio(w[:, 0], counts[0]), _ratio(w[:, 1], counts[1])
    out["precision"], out["recall"] = prec, rec
    with np.errstate(invalid="ignore", divide="ignore"):
        out["fscore"] = np.where(prec + rec > 0, 2.0 * prec * rec / np.where(prec + rec > 0, prec + rec, 1.0),
                                 np.where(np.isnan(prec + rec), np.nan, 0.0))

    def mean(x):
        return x.mean(0) if N else np.full(x.shape[1:], np.nan)
    batch = dict(meshes=N)
    for name in ("vert", "point"):
        batch[name + "_mean"] = mean(out[name + "_mean"])
        batch[name + "_rms"] = np.sqrt(mean(out[name + "_rms"] ** 2))
        batch[name + "_max"] = out[name + "_max"].max() if N else np.nan
    batch["hausdorff"] = out["hausdorff"].max() if N else np.nan
    batch["chamfer_l2"] = mean(out["chamfer_l2"])
    for k in ("precision", "recall", "fscore"):
        batch[k] = mean(out[k])
    key = out["hausdorff"] if num_points > 0 else out["vert_max"]
    batch["worst_mesh"] = int(np.argmax(key)) if N else -1
    out["batch"] = batch
    return out


_MESH_ROW_KEYS = ("vert_mean", "vert_rms", "vert_max", "point_mean", "point_rms", "point_max", "hausdorff", "chamfer_l2",
                  "precision", "recall", "fscore")


def mesh_score_report(summary, thresholds, names):
    """the document fitter_3d writes as metrics.json: thresholds, one row per mesh keyed by its name, the batch figures"""
    meshes = {name: {k: summary[k][i] for k in _MESH_ROW_KEYS} for i, name in enumerate(names)}
    return _plain(dict(thresholds=[float(t) for t in thresholds], meshes=meshes, batch=summary["batch"]))


def mesh_score_line(summary, thresholds):
    """one line for a log: the batch figures"""
    b = summary["batch"]
    text = "%d mesh(es): vertex->target mean %.5f max %.5f" % (b["meshes"], b["vert_mean"], b["vert_max"])
    if not np.isnan(b["point_mean"]):
        text += "  target->surface mean %.5f max %.5f  Hausdorff %.5f" % (b["point_mean"], b["point_max"], b["hausdorff"])
        text += "".join("  F@%g %.4f" % (float(t), f) for t, f in zip(thresholds, np.atleast_1d(b["fscore"])))
    return text


def _plain(x):
    """numpy -> what json writes; nan stays nan (json's NaN literal, which json.load reads back)"""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        return [_plain(v) for v in x.tolist()]
    if isinstance(x, (np.floating, np.integer)):
        return x.item()
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def report(summary, thresholds, filenames):
    """the document written as metrics.json: thresholds, one row per frame keyed by file name, the sequence figures"""
    frames = {}
    for i, name in enumerate(filenames):
        row = {k: summary[k][i] for k in ("iou", "intersection", "union", "rendered", "target")}
        if "pck" in summary:
            row.update(visible=summary["visible"][i], correct=summary["correct"][i], pck=summary["pck"][i],
                       pck_groups={g: v[i] for g, v in summary["pck_groups"].items()})
        frames[name] = row
    return _plain(dict(thresholds=[float(t) for t in thresholds], frames=frames, sequence=summary["sequence"]))


def write_report(path, summary, thresholds, filenames):
    with open(path, "w") as fh:
        json.dump(report(summary, thresholds, filenames), fh, indent=1)


def summary_line(summary, thresholds):
    """one line for a log: the sequence figures"""
    seq = summary["sequence"]
    text = "IoU %.4f over %d frame(s)" % (seq["iou"], seq["frames_with_iou"])
    if "pck" in seq:
        text += "  " + "  ".join("PCK@%g %.4f" % (float(t), p) for t, p in zip(thresholds, np.atleast_1d(seq["pck"])))
        text += "  (%d visible keypoints)" % seq["visible"]
    return text

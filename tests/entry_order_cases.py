"""The acts of tests/test_gpu_entry_order.py: every entry point that takes an engine handle, as a named function
(engine) -> {name: numpy array}; further down, the acts of tests/test_gpu_mesh_entry_order.py on a mesh objective.  Importing this
module needs no GPU (tests/test_entry_order_cpu.py reads the table and the
inputs); calling an act does.

An act builds its inputs from fixed seeds (host arrays made once per process, SCENES / AUX below; device tensors afresh in
every call, every output buffer filled with SENTINEL first, so an output nobody wrote shows), makes ONE library call -- or one
short fixed group: a setter, a call and the setter back; a forward and its backward -- through smalify_amd.engine /
FusedFitter, and returns every output the caller can see plus status() and, where a silhouette forward ran, the
face_list_lengths it left.

Two scenes, both tests/parity_cases.make_problem_cpu(M, 64, 3, ...):
  X   seed 21, z 1.45: the side view, a large animal (1252 / 953 / 1711 / 1374 target pixels at M = 4)
  Y   seed 33, z 0.0:  the head-on view with more than K = 100 candidate faces at a pixel (249 / 325 / 253 / 213 pixels)
Their target silhouettes overlap with an IoU of 0.14 .. 0.18 per frame: the depth cache one leaves is foreign to the other.

ACTS maps name -> Act(fn, kind, calls): kind 'eval' / 'rows' / 'render' are the single evaluations and renders that are also
held to the foreign-cache bars (no reset before them); `calls` names the C entry points the act reaches, which
tests/test_entry_order_cpu.py sets against smalify_amd._lib.SIGNATURES."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from oracle import smal_oracle as so
from smalify_amd import _lib
from smalify_amd import config as cfg
from smalify_amd import model_io, synthetic
from tests import parity_cases as pc

S = 64
MAX_FRAMES = 8
WINDOW = 3
SENTINEL = -777.25
SCENE_ARGS = {"X4": (4, 21, 1.45), "X1": (1, 21, 1.45), "Y8": (8, 33, 0.0), "Y3": (3, 33, 0.0)}
ALL = ("betas", "log_beta_scales", "global_rotation", "joint_rotations", "trans")
SHARD = dict(frame_offset=2, total_frames=9)       # frames 2 .. 5 of 9 with windows of 3: both ends cut a window
LIMIT_WEIGHT = 40.0
RGB = (0.3, 0.6, 0.9)
THRESHOLDS = (0.15, 0.05)

_SCENES = {}
_AUX = {}


def scene(name):
    """-> dict(cur, tg, verts (M,V,3) float32 world vertices at the evaluated pose, pts (M,25,3), proj (M,25,2)): host arrays"""
    if name not in _SCENES:
        M, seed, z = SCENE_ARGS[name]
        _, cur, tg = pc.make_problem_cpu(M, S, WINDOW, seed=seed, z=z)
        _, om = pc.get_oracle_model()
        theta = np.concatenate([cur["global_rotation"][:, None], cur["joint_rotations"]], 1)
        with torch.no_grad():
            vo, jo, _, _ = so.smal_forward(om, torch.from_numpy(np.tile(cur["betas"], (M, 1))).double(), torch.from_numpy(theta).double(),
                                           torch.from_numpy(np.tile(cur["log_beta_scales"], (M, 1))).double())
            t = torch.from_numpy(cur["trans"]).double()[:, None]
            pts = (jo + t)[:, so.CANONICAL].float()
            proj = so.project_points(pts.double(), S).float()
        rs = np.random.RandomState(seed + 100)
        halos = [np.concatenate([cur["global_rotation"][i] + 0.03, cur["joint_rotations"][i].reshape(-1) - 0.02, cur["trans"][i] + 0.01])
                 for i in (0, M - 1)]
        _SCENES[name] = dict(M=M, cur=cur, tg=tg, verts=(vo + t).float().numpy(), pts=pts.numpy(), proj=proj.numpy(),
                             dsil=rs.randn(M, S, S).astype(np.float32), halo_prev=halos[0].astype(np.float32),
                             halo_next=halos[1].astype(np.float32))
    return _SCENES[name]


def aux():
    """the inputs of the acts that take no scene (LBS, pose prior): host arrays"""
    if not _AUX:
        md, _ = pc.get_oracle_model()
        rs = np.random.RandomState(5)
        M = 3
        theta = (0.3 * rs.randn(M, 35, 3)).astype(np.float32)
        theta[0, 3:] = 0.0
        with torch.no_grad():
            Rs = so.rodrigues(torch.from_numpy(theta).double().reshape(-1, 3)).reshape(M, 35, 3, 3).float().numpy()
        _AUX.update(beta=(0.5 * rs.randn(M, 20)).astype(np.float32), theta=theta, Rs=np.ascontiguousarray(Rs),
                    logscale=(0.2 * rs.randn(M, 6)).astype(np.float32), wv=rs.randn(M, md.num_verts, 3).astype(np.float32),
                    wj=rs.randn(M, 41, 3).astype(np.float32), v_offset=(0.01 * rs.randn(M, md.num_verts, 3)).astype(np.float32),
                    prior_x=(0.2 * rs.randn(4, 105)).astype(np.float32), prior_dout=rs.randn(4, 105).astype(np.float32))
    return _AUX


def all_inputs():
    """every host array an act reads, flat: {path: array} (the determinism check of tests/test_entry_order_cpu.py)"""
    out = {}
    for name in SCENE_ARGS:
        sc = scene(name)
        for k, v in sc.items():
            if isinstance(v, dict):
                out.update({"%s/%s/%s" % (name, k, kk): np.asarray(vv) for kk, vv in v.items()})
            elif isinstance(v, np.ndarray):
                out["%s/%s" % (name, k)] = v
    out.update({"aux/" + k: v for k, v in aux().items()})
    return out


# ---- the engine ---------------------------------------------------------------------------------------------------------
def new_engine(device_model=None):
    """the engine of every act: the stand-in model, 8 frames of 64 x 64, the synthetic priors (parity_cases.get_engine's)"""
    from smalify_amd import engine as eng
    e = eng.Engine(pc.get_model()[2] if device_model is None else device_model, MAX_FRAMES, S)
    e.set_pose_prior(*synthetic.synthetic_pose_prior())
    e.set_shape_prior(*synthetic.synthetic_shape_prior())
    return e


def _host(e, M=0, **tensors):
    """the outputs on the host, with the engine's status bits (the read synchronises the stream) and, for M > 0, the lengths of the
    candidate lists the silhouette forward of these M frames left"""
    out = {}
    if M:
        out["face_list_lengths"] = e.face_list_lengths(M).cpu().numpy()
    out["status"] = np.array([e.status()], np.int32)
    for k, v in tensors.items():
        if v is not None:
            out[k] = v.detach().cpu().numpy().copy()
    return out


def _full(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL if dtype == torch.float32 else 77, dtype=dtype, device="cuda")


def _stage(stage):
    W = np.array(cfg.OPT_WEIGHTS).T
    return W[stage][:6].copy(), float(W[stage][6]), float(W[stage][8])


# ---- fit_eval forms -----------------------------------------------------------------------------------------------------------
def _eval_kwargs(name, stage=2, want=ALL, outs=("sil_out", "proj_out", "verts_out"), subject=False, u8=False, per_frame=False,
                 shard=False, w_limit=None):
    """-> (keyword arguments of Engine.fit_eval with fresh device tensors, {output name: tensor})"""
    sc = scene(name)
    M, cur, tg = sc["M"], sc["cur"], sc["tg"]
    V = pc.get_oracle_model()[0].v_template.shape[0]
    weights, w_temp, _ = _stage(stage)
    if w_limit is not None:
        weights[4] = w_limit
    vis = tg["vis"]
    if stage == 0:
        vis = so.stage0_visibility(torch.from_numpy(vis).double()).numpy().astype(np.float32)
    p = {k: pc.dev(v) for k, v in cur.items()}
    if subject:                                   # every frame its own subject: its own betas and limb scales
        p["betas"] = pc.dev(np.tile(cur["betas"], (M, 1)))
        p["log_beta_scales"] = pc.dev(np.tile(cur["log_beta_scales"], (M, 1)))
    tsil = pc.dev(tg["tsil"])
    if u8:
        tsil = torch.round(tsil * 255.0).to(torch.uint8).contiguous()
    shapes = dict(sil_out=(M, S, S), proj_out=(M, 25, 2), verts_out=(M, V, 3))
    o = {k: _full(*shapes[k]) for k in outs}
    o["losses"] = _full(9)
    grads = {k: torch.full_like(p[k], SENTINEL) for k in want}
    o.update({"g_" + k: g for k, g in grads.items()})
    kw = dict(p, target_joints=pc.dev(tg["tj"]), target_visibility=pc.dev(vis), target_sil=tsil, weights=weights, w_temp=w_temp,
              window=1 if subject else WINDOW, temporal=not subject, subject_frames=int(subject), want=want, losses=o["losses"],
              grads=grads, **{k: o[k] for k in outs})
    if per_frame:
        kw["losses_per_frame"] = o["losses_per_frame"] = _full(M, 9)
    if shard:
        kw.update(SHARD, halo_prev=pc.dev(sc["halo_prev"]), halo_next=pc.dev(sc["halo_next"]))
    return kw, o


def _eval(name, **how):
    def act(e):
        kw, o = _eval_kwargs(name, **how)
        e.fit_eval(**kw)
        return _host(e, scene(name)["M"] if "sil_out" in o else 0, **o)
    return act


def _rows(name, **how):
    def act(e):
        kw, o = _eval_kwargs(name, **how)
        W = e.num_windows(scene(name)["M"], WINDOW)
        o["window_losses"], o["window_g_betas"], o["window_g_log_beta_scales"] = _full(W, 9), _full(W, 20), _full(W, 6)
        e.fit_eval_windows(window_losses=o["window_losses"],
                           window_grads=dict(betas=o["window_g_betas"], log_beta_scales=o["window_g_log_beta_scales"]), **kw)
        return _host(e, scene(name)["M"], **o)
    return act


def _with_option(e):
    e.set_option(e.OPT_UNCLAMPED_EDGE_T, 1)
    try:
        return _eval("X4")(e)
    finally:
        e.set_option(e.OPT_UNCLAMPED_EDGE_T, 0)


def _with_limits(e):
    e.set_joint_limits(*model_io.joint_limit_table())
    try:
        return _eval("X4", w_limit=LIMIT_WEIGHT)(e)
    finally:
        e.clear_joint_limits()


# ---- fit_run -----------------------------------------------------------------------------------------------------------------
def _fitter(e, name="X4"):
    from smalify_amd import fitter as fit
    sc = scene(name)
    cur, tg = sc["cur"], sc["tg"]
    f = fit.FusedFitter(e, tg["tj"], tg["vis"], tg["tsil"], WINDOW, True, cur["betas"], cur["log_beta_scales"])
    for k in ("global_rotation", "joint_rotations", "trans"):
        f.p[k].copy_(pc.dev(cur[k]))
    f.begin_stage(2)
    return f


def _fitter_state(e, f, **more):
    return _host(e, f.N, flat=f.flat, grad=f.grad, exp_avg=f.exp_avg, exp_avg_sq=f.exp_avg_sq, losses=f.losses, **more)


def _run(iterations):
    def act(e):
        f = _fitter(e)
        weights, w_temp, lr = _stage(2)
        f.run_iterations(weights, w_temp, lr, 2, iterations)
        return _fitter_state(e, f)
    return act


def refused_layout(M=4):
    """the layout of _run_refused as tests/fold_forms.plan_fold takes it: FusedFitter's flat buffer, every tensor trained, the
    gradient of `trans` written to a buffer of its own -> (logscale_mode, offsets, ranges, grad_at_offset)"""
    offs = {"betas": 0, "log_beta_scales": 20, "joint_rotations": 26, "global_rotation": 26 + 102 * M, "trans": 26 + 105 * M}
    return 1, offs, [(0, 26 + 108 * M)], {k: k != "trans" for k in offs}


def _run_refused(e):
    """three iterations on a layout plan_fold refuses (the gradient of `trans` goes elsewhere): the plain chain runs; Adam steps
    `trans` by what its own gradient range holds, zeros"""
    from smalify_amd import engine as eng
    f = _fitter(e)
    weights, w_temp, lr = _stage(2)
    weights[4] = 0.0
    names = f.trainable(2)
    g_trans = torch.full_like(f.g["trans"], SENTINEL)
    a, _, _, keep = e.build_fit_args(
        betas=f.p["betas"], log_beta_scales=f.p["log_beta_scales"], global_rotation=f.p["global_rotation"],
        joint_rotations=f.p["joint_rotations"], trans=f.p["trans"], target_joints=f.target_joints, target_visibility=f.visibility_full,
        target_sil=f.target_sil, weights=weights, w_temp=w_temp, window=WINDOW, global_mask=f.global_mask, rotation_mask=f.rotation_mask,
        losses=f.losses, grads=dict(f.g, trans=g_trans), want=names)
    aa = eng.make_adam_args(f.flat, f.grad, f.exp_avg, f.exp_avg_sq, f._segments(names), lr)
    e.fit_run(a, aa, 3)
    out = _fitter_state(e, f, g_trans=g_trans)
    del keep
    return out


def _run_graph(e):
    """three iterations replayed from one captured iteration, on a side stream (a capture cannot run on the default stream)"""
    weights, w_temp, lr = _stage(2)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    e.set_graph(True)
    try:
        with torch.cuda.stream(side):
            f = _fitter(e)
            f.run_iterations(weights, w_temp, lr, 2, 3)
            side.synchronize()
            out = _fitter_state(e, f)
    finally:
        e.set_graph(False)
    torch.cuda.synchronize()
    return out


def _local_step(e):
    f = _fitter(e)
    weights, w_temp, lr = _stage(2)
    record = _full(f.num_shared() + 216)
    f.local_step(weights, w_temp, lr, 2, record)
    return _fitter_state(e, f, record=record)


# ---- renderer, metrics --------------------------------------------------------------------------------------------------------
def _render_forward(name, want_sil=True):
    def act(e):
        sc = scene(name)
        verts = pc.dev(sc["verts"])
        sil, proj = e.render_forward(verts, pc.dev(sc["pts"]), want_sil=want_sil)
        return _host(e, sc["M"] if want_sil else 0, sil=sil, proj=proj, verts_in=verts)
    return act


def _render_backward(e):
    sc = scene("X4")
    verts = pc.dev(sc["verts"])
    sil, _ = e.render_forward(verts)
    dverts = e.render_backward(verts, sil, pc.dev(sc["dsil"]))
    return _host(e, sc["M"], sil=sil, g_verts=dverts, verts_in=verts)


def _render_color(e):
    return _host(e, image=e.render_color(pc.dev(scene("X4")["verts"]), RGB))


def _fit_metrics(e):
    sc = scene("X4")
    out = e.fit_metrics(pc.dev(sc["verts"]), pc.dev(sc["tg"]["tsil"]), pc.dev(sc["proj"]), pc.dev(sc["tg"]["tj"]), pc.dev(sc["tg"]["vis"]),
                        thresholds=THRESHOLDS, want_mask=True)
    return _host(e, **out)


# ---- LBS, priors --------------------------------------------------------------------------------------------------------------
def _lbs_forward(e):
    a = aux()
    v, j, Rs, vs = e.lbs_forward(pc.dev(a["beta"]), pc.dev(a["theta"]), pc.dev(a["logscale"]))
    return _host(e, verts=v, joints=j, Rs=Rs, v_shaped=vs)


def _lbs_backward_offset(e):
    a = aux()
    db, dt, dl, doff = e.lbs_backward(pc.dev(a["beta"]), pc.dev(a["theta"]), pc.dev(a["logscale"]), pc.dev(a["wv"]), pc.dev(a["wj"]),
                                      v_offset=pc.dev(a["v_offset"]))
    return _host(e, g_beta=db, g_theta=dt, g_logscale=dl, g_v_offset=doff)


def _lbs_backward_matrices(e):
    a = aux()
    db, dRs, dl = e.lbs_backward(pc.dev(a["beta"]), pc.dev(a["Rs"]), pc.dev(a["logscale"]), pc.dev(a["wv"]), pc.dev(a["wj"]))
    return _host(e, g_beta=db, g_Rs=dRs, g_logscale=dl)


def _pose_prior(e):
    from smalify_amd import engine as eng
    a = aux()
    x = pc.dev(a["prior_x"])
    return _host(e, residual=eng.pose_prior(e, x), g_x=eng.pose_prior_backward(e, x, pc.dev(a["prior_dout"])))


def _temporal(e):
    from smalify_amd import engine as eng
    cur = scene("X4")["cur"]
    losses, gg, gj, gt = eng.temporal(e, _stage(2)[1], pc.dev(cur["global_rotation"]), pc.dev(cur["joint_rotations"]), pc.dev(cur["trans"]))
    return _host(e, losses3=losses, g_global_rotation=gg, g_joint_rotations=gj, g_trans=gt)


# ---- refusals: the host's refusal functions answer before any launch -----------------------------------------------------------
def _refused(e, call, **tensors):
    try:
        rc = call()
    except _lib.SmalfitError:
        rc = 1
    return _host(e, refused=torch.tensor([int(rc != 0)], dtype=torch.int32), **tensors)


def _refused_render(e):
    sc = scene("Y8")
    verts = pc.dev(np.concatenate([sc["verts"], sc["verts"][:1]]))                 # 9 frames on an engine of 8
    return _refused(e, lambda: e.render_forward(verts) and 0)


def _refused_rows(e):
    from smalify_amd import engine as eng
    kw, o = _eval_kwargs("X4")
    a, _, _, keep = e.build_fit_args(**kw)
    r = _lib.WindowRows()
    o["window_losses"] = _full(MAX_FRAMES, 9)
    r.num_windows, r.losses = e.num_windows(4, WINDOW) + 1, o["window_losses"].data_ptr()
    fn = _lib.resolve(e.lib, "smalfit_fit_eval_windows")
    out = _refused(e, lambda: fn(e.handle, eng._stream(), C.byref(a), C.byref(r)), **o)
    del keep
    return out


def _refused_graph_subject(e):
    from smalify_amd import engine as eng
    kw, o = _eval_kwargs("X4", subject=True, outs=())
    a, _, _, keep = e.build_fit_args(**kw)
    flat = torch.zeros(64, device="cuda")
    aa = eng.make_adam_args(flat, flat, flat, flat, [(0, 20)], 1e-3)
    e.set_graph(True)
    try:
        out = _refused(e, lambda: e.fit_run(a, aa, 2) or 0, **o)
    finally:
        e.set_graph(False)
    del keep
    return out


Act = collections.namedtuple("Act", "fn kind calls")
EVAL, ROWS, RUN = ("smalfit_fit_eval",), ("smalfit_fit_eval_windows",), ("smalfit_fit_run",)
READS = ("smalfit_engine_status", "smalfit_engine_face_list_lengths")              # every act ends with them

ACTS = collections.OrderedDict([
    # fit_eval forms
    ("eval X4", Act(_eval("X4"), "eval", EVAL)),
    ("eval Y8", Act(_eval("Y8"), "eval", EVAL)),
    ("eval X1", Act(_eval("X1"), "eval", EVAL)),
    ("eval stage 0", Act(_eval("X4", stage=0, want=("global_rotation", "trans"), outs=("proj_out", "verts_out")), "eval", EVAL)),
    ("eval no gradient", Act(_eval("X4", want=()), "eval", EVAL)),
    ("eval per frame", Act(_eval("X4", per_frame=True), "eval", EVAL)),
    ("eval subjects", Act(_eval("X4", subject=True), "eval", EVAL)),
    ("eval subjects per frame", Act(_eval("X4", subject=True, per_frame=True), "eval", EVAL)),
    ("eval shard", Act(_eval("X4", shard=True), "eval", EVAL)),
    ("eval u8", Act(_eval("X4", u8=True), "eval", EVAL)),
    # window rows
    ("rows", Act(_rows("X4"), "rows", ROWS)),
    ("rows per frame", Act(_rows("X4", per_frame=True), "rows", ROWS)),
    # fit_run
    ("run 1", Act(_run(1), "run", RUN)),
    ("run 3", Act(_run(3), "run", RUN)),
    ("run 4", Act(_run(4), "run", RUN)),
    ("run refused fold", Act(_run_refused, "run", RUN)),
    ("run graph", Act(_run_graph, "run", RUN + ("smalfit_engine_set_graph",))),
    # renderer and others
    ("render Y3", Act(_render_forward("Y3"), "render", ("smalfit_render_forward",))),
    ("render points only", Act(_render_forward("X4", want_sil=False), "other", ("smalfit_render_forward",))),
    ("render backward", Act(_render_backward, "render", ("smalfit_render_forward", "smalfit_render_backward"))),
    ("render color", Act(_render_color, "other", ("smalfit_render_color",))),
    ("fit metrics", Act(_fit_metrics, "other", ("smalfit_fit_metrics",))),
    # LBS
    ("lbs forward", Act(_lbs_forward, "other", ("smalfit_lbs_forward_ex",))),
    ("lbs backward v_offset", Act(_lbs_backward_offset, "other", ("smalfit_lbs_backward_ex",))),
    ("lbs backward matrices", Act(_lbs_backward_matrices, "other", ("smalfit_lbs_backward_ex",))),
    ("pose prior", Act(_pose_prior, "other", ("smalfit_pose_prior", "smalfit_pose_prior_backward"))),
    ("temporal", Act(_temporal, "other", ("smalfit_temporal",))),
    ("local step", Act(_local_step, "run", ("smalfit_shard_local_step",))),
    # settings and refusals
    ("option unclamped", Act(_with_option, "setting", EVAL + ("smalfit_engine_set_option",))),
    ("joint limits", Act(_with_limits, "setting", EVAL + ("smalfit_engine_set_joint_limits", "smalfit_engine_clear_joint_limits"))),
    ("refused render", Act(_refused_render, "refusal", ("smalfit_render_forward",))),
    ("refused rows", Act(_refused_rows, "refusal", ROWS)),
    ("refused graph subjects", Act(_refused_graph_subject, "refusal", RUN + ("smalfit_engine_set_graph",))),
])
NAMES = tuple(ACTS)
CACHED = tuple(n for n, a in ACTS.items() if a.kind in ("eval", "rows", "render"))     # held to the foreign-cache bars too

# what the harness itself calls on the engine around the acts
HARNESS_CALLS = ("smalfit_engine_create", "smalfit_engine_destroy", "smalfit_engine_set_pose_prior", "smalfit_engine_set_shape_prior",
                 "smalfit_engine_reset_raster_cache") + READS

# entry points with an engine handle that no act reaches, each with its reason
EXCLUDED = {
    "smalfit_engine_profile_begin": "times sections with events and forces the plain chain; tests/test_gpu_fold_step.py runs a profiled run against the folded loop",
    "smalfit_engine_profile_end": "the other half of the profile pair",
    "smalfit_lbs_forward": "the positional spelling of smalfit_lbs_forward_ex: the binding calls the _ex form only",
    "smalfit_lbs_backward": "the positional spelling of smalfit_lbs_backward_ex: the binding calls the _ex form only",
    "smalfit_shard_run": "needs a communicator's all-gather callback; tests/test_gpu_sharded.py runs it across processes",
}


# ==================================================================================================================================
# the 3-D handle: acts on one MeshObjective (tests/test_gpu_mesh_entry_order.py).  No call leaves a cache for the next one on this
# handle, so every act is held to a fresh objective's bits only.
# ==================================================================================================================================
MESH_V = 130                   # the ribbon of tests/mesh_score_cases.py: three blocks of 64 queries, the last partial
MESH_POINTS = 70               # the objective's capacity: one block of queries and a partial one
MESH_BATCHES = collections.OrderedDict([("one 7", (7,)), ("one 513", (513,)), ("ragged", (1, 513, 7))])      # target faces per mesh
MESH_WEIGHTS = (1.0, 1.0, 0.01, 0.1)
MESH_THRESHOLDS = (0.01, 0.1, 1.0)
MESH_CHAMFER_GATES = dict(max_dist_point=0.6, max_dist_vert=0.6, min_cos_point=0.0)
MESH_ROBUST = dict(sigma_chamfer_point=0.2, sigma_chamfer_vert=0.2, sigma_surface_point=0.25, sigma_surface_vert=0.25)
MESH_SURFACE_FORMS = collections.OrderedDict([
    ("plain", dict()),
    ("compatibility", dict(gates=dict(min_cos_vert=0.0, min_cos_point=0.0), normals=True)),
    ("truncation", dict(gates=dict(max_dist_vert=0.3, max_dist_point=0.3))),
    ("boundary", dict(gates=dict(reject_boundary=True))),
    ("all gates", dict(gates=dict(min_cos_vert=0.2, min_cos_point=0.2, max_dist_vert=0.3, max_dist_point=0.3, reject_boundary=True),
                       normals=True)),
    ("robust", dict(robust=MESH_ROBUST)),
    ("correspondences", dict(correspondences=True)),
    ("gated robust correspondences", dict(gates=dict(max_dist_vert=0.3), robust=MESH_ROBUST, correspondences=True)),
])
_MESH = {}


def mesh_faces():
    from tests import mesh_score_cases as mc
    return mc.ribbon(MESH_V, 1)[1]


def mesh_batch(name):
    """-> dict(meshes [(verts, faces)], lbs (N,V,3), trans (N,3), deform (N,V,3), fit (N,V,3) = their sum's stand-in for the
    calls that take finished vertices, points (N,MESH_POINTS,3) near the targets, normals (N,MESH_POINTS,3)): host arrays"""
    if name not in _MESH:
        from tests import mesh_score_cases as mc
        from tests import scan_index_cases as sic
        meshes = [sic.target(F) for F in MESH_BATCHES[name]]
        N = len(meshes)
        rs = np.random.RandomState(40 + N + len(meshes[0][1]))
        base = mc.ribbon(MESH_V, 1)[0]
        lbs = (base[None] + 0.05 * rs.randn(N, MESH_V, 3)).astype(np.float32)
        trans = (0.02 * rs.randn(N, 3)).astype(np.float32)
        deform = (0.002 * rs.randn(N, MESH_V, 3)).astype(np.float32)
        points = np.stack([mc.points_near(m[0], m[1], MESH_POINTS, 50 + n) for n, m in enumerate(meshes)]).astype(np.float32)
        normals = np.stack([sic.unit_normals(MESH_POINTS, 60 + n) for n in range(N)])
        _MESH[name] = dict(meshes=meshes, lbs=lbs, trans=trans, deform=deform, fit=(lbs + trans[:, None] + deform).astype(np.float32),
                           points=np.ascontiguousarray(points), normals=normals)
    return _MESH[name]


def mesh_inputs():
    out = {}
    for name in MESH_BATCHES:
        b = mesh_batch(name)
        out.update({"%s/%s" % (name, k): v for k, v in b.items() if isinstance(v, np.ndarray)})
        for n, (v, f) in enumerate(b["meshes"]):
            out["%s/target%d/verts" % (name, n)], out["%s/target%d/faces" % (name, n)] = v, f
    return out


class MeshHandles:
    """the targets of every batch, linear and indexed: made once per module (targets are read-only for every act)"""

    def __init__(self):
        from smalify_amd import engine as eng
        self.targets = {}
        for name in MESH_BATCHES:
            v, f = [m[0] for m in mesh_batch(name)["meshes"]], [m[1] for m in mesh_batch(name)["meshes"]]
            self.targets[name, "linear"] = eng.MeshTargets(v, f)
            self.targets[name, "indexed"] = eng.MeshTargets(v, f).build_index()


def new_objective():
    from smalify_amd import engine as eng
    return eng.MeshObjective(MESH_V, mesh_faces(), 3, MESH_POINTS)


def _mesh_host(o):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in o.items()}


def _mesh_eval(batch, S, form):
    def act(obj, handles):
        b = mesh_batch(batch)
        N = len(b["meshes"])
        weights = MESH_WEIGHTS if form != "chamfer off" else (0.0,) + MESH_WEIGHTS[1:]
        points = pc.dev(b["points"][:, :S]) if form != "chamfer off" else None
        out = {k: _full(*shape) for k, shape in (("losses", (5,)), ("verts", (N, MESH_V, 3)), ("dverts", (N, MESH_V, 3)), ("dtrans", (N, 3)))}
        kw = {}
        if form == "gated":
            kw = dict(chamfer_gates=MESH_CHAMFER_GATES, point_normals=pc.dev(b["normals"][:, :S]), targets=handles.targets[batch, "linear"])
        if form == "robust":
            kw = dict(robust=MESH_ROBUST)
        return _mesh_host(obj.eval(pc.dev(b["lbs"]), pc.dev(b["trans"]), pc.dev(b["deform"]), points, weights, out=out, **kw))
    return act


def _mesh_score(batch, S, index, thresholds):
    def act(obj, handles):
        b = mesh_batch(batch)
        return _mesh_host(obj.score(pc.dev(b["fit"]), handles.targets[batch, index], pc.dev(b["points"][:, :S]) if S else None, thresholds))
    return act


def _mesh_surface(batch, S, index, form):
    def act(obj, handles):
        b = mesh_batch(batch)
        how = MESH_SURFACE_FORMS[form]
        return _mesh_host(obj.surface(pc.dev(b["fit"]), handles.targets[batch, index], pc.dev(b["points"][:, :S]), 0.5, 1.0,
                                      correspondences=how.get("correspondences", False), gates=how.get("gates"),
                                      point_normals=pc.dev(b["normals"][:, :S]) if how.get("normals") else None, robust=how.get("robust")))
    return act


def _mesh_acts():
    acts = collections.OrderedDict()
    for batch in MESH_BATCHES:
        for S in (MESH_POINTS, 1):
            for form, entry in (("chamfer", "smalfit_mesh_objective_eval"), ("gated", "smalfit_mesh_objective_eval_gated"),
                                ("robust", "smalfit_mesh_objective_eval_robust")):
                acts["eval %s, %s, S=%d" % (form, batch, S)] = Act(_mesh_eval(batch, S, form), "mesh", (entry,))
        acts["eval chamfer off, %s" % batch] = Act(_mesh_eval(batch, 0, "chamfer off"), "mesh", ("smalfit_mesh_objective_eval",))
        for S, index, thr in ((0, "linear", MESH_THRESHOLDS), (MESH_POINTS, "indexed", MESH_THRESHOLDS), (1, "linear", ()),
                              (MESH_POINTS, "linear", ())):
            acts["score %s, S=%d, %s, %d thresholds" % (batch, S, index, len(thr))] = Act(_mesh_score(batch, S, index, thr), "mesh",
                                                                                         ("smalfit_mesh_score",))
        for form, how in MESH_SURFACE_FORMS.items():
            entry = "smalfit_mesh_surface_eval" + ("_robust" if "robust" in how else "_gated" if "gates" in how else "")
            for S, index in ((MESH_POINTS, "linear"), (1, "indexed")) + (((MESH_POINTS, "indexed"), (1, "linear")) if form == "plain" else ()):
                acts["surface %s, %s, S=%d, %s" % (form, batch, S, index)] = Act(_mesh_surface(batch, S, index, form), "mesh", (entry,))
    return acts


MESH_ACTS = _mesh_acts()
MESH_NAMES = tuple(MESH_ACTS)
# what tests/test_gpu_mesh_entry_order.py calls besides the acts: the handle itself, and the fused step through three Stages
MESH_HARNESS_CALLS = ("smalfit_mesh_objective_create", "smalfit_mesh_objective_destroy", "smalfit_mesh_objective_counts",
                      "smalfit_fit3d_step", "smalfit_fit3d_step_surface", "smalfit_fit3d_step_gated", "smalfit_fit3d_step_partial",
                      "smalfit_fit3d_step_robust")

"""The frame-sharded step in ONE process (no GPU import here): every contiguous split of a short clip, a simulator of
ShardedFitter.step's protocol with the collective replaced by a stack of the ranks' records, the references of the two shard
kernels and the case tables of tests/test_shard_cases_cpu.py (host) and tests/test_gpu_shard_step.py (-m gpu).

RankSim drives one local fitter per shard through what smalify_amd/distributed.py does per iteration: every rank's local step
writes its record (partial shared gradient | boundary frames after the step), the records are stacked into the gather buffer every
rank would receive, every rank reduces that buffer in rank order and steps the shared parameters, and the halos of the next
iteration are views of the buffer.  With FusedFitters these are exactly the launches a real world enqueues (smalfit_shard_local_step,
smalfit_shard_reduce_step) on the same bytes; with the float64 OracleLocalFitter below it is the generic branch of
ShardedFitter.step (evaluate / apply_adam / shared_grad / boundary_records), which proves the simulator on the CPU."""
from __future__ import annotations

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
SHARED_NAMES = ("betas", "log_beta_scales")
RECORD_TAIL = 216                      # masked pose (105) | translation (3) of a shard's first and of its last frame


def splits(N):
    """all 2^(N-1) ways to cut N frames into contiguous non-empty shards, each a list of (lo, hi)"""
    out = []
    for cut in range(1 << (N - 1)):
        edges = [0] + [i + 1 for i in range(N - 1) if cut >> i & 1] + [N]
        out.append([(edges[i], edges[i + 1]) for i in range(len(edges) - 1)])
    return out


def split_name(split):
    return "+".join(str(hi - lo) for lo, hi in split)


def split_of(sizes):
    lo, out = 0, []
    for n in sizes:
        out.append((lo, lo + n))
        lo += n
    return out


# ------------------------------------------------------------------------------------------------
# the float64 oracle behind the local-fitter protocol (tests/test_distributed_cpu.py runs it over gloo)
# ------------------------------------------------------------------------------------------------
class OracleLocalFitter:
    """FusedFitter protocol on top of oracle.smal_oracle for frames [lo, hi) of a problem."""

    def __init__(self, prob_full, params_full, lo, hi, window):
        from oracle import smal_oracle as so
        self.so = so
        m = prob_full.m
        self.prob = so.FitProblem(m, prob_full.S, prob_full.tj[lo:hi].numpy(), prob_full.vis[lo:hi].numpy(),
                                  prob_full.sil[lo:hi].numpy(), prob_full.pose_prec.numpy(), prob_full.pose_mean.numpy(),
                                  prob_full.pose_mask.numpy(), prob_full.shape_prec.numpy(), prob_full.shape_mean.numpy(),
                                  window, True, frame_offset=lo, total_frames=prob_full.N)
        self.N = hi - lo
        self.p = {k: (v[lo:hi].clone() if v.shape[0] == prob_full.N and v.dim() > 1 else v.clone())
                  for k, v in params_full.items()}
        self.grads = {}
        self.halo_prev = self.halo_next = None
        self.losses = torch.zeros(8, dtype=torch.float64)
        self._shared = torch.zeros(26, dtype=torch.float64)

    def trainable(self, stage_id):
        return self.so.trainable_names(stage_id)

    def begin_stage(self, stage_id):
        self.opt = None
        self.stage_id = stage_id

    def boundary_records(self):
        idx = [0, self.N - 1]
        return torch.cat([self.p["global_rotation"][idx], self.p["joint_rotations"][idx].reshape(2, 102),
                          self.p["trans"][idx]], 1).contiguous()

    def shared_grad(self):
        return self._shared

    def evaluate(self, weights, w_temp, stage_id, want=None):
        so = self.so
        names = self.trainable(stage_id) if want is None else want
        leaf = {k: v.detach().clone().requires_grad_(k in names) for k, v in self.p.items()}
        total, _ = so.epoch_loss(self.prob, leaf, weights, w_temp)

        def pair(a, b):       # temporal terms of one adjacent pair, a = (theta 105 | trans 3) records
            return w_temp * (((a[:3] - b[:3]) ** 2).mean() + ((a[3:105] - b[3:105]) ** 2).mean()
                             + ((a[105:] - b[105:]) ** 2).mean())

        def rec(i):
            return torch.cat([leaf["global_rotation"][i], leaf["joint_rotations"][i].reshape(102), leaf["trans"][i]])

        if self.halo_next is not None:
            total = total + pair(rec(self.N - 1), self.halo_next)
        if self.halo_prev is not None:
            total = total + pair(self.halo_prev, rec(0))
        total.backward()
        self.grads = {k: leaf[k].grad for k in names}
        if "betas" in self.grads:
            self._shared = torch.cat([self.grads["betas"], self.grads["log_beta_scales"]]).contiguous()
        return self.losses

    def apply_adam(self, names, lr, advance=True):   # the oracle's Adam counts steps per tensor
        so = self.so
        if self.opt is None:
            self.opt = so.Adam(so.PARAM_ORDER, lr=lr)
        if "betas" in names:
            self.grads["betas"], self.grads["log_beta_scales"] = self._shared[:20].clone(), self._shared[20:].clone()
        self.opt.step(self.p, {k: self.grads[k] for k in names})


# ------------------------------------------------------------------------------------------------
# the simulator
# ------------------------------------------------------------------------------------------------
class RankSim:
    """one local fitter per shard, in rank order; step() is one iteration of ShardedFitter.step on every rank with the
    all-gather replaced by a copy of the ranks' payload rows into the buffer every rank would receive.

    After every step: .losses (each rank's loss vector, copied), .gather (the (world, ns + 216) buffer the ranks reduced and
    their halos point into), .params() (each rank's parameters)."""

    def __init__(self, fitters, generic=None):
        """generic: drive the evaluate / apply_adam / shared_grad / boundary_records protocol (the last branch of
        ShardedFitter.step) even when the fitters have local_step / shared_step; default: whatever the fitters offer"""
        self.fitters = list(fitters)
        self.world = len(self.fitters)
        self.generic = (not hasattr(self.fitters[0], "local_step")) if generic is None else bool(generic)
        self.gather = self.payload = None
        self.losses = []

    def begin_stage(self, stage_id):
        for f in self.fitters:
            f.begin_stage(stage_id)

    def _set_halos(self, ns):
        """ShardedFitter._set_halos on every rank: views of the gather buffer, no copies"""
        rec = self.gather[:, ns:].view(self.world, 2, 108)
        for r, f in enumerate(self.fitters):
            f.halo_prev = rec[r - 1, 1] if r > 0 else None
            f.halo_next = rec[r + 1, 0] if r + 1 < self.world else None

    def start(self):
        """the initial gather of boundary_records() into the persistent buffer (ShardedFitter.run_iterations before its first
        iteration): rows hold zeros in the shared part, the boundary frames of the start state behind it"""
        f0 = self.fitters[0]
        if self.generic:
            sg = f0.shared_grad()
            ns, like = sg.numel(), dict(dtype=sg.dtype, device=sg.device)
        else:
            ns, like = f0.num_shared(), dict(dtype=torch.float32, device=f0.flat.device)
        self.payload = torch.zeros(self.world, ns + RECORD_TAIL, **like)
        self.gather = torch.zeros(self.world, ns + RECORD_TAIL, **like)
        for r, f in enumerate(self.fitters):
            self._fill_boundary(f, self.payload[r, ns:])
        self.gather.copy_(self.payload)
        self._set_halos(ns)
        return ns

    @staticmethod
    def _fill_boundary(f, out):
        try:
            f.boundary_records(out=out)
        except TypeError:                                   # fitters without the `out` fast path
            out.copy_(f.boundary_records().reshape(-1).to(out.dtype))

    def step(self, weights, w_temp, lr, stage_id):
        ns = self.start() if self.gather is None else self.gather.shape[1] - RECORD_TAIL
        fs = self.fitters
        if not self.generic:
            for r, f in enumerate(fs):
                f.local_step(weights, w_temp, lr, stage_id, self.payload[r])
            self.losses = [f.losses.clone() for f in fs]
            self.gather.copy_(self.payload)                 # the all-gather: every rank receives the same rows in rank order
            for f in fs:
                f.shared_step(self.gather, self.world, lr, stage_id)
            self._set_halos(ns)
            return self.losses
        names = fs[0].trainable(stage_id)
        local = tuple(k for k in names if k not in SHARED_NAMES)
        shared = tuple(k for k in names if k in SHARED_NAMES)
        for r, f in enumerate(fs):
            f.evaluate(weights, w_temp, stage_id, want=names)
            if local:
                f.apply_adam(local, lr)
            self.payload[r, :ns].copy_(f.shared_grad())
            self._fill_boundary(f, self.payload[r, ns:])
        self.losses = [f.losses.clone() for f in fs]
        self.gather.copy_(self.payload)
        if shared:
            for f in fs:
                sg = f.shared_grad()
                torch.sum(self.gather[:, :ns], dim=0, out=sg)        # what ShardedFitter.step does on every rank
                f.apply_adam(shared, lr, advance=not local)
        self._set_halos(ns)
        return self.losses

    def params(self):
        return [{k: v.detach().clone() for k, v in f.p.items()} for f in self.fitters]


# ------------------------------------------------------------------------------------------------
# references of the two kernels
# ------------------------------------------------------------------------------------------------
def rank_ordered_sum_f32(rows):
    """the documented contract of the cross-rank sum ("add the partial gradients in rank order"): a float32 accumulator that
    starts at 0 and adds the rows left to right, one rounding per add"""
    rows = np.asarray(rows, np.float32)
    acc = np.zeros(rows.shape[1:], np.float32)
    for r in range(rows.shape[0]):
        acc = (acc + rows[r]).astype(np.float32)
    return acc


def sum_f64(rows):
    return np.asarray(rows, np.float64).sum(0)


def sum_bound(rows):
    """the standard bound of a sequential float32 sum of W terms, per element: (W - 1) eps32 sum_r |x_r|"""
    rows = np.asarray(rows, np.float64)
    return (rows.shape[0] - 1) * EPS32 * np.abs(rows).sum(0)


def record_reference(ns, shared_grad, grot, jrot, trans, gmask, rmask):
    """shard_record_kernel: shared_grad[:ns], then for frame 0 and frame M-1  grot * gmask | jrot * rmask | trans.  Every product
    is ONE float32 multiply, so numpy float32 gives the exact bits."""
    f = lambda a: np.asarray(a, np.float32)                                    # noqa: E731
    grot, jrot, trans = f(grot).reshape(-1, 3), f(jrot).reshape(-1, 102), f(trans).reshape(-1, 3)
    gmask, rmask = f(gmask).reshape(3), f(rmask).reshape(102)
    out = [f(shared_grad).reshape(-1)[:ns]]
    for n in (0, grot.shape[0] - 1):
        out += [grot[n] * gmask, jrot[n] * rmask, trans[n]]
    return np.concatenate(out).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# part A: cases of the two kernels
# ------------------------------------------------------------------------------------------------
RECORD_NUM_SHARED = (0, 20, 26, 40, 41, 300)       # the record is ns + 216 floats: 40 and 41 put it at and one past a 256-thread block
RECORD_NUM_FRAMES = (1, 2, 5)


def record_case(ns, M, seed=211):
    """random parameters with one -0.0 and one denormal, masks of exact zeros and ones in mixed positions"""
    rs = np.random.RandomState(seed + 7 * ns + M)
    sg = rs.randn(max(ns, 1)).astype(np.float32)
    grot, jrot, trans = (rs.randn(M, k).astype(np.float32) for k in (3, 102, 3))
    gmask = np.array([1.0, 0.0, 1.0], np.float32)
    rmask = (rs.rand(102) < 0.7).astype(np.float32)
    rmask[:4] = (1.0, 0.0, 1.0, 0.0)
    # frame 0 and frame M - 1 both carry the special values, under a one and under a zero of the mask
    for n in {0, M - 1}:
        jrot[n, 0], jrot[n, 1] = -0.0, -0.0
        jrot[n, 2], jrot[n, 3] = 1e-41, -1e-41                  # float32 denormals
        grot[n, 0] = -0.0
        trans[n, 1] = 1e-41
    return dict(shared_grad=sg, grot=grot, jrot=jrot, trans=trans, gmask=gmask, rmask=rmask)


# (world, num_shared, stride: "ns" | "record" | "padded", num_trainable: "0" | "20" | "ns", step)
# every value of every axis appears; the first row holds all four corners at once (world 1, stride ns, nothing trained, step 0)
REDUCE_WORLDS, REDUCE_NUM_SHARED, REDUCE_STEPS = (1, 2, 3, 8, 64), (20, 26, 256, 257), (0, 1, 999)
REDUCE_STRIDES, REDUCE_TRAINED = ("ns", "record", "padded"), ("0", "20", "ns")
REDUCE_CASES = (
    (1, 26, "ns", "0", 0),
    (2, 26, "record", "ns", 0),
    (3, 26, "record", "20", 1),
    (8, 20, "record", "ns", 999),
    (64, 257, "padded", "ns", 1),
    (8, 256, "ns", "20", 0),
    (3, 257, "padded", "0", 999),
    (1, 20, "record", "20", 1),
    (2, 256, "padded", "ns", 999),
    (64, 26, "ns", "20", 0),
    (3, 20, "ns", "ns", 0),
    (1, 257, "ns", "0", 1),
)


def reduce_stride(ns, kind):
    return {"ns": ns, "record": ns + RECORD_TAIL, "padded": ns + RECORD_TAIL + 37}[kind]


def reduce_trained(ns, kind):
    return {"0": 0, "20": 20, "ns": ns}[kind]


def cancellation_rows(world, a=3.0e4, b=1.0e-4):
    """(world, 2) float32 columns holding +a, -a and b with |b| below half an ulp of |a| (zeros on further ranks); the float64 sum
    of both is b.  Column 0, ranks (a, -a, b): in rank order a cancels first and b survives, in the reverse order b is absorbed
    and the sum is 0 -- it tells the two orders apart.  Column 1, ranks (a, b, -a): b is absorbed before a cancels, so the
    contract's sum is 0 where a widened accumulator gives b -- it tells float32 from float64.  Needs world >= 3."""
    rows = np.zeros((world, 2), np.float32)
    rows[:3, 0] = (a, -a, b)
    rows[:3, 1] = (a, b, -a)
    return rows


def reduce_case(world, ns, stride_kind, trained_kind, step, seed=223):
    """-> dict: gathered (world, stride) float32 with NaN in every float beyond column ns; param / exp_avg / exp_avg_sq of
    ns + 40 floats as the kernel finds them (NaN moments at step 0: they must not be read) and as the reference takes them (zeros
    at step 0); `zero`: columns whose rows and moments are all zero (the parameter must keep its bits)"""
    stride, ntrain = reduce_stride(ns, stride_kind), reduce_trained(ns, trained_kind)
    rs = np.random.RandomState(seed + 1000 * world + 10 * ns + step % 7 + len(stride_kind))
    rows = (rs.randn(world, ns) * 10.0 ** rs.uniform(-3, 1, (world, ns))).astype(np.float32)
    if world >= 3:
        rows[:, 3:5] = cancellation_rows(world)
        rows[:, 17:19] = cancellation_rows(world, 7.0e5, -2.5e-2)
    zero = np.zeros(ns, bool)
    zero[[1, 11, ns - 1]] = True
    rows[:, zero] = 0.0
    gathered = np.full((world, stride), np.nan, np.float32)
    gathered[:, :ns] = rows
    n = ns + 40                                                  # the flat buffers go on past the shared parameters
    p = rs.randn(n).astype(np.float32)
    m = (rs.randn(n) * 0.1).astype(np.float32)
    v = (rs.rand(n) * 0.1).astype(np.float32)
    m[:ns][zero], v[:ns][zero] = 0.0, 0.0
    m_in, v_in = m.copy(), v.copy()
    if step == 0:
        m[:ns], v[:ns] = 0.0, 0.0                                # the reference: fresh moments
        m_in[:ns], v_in[:ns] = np.nan, np.nan                    # the kernel: stale ones it must not read
    return dict(world=world, ns=ns, stride=stride, ntrain=ntrain, step=step, rows=rows, gathered=gathered, zero=zero,
                param=p, exp_avg=m, exp_avg_sq=v, exp_avg_in=m_in, exp_avg_sq_in=v_in)


# ------------------------------------------------------------------------------------------------
# part B: local_step is its parts
# ------------------------------------------------------------------------------------------------
LOCAL_STEP_CLIP = dict(frames=8, window=4, shard=(2, 5), seed=31)
LOCAL_STEP_STAGES = (0, 2)
# (name, use_unity_prior, allow_limb_scaling)
LOCAL_STEP_LAYOUTS = (("unity", True, True), ("unity_no_limb_scaling", True, False), ("per_frame_scales", False, True))

# ------------------------------------------------------------------------------------------------
# part C: every cut of a short clip
# ------------------------------------------------------------------------------------------------
CLIP = dict(frames=6, size=64, window=4, seed=31)
SCHEDULE = ((0, 2), (1, 2), (2, 3), (3, 2))                 # all four rows of config.OPT_WEIGHTS
START_STAGE = 2                                              # weights of the one evaluation at the start state (every term on)
VARIANT_SPLITS = {6: ((6,), (1, 1, 1, 1, 1, 1), (1, 4, 1), (3, 3)),
                  5: ((5,), (1, 1, 1, 1, 1), (1, 3, 1), (3, 2))}       # the same four kinds of cut of the 5-frame clip
# name -> what differs from the 32-split run (frames: the first `frames` of the clip)
VARIANTS = {
    "window8_of_5": dict(frames=5, window=8),               # one window spans every rank
    "window1_of_5": dict(frames=5, window=1),               # every frame its own window
    "per_frame_scales": dict(unity=False),                  # 20-dim prior, 20 shared floats, the scales stepped locally
    "no_limb_scaling": dict(allow_limb_scaling=False),      # 20 of the 26 shared floats trained
    "joint_limits": dict(joint_limits=True),
    "masks": dict(masks=True),                              # zeros in both masks: a halo without them changes the temporal term
}


def variant_masks(seed=229):
    rs = np.random.RandomState(seed)
    rmask = (rs.rand(34, 3) < 0.75).astype(np.float32)
    rmask[0], rmask[5] = (1.0, 0.0, 1.0), (0.0, 0.0, 0.0)
    return np.array([1.0, 0.0, 1.0], np.float32), rmask


def clip_problem(frames=None, window=None, unity=True, joint_limits=False):
    """-> (cur, tg, make_prob): start parameters and targets of the first `frames` frames of CLIP (built once), and
    make_prob(dtype) -> the oracle's FitProblem of that clip"""
    from oracle import smal_oracle as so
    from smalify_amd import model_io, synthetic
    from tests import image_batch_cases as ic
    from tests import parity_cases as pc
    key = ("shard_clip",)
    if key not in pc._CACHE:
        pc._CACHE[key] = pc.make_problem_cpu(CLIP["frames"], CLIP["size"], CLIP["window"], seed=CLIP["seed"])
    _, cur, tg = pc._CACHE[key]
    n = CLIP["frames"] if frames is None else frames
    window = CLIP["window"] if window is None else window
    cur = {k: (v[:n].copy() if k not in SHARED_NAMES else v.copy()) for k, v in cur.items()}
    tg = {k: v[:n].copy() for k, v in tg.items()}
    if not unity:                                           # per-frame limb scales: (frames, 6), a different row per frame
        rs = np.random.RandomState(233)
        cur["log_beta_scales"] = (cur["log_beta_scales"][None] + 0.02 * rs.randn(n, 6)).astype(np.float32)
    md, _ = pc.get_oracle_model()
    pp, sp = synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior()
    prec, mean = (sp[0], sp[1]) if unity else ic.shape_prior_20()
    limits = model_io.joint_limit_table() if joint_limits else None

    def make_prob(dtype=torch.float64):
        return so.FitProblem(so.OracleModel(md, dtype=dtype), CLIP["size"], tg["tj"], tg["vis"], tg["tsil"], pp[0], pp[1], pp[2],
                             prec, mean, window, use_unity_prior=unity, dtype=dtype, joint_limits=limits)
    return cur, tg, make_prob


def oracle_names(stage_id, allow_limb_scaling=True):
    from oracle import smal_oracle as so
    return so.trainable_names(stage_id, allow_limb_scaling, scales_trainable_default=False)


def _masked(params, mk):
    return {k: v * mk[k] if k in mk else v for k, v in params.items()}


def oracle_eval(prob, cur, stage_id, masks=None):
    """one evaluation of the oracle at `cur` with the stage's weights, every tensor's gradient -> (terms (9,), {name: gradient})"""
    from oracle import smal_oracle as so
    from smalify_amd import config as cfg
    from tests import value_forms as vf
    W = np.array(cfg.OPT_WEIGHTS).T
    params = {k: torch.from_numpy(np.asarray(v)).to(prob.dtype) for k, v in cur.items()}
    mk = {} if masks is None else {"global_rotation": torch.from_numpy(masks[0]).to(prob.dtype),
                                   "joint_rotations": torch.from_numpy(masks[1]).to(prob.dtype)}
    w = W[stage_id][:6].copy()
    if prob.limits is None:
        w[4] = 0.0
    _, sums, grads = so.loss_and_grads(prob, _masked(params, mk), w, float(W[stage_id][6]), so.PARAM_ORDER)
    grads = {k: (g * mk[k] if k in mk else g).double().numpy() for k, g in grads.items()}
    return np.array([float(sums.get(t, 0.0)) for t in vf.LOSS_NAMES]), grads


def oracle_loop(prob, cur, schedule=SCHEDULE, allow_limb_scaling=True, masks=None):
    """the oracle's unsharded loop over `schedule` in prob.dtype (loss + autograd + Adam, a new Adam per stage, stage 0 on the
    torso keypoints: optimize_to_joints.py:96-137) -> (final parameters as float64 numpy, per iteration: dict(stage, terms (9,),
    params)).  A masked tensor enters the objective as param * mask, so its gradient is the masked value's times the mask."""
    from oracle import smal_oracle as so
    from smalify_amd import config as cfg
    from tests import value_forms as vf
    W = np.array(cfg.OPT_WEIGHTS).T
    params = {k: torch.from_numpy(np.asarray(v)).to(prob.dtype) for k, v in cur.items()}
    mk = {} if masks is None else {"global_rotation": torch.from_numpy(masks[0]).to(prob.dtype),
                                   "joint_rotations": torch.from_numpy(masks[1]).to(prob.dtype)}
    trace = []
    for stage_id, its in schedule:
        names = oracle_names(stage_id, allow_limb_scaling)
        vis0 = so.stage0_visibility(prob.vis) if stage_id == 0 else None
        w = W[stage_id][:6].copy()
        if prob.limits is None:
            w[4] = 0.0
        opt = so.Adam(so.PARAM_ORDER, lr=float(W[stage_id][8]))
        for _ in range(its):
            _, sums, grads = so.loss_and_grads(prob, _masked(params, mk), w, float(W[stage_id][6]), names, visibility=vis0)
            opt.step(params, {k: g * mk[k] if k in mk else g for k, g in grads.items()})
            trace.append(dict(stage=stage_id, terms=np.array([float(sums.get(t, 0.0)) for t in vf.LOSS_NAMES]),
                              params={k: v.double().numpy().copy() for k, v in params.items()}))
    return {k: v.double().numpy().copy() for k, v in params.items()}, trace

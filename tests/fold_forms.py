"""What smalfit_fit_run decides on the host before it launches anything -- a restatement, so that the GPU tests of the folded
optimiser step (tests/test_gpu_fold_step.py) can name the cases that reach each branch and say which path a case must take
at collection time, without a compiler, and tests/test_fold_forms_cpu.py can check both that the case lists reach every branch
and that the restatement answers like the host's own functions (smalify_amd/csrc/smalfit_plan.h, compiled for the host by g++:
tests/host_plan_shim.cpp, tests/host_plan.py).  Nothing here needs a GPU.

  smalfit_plan.h: run_loop (smalfit_fit_run dispatches on it)
      graph switch on, not profiled, iterations >= 2, a stream of the caller's   -> one captured iteration, replayed ("graph")
      iterations >= 2, not profiled, plan_fold accepts                           -> the folded loop ("folded"): iteration it's
                                                                                    gradient assembly + Adam ride in the head launch
                                                                                    of iteration it + 1 (lbs_head_step_kernel)
      otherwise                                                                  -> evaluation, Adam, evaluation, Adam ("plain")
  smalfit_plan.h: plan_fold -- the trainable ranges must be exactly a set of whole parameter tensors whose gradients the
      evaluation writes to the matching ranges of adam.grad; FoldRefusal names the reasons below in the same order
  smalfit_plan.h: shared_route, restore_slot, prior_slot, prior_windows -- where the shared parameters travel
  kernels_lbs_forward.inc: asm_beta_* / asm_ls_* -- the sums over frames behind the shared gradients, in slices and batches
"""
from __future__ import annotations

from . import lbs_forms as lf

TENSORS = ("betas", "log_beta_scales", "global_rotation", "joint_rotations", "trans")      # plan_fold's order k = 0 .. 4
NUM_BETAS = 20                        # kPendingNb: shape directions of the fitter


# ---- which loop -------------------------------------------------------------------------------------------------------
def path(iterations, graph, profiled, default_stream, accepted):
    """'graph', 'folded' or 'plain' for one smalfit_fit_run call; accepted: plan_fold's answer"""
    if graph and not profiled and iterations >= 2 and not default_stream:
        return "graph"
    if iterations >= 2 and not profiled and accepted:
        return "folded"
    return "plain"


def head_step_launches(iterations, graph, profiled, default_stream, accepted):
    """launches of lbs_head_step_kernel in one call: every iteration of the folded loop but the first"""
    return iterations - 1 if path(iterations, graph, profiled, default_stream, accepted) == "folded" else 0


# ---- plan_fold ----------------------------------------------------------------------------------------------------------
def counts(M, logscale_mode):
    """floats per tensor (plan_fold's cnt[]); the limb scales count 6 when shared (mode 1), M * 6 otherwise"""
    return {"betas": NUM_BETAS, "log_beta_scales": 6 if logscale_mode == 1 else M * 6, "global_rotation": M * 3,
            "joint_rotations": M * 102, "trans": M * 3}


def plan_fold(M, logscale_mode, offsets, ranges, grad_at_offset):
    """-> (accepted, {tensor: trained}, reason of a refusal or None).
    offsets: {tensor: its first float's index relative to adam.param} (any integer: a tensor may live outside the flat
    buffer); ranges: [(begin, end)] of the optimiser; grad_at_offset: {tensor: the evaluation writes its gradient to
    adam.grad + offset} (False also where no gradient is asked for).
    Reasons, in the order the host meets them: 'cut' (a range holds part of a tensor), 'gradient' (a trained tensor's gradient
    goes elsewhere), 'alias' (two trained tensors share floats), 'nothing' (no tensor inside any range), 'extra' (the ranges
    hold floats of no trained tensor).

    'cut' never decides alone for tensors that do not alias each other: the floats of a cut tensor that lie inside the range
    belong to no tensor that is wholly inside a range, so 'extra' would refuse the layout too.  It decides alone only where
    an UNTRAINED tensor aliases floats of a trained one (ALIASED_LAYOUT below): not a layout a fit can mean, so no GPU case."""
    train = {k: False for k in TENSORS}
    if M <= 0:
        return False, train, "nothing"
    cnt = counts(M, logscale_mode)
    covered = 0
    done = []
    for k in TENSORS:
        if k == "log_beta_scales" and logscale_mode == 0:
            continue                                     # (the host reads no limb scales: the pointer is not looked at)
        lo = offsets[k]
        inside = touches = False
        for b, en in ranges:
            if b <= lo and lo + cnt[k] <= en:
                inside = True
            elif lo < en and b < lo + cnt[k]:
                touches = True
        if touches:
            return False, {k: False for k in TENSORS}, "cut"
        if not inside:
            continue
        if not grad_at_offset.get(k, False):
            return False, {k: False for k in TENSORS}, "gradient"
        for j in done:
            if offsets[j] < lo + cnt[k] and lo < offsets[j] + cnt[j]:
                return False, {k: False for k in TENSORS}, "alias"
        train[k] = True
        done.append(k)
        covered += cnt[k]
    total = sum(en - b for b, en in ranges)
    if covered == 0:
        return False, {k: False for k in TENSORS}, "nothing"
    if covered != total:
        return False, {k: False for k in TENSORS}, "extra"
    return True, train, None


def layout(M, logscale_mode, order=None, pad=0):
    """{tensor: (offset, count)} of a flat buffer holding the tensors in `order` with `pad` floats after each, and its size.
    The default order is FusedFitter's: betas | log_beta_scales | joint_rotations | global_rotation | trans."""
    order = FITTER_ORDER if order is None else order
    cnt = counts(M, logscale_mode)
    offs, off = {}, 0
    for k in order:
        if k == "log_beta_scales" and logscale_mode == 0:
            continue
        offs[k] = (off, cnt[k])
        off += cnt[k] + pad
    return offs, off


def merged_ranges(offs, names):
    """the optimiser's ranges over the tensors `names`: runs of tensors adjacent in the buffer are one range (FusedFitter._segments)"""
    segs = []
    for o, c in sorted(offs[k] for k in names):
        if segs and segs[-1][1] == o:
            segs[-1][1] = o + c
        else:
            segs.append([o, o + c])
    return [tuple(s) for s in segs]


FITTER_ORDER = ("betas", "log_beta_scales", "joint_rotations", "global_rotation", "trans")


# ---- where the shared parameters travel --------------------------------------------------------------------------------
def shared_travel(iterations):
    """the pending steps of a folded call of `iterations` (one per iteration but the last) as (read, write) of the stepped
    shared parameters (betas, shared limb scales): 'caller' (the flat buffers) or a slot 0 / 1 of the engine's staging.
    A step never writes where it reads -- the launch's other blocks are still reading -- so the first step goes to slot 1,
    and the last one goes home only from the third iteration on."""
    out = []
    for it in range(iterations - 1):
        read = "caller" if it == 0 else it & 1
        write = "caller" if (it and it + 2 == iterations) else (it + 1) & 1
        out.append((read, write))
    return out


def restore_slot(iterations, shared_trained=True):
    """the slot shared_state_restore_kernel copies back to the caller's buffers after the loop, or None: only a call of two
    iterations ends with its only pending step in a slot"""
    return (iterations - 1) & 1 if shared_trained and iterations == 2 else None


def prior_slot(it):
    """the half of the shape prior's gradient buffers evaluation `it` writes (its successor's pending step reads it while the
    successor's own prior block writes the other)"""
    return it & 1


def prior_windows(window, frame_offset, M):
    """windows of the sequence that START among frames [frame_offset, frame_offset + M): the evaluation owns their shape-prior
    term (prior_w = w_betas * this)"""
    return (frame_offset + M + window - 1) // window - (frame_offset + window - 1) // window


# ---- the sums behind the shared gradients ------------------------------------------------------------------------------
ASM_FR, ASM_PA, ASM_LS = 8, 32, 4     # kAsmFr, kAsmPa, kAsmLs: operands a thread holds per batch
BETA_SLICES, LS_SLICES = 12, 32       # slices of the frames (and of the column-block partials) / of the frames
BETA_GROUPS = 8                       # kBetaGroups: frame groups of the shape-blend adjoint


def frame_batches(M):
    """batches of the d/d betas sum over frames: 12 slices x kAsmFr = 96 frames each"""
    return (M + BETA_SLICES * ASM_FR - 1) // (BETA_SLICES * ASM_FR)


def scale_batches(M):
    """batches of the d/d shared limb scales sum: 32 slices x kAsmLs = 128 frames each"""
    return (M + LS_SLICES * ASM_LS - 1) // (LS_SLICES * ASM_LS)


def column_partials(V=lf.NUM_VERTS):
    """nblk_beta * kBetaGroups: column-block partials of d/d betas per direction"""
    return (3 * lf.padded_verts(V) + 255) // 256 * BETA_GROUPS


def partial_batches(V=lf.NUM_VERTS):
    """12 slices x kAsmPa = 384 partials each"""
    n = column_partials(V)
    return (n + BETA_SLICES * ASM_PA - 1) // (BETA_SLICES * ASM_PA)


def empty_slices(M):
    """(frame slices of d/d betas, of d/d limb scales) that hold no frame at all"""
    return max(BETA_SLICES - M, 0), max(LS_SLICES - M, 0)


def step_kernel_forms(M):
    """everything about M frames that changes what the step kernel and its first reader do"""
    return (lf.skin_form(M), frame_batches(M), scale_batches(M), empty_slices(M)[0] > 0, empty_slices(M)[1] > 0, M == 1)


# ---- the case lists of tests/test_gpu_fold_step.py -------------------------------------------------------------------
FRAMES = (1, 4, 5, 11, 12, 31, 32, 96, 97, 128, 129)
FRAME_KS = (3, 4)
KS = (2, 3, 4, 7)                     # the fitter cases
ALL_KS = (2, 3, 4, 6, 7)              # every kind of call: restore | home from slot 1 | from slot 0 | longer, even and odd

_ALL = {0: ("betas", "global_rotation", "joint_rotations", "trans"), 1: TENSORS, 2: TENSORS}


def trainable_sets(logscale_mode):
    """{name: (trained tensors, tensors whose gradient is asked for)} of the engine cases, per logscale_mode"""
    every = _ALL[logscale_mode]
    sets = {"only_" + k: ((k,), (k,)) for k in every}
    if logscale_mode:
        sets["betas_and_scales"] = (("betas", "log_beta_scales"), ("betas", "log_beta_scales"))
        sets["all_but_scales"] = (tuple(k for k in every if k != "log_beta_scales"),) * 2
    sets["all"] = (every, every)
    sets["want_more"] = (("global_rotation", "trans"), every)         # gradients of tensors nobody trains
    return sets


# (name, reason plan_fold must give): tests/test_gpu_fold_step.py builds them with refused_layout()
REFUSED = (("half_of_joint_rotations", "cut"), ("starts_inside_trans", "cut"), ("padding_in_ranges", "extra"),
           ("gradient_elsewhere", "gradient"), ("tensor_outside_buffer", "extra"))


def refused_layout(name, M, logscale_mode=1):
    """-> dict(offs, size, ranges, offsets, grad_at_offset, outside, separate_grad): FusedFitter's buffer with every tensor
    trained, bent in one way.  `offsets` / `grad_at_offset` are plan_fold's arguments; `outside`: tensors living in a buffer
    of their own; `separate_grad`: tensors whose gradient is written to a buffer of its own"""
    pad = 5 if name == "padding_in_ranges" else 0
    offs, size = layout(M, logscale_mode, pad=pad)
    names = [k for k in TENSORS if k in offs]
    ranges = merged_ranges(offs, names)
    offsets = {k: offs[k][0] for k in names}
    gao = {k: True for k in names}
    outside, separate = (), ()
    if name == "half_of_joint_rotations":
        o, _ = offs["joint_rotations"]
        ranges = [(0, o + (M + 1) // 2 * 102), (offs["global_rotation"][0], size)]
    elif name == "starts_inside_trans":
        o, c = offs["trans"]
        ranges = [(0, o), (o + 1, o + c)]
    elif name == "padding_in_ranges":
        ranges = [(0, size)]
    elif name == "gradient_elsewhere":
        separate = ("trans",)
        gao["trans"] = False
    elif name == "tensor_outside_buffer":
        outside = ("global_rotation",)
        offsets["global_rotation"] = -(1 << 20)          # some other allocation: nowhere near the ranges
    else:
        raise KeyError(name)
    return dict(offs=offs, size=size, ranges=ranges, offsets=offsets, grad_at_offset=gao, outside=outside, separate_grad=separate)


# 'cut' deciding alone: betas untrained, their last ten floats aliasing the trained joint rotations (M = 1: 102 floats at 26)
ALIASED_LAYOUT = dict(M=1, logscale_mode=1, ranges=[(26, 128)],
                      offsets={"betas": 16, "log_beta_scales": 0, "joint_rotations": 26, "global_rotation": 128, "trans": 131},
                      grad_at_offset={"joint_rotations": True})

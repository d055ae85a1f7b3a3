// What the host decides before it launches anything, each rule once, as a pure function or a constant: which loop
// smalfit_fit_run runs, whether an optimiser step can ride in the next head launch and where the shared parameters then
// travel, which skinning kernel runs, the geometry of the launches that depends on the problem's size, and which argument
// blocks are refused.  Plain C++17 over include/smalfit.h and the standard library -- no HIP -- so that the library
// (smalfit_launch.inc, smalfit_mesh3d.inc) and the CPU tests (tests/host_plan_shim.cpp, compiled by g++) call the same code.
#pragma once
#include <algorithm>
#include <cstring>

#include "../../include/smalfit.h"

namespace smalfit {

// ------------------------------------------------------------------------------------------------
// constants and geometry
// ------------------------------------------------------------------------------------------------
constexpr int kBetaGroups = 8;         // frame groups of the shape-blend adjoint (dbeta_block) when betas are shared
// The sweep / backward pixel walk runs in float32 (kernels_raster.inc): row = floor((q + 1/2) / bw) keeps a margin of 1 / (2 bw) >= 1/2048
// against an error of ~rows * 2^-22, and byte offsets row * 8 S + 8 col stay below 2^24, for S <= 1024 -- twice the largest size
// the reference uses (config 5: 512).  Larger images are rejected rather than walked inexactly.
constexpr int kMaxImageSize = 1024;
constexpr int kHeadPriorFrames = 16;   // frames per prior block of lbs_head_images_kernel (kPriorFrames of kernels_lbs_forward.inc)
constexpr int kMeshQueries = 64;       // queries per chamfer block (kChamQueries of kernels_mesh3d.inc)
constexpr int kMeshThreads = 256;      // vertices / face pairs per block of the ring and gather kernels (kMeshBlock)

// Vp: the vertex count rounded up to whole blocks of 256 (planar bases, zero padded)
inline int padded_verts(int V) { return (V + 255) / 256 * 256; }
// column blocks of the shape-blend adjoint's partials: 256 floats of the 3 Vp columns each
inline int nblk_beta(int Vp) { return (3 * Vp + 255) / 256; }
inline int beta_groups(bool betas_shared) { return betas_shared ? kBetaGroups : 1; }

// the dbeta partials ride on the chain launch as bx * by * bz workgroups: column blocks x shape sets x frame groups
struct DbetaGrid {
  int bx, by, bz;
  int blocks() const { return bx * by * bz; }
};
inline DbetaGrid dbeta_grid(bool need_beta, int Vp, bool betas_shared, int M) {
  return {need_beta ? nblk_beta(Vp) : 0, betas_shared ? 1 : M, beta_groups(betas_shared)};
}
// rows of nblk_beta * NBall floats the engine keeps for them: per-frame sets and the shared set's groups never coexist, both fit
inline size_t dbeta_rows(int max_frames) { return (size_t)max_frames + kBetaGroups; }

// M-adaptive skinning launch (round 6): the wide matrix-core kernel (64 vertices x 16 frames per workgroup) fills the chip from 64
// frames on; below that its workgroups are too few and too long, and the split form (contraction over four waves, four times the
// workgroups, a third of the chain each) is 5 us faster at 8 frames, 3 us at 16 (profiles/r6_ab_skin_split.txt).  The
// matrix-core kernels work on tiles of 16 frames; below 5 frames the plain kernel wastes less
enum class SkinForm { Plain = 0, Split = 1, Wide = 2 };   // skin_kernel<8> | skin_mfma_split_kernel | skin_mfma_kernel
inline SkinForm skin_form(int M, int Vp) {
  if (M <= 4) return SkinForm::Plain;
  return (Vp / 64) * ((M + 15) / 16) >= 256 ? SkinForm::Wide : SkinForm::Split;
}

// workgroups of the head launch: M pose blocks | shape blocks (256 vertices each, per shape set) | prior blocks (one for the
// shared shape's prior, one per kHeadPriorFrames frames for independent images)
enum class HeadPrior { None = 0, Shared = 1, PerFrame = 2 };
inline int head_shape_blocks(int M, int Vp, bool shape_per_frame) { return Vp / 256 * (shape_per_frame ? M : 1); }
inline int head_prior_blocks(int M, HeadPrior prior) {
  return prior == HeadPrior::None ? 0 : (prior == HeadPrior::Shared ? 1 : (M + kHeadPriorFrames - 1) / kHeadPriorFrames);
}
inline int head_blocks(int M, int Vp, bool shape_per_frame, HeadPrior prior) {
  return M + head_shape_blocks(M, Vp, shape_per_frame) + head_prior_blocks(M, prior);
}

// the kinematic tree is walked root first: every joint's parent precedes it
inline bool parents_ordered(const int* parents, int num_joints) {
  for (int i = 1; i < num_joints; ++i)
    if (!(parents[i] >= 0 && parents[i] < i)) return false;
  return true;
}

// ------------------------------------------------------------------------------------------------
// the kinematic tree's schedule
// ------------------------------------------------------------------------------------------------
// kinematic tree by depth: joints of one level are independent, so the chain and its adjoint take `nlev` steps
// (10 for SMAL) instead of 34.  children lists are in DESCENDING joint order: accumulating a parent's adjoint from its
// children in that order reproduces the summation order of a plain reverse loop over the joints.
constexpr int kTreeMaxPass = 16, kTreeMaxChildren = 4;
struct TreeLevels {
  unsigned char nlev;
  unsigned char lvl_off[36];     // level L owns lvl_joint[lvl_off[L] .. lvl_off[L+1])
  unsigned char lvl_joint[35];
  unsigned char child_off[36];   // joint j owns child_idx[child_off[j] .. child_off[j+1])
  unsigned char child_idx[35];
  // The walks as a flat schedule (round 6): pass k handles up to five joints of one level (a wave = 5 joints x 12 lanes), levels in
  // ascending order.  With it a lane reads its joint / parent / children of EVERY pass before the walk starts (independent loads, one
  // latency) instead of chasing level offset -> joint -> parent -> child list through LDS inside every pass.  `fast` = the tree fits
  // (at most kTreeMaxPass passes, kTreeMaxChildren children per joint: SMAL's needs 12 and 4); deeper / bushier trees take the
  // table-driven loops as before.
  unsigned char fast, npass;
  unsigned char pass_joint[kTreeMaxPass][8];    // [pass][slot 0..4] joint, 255 = idle slot
  unsigned char pass_parent[kTreeMaxPass][8];
  unsigned char pass_nchild[kTreeMaxPass][8];
  unsigned char pass_child[kTreeMaxPass][8][kTreeMaxChildren];   // in the order of child_idx (descending joint index)
};
// -> the schedule of a tree of 35 joints with 0 <= parents[i] < i (parents_ordered; parents[0] is not read)
inline TreeLevels tree_levels(const int* parents) {
  TreeLevels tl;
  std::memset(&tl, 0, sizeof(tl));
  int depth[35] = {0}, maxd = 0;
  for (int i = 1; i < 35; ++i) { depth[i] = depth[parents[i]] + 1; maxd = std::max(maxd, depth[i]); }
  tl.nlev = (unsigned char)(maxd + 1);
  int pos = 0;
  for (int L = 0; L <= maxd; ++L) {
    tl.lvl_off[L] = (unsigned char)pos;
    for (int i = 0; i < 35; ++i) if (depth[i] == L) tl.lvl_joint[pos++] = (unsigned char)i;
  }
  for (int L = maxd + 1; L < 36; ++L) tl.lvl_off[L] = (unsigned char)pos;
  pos = 0;
  for (int j = 0; j < 35; ++j) {
    tl.child_off[j] = (unsigned char)pos;
    for (int c = 34; c >= 1; --c) if (parents[c] == j) tl.child_idx[pos++] = (unsigned char)c;
  }
  tl.child_off[35] = (unsigned char)pos;
  // the flat schedule of the walks (see TreeLevels)
  std::memset(tl.pass_joint, 255, sizeof(tl.pass_joint));
  int np = 0;
  bool fits = true;
  for (int L = 1; L <= maxd; ++L) {
    const int j0 = tl.lvl_off[L], nj = tl.lvl_off[L + 1] - j0;
    for (int base = 0; base < nj; base += 5, ++np) {
      if (np >= kTreeMaxPass) { fits = false; continue; }
      for (int s = 0; s < 5 && base + s < nj; ++s) {
        const int i = tl.lvl_joint[j0 + base + s];
        tl.pass_joint[np][s] = (unsigned char)i;
        tl.pass_parent[np][s] = (unsigned char)parents[i];
        const int nc = tl.child_off[i + 1] - tl.child_off[i];
        if (nc > kTreeMaxChildren) fits = false;
        tl.pass_nchild[np][s] = (unsigned char)std::min(nc, kTreeMaxChildren);
        for (int q = 0; q < std::min(nc, kTreeMaxChildren); ++q) tl.pass_child[np][s][q] = tl.child_idx[tl.child_off[i] + q];
      }
    }
  }
  if (tl.child_off[1] - tl.child_off[0] > 35) fits = false;
  tl.npass = (unsigned char)std::min(np, kTreeMaxPass);
  tl.fast = fits ? 1 : 0;
  return tl;
}
// passes the table-driven walks make (five joints of one level each): what npass would be without its cap
inline int tree_walk_passes(const TreeLevels& tl) {
  int np = 0;
  for (int L = 1; L < tl.nlev; ++L) np += (tl.lvl_off[L + 1] - tl.lvl_off[L] + 4) / 5;
  return np;
}

// ------------------------------------------------------------------------------------------------
// smalfit_model_desc: which models are refused, and which the fitter refuses
// ------------------------------------------------------------------------------------------------
// chain_bwd_kernel reduces d/d betas through the rest joints with one lane per shape direction of one wave: 64 of them
constexpr int kMaxModelBetas = 64;
// the fitter (smalfit_fit_eval and everything built on it) optimises the first 20 shape directions (kPendingNb of kernels_lbs_forward.inc)
constexpr int kFitBetas = 20;
// -> why smalfit_model_create refuses a model of these dimensions (the text behind "smalfit_model_create: "), or nullptr
inline const char* model_dims_refusal(int num_verts, int num_faces, int num_betas) {
  if (num_verts <= 0 || num_faces <= 0 || num_betas <= 0) return "bad dimensions";
  static_assert(kMaxModelBetas == 64, "the message below names the limit");
  if (num_betas > kMaxModelBetas) return "num_betas above 64 is not supported (the rest-joint path of d/d betas reduces 64 shape directions)";
  return nullptr;
}
// -> why the fitter refuses a model of `model_betas` shape directions (the text behind "smalfit_fit_eval: "), or nullptr
inline const char* fit_model_refusal(int model_betas) {
  static_assert(kFitBetas == 20, "the message below names the count");
  return model_betas >= kFitBetas ? nullptr : "the model has fewer than the 20 shape directions the fitter optimises";
}

// the 3D mesh objective: grids over S target points, V vertices, P face pairs
struct MeshGrids { int bx, by, bv, bp; };   // chamfer over the points | over the vertices | ring / gather over vertices | face pairs
inline int mesh_query_blocks(int queries) { return (queries + kMeshQueries - 1) / kMeshQueries; }
inline int mesh_element_blocks(int elements) { return (elements + kMeshThreads - 1) / kMeshThreads; }
inline MeshGrids mesh_grids(int S, int V, int P) {
  return {mesh_query_blocks(S), mesh_query_blocks(V), mesh_element_blocks(V), mesh_element_blocks(P)};
}
inline float mesh_weight(float w) { return std::max(w, 0.f); }                                  // negative weights count as 0
inline int mesh_points(float w_chamfer, int num_points) { return w_chamfer > 0.f ? num_points : 1; }   // chamfer off: a grid of one block's worth, never launched

// ------------------------------------------------------------------------------------------------
// smalfit_fit_args: which blocks are refused
// ------------------------------------------------------------------------------------------------
// struct_size first: with a block laid out by another version of smalfit.h no other field can be trusted (subject_frames sits
// at the block's tail: a block of an older header ends before it)
inline const char* fit_args_size_refusal(const smalfit_fit_args* a) {
  return a->struct_size == (unsigned)sizeof(smalfit_fit_args)
             ? nullptr : "smalfit_fit_args.struct_size does not match this library (built against another smalfit.h?)";
}
inline bool independent_images(const smalfit_fit_args* a) { return a->subject_frames == 1; }
inline int shape_prior_dim(const smalfit_fit_args* a, int engine_dim) { return a->shape_prior_dim > 0 ? a->shape_prior_dim : engine_dim; }
inline bool prior_uses_limb_scales(const smalfit_fit_args* a, int engine_dim) { return a->w_betas > 0.f && shape_prior_dim(a, engine_dim) > 20; }

struct EngineFacts {
  int max_frames;        // the engine's capacity
  bool has_pose_prior;   // smalfit_engine_set_pose_prior was called
  int shape_dim;         // dimension given to smalfit_engine_set_shape_prior, 0: none
};
// -> why smalfit_fit_eval refuses the block (the text behind "smalfit_fit_eval: "), or nullptr
inline const char* fit_args_refusal(const smalfit_fit_args* a, const EngineFacts& e) {
  if (const char* msg = fit_args_size_refusal(a)) return msg;
  const int M = a->num_frames;
  if (M <= 0 || M > e.max_frames) return "num_frames exceeds the engine's max_frames";
  if (a->window <= 0) return "window must be positive";
  if (a->frame_offset < 0) return "frame_offset must be >= 0";
  if (a->total_frames != 0 && a->total_frames < a->frame_offset + M) return "total_frames is smaller than frame_offset + num_frames";
  if (!a->betas || !a->global_rotation || !a->joint_rotations || !a->trans || !a->losses) return "missing parameter / losses pointer";
  if (a->w_j2d > 0.f && (!a->target_joints || !a->target_visibility)) return "keypoint targets missing";
  if (a->w_sil > 0.f && !a->target_sil && !a->target_sil_u8) return "target_sil missing with w_sil > 0";
  if (a->w_pose > 0.f && !e.has_pose_prior) return "pose prior not set";
  if (a->w_betas > 0.f && e.shape_dim <= 0) return "shape prior not set";
  if (a->logscale_mode != 0 && !a->log_beta_scales) return "log_beta_scales missing";
  // independent images: every frame its own subject.  Everything that couples frames is refused, not ignored
  if (a->subject_frames != 0 && a->subject_frames != 1)
    return "subject_frames must be 0 (one subject) or 1 (independent images); clips of K > 1 frames per subject in one batch are not implemented";
  const bool indep = independent_images(a), prior_ls = prior_uses_limb_scales(a, e.shape_dim);
  if (indep) {
    if (a->window != 1) return "subject_frames = 1 needs window = 1 (an image is its own window)";
    if (a->temporal) return "subject_frames = 1 needs temporal = 0 (unrelated images have no neighbours)";
    if (a->logscale_mode == 1) return "subject_frames = 1 takes logscale_mode 0 or 2 (nothing is shared between images)";
    if (a->halo_prev || a->halo_next) return "subject_frames = 1 needs halo_prev = halo_next = NULL";
    if (a->frame_offset != 0 || a->total_frames != 0) return "subject_frames = 1 needs frame_offset = total_frames = 0";
    if (prior_ls && a->logscale_mode != 2) return "a 26-dim shape prior of independent images needs per-frame log_beta_scales (logscale_mode 2)";
  } else if (prior_ls && a->logscale_mode != 1) {
    return "a 26-dim shape prior needs shared log_beta_scales";
  }
  return nullptr;
}

// frames of the whole sequence these M frames belong to
inline int sequence_frames(const smalfit_fit_args* a) { return a->total_frames > 0 ? a->total_frames : a->frame_offset + a->num_frames; }
// The shape prior is evaluated once per window (smal_fitter.py:162-171 inside forward()): an evaluation owns the windows that
// START among its frames [frame_offset, frame_offset + M) -- a shard in the middle of a window owns none of it
inline int prior_windows(int window, int frame_offset, int M) {
  return (frame_offset + M + window - 1) / window - (frame_offset + window - 1) / window;
}

// ------------------------------------------------------------------------------------------------
// smalfit_window_rows: one row per window of the sequence (smalfit_fit_eval_windows)
// ------------------------------------------------------------------------------------------------
// windows of the SEQUENCE that hold at least one of the M frames [frame_offset, frame_offset + M); the first may be one this
// evaluation does not own (prior_windows counts the owned ones)
inline int window_rows_count(int window, int frame_offset, int M) {
  return (frame_offset + M - 1) / window - frame_offset / window + 1;
}
// the engine keeps the rows of an evaluation in its workspace before they are added up: floats per row
constexpr int kWindowRowBetas = 32, kWindowRowScales = 8;
inline const char* window_rows_size_refusal(const smalfit_window_rows* r) {
  return r->struct_size == (unsigned)sizeof(smalfit_window_rows)
             ? nullptr : "smalfit_window_rows.struct_size does not match this library (built against another smalfit.h?)";
}
// -> why smalfit_fit_eval_windows refuses the rows for a block that fit_args_refusal accepts, or nullptr
inline const char* window_rows_refusal(const smalfit_fit_args* a, const smalfit_window_rows* r) {
  if (const char* msg = window_rows_size_refusal(r)) return msg;
  if (!r->losses) return "smalfit_window_rows.losses missing";
  if (a->subject_frames != 0) return "window rows need subject_frames = 0 (independent images already have one row per image)";
  if (a->window <= 0 || a->num_frames <= 0 || a->frame_offset < 0 ||
      r->num_windows != window_rows_count(a->window, a->frame_offset, a->num_frames))
    return "smalfit_window_rows.num_windows is not the number of windows these frames belong to";
  if (r->g_log_beta_scales && a->logscale_mode != 1)
    return "smalfit_window_rows.g_log_beta_scales needs shared log_beta_scales (logscale_mode 1)";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// smalfit_adam_args: the trainable ranges, packed for the segment kernels
// ------------------------------------------------------------------------------------------------
struct AdamSegments {
  int nseg;
  int beg[4];
  int off[5];        // prefix sums of the range lengths; off[nseg] = total
};
// -> why the ranges of `o` are refused, or nullptr with `sg` filled
inline const char* pack_adam_segments(const smalfit_adam_args* o, AdamSegments& sg) {
  if (!o->param || !o->grad || !o->exp_avg || !o->exp_avg_sq) return "smalfit adam: null buffer";
  if (o->num_segments < 0 || o->num_segments > 4) return "smalfit adam: at most 4 segments";
  std::memset(&sg, 0, sizeof(sg));
  sg.nseg = o->num_segments;
  int total = 0;
  for (int k = 0; k < sg.nseg; ++k) {
    if (o->seg_begin[k] < 0 || o->seg_end[k] < o->seg_begin[k]) return "smalfit adam: bad segment";
    sg.beg[k] = o->seg_begin[k];
    sg.off[k] = total;
    total += o->seg_end[k] - o->seg_begin[k];
  }
  for (int k = sg.nseg; k <= 4; ++k) sg.off[k] = total;
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// smalfit_fit_run: the folded optimiser step
// ------------------------------------------------------------------------------------------------
// Can the optimiser step of `o` be folded into the next evaluation's head launch?  Only when the trainable ranges are exactly a
// set of whole parameter tensors of `a` (the ranges of adjacent tensors may be merged) whose gradients the evaluation writes to
// the matching ranges of o->grad: then every trainable float has one known reader (PendingStep).  -> which tensors, and where.
enum class FoldRefusal {
  None = 0,
  Cut,        // a range holds part of a tensor
  Gradient,   // a trained tensor's gradient is not written where Adam reads it
  Alias,      // two trained tensors share floats
  Nothing,    // no tensor inside any range (or nothing to fold at all: no frames, a missing tensor, independent images, whose
              // per-image betas are not folded yet, a tensor off the buffer's float grid)
  Extra,      // the ranges hold floats of no trained tensor
};
struct FoldPlan {
  bool train[5];      // betas, log_beta_scales, global_rotation, joint_rotations, trans
  int off[5];         // their offsets in the flat buffers
  FoldRefusal why;
  bool accepted() const { return why == FoldRefusal::None; }
};
inline FoldPlan plan_fold(const smalfit_fit_args* a, const smalfit_adam_args* o, const AdamSegments& sg) {
  FoldPlan plan{};
  auto refuse = [](FoldRefusal why) { FoldPlan none{}; none.why = why; return none; };
  const int M = a->num_frames;
  if (M <= 0 || !a->betas || !a->global_rotation || !a->joint_rotations || !a->trans) return refuse(FoldRefusal::Nothing);
  if (a->subject_frames != 0) return refuse(FoldRefusal::Nothing);
  const float* ptr[5] = {a->betas, a->logscale_mode ? a->log_beta_scales : nullptr, a->global_rotation, a->joint_rotations, a->trans};
  const float* gptr[5] = {a->g_betas, a->g_log_beta_scales, a->g_global_rotation, a->g_joint_rotations, a->g_trans};
  const long long cnt[5] = {20, a->logscale_mode == 1 ? 6 : (long long)M * 6, (long long)M * 3, (long long)M * 102, (long long)M * 3};
  long long lo[5], covered = 0;
  for (int k = 0; k < 5; ++k) {
    lo[k] = 0;
    if (!ptr[k]) continue;
    const long long bytes = (long long)((const char*)ptr[k] - (const char*)o->param);
    if (bytes % 4) return refuse(FoldRefusal::Nothing);
    lo[k] = bytes / 4;
    bool inside = false, touches = false;
    for (int q = 0; q < sg.nseg; ++q) {
      const long long b = sg.beg[q], en = b + (sg.off[q + 1] - sg.off[q]);
      if (b <= lo[k] && lo[k] + cnt[k] <= en) inside = true;
      else if (lo[k] < en && b < lo[k] + cnt[k]) touches = true;
    }
    if (touches) return refuse(FoldRefusal::Cut);
    if (!inside) continue;
    if (gptr[k] != o->grad + lo[k]) return refuse(FoldRefusal::Gradient);
    for (int j = 0; j < k; ++j)
      if (plan.train[j] && lo[j] < lo[k] + cnt[k] && lo[k] < lo[j] + cnt[j]) return refuse(FoldRefusal::Alias);
    plan.train[k] = true; plan.off[k] = (int)lo[k];
    covered += cnt[k];
  }
  if (covered == 0) return refuse(FoldRefusal::Nothing);
  if (covered != sg.off[sg.nseg]) return refuse(FoldRefusal::Extra);
  return plan;
}

// which loop smalfit_fit_run runs
enum class RunLoop {
  Graph = 0,    // one iteration (tick, the evaluation's kernels, Adam) captured once per (arguments, stream) and replayed
  Folded = 1,   // gradient assembly and Adam of every iteration but the last ride in the NEXT iteration's head launch
  Plain = 2,    // evaluation, Adam, evaluation, Adam
};
inline RunLoop run_loop(bool graph_on, bool profiling, int iterations, bool callers_stream, bool fold_accepted) {
  // a call of one iteration leaves nothing to replay or to hand on; a profiled run keeps the launches its sections name
  const bool repeats = iterations >= 2 && !profiling;
  if (repeats && graph_on && callers_stream) return RunLoop::Graph;   // (a capture needs a stream of the caller's, not the default one)
  if (repeats && fold_accepted) return RunLoop::Folded;
  return RunLoop::Plain;
}

// The shared parameters (betas; the limb scales when one set serves all frames) cannot be stepped in place: the head launch's
// other blocks are still reading them.  They travel through the two slots of smalfit_engine::shstate: the pending step that
// iteration `it` leaves reads where its predecessor wrote -- the first one the caller's buffers -- and writes the other slot;
// from the third iteration on the last pending step (it + 2 == iterations) writes home to the caller's buffers
constexpr int kCaller = -1;                   // in place of a slot: the caller's flat buffers
constexpr int kSharedSlotFloats = 96;         // [value, exp_avg, exp_avg_sq][32: betas 20 | limb scales 6]
constexpr int kSharedSlotBetas = 0, kSharedSlotScales = 20;
inline bool tensor_is_shared(int k, int logscale_mode) { return k == 0 || (k == 1 && logscale_mode == 1); }
struct SharedRoute { int read, write; };      // slot 0 / 1 or kCaller
inline SharedRoute shared_route(int it, int iterations) {
  return {it ? (it & 1) : kCaller, (it && it + 2 == iterations) ? kCaller : ((it + 1) & 1)};
}
// the slot shared_state_restore_kernel copies home after the loop, or kCaller (none): the only pending step of a call of two
// iterations read the caller's buffers, so it could not store there
inline int restore_slot(int iterations, bool shared_trained) { return shared_trained && iterations == 2 ? ((iterations - 1) & 1) : kCaller; }
// the half of the shape prior's gradient buffers evaluation `it` writes (its successor's pending step reads it while the
// successor's own prior block writes the other)
inline int prior_slot(int it) { return it & 1; }

}  // namespace smalfit

// What the host decides before it launches anything, each rule once, as a pure function or a constant: which loop
// smalfit_fit_run runs, whether an optimiser step can ride in the next head launch and where the shared parameters then
// travel, which skinning kernel runs, what an evaluation launches and with which switches (plan_eval), the geometry of the
// launches that depends on the problem's size -- with the constants the kernels decode their block roles by, defined here once --
// which arguments every entry point refuses (the mesh objective's and smalfit_model_create's data checks included), and the shape
// of a smalfit_fit3d_step (plan_fit3d, with the layout of its Adam launch's argument).  Plain C++17 over include/smalfit.h and the
// standard library -- no HIP -- so that the library (smalfit_launch.inc, smalfit_mesh3d.inc) and the CPU tests
// (tests/host_plan_shim.cpp, compiled by g++) call the same code.  Its siblings under the same rule build the host's tables:
// smal_model_pack.h (a model's), mesh3d_topology.h (a mesh objective's and its targets').
#pragma once
#include <algorithm>
#include <cmath>
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
// (the next three still mirror a constant that a kernel file defines under another name, tied by a static_assert where both are
// visible: tests/test_fold_forms_cpu.py pins kPriorFrames's definition in kernels_lbs_forward.inc, and smalfit_mesh3d.inc names
// both halves of the other two pairs.  Every other constant a launch is sized by is defined below, once)
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

// ------------------------------------------------------------------------------------------------
// grids of the fit path with their riders: the host launches what these return, the kernels decode their roles through the same
// functions and constants (constexpr: callable from device code)
// ------------------------------------------------------------------------------------------------
// Frame-to-XCD affinity of the per-frame kernels (kernels_raster.inc: xcd_block): a 1-D grid in which frame n's workgroups land on
// XCD n % 8, so frames are dealt in rounds of eight
constexpr int xcd_frames(int M) { return ((M + 7) / 8) * 8; }
constexpr int xcd_grid(int blocks_per_frame, int M) { return blocks_per_frame * ((M + 7) / 8) * 8; }
// threads per workgroup of every kernel below unless it says otherwise; elementwise launches: one thread per element
constexpr int elem_blocks(long long elements) { return (int)((elements + 255) / 256); }
constexpr int vertex_blocks(int Vp) { return Vp / 256; }
constexpr int rigid_blocks(int count) { return (count + 63) / 64; }           // global_rigid_kernel and its adjoint: one wave per workgroup, a lane per chain
struct Grid2 { int x, y; };
constexpr int color_face_blocks(int F) { return (F + 15) / 16; }             // color_zbuf_kernel: 16 faces per workgroup
// smalfit_fit_metrics: cover_kernel walks the faces as color_zbuf_kernel does; sil_counts_kernel gives a thread kSilCountPixels
// pixels of one frame (one 16-byte read of the mask), 256 threads per slab; pck_kernel one wave per frame
constexpr int kSilCountPixels = 16;
constexpr Grid2 cover_grid(int F, int M) { return Grid2{color_face_blocks(F), M}; }
constexpr int sil_count_slabs(int S) { return ((S * S + kSilCountPixels - 1) / kSilCountPixels + 255) / 256; }
constexpr Grid2 sil_counts_grid(int S, int M) { return Grid2{sil_count_slabs(S), M}; }
constexpr int pck_grid(int M) { return M; }

// skinning: (vertex blocks, frame tiles) of the form skin_form chose
constexpr int kSkinGroups = 2;               // skin_mfma_split_kernel: 16-vertex groups per workgroup (4 waves each): they share the staged transforms of the 16 frames
constexpr int kSkinVerts = 16 * kSkinGroups;       // its vertices per workgroup
constexpr int kSkinThreads = 256 * kSkinGroups;    // and its threads
constexpr Grid2 skin_grid(SkinForm form, int M, int Vp) {
  return form == SkinForm::Wide ? Grid2{Vp / 64, (M + 15) / 16} : form == SkinForm::Split ? Grid2{Vp / kSkinVerts, (M + 15) / 16} : Grid2{Vp / 64, (M + 7) / 8};
}
constexpr int kJointBlocks = 41;             // joints_kernel / the sweep launch's joint riders: one workgroup per regressed joint and frame

// the riders of the sweep launch (until the box launch was folded into the sweep: of face_bbox_kernel, whose grid was
// [frame blocks, a multiple of 8] [face blocks of 256 faces, frame n on XCD n % 8] [joint riders, 41 per frame])
constexpr int box_frame_blocks(int M) { return xcd_frames(M); }
constexpr int box_blocks_per_frame(int F) { return (F + 255) / 256; }
// (box_face_blocks and box_grid have no caller in the library any more: tests/host_plan_shim.cpp and tests/test_host_plan_cpu.py pin them)
constexpr int box_face_blocks(int F, int M) { return xcd_grid(box_blocks_per_frame(F), M); }
constexpr int box_joint_blocks(int M, bool joints) { return joints ? kJointBlocks * M : 0; }
constexpr int box_grid(int F, int M, bool joints) { return box_frame_blocks(M) + box_face_blocks(F, M) + box_joint_blocks(M, joints); }

// workgroup b of an xcd_grid(blocks_per_frame, M) -> its frame (may be >= M: a workgroup of the padding) and its block of that frame
struct XcdBlock { int n, bx; };
constexpr XcdBlock xcd_block_at(int b, int blocks_per_frame) {
  const int xcd = b & 7, slot = b >> 3;
  return XcdBlock{(slot / blocks_per_frame) * 8 + xcd, slot - (slot / blocks_per_frame) * blocks_per_frame};
}

// raster_sweep_kernel: [frame riders, a multiple of 8] [sweep blocks of 32 faces, frame n on XCD n % 8] [joint riders, 41 per frame]
constexpr int kRectFaces = 8;                // faces per entry of the union-box index
constexpr int kSweepFaces = 32;              // faces per sweep block
constexpr int rect_count(int F) { return (F + kRectFaces - 1) / kRectFaces; }
constexpr int sweep_blocks_per_frame(int F) { return (F + kSweepFaces - 1) / kSweepFaces; }
constexpr int sweep_grid(int F, int M) { return xcd_grid(sweep_blocks_per_frame(F), M); }
constexpr int sweep_launch_grid(int F, int M, bool joints) { return box_frame_blocks(M) + sweep_grid(F, M) + box_joint_blocks(M, joints); }
// what workgroup b of that launch does.  Frame: the active region of frame n (n >= M: nothing).  Faces: block bx of frame n
// (n >= M: nothing).  Joint: regressed joint bx of frame n
enum class SweepRole { Frame = 0, Faces = 1, Joint = 2 };
struct SweepBlock { SweepRole role; int n, bx; };
constexpr SweepBlock sweep_block_at(int b, int F, int M) {
  if (b < box_frame_blocks(M)) return SweepBlock{SweepRole::Frame, b, 0};
  const int k = b - box_frame_blocks(M);
  if (k >= sweep_grid(F, M)) return SweepBlock{SweepRole::Joint, (k - sweep_grid(F, M)) / kJointBlocks, (k - sweep_grid(F, M)) % kJointBlocks};
  return SweepBlock{SweepRole::Faces, xcd_block_at(k, sweep_blocks_per_frame(F)).n, xcd_block_at(k, sweep_blocks_per_frame(F)).bx};
}

// raster_resolve_kernel: [loss riders, one per frame, padded to a multiple of 8] [tiles of kResEdge^2 pixels, frame n on XCD n % 8]
constexpr int kResSub = 2;                   // a resolve workgroup takes (16 kResSub)^2 pixels, kResSub^2 per thread: the launch is
                                             // bound by the number of workgroups, not by bytes
constexpr int kResEdge = 16 * kResSub;
constexpr int resolve_tiles_x(int S) { return (S + kResEdge - 1) / kResEdge; }
constexpr int resolve_tiles(int S) { return resolve_tiles_x(S) * resolve_tiles_x(S); }
constexpr int resolve_loss_blocks(int loss_frames) { return loss_frames > 0 ? ((loss_frames + 7) / 8) * 8 : 0; }
constexpr int resolve_grid(int tiles, int M, int loss_frames) { return xcd_grid(tiles, M) + resolve_loss_blocks(loss_frames); }

// raster_band_kernel / raster_select_kernel: persistent grids
constexpr int kBandBlocks = 1536;
constexpr int kSelWaves = 2;                 // waves per select block: 11 KB of LDS per wave -> 7 blocks (14 waves) per CU
constexpr int kSelGroups = 16;               // ticket counters per XCD of the selection kernel (one per group of its workgroups)
constexpr int kSelectBlocks = 1792;          // 7 resident 2-wave blocks x 256 CUs
static_assert(kSelectBlocks % (8 * kSelGroups) == 0, "every ticket group of every XCD needs the same number of selection workgroups (a group without one would leave its pixels undone)");
constexpr int kQueueLossBlocks = kSelectBlocks + kBandBlocks;   // partials of the queue kernels' loss: the select kernel's, then the band kernel's
constexpr int kFrameLossStride = 32;         // unsigned long longs between two frames' counters of the queue kernels' loss

// raster_bwd_kernel
constexpr int kBwdLanes = 16;                // lanes per face of the backward gather
constexpr int kBwdFaces = 4;                 // faces per workgroup
constexpr int raster_bwd_blocks_per_frame(int F) { return (F + kBwdFaces - 1) / kBwdFaces; }
constexpr int raster_bwd_grid(int F, int M) { return xcd_grid(raster_bwd_blocks_per_frame(F), M); }
// 1 / S for its pixel-to-NDC map, divided here once: IEEE division, the bits the device's correctly rounded sequence gave in every wave
inline float raster_bwd_inv_s(int S) { return 1.0f / (float)S; }
// It addresses what a face owns in its frame -- record, box, candidate list, list length, adjoint row -- by an unsigned 32-bit
// byte offset from the frame's base.  The largest is the list's: 128 bytes per face (kListCap of kernels_raster.inc, which
// asserts the product), so a model may have 2^25 faces.  model_dims_refusal turns larger ones away
constexpr int kMaxModelFaces = 1 << 25;

// vertex_bwd_kernel
constexpr int vertex_bwd_grid(int Vp, int M) { return xcd_grid(vertex_blocks(Vp), M); }

// lbs_bwd_mid_kernel: [pose-blend ids] [dA blocks].  Block -> XCD placement of the pose-blend part: the 10 feature-pair blocks of one
// column split read the same columns of dvp: their ids are laid out as chunks of 8 splits x 10 feature pairs with the split in
// the low 3 bits, per chunk of PBM_TILES tiles of 16 frames
constexpr int PBM_SPLITS = 24, PBM_TILES = 4;
static_assert(PBM_SPLITS % 8 == 0, "the blocks of a column split are placed on one XCD (ids in chunks of 8 splits)");
constexpr int mid_pb_ids(int M) { return 10 * PBM_SPLITS * (((M + 15) / 16 + PBM_TILES - 1) / PBM_TILES); }
constexpr int mid_da_ids(int M) { return xcd_grid(35, M); }       // dA blocks: frame n on XCD n % 8 (see vertex_bwd_kernel)
constexpr int mid_grid(int M, int nPB) { return (nPB ? mid_pb_ids(M) : 0) + mid_da_ids(M); }

// chain_bwd_kernel: [M frame blocks] [the dbeta partials' riders]
inline int chain_grid(int M, const DbetaGrid& db) { return M + db.blocks(); }

// assemble_kernel: [one block per shape set] [limb scales] [kAsmElem element blocks] [kAsmLoss loss partials]
constexpr int kAsmElem = 4, kAsmLoss = 16;   // blocks for element-wise gradients / loss partial sums
constexpr int kAsmRows = 4;                  // blocks of frame_loss_rows_kernel
constexpr int asm_shape_sets(int betas_shared, int M) { return betas_shared ? 1 : M; }
constexpr int assemble_grid(int shape_sets) { return shape_sets + 1 + kAsmElem + kAsmLoss; }
constexpr int window_rows_grid(int W) { return W; }                // one block per row
constexpr int frame_loss_rows_grid() { return kAsmRows; }

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
  static_assert(kMaxModelFaces == 33554432, "the message below names the limit");
  if (num_faces > kMaxModelFaces) return "num_faces above 33554432 is not supported (the backward gather addresses a frame's faces by 32-bit byte offsets)";
  static_assert(kMaxModelBetas == 64, "the message below names the limit");
  if (num_betas > kMaxModelBetas) return "num_betas above 64 is not supported (the rest-joint path of d/d betas reduces 64 shape directions)";
  return nullptr;
}
// -> why smalfit_model_create refuses the data of a model whose dimensions model_dims_refusal accepts, or nullptr.  Reads the 35
// parents and the 3 F face indices; `landmarks`: the vertex ids ModelDev carries (kDefaultLandmarks of smal_model_pack.h)
constexpr const char* kParentsRefusal = "parents must satisfy 0 <= parents[i] < i";
inline const char* model_desc_refusal(const smalfit_model_desc* d, const int* landmarks, int num_landmarks) {
  if (!parents_ordered(d->parents, 35)) return kParentsRefusal;
  for (int i = 0; i < d->num_faces * 3; ++i)
    if (d->faces[i] < 0 || d->faces[i] >= d->num_verts) return "face index out of range";
  for (int i = 0; i < num_landmarks; ++i)
    if (landmarks[i] >= d->num_verts) return "model has fewer vertices than the SMAL landmark ids";
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
// the elementwise launches round the objective, 256 threads each: compose over the N V 3 coordinates, the sampler over the S points
// of a mesh (x the meshes), Adam over a trained tensor's floats
inline int mesh_compose_blocks(int N, int V) { return elem_blocks((long long)N * V * 3); }
inline Grid2 mesh_sample_grid(int S, int N) { return Grid2{elem_blocks(S), N}; }
constexpr int fit3d_adam_blocks(int count) { return elem_blocks(count); }
// assemble_kernel with only its per-frame-betas roles (smalfit_lbs_backward_ex, smalfit_fit3d_step): one block per frame
constexpr int frame_betas_grid(int M) { return M; }
// smalfit_mesh_score: mesh3d_surface_dist_kernel takes kMeshQueries queries per block, like the chamfer kernels, and stages the
// scanned triangles kSurfaceChunk records of 64 bytes at a time: 32 KB of LDS, so four blocks (16 waves) share a CU's 160 KB --
// the scan is vector arithmetic (some 95 instructions per pair against four broadcast LDS reads), and four waves per SIMD
// are taken to be enough to cover those reads; a larger chunk would save barriers (one pair per 512 triangles already) and cost residency.
// mesh3d_score_reduce_kernel: one block per (direction, mesh)
constexpr int kSurfaceChunk = 512;
constexpr int kScoreDirections = 2;          // 0: fitted vertex -> target surface, 1: target point -> fitted surface
inline Grid2 surface_dist_grid(int queries, int N) { return Grid2{mesh_query_blocks(queries), N}; }
constexpr Grid2 score_reduce_grid(int N) { return Grid2{kScoreDirections, N}; }
// the surface term (smalfit_mesh_surface_eval, smalfit_fit3d_step_surface) runs every iteration, where the grid above leaves
// three quarters of the CUs idle at one mesh (61 and 47 blocks).  mesh3d_surface_near_kernel keeps the 64 queries and the staged
// chunk and takes a third grid dimension: the scanned triangles in `slices` contiguous spans, whose minima meet in one 64-bit
// (distance bits, face) key per query.  The slice count aims at the 1024 blocks the 256 CUs hold at once (four a CU by the 34 KB
// of LDS: 16 waves, four a SIMD to cover the broadcast LDS reads) without going over them -- a fifth block on some CUs would be a
// tail of a quarter of the launch --, keeps at least kSurfaceMinSlice triangles a slice -- below that the staging and the atomic
// outweigh the scan -- and is rounded so that no slice is empty.  A ragged batch of targets is sliced by its largest mesh; a
// smaller mesh's surplus blocks return before they stage anything.
constexpr int kSurfaceTargetBlocks = 1024;
constexpr int kSurfaceMinSlice = 64;
constexpr int kSurfaceHitChunk = 512;        // SurfaceHit records (48 bytes) staged at a time by mesh3d_surface_grad_kernel: 24 KB
constexpr int surface_slice_span(int faces, int slices) { return (faces + slices - 1) / slices; }   // triangles per slice
inline int surface_slices(int queries, int faces, int N) {
  const long long blocks = std::max(1LL, (long long)mesh_query_blocks(queries) * N);
  long long want = kSurfaceTargetBlocks / blocks;
  want = std::max(1LL, std::min(want, (long long)(faces / kSurfaceMinSlice)));
  const int span = surface_slice_span(faces, (int)want);
  return std::max(1, surface_slice_span(faces, std::max(span, 1)));   // = ceil(faces / span): the last slice starts inside the mesh
}
struct Grid3 { int x, y, z; };
inline Grid3 surface_near_grid(int queries, int faces, int N) { return Grid3{mesh_query_blocks(queries), N, surface_slices(queries, faces, N)}; }
// one query per thread: the winner's barycentrics and residual, per-block sums of d^2
inline Grid2 surface_hit_grid(int queries, int N) { return Grid2{mesh_element_blocks(queries), N}; }
// the term's vertex gradient: 64 vertices per block, one per lane, the same 64 in each of its kSurfaceGradWaves waves, which split
// the staged hits between them (the chamfer kernels' scheme with 16 waves for 4: 61 blocks of 4 waves are a quarter of the chip's
// SIMDs at one mesh, and the gather is as long as a chamfer scan)
constexpr int kSurfaceGradWaves = 16;
inline Grid2 surface_grad_grid(int V, int N) { return Grid2{mesh_query_blocks(V), N}; }
// the vertex direction over targets that carry a scan index (mesh3d_grid.h): one WAVE per query, kScanGridQueries queries per
// 256-thread block -- a query's candidates come in rings of cells, 64 at a time, and ring counts differ from query to query, so a
// lane per query would diverge on every load; no slices, no LDS.  The same grid serves the term's scan and the score's
constexpr int kScanGridQueries = 4;
inline Grid2 scan_grid_near_grid(int V, int N) { return Grid2{(V + kScanGridQueries - 1) / kScanGridQueries, N}; }
inline Grid2 scan_grid_dist_grid(int V, int N) { return scan_grid_near_grid(V, N); }
// -> why smalfit_mesh_targets_build_index refuses (the text behind "smalfit_mesh_targets_build_index: "), or nullptr; reads the
// num_floats coordinates of the handle's target vertices
struct ScanIndexFacts {
  const float* verts;
  size_t num_floats;
};
inline const char* scan_index_args_refusal(const smalfit_scan_index_args* a, const ScanIndexFacts& f) {
  if (a->struct_size != (unsigned)sizeof(smalfit_scan_index_args))
    return "smalfit_scan_index_args.struct_size does not match this library (built against another smalfit.h?)";
  if (!(std::isfinite(a->cell_scale) && a->cell_scale >= 0.f)) return "cell_scale must be finite and >= 0 (0: the library's own)";
  for (size_t i = 0; i < f.num_floats; ++i)
    if (!std::isfinite(f.verts[i])) return "scan index needs finite target vertices";
  return nullptr;
}
inline const char* scan_index_stats_refusal(const smalfit_scan_index_stats* out, bool has_index, int mesh, int num_meshes) {
  if (!out) return "null argument";
  if (out->struct_size != (unsigned)sizeof(smalfit_scan_index_stats))
    return "smalfit_scan_index_stats.struct_size does not match this library (built against another smalfit.h?)";
  if (!has_index) return "the targets have no scan index (smalfit_mesh_targets_build_index)";
  if (mesh < 0 || mesh >= num_meshes) return "mesh out of range";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// the mesh objective's entry points: which arguments are refused (the text behind "<entry point>: " or nullptr, the first fault;
// handles and pointers are asked for as null_argument_refusal / null_handle_refusal before these read a capacity)
// ------------------------------------------------------------------------------------------------
inline const char* null_handle_refusal(bool given) { return given ? nullptr : "null handle"; }
inline const char* mesh_objective_create_refusal(bool given, int max_meshes, int max_points) {
  if (!given) return "null argument";
  return max_meshes > 0 && max_points > 0 ? nullptr : "max_meshes and max_points must be positive";
}
inline const char* mesh_eval_refusal(int num_meshes, int max_meshes, float w_chamfer, bool points, int num_points, int max_points) {
  if (num_meshes <= 0 || num_meshes > max_meshes) return "num_meshes out of range";
  if (w_chamfer > 0.f && (!points || num_points <= 0 || num_points > max_points))
    return "the chamfer term needs 1 <= num_points <= max_points target points";
  return nullptr;
}
// (reads the num_meshes counts of both tables)
inline const char* mesh_targets_create_refusal(bool given, int num_meshes, const int* vert_counts, const int* face_counts) {
  if (!given) return "null argument";
  if (num_meshes <= 0) return "no meshes";
  for (int n = 0; n < num_meshes; ++n)
    if (vert_counts[n] <= 0 || face_counts[n] <= 0) return "empty target mesh";
  return nullptr;
}
inline const char* mesh_sample_refusal(bool given, int num_points) {
  if (!given) return "null argument";
  return num_points > 0 ? nullptr : "num_points must be positive";
}
// -> why smalfit_mesh_score refuses the block (the text behind "smalfit_mesh_score: "), or nullptr.  struct_size first: with a
// block laid out by another header no other field can be trusted
struct MeshScoreFacts { int max_meshes, max_points, target_meshes; };   // the objective's capacities, the targets' mesh count
inline const char* mesh_score_args_refusal(const smalfit_mesh_score_args* a, const MeshScoreFacts& f) {
  if (a->struct_size != (unsigned)sizeof(smalfit_mesh_score_args))
    return "smalfit_mesh_score_args.struct_size does not match this library (built against another smalfit.h?)";
  if (a->num_meshes <= 0 || a->num_meshes > f.max_meshes) return "num_meshes exceeds the objective's max_meshes";
  if (a->num_meshes != f.target_meshes) return "number of target meshes differs from num_meshes";
  if (!a->verts || !a->sums) return "verts / sums missing";
  if (!a->points && a->num_points != 0) return "num_points must be 0 without points";
  if (!a->points && a->point_dist) return "point_dist given without points";
  if (a->points && (a->num_points <= 0 || a->num_points > f.max_points)) return "points need 1 <= num_points <= max_points";
  static_assert(SMALFIT_MAX_SCORE_THRESHOLDS == 8, "the message below names the limit");
  if (a->num_thresholds < 0 || a->num_thresholds > SMALFIT_MAX_SCORE_THRESHOLDS) return "num_thresholds must be 0..8";
  for (int t = 0; t < a->num_thresholds; ++t)
    if (!(std::isfinite(a->thresholds[t]) && a->thresholds[t] > 0.f)) return "every threshold must be finite and > 0";
  if (a->num_thresholds == 0 && a->within) return "within given with num_thresholds = 0";
  return nullptr;
}

// ---- the rigid pre-alignment (smalfit_rigid_align; worded in include/smalfit.h) ---------------------------------------------
// rigid_scan_kernel<DIR>: 64 queries a block like the chamfer kernels, x the K starts x the N meshes -- the starts are the
// parallelism one mesh lacks (61 and 47 query blocks at the fitter's size, 24 starts make 2592 of them).  rigid_solve_kernel: one
// wave per (start, mesh).  rigid_init_kernel (means, starts): one block per mesh.  rigid_pick_kernel: one mesh per thread.
constexpr int kRigidMaxIterations = 1000;
constexpr int kRigidMaxMeshes = 65535;          // a launch's largest y / z dimension
constexpr double kRigidStartTolerance = 1e-4;   // how far a caller's float32 start may be from a proper rotation
inline Grid3 rigid_scan_grid(int queries, int K, int N) { return Grid3{mesh_query_blocks(queries), K, N}; }
inline Grid2 rigid_solve_grid(int K, int N) { return Grid2{K, N}; }
constexpr int rigid_init_blocks(int N) { return N; }
inline int rigid_pick_blocks(int N) { return (N + 63) / 64; }
// launches of one call: the init, I + 1 rounds of (a scan per direction that is on, the solve), the pick
inline int rigid_align_launches(int iterations, bool vert_dir, bool point_dir) {
  return 1 + (iterations + 1) * ((vert_dir ? 1 : 0) + (point_dir ? 1 : 0) + 1) + 1;
}
inline const char* rigid_aligner_create_refusal(bool given, int max_meshes, int max_verts, int max_points, int max_starts) {
  if (!given) return "null argument";
  if (max_meshes <= 0 || max_verts <= 0 || max_points <= 0) return "max_meshes, max_verts and max_points must be positive";
  if (max_meshes > kRigidMaxMeshes) return "max_meshes must be at most 65535";   // (the meshes are a grid's z and y dimension)
  static_assert(SMALFIT_MAX_RIGID_STARTS == 64, "the message below names the limit");
  return max_starts >= 1 && max_starts <= SMALFIT_MAX_RIGID_STARTS ? nullptr : "max_starts must be 1..64";
}
// -> why a (3,3) row-major start is no proper rotation (finite, R R^T = I and det R = +1 to within kRigidStartTolerance), or nullptr
inline const char* rigid_start_refusal(const float* R) {
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(R[i])) return "every start must be finite";
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double d = i == j ? -1.0 : 0.0;
      for (int k = 0; k < 3; ++k) d += (double)R[3 * i + k] * (double)R[3 * j + k];
      if (!(std::fabs(d) <= kRigidStartTolerance)) return "every start must be orthonormal to within 1e-4";
    }
  const double det = (double)R[0] * ((double)R[4] * R[8] - (double)R[5] * R[7]) - (double)R[1] * ((double)R[3] * R[8] - (double)R[5] * R[6]) +
                     (double)R[2] * ((double)R[3] * R[7] - (double)R[4] * R[6]);
  return std::fabs(det - 1.0) <= kRigidStartTolerance ? nullptr : "every start must have determinant +1 (a reflection is no start)";
}
// -> why smalfit_rigid_align refuses the block (the text behind "smalfit_rigid_align: "), or nullptr.  struct_size first; reads the
// K host matrices of `starts` when they are given
struct RigidAlignFacts { int max_meshes, max_verts, max_points, max_starts; };   // the handle's capacities
inline const char* rigid_align_args_refusal(const smalfit_rigid_align_args* a, const RigidAlignFacts& f) {
  if (a->struct_size != (unsigned)sizeof(smalfit_rigid_align_args))
    return "smalfit_rigid_align_args.struct_size does not match this library (built against another smalfit.h?)";
  if (a->num_meshes < 1 || a->num_meshes > f.max_meshes) return "num_meshes must be 1 .. the aligner's max_meshes";
  if (a->num_verts < 1 || a->num_verts > f.max_verts) return "num_verts must be 1 .. the aligner's max_verts";
  if (a->num_points < 1 || a->num_points > f.max_points) return "num_points must be 1 .. the aligner's max_points";
  if (a->num_starts < 1 || a->num_starts > SMALFIT_MAX_RIGID_STARTS || a->num_starts > f.max_starts)
    return "num_starts must be 1 .. the aligner's max_starts (at most 64)";
  static_assert(kRigidMaxIterations == 1000, "the message below names the limit");
  if (a->iterations < 0 || a->iterations > kRigidMaxIterations) return "iterations must be 0..1000";
  if (!(std::isfinite(a->w_point) && a->w_point >= 0.f && std::isfinite(a->w_vert) && a->w_vert >= 0.f))
    return "w_point and w_vert must be finite and >= 0";
  if (a->w_point == 0.f && a->w_vert == 0.f) return "w_point and w_vert are both 0";
  if (!a->verts || !a->points) return "verts / points missing";
  if (a->starts && a->start_transforms) return "starts and start_transforms are both given";
  static_assert(SMALFIT_NUM_CUBE_ROTATIONS == 24, "the message below names the count");
  if (!a->starts && !a->start_transforms && a->num_starts != SMALFIT_NUM_CUBE_ROTATIONS)
    return "the built-in starts are 24: num_starts must be 24 without starts";
  if (a->starts)
    for (int k = 0; k < a->num_starts; ++k)
      if (const char* msg = rigid_start_refusal(a->starts + 9 * (size_t)k)) return msg;
  if (!a->transforms || !a->scores || !a->best || !a->best_transform || !a->kept_rotation)
    return "transforms / scores / best / best_transform / kept_rotation missing";
  return nullptr;
}
// ---- trimming (smalfit_trimmed_rigid_align) ----
// rigid_trim_kernel: one block of 256 per (direction that is on, start, mesh): selects the threshold key of the round, forms the
// kept pairs' sums into the scan's own slots.  It runs between the scans and the solve of every round
inline Grid3 rigid_trim_grid(bool vert_dir, bool point_dir, int K, int N) { return Grid3{(vert_dir ? 1 : 0) + (point_dir ? 1 : 0), K, N}; }
// launches of one trimmed call: the init, I + 1 rounds of (a scan per direction that is on, the selection, the solve), the pick
inline int rigid_trim_launches(int iterations, bool vert_dir, bool point_dir) {
  return 1 + (iterations + 1) * ((vert_dir ? 1 : 0) + (point_dir ? 1 : 0) + 2) + 1;
}
// -> why smalfit_trimmed_rigid_align refuses the trim block, or nullptr; asked after rigid_align_args_refusal accepted the call's
// own block.  struct_size first, then the range of each keep; a keep of a direction of weight 0 is not read
struct RigidTrimFacts { int num_verts, num_points; bool vert_dir, point_dir; };
inline const char* rigid_trim_args_refusal(const smalfit_rigid_trim_args* t, const RigidTrimFacts& f) {
  if (t->struct_size != (unsigned)sizeof(smalfit_rigid_trim_args))
    return "smalfit_rigid_trim_args.struct_size does not match this library (built against another smalfit.h?)";
  if (f.vert_dir && (t->keep_vert < 1 || t->keep_vert > f.num_verts)) return "keep_vert must be 1 .. num_verts";
  if (f.point_dir && (t->keep_point < 1 || t->keep_point > f.num_points)) return "keep_point must be 1 .. num_points";
  return nullptr;
}
// an accepted block trims: some direction that is on keeps fewer than its count
inline bool rigid_trim_on(const smalfit_rigid_trim_args* t, const RigidTrimFacts& f) {
  return t && ((f.vert_dir && t->keep_vert != f.num_verts) || (f.point_dir && t->keep_point != f.num_points));
}

// -> why smalfit_mesh_surface_eval / smalfit_fit3d_step_surface refuse the surface block (the text behind "<entry point>: "), or
// nullptr.  In a step the vertices and the points are the step's own: the block must carry neither, and what the points need is
// asked of the step's block (step_points: its num_points; step_has_points: its `points` is given)
struct SurfaceTermFacts {
  int max_meshes, max_points;   // the objective's capacities
  bool targets;                 // target meshes were given
  int target_meshes;            // how many (read only with `targets`)
  bool step;                    // the block rides on a smalfit_fit3d_args
  int step_meshes, step_points;
  bool step_has_points;
};
inline bool surface_term_on(const smalfit_surface_term_args* s) { return s && (s->w_point_surface > 0.f || s->w_vert_surface > 0.f); }
inline const char* surface_term_args_refusal(const smalfit_surface_term_args* a, const SurfaceTermFacts& f) {
  if (a->struct_size != (unsigned)sizeof(smalfit_surface_term_args))
    return "smalfit_surface_term_args.struct_size does not match this library (built against another smalfit.h?)";
  if (a->num_meshes <= 0 || a->num_meshes > f.max_meshes) return "num_meshes exceeds the objective's max_meshes";
  if (f.step && a->num_meshes != f.step_meshes) return "num_meshes differs from the step's";
  if (a->w_vert_surface > 0.f) {
    if (!f.targets) return "the vertex-surface term needs the target meshes";
    if (f.target_meshes != a->num_meshes) return "number of target meshes differs from num_meshes";
  }
  if (!a->losses) return "losses missing";
  if (f.step) {
    if (a->verts || a->points) return "verts and points must be NULL in a step: it uses its own";
    if (a->w_point_surface > 0.f) {
      if (f.step_points <= 0 || f.step_points > f.max_points) return "the point-surface term needs 1 <= num_points <= max_points";
      if (!f.step_has_points && !f.targets) return "neither target points nor target meshes given";
      if (!f.step_has_points && f.target_meshes != a->num_meshes) return "number of target meshes differs from num_meshes";
    }
  } else {
    if (!a->verts) return "verts missing";
    if (a->w_point_surface > 0.f && (!a->points || a->num_points <= 0 || a->num_points > f.max_points))
      return "the point-surface term needs 1 <= num_points <= max_points points";
  }
  if (a->point_bary && !a->point_face) return "point_bary given without point_face";
  if (a->vert_bary && !a->vert_face) return "vert_bary given without vert_face";
  if (a->point_residual && !a->point_face) return "point_residual given without point_face";
  if (a->vert_residual && !a->vert_face) return "vert_residual given without vert_face";
  return nullptr;
}

// The gates of the surface term (smalfit_surface_gate_args): what a block switches on, in the form the kernels take it.
// tau^2 and c |c| are formed here, once, in float32; an open truncation is tau2 = +inf (no d^2 exceeds it), an open
// compatibility test is cos_* = false (the scan of that direction is the ungated instantiation and reads no normals)
struct SurfaceGatePlan {
  bool any;                    // some gate is on, or a kept mask is asked for: the gated hit kernels run and count
  bool cos_point, cos_vert;    // the compatibility test of a direction is on
  float cc_point, cc_vert;     // c |c|
  float tau2_point, tau2_vert;
  bool boundary;
};
inline bool surface_gate_dist_on(float tau) { return tau > 0.f && std::isfinite(tau); }
inline bool surface_gate_cos_on(float c) { return c > -1.0f; }
// of a block surface_gate_args_refusal accepts (g may be NULL: everything off); a gate of a skipped direction is off
inline SurfaceGatePlan plan_surface_gates(const smalfit_surface_gate_args* g, bool point_dir, bool vert_dir) {
  SurfaceGatePlan p{};
  p.tau2_point = p.tau2_vert = INFINITY;
  if (!g) return p;
  p.cos_point = point_dir && surface_gate_cos_on(g->min_cos_point);
  p.cos_vert = vert_dir && surface_gate_cos_on(g->min_cos_vert);
  p.cc_point = g->min_cos_point * std::fabs(g->min_cos_point);
  p.cc_vert = g->min_cos_vert * std::fabs(g->min_cos_vert);
  if (point_dir && surface_gate_dist_on(g->max_dist_point)) p.tau2_point = g->max_dist_point * g->max_dist_point;
  if (vert_dir && surface_gate_dist_on(g->max_dist_vert)) p.tau2_vert = g->max_dist_vert * g->max_dist_vert;
  p.boundary = vert_dir && g->reject_boundary != 0;
  p.any = p.cos_point || p.cos_vert || p.tau2_point != INFINITY || p.tau2_vert != INFINITY || p.boundary ||
          (point_dir && g->point_kept) || (vert_dir && g->vert_kept);
  return p;
}

// -> why the gated entry points refuse the gate block (the text behind "<entry point>: "), or nullptr; asked after
// surface_term_args_refusal has accepted the term's block `a`
struct SurfaceGateFacts {
  bool targets;           // target meshes were given
  bool step;              // the block rides on a step
  bool step_has_points;   // ... whose points are the caller's
};
inline const char* surface_gate_args_refusal(const smalfit_surface_gate_args* g, const smalfit_surface_term_args* a,
                                             const SurfaceGateFacts& f) {
  if (g->struct_size != (unsigned)sizeof(smalfit_surface_gate_args))
    return "smalfit_surface_gate_args.struct_size does not match this library (built against another smalfit.h?)";
  if (!(g->min_cos_point <= 1.0f)) return "min_cos_point must be <= 1 and not NaN";
  if (!(g->min_cos_vert <= 1.0f)) return "min_cos_vert must be <= 1 and not NaN";
  if (!g->kept) return "kept missing";
  const bool vert_gate = g->reject_boundary != 0 || surface_gate_cos_on(g->min_cos_vert) || surface_gate_dist_on(g->max_dist_vert);
  if (vert_gate && !f.targets) return "a vertex gate needs the target meshes";
  const bool point_dir = a->w_point_surface > 0.f, vert_dir = a->w_vert_surface > 0.f;
  const bool sampled = f.step && !f.step_has_points;
  if (sampled && g->point_normals) return "point_normals must be NULL in a step that samples its points: it draws its own";
  if (point_dir && surface_gate_cos_on(g->min_cos_point) && !sampled && !g->point_normals)
    return "min_cos_point needs point_normals with the caller's points";
  if (g->point_kept && !point_dir) return "point_kept given while the point direction is skipped";
  if (g->vert_kept && !vert_dir) return "vert_kept given while the vertex direction is skipped";
  if (g->vert_normals && !(vert_dir && surface_gate_cos_on(g->min_cos_vert))) return "vert_normals given without min_cos_vert";
  return nullptr;
}
// mesh3d_vertex_normal_kernel: one vertex per thread
inline Grid2 vertex_normal_grid(int V, int N) { return Grid2{mesh_element_blocks(V), N}; }

// The gates of the chamfer term (smalfit_chamfer_gate_args).  mesh3d_chamfer_kernel<ROLE, true> stages 32-byte records (position,
// owner | unit normal, tag) where the ungated kernel stages 16: half as many at a time fill the same 16 KB, so a block's LDS --
// the chunk, the four waves' minima (2 KB) and, in the vertex direction, their gathered sums (3 KB) -- stays 21 KB, under the
// 32 KB that four blocks a CU allow
constexpr int kChamGateRecordBytes = 32;
constexpr int kChamGateChunk = 512;
constexpr int kChamGateLdsBytes = kChamGateChunk * kChamGateRecordBytes + 2 * 4 * kMeshQueries * 4 + 4 * kMeshQueries * 3 * 4;
static_assert(kChamGateLdsBytes <= 32 * 1024, "four gated chamfer blocks share a CU");
// what a block switches on, in the form the kernels take it: tau^2 formed here, once, in float32 (+inf: no truncation); an open
// compatibility test is c = -inf (every record passes and no normal is read).  A direction runs the gated instantiation when one
// of its gates is on or one of its per-query outputs is asked for; otherwise it is the ungated kernel, and its kept count is
// every query
struct ChamferGatePlan {
  bool gated_point, gated_vert;   // point -> vertex | vertex -> point runs mesh3d_chamfer_kernel<., true>
  bool cos_point, cos_vert;
  float c_point, c_vert;
  float tau2_point, tau2_vert;
  bool boundary;
  bool vert_normals, point_normals;   // u_v / m_s are read: some compatibility test is on (each reads both sets)
  bool point_boundary;                // b_s is read
  bool any() const { return gated_point || gated_vert; }
};
// of a block chamfer_gate_args_refusal accepts (g may be NULL: everything off); with the chamfer term off everything is off
inline ChamferGatePlan plan_chamfer_gates(const smalfit_chamfer_gate_args* g, bool chamfer_on) {
  ChamferGatePlan p{};
  p.c_point = p.c_vert = -INFINITY;
  p.tau2_point = p.tau2_vert = INFINITY;
  if (!g || !chamfer_on) return p;
  p.cos_point = surface_gate_cos_on(g->min_cos_point);
  p.cos_vert = surface_gate_cos_on(g->min_cos_vert);
  if (p.cos_point) p.c_point = g->min_cos_point;
  if (p.cos_vert) p.c_vert = g->min_cos_vert;
  if (surface_gate_dist_on(g->max_dist_point)) p.tau2_point = g->max_dist_point * g->max_dist_point;
  if (surface_gate_dist_on(g->max_dist_vert)) p.tau2_vert = g->max_dist_vert * g->max_dist_vert;
  p.boundary = g->reject_boundary != 0;
  p.gated_point = p.cos_point || p.tau2_point != INFINITY || g->point_kept || g->point_nn;
  p.gated_vert = p.cos_vert || p.tau2_vert != INFINITY || p.boundary || g->vert_kept || g->vert_nn;
  p.vert_normals = p.point_normals = p.cos_point || p.cos_vert;
  p.point_boundary = p.boundary;
  return p;
}
// -> why the gated entry points refuse the chamfer gate block (the text behind "<entry point>: "), or nullptr; asked after the
// call's own arguments have been accepted
struct ChamferGateFacts {
  bool chamfer_on;        // w_chamfer > 0
  bool step;              // the block rides on a step
  bool step_has_points;   // ... whose points are the caller's
};
inline const char* chamfer_gate_args_refusal(const smalfit_chamfer_gate_args* g, const ChamferGateFacts& f) {
  if (g->struct_size != (unsigned)sizeof(smalfit_chamfer_gate_args))
    return "smalfit_chamfer_gate_args.struct_size does not match this library (built against another smalfit.h?)";
  if (!(g->min_cos_point <= 1.0f)) return "min_cos_point must be <= 1 and not NaN";
  if (!(g->min_cos_vert <= 1.0f)) return "min_cos_vert must be <= 1 and not NaN";
  if (!g->kept) return "kept missing";
  const bool sampled = f.step && !f.step_has_points;
  if (sampled && (g->point_normals || g->point_boundary))
    return "point_normals and point_boundary must be NULL in a step that samples its points: it draws its own";
  if (!f.chamfer_on) return nullptr;   // accepted and ignored
  const bool cos_on = surface_gate_cos_on(g->min_cos_point) || surface_gate_cos_on(g->min_cos_vert);
  if (cos_on && !sampled && !g->point_normals) return "a min_cos gate needs point_normals with the caller's points";
  if (g->reject_boundary != 0 && !sampled && !g->point_boundary) return "reject_boundary needs point_boundary with the caller's points";
  return nullptr;
}

// The robust kernel of both data terms (smalfit_robust_args; robust_gm of mesh3d_math.h).  The ROBUST instantiations of
// mesh3d_chamfer_kernel<1, ., .> stage the points' weights in a float array beside the records: 4 KB more at kChamChunk, 2 KB at
// kChamGateChunk, so a block stays under the 32 KB that four blocks a CU allow
constexpr int kChamRobustLdsBytes = kChamGateLdsBytes + 1024 * 4;
static_assert(kChamRobustLdsBytes <= 32 * 1024, "four robust chamfer blocks share a CU");
// a scale is on when sigma > 0 and finite; its float32 square, formed here, once, is what the kernels take
inline bool robust_scale_on(float sigma) { return sigma > 0.f && std::isfinite(sigma); }
inline float robust_scale_sq(float sigma) { return sigma * sigma; }
// what a call computes of the two terms: a scale of a skipped direction is off
struct RobustFacts {
  bool chamfer_call, surface_call;   // the entry point evaluates the chamfer term | the surface term at all
  bool chamfer_on;                   // w_chamfer > 0
  bool point_dir, vert_dir;          // w_point_surface > 0 | w_vert_surface > 0 (in a step: of a surface block that is on)
};
// what a block switches on, in the form the kernels take it (r may be NULL: everything off).  s2 = 0: off.  The chamfer term
// runs its ROBUST instantiations in BOTH directions when either of its scales is on (the vertices' kernel gathers the weights
// the points' kernel wrote; a direction whose own scale is off takes w = 1, rho = d^2 there); the surface term's hit kernel of a
// direction is the ROBUST one exactly when that direction's scale is on.  A ROBUST instantiation writes per-block partial sums
// of w beside its partial sums of rho; where none ran, the weight sums are read off the kept counts
struct RobustPlan {
  bool chamfer;                      // mesh3d_chamfer_kernel<0, ., true> and <1, ., true> run and write weight partials
  bool surface_point, surface_vert;  // mesh3d_surface_hit_kernel<1, ., true> | <0, ., true> runs and writes weight partials
  float s2_chamfer_point, s2_chamfer_vert, s2_surface_point, s2_surface_vert;
  bool any() const { return chamfer || surface_point || surface_vert; }
};
inline RobustPlan plan_robust(const smalfit_robust_args* r, const RobustFacts& f) {
  RobustPlan p{};
  if (!r) return p;
  if (f.chamfer_call && f.chamfer_on) {
    if (robust_scale_on(r->sigma_chamfer_point)) p.s2_chamfer_point = robust_scale_sq(r->sigma_chamfer_point);
    if (robust_scale_on(r->sigma_chamfer_vert)) p.s2_chamfer_vert = robust_scale_sq(r->sigma_chamfer_vert);
  }
  if (f.surface_call && f.point_dir && robust_scale_on(r->sigma_surface_point)) p.s2_surface_point = robust_scale_sq(r->sigma_surface_point);
  if (f.surface_call && f.vert_dir && robust_scale_on(r->sigma_surface_vert)) p.s2_surface_vert = robust_scale_sq(r->sigma_surface_vert);
  p.chamfer = p.s2_chamfer_point > 0.f || p.s2_chamfer_vert > 0.f;
  p.surface_point = p.s2_surface_point > 0.f;
  p.surface_vert = p.s2_surface_vert > 0.f;
  return p;
}
// -> why the robust entry points refuse the block (the text behind "<entry point>: "), or nullptr; asked after the call's other
// blocks have been accepted.  The order: the struct's size, the four squares (chamfer point, chamfer vertex, surface point,
// surface vertex), outputs of a term the call does not evaluate, the four per-query outputs against their scales
inline const char* robust_args_refusal(const smalfit_robust_args* r, const RobustFacts& f) {
  if (r->struct_size != (unsigned)sizeof(smalfit_robust_args))
    return "smalfit_robust_args.struct_size does not match this library (built against another smalfit.h?)";
  if (robust_scale_on(r->sigma_chamfer_point) && !std::isnormal(robust_scale_sq(r->sigma_chamfer_point)))
    return "the float32 square of sigma_chamfer_point is not a normal number";
  if (robust_scale_on(r->sigma_chamfer_vert) && !std::isnormal(robust_scale_sq(r->sigma_chamfer_vert)))
    return "the float32 square of sigma_chamfer_vert is not a normal number";
  if (robust_scale_on(r->sigma_surface_point) && !std::isnormal(robust_scale_sq(r->sigma_surface_point)))
    return "the float32 square of sigma_surface_point is not a normal number";
  if (robust_scale_on(r->sigma_surface_vert) && !std::isnormal(robust_scale_sq(r->sigma_surface_vert)))
    return "the float32 square of sigma_surface_vert is not a normal number";
  if (!f.chamfer_call && (r->chamfer_weight_sums || r->chamfer_point_weights || r->chamfer_vert_weights))
    return "chamfer weight outputs given to a call that does not evaluate the chamfer term";
  if (!f.surface_call && (r->surface_weight_sums || r->surface_point_weights || r->surface_vert_weights))
    return "surface weight outputs given to a call that does not evaluate the surface term";
  const RobustPlan p = plan_robust(r, f);
  if (r->chamfer_point_weights && !(p.s2_chamfer_point > 0.f)) return "chamfer_point_weights given while sigma_chamfer_point is off";
  if (r->chamfer_vert_weights && !(p.s2_chamfer_vert > 0.f)) return "chamfer_vert_weights given while sigma_chamfer_vert is off";
  if (r->surface_point_weights && !(p.s2_surface_point > 0.f)) return "surface_point_weights given while sigma_surface_point is off";
  if (r->surface_vert_weights && !(p.s2_surface_vert > 0.f)) return "surface_vert_weights given while sigma_surface_vert is off";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// smalfit_fit3d_step: which blocks are refused, and what a step launches
// ------------------------------------------------------------------------------------------------
constexpr int kFit3dParams = 5;   // betas, global_rot, joint_rot, trans, deform_verts
// fit3d_adam_kernel's argument (kernels_mesh3d.inc): torch.optim.Adam over the trained parameters, one launch; a segment's
// gradient may be a column block of a wider row-major buffer (global_rot / joint_rot are columns 0..2 / 3..104 of d theta [N][105])
struct Fit3dAdamSeg {
  float* p;
  const float* g;
  float* m;
  float* v;
  int count, row_len, g_stride, g_offset;
  float step_size;   // lr / (1 - beta1^t)
  int block0;        // first block of this segment
};
struct Fit3dAdamArgs {
  Fit3dAdamSeg seg[kFit3dParams];
  int nseg;
  float b1, b2, eps, bc2_sqrt;
};

struct Fit3dFacts {
  int max_frames, model_verts, model_betas;          // the engine and its model
  int max_meshes, max_points, objective_verts;       // the objective
  bool targets;                                      // target meshes were given
  int target_meshes;                                 // how many (read only with `targets`)
};
// -> why smalfit_fit3d_step refuses the block (the text behind "smalfit_fit3d_step: "), or nullptr
inline const char* fit3d_args_refusal(const smalfit_fit3d_args* a, const Fit3dFacts& f) {
  const int N = a->num_meshes, nb = a->num_betas, S = a->num_points;
  if (N <= 0 || N > f.max_frames || N > f.max_meshes) return "num_meshes exceeds the engine's max_frames or the objective's max_meshes";
  if (f.model_verts != f.objective_verts) return "engine and objective were built for different meshes";
  if (nb <= 0 || nb > f.model_betas || nb > 64) return "num_betas out of range";
  if (!a->betas || !a->global_rot || !a->joint_rot || !a->trans || !a->losses) return "missing parameter / losses pointer";
  if (a->weights[0] > 0.f) {
    if (S <= 0 || S > f.max_points) return "the chamfer term needs 1 <= num_points <= max_points";
    if (!a->points && !f.targets) return "neither target points nor target meshes given";
    if (!a->points && f.target_meshes != N) return "number of target meshes differs from num_meshes";
  }
  bool any = false;
  if (a->lr_betas > 0.f) {
    if (!a->betas || !a->m_betas || !a->v_betas) return "betas is trained (lr > 0) but its parameter or Adam state is missing";
    any = true;
  }
  if (a->lr_global_rot > 0.f) {
    if (!a->global_rot || !a->m_global_rot || !a->v_global_rot) return "global_rot is trained (lr > 0) but its parameter or Adam state is missing";
    any = true;
  }
  if (a->lr_joint_rot > 0.f) {
    if (!a->joint_rot || !a->m_joint_rot || !a->v_joint_rot) return "joint_rot is trained (lr > 0) but its parameter or Adam state is missing";
    any = true;
  }
  if (a->lr_trans > 0.f) {
    if (!a->trans || !a->m_trans || !a->v_trans) return "trans is trained (lr > 0) but its parameter or Adam state is missing";
    any = true;
  }
  if (a->lr_deform_verts > 0.f) {
    if (!a->deform_verts || !a->m_deform_verts || !a->v_deform_verts) return "deform_verts is trained (lr > 0) but its parameter or Adam state is missing";
    any = true;
  }
  if (any && a->adam_t <= 0) return "adam_t must be the 1-based step count";
  return nullptr;
}

// where the chamfer term's target points come from
enum class Fit3dPoints {
  None = 0,            // chamfer and the point-surface term off: none are read
  SampleToObjective,   // sampled from the target meshes into the objective's buffer
  SampleToCaller,      // ... into points_out
  Callers,             // the caller's, read in place
  CallersCopied,       // ... and copied to points_out
};
struct Fit3dAdamGeometry { int tensor, count, row_len, g_stride, g_offset, block0; };   // (tensor: index in the order of kFit3dParams)
struct Fit3dPlan {
  bool chamfer;
  Fit3dPoints points;
  bool need_pose, need_beta;   // the LBS adjoint runs for either; need_beta: with the shape-blend adjoint and the per-frame betas assembly
  bool planar_vertex_grad;     // the gather kernel leaves a planar copy of d verts where the LBS adjoint reads it
  bool any_trained;            // else the step ends behind the objective
  int nseg;                    // trained tensors, in the order of kFit3dParams
  Fit3dAdamGeometry seg[kFit3dParams];
  int adam_blocks;             // grid of fit3d_adam_kernel
};
// -> the plan of a block that fit3d_args_refusal accepts, on a model of `model_verts` vertices.  point_surface: the step carries
// a surface block with w_point_surface > 0, which reads the step's points whether the chamfer term runs or not
inline Fit3dPlan plan_fit3d(const smalfit_fit3d_args* a, int model_verts, bool point_surface = false) {
  Fit3dPlan p{};
  const int N = a->num_meshes, nb = a->num_betas, V3 = model_verts * 3;
  p.chamfer = a->weights[0] > 0.f;
  if (!p.chamfer && !point_surface) p.points = Fit3dPoints::None;
  else if (!a->points) p.points = a->points_out ? Fit3dPoints::SampleToCaller : Fit3dPoints::SampleToObjective;
  else p.points = a->points_out && a->points_out != a->points ? Fit3dPoints::CallersCopied : Fit3dPoints::Callers;
  p.need_pose = a->lr_global_rot > 0.f || a->lr_joint_rot > 0.f;
  p.need_beta = a->lr_betas > 0.f;
  p.planar_vertex_grad = p.need_pose || p.need_beta;
  const float lr[kFit3dParams] = {a->lr_betas, a->lr_global_rot, a->lr_joint_rot, a->lr_trans, a->lr_deform_verts};
  const int counts[kFit3dParams] = {N * nb, N * 3, N * 102, N * 3, N * V3};
  const int row_len[kFit3dParams] = {nb, 3, 102, 3, V3};
  const int g_stride[kFit3dParams] = {nb, 105, 105, 3, V3};
  const int g_offset[kFit3dParams] = {0, 0, 3, 0, 0};
  for (int k = 0; k < kFit3dParams; ++k) {
    if (!(lr[k] > 0.f)) continue;
    p.seg[p.nseg++] = Fit3dAdamGeometry{k, counts[k], row_len[k], g_stride[k], g_offset[k], p.adam_blocks};
    p.adam_blocks += fit3d_adam_blocks(counts[k]);
  }
  p.any_trained = p.nseg > 0;
  return p;
}

// What the opt-in blocks of a step share (blocks the refusals accept; any may be NULL).  The points' unit normals and boundary
// bytes are drawn WITH the points, once, when the step samples them and a compatibility test of either term (the boundary rule
// of the chamfer term) reads them; with the caller's points each term reads its own gate block's pointers.  The fitted vertex
// normals are gathered once: behind compose when the chamfer gates read them -- into the surface gate block's vert_normals where
// the surface term's min_cos_vert wants a copy, else into the objective's buffer -- and the surface term then reads those
// instead of gathering its own
enum class RiderSource { Callers = 0, Drawn = 1 };              // the gate block's pointer (may be NULL) | what the sampler drew
enum class VertNormalsDest { Objective = 0, SurfaceGateBlock = 1 };
struct Fit3dRiders {
  bool draw_normals, draw_boundary;        // the sampler also writes the points' unit normals | boundary bytes
  RiderSource surface_normals;             // the point normals the surface gates read
  RiderSource chamfer_normals, chamfer_boundary;
  VertNormalsDest vert_normals;            // where the fitted vertex normals are written, whichever term gathers them
  bool surface_reuses_vert_normals;        // the chamfer gates gathered them: the surface term launches no gather of its own
};
inline Fit3dRiders plan_fit3d_riders(const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate,
                                     const smalfit_chamfer_gate_args* cg, float w_chamfer, Fit3dPoints points) {
  Fit3dRiders r{};
  const bool surface = surface_term_on(sf);   // a block with both weights <= 0 is the step without it, its gates included
  const SurfaceGatePlan sp = plan_surface_gates(surface ? gate : nullptr, surface && sf->w_point_surface > 0.f, surface && sf->w_vert_surface > 0.f);
  const ChamferGatePlan cp = plan_chamfer_gates(cg, w_chamfer > 0.f);
  if (points == Fit3dPoints::SampleToCaller || points == Fit3dPoints::SampleToObjective) {
    r.draw_normals = sp.cos_point || cp.point_normals;
    r.draw_boundary = cp.point_boundary;
    if (sp.cos_point) r.surface_normals = RiderSource::Drawn;
    if (cp.point_normals) r.chamfer_normals = RiderSource::Drawn;
    if (cp.point_boundary) r.chamfer_boundary = RiderSource::Drawn;
  }
  if (sp.cos_vert && gate->vert_normals) r.vert_normals = VertNormalsDest::SurfaceGateBlock;
  r.surface_reuses_vert_normals = cp.vert_normals && sp.cos_vert;
  return r;
}

// ------------------------------------------------------------------------------------------------
// the scan-sequence block (smalfit_scan_sequence_*): which lengths and blocks are refused, and whether anything is launched
// ------------------------------------------------------------------------------------------------
// -> why smalfit_scan_sequence_create refuses (the text behind its name), or nullptr.  clip_lengths is the host's
inline const char* sequence_create_refusal(bool given, int num_meshes, int num_clips, const int* clip_lengths) {
  if (!given || !clip_lengths) return "null argument";
  if (num_meshes <= 0 || num_clips <= 0) return "num_meshes and num_clips must be positive";
  long long sum = 0;
  for (int c = 0; c < num_clips; ++c) {
    if (clip_lengths[c] <= 0) return "every clip length must be positive";
    sum += clip_lengths[c];
  }
  if (sum != num_meshes) return "clip_lengths do not sum to num_meshes";
  return nullptr;
}
struct SequenceFacts {
  int handle_meshes, lengths_sum;   // the N the handle was built for | the sum of its clip lengths
  int num_meshes;                   // the N of this call
  bool step;                        // the block rides on a smalfit_fit3d_args (else smalfit_scan_sequence_couple)
  bool global_rot, joint_rot, trans;   // the parameters the call was given
};
// -> why the sequence entry points refuse the block (the text behind "<entry point>: "), or nullptr; asked after the call's other
// blocks have been accepted.  The order: the handle's N, the lengths against N, the three weights (joint, global, trans), losses,
// step_total outside a step, a term without its parameter
inline const char* sequence_args_refusal(const smalfit_sequence_args* q, const SequenceFacts& f) {
  if (f.handle_meshes != f.num_meshes) return "the sequence handle was built for another num_meshes";
  if (f.lengths_sum != f.num_meshes) return "clip_lengths do not sum to num_meshes";
  if (!std::isfinite(q->w_temp_joint)) return "w_temp_joint is not finite";
  if (!std::isfinite(q->w_temp_global)) return "w_temp_global is not finite";
  if (!std::isfinite(q->w_temp_trans)) return "w_temp_trans is not finite";
  if (!q->losses) return "losses is NULL";
  if (!f.step && q->step_total) return "step_total given outside a step";
  if (q->w_temp_joint > 0.f && !f.joint_rot) return "w_temp_joint > 0 but joint_rot is missing";
  if (q->w_temp_global > 0.f && !f.global_rot) return "w_temp_global > 0 but global_rot is missing";
  if (q->w_temp_trans > 0.f && !f.trans) return "w_temp_trans > 0 but trans is missing";
  return nullptr;
}
// what a block that sequence_args_refusal accepts couples.  any_long_clip: some clip is longer than 1; betas_given: there is a
// betas gradient to share (a step: lr_betas > 0; couple: g_betas given).  launch: fit3d_sequence_kernel runs at all -- a block
// that couples nothing launches nothing and its losses read 0
struct SequencePlan {
  bool launch;
  bool share;                  // the shape sum runs
  bool joint, global, trans;   // the term is evaluated
};
inline SequencePlan plan_sequence(const smalfit_sequence_args* q, bool any_long_clip, bool betas_given) {
  SequencePlan p{};
  if (!q || !any_long_clip) return p;
  p.share = q->share_shape != 0 && betas_given;
  p.joint = q->w_temp_joint > 0.f;
  p.global = q->w_temp_global > 0.f;
  p.trans = q->w_temp_trans > 0.f;
  p.launch = p.share || p.joint || p.global || p.trans;
  if (!p.launch) p = SequencePlan{};
  return p;
}
// fit3d_sequence_kernel: block 0 sums the losses; behind it one thread per output element, the shape sums (clip, column) first,
// then the temporal gradients (mesh, 105 columns of d theta | 3 of d trans)
constexpr int kSeqBlock = 256;
constexpr int kSeqGradCols = 105 + 3;
inline int sequence_shape_elements(const SequencePlan& p, int num_clips, int num_betas) { return p.share ? num_clips * num_betas : 0; }
inline int sequence_blocks(const SequencePlan& p, int num_meshes, int num_clips, int num_betas) {
  const int elements = sequence_shape_elements(p, num_clips, num_betas) + (p.joint || p.global || p.trans ? num_meshes * kSeqGradCols : 0);
  return 1 + (elements + kSeqBlock - 1) / kSeqBlock;
}

// the temporal terms on posed vertices (smalfit_scan_sequence_vertex_term, smalfit_scan_sequence_vertex_step)
struct SequenceVertexFacts {
  bool step;                        // the block rides on a step (else smalfit_scan_sequence_vertex_term)
  int num_verts;                    // V of the call
  bool verts;                       // the vertices were given (a step composes its own)
  int handle_meshes, num_meshes;    // the N the handle was built for | the N of this call
};
// -> why the vertex entry points refuse the block (the text behind "<entry point>: "), or nullptr; asked after the call's other
// blocks have been accepted.  The order: the block, losses, the two weights (velocity, acceleration), step_total outside a step,
// num_verts, verts, the handle's N
inline const char* sequence_vertex_args_refusal(const smalfit_sequence_vertex_args* q, const SequenceVertexFacts& f) {
  if (!q) return "the vertex block is NULL";
  if (!q->losses) return "losses is NULL";
  if (!std::isfinite(q->w_temp_vert_vel)) return "w_temp_vert_vel is not finite";
  if (!std::isfinite(q->w_temp_vert_acc)) return "w_temp_vert_acc is not finite";
  if (!f.step && q->step_total) return "step_total given outside a step";
  if (f.num_verts < 1) return "num_verts must be positive";
  if (!f.verts) return "verts is NULL";
  if (f.handle_meshes != f.num_meshes) return "the sequence handle was built for another num_meshes";
  return nullptr;
}
// what a block that sequence_vertex_args_refusal accepts evaluates.  longest_clip: the length of the handle's longest clip.  A
// velocity pair needs a clip of 2, an acceleration triple one of 3.  launch: the two kernels run at all -- a block with both weights
// <= 0, or with no clip long enough for an enabled term, launches nothing and its losses read 0
struct SequenceVertexPlan {
  bool launch;
  bool vel, acc;   // the term is evaluated
};
inline SequenceVertexPlan plan_sequence_vertex(const smalfit_sequence_vertex_args* q, int longest_clip) {
  SequenceVertexPlan p{};
  if (!q) return p;
  p.vel = q->w_temp_vert_vel > 0.f && longest_clip >= 2;
  p.acc = q->w_temp_vert_acc > 0.f && longest_clip >= 3;
  p.launch = p.vel || p.acc;
  return p;
}
// fit3d_sequence_vertex_kernel: one thread per vertex (n, v), 256 a block, a row of blocks per mesh; every block leaves
// kSeqVertexSums partials [sum][n][block] (S_vel, S_acc, the three columns of d trans), which the one-block
// fit3d_sequence_vertex_finish_kernel adds in ascending mesh, then ascending block order
constexpr int kSeqVertexBlock = 256;
constexpr int kSeqVertexSums = 5;
inline Grid2 sequence_vertex_grid(int V, int N) { return Grid2{(V + kSeqVertexBlock - 1) / kSeqVertexBlock, N}; }
inline size_t sequence_vertex_partials(int V, int N) { return (size_t)kSeqVertexSums * (size_t)N * (size_t)sequence_vertex_grid(V, N).x; }

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
  bool has_joint_limits = false;   // smalfit_engine_set_joint_limits was called (and not cleared since)
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

// Where the M frames of an evaluation sit in their sequence: frames are grouped into consecutive windows of `window`
// frames counted from the START OF THE SEQUENCE (optimize_to_joints.py:119-120, the last window may be ragged), and the
// reference's per-window normalisers 1/(B 50), 1/(B 105), 1/(B S^2) (smal_fitter.py:144,157,173) use the size B of the
// window a frame belongs to.  An evaluation may hold any contiguous part of the sequence -- a whole sequence
// (offset 0, total M), a shard of it, or a single frame of an 8-frame window (one frame per GPU).
struct WinMap {
  int window;   // WINDOW_SIZE
  int offset;   // index of local frame 0 in the sequence
  int total;    // frames in the whole sequence
};

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
// smalfit_metrics_args: which blocks are refused (smalfit_fit_metrics)
// ------------------------------------------------------------------------------------------------
inline bool metrics_keypoints(const smalfit_metrics_args* a) { return a->proj_joints && a->target_joints && a->target_visibility; }
// -> why smalfit_fit_metrics refuses the block (the text behind "smalfit_fit_metrics: "), or nullptr.  struct_size first: with a
// block laid out by another header no other field can be trusted
inline const char* metrics_args_refusal(const smalfit_metrics_args* a, int max_frames) {
  if (a->struct_size != (unsigned)sizeof(smalfit_metrics_args))
    return "smalfit_metrics_args.struct_size does not match this library (built against another smalfit.h?)";
  if (a->num_frames <= 0 || a->num_frames > max_frames) return "num_frames exceeds the engine's max_frames";
  if (!a->verts || !a->sil_counts) return "verts / sil_counts missing";
  if (!a->target_sil && !a->target_sil_u8) return "target_sil missing (give target_sil or target_sil_u8)";
  const bool any = a->proj_joints || a->target_joints || a->target_visibility;
  if (any && !metrics_keypoints(a)) return "give all of proj_joints, target_joints and target_visibility, or none of them";
  if (!any) return a->keypoint_dist || a->pck_counts ? "keypoint_dist / pck_counts given without the keypoint inputs" : nullptr;
  static_assert(SMALFIT_MAX_PCK_THRESHOLDS == 8, "the message below names the limit");
  if (a->num_thresholds < 1 || a->num_thresholds > SMALFIT_MAX_PCK_THRESHOLDS) return "num_thresholds must be 1..8";
  for (int t = 0; t < a->num_thresholds; ++t)
    if (!(std::isfinite(a->thresholds[t]) && a->thresholds[t] > 0.f)) return "every threshold must be finite and > 0";
  return nullptr;
}

// ------------------------------------------------------------------------------------------------
// one evaluation (smalfit_fit_eval, smalfit_fit_eval_windows, the evaluations of smalfit_fit_run): what it launches, with
// which switches.  fit_eval_impl fills its argument structs from these fields and the pointers of the block; it decides nothing
// ------------------------------------------------------------------------------------------------
// How the caller strings evaluations together and which rows it wants beside the totals
struct EvalMode {
  bool pending = false;      // the head launch takes over the optimiser step the previous evaluation left (smalfit_fit_run)
  bool assemble = true;      // run assemble_kernel (gradients to the caller's buffers, the nine loss terms)
  // smalfit_fit_eval_windows: one row per window (window_rows_refusal has accepted the rows)
  bool window_rows = false;
  bool want_betas = false;   // smalfit_window_rows.g_betas given
  bool want_scales = false;  // smalfit_window_rows.g_log_beta_scales given
};
enum class HeadKernel { Plain = 0, Images = 1, Step = 2 };   // lbs_head_kernel | lbs_head_images_kernel | lbs_head_step_kernel
enum class SilTargetKind { None = 0, F32 = 1, U8 = 2 };
enum class LossLaunch { OwnKernel = 0, InResolve = 1 };     // loss_kernel | riders of raster_resolve_kernel
struct EvalPlan {
  // frames and strides
  int M;
  WinMap win;                // where the M frames sit in their sequence
  bool independent;          // every frame its own subject
  int nb;                    // shape directions the fitter optimises
  int betas_stride;          // floats between two frames' betas; 0: one shape for all
  int ls_stride;             // floats between two frames' limb scales; 0: one set for all
  bool limb_scales;          // log_beta_scales is read at all
  // shape prior
  bool shape_prior;
  int prior_dim;             // 0 without the prior
  bool prior_uses_ls;        // the prior spans the limb scales too (dimension above 20)
  int prior_windows;         // windows whose prior term this evaluation owns (independent images: window = 1, so one per image)
  float prior_weight;        // w_betas x the owned windows; independent images: w_betas, once per image
  bool prior_per_frame;
  HeadPrior head_prior;
  // head kernel
  HeadKernel head;
  // silhouette and rasteriser
  bool sil_on;               // the silhouette term is in the loss
  bool rasterise;            // the rasteriser runs: for the term or for sil_out alone
  SilTargetKind sil_target;
  bool frame_loss;           // the queue kernels also count their loss per frame (the kFrameLoss instantiations)
  bool queue_loss;           // the queue kernels write their loss partials at all
  bool raster_backward;
  // loss launch
  LossLaunch loss_launch;
  bool joints_in_head;       // joints_kernel runs behind the skinning (else its blocks ride in the sweep launch)
  // effective weights
  float w_temp;              // 0 unless `temporal`
  float w_limit;             // 0 unless the engine has a limit table: the reference's weight table carries w_limit = 100 in stages
                             // 1-3 while the term itself is commented out (smal_fitter.py:146-151)
  bool halos;                // halo_prev / halo_next are read (where given)
  // outputs and adjoints
  bool verts_out;
  bool need_pose, need_beta, need_ls;
  // backward
  int bwd_betas_shared;      // the dbeta partials are summed over the frames (0: one row of partials per frame)
  int j_stride;              // floats between two frames' rest joints; 0: one set
  // assembly
  int asm_betas_shared, asm_ls_shared;
  int ngrp_beta;             // frame groups of the dbeta partials the assembly would add up
  int asm_shape_sets;        // blocks of assemble_kernel's first role
  // per-frame rows
  bool rows;                 // frame_loss_rows_kernel writes losses_per_frame
  // window rows
  int W;                     // rows; 0 without them
  bool ls_rows;              // the shared limb scales' gradient is formed per window too
  int clear_qloss;           // window_rows_kernel is the last reader of the per-frame loss counters and clears them
  bool assembly_leaves_betas, assembly_leaves_scales;   // ... to window_rows_kernel
};
// -> the plan of a block that fit_args_refusal and fit_model_refusal accept (and, with window rows, window_rows_refusal)
inline EvalPlan plan_eval(const smalfit_fit_args* a, const EngineFacts& e, const EvalMode& mode) {
  EvalPlan p{};
  const int M = p.M = a->num_frames;
  p.win = WinMap{a->window, a->frame_offset, sequence_frames(a)};
  const bool indep = p.independent = independent_images(a);
  const bool wr = mode.window_rows;
  p.nb = kFitBetas;
  p.betas_stride = indep ? p.nb : 0;
  p.ls_stride = a->logscale_mode == 2 ? 6 : 0;
  p.limb_scales = a->logscale_mode != 0;

  p.shape_prior = a->w_betas > 0.f;
  p.prior_dim = p.shape_prior ? shape_prior_dim(a, e.shape_dim) : 0;
  p.prior_uses_ls = prior_uses_limb_scales(a, e.shape_dim);
  p.prior_windows = p.shape_prior ? prior_windows(p.win.window, p.win.offset, M) : 0;
  p.prior_weight = !p.shape_prior ? 0.f : (indep ? a->w_betas : a->w_betas * (float)p.prior_windows);
  p.prior_per_frame = p.shape_prior && indep;
  p.head_prior = !p.shape_prior ? HeadPrior::None : (indep ? HeadPrior::PerFrame : HeadPrior::Shared);
  // (one subject under a pending step: plan_fold refuses independent images.  Independent images without the prior take the plain kernel)
  p.head = mode.pending ? HeadKernel::Step : (p.prior_per_frame ? HeadKernel::Images : HeadKernel::Plain);

  p.sil_on = a->w_sil > 0.f;
  p.rasterise = p.sil_on || a->sil_out != nullptr;
  p.sil_target = !p.sil_on ? SilTargetKind::None : (a->target_sil_u8 ? SilTargetKind::U8 : SilTargetKind::F32);
  // one row of loss terms per frame: only an evaluation that assembles writes (and clears the counters behind) them
  p.rows = a->losses_per_frame != nullptr && mode.assemble;
  p.frame_loss = (p.rows || wr) && p.sil_on;
  p.queue_loss = p.sil_on;
  p.raster_backward = p.sil_on;
  // with the rasteriser running, the joint regression and the loss terms ride in its launches
  p.loss_launch = p.rasterise ? LossLaunch::InResolve : LossLaunch::OwnKernel;
  p.joints_in_head = !p.rasterise;

  p.w_temp = a->temporal ? a->w_temp : 0.f;
  p.w_limit = e.has_joint_limits ? a->w_limit : 0.f;
  p.halos = a->temporal != 0;

  p.verts_out = a->verts_out != nullptr;
  p.need_pose = a->g_joint_rotations != nullptr;
  p.need_beta = a->g_betas != nullptr || (wr && mode.want_betas);
  p.need_ls = (a->g_log_beta_scales != nullptr || (wr && mode.want_scales)) && a->logscale_mode != 0;

  // independent images: per-frame partials of the shape-blend adjoint, per-frame rest joints; window rows: the same partial
  // layout -- M rows of nblk_beta * nb floats, dbeta_rows() holds them -- over the one shared shape
  p.bwd_betas_shared = (indep || wr) ? 0 : 1;
  p.j_stride = indep ? 105 : 0;

  p.asm_betas_shared = indep ? 0 : 1;
  p.asm_ls_shared = indep ? 0 : (a->logscale_mode == 1 ? 1 : 0);
  // (odd, and kept: under window rows the backward pass wrote ONE group of per-frame partials, yet this stays the shared
  // shape's group count.  Nothing reads it then: the assembly leaves the betas to window_rows_kernel, which walks the rows itself)
  p.ngrp_beta = beta_groups(!indep);
  p.asm_shape_sets = asm_shape_sets(p.asm_betas_shared, M);

  // (window_rows_refusal has checked the caller's num_windows against this count)
  p.W = wr ? window_rows_count(a->window, a->frame_offset, M) : 0;
  p.ls_rows = wr && p.need_ls && a->logscale_mode == 1;
  p.clear_qloss = wr && !p.rows ? 1 : 0;
  // the assembly leaves the shared gradients to window_rows_kernel (per-frame limb scales stay its own)
  p.assembly_leaves_betas = wr;
  p.assembly_leaves_scales = wr && a->logscale_mode == 1;
  return p;
}

// ------------------------------------------------------------------------------------------------
// the other entry points: which arguments are refused.  Each returns the text behind "<entry point>: " or nullptr; the first
// fault is reported.  Pointers are asked for as `given` (all of them present), nothing is dereferenced unless it says so
// ------------------------------------------------------------------------------------------------
inline const char* null_argument_refusal(bool given) { return given ? nullptr : "null argument"; }
inline const char* bad_argument_refusal(bool good) { return good ? nullptr : "bad argument"; }
// the stateless operators (rodrigues, rigid transformation, point projection and their adjoints): a count and pointers
inline const char* operator_args_refusal(int count, bool given) { return bad_argument_refusal(count > 0 && given); }
inline const char* step_refusal(int step) { return step >= 0 ? nullptr : "step must be >= 0"; }
inline const char* iterations_refusal(int iterations) { return iterations > 0 ? nullptr : "iterations must be positive"; }

// smalfit_engine_create
inline const char* engine_create_refusal(bool given, int max_frames, int image_size) {
  if (!given || max_frames <= 0 || image_size <= 0) return "bad argument";
  static_assert(kMaxImageSize == 1024, "the message below names the limit");
  if (image_size > kMaxImageSize) return "image_size above 1024 is not supported (float32 pixel walk, see kernels_raster.inc)";
  return nullptr;
}
constexpr int kMaxShapePriorDim = 26;        // 20 betas | 6 limb scales
inline const char* shape_prior_refusal(bool given, int dim) {
  static_assert(kMaxShapePriorDim == 26, "the message below names the limit");
  return given && dim > 0 && dim <= kMaxShapePriorDim ? nullptr : "bad argument (dim must be 1..26)";
}
// (reads the 102 limits of both tables)
inline const char* joint_limits_refusal(const float* min_values, const float* max_values) {
  if (!min_values || !max_values) return "null argument";
  for (int i = 0; i < 102; ++i)
    if (!(min_values[i] <= max_values[i])) return "min must not exceed max";
  return nullptr;
}
inline const char* option_refusal(int option, int value) {
  switch (option) {
    case SMALFIT_OPT_UNCLAMPED_EDGE_T: return value == 0 || value == 1 ? nullptr : "SMALFIT_OPT_UNCLAMPED_EDGE_T takes 0 or 1";
    default: return "unknown option";
  }
}
inline const char* profile_begin_refusal(bool given, int max_evals, int stride) { return bad_argument_refusal(given && max_evals > 0 && stride > 0); }

// smalfit_lbs_forward_ex / smalfit_lbs_backward_ex (SMAL.__call__ and its adjoint)
inline const char* lbs_args_refusal(const smalfit_lbs_args* a, int max_frames, int model_betas) {
  if (a->num_frames <= 0 || a->num_frames > max_frames) return "num_frames exceeds the engine's max_frames";
  if (a->num_betas <= 0 || a->num_betas > model_betas) return "num_betas out of range";
  if (!a->beta) return "beta missing";
  if ((a->theta == nullptr) == (a->Rs == nullptr)) return "give exactly one of theta (axis-angle) and Rs (rotation matrices)";
  return nullptr;
}
inline const char* lbs_outputs_refusal(const smalfit_lbs_args* a) { return a->verts && a->joints ? nullptr : "verts / joints outputs missing"; }

// smalfit_render_forward / _color / _backward, smalfit_temporal: a frame count against the engine's capacity
inline const char* render_frames_refusal(int M, int max_frames) { return M > 0 && M <= max_frames ? nullptr : "M exceeds the engine's max_frames"; }
inline const char* temporal_frames_refusal(int N, int max_frames) { return N > 0 && N <= max_frames ? nullptr : "N exceeds the engine's max_frames"; }
// smalfit_pose_prior / _backward
inline const char* pose_prior_refusal(bool given, int N, bool has_pose_prior) {
  if (!given || N <= 0) return "bad argument";
  return has_pose_prior ? nullptr : "pose prior not set";
}

// smalfit_fit_run under smalfit_engine_set_graph; the shard entry points.  (`a` has passed fit_args_size_refusal or is not read:
// subject_frames sits at the block's tail.)
inline const char* graph_subject_refusal(bool graph_on, const smalfit_fit_args* a) {
  return graph_on && a->subject_frames != 0 ? "subject_frames != 0 is not supported by the graph replay (smalfit_engine_set_graph)" : nullptr;
}
inline const char* shard_subject_refusal(const smalfit_fit_args* a) {
  // (a block of another header is refused by the evaluation itself)
  return !fit_args_size_refusal(a) && a->subject_frames != 0
             ? "subject_frames != 0 cannot be sharded (independent images need no collective: give each rank its own batch)" : nullptr;
}
inline const char* shard_record_refusal(int num_shared, int num_frames, bool given) { return bad_argument_refusal(num_shared >= 0 && num_frames > 0 && given); }
inline const char* shard_reduce_refusal(int world_size, int record_stride, bool gathered, int num_shared, int num_trainable, const smalfit_adam_args* o) {
  if (world_size <= 0 || record_stride < num_shared || !gathered || num_shared <= 0 || num_trainable < 0 || num_trainable > num_shared || !o) return "bad argument";
  if (!o->param || !o->grad || !o->exp_avg || !o->exp_avg_sq || o->step < 0) return "bad optimiser state";
  return nullptr;
}
inline const char* shard_run_refusal(const smalfit_fit_args* a, const smalfit_adam_args* ol, const smalfit_adam_args* os, const smalfit_shard_args* sh, int iterations) {
  if (sh->struct_size != (unsigned)sizeof(smalfit_shard_args)) return "smalfit_shard_args.struct_size does not match this library (built against another smalfit.h?)";
  if (iterations <= 0) return "iterations must be positive";
  if (sh->world_size <= 0 || sh->rank < 0 || sh->rank >= sh->world_size) return "bad rank / world_size";
  if (sh->num_shared <= 0 || sh->num_trainable_shared < 0 || sh->num_trainable_shared > sh->num_shared) return "bad num_shared / num_trainable_shared";
  if (!sh->shared_grad || !sh->record || !sh->gathered || !sh->allgather) return "missing buffer / collective";
  if (ol->step < 0 || os->step != ol->step) return "adam_local and adam_shared must carry the same step >= 0";
  return shard_subject_refusal(a);
}
// smalfit_adam_step: one range [0, count) at the 1-based step t
inline const char* adam_step_refusal(int count, bool given, int t) { return bad_argument_refusal(count > 0 && given && t > 0); }

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

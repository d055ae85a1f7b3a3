// TEST-ONLY host build (g++) of the host's launch decisions (smalify_amd/csrc/smalfit_plan.h) and of the model packer
// (smal_model_pack.h): extern "C" wrappers over the very functions smalfit_launch.inc and smalfit_mesh3d.inc call, so that the CPU
// tests compare the Python restatements (tests/fold_forms.py, lbs_forms.py, mesh3d_forms.py, model_forms.py) with the rules
// themselves.  Never part of the product.
#include <cstdint>
#include <cstring>

#include "../smalify_amd/csrc/smal_model_pack.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {

// [kBetaGroups, kMaxImageSize, kMeshQueries, kMeshThreads, kHeadPriorFrames, kCaller, kSharedSlotFloats, sizeof(smalfit_fit_args)]
void hp_constants(int* out8) {
  const int c[8] = {kBetaGroups, kMaxImageSize, kMeshQueries, kMeshThreads, kHeadPriorFrames, kCaller, kSharedSlotFloats,
                    (int)sizeof(smalfit_fit_args)};
  for (int i = 0; i < 8; ++i) out8[i] = c[i];
}

int hp_run_loop(int graph_on, int profiling, int iterations, int callers_stream, int fold_accepted) {
  return (int)run_loop(graph_on != 0, profiling != 0, iterations, callers_stream != 0, fold_accepted != 0);
}

// plan_fold on a layout given by offsets: tensor k lives at param + offset[k] floats (any integer; present[k] = 0: a null
// pointer), its gradient goes to grad + offset[k] where grad_at_offset[k], to a buffer of its own otherwise.  Nothing is
// dereferenced.  -> the refusal (0: accepted); train5 / off5: the plan
int hp_plan_fold(int M, int logscale_mode, int subject_frames, const long long* offset5, const int* present5,
                 const int* grad_at_offset5, int nseg, const int* seg_begin, const int* seg_end, int* train5, int* off5) {
  const uintptr_t param = (uintptr_t)1 << 40, grad = (uintptr_t)2 << 40, elsewhere = (uintptr_t)3 << 40;
  auto at = [](uintptr_t base, long long floats) { return (float*)(base + (uintptr_t)(floats * 4)); };
  smalfit_fit_args a{};
  a.struct_size = sizeof(a);
  a.num_frames = M; a.logscale_mode = logscale_mode; a.subject_frames = subject_frames;
  const float** ptr[5] = {&a.betas, &a.log_beta_scales, &a.global_rotation, &a.joint_rotations, &a.trans};
  float** gptr[5] = {&a.g_betas, &a.g_log_beta_scales, &a.g_global_rotation, &a.g_joint_rotations, &a.g_trans};
  for (int k = 0; k < 5; ++k) {
    if (!present5[k]) continue;
    *ptr[k] = at(param, offset5[k]);
    *gptr[k] = grad_at_offset5[k] ? at(grad, offset5[k]) : at(elsewhere, 64 * k);
  }
  smalfit_adam_args o{};
  o.param = at(param, 0); o.grad = at(grad, 0); o.exp_avg = at(elsewhere, 1 << 20); o.exp_avg_sq = at(elsewhere, 2 << 20);
  o.num_segments = nseg;
  for (int q = 0; q < nseg && q < 4; ++q) { o.seg_begin[q] = seg_begin[q]; o.seg_end[q] = seg_end[q]; }
  AdamSegments sg;
  if (pack_adam_segments(&o, sg)) return -1;
  const FoldPlan plan = plan_fold(&a, &o, sg);
  for (int k = 0; k < 5; ++k) { train5[k] = plan.train[k]; off5[k] = plan.off[k]; }
  return (int)plan.why;
}

// -> the refusal's text or NULL; sg10: the packed ranges as AdamSegments lays them out (nseg, beg[4], off[5])
const char* hp_pack_adam_segments(const smalfit_adam_args* o, int* sg10) {
  AdamSegments sg;
  const char* why = pack_adam_segments(o, sg);
  if (!why) std::memcpy(sg10, &sg, sizeof(sg));
  static_assert(sizeof(AdamSegments) == 10 * sizeof(int), "nseg, beg[4], off[5]");
  return why;
}

void hp_shared_route(int it, int iterations, int* read_write) {
  const SharedRoute r = shared_route(it, iterations);
  read_write[0] = r.read; read_write[1] = r.write;
}
int hp_restore_slot(int iterations, int shared_trained) { return restore_slot(iterations, shared_trained != 0); }
int hp_prior_slot(int it) { return prior_slot(it); }
int hp_prior_windows(int window, int frame_offset, int M) { return prior_windows(window, frame_offset, M); }
int hp_tensor_is_shared(int k, int logscale_mode) { return tensor_is_shared(k, logscale_mode); }

int hp_padded_verts(int V) { return padded_verts(V); }
int hp_nblk_beta(int Vp) { return nblk_beta(Vp); }
int hp_skin_form(int M, int Vp) { return (int)skin_form(M, Vp); }
int hp_head_blocks(int M, int Vp, int shape_per_frame, int prior) { return head_blocks(M, Vp, shape_per_frame != 0, (HeadPrior)prior); }
void hp_dbeta_grid(int need_beta, int Vp, int betas_shared, int M, int* out3) {
  const DbetaGrid g = dbeta_grid(need_beta != 0, Vp, betas_shared != 0, M);
  out3[0] = g.bx; out3[1] = g.by; out3[2] = g.bz;
}
int hp_parents_ordered(const int* parents, int n) { return parents_ordered(parents, n); }

// tree_levels of 35 parents -> facts6: fast, npass, nlev, passes of the table-driven walk, most children of a non-root joint,
// children of the root; [kTreeMaxPass, kTreeMaxChildren] in limits2.  tables (may be null): pass_joint, pass_parent, pass_nchild
// as [kTreeMaxPass][8] ints each, then pass_child as [kTreeMaxPass][8][kTreeMaxChildren]
void hp_tree_levels(const int* parents35, int* facts6, int* limits2, int* tables) {
  const TreeLevels tl = tree_levels(parents35);
  int most = 0;
  for (int j = 1; j < 35; ++j) most = std::max(most, tl.child_off[j + 1] - tl.child_off[j]);
  const int f[6] = {tl.fast, tl.npass, tl.nlev, tree_walk_passes(tl), most, tl.child_off[1] - tl.child_off[0]};
  for (int i = 0; i < 6; ++i) facts6[i] = f[i];
  limits2[0] = kTreeMaxPass; limits2[1] = kTreeMaxChildren;
  if (!tables) return;
  for (int k = 0; k < kTreeMaxPass; ++k)
    for (int s = 0; s < 8; ++s) {
      tables[k * 8 + s] = tl.pass_joint[k][s];
      tables[(kTreeMaxPass + k) * 8 + s] = tl.pass_parent[k][s];
      tables[(2 * kTreeMaxPass + k) * 8 + s] = tl.pass_nchild[k][s];
      for (int q = 0; q < kTreeMaxChildren; ++q) tables[3 * kTreeMaxPass * 8 + (k * 8 + s) * kTreeMaxChildren + q] = tl.pass_child[k][s][q];
    }
}
const char* hp_model_dims_refusal(int V, int F, int NB) { return model_dims_refusal(V, F, NB); }
const char* hp_fit_model_refusal(int model_betas) { return fit_model_refusal(model_betas); }

void hp_mesh_grids(int S, int V, int P, int* out4) {
  const MeshGrids g = mesh_grids(S, V, P);
  out4[0] = g.bx; out4[1] = g.by; out4[2] = g.bv; out4[3] = g.bp;
}
int hp_mesh_query_blocks(int queries) { return mesh_query_blocks(queries); }
float hp_mesh_weight(float w) { return mesh_weight(w); }
int hp_mesh_points(float w_chamfer, int num_points) { return mesh_points(w_chamfer, num_points); }

const char* hp_fit_args_refusal(const smalfit_fit_args* a, int max_frames, int has_pose_prior, int shape_dim) {
  return fit_args_refusal(a, EngineFacts{max_frames, has_pose_prior != 0, shape_dim});
}
const char* hp_fit_args_size_refusal(const smalfit_fit_args* a) { return fit_args_size_refusal(a); }
int hp_sequence_frames(const smalfit_fit_args* a) { return sequence_frames(a); }

// plan_eval of a block the refusals accept -> ints42 / floats3 in the order of tests/host_plan.py: EVAL_INTS, EVAL_FLOATS
void hp_plan_eval(const smalfit_fit_args* a, int max_frames, int has_pose_prior, int shape_dim, int has_joint_limits, int pending,
                  int assemble, int window_rows, int want_betas, int want_scales, int* ints42, float* floats3) {
  EvalMode mode;
  mode.pending = pending != 0; mode.assemble = assemble != 0;
  mode.window_rows = window_rows != 0; mode.want_betas = want_betas != 0; mode.want_scales = want_scales != 0;
  const EvalPlan p = plan_eval(a, EngineFacts{max_frames, has_pose_prior != 0, shape_dim, has_joint_limits != 0}, mode);
  const int v[42] = {p.M, p.win.window, p.win.offset, p.win.total, p.independent, p.nb, p.betas_stride, p.ls_stride, p.limb_scales,
                     p.shape_prior, p.prior_dim, p.prior_uses_ls, p.prior_windows, p.prior_per_frame, (int)p.head_prior, (int)p.head,
                     p.sil_on, p.rasterise, (int)p.sil_target, p.frame_loss, p.queue_loss, p.raster_backward, (int)p.loss_launch,
                     p.joints_in_head, p.halos, p.verts_out, p.need_pose, p.need_beta, p.need_ls, p.bwd_betas_shared, p.j_stride,
                     p.asm_betas_shared, p.asm_ls_shared, p.ngrp_beta, p.asm_shape_sets, p.rows, p.W, p.ls_rows, p.clear_qloss,
                     p.assembly_leaves_betas, p.assembly_leaves_scales, 0};
  for (int i = 0; i < 42; ++i) ints42[i] = v[i];
  floats3[0] = p.prior_weight; floats3[1] = p.w_temp; floats3[2] = p.w_limit;
}
int hp_window_rows_count(int window, int frame_offset, int M) { return window_rows_count(window, frame_offset, M); }

// the fit path's grids.  [kSweepFaces, kBwdFaces, kBwdLanes, kResEdge, kRectFaces, kAsmElem, kAsmLoss, kAsmRows, kBandBlocks,
// kSelectBlocks, kSelWaves, kSelGroups, PBM_SPLITS, PBM_TILES, kFrameLossStride, kJointBlocks, kSkinVerts, kSkinThreads, kQueueLossBlocks]
void hp_grid_constants(int* out19) {
  const int c[19] = {kSweepFaces, kBwdFaces, kBwdLanes, kResEdge, kRectFaces, kAsmElem, kAsmLoss, kAsmRows, kBandBlocks, kSelectBlocks,
                     kSelWaves, kSelGroups, PBM_SPLITS, PBM_TILES, kFrameLossStride, kJointBlocks, kSkinVerts, kSkinThreads, kQueueLossBlocks};
  for (int i = 0; i < 19; ++i) out19[i] = c[i];
}
int hp_xcd_grid(int blocks_per_frame, int M) { return xcd_grid(blocks_per_frame, M); }
// [frame blocks, face blocks, joint riders, the launch]
void hp_box_grid(int F, int M, int joints, int* out4) {
  out4[0] = box_frame_blocks(M); out4[1] = box_face_blocks(F, M); out4[2] = box_joint_blocks(M, joints != 0); out4[3] = box_grid(F, M, joints != 0);
}
int hp_sweep_grid(int F, int M) { return sweep_grid(F, M); }
int hp_rect_count(int F) { return rect_count(F); }
// [tiles per frame, loss riders, the launch]
void hp_resolve_grid(int S, int M, int loss_frames, int* out3) {
  out3[0] = resolve_tiles(S); out3[1] = resolve_loss_blocks(loss_frames); out3[2] = resolve_grid(resolve_tiles(S), M, loss_frames);
}
int hp_raster_bwd_grid(int F, int M) { return raster_bwd_grid(F, M); }
int hp_vertex_bwd_grid(int Vp, int M) { return vertex_bwd_grid(Vp, M); }
// [pose-blend ids, dA ids, the launch]
void hp_mid_grid(int M, int need_pose, int* out3) {
  out3[0] = mid_pb_ids(M); out3[1] = mid_da_ids(M); out3[2] = mid_grid(M, need_pose ? mid_pb_ids(M) : 0);
}
int hp_chain_grid(int M, int need_beta, int Vp, int betas_shared) { return chain_grid(M, dbeta_grid(need_beta != 0, Vp, betas_shared != 0, M)); }
int hp_assemble_grid(int betas_shared, int M) { return assemble_grid(asm_shape_sets(betas_shared, M)); }
int hp_window_rows_grid(int W) { return window_rows_grid(W); }
int hp_frame_loss_rows_grid(void) { return frame_loss_rows_grid(); }
void hp_skin_grid(int M, int Vp, int* out2) { const Grid2 g = skin_grid(skin_form(M, Vp), M, Vp); out2[0] = g.x; out2[1] = g.y; }
int hp_elem_blocks(long long elements) { return elem_blocks(elements); }

// the other entry points' refusals: the text or NULL
const char* hp_null_argument_refusal(int given) { return null_argument_refusal(given != 0); }
const char* hp_operator_args_refusal(int count, int given) { return operator_args_refusal(count, given != 0); }
const char* hp_step_refusal(int step) { return step_refusal(step); }
const char* hp_iterations_refusal(int iterations) { return iterations_refusal(iterations); }
const char* hp_engine_create_refusal(int given, int max_frames, int image_size) { return engine_create_refusal(given != 0, max_frames, image_size); }
const char* hp_shape_prior_refusal(int given, int dim) { return shape_prior_refusal(given != 0, dim); }
const char* hp_joint_limits_refusal(const float* lo, const float* hi) { return joint_limits_refusal(lo, hi); }
const char* hp_option_refusal(int option, int value) { return option_refusal(option, value); }
const char* hp_profile_begin_refusal(int given, int max_evals, int stride) { return profile_begin_refusal(given != 0, max_evals, stride); }
const char* hp_lbs_args_refusal(const smalfit_lbs_args* a, int max_frames, int model_betas) { return lbs_args_refusal(a, max_frames, model_betas); }
const char* hp_lbs_outputs_refusal(const smalfit_lbs_args* a) { return lbs_outputs_refusal(a); }
const char* hp_render_frames_refusal(int M, int max_frames) { return render_frames_refusal(M, max_frames); }
const char* hp_temporal_frames_refusal(int N, int max_frames) { return temporal_frames_refusal(N, max_frames); }
const char* hp_pose_prior_refusal(int given, int N, int has_pose_prior) { return pose_prior_refusal(given != 0, N, has_pose_prior != 0); }
const char* hp_graph_subject_refusal(int graph_on, const smalfit_fit_args* a) { return graph_subject_refusal(graph_on != 0, a); }
const char* hp_shard_subject_refusal(const smalfit_fit_args* a) { return shard_subject_refusal(a); }
const char* hp_shard_record_refusal(int num_shared, int num_frames, int given) { return shard_record_refusal(num_shared, num_frames, given != 0); }
const char* hp_shard_reduce_refusal(int world_size, int record_stride, int gathered, int num_shared, int num_trainable, const smalfit_adam_args* o) {
  return shard_reduce_refusal(world_size, record_stride, gathered != 0, num_shared, num_trainable, o);
}
const char* hp_shard_run_refusal(const smalfit_fit_args* a, const smalfit_adam_args* ol, const smalfit_adam_args* os, const smalfit_shard_args* sh, int iterations) {
  return shard_run_refusal(a, ol, os, sh, iterations);
}
const char* hp_adam_step_refusal(int count, int given, int t) { return adam_step_refusal(count, given != 0, t); }
const char* hp_window_rows_refusal(const smalfit_fit_args* a, const smalfit_window_rows* r) { return window_rows_refusal(a, r); }


// ---- smalfit_model_create: the data refusals and the packer ----
const char* hp_model_desc_refusal(const smalfit_model_desc* d) { return model_desc_refusal(d, kDefaultLandmarks, 6); }
void hp_default_landmarks(int* out6) { for (int i = 0; i < 6; ++i) out6[i] = kDefaultLandmarks[i]; }
// pack_smal_model and the blob as smalfit_model_create lays it out (the descriptor's arrays must outlive the handle: the parent
// table is referenced, not copied)
struct Packed {
  ModelPackHost p;
  std::array<TableRef, kModelTables> tables;
  size_t off[kModelTables];
  Blob blob;
};
void* hp_pack_model(const smalfit_model_desc* d) {
  Packed* k = new Packed{pack_smal_model(d), {}, {}, {}};
  k->tables = model_tables(k->p, d->parents);
  for (int i = 0; i < kModelTables; ++i) k->off[i] = k->blob.add(k->tables[i].data, k->tables[i].bytes);
  return k;
}
void hp_pack_free(void* h) { delete (Packed*)h; }
int hp_pack_num_tables(void) { return kModelTables; }
// [V, Vp, F, NB, Kw, Kj]
void hp_pack_dims(const void* h, int* out6) {
  const ModelPackHost& p = ((const Packed*)h)->p;
  const int v[6] = {p.V, p.Vp, p.F, p.NB, p.Kw, p.Kj};
  for (int i = 0; i < 6; ++i) out6[i] = v[i];
}
// table i in the order of model_tables -> its bytes; its offset in the blob
const void* hp_pack_table(const void* h, int i, unsigned long long* bytes, unsigned long long* offset) {
  const Packed* k = (const Packed*)h;
  *bytes = k->tables[i].bytes; *offset = k->off[i];
  return k->tables[i].data;
}
const void* hp_pack_blob(const void* h, unsigned long long* bytes) {
  const Packed* k = (const Packed*)h;
  *bytes = k->blob.bytes.size();
  return k->blob.bytes.data();
}

// ---- the mesh objective and smalfit_fit3d_step ----
const char* hp_null_handle_refusal(int given) { return null_handle_refusal(given != 0); }
const char* hp_mesh_objective_create_refusal(int given, int max_meshes, int max_points) { return mesh_objective_create_refusal(given != 0, max_meshes, max_points); }
const char* hp_mesh_eval_refusal(int num_meshes, int max_meshes, float w_chamfer, int points, int num_points, int max_points) {
  return mesh_eval_refusal(num_meshes, max_meshes, w_chamfer, points != 0, num_points, max_points);
}
const char* hp_mesh_targets_create_refusal(int given, int num_meshes, const int* vert_counts, const int* face_counts) {
  return mesh_targets_create_refusal(given != 0, num_meshes, vert_counts, face_counts);
}
const char* hp_mesh_sample_refusal(int given, int num_points) { return mesh_sample_refusal(given != 0, num_points); }
// facts8: max_frames, model_verts, model_betas, max_meshes, max_points, objective_verts, targets given, target meshes
const char* hp_fit3d_args_refusal(const smalfit_fit3d_args* a, const int* f) {
  return fit3d_args_refusal(a, Fit3dFacts{f[0], f[1], f[2], f[3], f[4], f[5], f[6] != 0, f[7]});
}
// plan_fit3d -> ints8: chamfer, points, need_pose, need_beta, planar_vertex_grad, any_trained, nseg, adam_blocks;
// segs: nseg x (tensor, count, row_len, g_stride, g_offset, block0)
void hp_plan_fit3d(const smalfit_fit3d_args* a, int model_verts, int* ints8, int* segs30) {
  const Fit3dPlan p = plan_fit3d(a, model_verts);
  const int v[8] = {p.chamfer, (int)p.points, p.need_pose, p.need_beta, p.planar_vertex_grad, p.any_trained, p.nseg, p.adam_blocks};
  for (int i = 0; i < 8; ++i) ints8[i] = v[i];
  for (int s = 0; s < p.nseg; ++s) {
    const Fit3dAdamGeometry& g = p.seg[s];
    const int w[6] = {g.tensor, g.count, g.row_len, g.g_stride, g.g_offset, g.block0};
    for (int i = 0; i < 6; ++i) segs30[s * 6 + i] = w[i];
  }
}
// plan_fit3d_riders (any block may be NULL; points: Fit3dPoints) -> ints7: draw_normals, draw_boundary, surface_normals,
// chamfer_normals, chamfer_boundary, vert_normals, surface_reuses_vert_normals
void hp_plan_fit3d_riders(const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate, const smalfit_chamfer_gate_args* cg,
                          float w_chamfer, int points, int* ints7) {
  const Fit3dRiders r = plan_fit3d_riders(sf, gate, cg, w_chamfer, (Fit3dPoints)points);
  const int v[7] = {r.draw_normals, r.draw_boundary, (int)r.surface_normals, (int)r.chamfer_normals, (int)r.chamfer_boundary,
                    (int)r.vert_normals, r.surface_reuses_vert_normals};
  for (int i = 0; i < 7; ++i) ints7[i] = v[i];
}
// [kFit3dParams, sizeof(Fit3dAdamSeg), sizeof(Fit3dAdamArgs), sizeof(smalfit_fit3d_args)]
void hp_fit3d_constants(int* out4) {
  out4[0] = kFit3dParams; out4[1] = (int)sizeof(Fit3dAdamSeg); out4[2] = (int)sizeof(Fit3dAdamArgs); out4[3] = (int)sizeof(smalfit_fit3d_args);
}
int hp_mesh_compose_blocks(int N, int V) { return mesh_compose_blocks(N, V); }
void hp_mesh_sample_grid(int S, int N, int* out2) { const Grid2 g = mesh_sample_grid(S, N); out2[0] = g.x; out2[1] = g.y; }
int hp_fit3d_adam_blocks(int count) { return fit3d_adam_blocks(count); }
int hp_frame_betas_grid(int M) { return frame_betas_grid(M); }

}  // extern "C"

// TEST-ONLY host build (g++) of the host's launch decisions (smalify_amd/csrc/smalfit_plan.h): extern "C" wrappers over the
// very functions smalfit_launch.inc and smalfit_mesh3d.inc call, so that the CPU tests compare the Python restatements
// (tests/fold_forms.py, lbs_forms.py, mesh3d_forms.py) with the rules themselves.  Never part of the product.
#include <cstdint>
#include <cstring>

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

}  // extern "C"

// Host side of the rigid pre-alignment (smalfit_rigid_aligner_create / _destroy, smalfit_rigid_align, _trimmed): the handle's work buffers and
// the launches of kernels_rigid_align.inc.  Included at the end of smalfit_kernels.hip, after smalfit_launch.inc (fail, refused,
// Carver, LAUNCH_OK).  What is refused and how the grids are sized is smalfit_plan.h.
#include <limits>

struct smalfit_rigid_aligner {
  int max_meshes = 0, max_verts = 0, max_points = 0, max_starts = 0;
  void* work = nullptr;
  float* cen = nullptr;      // [max_meshes][6]
  float* part_v = nullptr;   // [max_meshes][max_starts][query blocks over max_verts][kRigidMoments]
  float* part_p = nullptr;   // [max_meshes][max_starts][query blocks over max_points][kRigidMoments]
  // the trimmed calls' own buffers, allocated by the first of them: every query's d^2 and match of a round
  void* trim_work = nullptr;
  float* qd2_v = nullptr;    // [max_meshes][max_starts][max_verts]
  int* qnn_v = nullptr;
  float* qd2_p = nullptr;    // [max_meshes][max_starts][max_points]
  int* qnn_p = nullptr;
};

// the launches of one call; trim == nullptr: smalfit_rigid_align's own, else a selection between the scans and the solve of every round
static int rigid_align_launch(smalfit_rigid_aligner* r, void* stream, const smalfit_rigid_align_args* a,
                              const smalfit_rigid_trim_args* trim);

extern "C" {

int smalfit_rigid_aligner_create(int max_meshes, int max_verts, int max_points, int max_starts, smalfit_rigid_aligner** out) {
  if (refused("smalfit_rigid_aligner_create", rigid_aligner_create_refusal(out != nullptr, max_meshes, max_verts, max_points, max_starts)))
    return 1;
  auto* r = new smalfit_rigid_aligner();
  r->max_meshes = max_meshes; r->max_verts = max_verts; r->max_points = max_points; r->max_starts = max_starts;
  const size_t NK = (size_t)max_meshes * max_starts;
  Carver w;
  w.field(r->cen, (size_t)max_meshes * 6);
  w.field(r->part_v, NK * mesh_query_blocks(max_verts) * kRigidMoments);
  w.field(r->part_p, NK * mesh_query_blocks(max_points) * kRigidMoments);
  auto bail = [&](const char* what) {
    smalfit_rigid_aligner_destroy(r);
    return refused("smalfit_rigid_aligner_create", what);
  };
  if (hipMalloc(&r->work, w.bytes) != hipSuccess) return bail("hipMalloc of the work buffers failed (no HIP device?)");
  if (hipMemset(r->work, 0, w.bytes) != hipSuccess) return bail("hipMemset failed");
  w.point(r->work);
  *out = r;
  return 0;
}

void smalfit_rigid_aligner_destroy(smalfit_rigid_aligner* r) {
  if (!r) return;
  if (r->work) (void)hipFree(r->work);
  if (r->trim_work) (void)hipFree(r->trim_work);
  delete r;
}

int smalfit_rigid_align(smalfit_rigid_aligner* r, void* stream, const smalfit_rigid_align_args* a) {
  const char* who = "smalfit_rigid_align";
  if (refused(who, null_argument_refusal(r && a))) return 1;
  if (refused(who, rigid_align_args_refusal(a, RigidAlignFacts{r->max_meshes, r->max_verts, r->max_points, r->max_starts}))) return 1;
  return rigid_align_launch(r, stream, a, nullptr);
}

int smalfit_trimmed_rigid_align(smalfit_rigid_aligner* r, void* stream, const smalfit_rigid_align_args* a, const smalfit_rigid_trim_args* trim) {
  const char* who = "smalfit_trimmed_rigid_align";
  if (refused(who, null_argument_refusal(r && a))) return 1;
  if (refused(who, rigid_align_args_refusal(a, RigidAlignFacts{r->max_meshes, r->max_verts, r->max_points, r->max_starts}))) return 1;
  const RigidTrimFacts f{a->num_verts, a->num_points, a->w_vert > 0.f, a->w_point > 0.f};
  if (trim && refused(who, rigid_trim_args_refusal(trim, f))) return 1;
  if (rigid_trim_on(trim, f)) {
    if (!r->trim_work) {
      const size_t NK = (size_t)r->max_meshes * r->max_starts;
      Carver w;
      w.field(r->qd2_v, NK * r->max_verts);
      w.field(r->qnn_v, NK * r->max_verts);
      w.field(r->qd2_p, NK * r->max_points);
      w.field(r->qnn_p, NK * r->max_points);
      if (hipMalloc(&r->trim_work, w.bytes) != hipSuccess) {
        r->trim_work = nullptr;
        return refused(who, "hipMalloc of the trimming buffers failed");
      }
      w.point(r->trim_work);
    }
    return rigid_align_launch(r, stream, a, trim);
  }
  // off: smalfit_rigid_align launch for launch; every query of a direction that is on is kept and no threshold was formed
  if (trim) {
    hipStream_t st = (hipStream_t)stream;
    const size_t NK = (size_t)a->num_meshes * a->num_starts;
    if (trim->vert_kept && f.vert_dir && hipMemsetAsync(trim->vert_kept, 1, NK * a->num_verts, st) != hipSuccess) return refused(who, "hipMemsetAsync failed");
    if (trim->point_kept && f.point_dir && hipMemsetAsync(trim->point_kept, 1, NK * a->num_points, st) != hipSuccess) return refused(who, "hipMemsetAsync failed");
    if (trim->trim_d2 && hipMemsetAsync(trim->trim_d2, 0, NK * 2 * sizeof(float), st) != hipSuccess) return refused(who, "hipMemsetAsync failed");
  }
  return rigid_align_launch(r, stream, a, nullptr);
}

}  // extern "C"

static int rigid_align_launch(smalfit_rigid_aligner* r, void* stream, const smalfit_rigid_align_args* a,
                              const smalfit_rigid_trim_args* trim) {
  hipStream_t st = (hipStream_t)stream;
  RigidArgs k{};
  k.N = a->num_meshes; k.V = a->num_verts; k.S = a->num_points; k.K = a->num_starts;
  k.verts = a->verts; k.points = a->points; k.T = a->transforms;
  k.cen = r->cen; k.part_v = r->part_v; k.part_p = r->part_p;
  const Grid3 gv = rigid_scan_grid(k.V, k.K, k.N), gp = rigid_scan_grid(k.S, k.K, k.N);
  k.bv = gv.x; k.bp = gp.x;
  RigidStarts starts{};
  if (!a->start_transforms)
    for (int s = 0; s < k.K; ++s) {
      if (a->starts) std::memcpy(starts.R[s], a->starts + 9 * (size_t)s, 9 * sizeof(float));
      else rigid_cube_rotation(s, starts.R[s]);
    }
  rigid_init_kernel<<<rigid_init_blocks(k.N), 256, 0, st>>>(k, starts, a->start_transforms);
  LAUNCH_OK("rigid_init_kernel");
  RigidSolveArgs s{};
  s.wv = a->w_vert / (float)k.V; s.wp = a->w_point / (float)k.S;
  // (a positive weight whose quotient underflows to 0 would switch its direction off half way: the direction follows the weight)
  const bool vert_dir = a->w_vert > 0.f, point_dir = a->w_point > 0.f;
  if (vert_dir && !(s.wv > 0.f)) s.wv = std::numeric_limits<float>::min();
  if (point_dir && !(s.wp > 0.f)) s.wp = std::numeric_limits<float>::min();
  s.iterations = a->iterations; s.scores = a->scores; s.kept_rotation = a->kept_rotation; s.history = a->history;
  const Grid2 gs = rigid_solve_grid(k.K, k.N);
  RigidTrimArgs t{};
  const Grid3 gt = rigid_trim_grid(vert_dir, point_dir, k.K, k.N);
  if (trim) {
    k.qd2_v = r->qd2_v; k.qnn_v = r->qnn_v; k.qd2_p = r->qd2_p; k.qnn_p = r->qnn_p;
    t.first_dir = vert_dir ? 0 : 1; t.dirs = gt.x;
    t.keep_v = trim->keep_vert; t.keep_p = trim->keep_point;
  }
  for (int it = 0; it <= a->iterations; ++it) {
    const bool last = it == a->iterations;
    k.vert_nn = last ? a->vert_nn : nullptr;
    k.point_nn = last ? a->point_nn : nullptr;
    if (vert_dir) {
      if (trim) rigid_scan_kernel<0, true><<<dim3(gv.x, gv.y, gv.z), 256, 0, st>>>(k);
      else rigid_scan_kernel<0><<<dim3(gv.x, gv.y, gv.z), 256, 0, st>>>(k);
      LAUNCH_OK("rigid_scan_kernel<0>");
    }
    if (point_dir) {
      if (trim) rigid_scan_kernel<1, true><<<dim3(gp.x, gp.y, gp.z), 256, 0, st>>>(k);
      else rigid_scan_kernel<1><<<dim3(gp.x, gp.y, gp.z), 256, 0, st>>>(k);
      LAUNCH_OK("rigid_scan_kernel<1>");
    }
    if (trim) {
      t.vert_kept = last ? trim->vert_kept : nullptr;
      t.point_kept = last ? trim->point_kept : nullptr;
      t.trim_d2 = last ? trim->trim_d2 : nullptr;
      rigid_trim_kernel<<<dim3(gt.x, gt.y, gt.z), 256, 0, st>>>(k, t);
      LAUNCH_OK("rigid_trim_kernel");
    }
    s.it = it;
    rigid_solve_kernel<<<dim3(gs.x, gs.y), 64, 0, st>>>(k, s);
    LAUNCH_OK("rigid_solve_kernel");
  }
  rigid_pick_kernel<<<rigid_pick_blocks(k.N), 64, 0, st>>>(k.N, k.K, a->scores, a->transforms, a->best, a->best_transform);
  LAUNCH_OK("rigid_pick_kernel");
  return 0;
}

// Host side of the rigid pre-alignment (smalfit_rigid_aligner_create / _destroy, smalfit_rigid_align): the handle's work buffers and
// the launches of kernels_rigid_align.inc.  Included at the end of smalfit_kernels.hip, after smalfit_launch.inc (fail, refused,
// Carver, LAUNCH_OK).  What is refused and how the grids are sized is smalfit_plan.h.
#include <limits>

struct smalfit_rigid_aligner {
  int max_meshes = 0, max_verts = 0, max_points = 0, max_starts = 0;
  void* work = nullptr;
  float* cen = nullptr;      // [max_meshes][6]
  float* part_v = nullptr;   // [max_meshes][max_starts][query blocks over max_verts][kRigidMoments]
  float* part_p = nullptr;   // [max_meshes][max_starts][query blocks over max_points][kRigidMoments]
};

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
  delete r;
}

int smalfit_rigid_align(smalfit_rigid_aligner* r, void* stream, const smalfit_rigid_align_args* a) {
  const char* who = "smalfit_rigid_align";
  if (refused(who, null_argument_refusal(r && a))) return 1;
  if (refused(who, rigid_align_args_refusal(a, RigidAlignFacts{r->max_meshes, r->max_verts, r->max_points, r->max_starts}))) return 1;
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
  for (int it = 0; it <= a->iterations; ++it) {
    const bool last = it == a->iterations;
    k.vert_nn = last ? a->vert_nn : nullptr;
    k.point_nn = last ? a->point_nn : nullptr;
    if (vert_dir) {
      rigid_scan_kernel<0><<<dim3(gv.x, gv.y, gv.z), 256, 0, st>>>(k);
      LAUNCH_OK("rigid_scan_kernel<0>");
    }
    if (point_dir) {
      rigid_scan_kernel<1><<<dim3(gp.x, gp.y, gp.z), 256, 0, st>>>(k);
      LAUNCH_OK("rigid_scan_kernel<1>");
    }
    s.it = it;
    rigid_solve_kernel<<<dim3(gs.x, gs.y), 64, 0, st>>>(k, s);
    LAUNCH_OK("rigid_solve_kernel");
  }
  rigid_pick_kernel<<<rigid_pick_blocks(k.N), 64, 0, st>>>(k.N, k.K, a->scores, a->transforms, a->best, a->best_transform);
  LAUNCH_OK("rigid_pick_kernel");
  return 0;
}

}  // extern "C"

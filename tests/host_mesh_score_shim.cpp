// smalify_amd/csrc/mesh3d_math.h (the point-to-triangle maths of smalfit_mesh_score) and smalfit_plan.h (its rules, grids and
// chunk size) as C functions for tests/test_mesh_score_cpu.py and tests/test_gpu_mesh_score.py.  Built by g++
// (tests/host_mesh_score.py), no HIP: the kernels and this shim evaluate the same code.
#include <cmath>
#include <cstddef>

#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {
// out[i] = sqrtf(point_triangle_dist2(p[i], a[i], b[i], c[i])): count independent pairs, every array (count, 3)
void hms_point_triangle_dist(int count, const float* p, const float* a, const float* b, const float* c, float* out) {
  for (int i = 0; i < count; ++i) {
    const size_t o = 3 * (size_t)i;
    out[i] = sqrtf(point_triangle_dist2(p + o, a + o, b + o, c + o));
  }
}
// out[i] = the least distance from q[i] to the triangles (verts, faces), as mesh3d_surface_dist_kernel forms it: the staged
// record, the scan, the square root of the minimum
void hms_surface_dist(int num_queries, const float* q, const float* verts, int num_faces, const int* faces, float* out) {
  for (int i = 0; i < num_queries; ++i) {
    float best = INFINITY;
    for (int f = 0; f < num_faces; ++f) {
      const ScanTri t = make_scan_tri(verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1],
                                      verts + 3 * (size_t)faces[3 * f + 2]);
      best = surface_scan(q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2], &t, 0, 1, best);
    }
    out[i] = sqrtf(best);
  }
}
int hms_sizeof_scan_tri() { return (int)sizeof(ScanTri); }

// the block is laid out by the caller (ctypes mirror of smalify_amd/_lib.py); nullptr = accepted
const char* hms_mesh_score_args_refusal(const smalfit_mesh_score_args* a, int max_meshes, int max_points, int target_meshes) {
  return mesh_score_args_refusal(a, MeshScoreFacts{max_meshes, max_points, target_meshes});
}
int hms_sizeof_args() { return (int)sizeof(smalfit_mesh_score_args); }
// offsets in the order of the declaration; returns how many
int hms_offsets(int* out) {
  const size_t o[] = {offsetof(smalfit_mesh_score_args, struct_size), offsetof(smalfit_mesh_score_args, num_meshes),
                      offsetof(smalfit_mesh_score_args, verts), offsetof(smalfit_mesh_score_args, points),
                      offsetof(smalfit_mesh_score_args, num_points), offsetof(smalfit_mesh_score_args, num_thresholds),
                      offsetof(smalfit_mesh_score_args, thresholds), offsetof(smalfit_mesh_score_args, vert_dist),
                      offsetof(smalfit_mesh_score_args, point_dist), offsetof(smalfit_mesh_score_args, sums),
                      offsetof(smalfit_mesh_score_args, within)};
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
int hms_max_thresholds() { return SMALFIT_MAX_SCORE_THRESHOLDS; }
int hms_surface_chunk() { return kSurfaceChunk; }
int hms_queries() { return kMeshQueries; }
void hms_surface_dist_grid(int queries, int N, int* out) { const Grid2 g = surface_dist_grid(queries, N); out[0] = g.x; out[1] = g.y; }
void hms_score_reduce_grid(int N, int* out) { const Grid2 g = score_reduce_grid(N); out[0] = g.x; out[1] = g.y; }
}

// smalify_amd/csrc/mesh3d_math.h (the closest point on a triangle, the nearest-face scan and the vertex gather of the surface term)
// and smalfit_plan.h (its rules, slice count and grids, the points a step takes) as C functions for
// tests/test_surface_term_cpu.py and tests/test_gpu_surface_term.py.  Built by g++ (tests/host_surface_term.py), no HIP: the
// kernels and this shim evaluate the same code.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {
// count independent pairs, every array (count, 3): d2 (count), bary (count, 3), r (count, 3) of point_triangle_closest, and
// dist2 (count) of point_triangle_dist2 beside it
void hst_closest(int count, const float* p, const float* a, const float* b, const float* c, float* d2, float* bary, float* r,
                 float* dist2) {
  for (int i = 0; i < count; ++i) {
    const size_t o = 3 * (size_t)i;
    const TriHit h = point_triangle_closest(p + o, a + o, b + o, c + o);
    d2[i] = h.d2;
    for (int k = 0; k < 3; ++k) {
      bary[o + k] = h.b[k];
      r[o + k] = h.r[k];
    }
    dist2[i] = point_triangle_dist2(p + o, a + o, b + o, c + o);
  }
}
// every query against the triangles (verts, faces) as the kernels do it: staged records, the scan in `slices` spans whose
// minima meet in the 64-bit key, the closest point on the face the key names
void hst_nearest(int num_queries, const float* q, const float* verts, int num_faces, const int* faces, int slices, int* face,
                 float* d2, float* bary, float* r) {
  const int span = surface_slice_span(num_faces, slices);
  for (int i = 0; i < num_queries; ++i) {
    const float* p = q + 3 * (size_t)i;
    unsigned long long key = ~0ull;
    for (int z = 0; z < slices; ++z) {
      float best = INFINITY;
      int bidx = 0x7fffffff;
      for (int f = z * span; f < num_faces && f < (z + 1) * span; ++f) {
        const ScanTri t = make_scan_tri(verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1],
                                        verts + 3 * (size_t)faces[3 * f + 2]);
        surface_scan_nearest(p[0], p[1], p[2], &t, 0, 1, f, best, bidx);
      }
      if (bidx == 0x7fffffff) continue;
      unsigned bits;
      std::memcpy(&bits, &best, 4);
      const unsigned long long k = ((unsigned long long)bits << 32) | (unsigned)bidx;
      if (k < key) key = k;
    }
    const int f = key == ~0ull ? 0 : (int)(unsigned)(key & 0xFFFFFFFFull);
    const TriHit h = point_triangle_closest(p, verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1],
                                            verts + 3 * (size_t)faces[3 * f + 2]);
    face[i] = f;
    const unsigned bits = (unsigned)(key >> 32);
    std::memcpy(&d2[i], &bits, 4);
    if (key == ~0ull) d2[i] = h.d2;
    for (int k = 0; k < 3; ++k) {
      bary[3 * (size_t)i + k] = h.b[k];
      r[3 * (size_t)i + k] = h.r[k];
    }
  }
}
// g (V, 3) = sum over the S hits of the share of every vertex, as mesh3d_surface_grad_kernel gathers it (one range)
void hst_gather(int V, int S, const int* corners /* (S,3) */, const float* bary, const float* r, float* g) {
  SurfaceHit* h = new SurfaceHit[S > 0 ? S : 1];
  for (int j = 0; j < S; ++j) {
    h[j] = SurfaceHit{corners[3 * j], corners[3 * j + 1], corners[3 * j + 2], bary[3 * j], bary[3 * j + 1], bary[3 * j + 2],
                      r[3 * j], r[3 * j + 1], r[3 * j + 2], 0.f, 0.f, 0.f};
  }
  for (int v = 0; v < V; ++v) {
    float acc[3] = {0.f, 0.f, 0.f};
    surface_hit_gather(h, 0, S, v, acc);
    for (int k = 0; k < 3; ++k) g[3 * v + k] = acc[k];
  }
  delete[] h;
}
int hst_sizeof_hit() { return (int)sizeof(SurfaceHit); }

// the block is laid out by the caller (ctypes mirror of smalify_amd/_lib.py); nullptr = accepted
const char* hst_refusal(const smalfit_surface_term_args* a, int max_meshes, int max_points, int targets, int target_meshes, int step,
                        int step_meshes, int step_points, int step_has_points) {
  return surface_term_args_refusal(a, SurfaceTermFacts{max_meshes, max_points, targets != 0, target_meshes, step != 0, step_meshes,
                                                       step_points, step_has_points != 0});
}
int hst_term_on(const smalfit_surface_term_args* a) { return surface_term_on(a) ? 1 : 0; }
int hst_sizeof_args() { return (int)sizeof(smalfit_surface_term_args); }
int hst_sizeof_fit3d_args() { return (int)sizeof(smalfit_fit3d_args); }
// offsets in the order of the declaration; returns how many
int hst_offsets(int* out) {
#define OFF(f) offsetof(smalfit_surface_term_args, f)
  const size_t o[] = {OFF(struct_size), OFF(num_meshes), OFF(w_point_surface), OFF(w_vert_surface), OFF(verts), OFF(points),
                      OFF(num_points), OFF(losses), OFF(rows), OFF(dverts), OFF(dtrans), OFF(point_face), OFF(point_bary),
                      OFF(vert_face), OFF(vert_bary), OFF(point_residual), OFF(vert_residual), OFF(step_total)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
int hst_surface_slices(int queries, int faces, int N) { return surface_slices(queries, faces, N); }
int hst_surface_slice_span(int faces, int slices) { return surface_slice_span(faces, slices); }
void hst_surface_near_grid(int queries, int faces, int N, int* out) {
  const Grid3 g = surface_near_grid(queries, faces, N);
  out[0] = g.x; out[1] = g.y; out[2] = g.z;
}
void hst_surface_hit_grid(int queries, int N, int* out) { const Grid2 g = surface_hit_grid(queries, N); out[0] = g.x; out[1] = g.y; }
void hst_surface_grad_grid(int V, int N, int* out) { const Grid2 g = surface_grad_grid(V, N); out[0] = g.x; out[1] = g.y; }
int hst_target_blocks() { return kSurfaceTargetBlocks; }
int hst_min_slice() { return kSurfaceMinSlice; }
int hst_hit_chunk() { return kSurfaceHitChunk; }
int hst_surface_chunk() { return kSurfaceChunk; }
// Fit3dPoints of a step: chamfer weight, the caller's points / points_out given, the point-surface term on
int hst_fit3d_points(float w_chamfer, int points, int points_out, int same, int point_surface) {
  static float dummy[2];
  smalfit_fit3d_args a{};
  a.num_meshes = 1; a.num_betas = 20; a.num_points = 8;
  a.weights[0] = w_chamfer;
  a.points = points ? dummy : nullptr;
  a.points_out = points_out ? (same ? dummy : dummy + 1) : nullptr;
  return (int)plan_fit3d(&a, 8, point_surface != 0).points;
}
}

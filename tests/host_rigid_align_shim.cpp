// The host side of the rigid pre-alignment as C functions for tests/test_rigid_align_cpu.py and tests/test_gpu_rigid_align.py:
// rigid_align_math.h (the transform chain, the pair sums, the solve, the 24 built-in starts), mesh3d_math.h (the scan the kernels
// call) and smalfit_plan.h (the refusals, the grids).  Built by g++ without contraction (tests/host_rigid_align.py), no HIP: the
// kernels and this shim evaluate the same code.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/rigid_align_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

namespace {
// the means as the header words them: 256 lanes, lane l the elements l, l + 256, ...; a wave's 64 lanes by the xor butterfly, the
// four waves in wave order
float strided_mean(const float* src, int count, int c) {
  float lane[256];
  for (int l = 0; l < 256; ++l) {
    float s = 0.f;
    for (int i = l; i < count; i += 256) s += src[3 * (size_t)i + c];
    lane[l] = s;
  }
  float total = 0.f;
  for (int w = 0; w < 4; ++w) {
    float v[64], t[64];
    for (int l = 0; l < 64; ++l) v[l] = lane[64 * w + l];
    for (int o = 32; o > 0; o >>= 1) {
      for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ o];
      for (int l = 0; l < 64; ++l) v[l] = t[l];
    }
    total += v[0];
  }
  return total / (float)count;
}

// one direction's scan for every query: dir 0 the transformed vertices ask the points, dir 1 the points ask the transformed
// vertices; ascending order with strict '<' is the kernels' merged result (nearest_merge is lexicographic)
void scan_direction(int dir, const float* T, int V, const float* x, int S, const float* p, int* idx, float* d2) {
  const int nq = dir == 0 ? V : S, no = dir == 0 ? S : V;
  std::vector<ScanPoint> rec(no);
  for (int j = 0; j < no; ++j) {
    const float* src = (dir == 0 ? p : x) + 3 * (size_t)j;
    float z[3] = {src[0], src[1], src[2]};
    if (dir == 1) rigid_apply(T, src[0], src[1], src[2], z);
    rec[j] = ScanPoint{z[0], z[1], z[2], 0};
  }
  for (int i = 0; i < nq; ++i) {
    const float* src = (dir == 0 ? x : p) + 3 * (size_t)i;
    float q[3] = {src[0], src[1], src[2]};
    if (dir == 0) rigid_apply(T, src[0], src[1], src[2], q);
    float best = INFINITY, g[3] = {0.f, 0.f, 0.f};
    int bi = 0x7fffffff;
    nearest_scan<false>(q[0], q[1], q[2], rec.data(), 0, no, 0, best, bi, 0, g);
    idx[i] = (unsigned)bi < (unsigned)no ? bi : -1;
    d2[i] = best;
  }
}

// the sums of one direction's pairs in plain ascending order (the kernels add blocks of 64; the order is the host's own here)
void direction_moments(int dir, int V, const float* x, int S, const float* p, const int* idx, const float* d2, const float* cX,
                       const float* cP, float* m) {
  const int nq = dir == 0 ? V : S;
  for (int i = 0; i < kRigidMoments; ++i) m[i] = 0.f;
  for (int i = 0; i < nq; ++i) {
    float one[kRigidMoments] = {};
    if (idx[i] >= 0) {
      const float* xs = x + 3 * (size_t)(dir == 0 ? i : idx[i]);
      const float* ps = p + 3 * (size_t)(dir == 0 ? idx[i] : i);
      const float xc[3] = {xs[0] - cX[0], xs[1] - cX[1], xs[2] - cX[2]}, pc[3] = {ps[0] - cP[0], ps[1] - cP[1], ps[2] - cP[2]};
      rigid_pair_moments(xc, pc, d2[i], one);
    }
    one[kRigidMoments - 1] = d2[i];
    for (int k = 0; k < kRigidMoments; ++k) m[k] += one[k];
  }
}
}  // namespace

extern "C" {
void hra_constants(float* out) {
  out[0] = (float)kRigidMoments; out[1] = (float)kRigidSweeps; out[2] = kRigidRankEps; out[3] = (float)kRigidCubeRotations;
  out[4] = (float)kRigidMaxIterations; out[5] = (float)kRigidStartTolerance; out[6] = (float)kMeshQueries;
}
void hra_apply(const float* T, int count, const float* x, float* out) {
  for (int i = 0; i < count; ++i) rigid_apply(T, x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], out + 3 * (size_t)i);
}
void hra_means(int count, const float* x, float* out) {
  for (int c = 0; c < 3; ++c) out[c] = strided_mean(x, count, c);
}
void hra_cube_rotation(int k, float* R) { rigid_cube_rotation(k, R); }
void hra_start_transform(const float* R, const float* cX, const float* cP, float* T) { rigid_start_transform(R, cX, cP, T); }
// dir 0: idx / d2 of the V vertices; dir 1: of the S points (-1: no match)
void hra_nearest(int dir, const float* T, int V, const float* x, int S, const float* p, int* idx, float* d2) {
  scan_direction(dir, T, V, x, S, p, idx, d2);
}
void hra_pair_moments(const float* xc, const float* pc, float d2, float* m) { rigid_pair_moments(xc, pc, d2, m); }
// mv / mp may be NULL: the direction is skipped
void hra_combine(const float* mv, const float* mp, float wv, float wp, float* M) { rigid_combine(mv, mp, wv, wp, M); }
// out2: l1 - l2 and the scale of the rank test; returns 1 when the previous rotation was kept
int hra_solve(const float* M, const float* cX, const float* cP, const float* prev, float* T, float* out2) {
  return rigid_solve(M, cX, cP, prev, T, out2, out2 + 1);
}
// one whole iteration in float32 from transform Tin: scans (the directions with a positive weight), sums, solve.  cost: the cost
// before the solve; idx_v (V) / idx_p (S) may be NULL.  Returns 1 when the rotation was kept
int hra_iterate(int V, const float* x, int S, const float* p, const float* Tin, float w_point, float w_vert, float* Tout, float* cost,
                int* idx_v, int* idx_p) {
  float cX[3], cP[3];
  hra_means(V, x, cX);
  hra_means(S, p, cP);
  std::vector<int> iv(V), ip(S);
  std::vector<float> dv(V), dp(S);
  float mv[kRigidMoments], mp[kRigidMoments], M[kRigidMoments];
  if (w_vert > 0.f) {
    scan_direction(0, Tin, V, x, S, p, iv.data(), dv.data());
    direction_moments(0, V, x, S, p, iv.data(), dv.data(), cX, cP, mv);
    if (idx_v) std::copy(iv.begin(), iv.end(), idx_v);
  }
  if (w_point > 0.f) {
    scan_direction(1, Tin, V, x, S, p, ip.data(), dp.data());
    direction_moments(1, V, x, S, p, ip.data(), dp.data(), cX, cP, mp);
    if (idx_p) std::copy(ip.begin(), ip.end(), idx_p);
  }
  rigid_combine(w_vert > 0.f ? mv : nullptr, w_point > 0.f ? mp : nullptr, w_vert / (float)V, w_point / (float)S, M);
  *cost = M[kRigidMoments - 1];
  return rigid_solve(M, cX, cP, Tin, Tout);
}
// facts: the handle's max_meshes, max_verts, max_points, max_starts; nullptr = accepted
const char* hra_refusal(const smalfit_rigid_align_args* a, const int* f) {
  return rigid_align_args_refusal(a, RigidAlignFacts{f[0], f[1], f[2], f[3]});
}
const char* hra_create_refusal(int given, int max_meshes, int max_verts, int max_points, int max_starts) {
  return rigid_aligner_create_refusal(given != 0, max_meshes, max_verts, max_points, max_starts);
}
const char* hra_start_refusal(const float* R) { return rigid_start_refusal(R); }
// out: the vertex scan's grid (3), the point scan's (3), the solve's (2), init blocks, pick blocks, launches with both directions,
// with one
void hra_grids(int V, int S, int K, int N, int iterations, int* out) {
  const Grid3 gv = rigid_scan_grid(V, K, N), gp = rigid_scan_grid(S, K, N);
  const Grid2 gs = rigid_solve_grid(K, N);
  out[0] = gv.x; out[1] = gv.y; out[2] = gv.z; out[3] = gp.x; out[4] = gp.y; out[5] = gp.z; out[6] = gs.x; out[7] = gs.y;
  out[8] = rigid_init_blocks(N); out[9] = rigid_pick_blocks(N);
  out[10] = rigid_align_launches(iterations, true, true); out[11] = rigid_align_launches(iterations, true, false);
}
int hra_sizeof_args() { return (int)sizeof(smalfit_rigid_align_args); }
// offsets in the order of the declaration; returns how many
int hra_offsets(int* out) {
#define OFF(f) offsetof(smalfit_rigid_align_args, f)
  const size_t o[] = {OFF(struct_size), OFF(num_meshes), OFF(num_verts), OFF(num_points), OFF(verts), OFF(points), OFF(num_starts),
                      OFF(iterations), OFF(starts), OFF(start_transforms), OFF(w_point), OFF(w_vert), OFF(transforms), OFF(scores),
                      OFF(best), OFF(best_transform), OFF(kept_rotation), OFF(history), OFF(vert_nn), OFF(point_nn)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}

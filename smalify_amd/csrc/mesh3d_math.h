// Per-element maths of the 3D mesh-fitting objective, shared by kernels_mesh3d.inc and by the
// test-only host shim (tests/host_mesh3d_shim.cpp).  SMALFIT_HD as in smalfit_math.h.
//
// Reference behaviour restated here: fitter_3d/trainer.py:205-227 (Stage.forward) calls PyTorch3D v0.2.5
//   sample_points_from_meshes  -> sample_face / barycentric_sample   (area-weighted face, sqrt-u barycentric map)
//   chamfer_distance           -> nearest_scan                       (squared distance, K = 1, ties -> lowest index)
//   mesh_edge_loss             -> vertex_ring                        (mean |v0 - v1|^2 over unique edges)
//   mesh_laplacian_smoothing   -> vertex_ring / laplacian_adjoint    (uniform weights: | mean of ring - v |)
//   mesh_normal_consistency    -> face_pair_eval                     (1 - cos of the normals either side of an edge,
//                                                                     cos = <n0,n1> rsqrt(max(|n0|^2 |n1|^2, 1e-16)))
#pragma once
#include <math.h>
#include <stdint.h>

#include "smalfit_math.h"

namespace smalfit {

constexpr float kCosEps2 = 1e-16f;   // torch cosine_similarity: eps = 1e-8, clamp on the product of squared norms

// ------------------------------------------------------------------------------------------------
// counter-based random numbers: Philox-4x32-10 (Salmon et al. 2011), one call per sample
// ------------------------------------------------------------------------------------------------
struct Philox4 {
  uint32_t v[4];
};

SMALFIT_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// uniform in [0, 1) with 24 random bits
SMALFIT_HD float unit_float(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

// first face whose cumulative-area threshold exceeds r (thresholds: cumulative area / total * 2^32, non-decreasing);
// a zero-area face has the threshold of its predecessor and is never returned
SMALFIT_HD int sample_face(const uint32_t* thr, int F, uint32_t r) {
  int lo = 0, hi = F - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the barycentric map of pytorch3d's _rand_barycentric_coords.  The multiply-adds are explicit fmaf, in the order the device
// compiler contracted `w0 a + w1 b + w2 c` to (the kernel's instructions are unchanged): written as plain products and sums the
// host, which does not contract, was a last bit away from the device on a fifth of the coordinates -- now a point drawn on the
// host is the device's point to the bit (tests/test_gpu_template_mesh.py)
SMALFIT_HD void barycentric_sample(const float* a, const float* b, const float* c, float u, float v, float out[3]) {
  const float su = sqrtf(u);
  const float w0 = 1.0f - su, w1 = su * (1.0f - v), w2 = su * v;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = fmaf(w2, c[k], fmaf(w0, a[k], w1 * b[k]));
}

// ------------------------------------------------------------------------------------------------
// chamfer: nearest neighbour scan over the staged points p[begin .. end) (16-byte records: one LDS read per point);
// strict '<' over ascending indices keeps the lowest index among equal distances.  With OWNER the record also carries
// the index of the vertex that point chose in the other direction, and the scan accumulates sum (q - p_j) over the j
// with owner == self: the reverse-direction gradient gathered at the vertex instead of scattered from the points.
// ------------------------------------------------------------------------------------------------
struct alignas(16) ScanPoint {
  float x, y, z;
  int owner;
};

// WEIGHTED (the robust kernel below): wt[j] is the weight w_s of staged point j, and the gather becomes sum w_s (q - p_j): the
// mask carries the weight in place of 1, so the loop stays branch-free and no divide enters it
template <bool OWNER, bool WEIGHTED = false>
SMALFIT_HD void nearest_scan(float qx, float qy, float qz, const ScanPoint* p, int begin, int end, int index_base,
                             float& best, int& best_idx, int self, float g[3], const float* wt = nullptr) {
#pragma unroll 4
  for (int j = begin; j < end; ++j) {
    const ScanPoint s = p[j];
    const float dx = qx - s.x, dy = qy - s.y, dz = qz - s.z;
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    if (d2 < best) {
      best = d2;
      best_idx = index_base + j;
    }
    if (OWNER) {
      float mk = s.owner == self ? 1.0f : 0.0f;   // branch-free: g + 1 * d and g + 0 * d are exact
      if (WEIGHTED) mk = s.owner == self ? wt[j] : 0.0f;
      g[0] = fmaf(mk, dx, g[0]);
      g[1] = fmaf(mk, dy, g[1]);
      g[2] = fmaf(mk, dz, g[2]);
    }
  }
}

// the share [b, e) of wave w of 4 in a staged chunk of cnt records: quarters rounded up, the last ones short or empty.  The one
// definition for every kernel that splits a chunk over its four waves, and for the host shims that walk the same split
struct Span { int b, e; };
SMALFIT_HD Span quarter_span(int w, int cnt) {
  const int per = (cnt + 3) >> 2;
  const int b = w * per < cnt ? w * per : cnt;
  return Span{b, b + per < cnt ? b + per : cnt};
}

// lexicographic (distance, index) minimum: combines the scans of disjoint index ranges in any order
SMALFIT_HD void nearest_merge(float& best, int& best_idx, float d2, int idx) {
  if (d2 < best || (d2 == best && idx < best_idx)) {
    best = d2;
    best_idx = idx;
  }
}

// ---- the gated chamfer scan (smalfit_chamfer_gate_args; worded in include/smalfit.h) --------------------------------------
// The staged record of nearest_scan with the scanned element's unit normal behind it: two 16-byte rows, each one broadcast LDS
// read.  `tag` = 2 * (index in the scanned set) + (its boundary byte != 0): ascending with the index, so the lowest-index tie
// rule holds on tags as it does on indices, and the winner brings its boundary bit along without a register of its own.
struct alignas(16) GatedScanPoint {
  float x, y, z;
  int owner;
  float nx, ny, nz;
  int tag;
};
SMALFIT_HD float dot3(float ax, float ay, float az, float bx, float by, float bz);   // (defined with the triangle records below)
typedef float GatedRow __attribute__((vector_size(16), may_alias));   // one 16-byte row of the record, read whole
SMALFIT_HD int float_bits(float f) {
  int i;
  __builtin_memcpy(&i, &f, sizeof(i));
  return i;
}
constexpr int kNoTag = 0x7fffffff;  // no candidate yet (nearest_scan's "no index"); an index stays below 2^30
SMALFIT_HD int gated_tag(int index, int boundary) { return 2 * index + (boundary != 0 ? 1 : 0); }

// the two unit normals are compatible with threshold c when <a, b> >= c: float32, branch-free; a zero normal gives 0 on the
// left, a NaN compares false.  c = -inf with both normals zero (never read) is the test switched off
SMALFIT_HD bool unit_normals_compatible(float ax, float ay, float az, float bx, float by, float bz, float c) {
  return dot3(ax, ay, az, bx, by, bz) >= c;
}

// nearest_scan over the records compatible with the query's normal (ux, uy, uz): the same d^2 expression, the same strict '<',
// the same lowest-index tie rule; best_tag is the winner's tag.  The owner gather keeps its mask over ALL staged records,
// compatible or not: those matches were vetted in the other direction
template <bool OWNER, bool WEIGHTED = false>
SMALFIT_HD void nearest_scan_gated(float qx, float qy, float qz, float ux, float uy, float uz, float c, const GatedScanPoint* p,
                                   int begin, int end, float& best, int& best_tag, int self, float g[3], const float* wt = nullptr) {
#pragma unroll 4
  for (int j = begin; j < end; ++j) {
    // each row as ONE 16-byte read, the tag with the normal it shares a row with: read field by field, the tag's load is sunk
    // into the branch that takes it, the loop falls into a block per record and no read overlaps the arithmetic before it
    const GatedRow r0 = *reinterpret_cast<const GatedRow*>(&p[j].x), r1 = *reinterpret_cast<const GatedRow*>(&p[j].nx);
    const float dx = qx - r0[0], dy = qy - r0[1], dz = qz - r0[2];
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const bool ok = unit_normals_compatible(ux, uy, uz, r1[0], r1[1], r1[2], c);
    const bool take = ok & (d2 < best);
    best = take ? d2 : best;
    best_tag = take ? float_bits(r1[3]) : best_tag;
    if (OWNER) {
      float mk = float_bits(r0[3]) == self ? 1.0f : 0.0f;
      if (WEIGHTED) mk = float_bits(r0[3]) == self ? wt[j] : 0.0f;   // (as in nearest_scan)
      g[0] = fmaf(mk, dx, g[0]);
      g[1] = fmaf(mk, dy, g[1]);
      g[2] = fmaf(mk, dz, g[2]);
    }
  }
}

// what is decided once per query after the waves' minima have met: found (a compatible candidate exists), truncation
// (d^2 > tau^2 drops; tau2 = +inf: off) and, boundary != 0, the boundary rule on the WINNER's bit
struct GatedMatch {
  int index;   // of the winner, -1 when none was found
  bool kept;
};
SMALFIT_HD GatedMatch gated_match(float best, int best_tag, float tau2, int reject_boundary) {
  GatedMatch m;
  const bool found = best_tag != kNoTag;
  m.index = found ? best_tag >> 1 : -1;
  m.kept = found & !(best > tau2) & !((reject_boundary != 0) & ((best_tag & 1) != 0));
  return m;
}

// ---- the robust kernel of both data terms (smalfit_robust_args; worded in include/smalfit.h) -----------------------------
// Geman-McClure on a kept match's float32 d^2 with s2 = sigma * sigma (formed once on the host, in float32):
//   u = s2 / (s2 + d2)     one float32 add, one correctly rounded float32 divide
//   rho = d2 * u           what the sums take in place of d^2 (-> s2 far away)
//   w = u * u              = d rho / d (d^2): what the match's gradient is multiplied by
// d2 = 0 gives u = 1, rho = 0, w = 1.  The one definition: every kernel that applies the kernel and the host shim call this
SMALFIT_HD void robust_gm(float d2, float s2, float& rho, float& w) {
  const float u = s2 / (s2 + d2);
  rho = d2 * u;
  w = u * u;
}

// ---- mesh3d_chamfer_kernel<ROLE, GATED, ROBUST> in pieces: how it scans either record type, what it decides per query -------
// the scan of either record type over p[begin .. end), staged from element index_base on (u, c: read by the gated scan alone)
template <bool OWNER, bool WEIGHTED>
SMALFIT_HD void scan_records(float qx, float qy, float qz, float, float, float, float, const ScanPoint* p, int begin, int end,
                             int index_base, float& best, int& best_idx, int self, float g[3], const float* wt) {
  nearest_scan<OWNER, WEIGHTED>(qx, qy, qz, p, begin, end, index_base, best, best_idx, self, g, wt);
}
template <bool OWNER, bool WEIGHTED>
SMALFIT_HD void scan_records(float qx, float qy, float qz, float ux, float uy, float uz, float c, const GatedScanPoint* p, int begin,
                             int end, int, float& best, int& best_tag, int self, float g[3], const float* wt) {
  nearest_scan_gated<OWNER, WEIGHTED>(qx, qy, qz, ux, uy, uz, c, p, begin, end, best, best_tag, self, g, wt);
}

// what is decided once per query after the waves' minima have met.  Ungated: the match is the nearest element and every active
// query is kept.  GATED: gated_match on the winner's tag.  ROBUST: robust_gm on the match's d^2 under s2 (s2 = 0: this direction's
// scale is off, w = 1 and rho = d^2).  Without ROBUST rho = d^2 and w = 1; a dropped query's w is 0.  The sums take rho of the kept
struct ChamferMatch { int index; bool kept; float rho, w; };   // index: of the matched element (GATED: -1 when none was found)
template <bool GATED, bool ROBUST>
SMALFIT_HD ChamferMatch chamfer_match(float best, int bidx, float tau2, int reject_boundary, float s2, bool active) {
  ChamferMatch m;
  m.index = bidx;
  m.kept = active;
  if constexpr (GATED) {
    const GatedMatch mt = gated_match(best, bidx, tau2, reject_boundary);
    m.index = mt.index;
    m.kept = active && mt.kept;
  }
  float rho = best, w = 1.0f;
  if constexpr (ROBUST) {
    if (s2 > 0.f) robust_gm(best, s2, rho, w);
  }
  m.rho = rho;
  m.w = m.kept ? w : 0.f;
  return m;
}

// d/dy of a vertex's chamfer terms: cy (y - x_match) for its own match + cx sum (y - x_s) over the points that chose it (g, as the
// scans gathered it).  A vertex that is not kept, or whose match is no element (no finite distance: NaN input), reads x_0: in bounds
SMALFIT_HD void chamfer_vertex_grad(float cy, float cx, const float y[3], const float* x, int count, bool kept, int index,
                                    const float g[3], float out[3]) {
  const float* xn = x + 3 * (size_t)(kept && (unsigned)index < (unsigned)count ? index : 0);   // (one compare: a negative index is a large unsigned one)
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = cy * (y[k] - xn[k]) + cx * g[k];
}

// ------------------------------------------------------------------------------------------------
// point to triangle (smalfit_mesh_score; no counterpart in the reference: the definition is worded in include/smalfit.h).
// The squared distance from p to the closed triangle (a, b, c) is the minimum of
//   the three point-to-segment distances, the parameter clamped to [0, 1] (a zero-length segment is its end point), and
//   the distance to the plane, when the normal n = (b - a) x (c - a) is not zero and p projects inside: the three edge
//   functions <(b - a) x (p - a), n>, <(c - b) x (p - b), n>, <(a - c) x (p - c), n> are all >= 0.
// A degenerate triangle is exactly its three segments: no special case, nothing is divided by a value that can be zero.
// NOT the region walk (Ericson's closest point on a triangle): its cross terms cancel on slivers, and in float32 it was
// measured 3e4 ulp of the largest coordinate off where this form stays within 23 (tests/test_mesh_score_cpu.py).
// The staged record: four 16-byte rows, each one broadcast LDS read in the scan of mesh3d_surface_dist_kernel.
// ------------------------------------------------------------------------------------------------
struct alignas(16) ScanTri {
  float ax, ay, az, inv_ab;   // corner a | 1 / |b - a|^2
  float bx, by, bz, inv_bc;   // corner b | 1 / |c - b|^2
  float cx, cy, cz, inv_ca;   // corner c | 1 / |a - c|^2
  float nx, ny, nz, inv_nn;   // (b - a) x (c - a) | 1 / |n|^2      (every reciprocal: 0 where the squared length is 0)
};

SMALFIT_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }
SMALFIT_HD float recip_or_zero(float x) { return x > 0.f ? 1.0f / x : 0.f; }

// the record normal n = (b - a) x (c - a), unnormalised: the one expression behind ScanTri's n and the query normals of the
// gated surface term (face_unit_normal, vertex_normal below)
SMALFIT_HD void scan_tri_normal(const float* a, const float* b, const float* c, float n[3]) {
  const float e0[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  n[0] = e0[1] * ac[2] - e0[2] * ac[1];
  n[1] = e0[2] * ac[0] - e0[0] * ac[2];
  n[2] = e0[0] * ac[1] - e0[1] * ac[0];
}

SMALFIT_HD ScanTri make_scan_tri(const float* a, const float* b, const float* c) {
  ScanTri t;
  t.ax = a[0]; t.ay = a[1]; t.az = a[2];
  t.bx = b[0]; t.by = b[1]; t.bz = b[2];
  t.cx = c[0]; t.cy = c[1]; t.cz = c[2];
  const float e0[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float e1[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
  const float e2[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
  float n[3];
  scan_tri_normal(a, b, c, n);
  t.nx = n[0]; t.ny = n[1]; t.nz = n[2];
  t.inv_ab = recip_or_zero(dot3(e0[0], e0[1], e0[2], e0[0], e0[1], e0[2]));
  t.inv_bc = recip_or_zero(dot3(e1[0], e1[1], e1[2], e1[0], e1[1], e1[2]));
  t.inv_ca = recip_or_zero(dot3(e2[0], e2[1], e2[2], e2[0], e2[1], e2[2]));
  t.inv_nn = recip_or_zero(dot3(n[0], n[1], n[2], n[0], n[1], n[2]));
  return t;
}

// d = p - (start of the segment), e = end - start, inv = 1 / |e|^2 or 0.  fmaxf / fminf: a NaN parameter (0 x inf, the
// reciprocal of a subnormal squared length) counts as 0, the start point
SMALFIT_HD float point_segment_dist2(float dx, float dy, float dz, float ex, float ey, float ez, float inv) {
  const float t = fminf(fmaxf(dot3(dx, dy, dz, ex, ey, ez) * inv, 0.f), 1.0f);
  const float rx = fmaf(-t, ex, dx), ry = fmaf(-t, ey, dy), rz = fmaf(-t, ez, dz);
  return dot3(rx, ry, rz, rx, ry, rz);
}

// <e x d, n>: the edge function of the edge e, d = p - (start of the edge)
SMALFIT_HD float edge_function(float ex, float ey, float ez, float dx, float dy, float dz, float nx, float ny, float nz) {
  const float cx = ey * dz - ez * dy, cy = ez * dx - ex * dz, cz = ex * dy - ey * dx;
  return dot3(cx, cy, cz, nx, ny, nz);
}

SMALFIT_HD float point_scan_tri_dist2(float px, float py, float pz, const ScanTri& t) {
  const float pax = px - t.ax, pay = py - t.ay, paz = pz - t.az;
  const float pbx = px - t.bx, pby = py - t.by, pbz = pz - t.bz;
  const float pcx = px - t.cx, pcy = py - t.cy, pcz = pz - t.cz;
  const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
  const float bcx = t.cx - t.bx, bcy = t.cy - t.by, bcz = t.cz - t.bz;
  const float cax = t.ax - t.cx, cay = t.ay - t.cy, caz = t.az - t.cz;
  float d2 = point_segment_dist2(pax, pay, paz, abx, aby, abz, t.inv_ab);
  d2 = fminf(d2, point_segment_dist2(pbx, pby, pbz, bcx, bcy, bcz, t.inv_bc));
  d2 = fminf(d2, point_segment_dist2(pcx, pcy, pcz, cax, cay, caz, t.inv_ca));
  // (all three evaluated, then combined: no divergent branch inside the scan loop)
  const float s0 = edge_function(abx, aby, abz, pax, pay, paz, t.nx, t.ny, t.nz);
  const float s1 = edge_function(bcx, bcy, bcz, pbx, pby, pbz, t.nx, t.ny, t.nz);
  const float s2 = edge_function(cax, cay, caz, pcx, pcy, pcz, t.nx, t.ny, t.nz);
  const bool inside = (t.inv_nn > 0.f) & (s0 >= 0.f) & (s1 >= 0.f) & (s2 >= 0.f);
  const float h = dot3(pax, pay, paz, t.nx, t.ny, t.nz);
  // (fminf: a NaN plane distance -- 0 x inf under a subnormal |n|^2 -- leaves the segments' value)
  return inside ? fminf(h * h * t.inv_nn, d2) : d2;
}

SMALFIT_HD float point_triangle_dist2(const float* p, const float* a, const float* b, const float* c) {
  return point_scan_tri_dist2(p[0], p[1], p[2], make_scan_tri(a, b, c));
}

// nearest of the staged triangles t[begin .. end): a minimum over float32 values does not depend on the scan's order
SMALFIT_HD float surface_scan(float px, float py, float pz, const ScanTri* t, int begin, int end, float best) {
#pragma unroll 2
  for (int j = begin; j < end; ++j) best = fminf(best, point_scan_tri_dist2(px, py, pz, t[j]));
  return best;
}

// The same distance with WHERE on the triangle it is reached (the surface term of smalfit_mesh_surface_eval /
// smalfit_fit3d_step_surface; worded in include/smalfit.h).  d2 is formed by the expressions of point_scan_tri_dist2 in their
// order, so the two agree bit for bit; the winner is the first of (ab, bc, ca, plane) to reach that minimum.  Its barycentrics
// over (a, b, c): a segment's clamped parameter t gives (1 - t, t, 0) on that edge; the plane gives (s1, s2, s0) over their own
// sum (= |n|^2 up to rounding: divided by the sum, the weights add up to 1 on a sliver too).  The residual r = p - q comes from
// the winner's own intermediates, d - t e or (h / |n|^2) n: no closest point is subtracted from p.
struct TriHit {
  float d2;
  float b[3];   // weights of the corners a, b, c
  float r[3];   // p - (closest point)
};

// ... and WHICH candidate won (0 ab, 1 bc, 2 ca, 3 plane) with its clamped parameter (0 for the plane): what the boundary rule
// of the gated term asks.  point_scan_tri_closest is this function without the two: its outputs keep their bits
struct TriHitWhere {
  TriHit h;
  int winner;
  float t;
};

SMALFIT_HD TriHitWhere point_scan_tri_closest_where(float px, float py, float pz, const ScanTri& t) {
  const float pax = px - t.ax, pay = py - t.ay, paz = pz - t.az;
  const float pbx = px - t.bx, pby = py - t.by, pbz = pz - t.bz;
  const float pcx = px - t.cx, pcy = py - t.cy, pcz = pz - t.cz;
  const float abx = t.bx - t.ax, aby = t.by - t.ay, abz = t.bz - t.az;
  const float bcx = t.cx - t.bx, bcy = t.cy - t.by, bcz = t.cz - t.bz;
  const float cax = t.ax - t.cx, cay = t.ay - t.cy, caz = t.az - t.cz;
  // the three segments: parameter, residual d - t e, its squared length (the expressions of point_segment_dist2)
  const float t0 = fminf(fmaxf(dot3(pax, pay, paz, abx, aby, abz) * t.inv_ab, 0.f), 1.0f);
  const float r0x = fmaf(-t0, abx, pax), r0y = fmaf(-t0, aby, pay), r0z = fmaf(-t0, abz, paz);
  const float d0 = dot3(r0x, r0y, r0z, r0x, r0y, r0z);
  const float t1 = fminf(fmaxf(dot3(pbx, pby, pbz, bcx, bcy, bcz) * t.inv_bc, 0.f), 1.0f);
  const float r1x = fmaf(-t1, bcx, pbx), r1y = fmaf(-t1, bcy, pby), r1z = fmaf(-t1, bcz, pbz);
  const float d1 = dot3(r1x, r1y, r1z, r1x, r1y, r1z);
  const float t2 = fminf(fmaxf(dot3(pcx, pcy, pcz, cax, cay, caz) * t.inv_ca, 0.f), 1.0f);
  const float r2x = fmaf(-t2, cax, pcx), r2y = fmaf(-t2, cay, pcy), r2z = fmaf(-t2, caz, pcz);
  const float d2c = dot3(r2x, r2y, r2z, r2x, r2y, r2z);
  const float dseg = fminf(fminf(d0, d1), d2c);
  const float s0 = edge_function(abx, aby, abz, pax, pay, paz, t.nx, t.ny, t.nz);
  const float s1 = edge_function(bcx, bcy, bcz, pbx, pby, pbz, t.nx, t.ny, t.nz);
  const float s2 = edge_function(cax, cay, caz, pcx, pcy, pcz, t.nx, t.ny, t.nz);
  const bool inside = (t.inv_nn > 0.f) & (s0 >= 0.f) & (s1 >= 0.f) & (s2 >= 0.f);
  const float h = dot3(pax, pay, paz, t.nx, t.ny, t.nz);
  const float dp = h * h * t.inv_nn;
  // the winner: the first of (ab, bc, ca, plane) to reach the minimum (selects, no branch)
  const bool k1 = d1 < d0;
  const float sel1 = k1 ? d1 : d0;
  const bool k2 = d2c < sel1;
  const float sel2 = k2 ? d2c : sel1;
  const float ssum = s0 + s1 + s2;
  const bool kp = inside & (dp < sel2) & (ssum > 0.f);
  const float is = kp ? 1.0f / ssum : 0.f, k = h * t.inv_nn;
  TriHitWhere ow;
  ow.winner = kp ? 3 : (k2 ? 2 : (k1 ? 1 : 0));
  ow.t = kp ? 0.f : (k2 ? t2 : (k1 ? t1 : t0));
  TriHit& o = ow.h;
  o.d2 = inside ? fminf(dp, dseg) : dseg;
  o.b[0] = kp ? s1 * is : (k2 ? t2 : (k1 ? 0.f : 1.0f - t0));
  o.b[1] = kp ? s2 * is : (k2 ? 0.f : (k1 ? 1.0f - t1 : t0));
  o.b[2] = kp ? s0 * is : (k2 ? 1.0f - t2 : (k1 ? t1 : 0.f));
  o.r[0] = kp ? k * t.nx : (k2 ? r2x : (k1 ? r1x : r0x));
  o.r[1] = kp ? k * t.ny : (k2 ? r2y : (k1 ? r1y : r0y));
  o.r[2] = kp ? k * t.nz : (k2 ? r2z : (k1 ? r1z : r0z));
  return ow;
}

SMALFIT_HD TriHit point_scan_tri_closest(float px, float py, float pz, const ScanTri& t) {
  return point_scan_tri_closest_where(px, py, pz, t).h;
}

SMALFIT_HD TriHit point_triangle_closest(const float* p, const float* a, const float* b, const float* c) {
  return point_scan_tri_closest(p[0], p[1], p[2], make_scan_tri(a, b, c));
}

// nearest of the staged triangles t[begin .. end) WITH its index: strict '<' over ascending indices keeps the lowest index among
// equal distances; disjoint ranges combine through nearest_merge or an integer minimum of (distance bits, index) keys
SMALFIT_HD void surface_scan_nearest(float px, float py, float pz, const ScanTri* t, int begin, int end, int index_base,
                                     float& best, int& best_idx) {
#pragma unroll 2
  for (int j = begin; j < end; ++j) {
    const float d2 = point_scan_tri_dist2(px, py, pz, t[j]);
    if (d2 < best) {
      best = d2;
      best_idx = index_base + j;
    }
  }
}

// ---- the gates of the surface term (smalfit_surface_gate_args; worded in include/smalfit.h) ---------------------------------
// Compatibility of a query's unit normal u with a record's unnormalised normal n: the signed squared cosine
// g |g| / |n|^2, g = <u, n>, against c |c| -- monotone in the cosine, one branch-free expression, no square root in the scan.
// A degenerate record (inv_nn = 0) or a zero u gives 0: compatible exactly when c <= 0.  A NaN compares false: incompatible
SMALFIT_HD float signed_sq_cos(float ux, float uy, float uz, float nx, float ny, float nz, float inv_nn) {
  const float g = dot3(ux, uy, uz, nx, ny, nz);
  return g * fabsf(g) * inv_nn;
}
SMALFIT_HD float cos_threshold(float c) { return c * fabsf(c); }
SMALFIT_HD bool normal_compatible(float ux, float uy, float uz, float nx, float ny, float nz, float inv_nn, float cc) {
  return signed_sq_cos(ux, uy, uz, nx, ny, nz, inv_nn) >= cc;
}

// surface_scan_nearest over the compatible records only (cc = cos_threshold(c)): the same strict '<', the same key
SMALFIT_HD void surface_scan_nearest_compatible(float px, float py, float pz, float ux, float uy, float uz, float cc, const ScanTri* t,
                                                int begin, int end, int index_base, float& best, int& best_idx) {
#pragma unroll 2
  for (int j = begin; j < end; ++j) {
    const float d2 = point_scan_tri_dist2(px, py, pz, t[j]);
    const bool ok = normal_compatible(ux, uy, uz, t[j].nx, t[j].ny, t[j].nz, t[j].inv_nn, cc);
    if (ok & (d2 < best)) {
      best = d2;
      best_idx = index_base + j;
    }
  }
}

// Boundary rule.  flags of the winning face (mesh3d_topology.h::boundary_flags): bits 0-2 the edges ab, bc, ca used by no other
// face, bits 3-5 the corners a, b, c that end such an edge.  A match is on the boundary when its winning candidate is a segment
// and that segment is a boundary edge, or its clamped parameter is exactly 0 / exactly 1 and the segment's start / end corner is
// a boundary vertex (segment k runs from corner k to corner (k + 1) % 3)
SMALFIT_HD bool boundary_match(unsigned flags, int winner, float t) {
  if (winner > 2) return false;
  const int start = winner, end = winner == 2 ? 0 : winner + 1;
  const bool edge = (flags >> winner) & 1u;
  const bool at_start = (t == 0.f) & (((flags >> (3 + start)) & 1u) != 0u);
  const bool at_end = (t == 1.0f) & (((flags >> (3 + end)) & 1u) != 0u);
  return edge | at_start | at_end;
}

// v / |v|, the zero vector for a zero (or NaN) length
SMALFIT_HD void unit_or_zero(const float v[3], float out[3]) {
  const float len = sqrtf(dot3(v[0], v[1], v[2], v[0], v[1], v[2]));
  const float inv = len > 0.f ? 1.0f / len : 0.f;
  out[0] = v[0] * inv;
  out[1] = v[1] * inv;
  out[2] = v[2] * inv;
}
// the unit normal of a face: its record normal over its length (a target point carries the one of the face it was sampled on)
SMALFIT_HD void face_unit_normal(const float* a, const float* b, const float* c, float out[3]) {
  float n[3];
  scan_tri_normal(a, b, c, n);
  unit_or_zero(n, out);
}
// the normal of fitted vertex v: the sum of the record normals of its incident faces (CSR of mesh3d_topology.h, ascending face
// index) over its length
SMALFIT_HD void vertex_normal(const float* verts, const int* faces, const int* vf_off, const int* vf, int v, float out[3]) {
  float s[3] = {0.f, 0.f, 0.f};
  for (int i = vf_off[v]; i < vf_off[v + 1]; ++i) {
    const int* fc = faces + 3 * (size_t)vf[i];
    float n[3];
    scan_tri_normal(verts + 3 * (size_t)fc[0], verts + 3 * (size_t)fc[1], verts + 3 * (size_t)fc[2], n);
    s[0] += n[0];
    s[1] += n[1];
    s[2] += n[2];
  }
  unit_or_zero(s, out);
}

// what a point -> surface query leaves for the vertices of the face it chose (48 bytes: three 16-byte rows, broadcast LDS reads
// in mesh3d_surface_grad_kernel): every corner i receives -b_i r
struct alignas(16) SurfaceHit {
  int c0, c1, c2;      // vertex ids of the winning face's corners
  float b0;
  float b1, b2, rx, ry;
  float rz, pad0, pad1, pad2;
};

// the share of vertex `self` in sum_j -b_i(j) r(j) over the staged hits h[begin .. end), in index order.  A face has three
// distinct corners, so at most one of the three weights is taken: the selection is exact
SMALFIT_HD void surface_hit_gather(const SurfaceHit* h, int begin, int end, int self, float g[3]) {
#pragma unroll 4
  for (int j = begin; j < end; ++j) {
    const SurfaceHit s = h[j];
    const float w = (s.c0 == self ? s.b0 : 0.f) + (s.c1 == self ? s.b1 : 0.f) + (s.c2 == self ? s.b2 : 0.f);
    g[0] = fmaf(w, s.rx, g[0]);
    g[1] = fmaf(w, s.ry, g[1]);
    g[2] = fmaf(w, s.rz, g[2]);
  }
}

// ------------------------------------------------------------------------------------------------
// one-ring of a vertex (neighbours through unique edges, ascending): everything the edge and Laplacian terms need
// ------------------------------------------------------------------------------------------------
struct RingEval {
  float edge_sum;      // sum over the ring of |v - u|^2 (every edge is seen from both ends: halve the total)
  float edge_grad[3];  // sum over the ring of (v - u):  d/dv of sum over incident edges |v - u|^2 = 2 * this
  float lap_norm;      // | mean(ring) - v |
  float lap_unit[3];   // (mean(ring) - v) / lap_norm, 0 when the norm is 0 (torch's subgradient of norm at 0)
};

SMALFIT_HD void vertex_ring(const float* verts /* [V][3] of one mesh */, int v, const int* nbr, int deg, RingEval& r) {
  const float x = verts[3 * v], y = verts[3 * v + 1], z = verts[3 * v + 2];
  float es = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  for (int k = 0; k < deg; ++k) {
    const int u = nbr[k];
    const float ux = verts[3 * u], uy = verts[3 * u + 1], uz = verts[3 * u + 2];
    const float dx = x - ux, dy = y - uy, dz = z - uz;
    es += fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    gx += dx; gy += dy; gz += dz;
  }
  r.edge_sum = es;
  r.edge_grad[0] = gx; r.edge_grad[1] = gy; r.edge_grad[2] = gz;
  // mean(ring) - v = -(sum over the ring of (v - u)) / deg: from the differences the edge term already sums, never from a sum
  // of absolute coordinates -- that form lost the digits of |v| / |mean(ring) - v| on a mesh that stands far from the origin
  float lx = 0.f, ly = 0.f, lz = 0.f;
  if (deg > 0) {
    const float inv = 1.0f / (float)deg;
    lx = -(gx * inv); ly = -(gy * inv); lz = -(gz * inv);
  }
  const float n2 = fmaf(lz, lz, fmaf(ly, ly, lx * lx));
  const float n = sqrtf(n2);
  const float in = n > 0.f ? 1.0f / n : 0.f;
  r.lap_norm = n;
  r.lap_unit[0] = lx * in; r.lap_unit[1] = ly * in; r.lap_unit[2] = lz * in;
}

// d(sum_i |L v|_i) / d v_j = -unit_j [deg_j > 0] + sum over the ring i of unit_i / deg_i   (L = D^-1 A - I, symmetric pattern)
SMALFIT_HD void laplacian_adjoint(const float* unit /* [V][3] */, int v, const int* nbr, int deg, const int* nbr_off,
                                  float g[3]) {
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (deg > 0) {
    gx = -unit[3 * v]; gy = -unit[3 * v + 1]; gz = -unit[3 * v + 2];
  }
  for (int k = 0; k < deg; ++k) {
    const int i = nbr[k];
    const float inv = 1.0f / (float)(nbr_off[i + 1] - nbr_off[i]);
    gx = fmaf(unit[3 * i], inv, gx);
    gy = fmaf(unit[3 * i + 1], inv, gy);
    gz = fmaf(unit[3 * i + 2], inv, gz);
  }
  g[0] = gx; g[1] = gy; g[2] = gz;
}

// ------------------------------------------------------------------------------------------------
// normal consistency of the two faces (v0, v1, a) and (v0, v1, b) sharing the edge (v0, v1)
// returns 1 - cos; grad[r][k] = d(1 - cos) / d(vertex r), r = 0..3 for v0, v1, a, b
// ------------------------------------------------------------------------------------------------
SMALFIT_HD void cross3(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// a x b with every product rounded on its own, never contracted to fma(a1, b2, -(a2 b1)): a x a is then the zero vector
// exactly.  A face collapsed onto its edge (a == p1) has n0 = e x e; contracted, that is the rounding error of a product, ~6e-8 |e|^2,
// and under the clamp r = 1e8 multiplies it back to |e|^2 |n1|: a cosine of order 1 on a mesh of extent 16 where torch gives 0
SMALFIT_HD void cross3_rounded(const float a[3], const float b[3], float o[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p0 = a[1] * b[2], q0 = a[2] * b[1], p1 = a[2] * b[0], q1 = a[0] * b[2], p2 = a[0] * b[1], q2 = a[1] * b[0];
  o[0] = p0 - q0;
  o[1] = p1 - q1;
  o[2] = p2 - q2;
}

SMALFIT_HD float face_pair_eval(const float* p0, const float* p1, const float* pa, const float* pb, float grad[4][3]) {
  float e[3], ea[3], eb[3], n0[3], n1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[k] = p1[k] - p0[k];
    ea[k] = pa[k] - p0[k];
    eb[k] = pb[k] - p0[k];
  }
  cross3_rounded(e, ea, n0);
  cross3_rounded(eb, e, n1);             // -(e x eb)
  const float w12 = n0[0] * n1[0] + n0[1] * n1[1] + n0[2] * n1[2];
  const float w1 = n0[0] * n0[0] + n0[1] * n0[1] + n0[2] * n0[2];
  const float w2 = n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2];
  const float prod = w1 * w2;
  const bool clamped = !(prod > kCosEps2);
  const float r = 1.0f / sqrtf(clamped ? kCosEps2 : prod);
  const float cosv = w12 * r;
  // d cos / d n0 = r n1 - w12 r^3 w2 n0 ; d cos / d n1 = r n0 - w12 r^3 w1 n1 (second terms vanish under the clamp)
  const float r3 = clamped ? 0.f : r * r * r * w12;
  float G0[3], G1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    G0[k] = -(r * n1[k] - r3 * w2 * n0[k]);      // adjoint of n0 for the value 1 - cos
    G1[k] = -(r * n0[k] - r3 * w1 * n1[k]);
  }
  // n0 = e x ea : d/de = ea x G0, d/dea = G0 x e ;  n1 = eb x e : d/deb = e x G1, d/de = G1 x eb
  float de0[3], dea[3], deb[3], de1[3];
  cross3(ea, G0, de0);
  cross3(G0, e, dea);
  cross3(e, G1, deb);
  cross3(G1, eb, de1);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float de = de0[k] + de1[k];
    grad[1][k] = de;
    grad[2][k] = dea[k];
    grad[3][k] = deb[k];
    grad[0][k] = -(de + dea[k] + deb[k]);
  }
  return 1.0f - cosv;
}

}  // namespace smalfit

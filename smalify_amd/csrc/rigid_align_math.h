// The arithmetic of the rigid pre-alignment (smalfit_rigid_align; the definition is worded in include/smalfit.h), shared by
// kernels_rigid_align.inc and by the test-only host shim (tests/host_rigid_align_shim.cpp).  SMALFIT_HD as in smalfit_math.h.
// No counterpart in the reference.  Everything is float32; the chains the header words are explicit fmaf.
#pragma once
#include <math.h>

#include "smalfit_math.h"

namespace smalfit {

// what a block sums over its pairs, on coordinates centred at c_X (x) and c_P (p):
//   [0] 1   [1..3] x   [4..6] p   [7..15] x_a p_b (row a)   [16] |x|^2   [17] |p|^2   [18] d^2
constexpr int kRigidMoments = 19;
constexpr int kRigidSweeps = 8;           // cyclic Jacobi sweeps of the 4x4 solve, 6 rotations each
constexpr float kRigidRankEps = 1e-5f;    // the rank test: l1 - l2 > kRigidRankEps sqrt(sum w |x|^2) sqrt(sum w |p|^2)
constexpr int kRigidCubeRotations = 24;

// z = R x + t, T = three rows [R_i0 R_i1 R_i2 t_i]: one chain per coordinate
SMALFIT_HD void rigid_apply(const float T[12], float x, float y, float z, float out[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = fmaf(T[4 * i + 2], z, fmaf(T[4 * i + 1], y, fmaf(T[4 * i], x, T[4 * i + 3])));
}

// the start of rotation R (row-major 3x3): z = R (x - c_X) + c_P
SMALFIT_HD void rigid_start_transform(const float R[9], const float cX[3], const float cP[3], float T[12]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T[4 * i] = R[3 * i];
    T[4 * i + 1] = R[3 * i + 1];
    T[4 * i + 2] = R[3 * i + 2];
    T[4 * i + 3] = cP[i] - fmaf(R[3 * i + 2], cX[2], fmaf(R[3 * i + 1], cX[1], R[3 * i] * cX[0]));
  }
}

// the k-th of the 24 rotations of the cube, in the header's order: permutations of (0, 1, 2) in lexicographic order, within each
// the sign triples +++ ... --- counted as a 3-bit number (bit 2: s_0), keeping determinant +1.  k outside 0..23: the identity
SMALFIT_HD void rigid_cube_rotation(int k, float R[9]) {
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  const int parity[6] = {1, -1, -1, 1, 1, -1};
  for (int i = 0; i < 9; ++i) R[i] = 0.f;
  int seen = 0;
  for (int pi = 0; pi < 6; ++pi)
    for (int sg = 0; sg < 8; ++sg) {
      const int s0 = (sg & 4) ? -1 : 1, s1 = (sg & 2) ? -1 : 1, s2 = (sg & 1) ? -1 : 1;
      if (parity[pi] * s0 * s1 * s2 != 1) continue;
      if (seen++ == k) {
        R[perm[pi][0]] = (float)s0;
        R[3 + perm[pi][1]] = (float)s1;
        R[6 + perm[pi][2]] = (float)s2;
        return;
      }
    }
  R[0] = R[4] = R[8] = 1.0f;
}

// one pair's share of a block's sums: xc = x - c_X, pc = p - c_P, d2 the scan's own bits
SMALFIT_HD void rigid_pair_moments(const float xc[3], const float pc[3], float d2, float m[kRigidMoments]) {
  m[0] = 1.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m[1 + a] = xc[a];
    m[4 + a] = pc[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) m[7 + 3 * a + b] = xc[a] * pc[b];
  }
  m[16] = fmaf(xc[2], xc[2], fmaf(xc[1], xc[1], xc[0] * xc[0]));
  m[17] = fmaf(pc[2], pc[2], fmaf(pc[1], pc[1], pc[0] * pc[0]));
  m[18] = d2;
}

// the two directions' sums under their weights wv = w_vert / V, wp = w_point / S (a skipped direction: null, adds nothing)
SMALFIT_HD void rigid_combine(const float* mv, const float* mp, float wv, float wp, float M[kRigidMoments]) {
#pragma unroll
  for (int i = 0; i < kRigidMoments; ++i) {
    const float v = mv != nullptr ? wv * mv[i] : 0.f;
    M[i] = mp != nullptr ? fmaf(wp, mp[i], v) : v;
  }
}

// one Jacobi rotation of the symmetric A on the pivot (p, q), accumulated into the eigenvector columns of E
SMALFIT_HD void rigid_jacobi_rotate(float A[4][4], float E[4][4], int p, int q) {
  const float apq = A[p][q];
  if (!(apq != 0.f)) return;   // (zero, or NaN: nothing to do)
  const float theta = (A[q][q] - A[p][p]) / (2.0f * apq);
  const float t = (theta < 0.f ? -1.0f : 1.0f) / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.0f)));
  const float c = 1.0f / sqrtf(fmaf(t, t, 1.0f)), s = t * c;
  A[p][p] = fmaf(-t, apq, A[p][p]);
  A[q][q] = fmaf(t, apq, A[q][q]);
  A[p][q] = A[q][p] = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != p && r != q) {
      const float arp = A[r][p], arq = A[r][q];
      A[r][p] = A[p][r] = fmaf(c, arp, -(s * arq));
      A[r][q] = A[q][r] = fmaf(s, arp, c * arq);
    }
    const float erp = E[r][p], erq = E[r][q];
    E[r][p] = fmaf(c, erp, -(s * erq));
    E[r][q] = fmaf(s, erp, c * erq);
  }
}

// the rotation of the unit quaternion (w, x, y, z)
SMALFIT_HD void rigid_quat_rotation(const float q[4], float R[9]) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  R[0] = ww + xx - yy - zz;
  R[1] = 2.0f * (x * y - w * z);
  R[2] = 2.0f * (x * z + w * y);
  R[3] = 2.0f * (x * y + w * z);
  R[4] = ww - xx + yy - zz;
  R[5] = 2.0f * (y * z - w * x);
  R[6] = 2.0f * (x * z - w * y);
  R[7] = 2.0f * (y * z + w * x);
  R[8] = ww - xx - yy + zz;
}

// The weighted least-squares rigid fit of the combined sums M (Horn 1987): -> T = [R | t]; returns 1 when the rank test failed and
// the rotation of `prev` was kept (t is updated either way), 0 otherwise.  gap / scale (either may be null) receive l1 - l2 and
// sqrt(sum w |x|^2) sqrt(sum w |p|^2), the two sides of the test
SMALFIT_HD int rigid_solve(const float M[kRigidMoments], const float cX[3], const float cP[3], const float prev[12], float T[12],
                           float* gap = nullptr, float* scale = nullptr) {
  const float W = M[0];
  const float iw = W > 0.f ? 1.0f / W : 0.f;
  float mx[3], mp[3], H[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mx[a] = M[1 + a] * iw;
    mp[a] = M[4 + a] * iw;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) H[a][b] = fmaf(-M[1 + a], mp[b], M[7 + 3 * a + b]);
  float A[4][4], E[4][4];
  A[0][0] = H[0][0] + H[1][1] + H[2][2];
  A[1][1] = H[0][0] - H[1][1] - H[2][2];
  A[2][2] = -H[0][0] + H[1][1] - H[2][2];
  A[3][3] = -H[0][0] - H[1][1] + H[2][2];
  A[0][1] = A[1][0] = H[1][2] - H[2][1];
  A[0][2] = A[2][0] = H[2][0] - H[0][2];
  A[0][3] = A[3][0] = H[0][1] - H[1][0];
  A[1][2] = A[2][1] = H[0][1] + H[1][0];
  A[1][3] = A[3][1] = H[2][0] + H[0][2];
  A[2][3] = A[3][2] = H[1][2] + H[2][1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) E[i][j] = i == j ? 1.0f : 0.f;
  for (int sweep = 0; sweep < kRigidSweeps; ++sweep) {
    rigid_jacobi_rotate(A, E, 0, 1);
    rigid_jacobi_rotate(A, E, 0, 2);
    rigid_jacobi_rotate(A, E, 0, 3);
    rigid_jacobi_rotate(A, E, 1, 2);
    rigid_jacobi_rotate(A, E, 1, 3);
    rigid_jacobi_rotate(A, E, 2, 3);
  }
  // the largest diagonal entry, the lowest index among equal ones; l2: the largest of the other three
  int i1 = 0;
  float l1 = A[0][0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > l1) {
      l1 = A[i][i];
      i1 = i;
    }
  float l2 = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i != i1 && A[i][i] > l2) l2 = A[i][i];
  float q[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = i1 == 0 ? E[r][0] : i1 == 1 ? E[r][1] : i1 == 2 ? E[r][2] : E[r][3];
  const float n2 = fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0])));
  // (a root of each sum, not of their product: the product is of degree 4 in the lengths and would leave float32's range long
  // before any other intermediate of the solve, all of degree 2 at most, does)
  const float sc = sqrtf(M[16]) * sqrtf(M[17]);
  const float gp = l1 - l2;
  if (gap != nullptr) *gap = gp;
  if (scale != nullptr) *scale = sc;
  const bool determined = gp > kRigidRankEps * sc;   // (a NaN compares false)
  float R[9];
  if (determined) {
    const float in = 1.0f / sqrtf(n2);
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] *= in;
    rigid_quat_rotation(q, R);
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      R[3 * i] = prev[4 * i];
      R[3 * i + 1] = prev[4 * i + 1];
      R[3 * i + 2] = prev[4 * i + 2];
    }
  }
  const float bx[3] = {cX[0] + mx[0], cX[1] + mx[1], cX[2] + mx[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T[4 * i] = R[3 * i];
    T[4 * i + 1] = R[3 * i + 1];
    T[4 * i + 2] = R[3 * i + 2];
    T[4 * i + 3] = (cP[i] + mp[i]) - fmaf(R[3 * i + 2], bx[2], fmaf(R[3 * i + 1], bx[1], R[3 * i] * bx[0]));
  }
  return determined ? 0 : 1;
}

// ---- trimming (smalfit_trimmed_rigid_align) -------------------------------------------------------------------------------------
// the key of query q is (bits of its d^2, q): d^2 >= 0 is never -0, so its bits read as uint32 order as the value does
SMALFIT_HD unsigned rigid_key_bits(float d2) { return __builtin_bit_cast(unsigned, d2); }
SMALFIT_HD float rigid_key_value(unsigned bits) { return __builtin_bit_cast(float, bits); }
// key (bits, q) <= the threshold key (tbits, tq), lexicographically: the query is kept.  tq = -1 keeps nothing (no key was there)
SMALFIT_HD bool rigid_key_kept(unsigned bits, int q, unsigned tbits, int tq) { return bits < tbits || (bits == tbits && q <= tq); }
// how many of `count` queries the fraction in (0, 1] keeps: min(count, max(1, ceil(fraction count))), in double, on the host
inline int rigid_keep_count(double fraction, int count) {
  const double c = ceil(fraction * (double)count);
  return c >= (double)count ? count : c < 1.0 ? 1 : (int)c;
}

}  // namespace smalfit

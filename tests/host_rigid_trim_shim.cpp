// The host side of the trimmed rigid pre-alignment as C functions for tests/test_rigid_trim_cpu.py and
// tests/test_gpu_rigid_trim.py: the key order and the fraction -> count rule of rigid_align_math.h, the rules and grids of
// smalfit_plan.h, and one whole trimmed float32 iteration on the scans and sums of tests/host_rigid_align_shim.cpp (included as it
// is: its helpers are this shim's too).  The selection here is a plain sort of the keys, not the kernel's radix passes.  Built by
// g++ without contraction (tests/host_rigid_trim.py), no HIP.
#include "host_rigid_align_shim.cpp"

namespace {
// the `keep` lowest keys of the queries that have one (idx >= 0) -> kept bytes; thr: the highest kept key (bits, query), (0, -1)
// when nothing was kept
void select_keys(int count, const float* d2, const int* idx, int keep, unsigned char* kept, unsigned* thr_bits, int* thr_q) {
  std::vector<std::pair<unsigned, int>> keys;
  for (int q = 0; q < count; ++q)
    if (idx[q] >= 0) keys.push_back({rigid_key_bits(d2[q]), q});
  std::sort(keys.begin(), keys.end());
  const int m = std::min(keep, (int)keys.size());
  *thr_bits = m > 0 ? keys[m - 1].first : 0u;
  *thr_q = m > 0 ? keys[m - 1].second : -1;
  for (int q = 0; q < count; ++q) kept[q] = idx[q] >= 0 && rigid_key_kept(rigid_key_bits(d2[q]), q, *thr_bits, *thr_q) ? 1 : 0;
}

// direction_moments of the other shim over the kept pairs: a dropped query adds 0 in place of every sum, its d^2 too
void kept_moments(int dir, int V, const float* x, int S, const float* p, const int* idx, const float* d2, const unsigned char* kept,
                  const float* cX, const float* cP, float* m) {
  const int nq = dir == 0 ? V : S;
  for (int i = 0; i < kRigidMoments; ++i) m[i] = 0.f;
  for (int i = 0; i < nq; ++i) {
    if (!kept[i]) continue;
    const float* xs = x + 3 * (size_t)(dir == 0 ? i : idx[i]);
    const float* ps = p + 3 * (size_t)(dir == 0 ? idx[i] : i);
    const float xc[3] = {xs[0] - cX[0], xs[1] - cX[1], xs[2] - cX[2]}, pc[3] = {ps[0] - cP[0], ps[1] - cP[1], ps[2] - cP[2]};
    float one[kRigidMoments];
    rigid_pair_moments(xc, pc, d2[i], one);
    for (int k = 0; k < kRigidMoments; ++k) m[k] += one[k];
  }
}
}  // namespace

extern "C" {
int hrt_keep_count(double fraction, int count) { return rigid_keep_count(fraction, count); }
unsigned hrt_key_bits(float d2) { return rigid_key_bits(d2); }
int hrt_key_kept(unsigned bits, int q, unsigned tbits, int tq) { return rigid_key_kept(bits, q, tbits, tq) ? 1 : 0; }
// thr: bits and query of the threshold
void hrt_select(int count, const float* d2, const int* idx, int keep, unsigned char* kept, unsigned* thr) {
  int q;
  select_keys(count, d2, idx, keep, kept, thr, &q);
  thr[1] = (unsigned)q;
}
// one whole trimmed iteration in float32 from transform Tin (hra_iterate with the pair set restricted).  kept_v (V) / kept_p (S),
// idx_v / idx_p may be NULL; trim_d2: the threshold d^2 of the vertices, of the points (0 for a skipped direction).  Returns 1
// when the rotation was kept
int hrt_iterate(int V, const float* x, int S, const float* p, const float* Tin, float w_point, float w_vert, int keep_point, int keep_vert,
                float* Tout, float* cost, int* idx_v, int* idx_p, unsigned char* kept_v, unsigned char* kept_p, float* trim_d2) {
  float cX[3], cP[3];
  hra_means(V, x, cX);
  hra_means(S, p, cP);
  std::vector<int> iv(V), ip(S);
  std::vector<float> dv(V), dp(S);
  std::vector<unsigned char> kv(V), kp(S);
  float mv[kRigidMoments], mp[kRigidMoments], M[kRigidMoments];
  trim_d2[0] = trim_d2[1] = 0.f;
  unsigned bits;
  int q;
  if (w_vert > 0.f) {
    scan_direction(0, Tin, V, x, S, p, iv.data(), dv.data());
    select_keys(V, dv.data(), iv.data(), keep_vert, kv.data(), &bits, &q);
    trim_d2[0] = q >= 0 ? rigid_key_value(bits) : 0.f;
    kept_moments(0, V, x, S, p, iv.data(), dv.data(), kv.data(), cX, cP, mv);
    if (idx_v) std::copy(iv.begin(), iv.end(), idx_v);
    if (kept_v) std::copy(kv.begin(), kv.end(), kept_v);
  }
  if (w_point > 0.f) {
    scan_direction(1, Tin, V, x, S, p, ip.data(), dp.data());
    select_keys(S, dp.data(), ip.data(), keep_point, kp.data(), &bits, &q);
    trim_d2[1] = q >= 0 ? rigid_key_value(bits) : 0.f;
    kept_moments(1, V, x, S, p, ip.data(), dp.data(), kp.data(), cX, cP, mp);
    if (idx_p) std::copy(ip.begin(), ip.end(), idx_p);
    if (kept_p) std::copy(kp.begin(), kp.end(), kept_p);
  }
  rigid_combine(w_vert > 0.f ? mv : nullptr, w_point > 0.f ? mp : nullptr, w_vert / (float)V, w_point / (float)S, M);
  *cost = M[kRigidMoments - 1];
  return rigid_solve(M, cX, cP, Tin, Tout);
}
// nullptr = accepted
const char* hrt_refusal(const smalfit_rigid_trim_args* t, int V, int S, int vert_dir, int point_dir) {
  return rigid_trim_args_refusal(t, RigidTrimFacts{V, S, vert_dir != 0, point_dir != 0});
}
int hrt_on(const smalfit_rigid_trim_args* t, int V, int S, int vert_dir, int point_dir) {
  return rigid_trim_on(t, RigidTrimFacts{V, S, vert_dir != 0, point_dir != 0}) ? 1 : 0;
}
// out: the selection's grid (3), launches of a trimmed call, of an untrimmed one
void hrt_grids(int vert_dir, int point_dir, int K, int N, int iterations, int* out) {
  const Grid3 g = rigid_trim_grid(vert_dir != 0, point_dir != 0, K, N);
  out[0] = g.x; out[1] = g.y; out[2] = g.z;
  out[3] = rigid_trim_launches(iterations, vert_dir != 0, point_dir != 0);
  out[4] = rigid_align_launches(iterations, vert_dir != 0, point_dir != 0);
}
int hrt_sizeof_args() { return (int)sizeof(smalfit_rigid_trim_args); }
int hrt_offsets(int* out) {
#define OFF(f) offsetof(smalfit_rigid_trim_args, f)
  const size_t o[] = {OFF(struct_size), OFF(keep_vert), OFF(keep_point), OFF(vert_kept), OFF(point_kept), OFF(trim_d2)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}

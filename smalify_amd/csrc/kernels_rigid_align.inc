// Kernels of the rigid pre-alignment (smalfit_rigid_align; the definition is worded in include/smalfit.h, its arithmetic is
// rigid_align_math.h).  Included by smalfit_kernels.hip inside namespace smalfit.  No counterpart in the reference.
//   rigid_init_kernel      the means c_X, c_P of every mesh and the transform of every start
//   rigid_scan_kernel<DIR> one round of nearest-neighbour scans under the current transforms: DIR 0 the vertices ask (transformed
//                          in registers, the staged points do not depend on the start), DIR 1 the points ask (the vertices are
//                          transformed while they are staged); every block leaves the sums of its 64 pairs in a slot of its own
//   rigid_solve_kernel     adds the slots in block order, records the cost, solves, writes the next transform
//   rigid_pick_kernel      best, best_transform
// Trimmed calls (smalfit_trimmed_rigid_align) run rigid_scan_kernel<DIR, true>, which leaves every query's d^2 and match and no
// sums, then
//   rigid_trim_kernel      per (direction, start, mesh): a radix select of the keep-th key, then the kept pairs' sums in the scan's
//                          slots, so the solve reads what it always reads
// No float atomics; every float sum has a fixed order.

struct RigidArgs {
  int N, V, S, K;
  const float* verts;    // [N][V][3]
  const float* points;   // [N][S][3]
  float* T;              // [N][K][12]: the caller's `transforms`, the working transforms of the call
  float* cen;            // [N][6]: c_X | c_P
  float* part_v;         // [N][K][bv][kRigidMoments]: slots of DIR 0
  float* part_p;         // [N][K][bp][kRigidMoments]: slots of DIR 1
  int bv, bp;            // query blocks over the vertices | over the points
  int* vert_nn;          // [N][K][V] or null: written by the scans of the score's round alone
  int* point_nn;         // [N][K][S] or null
  // trimmed calls alone (null otherwise): every query's d^2 and match (-1: none) of the round, from the scan to the selection
  float* qd2_v;          // [N][K][V]
  int* qnn_v;            // [N][K][V]
  float* qd2_p;          // [N][K][S]
  int* qnn_p;            // [N][K][S]
};

struct RigidStarts {
  float R[SMALFIT_MAX_RIGID_STARTS][9];   // by value in the launch's argument: 2304 bytes, no copy to enqueue
};

constexpr int kRigidQueries = 64;    // queries per block: one per lane, the same 64 in each of the 4 waves
constexpr int kRigidChunk = 1024;    // records of the scanned set staged in LDS at a time; a wave scans a quarter
static_assert(kRigidQueries == kMeshQueries, "smalfit_plan.h sizes the scan grids by kMeshQueries");

// sum of the count elements src[3 i + c], lane l of 256 taking i = l, l + 256, ... in ascending order; block_sum adds the lanes
__device__ __forceinline__ float rigid_strided_sum(const float* src, int count, int c, float* red) {
  float s = 0.f;
  for (int i = threadIdx.x; i < count; i += 256) s += src[3 * (size_t)i + c];
  return block_sum(s, red);
}

__global__ __launch_bounds__(256) void rigid_init_kernel(RigidArgs a, RigidStarts st, const float* start_transforms) {
  __shared__ float red[16];
  const int n = blockIdx.x;
  const float* x = a.verts + (size_t)n * a.V * 3;
  const float* p = a.points + (size_t)n * a.S * 3;
  float cX[3], cP[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) cX[c] = rigid_strided_sum(x, a.V, c, red) / (float)a.V;
#pragma unroll
  for (int c = 0; c < 3; ++c) cP[c] = rigid_strided_sum(p, a.S, c, red) / (float)a.S;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a.cen[6 * (size_t)n + c] = cX[c];
      a.cen[6 * (size_t)n + 3 + c] = cP[c];
    }
  }
  const int k = threadIdx.x;
  if (k >= a.K) return;
  float* T = a.T + ((size_t)n * a.K + k) * 12;
  if (start_transforms != nullptr) {
    const float* src = start_transforms + ((size_t)n * a.K + k) * 12;
    float t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = src[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = t[i];
    return;
  }
  float t[12];
  rigid_start_transform(st.R[k], cX, cP, t);
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = t[i];
}

template <int DIR, bool TRIM = false>
__global__ __launch_bounds__(256) void rigid_scan_kernel(RigidArgs a) {
  __shared__ float sd[4][kRigidQueries];
  __shared__ int si[4][kRigidQueries];
  __shared__ ScanPoint rec[kRigidChunk];
  const int n = blockIdx.z, k = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR: the scan loop is scalar
  const int nq = DIR == 0 ? a.V : a.S, no = DIR == 0 ? a.S : a.V;
  const float* x = a.verts + (size_t)n * a.V * 3;
  const float* p = a.points + (size_t)n * a.S * 3;
  const float* q = DIR == 0 ? x : p;
  const float* o = DIR == 0 ? p : x;
  const size_t nk = (size_t)n * a.K + k;
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = a.T[nk * 12 + i];
  const int qi = blockIdx.x * kRigidQueries + lane;
  const bool active = qi < nq;
  float raw[3] = {0.f, 0.f, 0.f};
  if (active) {
    raw[0] = q[3 * (size_t)qi];
    raw[1] = q[3 * (size_t)qi + 1];
    raw[2] = q[3 * (size_t)qi + 2];
  }
  float qq[3] = {raw[0], raw[1], raw[2]};
  if (DIR == 0) rigid_apply(T, raw[0], raw[1], raw[2], qq);
  float best = INFINITY;
  int bidx = 0x7fffffff;
  float g[3] = {0.f, 0.f, 0.f};
  for (int base = 0; base < no; base += kRigidChunk) {
    const int cnt = min(kRigidChunk, no - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float* src = o + 3 * (size_t)(base + i);
      float z[3] = {src[0], src[1], src[2]};
      if (DIR == 1) rigid_apply(T, src[0], src[1], src[2], z);
      ScanPoint s;
      s.x = z[0];
      s.y = z[1];
      s.z = z[2];
      s.owner = 0;
      rec[i] = s;
    }
    __syncthreads();
    const Span sp = quarter_span(w, cnt);
    nearest_scan<false>(qq[0], qq[1], qq[2], rec, sp.b, sp.e, base, best, bidx, 0, g);
  }
  sd[w][lane] = best;
  si[w][lane] = bidx;
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) nearest_merge(best, bidx, sd[s][lane], si[s][lane]);
  // the pair of this query: (x_v, p_nn'(v)) or (x_nn(s), p_s), centred; a query without a match (NaN input) adds its d^2 alone
  const bool valid = active && (unsigned)bidx < (unsigned)no;
  if constexpr (TRIM) {
    // the trimmed form: the round's keys for rigid_trim_kernel, which forms the sums of the pairs it keeps
    if (active) {
      (DIR == 0 ? a.qd2_v : a.qd2_p)[nk * nq + qi] = best;
      (DIR == 0 ? a.qnn_v : a.qnn_p)[nk * nq + qi] = valid ? bidx : -1;
      int* nn = DIR == 0 ? a.vert_nn : a.point_nn;
      if (nn != nullptr) nn[nk * nq + qi] = valid ? bidx : -1;
    }
    return;
  }
  const float* partner = o + 3 * (size_t)(valid ? bidx : 0);
  const float pr[3] = {partner[0], partner[1], partner[2]};
  const float* cen = a.cen + 6 * (size_t)n;
  float xc[3], pc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    xc[c] = (DIR == 0 ? raw[c] : pr[c]) - cen[c];
    pc[c] = (DIR == 0 ? pr[c] : raw[c]) - cen[3 + c];
  }
  float m[kRigidMoments];
  rigid_pair_moments(xc, pc, best, m);
#pragma unroll
  for (int i = 0; i < kRigidMoments - 1; ++i) m[i] = wave_sum(valid ? m[i] : 0.f);
  m[kRigidMoments - 1] = wave_sum(active ? m[kRigidMoments - 1] : 0.f);
  int* nn = DIR == 0 ? a.vert_nn : a.point_nn;
  if (nn != nullptr && active) nn[nk * nq + qi] = valid ? bidx : -1;
  if (lane == 0) {
    float* slot = (DIR == 0 ? a.part_v : a.part_p) + (nk * gridDim.x + blockIdx.x) * kRigidMoments;
#pragma unroll
    for (int i = 0; i < kRigidMoments; ++i) slot[i] = m[i];
  }
}

struct RigidTrimArgs {
  int first_dir;              // the direction of block x = 0: 0 when the vertices ask, 1 when only the points do
  int dirs;                   // directions that are on: gridDim.x
  int keep_v, keep_p;
  unsigned char* vert_kept;   // [N][K][V] or null: the score's round alone, like vert_nn
  unsigned char* point_kept;  // [N][K][S] or null
  float* trim_d2;             // [N][K][2] or null
};

// inclusive scan of one int per thread over the block's 256 threads in thread order (a wave's lanes by shuffles, the four waves
// through `wtot`); *total: the sum over the block.  Two barriers; wtot is free again after it returns
__device__ __forceinline__ int rigid_block_scan(int v, int* wtot, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  __syncthreads();
  if (lane == 63) wtot[w] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = wtot[i];
    before += i < w ? t : 0;
    all += t;
  }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(256) void rigid_trim_kernel(RigidArgs a, RigidTrimArgs t) {
  __shared__ int hist[4][256];   // a histogram per wave: integer counters, their sums do not depend on the order of arrival
  __shared__ int wtot[4];
  __shared__ int sel[2];         // the chosen bucket and the rank left inside it
  __shared__ int tie;            // the threshold's query index
  const int n = blockIdx.z, k = blockIdx.y, lane = threadIdx.x & 63, tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int dir = t.first_dir + blockIdx.x;
  const int nq = dir == 0 ? a.V : a.S, no = dir == 0 ? a.S : a.V;
  const size_t nk = (size_t)n * a.K + k;
  const float* qd2 = (dir == 0 ? a.qd2_v : a.qd2_p) + nk * nq;
  const int* qnn = (dir == 0 ? a.qnn_v : a.qnn_p) + nk * nq;
  // ---- the keep-th key: four passes over the bits of d^2, eight at a time from the top; the keys are read again from memory every
  // pass (max_verts is not bounded by LDS)
  unsigned prefix = 0, mask = 0;
  int rank = dir == 0 ? t.keep_v : t.keep_p;   // 1-based, among the keys that share the prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) hist[i][tid] = 0;
    __syncthreads();
    for (int i = tid; i < nq; i += 256) {
      const unsigned bits = rigid_key_bits(qd2[i]);
      if (qnn[i] >= 0 && (bits & mask) == prefix) atomicAdd(&hist[w][(bits >> shift) & 255u], 1);
    }
    __syncthreads();
    const int mine = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
    int keys;
    const int incl = rigid_block_scan(mine, wtot, &keys);
    if (shift == 24) rank = min(rank, keys);   // fewer keys than keep: all of them are kept
    if (incl - mine < rank && rank <= incl) {  // one bucket holds the rank (none when there is no key at all)
      sel[0] = tid;
      sel[1] = rank - (incl - mine);
    }
    __syncthreads();
    if (rank > 0) {
      prefix |= (unsigned)sel[0] << shift;
      rank = sel[1];
    }
    mask |= 255u << shift;
  }
  // ---- ties: of the keys whose d^2 is the threshold's, the `rank` of the lowest query index are kept: an in-order scan
  const unsigned tbits = prefix;
  if (tid == 0) tie = -1;
  int seen = 0;
  for (int base = 0; base < nq; base += 256) {
    const int i = base + tid;
    const int hit = i < nq && qnn[i] >= 0 && rigid_key_bits(qd2[i]) == tbits ? 1 : 0;
    int total;
    const int incl = rigid_block_scan(hit, wtot, &total);
    if (hit && seen + incl == rank) tie = i;
    seen += total;
  }
  __syncthreads();
  const int tq = tie;
  // ---- the kept pairs' sums: the waves take the blocks of 64 queries in turn, each block summed as the scan sums it
  const float* x = a.verts + (size_t)n * a.V * 3;
  const float* p = a.points + (size_t)n * a.S * 3;
  const float* q = dir == 0 ? x : p;
  const float* o = dir == 0 ? p : x;
  const float* cen = a.cen + 6 * (size_t)n;
  const int blocks = dir == 0 ? a.bv : a.bp;
  unsigned char* kept_out = dir == 0 ? t.vert_kept : t.point_kept;
  for (int b = w; b < blocks; b += 4) {
    const int qi = b * kRigidQueries + lane;
    const bool active = qi < nq;
    const float d2 = active ? qd2[qi] : 0.f;
    const int nn = active ? qnn[qi] : -1;
    const bool kept = nn >= 0 && nn < no && rigid_key_kept(rigid_key_bits(d2), qi, tbits, tq);
    const float* qs = q + 3 * (size_t)(active ? qi : 0);
    const float* partner = o + 3 * (size_t)(kept ? nn : 0);
    const float raw[3] = {qs[0], qs[1], qs[2]};
    const float pr[3] = {partner[0], partner[1], partner[2]};
    float xc[3], pc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xc[c] = (dir == 0 ? raw[c] : pr[c]) - cen[c];
      pc[c] = (dir == 0 ? pr[c] : raw[c]) - cen[3 + c];
    }
    float m[kRigidMoments];
    rigid_pair_moments(xc, pc, d2, m);
#pragma unroll
    for (int i = 0; i < kRigidMoments; ++i) m[i] = wave_sum(kept ? m[i] : 0.f);
    if (kept_out != nullptr && active) kept_out[nk * nq + qi] = kept ? 1 : 0;
    if (lane == 0) {
      float* slot = (dir == 0 ? a.part_v : a.part_p) + (nk * blocks + b) * kRigidMoments;
#pragma unroll
      for (int i = 0; i < kRigidMoments; ++i) slot[i] = m[i];
    }
  }
  if (t.trim_d2 != nullptr && tid == 0) {
    t.trim_d2[nk * 2 + dir] = tq >= 0 ? rigid_key_value(tbits) : 0.f;
    if (t.dirs == 1) t.trim_d2[nk * 2 + (1 - dir)] = 0.f;
  }
}

struct RigidSolveArgs {
  float wv, wp;          // w_vert / V, w_point / S: one float32 divide each, on the host; 0: the direction is skipped
  int it, iterations;    // the round 0 .. I; round I records the score and solves nothing
  float* scores;         // [N][K]
  int* kept_rotation;    // [N][K]
  float* history;        // [N][K][I + 1] or null
};

__global__ __launch_bounds__(64) void rigid_solve_kernel(RigidArgs a, RigidSolveArgs s) {
  __shared__ float sm[2 * kRigidMoments];
  const int n = blockIdx.y, k = blockIdx.x, lane = threadIdx.x;
  const size_t nk = (size_t)n * a.K + k;
  if (lane < 2 * kRigidMoments) {
    const int dir = lane >= kRigidMoments ? 1 : 0, mi = lane - dir * kRigidMoments;
    const bool on = dir == 0 ? s.wv > 0.f : s.wp > 0.f;
    const int nb = dir == 0 ? a.bv : a.bp;
    const float* part = (dir == 0 ? a.part_v : a.part_p) + nk * nb * kRigidMoments + mi;
    float t = 0.f;
    if (on) {
      // (unrolled: eight independent loads in flight; the adds stay in block order)
#pragma unroll 8
      for (int b = 0; b < nb; ++b) t += part[(size_t)b * kRigidMoments];
    }
    sm[lane] = t;
  }
  __syncthreads();
  if (lane != 0) return;
  float M[kRigidMoments];
  rigid_combine(s.wv > 0.f ? sm : nullptr, s.wp > 0.f ? sm + kRigidMoments : nullptr, s.wv, s.wp, M);
  const float cost = M[kRigidMoments - 1];
  if (s.history != nullptr) s.history[nk * (size_t)(s.iterations + 1) + s.it] = cost;
  const int kept_before = s.it == 0 ? 0 : s.kept_rotation[nk];
  if (s.it == s.iterations) {
    s.scores[nk] = cost;
    s.kept_rotation[nk] = kept_before;
    return;
  }
  float prev[12], next[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) prev[i] = a.T[nk * 12 + i];
  const float* cen = a.cen + 6 * (size_t)n;
  const int kept = rigid_solve(M, cen, cen + 3, prev, next);
#pragma unroll
  for (int i = 0; i < 12; ++i) a.T[nk * 12 + i] = next[i];
  s.kept_rotation[nk] = kept_before + kept;
}

// the lowest score, the lowest k among equal ones; a NaN never wins (all NaN: start 0)
__global__ __launch_bounds__(64) void rigid_pick_kernel(int N, int K, const float* scores, const float* T, int* best, float* best_transform) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  int b = -1;
  float bs = 0.f;
  for (int k = 0; k < K; ++k) {
    const float sc = scores[(size_t)n * K + k];
    if (sc == sc && (b < 0 || sc < bs)) {
      b = k;
      bs = sc;
    }
  }
  if (b < 0) b = 0;
  best[n] = b;
  for (int i = 0; i < 12; ++i) best_transform[(size_t)n * 12 + i] = T[((size_t)n * K + b) * 12 + i];
}

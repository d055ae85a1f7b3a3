// Kernels of the 3D mesh-fitting objective (SURVEY.md §8f row 3; reference fitter_3d/trainer.py:205-227 and the
// PyTorch3D v0.2.5 losses it calls).  Included by smalfit_kernels.hip inside namespace smalfit.
//
// One evaluation = 6 launches on N meshes of the SMAL topology (V vertices, E unique edges, P face pairs) against S
// sampled target points per mesh:
//   mesh3d_compose      verts = LBS verts + trans + deform_verts                            (trainer.py:94-108)
//   mesh3d_chamfer<0>   every target point finds its nearest vertex (index kept for the adjoint)
//   mesh3d_chamfer<1>   every vertex finds its nearest target point AND gathers the points that chose it:
//                       the whole chamfer gradient of a vertex is formed in one thread, no scatter, no atomics
//   mesh3d_ring         per vertex: edge term + its gradient, Laplacian residual direction; per face pair: normal
//                       consistency and its 4 vertex gradients
//   mesh3d_gather       per vertex: Laplacian adjoint over the ring + the pair gradients it takes part in (CSR from
//                       mesh3d_topology.h) + the two stored gradients -> dL/dverts, per-block partial of dL/dtrans
//   mesh3d_reduce       fixed-order sums of the per-block partials -> the 4 terms, the total, dL/dtrans
// All bounds are HBM/L2 latency and VALU issue on ~50 KB of vertices per mesh; the only O(S V) work is the two chamfer
// scans (2 x 11.7 M point pairs per mesh at S = 3000), staged through LDS and split over the 4 waves of a block.
// Everything is deterministic: every sum has a fixed order.

struct Mesh3dTables {
  int V, E, P;
  const int* nbr_off;   // [V+1]
  const int* nbr;       // [2E]
  const int* pairs;     // [P][4]
  const int* inc_off;   // [V+1]
  const int* inc;       // [4P]
};

struct Mesh3dArgs {
  int N, V, S;
  Mesh3dTables t;
  const float* lbs_verts;  // [N][V][3], or null when lbs_planar is given
  const float* lbs_planar; // [N][3][Vp]: the engine's own layout (smalfit_fit3d_step reads it in place)
  int Vp;
  const float* trans;      // [N][3]
  const float* deform;     // [N][V][3] or null
  float* verts;            // [N][V][3] composed
  const float* points;     // [N][S][3]
  int* nn_idx;             // [N][S] nearest vertex of every target point
  float* gcham;            // [N][V][3] gradient of w_chamfer * chamfer
  float* gedge;            // [N][V][3] gradient of w_edge * edge
  float* lap_unit;         // [N][V][3]
  float* gpair;            // [N][P][4][3] d(1 - cos) / d(v0, v1, a, b), unweighted
  float* dverts;           // [N][V][3]
  float* dverts_planar;    // [N][3][Vp] second copy for the LBS adjoint (padding zeroed), or null
  float* dtrans;           // [N][3]
  float* losses;           // [5] chamfer, edge, normal, laplacian (unweighted), total
  float w_chamfer, w_edge, w_normal, w_laplacian;   // <= 0: term skipped (trainer.py:203)
  // per-block partials
  float* part_cx;          // [N][bx]
  float* part_cy;          // [N][by]
  float* part_edge;        // [N][bv]
  float* part_lap;         // [N][bv]
  float* part_normal;      // [N][bp]
  float* part_dtr;         // [N][bv][3]
  int bx, by, bv, bp;
  // the gates of the chamfer term (smalfit_chamfer_gate_args, planned by plan_chamfer_gates); read by the GATED instantiations and,
  // `kept`, by the reduce
  const float* normals_v;        // [N][V][3] unit normals of the fitted vertices, or null: the compatibility tests are off
  const float* normals_p;        // [N][S][3] unit normals of the points, or null
  const unsigned char* bound_p;  // [N][S] boundary bytes of the points, or null: no boundary rule
  float cos_p, cos_v;            // c of point -> vertex | vertex -> point; -inf: off
  float tau2_p, tau2_v;          // +inf: no truncation
  int* part_kx;                  // [N][bx] per-block kept counts of chamfer<0, true>, null where chamfer<0, false> ran
  int* part_ky;                  // [N][by]
  int* kept;                     // [N][2] or null
  unsigned char* point_kept;     // [N][S] or null
  unsigned char* vert_kept;      // [N][V] or null
  int* point_nn;                 // [N][S] or null: a copy of nn_idx
  int* vert_nn;                  // [N][V] or null
  // the robust kernel (smalfit_robust_args, planned by plan_robust); read by the ROBUST instantiations and, `weight_sums`, by the reduce
  float s2_p, s2_v;              // sigma^2 of point -> vertex | vertex -> point; 0: off (w = 1, rho = d^2)
  float* wts;                    // [N][S] w_s of every point's match (0: dropped), written by chamfer<0, ., true>, staged by <1, ., true>
  float* part_wx;                // [N][bx] per-block sums of w of chamfer<0, ., true>, null where no ROBUST instantiation ran
  float* part_wy;                // [N][by]
  float* weight_sums;            // [N][2] or null
  float* point_w;                // [N][S] or null: a copy of wts
  float* vert_w;                 // [N][V] or null
};

constexpr int kChamQueries = 64;    // queries per block: one per lane, the same 64 in each of the 4 waves
constexpr int kChamChunk = 1024;    // points of the scanned set staged in LDS at a time; a wave scans a quarter
static_assert(kChamGateChunk * sizeof(GatedScanPoint) == kChamChunk * sizeof(ScanPoint), "the gated chunk fills the ungated one's LDS");
constexpr int kMeshBlock = 256;

__global__ __launch_bounds__(256) void mesh3d_compose_kernel(Mesh3dArgs a) {
  const size_t total = (size_t)a.N * a.V * 3;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i / ((size_t)a.V * 3));
  const int k = (int)(i % 3);
  const int vtx = (int)((i / 3) % (size_t)a.V);
  const float lbs = a.lbs_planar != nullptr ? a.lbs_planar[((size_t)n * 3 + k) * a.Vp + vtx] : a.lbs_verts[i];
  float v = lbs + a.trans[3 * n + k];
  if (a.deform != nullptr) v += a.deform[i];
  a.verts[i] = v;
}

// ROLE 0: queries = target points, scanned set = vertices.  ROLE 1: queries = vertices, scanned set = target points.
// One staging loop, one scan call, one tail; the flags choose the record, the decision and the outputs:
//   record    <., false, .> stages ScanPoint, kChamChunk at a time; GATED the 32-byte GatedScanPoint, kChamGateChunk at a time -- the
//             same 16 KB, so a block's LDS and its four blocks a CU do not change -- and scans for the nearest COMPATIBLE element
//             (the query's unit normal in three registers, c a scalar; c = -inf: no normal is read, every record is compatible).
//             ROBUST ROLE 1 stages the points' weights w_s in a float array beside the records and gathers sum w_s (y_v - x_s)
//             with the same branch-free mask: no divide enters the scan
//   decision  the waves' minima meet, then wave 0 decides once per query: chamfer_match<GATED, ROBUST> (mesh3d_math.h)
//   outputs   a dropped point writes nn_idx = -1, so no vertex gathers it; a dropped query adds nothing to the block's sum or to
//             its own gradient term (chamfer_vertex_grad); GATED puts the block's kept count beside its sum, ROBUST the block's
//             sum of w, and ROLE 0 leaves w_s per point (0 for a dropped one)
template <int ROLE, bool GATED, bool ROBUST = false>
__global__ __launch_bounds__(256) void mesh3d_chamfer_kernel(Mesh3dArgs a) {
  __shared__ float sd[4][kChamQueries];
  __shared__ int si[4][kChamQueries];
  __shared__ float sg[ROLE == 1 ? 4 : 1][kChamQueries][3];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR: the scan loop is scalar
  const int nq = ROLE == 0 ? a.S : a.V, no = ROLE == 0 ? a.V : a.S;
  const float* q = ROLE == 0 ? a.points + (size_t)n * a.S * 3 : a.verts + (size_t)n * a.V * 3;
  const float* o = ROLE == 0 ? a.verts + (size_t)n * a.V * 3 : a.points + (size_t)n * a.S * 3;
  const int* own = a.nn_idx + (size_t)n * a.S;
  const int qi = blockIdx.x * kChamQueries + lane;
  const bool active = qi < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = q[3 * (size_t)qi];
    qy = q[3 * (size_t)qi + 1];
    qz = q[3 * (size_t)qi + 2];
  }
  // GATED: the query's unit normal and the scanned set's, read only while this direction's compatibility test is on
  const float c = ROLE == 0 ? a.cos_p : a.cos_v;
  const bool use_normals = GATED && c != -INFINITY;
  const float* on = ROLE == 0 ? a.normals_v + (size_t)n * a.V * 3 : a.normals_p + (size_t)n * a.S * 3;
  const unsigned char* ob = ROLE == 1 && a.bound_p != nullptr ? a.bound_p + (size_t)n * a.S : nullptr;
  float ux = 0.f, uy = 0.f, uz = 0.f;
  if (use_normals && active) {
    const float* u = (ROLE == 0 ? a.normals_p : a.normals_v) + ((size_t)n * nq + qi) * 3;
    ux = u[0];
    uy = u[1];
    uz = u[2];
  }
  float best = INFINITY;
  int bidx = 0x7fffffff;   // GATED: the winner's tag (gated_tag: ascending with the index)
  float g[3] = {0.f, 0.f, 0.f};
  // one staging loop for both record types: the chunk is sized so that either fills the same 16 KB
  using Record = typename std::conditional<GATED, GatedScanPoint, ScanPoint>::type;
  constexpr int kChunk = GATED ? kChamGateChunk : kChamChunk;
  constexpr bool kWeighted = ROBUST && ROLE == 1;
  __shared__ float sw[kWeighted ? kChunk : 1];   // (not used, and not allocated, unless kWeighted)
  __shared__ Record rec[kChunk];
  const float* wsrc = a.wts + (size_t)n * a.S;
  for (int base = 0; base < no; base += kChunk) {
    const int cnt = min(kChunk, no - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const float* src = o + 3 * (size_t)(base + i);
      Record s;
      s.x = src[0];
      s.y = src[1];
      s.z = src[2];
      s.owner = ROLE == 1 ? own[base + i] : 0;
      if constexpr (GATED) {
        s.nx = s.ny = s.nz = 0.f;
        if (use_normals) {
          const float* sn = on + 3 * (size_t)(base + i);
          s.nx = sn[0];
          s.ny = sn[1];
          s.nz = sn[2];
        }
        s.tag = gated_tag(base + i, ob != nullptr ? ob[base + i] : 0);
      }
      rec[i] = s;
      if constexpr (kWeighted) sw[i] = wsrc[base + i];
    }
    __syncthreads();
    // the span is wave-uniform: every lane reads the same 16-byte LDS rows of a record (broadcast, conflict free)
    const Span sp = quarter_span(w, cnt);
    scan_records<ROLE == 1, kWeighted>(qx, qy, qz, ux, uy, uz, c, rec, sp.b, sp.e, base, best, bidx, qi, g, kWeighted ? sw : nullptr);
  }
  sd[w][lane] = best;
  si[w][lane] = bidx;
  if (ROLE == 1) {
    sg[w][lane][0] = g[0];
    sg[w][lane][1] = g[1];
    sg[w][lane][2] = g[2];
  }
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) {
    nearest_merge(best, bidx, sd[s][lane], si[s][lane]);
    if (ROLE == 1) {
      g[0] += sg[s][lane][0];
      g[1] += sg[s][lane][1];
      g[2] += sg[s][lane][2];
    }
  }
  // one tail: the decision of this instantiation, then the outputs it has
  const ChamferMatch m = chamfer_match<GATED, ROBUST>(best, bidx, ROLE == 0 ? a.tau2_p : a.tau2_v, ob != nullptr ? 1 : 0,
                                                      ROLE == 0 ? a.s2_p : a.s2_v, active);
  if (active) {
    const size_t oq = (size_t)n * nq + qi;
    if (ROLE == 0) {
      const int nn = GATED && !m.kept ? -1 : m.index;   // a dropped point is gathered by no vertex
      a.nn_idx[oq] = nn;
      if constexpr (ROBUST) {
        a.wts[oq] = m.w;
        if (a.point_w != nullptr) a.point_w[oq] = m.w;
      }
      if constexpr (GATED) {
        if (a.point_nn != nullptr) a.point_nn[oq] = nn;
        if (a.point_kept != nullptr) a.point_kept[oq] = m.kept ? 1 : 0;
      }
    } else {
      if constexpr (ROBUST) {
        if (a.vert_w != nullptr) a.vert_w[oq] = m.w;
      }
      if constexpr (GATED) {
        if (a.vert_nn != nullptr) a.vert_nn[oq] = m.index;
        if (a.vert_kept != nullptr) a.vert_kept[oq] = m.kept ? 1 : 0;
      }
      // d/dy_j of [ (1/(V N)) rho(|y_j - x_nn(j)|^2) + (1/(S N)) sum_{i: nn(i) = j} rho(|x_i - y_j|^2) ]; a dropped vertex keeps only
      // what it gathered
      float cy = a.w_chamfer * 2.0f / ((float)a.V * (float)a.N);
      if constexpr (ROBUST) cy = cy * m.w;
      else if constexpr (GATED) cy = m.kept ? cy : 0.f;
      const float cx = a.w_chamfer * 2.0f / ((float)a.S * (float)a.N);
      const float y[3] = {qx, qy, qz};
      chamfer_vertex_grad(cy, cx, y, o, no, m.kept, m.index, g, a.gcham + oq * 3);
    }
  }
  const float tot = wave_sum(m.kept ? m.rho : 0.f);
  float wtot = 0.f;
  if constexpr (ROBUST) wtot = wave_sum(m.w);
  const int cnt = GATED ? __popcll(__ballot(m.kept)) : 0;   // (an integer count: no order to fix)
  if (lane == 0) {
    const size_t slot = (size_t)n * gridDim.x + blockIdx.x;
    (ROLE == 0 ? a.part_cx : a.part_cy)[slot] = tot;
    if constexpr (ROBUST) (ROLE == 0 ? a.part_wx : a.part_wy)[slot] = wtot;
    if constexpr (GATED) (ROLE == 0 ? a.part_kx : a.part_ky)[slot] = cnt;
  }
}

// blocks [0, bv): one vertex per thread; blocks [bv, bv + bp): one face pair per thread
__global__ __launch_bounds__(kMeshBlock) void mesh3d_ring_kernel(Mesh3dArgs a) {
  __shared__ float red[16];
  const int n = blockIdx.y;
  const float* verts = a.verts + (size_t)n * a.V * 3;
  if ((int)blockIdx.x < a.bv) {
    const int v = blockIdx.x * kMeshBlock + threadIdx.x;
    float es = 0.f, ln = 0.f;
    if (v < a.V) {
      const int off = a.t.nbr_off[v], deg = a.t.nbr_off[v + 1] - off;
      RingEval r;
      vertex_ring(verts, v, a.t.nbr + off, deg, r);
      es = r.edge_sum;
      ln = r.lap_norm;
      const float ce = a.w_edge * 2.0f / ((float)a.t.E * (float)a.N);
      const size_t o = ((size_t)n * a.V + v) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.gedge[o + k] = ce * r.edge_grad[k];
        a.lap_unit[o + k] = r.lap_unit[k];
      }
    }
    const float te = block_sum(es, red);
    const float tl = block_sum(ln, red);
    if (threadIdx.x == 0) {
      a.part_edge[(size_t)n * a.bv + blockIdx.x] = te;
      a.part_lap[(size_t)n * a.bv + blockIdx.x] = tl;
    }
  } else {
    const int blk = blockIdx.x - a.bv;
    const int p = blk * kMeshBlock + threadIdx.x;
    float val = 0.f;
    if (p < a.t.P) {
      const int* row = a.t.pairs + 4 * (size_t)p;
      float grad[4][3];
      val = face_pair_eval(verts + 3 * (size_t)row[0], verts + 3 * (size_t)row[1], verts + 3 * (size_t)row[2],
                           verts + 3 * (size_t)row[3], grad);
      float* out = a.gpair + ((size_t)n * a.t.P + p) * 12;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * r + k] = grad[r][k];
    }
    const float tn = block_sum(val, red);
    if (threadIdx.x == 0) a.part_normal[(size_t)n * a.bp + blk] = tn;
  }
}

__global__ __launch_bounds__(kMeshBlock) void mesh3d_gather_kernel(Mesh3dArgs a) {
  __shared__ float red[16];
  const int n = blockIdx.y;
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  float g[3] = {0.f, 0.f, 0.f};
  if (v < a.V) {
    const size_t o = ((size_t)n * a.V + v) * 3;
    const int off = a.t.nbr_off[v], deg = a.t.nbr_off[v + 1] - off;
    float gl[3];
    laplacian_adjoint(a.lap_unit + (size_t)n * a.V * 3, v, a.t.nbr + off, deg, a.t.nbr_off, gl);
    float gn[3] = {0.f, 0.f, 0.f};
    const float* gp = a.gpair + (size_t)n * a.t.P * 12;
    for (int s = a.t.inc_off[v]; s < a.t.inc_off[v + 1]; ++s) {
      const float* src = gp + 3 * (size_t)a.t.inc[s];
      gn[0] += src[0];
      gn[1] += src[1];
      gn[2] += src[2];
    }
    const float cl = a.w_laplacian / ((float)a.V * (float)a.N);
    const float cn = a.t.P > 0 ? a.w_normal / ((float)a.t.P * (float)a.N) : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g[k] = a.gcham[o + k] + a.gedge[o + k] + cl * gl[k] + cn * gn[k];
      a.dverts[o + k] = g[k];
    }
  }
  if (a.dverts_planar != nullptr && v < a.Vp) {   // the grid covers exactly Vp = 256 * bv vertices: padding gets zeros
#pragma unroll
    for (int k = 0; k < 3; ++k) a.dverts_planar[((size_t)n * 3 + k) * a.Vp + v] = g[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = block_sum(g[k], red);
    if (threadIdx.x == 0) a.part_dtr[((size_t)n * a.bv + blockIdx.x) * 3 + k] = t;
  }
}

// one block: thread-strided partial sums in a fixed order, then the fixed tree of block_sum
__device__ __forceinline__ float mesh3d_sum(const float* p, int count, float* red) {
  float s = 0.f;
  for (int i = threadIdx.x; i < count; i += blockDim.x) s += p[i];
  return block_sum(s, red);
}

// a mesh's total of per-block partials, in block order, one thread per mesh; `otherwise` where no kernel wrote any (part == null)
template <typename T>
__device__ __forceinline__ T mesh_total(const T* part, int n, int blocks, T otherwise) {
  if (part == nullptr) return otherwise;
  T s = 0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)n * blocks + b];
  return s;
}
// what a reduce reports of one direction of a data term on mesh n: the kept count, summed from the counting (GATED) kernel's
// partials -- where none ran nothing was dropped and nothing counted: every query of a direction that is on -- and the sum of
// the weights, from the ROBUST kernel's partials -- where none ran every weight is 1: the kept count, as a float
struct DirectionTotals { int kept; float w; };
__device__ __forceinline__ DirectionTotals direction_totals(const int* part_kept, const float* part_w, int n, int blocks, bool on,
                                                            int queries) {
  DirectionTotals t;
  t.kept = mesh_total(part_kept, n, blocks, on ? queries : 0);
  t.w = mesh_total(part_w, n, blocks, (float)t.kept);
  return t;
}
// rows [n][2] = points | vertices of the outputs that were asked for
__device__ __forceinline__ void write_direction_totals(int* kept, float* weight_sums, int n, const DirectionTotals& p,
                                                       const DirectionTotals& v) {
  if (kept != nullptr) {
    kept[2 * n] = p.kept;
    kept[2 * n + 1] = v.kept;
  }
  if (weight_sums != nullptr) {
    weight_sums[2 * n] = p.w;
    weight_sums[2 * n + 1] = v.w;
  }
}

__global__ __launch_bounds__(256) void mesh3d_reduce_kernel(Mesh3dArgs a) {
  __shared__ float red[16];
  const float fn = (float)a.N;
  const float cx = mesh3d_sum(a.part_cx, a.N * a.bx, red) / ((float)a.S * fn);
  const float cy = mesh3d_sum(a.part_cy, a.N * a.by, red) / ((float)a.V * fn);
  const float ed = mesh3d_sum(a.part_edge, a.N * a.bv, red) / (2.0f * (float)a.t.E * fn);   // every edge seen from both ends
  const float lp = mesh3d_sum(a.part_lap, a.N * a.bv, red) / ((float)a.V * fn);
  const float nm = a.t.P > 0 ? mesh3d_sum(a.part_normal, a.N * a.bp, red) / ((float)a.t.P * fn) : 0.f;
  if (threadIdx.x == 0) {
    const float ch = a.w_chamfer > 0.f ? cx + cy : 0.f;
    a.losses[0] = ch;
    a.losses[1] = ed;
    a.losses[2] = nm;
    a.losses[3] = lp;
    a.losses[4] = (a.w_chamfer > 0.f ? a.w_chamfer * ch : 0.f) + (a.w_edge > 0.f ? a.w_edge * ed : 0.f) +
                  (a.w_normal > 0.f ? a.w_normal * nm : 0.f) + (a.w_laplacian > 0.f ? a.w_laplacian * lp : 0.f);
  }
  for (int o = threadIdx.x; o < 3 * a.N; o += blockDim.x) {
    const int n = o / 3, k = o % 3;
    float s = 0.f;
    for (int b = 0; b < a.bv; ++b) s += a.part_dtr[((size_t)n * a.bv + b) * 3 + k];
    a.dtrans[o] = s;
  }
  if (a.kept != nullptr || a.weight_sums != nullptr) {
    for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
      const DirectionTotals p = direction_totals(a.part_kx, a.part_wx, n, a.bx, a.w_chamfer > 0.f, a.S);
      const DirectionTotals v = direction_totals(a.part_ky, a.part_wy, n, a.by, a.w_chamfer > 0.f, a.V);
      write_direction_totals(a.kept, a.weight_sums, n, p, v);
    }
  }
}

// ---- sample_points_from_meshes ----------------------------------------------------------------------------------
struct MeshTargetsDev {
  int N;
  const int* voff;          // [N+1] vertex offsets of the packed meshes
  const int* foff;          // [N+1] face offsets
  const float* verts;       // packed [sum V][3]
  const int* faces;         // packed [sum F][3], indices local to the mesh
  const uint32_t* thr;      // packed [sum F] cumulative-area thresholds (mesh3d_topology.h)
};

// ATTRS: also what the gates ask of a point (smalfit_mesh_targets_sample_attrs; the points are those of <false>): the unit normal
// of the sampled face (normals != null) and its boundary byte, bflags of that face != 0 (boundary != null)
template <bool ATTRS>
__global__ __launch_bounds__(256) void mesh3d_sample_kernel(MeshTargetsDev t, int S, uint32_t seed_lo, uint32_t seed_hi,
                                                           uint32_t iteration, float* points /* [N][S][3] */,
                                                           float* normals /* [N][S][3] or null, ATTRS only */,
                                                           unsigned char* boundary /* [N][S] or null, ATTRS only */,
                                                           const unsigned char* bflags /* packed [sum F], ATTRS only */) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S) return;
  const Philox4 r = philox4x32_10((uint32_t)i, (uint32_t)n, iteration, 0u, seed_lo, seed_hi);
  const int f0 = t.foff[n], nf = t.foff[n + 1] - f0;
  const int f = sample_face(t.thr + f0, nf, r.v[0]);
  const int* fc = t.faces + 3 * (size_t)(f0 + f);
  const float* base = t.verts + 3 * (size_t)t.voff[n];
  float out[3];
  barycentric_sample(base + 3 * (size_t)fc[0], base + 3 * (size_t)fc[1], base + 3 * (size_t)fc[2], unit_float(r.v[1]),
                     unit_float(r.v[2]), out);
  float* dst = points + ((size_t)n * S + i) * 3;
  dst[0] = out[0];
  dst[1] = out[1];
  dst[2] = out[2];
  if (ATTRS) {
    if (normals != nullptr) {
      float u[3];
      face_unit_normal(base + 3 * (size_t)fc[0], base + 3 * (size_t)fc[1], base + 3 * (size_t)fc[2], u);
      float* dn = normals + ((size_t)n * S + i) * 3;
      dn[0] = u[0];
      dn[1] = u[1];
      dn[2] = u[2];
    }
    if (boundary != nullptr) boundary[(size_t)n * S + i] = bflags[f0 + f] != 0 ? 1 : 0;
  }
}

// ---- smalfit_mesh_score: exact point-to-surface distances both ways, per mesh ------------------------------------------
// 3 launches: mesh3d_surface_dist<0> (every fitted vertex against the triangles of its target mesh), mesh3d_surface_dist<1>
// (every target point against the triangles of the fitted mesh; skipped without points), mesh3d_score_reduce (one block per
// direction and mesh: sum d, sum d^2, max d, counts within the thresholds).  O(V F_target + S F) pair tests per mesh, each
// point_scan_tri_dist2 of mesh3d_math.h; a minimum has no order and every sum a fixed one, so the results are reproducible.
struct MeshScoreArgs {
  int N, V, S, F;           // meshes, fitted vertices, points per mesh (0: none), faces of the fitted topology
  const float* verts;       // [N][V][3]
  const float* points;      // [N][S][3] or null
  const int* faces;         // [F][3] of the fitted topology
  MeshTargetsDev t;
  float* vert_dist;         // [N][V]
  float* point_dist;        // [N][S]
  float* sums;              // [N][2][3]
  int* within;              // [N][2][T] or null
  int T;
  float thr[SMALFIT_MAX_SCORE_THRESHOLDS];
};

// ROLE 0: queries = fitted vertices, scanned = the triangles of target mesh n (its own slice of the packed targets).
// ROLE 1: queries = the caller's points, scanned = the triangles of the fitted mesh n.
template <int ROLE>
__global__ __launch_bounds__(256) void mesh3d_surface_dist_kernel(MeshScoreArgs a) {
  __shared__ ScanTri st[kSurfaceChunk];
  __shared__ float sd[4][kChamQueries];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave index in an SGPR: the scan loop is scalar
  const int nq = ROLE == 0 ? a.V : a.S;
  const float* q = ROLE == 0 ? a.verts + (size_t)n * a.V * 3 : a.points + (size_t)n * a.S * 3;
  const int f0 = ROLE == 0 ? a.t.foff[n] : 0;
  const int nf = ROLE == 0 ? a.t.foff[n + 1] - f0 : a.F;
  const int* faces = (ROLE == 0 ? a.t.faces : a.faces) + 3 * (size_t)f0;
  const float* corners = ROLE == 0 ? a.t.verts + 3 * (size_t)a.t.voff[n] : a.verts + (size_t)n * a.V * 3;
  const int qi = blockIdx.x * kChamQueries + lane;
  const bool active = qi < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = q[3 * (size_t)qi];
    qy = q[3 * (size_t)qi + 1];
    qz = q[3 * (size_t)qi + 2];
  }
  float best = INFINITY;
  for (int base = 0; base < nf; base += kSurfaceChunk) {
    const int cnt = min(kSurfaceChunk, nf - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const int* fc = faces + 3 * (size_t)(base + i);
      st[i] = make_scan_tri(corners + 3 * (size_t)fc[0], corners + 3 * (size_t)fc[1], corners + 3 * (size_t)fc[2]);
    }
    __syncthreads();
    // the span is wave-uniform: every lane reads the same four 16-byte rows of a record (broadcast, conflict free)
    const Span sp = quarter_span(w, cnt);
    best = surface_scan(qx, qy, qz, st, sp.b, sp.e, best);
  }
  sd[w][lane] = best;
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) best = fminf(best, sd[s][lane]);
  if (active) (ROLE == 0 ? a.vert_dist + (size_t)n * a.V : a.point_dist + (size_t)n * a.S)[qi] = sqrtf(best);
}

// block (dir, n): thread-strided partials in a fixed order, then the fixed tree of block_sum; the maximum and the integer
// counts have no order.  Direction 1 without points has no queries: its rows are zeros
__global__ __launch_bounds__(256) void mesh3d_score_reduce_kernel(MeshScoreArgs a) {
  __shared__ float red[16];
  __shared__ float wmax[4];
  __shared__ int wcnt[4][SMALFIT_MAX_SCORE_THRESHOLDS];
  const int dir = blockIdx.x, n = blockIdx.y;
  const int nq = dir == 0 ? a.V : a.S;
  const float* d = dir == 0 ? a.vert_dist + (size_t)n * a.V : a.point_dist + (size_t)n * a.S;
  float s1 = 0.f, s2 = 0.f, mx = 0.f;
  int cnt[SMALFIT_MAX_SCORE_THRESHOLDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nq; i += 256) {
    const float v = d[i];
    s1 += v;
    s2 += v * v;
    mx = fmaxf(mx, v);
#pragma unroll
    for (int t = 0; t < SMALFIT_MAX_SCORE_THRESHOLDS; ++t) cnt[t] += (t < a.T && v <= a.thr[t]) ? 1 : 0;
  }
  const float t1 = block_sum(s1, red);
  const float t2 = block_sum(s2, red);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
#pragma unroll
  for (int t = 0; t < SMALFIT_MAX_SCORE_THRESHOLDS; ++t)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt[t] += __shfl_xor(cnt[t], o, 64);
  if (lane == 0) {
    wmax[w] = mx;
#pragma unroll
    for (int t = 0; t < SMALFIT_MAX_SCORE_THRESHOLDS; ++t) wcnt[w][t] = cnt[t];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = a.sums + ((size_t)n * kScoreDirections + dir) * 3;
    out[0] = t1;
    out[1] = t2;
    out[2] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  }
  if (a.within != nullptr && (int)threadIdx.x < a.T)
    a.within[((size_t)n * kScoreDirections + dir) * a.T + threadIdx.x] =
        wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
}

// ---- the surface term: the same distances as a term to descend on, every iteration -------------------------------------------
// One memset of the keys, then per direction mesh3d_surface_near<ROLE> (the scan, split over the triangles: grid z) and
// mesh3d_surface_hit<ROLE> (one query per thread: the winner's barycentrics and residual, per-block sums of d^2), then
// mesh3d_surface_grad (one vertex per lane: its own residual + the hits of the points that chose a face it is a corner of,
// gathered in a fixed order -- no scatter, no floating-point atomics) and mesh3d_surface_reduce (one block).  The slices of a
// query meet in a 64-bit key, d^2's bits high and the face index low: d^2 >= 0, so the order of the bits is the order of the
// values, and the integer minimum is the lowest face among equal distances whatever order the blocks run in.
struct SurfaceTermArgs {
  int N, V, S, F;            // meshes, fitted vertices, points per mesh, faces of the fitted topology
  const float* verts;        // [N][V][3]
  const float* points;       // [N][S][3] (read when w_ps > 0)
  const int* faces;          // [F][3] of the fitted topology
  MeshTargetsDev t;          // (read when w_vs > 0)
  const ScanTri* target_tris;// packed [sum F]: the targets' staged records, built once at smalfit_mesh_targets_create
  float w_ps, w_vs;          // both clamped at 0
  unsigned long long* keys_v;// [N][V]
  unsigned long long* keys_p;// [N][S]
  SurfaceHit* hits;          // [N][S]
  float* res_v;              // [N][V][3] residual of every vertex
  int* point_face; float* point_bary; int* vert_face; float* vert_bary;   // optional
  float* point_residual; float* vert_residual;                            // optional
  float* part_ps;            // [N][hp] per-block sums of d^2, hp = blocks of mesh3d_surface_hit<1>
  float* part_vs;            // [N][hv]
  float* part_dtr;           // [N][gv][3]
  int hp, hv, gv;
  float* acc_dverts;         // [N][V][3] or null: the step's d verts, the term's gradient is added to it ...
  float* acc_planar;         // [N][3][Vp] or null: ... and to its planar copy for the LBS adjoint ...
  float* acc_dtrans;         // [N][3] or null: ... and its sum over a mesh to the step's d trans
  int Vp;
  float* dverts;             // [N][V][3] or null: written
  float* dtrans;             // [N][3] or null
  float* losses;             // [3]
  float* rows;               // [N][2] or null
  const float* step_losses;  // [5] of the step this term rides on, or null
  float* step_total;         // [1] or null: step_losses[4] + the weighted term
  // the gates (smalfit_surface_gate_args, planned by plan_surface_gates); read by the GATED instantiations and, `kept`, by the reduce
  const float* normals_v;    // [N][V][3] unit normals of the fitted vertices (mesh3d_vertex_normal_kernel), near<0, true> only
  const float* normals_p;    // [N][S][3] unit normals of the points, near<1, true> only
  float cc_v, cc_p;          // c |c| of the compatibility test
  float tau2_v, tau2_p;      // +inf: no truncation
  const unsigned char* bflags; // packed [sum F] boundary flags of the targets, or null: no boundary rule
  int* part_kv;              // [N][hv] per-block kept counts of hit<0, true>, null where hit<0, false> ran
  int* part_kp;              // [N][hp]
  unsigned char* vert_kept;  // [N][V] or null
  unsigned char* point_kept; // [N][S] or null
  int* kept;                 // [N][2] or null
  const int* vf_off;         // [V+1], [3F]: vertex -> incident faces of the fitted topology (mesh3d_vertex_normal_kernel)
  const int* vf;
  float* normals_out;        // [N][V][3] what mesh3d_vertex_normal_kernel writes (= normals_v)
  // the robust kernel (smalfit_robust_args, planned by plan_robust); read by the ROBUST instantiations and, `weight_sums`, by the reduce
  float s2_v, s2_p;          // sigma^2 of vertex -> surface | point -> surface (> 0 where the ROBUST instantiation runs)
  float* part_wv;            // [N][hv] per-block sums of w of hit<0, ., true>, null where hit<0, ., false> ran
  float* part_wp;            // [N][hp]
  float* weight_sums;        // [N][2] or null
  float* vert_w;             // [N][V] or null
  float* point_w;            // [N][S] or null
};

// ROLE 0: queries = fitted vertices, scanned = the staged records of target mesh n.  ROLE 1: queries = the points, scanned = the
// triangles of the fitted mesh n, staged from its vertices as in mesh3d_surface_dist_kernel.  Block (x, n, z) scans slice z
// GATED: the nearest COMPATIBLE triangle -- the lane's unit normal in three registers, c |c| a scalar; a query with no compatible
// triangle leaves its key all ones.  <ROLE, false> is the scan of the ungated term
template <int ROLE, bool GATED>
__global__ __launch_bounds__(256) void mesh3d_surface_near_kernel(SurfaceTermArgs a) {
  __shared__ ScanTri st[kSurfaceChunk];
  __shared__ float sd[4][kChamQueries];
  __shared__ int si[4][kChamQueries];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nq = ROLE == 0 ? a.V : a.S;
  const float* q = ROLE == 0 ? a.verts + (size_t)n * a.V * 3 : a.points + (size_t)n * a.S * 3;
  const int f0 = ROLE == 0 ? a.t.foff[n] : 0;
  const int nf = ROLE == 0 ? a.t.foff[n + 1] - f0 : a.F;
  const int span = surface_slice_span(nf, (int)gridDim.z);
  const int sb = (int)blockIdx.z * span;
  if (sb >= nf) return;                              // (block-uniform, before any barrier) a smaller mesh of a ragged batch
  const int se = min(sb + span, nf);
  const int* faces = a.faces;
  const float* corners = a.verts + (size_t)n * a.V * 3;
  const float4* recs = reinterpret_cast<const float4*>(a.target_tris + (ROLE == 0 ? f0 : 0));
  const int qi = blockIdx.x * kChamQueries + lane;
  const bool active = qi < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active) {
    qx = q[3 * (size_t)qi];
    qy = q[3 * (size_t)qi + 1];
    qz = q[3 * (size_t)qi + 2];
  }
  float ux = 0.f, uy = 0.f, uz = 0.f;
  const float cc = ROLE == 0 ? a.cc_v : a.cc_p;
  if (GATED && active) {
    const float* u = (ROLE == 0 ? a.normals_v : a.normals_p) + ((size_t)n * nq + qi) * 3;
    ux = u[0];
    uy = u[1];
    uz = u[2];
  }
  float best = INFINITY;
  int bidx = 0x7fffffff;
  for (int base = sb; base < se; base += kSurfaceChunk) {
    const int cnt = min(kSurfaceChunk, se - base);
    __syncthreads();
    if (ROLE == 0) {
      float4* dst = reinterpret_cast<float4*>(st);
      for (int i = threadIdx.x; i < 4 * cnt; i += 256) dst[i] = recs[4 * (size_t)base + i];
    } else {
      for (int i = threadIdx.x; i < cnt; i += 256) {
        const int* fc = faces + 3 * (size_t)(base + i);
        st[i] = make_scan_tri(corners + 3 * (size_t)fc[0], corners + 3 * (size_t)fc[1], corners + 3 * (size_t)fc[2]);
      }
    }
    __syncthreads();
    const Span sp = quarter_span(w, cnt);
    if (GATED) surface_scan_nearest_compatible(qx, qy, qz, ux, uy, uz, cc, st, sp.b, sp.e, base, best, bidx);
    else surface_scan_nearest(qx, qy, qz, st, sp.b, sp.e, base, best, bidx);
  }
  sd[w][lane] = best;
  si[w][lane] = bidx;
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int s = 1; s < 4; ++s) nearest_merge(best, bidx, sd[s][lane], si[s][lane]);
  if (active && bidx != 0x7fffffff) {                // (no finite distance -- NaN input: the key stays all ones)
    unsigned long long* keys = ROLE == 0 ? a.keys_v + (size_t)n * a.V : a.keys_p + (size_t)n * a.S;
    atomicMin(&keys[qi], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)bidx);
  }
}

// one query per thread: the closest point on the face its key names.  GATED: a query is DROPPED when its key is all ones (no
// face, or none compatible), when d^2 > tau^2, or (ROLE 0) by the boundary rule; a dropped query leaves d^2 = 0, a zero residual
// and zero weights -- mesh3d_surface_grad_kernel runs unchanged -- and face -1; the block's kept count goes beside its sum of d^2
// ROBUST: robust_gm on the match's d^2 (the scan's own bits): the block sums rho in place of d^2 and w beside it, and what
// mesh3d_surface_grad_kernel reads (res_v / hits) carries w r, so that kernel runs unchanged; the optional residual outputs
// keep the geometric r, and a dropped query's weight is 0
template <int ROLE, bool GATED, bool ROBUST = false>
__global__ __launch_bounds__(kMeshBlock) void mesh3d_surface_hit_kernel(SurfaceTermArgs a) {
  __shared__ float red[16];
  const int n = blockIdx.y;
  const int nq = ROLE == 0 ? a.V : a.S;
  const int qi = blockIdx.x * kMeshBlock + threadIdx.x;
  float d2 = 0.f;
  int kept = 0;
  float wq = 0.f;   // ROBUST only
  if (qi < nq) {
    const size_t o = (size_t)n * nq + qi;
    const float* q = (ROLE == 0 ? a.verts : a.points) + 3 * o;
    const unsigned long long key = (ROLE == 0 ? a.keys_v : a.keys_p)[o];
    const int f0 = ROLE == 0 ? a.t.foff[n] : 0;
    const int nf = ROLE == 0 ? a.t.foff[n + 1] - f0 : a.F;
    int face = (int)(unsigned)(key & 0xFFFFFFFFull);
    if (key == ~0ull || face >= nf) face = 0;        // no finite distance: stay in bounds
    const int* fc = (ROLE == 0 ? a.t.faces + 3 * (size_t)f0 : a.faces) + 3 * (size_t)face;
    ScanTri tri;
    if (ROLE == 0) {
      tri = a.target_tris[f0 + face];
    } else {
      const float* corners = a.verts + (size_t)n * a.V * 3;
      tri = make_scan_tri(corners + 3 * (size_t)fc[0], corners + 3 * (size_t)fc[1], corners + 3 * (size_t)fc[2]);
    }
    TriHit h;
    if (GATED) {
      const TriHitWhere hw = point_scan_tri_closest_where(q[0], q[1], q[2], tri);
      h = hw.h;
      d2 = __uint_as_float((unsigned)(key >> 32));
      bool keep = key != ~0ull && (int)(unsigned)(key & 0xFFFFFFFFull) < nf;
      keep = keep && !(d2 > (ROLE == 0 ? a.tau2_v : a.tau2_p));
      if (ROLE == 0 && a.bflags != nullptr) keep = keep && !boundary_match(a.bflags[f0 + face], hw.winner, hw.t);
      if (!keep) {
        d2 = 0.f;
        face = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) h.b[k] = h.r[k] = 0.f;
      }
      kept = keep ? 1 : 0;
      unsigned char* ok = ROLE == 0 ? a.vert_kept : a.point_kept;
      if (ok != nullptr) ok[o] = (unsigned char)kept;
    } else {
      h = point_scan_tri_closest(q[0], q[1], q[2], tri);
      d2 = key == ~0ull ? h.d2 : __uint_as_float((unsigned)(key >> 32));   // the scan's own bits
    }
    float wr[3] = {h.r[0], h.r[1], h.r[2]};   // what the gradient gathers: r, ROBUST: w r
    if constexpr (ROBUST) {
      float rho;
      robust_gm(d2, ROLE == 0 ? a.s2_v : a.s2_p, rho, wq);
      d2 = rho;
      if (GATED && kept == 0) wq = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) wr[k] = wq * h.r[k];
      float* ow = ROLE == 0 ? a.vert_w : a.point_w;
      if (ow != nullptr) ow[o] = wq;
    }
    if (ROLE == 0) {
      a.res_v[3 * o] = wr[0];
      a.res_v[3 * o + 1] = wr[1];
      a.res_v[3 * o + 2] = wr[2];
    } else {
      SurfaceHit s;
      s.c0 = fc[0]; s.c1 = fc[1]; s.c2 = fc[2];
      s.b0 = h.b[0]; s.b1 = h.b[1]; s.b2 = h.b[2];
      s.rx = wr[0]; s.ry = wr[1]; s.rz = wr[2];
      s.pad0 = s.pad1 = s.pad2 = 0.f;
      a.hits[o] = s;
    }
    int* of = ROLE == 0 ? a.vert_face : a.point_face;
    float* ob = ROLE == 0 ? a.vert_bary : a.point_bary;
    if (of != nullptr) of[o] = face;
    if (ob != nullptr) {
      ob[3 * o] = h.b[0];
      ob[3 * o + 1] = h.b[1];
      ob[3 * o + 2] = h.b[2];
    }
    float* orr = ROLE == 0 ? a.vert_residual : a.point_residual;
    if (orr != nullptr) {
      orr[3 * o] = h.r[0];
      orr[3 * o + 1] = h.r[1];
      orr[3 * o + 2] = h.r[2];
    }
  }
  const float tot = block_sum(d2, red);
  if (threadIdx.x == 0) (ROLE == 0 ? a.part_vs : a.part_ps)[(size_t)n * gridDim.x + blockIdx.x] = tot;
  if (GATED) {
    const int cnt = __syncthreads_count(kept);      // (an integer count: no order to fix)
    if (threadIdx.x == 0) (ROLE == 0 ? a.part_kv : a.part_kp)[(size_t)n * gridDim.x + blockIdx.x] = cnt;
  }
  if constexpr (ROBUST) {
    const float wtot = block_sum(wq, red);
    if (threadIdx.x == 0) (ROLE == 0 ? a.part_wv : a.part_wp)[(size_t)n * gridDim.x + blockIdx.x] = wtot;
  }
}

// the unit normal of every fitted vertex, one per thread: a gather over its incident faces in ascending face index, no atomics
__global__ __launch_bounds__(kMeshBlock) void mesh3d_vertex_normal_kernel(SurfaceTermArgs a) {
  const int n = blockIdx.y;
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= a.V) return;
  float u[3];
  vertex_normal(a.verts + (size_t)n * a.V * 3, a.faces, a.vf_off, a.vf, v, u);
  float* dst = a.normals_out + ((size_t)n * a.V + v) * 3;
  dst[0] = u[0];
  dst[1] = u[1];
  dst[2] = u[2];
}

// the term's gradient of one vertex in one thread: 2 w_vs / (N V) r_v  -  2 w_ps / (N S) sum over the points whose face has
// this vertex as corner i of b_i r.  64 vertices per block, the staged hits split over its kSurfaceGradWaves waves (as
// mesh3d_chamfer_kernel<1> gathers by owner over 4); the waves' partial sums are added in wave order
constexpr int kGradThreads = 64 * kSurfaceGradWaves;
__global__ __launch_bounds__(kGradThreads) void mesh3d_surface_grad_kernel(SurfaceTermArgs a) {
  __shared__ SurfaceHit sh[kSurfaceHitChunk];
  __shared__ float sg[kSurfaceGradWaves][kChamQueries][3];
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int v = blockIdx.x * kChamQueries + lane;
  const bool active = v < a.V;
  float g[3] = {0.f, 0.f, 0.f};
  if (a.w_ps > 0.f) {
    const float4* src = reinterpret_cast<const float4*>(a.hits + (size_t)n * a.S);
    for (int base = 0; base < a.S; base += kSurfaceHitChunk) {
      const int cnt = min(kSurfaceHitChunk, a.S - base);
      __syncthreads();
      float4* dst = reinterpret_cast<float4*>(sh);
      for (int i = threadIdx.x; i < 3 * cnt; i += kGradThreads) dst[i] = src[3 * (size_t)base + i];
      __syncthreads();
      const int per = (cnt + kSurfaceGradWaves - 1) / kSurfaceGradWaves;
      const int b = min(w * per, cnt), e = min(b + per, cnt);
      surface_hit_gather(sh, b, e, active ? v : -1, g);
    }
  }
  sg[w][lane][0] = g[0];
  sg[w][lane][1] = g[1];
  sg[w][lane][2] = g[2];
  __syncthreads();
  if (w != 0) return;
  const float cps = a.w_ps * 2.0f / ((float)a.S * (float)a.N);
  const float cvs = a.w_vs * 2.0f / ((float)a.V * (float)a.N);
  const size_t o = ((size_t)n * a.V + (active ? v : 0)) * 3;
  float out[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float gp = sg[0][lane][k];
#pragma unroll
    for (int s = 1; s < kSurfaceGradWaves; ++s) gp += sg[s][lane][k];
    const float rv = (active && a.w_vs > 0.f) ? a.res_v[o + k] : 0.f;
    out[k] = active ? cvs * rv - cps * gp : 0.f;
  }
  if (active) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.acc_dverts != nullptr) a.acc_dverts[o + k] += out[k];     // (this thread alone writes the vertex)
      if (a.acc_planar != nullptr) a.acc_planar[((size_t)n * 3 + k) * a.Vp + v] += out[k];
      if (a.dverts != nullptr) a.dverts[o + k] = out[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float t = wave_sum(out[k]);
    if (lane == 0) a.part_dtr[((size_t)n * a.gv + blockIdx.x) * 3 + k] = t;
  }
}

// one block: per mesh the sums of d^2, the two means and the weighted term (every sum in a fixed order); d term / d trans
__global__ __launch_bounds__(256) void mesh3d_surface_reduce_kernel(SurfaceTermArgs a) {
  __shared__ float red[16];
  // a mesh per thread: its few per-block sums one after the other; then the meshes thread-strided and the tree of block_sum
  float tp = 0.f, tv = 0.f;
  for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
    float sp = 0.f, sv = 0.f;
    if (a.w_ps > 0.f)
      for (int b = 0; b < a.hp; ++b) sp += a.part_ps[(size_t)n * a.hp + b];
    if (a.w_vs > 0.f)
      for (int b = 0; b < a.hv; ++b) sv += a.part_vs[(size_t)n * a.hv + b];
    tp += sp;
    tv += sv;
    if (a.rows != nullptr) {
      a.rows[2 * n] = sp;
      a.rows[2 * n + 1] = sv;
    }
    if (a.kept != nullptr || a.weight_sums != nullptr)
      write_direction_totals(a.kept, a.weight_sums, n, direction_totals(a.part_kp, a.part_wp, n, a.hp, a.w_ps > 0.f, a.S),
                             direction_totals(a.part_kv, a.part_wv, n, a.hv, a.w_vs > 0.f, a.V));
  }
  tp = block_sum(tp, red);
  tv = block_sum(tv, red);
  if (threadIdx.x == 0) {
    const float lps = a.w_ps > 0.f ? tp / ((float)a.S * (float)a.N) : 0.f;
    const float lvs = a.w_vs > 0.f ? tv / ((float)a.V * (float)a.N) : 0.f;
    a.losses[0] = lps;
    a.losses[1] = lvs;
    const float term = a.w_ps * lps + a.w_vs * lvs;
    a.losses[2] = term;
    if (a.step_total != nullptr && a.step_losses != nullptr) *a.step_total = a.step_losses[4] + term;   // (mesh3d_reduce_kernel ran before)
  }
  if (a.dtrans != nullptr || a.acc_dtrans != nullptr) {
    for (int o = threadIdx.x; o < 3 * a.N; o += blockDim.x) {
      const int n = o / 3, k = o % 3;
      float s = 0.f;
      for (int b = 0; b < a.gv; ++b) s += a.part_dtr[((size_t)n * a.gv + b) * 3 + k];
      if (a.dtrans != nullptr) a.dtrans[o] = s;
      if (a.acc_dtrans != nullptr) a.acc_dtrans[o] += s;
    }
  }
}

// ---- the scan index: the vertex direction over a grid of the target (mesh3d_grid.h) ---------------------------------------------
// Targets that carry an index (smalfit_mesh_targets_build_index) send mesh3d_surface_near_kernel<0, .> and
// mesh3d_surface_dist_kernel<0> through the two kernels below instead; everything downstream reads the same key / the same
// distance.  One WAVE per query, kScanGridQueries queries a block, grid (ceil(V / 4), N); no LDS, no barrier: a wave's loops are
// its own.  grid_nearest: the oversize list, then ring after ring of cells round the query's own -- the lanes take a ring's cells
// 64 at a time and read their CSR offsets, an inclusive prefix sum over the wave (shuffles) turns the 64 counts into one
// candidate list, the lanes stride over it, each finding its owner cell by a 6-step search in the prefix row (held in registers,
// read by lane index) and gathering its record as four 16-byte loads -- until scan_walk_done, or the whole grid is seen, or
// scan_max_rings(faces) rings are: then the whole record array, lane-strided.  The pair arithmetic is point_scan_tri_dist2 /
// normal_compatible on the linear scan's records; candidates meet by scan_take in a lane and nearest_merge across lanes: the
// lexicographic (d^2, face) minimum, whatever order they came in and however often
struct ScanIndexDev {
  const ScanGrid* grids;     // [N]
  const int* cell_off;       // every mesh's [cells + 1], absolute offsets into cell_face
  const int* cell_face;
  const int* oversize;
};
struct SurfaceGridArgs {
  int N, V;
  const float* verts;            // [N][V][3]
  MeshTargetsDev t;
  const ScanTri* target_tris;    // packed [sum F] (near: the records the linear scan reads)
  ScanIndexDev ix;
  unsigned long long* keys_v;    // [N][V] (near)
  const float* normals_v;        // [N][V][3] (near<true>)
  float cc_v, tau2_v;
  float* vert_dist;              // [N][V] (dist)
};
struct NearestFace { float d2; int face; };

// BUILD: the record is formed from the target's corners as mesh3d_surface_dist_kernel<0> stages it (make_scan_tri on the device;
// the empty asm keeps its values apart from their use, as the trip through LDS does there); else the staged record is loaded
template <bool BUILD>
__device__ __forceinline__ ScanTri grid_record(const float4* recs, const int* faces, const float* corners, int f) {
  ScanTri t;
  if constexpr (BUILD) {
    const int* fc = faces + 3 * (size_t)f;
    t = make_scan_tri(corners + 3 * (size_t)fc[0], corners + 3 * (size_t)fc[1], corners + 3 * (size_t)fc[2]);
    float* w = reinterpret_cast<float*>(&t);
#pragma unroll
    for (int k = 0; k < 16; ++k) asm volatile("" : "+v"(w[k]));
  } else {
    float4* d = reinterpret_cast<float4*>(&t);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = recs[4 * (size_t)f + k];
  }
  return t;
}

template <bool GATED, bool BUILD>
__device__ __forceinline__ NearestFace grid_nearest(const ScanGrid& g, const ScanIndexDev& ix, const float4* recs, const int* faces,
                                                    const float* corners, int nf, float qx, float qy, float qz, float ux, float uy,
                                                    float uz, float cc, float tau2, int lane) {
  float best = INFINITY;
  int face = kScanNoFace;
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) return NearestFace{best, face};   // (wave-uniform) no key, as the linear scan
  auto test = [&](int f) {
    const ScanTri t = grid_record<BUILD>(recs, faces, corners, f);
    const float d2 = point_scan_tri_dist2(qx, qy, qz, t);
    bool ok = true;
    if constexpr (GATED) ok = normal_compatible(ux, uy, uz, t.nx, t.ny, t.nz, t.inv_nn, cc);
    if (ok) scan_take(best, face, d2, f);
  };
  for (int i = lane; i < g.over_count; i += 64) test(ix.oversize[g.over_base + i]);
  const float L = scan_extent(g, qx, qy, qz), slack = scan_slack(L), box = scan_box_dist(g, qx, qy, qz, L);
  const int c[3] = {scan_cell(qx, g.lo[0], g.inv_h, g.dims[0]), scan_cell(qy, g.lo[1], g.inv_h, g.dims[1]),
                    scan_cell(qz, g.lo[2], g.inv_h, g.dims[2])};
  const int* cell_off = ix.cell_off + g.cell_base;
  bool done = false;
  const int last = scan_max_rings(nf);
#pragma unroll 1
  for (int r = 0; r <= last; ++r) {
    const ScanRing ring = scan_ring_boxes(g, c, r);
    const int total = ring.start[6];
#pragma unroll 1
    for (int base = 0; base < total; base += 64) {
      const int i = base + lane;
      const int ci = scan_ring_cell(g, ring, min(i, total - 1));
      int start = 0, cnt = 0;
      if (i < total) {
        start = cell_off[ci];
        cnt = cell_off[ci + 1] - start;
      }
      int inc = cnt;   // inclusive prefix sum of the 64 counts
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      const int excl = inc - cnt;
      const int T = __builtin_amdgcn_readfirstlane(__shfl(inc, 63, 64));
#pragma unroll 1
      for (int jb = 0; jb < T; jb += 64) {
        const int j = jb + lane, jj = min(j, T - 1);
        int lo = 0, hi = 63;   // the first lane whose inclusive sum exceeds jj owns candidate jj
#pragma unroll
        for (int s = 0; s < 6; ++s) {
          const int mid = (lo + hi) >> 1;
          const bool left = __shfl(inc, mid, 64) > jj;
          hi = left ? mid : hi;
          lo = left ? lo : mid + 1;
        }
        const int f = ix.cell_face[__shfl(start, lo, 64) + (jj - __shfl(excl, lo, 64))];
        if (j < T) test(f);
      }
    }
    const ScanBlock b = scan_block(g, c, r);
    if (scan_block_whole(g, b)) {
      done = true;
      break;
    }
    float wbest = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wbest = fminf(wbest, __shfl_xor(wbest, o, 64));
    const float bound = fmaxf(scan_ring_bound(g, b, qx, qy, qz, L), box);
    if (scan_walk_done(wbest, bound, slack, tau2)) {
      done = true;
      break;
    }
  }
  if (!done)
    for (int f = lane; f < nf; f += 64) test(f);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float od = __shfl_xor(best, o, 64);
    const int of = __shfl_xor(face, o, 64);
    nearest_merge(best, face, od, of);
  }
  return NearestFace{best, face};
}

// ROLE 0 of mesh3d_surface_near_kernel over the index: the same key into keys_v (atomicMin on the all-ones key the memset left:
// the memset and the hit kernel do not change).  A walk that tau2_v ended early, or whose best is above tau2_v, writes none
template <bool GATED>
__global__ __launch_bounds__(64 * kScanGridQueries) void mesh3d_surface_near_grid_kernel(SurfaceGridArgs a) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int qi = blockIdx.x * kScanGridQueries + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (qi >= a.V) return;
  const size_t o = (size_t)n * a.V + qi;
  const float qx = a.verts[3 * o], qy = a.verts[3 * o + 1], qz = a.verts[3 * o + 2];
  float ux = 0.f, uy = 0.f, uz = 0.f;
  if constexpr (GATED) {
    ux = a.normals_v[3 * o];
    uy = a.normals_v[3 * o + 1];
    uz = a.normals_v[3 * o + 2];
  }
  const int f0 = a.t.foff[n], nf = a.t.foff[n + 1] - f0;
  const ScanGrid g = a.ix.grids[n];
  const NearestFace h = grid_nearest<GATED, false>(g, a.ix, reinterpret_cast<const float4*>(a.target_tris + f0), nullptr, nullptr, nf, qx,
                                                   qy, qz, ux, uy, uz, a.cc_v, a.tau2_v, lane);
  if (lane == 0 && scan_key_written(h.d2, h.face, a.tau2_v))
    atomicMin(&a.keys_v[o], ((unsigned long long)__float_as_uint(h.d2) << 32) | (unsigned)h.face);
}

// mesh3d_surface_dist_kernel<0> over the index: vert_dist = sqrt(least d^2), the records formed as that kernel forms them
__global__ __launch_bounds__(64 * kScanGridQueries) void mesh3d_surface_dist_grid_kernel(SurfaceGridArgs a) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int qi = blockIdx.x * kScanGridQueries + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (qi >= a.V) return;
  const size_t o = (size_t)n * a.V + qi;
  const float qx = a.verts[3 * o], qy = a.verts[3 * o + 1], qz = a.verts[3 * o + 2];
  const int f0 = a.t.foff[n], nf = a.t.foff[n + 1] - f0;
  const ScanGrid g = a.ix.grids[n];
  const NearestFace h = grid_nearest<false, true>(g, a.ix, nullptr, a.t.faces + 3 * (size_t)f0, a.t.verts + 3 * (size_t)a.t.voff[n], nf,
                                                  qx, qy, qz, 0.f, 0.f, 0.f, 0.f, INFINITY, lane);
  if (lane == 0) a.vert_dist[o] = sqrtf(h.d2);
}

// ---- the scan-sequence block: one shape per clip, temporal smoothness ---------------------------------------------------
// One launch between the betas assembly and Adam (include/smalfit.h, "scan sequences"; the arithmetic is fit3d_sequence_math.h,
// the grid sequence_blocks of smalfit_plan.h).  The sizes are tiny (N <= the engine's max_frames, 105 + 3 + num_betas columns): the
// launch is latency, not bandwidth.  No atomics.  Block 0 sums the three losses in a fixed order; behind it one thread owns one
// output element: thread (clip, column) of the shape sum reads all of its clip's rows before it writes any of them, thread
// (mesh, element) of a temporal gradient reads parameters, which Adam has not touched yet, and its own gradient element.
struct Fit3dSequenceArgs {
  int N, G, nb;
  const int* clip_start;    // [G]
  const int* clip_len;      // [G]
  const int* mesh_start;    // [N] first mesh of the clip of mesh n
  const int* mesh_len;      // [N] length of that clip
  const float* global_rot;  // [N][3]    read only while its term is on
  const float* joint_rot;   // [N][102]
  const float* trans;       // [N][3]
  float* g_betas;           // [N][nb]; read only when nshape > 0
  float* g_theta;           // [N][105]; read only with add_global | add_joint
  float* g_trans;           // [N][3]; read only with add_trans
  int nshape;               // G nb when the shape sum runs, else 0
  bool joint, global, trans_on;              // the term is evaluated (its weight > 0)
  bool add_joint, add_global, add_trans;     // ... and its gradient added
  float w_joint, w_global, w_trans;
  float c_joint, c_global, c_trans;          // temporal_grad_scale
  float* losses;            // [4]
  const float* base_total;     // the step's weighted total, or null
  const float* surface_total;  // the surface term's, or null
  float* step_total;           // [1] or null
  // a step with the vertex terms on (smalfit_scan_sequence_vertex_step), else both null: their sum, which
  // fit3d_sequence_vertex_finish_kernel has written, and where the vertex block's step_total goes
  const float* vertex_total;
  float* vertex_step_total;
};

// S of one term: lane l takes the elements l, l + 256, ... in ascending order, then the block's fixed-order sum
__device__ __forceinline__ float sequence_term_sum(const float* x, int L, const Fit3dSequenceArgs& a, float* red) {
  float s = 0.f;
  const int count = a.N * L;
  for (int i = threadIdx.x; i < count; i += kSeqBlock) {
    const int n = i / L;
    if (n + 1 < a.mesh_start[n] + a.mesh_len[n]) s = temporal_pair_sq(s, x[i], x[i + L]);
  }
  return block_sum(s, red);
}

__global__ __launch_bounds__(kSeqBlock) void fit3d_sequence_kernel(Fit3dSequenceArgs a) {
  if (blockIdx.x == 0) {
    __shared__ float red[16];
    const float sj = a.joint ? sequence_term_sum(a.joint_rot, kSeqJointLen, a, red) : 0.f;
    const float sg = a.global ? sequence_term_sum(a.global_rot, kSeqGlobalLen, a, red) : 0.f;
    const float st = a.trans_on ? sequence_term_sum(a.trans, kSeqTransLen, a, red) : 0.f;
    if (threadIdx.x == 0) {
      const float lj = a.joint ? temporal_loss(a.w_joint, sj, kSeqJointLen) : 0.f;
      const float lg = a.global ? temporal_loss(a.w_global, sg, kSeqGlobalLen) : 0.f;
      const float lt = a.trans_on ? temporal_loss(a.w_trans, st, kSeqTransLen) : 0.f;
      const float tot = temporal_total(lj, lg, lt);
      a.losses[0] = lj;
      a.losses[1] = lg;
      a.losses[2] = lt;
      a.losses[3] = tot;
      if (a.step_total != nullptr) {
        float base = a.base_total[0];
        if (a.surface_total != nullptr) base += a.surface_total[0];
        a.step_total[0] = base + tot;
      }
      if (a.vertex_step_total != nullptr) {
        float base = a.base_total[0];
        if (a.surface_total != nullptr) base += a.surface_total[0];
        a.vertex_step_total[0] = vertex_step_total(base, tot, a.vertex_total[0]);
      }
    }
    return;
  }
  const int i = ((int)blockIdx.x - 1) * kSeqBlock + (int)threadIdx.x;
  if (i < a.nshape) {
    const int c = i / a.nb, col = i - c * a.nb;
    const int start = a.clip_start[c], len = a.clip_len[c];
    if (len < 2) return;
    const float s = sequence_row_sum(a.g_betas, a.nb, col, start, len);
    for (int r = 0; r < len; ++r) a.g_betas[(size_t)(start + r) * a.nb + col] = s;
    return;
  }
  const int j = i - a.nshape;
  if (j >= a.N * kSeqGradCols) return;
  const int n = j / kSeqGradCols, k = j - n * kSeqGradCols;
  const int start = a.mesh_start[n], len = a.mesh_len[n];
  if (len < 2) return;
  const bool has_prev = n > start, has_next = n + 1 < start + len;
  float* g;
  const float* x;
  int L;
  float c;
  if (k < kSeqGlobalLen) {
    if (!a.add_global) return;
    g = a.g_theta + (size_t)n * kSeqThetaCols + k; x = a.global_rot + (size_t)n * kSeqGlobalLen + k; L = kSeqGlobalLen; c = a.c_global;
  } else if (k < kSeqThetaCols) {
    if (!a.add_joint) return;
    g = a.g_theta + (size_t)n * kSeqThetaCols + k; x = a.joint_rot + (size_t)n * kSeqJointLen + (k - kSeqGlobalLen); L = kSeqJointLen; c = a.c_joint;
  } else {
    if (!a.add_trans) return;
    g = a.g_trans + (size_t)n * kSeqTransLen + (k - kSeqThetaCols); x = a.trans + (size_t)n * kSeqTransLen + (k - kSeqThetaCols); L = kSeqTransLen; c = a.c_trans;
  }
  const float prev = has_prev ? x[-L] : 0.f, next = has_next ? x[L] : 0.f;
  *g = temporal_grad(*g, c, *x, prev, next, has_prev, has_next);
}

// ---- the temporal terms on posed vertices: velocity and acceleration --------------------------------------------------------
// Two launches between the surface term and the LBS adjoint (include/smalfit.h, "scan sequences", the vertex terms; the arithmetic
// is fit3d_sequence_vertex_math.h, the grid sequence_vertex_grid of smalfit_plan.h).  No atomics.  Thread (n, v) owns vertex v of
// mesh n and its three coordinates: it reads x of up to five meshes of its clip (N V 3 floats are 1.5 MB at 32 meshes: the
// neighbours' reads hit L2), forms t and adds it where the gradient is read from; mesh n owns the velocity pair (n, n + 1), a
// centre owns its acceleration triple.  block_sum leaves the block's five partials; the one-block finish kernel adds them in a
// fixed order.
struct Fit3dSequenceVertexArgs {
  int N, V, Vp, blocks;     // blocks: of one mesh's row
  const int* mesh_start;    // [N] first mesh of the clip of mesh n
  const int* mesh_len;      // [N] length of that clip
  const float* verts;       // [N][V][3]
  bool vel, acc;            // the term is evaluated
  float w_vel, w_acc;
  float c_vel, c_acc;       // temporal_grad_scale; 0 for a term that is not evaluated
  float* acc_dverts;        // [N][V][3] or null: t is added to it ...
  float* acc_planar;        // [N][3][Vp] or null: ... and to the planar copy for the LBS adjoint (padding stays untouched)
  float* dverts;            // [N][V][3] or null: t is written (the stand-alone call)
  float* parts;             // [kSeqVertexSums][N][blocks]: S_vel, S_acc, the three columns of d trans
  // the finish kernel only
  float* acc_dtrans;        // [N][3] or null: the sum of t over a mesh is added to it
  float* dtrans;            // [N][3] or null: ... is written
  float* losses;            // [3]
  const float* base_total;     // the step's weighted total, or null
  const float* surface_total;  // the surface term's, or null
  float* step_total;           // [1] or null: formed here when fit3d_sequence_kernel does not run behind this
};

__global__ __launch_bounds__(kSeqVertexBlock) void fit3d_sequence_vertex_kernel(Fit3dSequenceVertexArgs a) {
  __shared__ float red[16];
  const int n = blockIdx.y;
  const int v = blockIdx.x * kSeqVertexBlock + (int)threadIdx.x;
  const bool active = v < a.V;
  const SeqVertexPlace p = sequence_vertex_place(n, a.mesh_start[n], a.mesh_len[n]);
  const size_t stride = (size_t)a.V * 3;
  const size_t o = ((size_t)n * a.V + (active ? v : 0)) * 3;
  float t[3] = {0.f, 0.f, 0.f};
  float sv = 0.f, sa = 0.f;
  if (active) {
    const float* x0 = a.verts + o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = x0[k];
      // (a frame is read only where the clip holds it; with only the velocity term on, only the two nearest)
      const float xm1 = p.has_m1 ? x0[k - (ptrdiff_t)stride] : 0.f;
      const float xp1 = p.has_p1 ? x0[k + stride] : 0.f;
      float D = 0.f, A = 0.f;
      if (a.vel) {
        D = vertex_vel_stencil(x, xm1, xp1, p.has_m1, p.has_p1);
        if (p.has_p1) sv = temporal_pair_sq(sv, x, xp1);
      }
      if (a.acc) {
        const float xm2 = p.has_m2 ? x0[k - 2 * (ptrdiff_t)stride] : 0.f;
        const float xp2 = p.has_p2 ? x0[k + 2 * stride] : 0.f;
        A = vertex_acc_stencil5(p, xm2, xm1, x, xp1, xp2);
        if (p.centre_0) sa = vertex_accel_sq(sa, vertex_accel(xm1, x, xp1));
      }
      t[k] = vertex_term_grad(a.c_acc, A, a.c_vel, D);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.acc_dverts != nullptr) a.acc_dverts[o + k] += t[k];     // (this thread alone writes the vertex)
      if (a.acc_planar != nullptr) a.acc_planar[((size_t)n * 3 + k) * a.Vp + v] += t[k];
      if (a.dverts != nullptr) a.dverts[o + k] = t[k];
    }
  }
  const float sums[kSeqVertexSums] = {block_sum(sv, red), block_sum(sa, red), block_sum(t[0], red), block_sum(t[1], red),
                                      block_sum(t[2], red)};
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kSeqVertexSums; ++q) a.parts[((size_t)q * a.N + n) * a.blocks + blockIdx.x] = sums[q];
  }
}

// sum q of the partials: ascending mesh order, then ascending block order (one mesh only for the columns of d trans)
__device__ __forceinline__ float sequence_vertex_partial_sum(const Fit3dSequenceVertexArgs& a, int q, int n0, int n1) {
  const float* part = a.parts + (size_t)q * a.N * a.blocks;
  float s = 0.f;
  for (int i = n0 * a.blocks; i < n1 * a.blocks; ++i) s += part[i];
  return s;
}

// one block: lane 0 of wave 0 adds S_vel, lane 0 of wave 1 S_acc, the threads of waves 2 and 3 take the elements of d trans
__global__ __launch_bounds__(kSeqVertexBlock) void fit3d_sequence_vertex_finish_kernel(Fit3dSequenceVertexArgs a) {
  __shared__ float S[2];
  const int tid = (int)threadIdx.x;
  if (tid == 0) S[0] = a.vel ? sequence_vertex_partial_sum(a, 0, 0, a.N) : 0.f;
  if (tid == 64) S[1] = a.acc ? sequence_vertex_partial_sum(a, 1, 0, a.N) : 0.f;
  if (tid >= 128 && (a.dtrans != nullptr || a.acc_dtrans != nullptr)) {
    for (int e = tid - 128; e < 3 * a.N; e += kSeqVertexBlock - 128) {
      const int n = e / 3, k = e - 3 * n;
      const float s = sequence_vertex_partial_sum(a, 2 + k, n, n + 1);
      if (a.dtrans != nullptr) a.dtrans[e] = s;
      if (a.acc_dtrans != nullptr) a.acc_dtrans[e] += s;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  const int L = sequence_vertex_len(a.V);
  const float lv = a.vel ? temporal_loss(a.w_vel, S[0], L) : 0.f;
  const float la = a.acc ? temporal_loss(a.w_acc, S[1], L) : 0.f;
  const float tot = vertex_term_total(lv, la);
  a.losses[0] = lv;
  a.losses[1] = la;
  a.losses[2] = tot;
  if (a.step_total != nullptr) {
    float base = a.base_total[0];
    if (a.surface_total != nullptr) base += a.surface_total[0];
    a.step_total[0] = vertex_step_total(base, 0.f, tot);       // (the parameter terms are off: their sum reads 0)
  }
}

// ---- Adam on all trained parameters of a Stage.step in one launch ----------------------------------------------------
// torch.optim.Adam (adam_update) over the trained parameters, one launch (Fit3dAdamArgs: smalfit_plan.h, beside plan_fit3d, which
// sizes its segments)
__global__ __launch_bounds__(256) void fit3d_adam_kernel(Fit3dAdamArgs a) {
  int s = 0;
  while (s + 1 < a.nseg && (int)blockIdx.x >= a.seg[s + 1].block0) ++s;
  const Fit3dAdamSeg& sg = a.seg[s];
  const int i = ((int)blockIdx.x - sg.block0) * 256 + threadIdx.x;
  if (i >= sg.count) return;
  const int row = i / sg.row_len, col = i - row * sg.row_len;
  const float gi = sg.g[(size_t)row * sg.g_stride + sg.g_offset + col];
  // read in this order (gradient, b1, m, b2, v): the order of the loads decides which product of each moment update the
  // compiler fuses into a multiply-add, and with it the rounding of m and v (b1 = 0.9 in the 3D fitter: neither product
  // is exact); this order keeps the bits this kernel has always produced
  const float b1 = a.b1, m0 = sg.m[i], b2 = a.b2, v0 = sg.v[i];
  adam_update(gi, m0, v0, b1, b2, a.eps, sg.step_size, a.bc2_sqrt, sg.m[i], sg.v[i], sg.p[i]);
}

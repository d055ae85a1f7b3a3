// LBS adjoints, gradient assembly, Adam (K6-K12) -- part of smalfit_kernels.hip (included inside namespace smalfit; not a translation unit of its own)

// ------------------------------------------------------------------------------------------------
// K6: vertex adjoint: gather raster grads of incident faces, camera adjoint, joint-regressor adjoint,
//     skinning adjoint wrt v_posed.   block = 256 vertices of one frame
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vertex_bwd_kernel(ModelDev m, int M, const float* __restrict__ proj, const float* __restrict__ dface,
                  const float* __restrict__ dJ41 /*[M][41][3] or null*/,
                  const float* __restrict__ dverts_ext /*[M][3][Vp] extra world-space adjoint or null*/,
                  const float* __restrict__ Am, float* __restrict__ dvert /*[M][3][Vp]*/,
                  float* __restrict__ dvp /*[M][3][Vp]*/, float* __restrict__ dtr_part /*[VT][M][3]*/) {
  __shared__ float As[420];
  __shared__ float dJs[123];
  __shared__ float red[16];
  const int Vp = m.Vp;
  PHASE_MARK(pv0);
  // Frame -> XCD affinity (round 6, like the rasteriser kernels: workgroups are dealt to the 8 XCDs round-robin by linear id, every XCD
  // has its own L2): with one frame per workgroup and a 1-D grid, frame n runs on XCD n % 8 -- where raster_bwd_kernel left the
  // frame's face adjoints and where lbs_bwd_mid_kernel's dA blocks and chain_bwd_kernel's frame block will read what this kernel writes.
  int n, vblock;
  xcd_block(vertex_blocks(Vp), n, vblock);
  if (n >= M) return;
  const int v = vblock * 256 + threadIdx.x;
  // Round 6: everything whose address depends on the vertex alone -- the range of its incident (face, corner) list and the list's
  // first entries -- is requested BEFORE the transforms are staged and the workgroup meets at the barrier: behind it the chain
  // range -> entries -> face adjoints was three dependent trips to memory on a kernel that is one workgroup's latency.
  constexpr int kPre = 8;                      // incident corners held in registers (a vertex of a closed mesh has ~6)
  const int vc = min(v, m.V - 1);
  const int vf0 = m.vf_off[vc], vf1 = (v < m.V) ? m.vf_off[vc + 1] : vf0;
  int vfi[kPre];
  // (clamped: unconditional loads, see tools/isa_loads.py; an empty list at the end reads the zero entry smalfit_model_create pads vf_idx with)
#pragma unroll
  for (int q = 0; q < kPre; ++q) vfi[q] = m.vf_idx[min(vf0 + q, max(vf1 - 1, vf0))];
  for (int i = threadIdx.x; i < 420; i += 256) As[i] = Am[(size_t)n * 420 + i];
  for (int i = threadIdx.x; i < 123; i += 256) dJs[i] = dJ41 ? dJ41[(size_t)n * 123 + i] : 0.f;
  __syncthreads();
  int lm = -1;
#pragma unroll
  for (int i = 0; i < 6; ++i) if (v == m.landmarks[i]) lm = i;
  const bool live = v < m.V;
  float g[3] = {0.f, 0.f, 0.f};         // adjoint of translated world vertex (raster path)
  if (live && dface) {
    float gxn = 0.f, gyn = 0.f;
    const float2* df = reinterpret_cast<const float2*>(dface + (size_t)n * m.F * 6);     // (x, y) adjoint of every face corner: one 8-byte gather each
    float2 gq[kPre];
#pragma unroll
    for (int q = 0; q < kPre; ++q) gq[q] = df[vfi[q]];                                   // (all in flight together; entries past the list repeat its last)
#pragma unroll
    for (int q = 0; q < kPre; ++q)
      if (vf0 + q < vf1) { gxn += gq[q].x; gyn += gq[q].y; }                             // same order as the list: the same bits
    for (int i = vf0 + kPre; i < vf1; ++i) {
      const float2 g2 = df[m.vf_idx[i]];           // face*3 + corner
      gxn += g2.x;
      gyn += g2.y;
    }
    const float* pv = proj + (size_t)n * 3 * Vp;
    world_to_ndc_bwd(pv[v], pv[Vp + v], pv[2 * Vp + v], gxn, gyn, g[0], g[1], g[2]);
  }
  if (live && dverts_ext) {
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] += dverts_ext[((size_t)n * 3 + a) * Vp + v];
  }
  // translation adjoint: sum over vertices of the translated-vertex adjoint
  {
    const float s0 = wave_sum(live ? g[0] : 0.f), s1 = wave_sum(live ? g[1] : 0.f), s2 = wave_sum(live ? g[2] : 0.f);
    if ((threadIdx.x & 63) == 0) { float* q = &red[(threadIdx.x >> 6) * 4]; q[0] = s0; q[1] = s1; q[2] = s2; }
    __syncthreads();
    if (threadIdx.x < 3)
      dtr_part[((size_t)vblock * M + n) * 3 + threadIdx.x] =
          ((red[threadIdx.x] + red[4 + threadIdx.x]) + red[8 + threadIdx.x]) + red[12 + threadIdx.x];
  }
  // joints = J_regressor^T verts  (+ landmark picks)
  float dv[3] = {g[0], g[1], g[2]};
  if (live) {
#pragma unroll 4
    for (int e = 0; e < m.Kj; ++e) {
      const int j = m.jrv_j[e * Vp + v];
      const float c = m.jrv_val[e * Vp + v];
#pragma unroll
      for (int a = 0; a < 3; ++a) dv[a] = fmaf(c, dJs[j * 3 + a], dv[a]);
    }
    if (lm >= 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) dv[a] += dJs[(35 + lm) * 3 + a];
    }
  }
  // skinning: vert = T.R vp + T.t  ->  dvp = T.R^T dv
  float T[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) T[e] = 0.f;
  if (live) {
#pragma unroll 4
    for (int e = 0; e < m.Kw; ++e) {
      const int j = m.w_j[e * Vp + v];
      const float wv = m.w_val[e * Vp + v];
      const float* A = &As[j * 12];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) T[a * 3 + b] = fmaf(wv, A[a * 4 + b], T[a * 3 + b]);
    }
  }
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const float o = T[b] * dv[0] + T[3 + b] * dv[1] + T[6 + b] * dv[2];
    if (v < Vp) {
      dvp[((size_t)n * 3 + b) * Vp + v] = live ? o : 0.f;
      dvert[((size_t)n * 3 + b) * Vp + v] = live ? dv[b] : 0.f;
    }
  }
  PHASE_MARK(pv1);
  PHASE_END(PH_VERTEX_BWD, pv0, pv1);
}

// K7: dA[n][j] = sum over the skin-weight column of joint j of  w * dvert (x) [v_posed; 1]
__device__ __forceinline__ void
dA_block(const ModelDev& m, int j, int n, const float* __restrict__ dvert, const float* __restrict__ vposed,
         float* __restrict__ dA /*[M][35][12]*/, float (*part)[32]) {
  const int Vp = m.Vp;
  const float* dv = dvert + (size_t)n * 3 * Vp;
  const float* vp = vposed + (size_t)n * 3 * Vp;
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 2
  for (int i = m.wc_off[j] + threadIdx.x; i < m.wc_off[j + 1]; i += 256) {
    const int v = m.wc_v[i];
    const float wv = m.wc_val[i];
    const float p[4] = {vp[v], vp[Vp + v], vp[2 * Vp + v], 1.0f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float d = wv * dv[a * Vp + v];
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a * 4 + b] = fmaf(d, p[b], acc[a * 4 + b]);
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float tot = wave_sums<16>(acc, lane);           // value lane >> 2
  if ((lane & 3) == 0) part[w][lane >> 2] = tot;
  __syncthreads();
  if (threadIdx.x < 12)
    dA[((size_t)n * 35 + j) * 12 + threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// (kAsmElem, kAsmLoss, kAsmRows: the block roles of assemble_kernel and frame_loss_rows_kernel, smalfit_plan.h)

// K9: shape-blend adjoint.  shared betas: dbeta_part[block][b] = sum_col sd[b][col] * sum_n dvp[n][col]
//     per-frame betas (blockIdx.y = frame): no sum over frames.
__device__ __forceinline__ void
dbeta_block(const ModelDev& m, int M, int nb, int shared, int bx, int by, int bz, int gx, int gzn,
            const float* __restrict__ dvp, float* __restrict__ dbeta_part /*[nbs][gzn * gx][nb]*/, float (*part)[32]) {
  const int ncol = 3 * m.Vp;
  const int c = bx * 256 + threadIdx.x;
  float g = 0.f;
  if (c < ncol) {
    if (shared) {       // frames are split over bz
      const int per = (M + gzn - 1) / gzn;
      const int n0 = bz * per, n1 = min(M, n0 + per);
      // (summed in double, rounded once: the frames' adjoints of one column largely cancel in a fit that has settled -- round 6, with
      // the assembly's sums below, which measured no different from float32 sums)
      double gd = 0.0;
#pragma unroll 8
      for (int n = n0; n < n1; ++n) gd += (double)dvp[(size_t)n * ncol + c];
      g = (float)gd;
    } else {
      g = dvp[(size_t)by * ncol + c];
    }
  }
  const size_t pidx = (size_t)by * gzn * gx + (size_t)bz * gx + bx;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b0 = 0; b0 < nb; b0 += 32) {                 // shape directions in groups of 32
    // the 32 basis values are loaded unconditionally from clamped indices and masked afterwards: as conditional loads the
    // compiler kept 32 branches with an s_waitcnt vmcnt(0) behind every load -- 32 dependent trips to memory per block
    // (tools/isa_loads.py), which is what the launch these blocks ride in was waiting for
    float val[32];
    const int cc = min(c, ncol - 1);
#pragma unroll
    for (int b = 0; b < 32; ++b) val[b] = m.sd[(size_t)min(b0 + b, nb - 1) * ncol + cc];
#pragma unroll
    for (int b = 0; b < 32; ++b) val[b] = (c < ncol && b0 + b < nb) ? g * val[b] : 0.f;
    const float tot = wave_sums<32>(val, lane);         // value lane >> 1
    __syncthreads();
    if ((lane & 1) == 0) part[w][lane >> 1] = tot;
    __syncthreads();
    if (threadIdx.x < 32 && b0 + threadIdx.x < nb)
      dbeta_part[pidx * nb + b0 + threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
  }
}

// pose-blend adjoint on the matrix cores:  dpf[n][k] = sum_c dvp[n][c] * pd[k][c]  (c: the 3 Vp columns).
// A block owns 32 pose features, one of PBM_SPLITS column ranges and up to PBM_TILES tiles of 16 frames; its four waves take a
// quarter of the range each and their tiles are added through LDS in a fixed order.  Both operands are rows of length 3 Vp, so
// a lane fetches FOUR consecutive columns (one 16-byte load; 16 rows x 64 bytes per instruction) and the four
// v_mfma_f32_16x16x4_f32 that follow pair component i of A with component i of B: the instruction only needs A and B
// to agree on which column sits in which k slot.
// Round 3: the slice of the basis (B) a block fetches is used for ALL its frame tiles -- four tiles of 16 frames at 64 frames, so
// `posedirs` is read once per evaluation instead of once per tile (round 2: 119 MB counted for a 14.3 MB basis) -- and the
// column range is a quarter as long instead (24 splits instead of 6: the same number of blocks, the same number of matrix
// instructions per wave, a quarter of the B loads and half the dependent load batches).
constexpr int PBM_U = 2;   // (PBM_SPLITS, PBM_TILES: smalfit_plan.h)
__device__ __forceinline__ void
poseblend_bwd_mfma_block(const ModelDev& m, int M, int tchunk, int kpair, int split, const float* __restrict__ dvp,
                         float* __restrict__ dpf_part /*[PBM_SPLITS][M][308]*/, float (*red)[8][64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ncol = 3 * m.Vp, nsteps = ncol / 16;            // Vp is a multiple of 64
  const int per = (nsteps + PBM_SPLITS * 4 - 1) / (PBM_SPLITS * 4);
  const int s_beg = (split * 4 + w) * per, s_end = min(nsteps, s_beg + per);
  const int nft = (M + 15) / 16, t0 = tchunk * PBM_TILES, nt = min(PBM_TILES, nft - t0);   // uniform over the block
  const int k0 = kpair * 32;
  const int row = lane & 15, cq = (lane >> 4) * 4;
  const float4* pa[PBM_TILES];
#pragma unroll
  for (int t = 0; t < PBM_TILES; ++t)
    pa[t] = reinterpret_cast<const float4*>(dvp + (size_t)min((t0 + t) * 16 + row, M - 1) * ncol + cq);
  const float4* pb0 = reinterpret_cast<const float4*>(m.pd + (size_t)min(k0 + row, 305) * ncol + cq);
  const float4* pb1 = reinterpret_cast<const float4*>(m.pd + (size_t)min(k0 + 16 + row, 305) * ncol + cq);
  f32x4 acc0[PBM_TILES], acc1[PBM_TILES];
#pragma unroll
  for (int t = 0; t < PBM_TILES; ++t) { acc0[t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[t] = acc0[t]; }
  for (int st0 = s_beg; st0 < s_end; st0 += PBM_U) {
    float4 B0[PBM_U], B1[PBM_U], A[PBM_TILES][PBM_U];
#pragma unroll
    for (int u = 0; u < PBM_U; ++u) {
      const int st = min(st0 + u, nsteps - 1);               // past the end: a valid address, zeroed below
      B0[u] = pb0[st * 4]; B1[u] = pb1[st * 4];
#pragma unroll
      for (int t = 0; t < PBM_TILES; ++t) {
        A[t][u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < nt && st0 + u < s_end) A[t][u] = pa[t][st * 4];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < PBM_U; ++u) {
#pragma unroll
      for (int t = 0; t < PBM_TILES; ++t) {
        if (t < nt) {
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].x, B0[u].x, acc0[t], 0, 0, 0);
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].x, B1[u].x, acc1[t], 0, 0, 0);
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].y, B0[u].y, acc0[t], 0, 0, 0);
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].y, B1[u].y, acc1[t], 0, 0, 0);
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].z, B0[u].z, acc0[t], 0, 0, 0);
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].z, B1[u].z, acc1[t], 0, 0, 0);
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].w, B0[u].w, acc0[t], 0, 0, 0);
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[t][u].w, B1[u].w, acc1[t], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // D[row = 4 (lane >> 4) + r][col = lane & 15]; wave t finishes registers 2t, 2t+1 of the eight; one tile at a time
#pragma unroll
  for (int t = 0; t < PBM_TILES; ++t) {
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { red[w][r][lane] = acc0[t][r]; red[w][4 + r][lane] = acc1[t][r]; }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int reg = w * 2 + q, r = reg & 3, tile = reg >> 2;
        const float tot = ((red[0][reg][lane] + red[1][reg][lane]) + red[2][reg][lane]) + red[3][reg][lane];
        const int n = (t0 + t) * 16 + 4 * (lane >> 4) + r, k = k0 + tile * 16 + (lane & 15);
        if (n < M && k < 306) dpf_part[((size_t)split * M + n) * 308 + k] = tot;
      }
      __syncthreads();
    }
  }
}

// everything between the vertex adjoint and the chain adjoint in ONE launch (the parts are independent and each is
// latency-bound on its own): the pose-blend adjoint (4 waves = 4 tiles per block), then 35 x M blocks dA_j.  (The shape-blend
// adjoint partials ride on chain_bwd_kernel.)
// Block -> XCD placement of the pose-blend part (round 3).  Workgroups are dealt to the 8 XCDs round-robin by linear id and
// every XCD has its own L2.  The 10 feature-pair blocks of one column split read the same columns of dvp (A): their ids are
// laid out as chunks of 8 splits x 10 feature pairs with the split in the low 3 bits, so they share an XCD and that slice of
// dvp is fetched once; every element of `posedirs` (B) is fetched by exactly one block per chunk of PBM_TILES frame tiles.
// Speed only: results never depend on the placement.
// (mid_pb_ids, mid_da_ids, mid_grid: smalfit_plan.h)
__global__ void __launch_bounds__(256, 4)      // <= 128 registers (vector + accumulation): four workgroups per CU for the 35 M dA blocks
lbs_bwd_mid_kernel(ModelDev m, int M, int nPB, const float* __restrict__ dvert, const float* __restrict__ vposed,
                   const float* __restrict__ dvp, float* __restrict__ dA, float* __restrict__ dpf_part) {
  __shared__ float part[4][32];
  __shared__ float tile_red[4][8][64];
  int blk = blockIdx.x;
  if (nPB > 0) {
    const int ids = mid_pb_ids(M);
    if (blk < ids) {
      PHASE_MARK(pm0);
      const int tchunk = blk / (10 * PBM_SPLITS), r = blk - tchunk * (10 * PBM_SPLITS);
      const int chunk = r / 80, q = r - chunk * 80;
      poseblend_bwd_mfma_block(m, M, tchunk, q >> 3, chunk * 8 + (q & 7), dvp, dpf_part, tile_red);
      PHASE_MARK(pm1);
      PHASE_END(PH_MID_PB, pm0, pm1);
      return;
    }
    blk -= ids;
  }
  PHASE_MARK(pd0);
  int n, j;
  xcd_block_of(blk, 35, n, j);            // (the pose-blend ids before these are a multiple of 8: blk % 8 is the workgroup's XCD)
  if (n >= M) return;
  dA_block(m, j, n, dvert, vposed, dA, part);
  PHASE_MARK(pd1); PHASE_END(PH_MID_DA, pd0, pd1);
}

// The chain adjoint's work on joint i with parent p, lane e of the joint's 12, in two steps with a wave barrier between them
// (step 1 reads the dR' / dj of all the joint's lanes).  Both tree walks of chain_bwd_kernel call it; the LDS arrays are the kernel's.
struct ChainLds {
  const float (*R)[9], (*G)[12], (*sc)[3], (*isc)[3], (*J)[3], (*dG)[12];
  float (*dR)[9], (*cG)[12], (*cJ)[3], (*cS)[3], (*sOwn)[3], (*dRp)[9], (*djv)[3];
};
template <int kStep>
__device__ __forceinline__ void chain_joint_adjoint(const ChainLds& s, int i, int p, int e) {
  const auto R = s.R; const auto G = s.G; const auto sc = s.sc; const auto isc = s.isc; const auto J = s.J; const auto dG = s.dG;
  const auto dRp = s.dRp; const auto djv = s.djv;
  if constexpr (kStep == 0) {
    // dR' = G_p.R^T dG_i.R ; dj = G_p.R^T dG_i.t
    if (e < 9) {
      const int a = e / 3, b = e % 3;
      dRp[i][e] = G[p][0 * 4 + a] * dG[i][0 * 4 + b] + G[p][1 * 4 + a] * dG[i][1 * 4 + b] + G[p][2 * 4 + a] * dG[i][2 * 4 + b];
    } else {
      const int a = e - 9;
      djv[i][a] = G[p][0 * 4 + a] * dG[i][3] + G[p][1 * 4 + a] * dG[i][7] + G[p][2 * 4 + a] * dG[i][11];
    }
  } else if (e < 9) {
    const int a = e / 3, c = e % 3;
    // owed to dG_p.R[a][c]: sum_b dG_i.R[a][b] R'[c][b] + dG_i.t[a] (J_i - J_p)[c]
    float acc = dG[i][a * 4 + 3] * (J[i][c] - J[p][c]);
#pragma unroll
    for (int b = 0; b < 3; ++b) acc = fmaf(dG[i][a * 4 + b], R[i][c * 3 + b] * sc[i][b] * isc[p][c], acc);
    s.cG[i][a * 4 + c] = acc;
    // dR_i[a][c] += dR'[a][c] s_i[c] / s_p[a]
    s.dR[i][a * 3 + c] += dRp[i][a * 3 + c] * sc[i][c] * isc[p][a];
  } else {
    const int a = e - 9;
    s.cG[i][a * 4 + 3] = dG[i][a * 4 + 3];
    s.cJ[i][a] = djv[i][a];                          // dJ_i += dj, dJ_p -= dj (applied after the walk)
    {                                                // ds_i[b] += sum_a dR'[a][b] R_i[a][b] / s_p[a]   (b = a here)
      const int b = a;
      float acc = 0.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) acc = fmaf(dRp[i][r * 3 + b], R[i][r * 3 + b] * isc[p][r], acc);
      s.sOwn[i][b] = acc;
    }
    {                                                // ds_p[a] -= sum_b dR'[a][b] R'[a][b] / s_p[a]
      float acc = 0.f;
#pragma unroll
      for (int b = 0; b < 3; ++b) acc = fmaf(dRp[i][a * 3 + b], R[i][a * 3 + b] * sc[i][b] * isc[p][a], acc);
      s.cS[i][a] = acc * isc[p][a];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// K10: per-frame chain adjoint: dA, dpf -> d theta, d logscale, d rest joints
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
chain_bwd_kernel(ModelDev m, int M, const float* __restrict__ theta, const float* __restrict__ Rm,
                 const float* __restrict__ Gm, const float* __restrict__ scm,
                 const float* __restrict__ Jrest, int j_stride, const float* __restrict__ dA,
                 const float* __restrict__ dpf_part, int CS, const float* __restrict__ dth_direct,
                 float* __restrict__ dtheta /*[M][105]*/, float* __restrict__ dls /*[M][6]*/,
                 float* __restrict__ dJrest /*[M][105]*/, float* __restrict__ dbetaJ /*[M][NBall] or null*/,
                 float* __restrict__ dRs_out /*[M][35][9] adjoint of the rotation matrices (matrix input of SMAL.__call__), or null*/,
                 int nb, int betas_shared, int nDB_x, int nDB_y, int nDB_z, const float* __restrict__ dvp,
                 float* __restrict__ dbeta_part /*riders: workgroups >= M compute the shape-blend adjoint partials (dbeta_block), which only
                 the gradient assembly needs -- this launch has one workgroup per frame and leaves the chip idle otherwise*/) {
  PHASE_MARK(pc0);
  if ((int)blockIdx.x >= M) {
    __shared__ float rpart[4][32];
    const int blk = (int)blockIdx.x - M;
    dbeta_block(m, M, nb, betas_shared, blk % nDB_x, (blk / nDB_x) % nDB_y, blk / (nDB_x * nDB_y), nDB_x, nDB_z, dvp, dbeta_part, rpart);
    PHASE_MARK(pcr);
    PHASE_END(PH_CHAIN_RIDER, pc0, pcr);
    return;
  }
  // One block per frame: 256 threads for the loads / reductions at either end (latency), the first wave walks the
  // tree.  The tree is walked by depth (TreeLevels), 12 lanes per joint of the level.  Every joint
  // writes what it owes its parent into its own slots (cG, cJ, cS) and parents gather from their children in
  // descending joint order, so no two lanes ever add into the same word (deterministic).
  __shared__ float R[35][9], G[35][12], sc[35][3], J[35][3];
  __shared__ float dG[35][12], dR[35][9], dJ[35][3];
  __shared__ float cG[35][12], cJ[35][3], cS[35][3], sOwn[35][3];
  __shared__ float dRp[35][9], djv[35][3];
  __shared__ int sidx[105];
  __shared__ float psum[4][320];
  __shared__ float isc[35][3];          // 1 / s_j[a]
  __shared__ float sJS[105 * 48];       // d(rest joints)/d(beta), staged while the tree is walked
  __shared__ float dAs[35][12];         // this frame's dA, fetched with everything else in the first round trip
  __shared__ unsigned char t_lvl_off[36], t_lvl_joint[36], t_child_off[36], t_child_idx[36], t_par[36];
  __shared__ uint2 t_sch[kTreeMaxPass][8];    // per (pass, slot): joint | parent << 8 | children << 16 (joint 255: idle), the children's ids
  const int n = blockIdx.x, l = threadIdx.x;
  const TreeLevels& tl = m.tree;
  if (l < 36) {
    t_lvl_off[l] = tl.lvl_off[l]; t_child_off[l] = tl.child_off[l];
    if (l < 35) { t_lvl_joint[l] = tl.lvl_joint[l]; t_child_idx[l] = tl.child_idx[l]; t_par[l] = (unsigned char)max(m.parents[l], 0); }
  }
  if (l >= 128 && l < 128 + kTreeMaxPass * 8) {
    const int q = l - 128;
    const unsigned char* ch = tl.pass_child[q >> 3][q & 7];
    t_sch[q >> 3][q & 7] = make_uint2((unsigned)tl.pass_joint[q >> 3][q & 7] | ((unsigned)tl.pass_parent[q >> 3][q & 7] << 8) | ((unsigned)tl.pass_nchild[q >> 3][q & 7] << 16),
                                      (unsigned)ch[0] | ((unsigned)ch[1] << 8) | ((unsigned)ch[2] << 16) | ((unsigned)ch[3] << 24));
  }
  // the axis-angles (and their direct adjoint) of the Rodrigues adjoint at the END of the kernel are requested here, with everything
  // else: as loads behind the walk they were one more trip to memory on a kernel that is a single latency chain (round 6)
  const int lth = min(l, 34);
  const float th_pre[3] = {theta[((size_t)n * 35 + lth) * 3], theta[((size_t)n * 35 + lth) * 3 + 1], theta[((size_t)n * 35 + lth) * 3 + 2]};
  float dthd_pre[3] = {0.f, 0.f, 0.f};
  if (dth_direct) {
#pragma unroll
    for (int a = 0; a < 3; ++a) dthd_pre[a] = dth_direct[(size_t)n * 105 + lth * 3 + a];
  }
  const int nlev = tl.nlev;
  const bool js_lds = dbetaJ && m.NBall <= 48;
  const int njs = js_lds ? 105 * m.NBall : 1;    // up to 105 * 48 floats, staged while the tree is walked
  float js_tmp[20];
  const float* js_src = js_lds ? m.JS : Rm + (size_t)n * 315;                     // (not staged: any readable word)
#pragma unroll
  for (int r = 0; r < 20; ++r) js_tmp[r] = js_src[min(l + 256 * r, njs - 1)];    // (unconditional: in flight with everything below)
  // Every global operand of the frame is requested before the first is stored (unconditional loads from clamped indices,
  // the stores masked): as loops of conditional loads they were compiled into a dozen dependent trips to memory
  // (tools/isa_loads.py) at the head of a kernel that is one latency chain.
  {
    const int l2 = l + 256;
    const float r0v = Rm[(size_t)n * 315 + l], r1v = Rm[(size_t)n * 315 + min(l2, 314)];
    const float g0v = Gm[(size_t)n * 420 + l], g1v = Gm[(size_t)n * 420 + min(l2, 419)];
    const float a0v = dA[(size_t)n * 420 + l], a1v = dA[(size_t)n * 420 + min(l2, 419)];
    const int lc = min(l, 104);
    const float sv = scm[(size_t)n * 105 + lc], jv = Jrest[(size_t)n * j_stride + lc];
    const int siv = m.scale_idx[lc];
    // pose-feature adjoint -> dR of joints 1..34: sum of the column-split partials in a fixed order (four quarters of
    // the splits in parallel, then the quarters); root starts at 0
    constexpr int kMaxPer = (PBM_SPLITS + 3) / 4;            // partials per quarter held in registers (6 with 24 column splits)
    const int per = (CS + 3) / 4, qd = l >> 6, c0 = qd * per, c1 = min(CS, c0 + per);
    const size_t stride = (size_t)M * 308;
    float pv[5][kMaxPer];
    const bool fast = dpf_part != nullptr && per <= kMaxPer;
    if (fast) {
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const float* src = dpf_part + (size_t)n * 308 + min((l & 63) + 64 * r, 305);
#pragma unroll
        for (int c = 0; c < kMaxPer; ++c) pv[r][c] = src[(size_t)min(c0 + c, CS - 1) * stride];
      }
    }
    if (js_lds) {
#pragma unroll
      for (int r = 0; r < 20; ++r) { const int i = l + 256 * r; if (i < njs) sJS[i] = js_tmp[r]; }
    }
    R[l / 9][l % 9] = r0v;
    if (l2 < 315) R[l2 / 9][l2 % 9] = r1v;
    G[l / 12][l % 12] = g0v; dAs[l / 12][l % 12] = a0v;
    if (l2 < 420) { G[l2 / 12][l2 % 12] = g1v; dAs[l2 / 12][l2 % 12] = a1v; }
    if (l < 105) {
      sc[l / 3][l % 3] = sv; isc[l / 3][l % 3] = 1.0f / sv;
      J[l / 3][l % 3] = jv;
      sOwn[l / 3][l % 3] = 0.f; cS[l / 3][l % 3] = 0.f; cJ[l / 3][l % 3] = 0.f;
      sidx[l] = siv;
    }
    if (dpf_part) {
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const int el = (l & 63) + 64 * r;
        if (el < 306) {
          float sacc = 0.f;
          if (fast) {
            if (c0 < c1) sacc = pv[r][0];
#pragma unroll
            for (int c = 1; c < kMaxPer; ++c)
              if (c0 + c < c1) sacc += pv[r][c];               // ((v0 + v1) + v2) + ...
          } else {
            const float* src = dpf_part + (size_t)n * 308 + el;
            for (int c = c0; c < c1; ++c) sacc += src[c * stride];
          }
          psum[qd][el] = sacc;
        }
      }
    }
  }
  __syncthreads();
  PHASE_MARK(pc1);                      // every operand of the frame in LDS
  for (int i = l; i < 315; i += 256)
    dR[i / 9][i % 9] = (i >= 9 && dpf_part) ? ((psum[0][i - 9] + psum[1][i - 9]) + psum[2][i - 9]) + psum[3][i - 9] : 0.f;
  // A_j = [G.R | G.t - G.R J_j]
  for (int i = l; i < 420; i += 256) {
    const int j = i / 12, e = i % 12, a = e >> 2, b = e & 3;
    const float* da = dAs[j];
    dG[j][e] = (b < 3) ? da[e] - da[a * 4 + 3] * J[j][b] : da[e];
  }
  for (int i = l; i < 105; i += 256) {
    const int j = i / 3, c = i % 3;
    const float* da = dAs[j];
    dJ[j][c] = -(G[j][0 * 4 + c] * da[3] + G[j][1 * 4 + c] * da[7] + G[j][2 * 4 + c] * da[11]);
  }
  __syncthreads();
  PHASE_MARK(pc2);                      // dG / dJ set up
  const int slot = l / 12, e = l % 12;
  const ChainLds cl{R, G, sc, isc, J, dG, dR, cG, cJ, cS, sOwn, dRp, djv};
  if (l < 64 && tl.fast) {
    // Round 6: the lane's joint, parent and children of a pass are ONE 8-byte read (TreeLevels::pass_*, packed into t_sch below),
    // requested a pass ahead -- inside a pass the level offsets -> joint -> parent -> child list chase cost more than the
    // arithmetic (19 k cycles of the block's 42 k for 12 passes, profiles/r6_lbs_phase_breakdown.txt).  Passes run deepest level
    // first; the loop stays rolled (straight-line code run once by one wave pays an instruction-cache miss per line: the unrolled
    // form was slower than the table-driven loop).  Both walks do a joint's work in chain_joint_adjoint; theirs are the schedule, the
    // gather of the children's cG and the fences.  No test compares the two walks' bits (a tree takes one or the other) -- each is
    // held to the float64 oracle on trees that reach it, this one with kTreeMaxChildren children per joint and kTreeMaxPass passes
    // too (tests/test_gpu_model_forms.py).
    const int npass = tl.npass;
    const int slot_c = min(slot, 7);
    uint2 sch_n = t_sch[max(npass - 1, 0)][slot_c];
#pragma unroll 1
    for (int k = npass - 1; k >= 0; --k) {
      const uint2 sch = sch_n;
      sch_n = t_sch[max(k - 1, 0)][slot_c];
      const bool live = (sch.x & 255u) != 255u;
      const int i = live ? (int)(sch.x & 255u) : 0, p = live ? (int)((sch.x >> 8) & 255u) : 0, nch = live ? (int)(sch.x >> 16) : 0;
      const unsigned chil_k = sch.y;
      // gather what the children owe this joint's dG (children were finished one level deeper)
      if (live) {
        float acc = dG[i][e];
        float cv[kTreeMaxChildren];
#pragma unroll
        for (int q = 0; q < kTreeMaxChildren; ++q) cv[q] = cG[(chil_k >> (8 * q)) & 255u][e];     // (unused entries name joint 0: readable)
#pragma unroll
        for (int q = 0; q < kTreeMaxChildren; ++q) acc += (q < nch) ? cv[q] : 0.f;
        dG[i][e] = acc;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (live) chain_joint_adjoint<0>(cl, i, p, e);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (live) chain_joint_adjoint<1>(cl, i, p, e);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  } else if (l < 64)   // the walk needs 60 lanes: one wave, no block barriers (LDS operations of a wave complete in order)
  for (int L = nlev - 1; L >= 1; --L) {
    const int j0 = t_lvl_off[L], nj = t_lvl_off[L + 1] - j0;
    for (int base = 0; base < nj; base += 5) {           // 5 joints x 12 lanes per pass
      const bool live = (slot < 5) && (base + slot < nj);
      const int i = live ? t_lvl_joint[j0 + base + slot] : 0;
      const int p = live ? t_par[i] : 0;
      // gather what the children owe this joint's dG (children were finished one level deeper)
      if (live) {
        float acc = dG[i][e];
        for (int q = t_child_off[i]; q < t_child_off[i + 1]; ++q) acc += cG[t_child_idx[q]][e];
        dG[i][e] = acc;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (live) chain_joint_adjoint<0>(cl, i, p, e);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (live) chain_joint_adjoint<1>(cl, i, p, e);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  PHASE_MARK(pc3);                      // tree walk
  // root: gather its children, then its own rotation / joint adjoint
  if (l < 12) {
    float acc = dG[0][l];
    for (int q = t_child_off[0]; q < t_child_off[1]; ++q) acc += cG[t_child_idx[q]][l];
    dG[0][l] = acc;
  }
  __syncthreads();
  if (l < 9) dR[0][l] += dG[0][(l / 3) * 4 + (l % 3)];
  // joint and scale adjoints: children first (descending), then the joint's own term -- the order of a reverse loop
  for (int i = l; i < 105; i += 256) {
    const int j = i / 3, a = i % 3;
    float aj = dJ[j][a], as = 0.f;
    for (int q = t_child_off[j]; q < t_child_off[j + 1]; ++q) { aj -= cJ[t_child_idx[q]][a]; as -= cS[t_child_idx[q]][a]; }
    if (j > 0) { aj += cJ[j][a]; as += sOwn[j][a]; }
    else aj += dG[0][a * 4 + 3];
    dJ[j][a] = aj;
    sOwn[j][a] = as;                                      // now the full d loss / d s_j[a]
  }
  __syncthreads();
  PHASE_MARK(pc4);                      // root, joint / scale adjoints
  if (l < 35) {
    const float th[3] = {th_pre[0], th_pre[1], th_pre[2]};
    float g[9], d[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) g[q] = dR[l][q];
    if (dRs_out) {
#pragma unroll
      for (int q = 0; q < 9; ++q) dRs_out[((size_t)n * 35 + l) * 9 + q] = g[q];
    }
    rodrigues_bwd(th, g, d);
#pragma unroll
    for (int a = 0; a < 3; ++a)
      dtheta[(size_t)n * 105 + l * 3 + a] = d[a] + (dth_direct ? dthd_pre[a] : 0.f);
  }
  if (dls) {                                     // d log-scale: 6 masked sums over the 105 (joint, axis) scales
    const int w = l >> 6, lane = l & 63;
    for (int sidx_l = w; sidx_l < 6; sidx_l += 4) {
      float v = 0.f;
      if (sidx[lane] == sidx_l) v = sOwn[lane / 3][lane % 3] * sc[lane / 3][lane % 3];
      if (lane + 64 < 105 && sidx[lane + 64] == sidx_l) v += sOwn[(lane + 64) / 3][(lane + 64) % 3] * sc[(lane + 64) / 3][(lane + 64) % 3];
      v = wave_sum(v);
      if (lane == 0) dls[(size_t)n * 6 + sidx_l] = v;
    }
  }
  for (int i = l; i < 105; i += 256) dJrest[(size_t)n * 105 + i] = dJ[i / 3][i % 3];
  // rest joints are affine.  One lane of a wave per shape direction: NBall <= kMaxModelBetas = 64 (smalfit_plan.h: model_dims_refusal)
  if (dbetaJ) {
    const int w = l >> 6, b = l & 63;
    if (b < m.NBall) {
      float acc = 0.f;
      if (js_lds) {
#pragma unroll 9
        for (int r = 0; r < 27; ++r) { const int i = w * 27 + r; if (i < 105) acc = fmaf(dJ[i / 3][i % 3], sJS[i * m.NBall + b], acc); }
      } else {
        for (int i = w * 27; i < min(105, w * 27 + 27); ++i) acc = fmaf(dJ[i / 3][i % 3], m.JS[i * m.NBall + b], acc);
      }
      psum[w][b] = acc;
    }
    __syncthreads();
    if (l < m.NBall) dbetaJ[(size_t)n * m.NBall + l] = ((psum[0][l] + psum[1][l]) + psum[2][l]) + psum[3][l];
  }
  PHASE_MARK(pc5);                      // Rodrigues adjoint, limb scales, rest-joint path
  PHASE_ADD(PH_CHAIN, 0, pc0, pc1); PHASE_ADD(PH_CHAIN, 1, pc1, pc2); PHASE_ADD(PH_CHAIN, 2, pc2, pc3); PHASE_ADD(PH_CHAIN, 3, pc3, pc4); PHASE_ADD(PH_CHAIN, 4, pc4, pc5);
  PHASE_END(PH_CHAIN, pc0, pc5);
}

// ------------------------------------------------------------------------------------------------
// K11: gradient assembly (single block): shared-parameter reductions, masks, loss totals
// ------------------------------------------------------------------------------------------------
// kPerImage: independent images -- every shape set and every frame's limb scales carry a prior term of their own (AssembleExt).
// <false> is the kernel as it always was.
template <bool kPerImage>
__global__ void __launch_bounds__(256)
assemble_kernel(AssembleArgs a, AssembleExt x) {
  // Blocks take roles (kAsmElem / kAsmLoss are compile-time):
  //   [0, nbs)            d loss / d betas of shape set s: column-block partials + joint path + prior
  //   nbs                 limb scales
  //   next kAsmElem       rotations / translation: masks, vertex-block partials
  //   next kAsmLoss       partial sums of the silhouette loss
  // and the block that finishes last adds up the eight loss terms (fixed order: deterministic).
  __shared__ float red[16];
  __shared__ double bsum[12][32];
  __shared__ float part[32][8];
  __shared__ double dpart[32][8];
  __shared__ int is_last;
  const int t = threadIdx.x;
  PHASE_MARK(pa0);
  const int M = a.M;
  const int nbs = asm_shape_sets(a.betas_shared, M);
  int role = blockIdx.x;
  const int ph_role = (role < nbs) ? PH_ASM_BETA : PH_ASM_ELEM;
  if (role < nbs) {
    if (a.g_betas) {
      // (the sums themselves: asm_beta_fetch / _slices / _total, kernels_lbs_forward.inc)
      const int s = role;
      for (int b0 = 0; b0 < a.nb; b0 += 20) {     // more than 20 directions (up to NBall): further passes (a.nb is block-uniform)
        if (b0) __syncthreads();                  // the previous pass has read bsum
        BetaOperands bo;
        asm_beta_fetch(a, s, b0, bo);
        asm_beta_slices(a, s, b0, bo, bsum);
        __syncthreads();
        const float tot = asm_beta_total(a, s, b0, bo, bsum);
        // (independent images: shape set s has a prior term of its own, its gradient is row s)
        if constexpr (kPerImage) {
          if (t < 20 && b0 + t < a.nb) a.g_betas[s * a.nb + b0 + t] = x.gb_prior_pf ? tot + x.gb_prior_pf[(size_t)s * x.gb_stride + b0 + t] : tot;
        } else
        if (t < 20 && b0 + t < a.nb) a.g_betas[s * a.nb + b0 + t] = tot;
      }
    }
  } else if ((role -= nbs) == 0) {
    if (a.g_ls) {
      if (a.ls_shared) {
        LsOperands lo;
        asm_ls_fetch(a, lo);
        asm_ls_slices(a, lo, dpart);
        __syncthreads();
        const float tot = asm_ls_total(a, lo, dpart);
        if (t < 6) a.g_ls[t] = tot;
      } else {
        if (kPerImage && x.gls_prior_pf)     // independent images: frame n's own prior row
          for (int i = t; i < M * 6; i += 256) a.g_ls[i] = a.dls[i] + x.gls_prior_pf[(size_t)(i / 6) * x.gls_stride + i % 6];
        else
          for (int i = t; i < M * 6; i += 256) a.g_ls[i] = a.dls[i];
      }
    }
  } else if ((role -= 1) < kAsmElem) {
    const int gt = role * 256 + t, gs = kAsmElem * 256;
    for (int i = gt; i < M * 3; i += gs) {
      const int n = i / 3, e = i % 3;
      if (a.g_grot) a.g_grot[i] = asm_grot_elem(a, n, e);
      if (a.g_trans) a.g_trans[i] = asm_trans_elem(a, n, e);
    }
    if (a.g_jrot) {
      // eight elements per trip: loads first (clamped index), stores after -- as a loop of load-load-store the compiler kept
      // every store behind its own loads (the pointers may alias) and the eight unrolled elements were eight trips to memory
      const int total = M * 102;
      for (int i0 = gt; i0 < total; i0 += 8 * gs) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = min(i0 + u * gs, total - 1), n = i / 102, e = i % 102;
          v[u] = asm_jrot_elem(a, n, e);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i0 + u * gs < total) a.g_jrot[i0 + u * gs] = v[u];
      }
    }
  } else if (a.losses) {
    role -= kAsmElem;                    // [0, kAsmLoss)
    float lsil = 0.f;
    if (a.tile_loss) {
      for (int k = role * 256 + t; k < M * a.T; k += kAsmLoss * 256) {
        const int n = k / a.T;
        const int Bn = frame_window_size(n, a.win);
        lsil += a.tile_loss[k] * (a.w_sil / ((float)Bn * (float)a.S * (float)a.S));
      }
    }
    // the queue kernels' partials are integers whose split over blocks varies from run to run: add them up as
    // integers (exact, order-free) and convert the grand total once, in the last block
    long long qs = 0;
    if (a.qloss) for (int k = role * 256 + t; k < a.nqblk; k += kAsmLoss * 256) qs += a.qloss[k];
    qs = wave_sum_i64(qs);
    __shared__ long long qred[4];
    if ((t & 63) == 0) qred[t >> 6] = qs;
    lsil = block_sum(lsil, red);                        // (contains the barriers that also cover qred)
    if (t == 0) { a.lpart[role] = lsil; a.qpart[role] = (qred[0] + qred[1]) + (qred[2] + qred[3]); }
  }
  PHASE_MARK(pa1);
  PHASE_END(ph_role, pa0, pa1);
  (void)ph_role;
  if (!a.losses) return;
  // ---- the last block to arrive finishes the loss terms: [joint, pose, splay, betas, sil, temp_joint, temp_global, temp_trans, limit]
  __threadfence();
  __syncthreads();
  if (t == 0) is_last = (atomicAdd(a.counter, 1) == (int)gridDim.x - 1);
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  // silhouette: the kAsmLoss partials, one per lane, added in a fixed butterfly order
  static_assert(kAsmLoss == 16, "butterfly below");
  float lsil = 0.f;
  if (t < 64) {
    const volatile float* lp = a.lpart;
    lsil = (t < kAsmLoss) ? lp[t] : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) lsil += __shfl_xor(lsil, o, 64);
    const volatile long long* qp = a.qpart;
    long long qtot = (t < kAsmLoss) ? qp[t] : 0ll;
    qtot = wave_sum_i64(qtot);
    lsil += (float)((double)qtot * (1.0 / (double)kLossFix));
  }
  // per-frame terms: 32 frame slices x 8 terms in parallel, then the slices in order
  {
    const int k = t & 7, sl = t >> 3;
    float acc = 0.f;
    if (a.loss_part) for (int n = sl; n < M; n += 32) acc += a.loss_part[n * 8 + k];
    // (column 4 of the per-frame partials is unused -- the silhouette comes from the tiles: with one prior term per frame it adds those)
    if (kPerImage && x.prior_loss_pf && k == 4) { acc = 0.f; for (int n = sl; n < M; n += 32) acc += x.prior_loss_pf[n]; }
    part[sl][k] = acc;
  }
  __syncthreads();
  if (t < 8) {
    float acc = 0.f;
    if (t == 3) {
      acc = a.loss_betas ? *a.loss_betas : 0.f;
      if (kPerImage && x.prior_loss_pf) for (int i = 0; i < 32; ++i) acc += part[i][4];
    }
    else if (t == 4) acc = lsil;
    else for (int i = 0; i < 32; ++i) acc += part[i][t];
    a.losses[t] = acc;
  }
  if (t == 8) {                       // joint limits: column 3 of the per-frame partials
    float acc = 0.f;
    for (int i = 0; i < 32; ++i) acc += part[i][3];
    a.losses[8] = acc;
  }
  if (t == 0) *a.counter = 0;
  PHASE_MARK(pa2);
  PHASE_END(PH_ASM_LAST, pa1, pa2);
}

// One row of the nine loss terms per frame (smalfit_fit_args.losses_per_frame), launched only when a caller asks for it -- a kernel of
// its own so that assemble_kernel, the tail of every iteration, stays what it is.  One wave per frame; everything it reads was
// written by earlier launches.  The tile partials of a frame are added lane-strided and then in the butterfly's order (fixed), the
// queue kernels' share is an integer: two runs give the same bits.
__global__ void __launch_bounds__(256)
frame_loss_rows_kernel(AssembleArgs a, AssembleExt x) {
  const int t = threadIdx.x, lane = t & 63, M = a.M;
  for (int n = (int)blockIdx.x * 4 + (t >> 6); n < M; n += kAsmRows * 4) {
    const int Bn = frame_window_size(n, a.win);
    float lsil = 0.f;
    if (a.tile_loss) {
      const float wn = a.w_sil / ((float)Bn * (float)a.S * (float)a.S);
      for (int k = lane; k < a.T; k += 64) lsil += a.tile_loss[(size_t)n * a.T + k] * wn;
    }
    lsil = wave_sum(lsil);
    if (lane == 0) {
      if (a.tile_loss) {
        unsigned long long* fq = x.frame_qloss + (size_t)n * kFrameLossStride;
        lsil += (float)((double)*fq * (1.0 / (double)kLossFix));
        *fq = 0ull;                  // zero for the next evaluation that feeds it
      }
      float prior = 0.f;
      if (x.prior_loss_pf) prior = x.prior_loss_pf[n];
      else if (a.loss_betas && x.prior_windows > 0 && (n + a.win.offset) % a.win.window == 0) prior = *a.loss_betas / (float)x.prior_windows;
      const float* lp = a.loss_part + n * 8;
      float* o = x.losses_pf + (size_t)n * 9;
      o[0] = lp[0]; o[1] = lp[1]; o[2] = lp[2]; o[3] = prior; o[4] = lsil; o[5] = lp[5]; o[6] = lp[6]; o[7] = lp[7]; o[8] = lp[3];
    }
  }
}

// One row per WINDOW of the sequence (smalfit_fit_eval_windows): the nine loss terms of the window's frames and the window's share
// of the shared parameters' gradient, so that a caller can weight or backpropagate every window of ONE evaluation on its own
// (smal_fitter.py:107-175 is called per window, optimize_to_joints.py:119-122).  Launched only by that entry point, behind
// everything it reads, like frame_loss_rows_kernel: the backward pass ran in the per-frame partial layout of independent images
// (dbeta_part[n][column block][nb], chain_bwd_kernel's riders with betas_shared 0) and assemble_kernel left the shared gradients
// alone.  One block per window: 8 slices of its frames' column-block partials per shape direction, then the slices, the frames'
// rest-joint paths and the prior's share in a fixed order, in double, rounded once; wave 1 the shared limb scales, wave 2 the loss
// row (the queue kernels' integer share is added as integers and converted once).  The block that arrives last adds the rows in
// window order, in double: that is smalfit_fit_args.g_betas / g_log_beta_scales.  Two runs give the same bits.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__global__ void __launch_bounds__(256)
window_rows_kernel(AssembleArgs a, AssembleExt x, WindowRowsDev r) {
  __shared__ double bsum[8][kWindowRowBetas];
  __shared__ int is_last;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, w = blockIdx.x, M = a.M;
  // local frames [n0, n1) of the w-th window that holds any of these frames; a shard may start inside a window it does not own
  const int start = (a.win.offset / a.win.window + w) * a.win.window;
  const int n0 = max(start - a.win.offset, 0), n1 = min(start + a.win.window - a.win.offset, M);
  const bool owned = start >= a.win.offset && x.prior_windows > 0;
  if (r.row_betas) {
    const int bl = t & 31, slice = t >> 5;
    double acc = 0.0;
    if (bl < a.nb) {
      const int items = (n1 - n0) * a.nblk_beta;                                   // frame-major, column blocks inside: contiguous rows of nb
      const float* pp = a.dbeta_part + (size_t)n0 * a.nblk_beta * a.nb + bl;
#pragma unroll 8
      for (int i = slice; i < items; i += 8) acc += (double)pp[(size_t)i * a.nb];
    }
    bsum[slice][bl] = acc;
  }
  __syncthreads();
  if (r.row_betas && t < a.nb) {
    double tot = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) tot += bsum[s][t];
    for (int n = n0; n < n1; ++n) tot += (double)a.dbetaJ[(size_t)n * a.NBall + t];
    if (a.gb_prior && owned) tot += (double)a.gb_prior[t] / (double)x.prior_windows;
    const float row = (float)tot;
    r.row_betas[w * kWindowRowBetas + t] = row;
    if (r.g_betas) r.g_betas[w * a.nb + t] = row;
  } else if (r.row_ls && wave == 1 && lane < 6) {
    double tot = 0.0;
    for (int n = n0; n < n1; ++n) tot += (double)a.dls[(size_t)n * 6 + lane];
    if (a.gls_prior && owned) tot += (double)a.gls_prior[lane] / (double)x.prior_windows;
    const float row = (float)tot;
    r.row_ls[w * kWindowRowScales + lane] = row;
    if (r.g_ls) r.g_ls[w * 6 + lane] = row;
  } else if (wave == 2) {
    double lsil = 0.0;
    if (a.tile_loss) {
      // (every frame of a window has the window's normaliser)
      const float wn = a.w_sil / ((float)frame_window_size(n0, a.win) * (float)a.S * (float)a.S);
      const int cnt = (n1 - n0) * a.T;
      const float* tl = a.tile_loss + (size_t)n0 * a.T;
      for (int k = lane; k < cnt; k += 64) lsil += (double)(tl[k] * wn);
    }
    lsil = wave_sum_f64(lsil);
    if (lane == 4 && a.tile_loss) {
      unsigned long long q = 0ull;
      for (int n = n0; n < n1; ++n) {
        unsigned long long* fq = x.frame_qloss + (size_t)n * kFrameLossStride;
        q += *fq;
        if (r.clear_qloss) *fq = 0ull;           // zero for the next evaluation that feeds it
      }
      lsil += (double)q * (1.0 / (double)kLossFix);
    }
    if (lane < 9) {
      // columns: joint, pose, splay, betas, sil_reproj, temp_joint, temp_global, temp_trans, limit <- loss_part[n][0, 1, 2, -, -, 5, 6, 7, 3]
      float v;
      if (lane == 3) v = (a.loss_betas && owned) ? *a.loss_betas / (float)x.prior_windows : 0.f;
      else if (lane == 4) v = (float)lsil;
      else {
        const int src = lane == 8 ? 3 : lane;
        double acc = 0.0;
        for (int n = n0; n < n1; ++n) acc += (double)a.loss_part[n * 8 + src];
        v = (float)acc;
      }
      r.losses[w * 9 + lane] = v;
    }
  }
  if (!r.tot_betas && !r.tot_ls) return;
  // ---- the last block to arrive adds the rows in window order
  __threadfence();
  __syncthreads();
  if (t == 0) is_last = (atomicAdd(r.counter, 1) == (int)gridDim.x - 1);
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  if (r.tot_betas && t < a.nb) {
    const volatile float* rows = r.row_betas;
    double tot = 0.0;
    for (int i = 0; i < r.W; ++i) tot += (double)rows[i * kWindowRowBetas + t];
    r.tot_betas[t] = (float)tot;
  }
  if (r.tot_ls && wave == 1 && lane < 6) {
    const volatile float* rows = r.row_ls;
    double tot = 0.0;
    for (int i = 0; i < r.W; ++i) tot += (double)rows[i * kWindowRowScales + lane];
    r.tot_ls[lane] = (float)tot;
  }
  if (t == 0) *r.counter = 0;
}

// adjoint of a per-frame template offset (SMAL.__call__'s del_v / v_template): d v_shaped = d v_posed + J_regressor d(rest joints)
__global__ void offset_grad_kernel(ModelDev m, int M, const float* __restrict__ dvp /*[M][3][Vp]*/,
                                   const float* __restrict__ dJrest /*[M][105]*/, float* __restrict__ doff /*[M][V][3]*/) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
  if (v >= m.V) return;
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = dvp[((size_t)n * 3 + c) * m.Vp + v];
  for (int k = 0; k < m.Kj; ++k) {
    const float w = m.jrv_val[(size_t)k * m.Vp + v];
    const int j = m.jrv_j[(size_t)k * m.Vp + v];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = fmaf(w, dJrest[(size_t)n * 105 + j * 3 + c], g[c]);
  }
  float* o = doff + ((size_t)n * m.V + v) * 3;
  o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
}

// ------------------------------------------------------------------------------------------------
// K12: Adam over up to four [begin, end) ranges of one flat parameter buffer in a single launch (the trainable set of a
// stage; the update itself is adam_update).  fresh != 0: first step of a stage -- the moments are taken as zero instead
// of being read, so a stage needs no fill of the optimiser state.
// ------------------------------------------------------------------------------------------------
// (the packed ranges: AdamSegments of smalfit_plan.h)
// element j (< off[nseg]) of the packed ranges
__device__ __forceinline__ void adam_segments_element(const AdamSegments& sg, int j, float* p, const float* g, float* mm,
                                                      float* vv, float step_size, float b1, float b2, float eps,
                                                      float bc2_sqrt, bool fresh) {
  int sgi = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) sgi += (k < sg.nseg && j >= sg.off[k]) ? 1 : 0;
  const int i = sg.beg[sgi] + (j - sg.off[sgi]);
  const float gi = g[i];
  adam_update(gi, fresh ? 0.f : mm[i], fresh ? 0.f : vv[i], b1, b2, eps, step_size, bc2_sqrt, mm[i], vv[i], p[i]);
}
__global__ void adam_segments_kernel(AdamSegments sg, float* __restrict__ p, const float* __restrict__ g,
                                     float* __restrict__ mm, float* __restrict__ vv,
                                     float step_size, float b1, float b2, float eps, float bc2_sqrt, int fresh) {
  PHASE_MARK(pz0);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= sg.off[sg.nseg]) return;
  adam_segments_element(sg, j, p, g, mm, vv, step_size, b1, b2, eps, bc2_sqrt, fresh != 0);
  PHASE_MARK(pz1);
  PHASE_END(PH_ADAM, pz0, pz1);
}

// The same step for a captured HIP graph: the launch parameters of a graph node are frozen, so the step count comes from a
// device counter (advanced by tick_kernel at the head of every replay) and the bias terms are formed here.
__global__ void tick_kernel(int* counter) { *counter += 1; }
__global__ void set_counter_kernel(int* counter, int value) { *counter = value; }
__global__ void adam_segments_graph_kernel(AdamSegments sg, float* __restrict__ p, const float* __restrict__ g,
                                           float* __restrict__ mm, float* __restrict__ vv, const int* __restrict__ step_counter,
                                           float lr, float b1, float b2, float eps) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= sg.off[sg.nseg]) return;
  const int t = *step_counter;
  float step_size, bc2_sqrt;
  adam_bias_terms(lr, b1, b2, t, step_size, bc2_sqrt);
  adam_segments_element(sg, j, p, g, mm, vv, step_size, b1, b2, eps, bc2_sqrt, t == 1);
}

// betas / shared limb scales from a slot of the engine's shared-parameter staging (smalfit_engine::shstate) back to the caller's flat buffers (one launch per smalfit_fit_run)
__global__ void shared_state_restore_kernel(const float* __restrict__ slot, float* __restrict__ p, float* __restrict__ mm, float* __restrict__ vv,
                                            int nbeta, int off_beta, int nls, int off_ls) {
  const int t = threadIdx.x;
  int i = -1, j = t;
  if (t < nbeta) i = off_beta + t;
  else if (t >= 20 && t < 20 + nls) i = off_ls + (t - 20);
  if (i < 0) return;
  p[i] = slot[j]; mm[i] = slot[32 + j]; vv[i] = slot[64 + j];
}

// Frame-sharded fitting, per-rank record of one iteration (smalify_amd/distributed.py): the rank's partial gradient of
// the shared parameters (ns floats) followed by the masked pose (105) | translation (3) of its first and its last
// frame as they are AFTER this iteration's Adam step on the per-frame parameters -- the neighbours' temporal halo of the
// next iteration.
__global__ void shard_record_kernel(int ns, const float* __restrict__ shared_grad, int M, const float* __restrict__ grot,
                                    const float* __restrict__ jrot, const float* __restrict__ trans,
                                    const float* __restrict__ gmask, const float* __restrict__ rmask, float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < ns) { out[t] = shared_grad[t]; return; }
  const int u = t - ns;
  if (u >= 216) return;
  const int which = u / 108, c = u - which * 108;
  const int n = which ? M - 1 : 0;
  float v;
  if (c < 3) v = grot[n * 3 + c] * gmask[c];
  else if (c < 105) v = jrot[n * 102 + (c - 3)] * rmask[c - 3];
  else v = trans[n * 3 + (c - 105)];
  out[t] = v;
}

// ... and what every rank does with the gathered records: add the partial gradients in rank order (the same bits on
// every rank) and take the Adam step on the shared parameters [0, ns_train) of the flat buffer
__global__ void shard_reduce_adam_kernel(int world, int stride, const float* __restrict__ gathered, int ns, int ns_train,
                                         float* __restrict__ p, float* __restrict__ g, float* __restrict__ mm, float* __restrict__ vv,
                                         float step_size, float b1, float b2, float eps, float bc2_sqrt, int fresh) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  float gi = 0.f;
  for (int r = 0; r < world; ++r) gi += gathered[(size_t)r * stride + i];
  g[i] = gi;
  if (i >= ns_train) return;
  adam_update(gi, fresh ? 0.f : mm[i], fresh ? 0.f : vv[i], b1, b2, eps, step_size, bc2_sqrt, mm[i], vv[i], p[i]);
}

// ------------------------------------------------------------------------------------------------
// temporal term on its own (SMALFitter.get_temporal called outside forward): M frames, one block
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(128)
temporal_kernel(int M, float w_temp, const float* __restrict__ theta, const float* __restrict__ trans,
                float* __restrict__ losses /*[3] joint, global, trans*/, float* __restrict__ dtheta /*[M][105]*/,
                float* __restrict__ dtrans /*[M][3]*/) {
  __shared__ float red[16];
  const int t = threadIdx.x;
  float lj = 0.f, lg = 0.f, lt = 0.f;
  for (int idx = t; idx < M * 108; idx += 128) {
    const int n = idx / 108, e = idx % 108;
    const bool is_tr = e >= 105;
    const int k = is_tr ? e - 105 : e;
    const float D = is_tr ? 3.0f : (k < 3 ? 3.0f : 102.0f);
    const float cur = is_tr ? trans[n * 3 + k] : theta[n * 105 + k];
    float g = 0.f;
    if (n + 1 < M) {
      const float d = cur - (is_tr ? trans[(n + 1) * 3 + k] : theta[(n + 1) * 105 + k]);
      const float term = d * d * (w_temp / D);
      if (is_tr) lt += term; else if (k < 3) lg += term; else lj += term;
      g += d;
    }
    if (n > 0) g += cur - (is_tr ? trans[(n - 1) * 3 + k] : theta[(n - 1) * 105 + k]);
    g *= 2.0f * w_temp / D;
    if (is_tr) dtrans[n * 3 + k] = g; else dtheta[n * 105 + k] = g;
  }
  lj = block_sum(lj, red); lg = block_sum(lg, red); lt = block_sum(lt, red);
  if (t == 0) { losses[0] = lj; losses[1] = lg; losses[2] = lt; }
}

// apply masks to a (M,105) theta adjoint -> grads of global_rotation (M,3) and joint_rotations (M,102)
__global__ void split_theta_grad_kernel(int M, const float* __restrict__ dtheta, const float* __restrict__ gmask,
                                        const float* __restrict__ rmask, float* __restrict__ g_grot,
                                        float* __restrict__ g_jrot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * 105) return;
  const int n = i / 105, e = i % 105;
  if (e < 3) { if (g_grot) g_grot[n * 3 + e] = dtheta[i] * (gmask ? gmask[e] : 1.f); }
  else if (g_jrot) g_jrot[n * 102 + e - 3] = dtheta[i] * (rmask ? rmask[e - 3] : 1.f);
}

// keypoint projection for arbitrary points (Renderer.forward points branch) + adjoint
__global__ void project_points_kernel(int count, int S, const float* __restrict__ pts, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float xn, yn, zv;
  world_to_ndc(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], xn, yn, zv);
  const float half = 0.5f * (float)(S - 1);
  out[i * 2] = half * (1.0f - yn);
  out[i * 2 + 1] = half * (1.0f - xn);
}
__global__ void project_points_bwd_kernel(int count, int S, const float* __restrict__ pts,
                                          const float* __restrict__ dout, float* __restrict__ dpts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float xn, yn, zv;
  world_to_ndc(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], xn, yn, zv);
  const float half = 0.5f * (float)(S - 1);
  world_to_ndc_bwd(xn, yn, zv, -half * dout[i * 2 + 1], -half * dout[i * 2], dpts[i * 3], dpts[i * 3 + 1], dpts[i * 3 + 2]);
}

// Rodrigues on its own (batch_rodrigues drop-in) + adjoint
__global__ void rodrigues_kernel(int count, const float* __restrict__ th, float* __restrict__ R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float r[9];
  const float t[3] = {th[i * 3], th[i * 3 + 1], th[i * 3 + 2]};
  rodrigues_fwd(t, r);
#pragma unroll
  for (int e = 0; e < 9; ++e) R[i * 9 + e] = r[e];
}
__global__ void rodrigues_bwd_kernel(int count, const float* __restrict__ th, const float* __restrict__ dR,
                                     float* __restrict__ dth) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float t[3] = {th[i * 3], th[i * 3 + 1], th[i * 3 + 2]};
  float g[9], d[3];
#pragma unroll
  for (int e = 0; e < 9; ++e) g[e] = dR[i * 9 + e];
  rodrigues_bwd(t, g, d);
  dth[i * 3] = d[0]; dth[i * 3 + 1] = d[1]; dth[i * 3 + 2] = d[2];
}

// Prior.__call__ on its own (pose_prior_35.py:117-124): out[n][c] = (((x - mu) P)[c] * mask[c])^2
__global__ void __launch_bounds__(128)
pose_prior_kernel(const float* __restrict__ x, const float* __restrict__ prec, const float* __restrict__ mean,
                  const float* __restrict__ mask, float* __restrict__ out /*[N][105]*/) {
  __shared__ float xs[105];
  const int n = blockIdx.x, t = threadIdx.x;
  if (t < 105) xs[t] = x[n * 105 + t] - mean[t];
  __syncthreads();
  if (t < 105) {
    float acc = 0.f;
    for (int r = 0; r < 105; ++r) acc = fmaf(xs[r], prec[r * 105 + t], acc);
    acc *= mask[t];
    out[n * 105 + t] = acc * acc;
  }
}
// adjoint: dx[n][r] = sum_c dout[n][c] * 2 res[c] mask[c] P[r][c]
__global__ void __launch_bounds__(128)
pose_prior_bwd_kernel(const float* __restrict__ x, const float* __restrict__ prec, const float* __restrict__ mean,
                      const float* __restrict__ mask, const float* __restrict__ dout, float* __restrict__ dx) {
  __shared__ float xs[105], g[105];
  const int n = blockIdx.x, t = threadIdx.x;
  if (t < 105) xs[t] = x[n * 105 + t] - mean[t];
  __syncthreads();
  if (t < 105) {
    float acc = 0.f;
    for (int r = 0; r < 105; ++r) acc = fmaf(xs[r], prec[r * 105 + t], acc);
    g[t] = 2.0f * acc * mask[t] * mask[t] * dout[n * 105 + t];
  }
  __syncthreads();
  if (t < 105) {
    float acc = 0.f;
    for (int c = 0; c < 105; ++c) acc = fmaf(g[c], prec[t * 105 + c], acc);
    dx[n * 105 + t] = acc;
  }
}


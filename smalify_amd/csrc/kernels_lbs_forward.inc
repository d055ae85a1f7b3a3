// LBS forward and per-frame losses (K0-K4) -- part of smalfit_kernels.hip (included inside namespace smalfit; not a translation unit of its own)

// ------------------------------------------------------------------------------------------------
// Gradient assembly roles: ONE definition for assemble_kernel and for the pending step of lbs_head_step_kernel (the same
// operations in the same order: the same bits wherever they run).  Written for 256-thread blocks.  Each sum comes as a FETCH --
// its first batch of operands requested unconditionally from clamped indices, so that a caller can have everything it reads in
// flight at once -- and the additions, in the order of a plain loop over the operands.
// ------------------------------------------------------------------------------------------------
// d loss / d betas of shape set s, directions [b0, b0 + 20), in two halves around a block barrier: 12 slices of the frames' joint
// paths and the column-block partials per direction, then the slices in order (+ the prior's share).
// The shared-shape gradient is the sum of every frame's and every column block's partial, and in a fit that has settled those
// partials largely cancel: they are added in DOUBLE (round 6; fixed order as before) and rounded once.  That is the principled
// sum, but it moved no printed digit: config 3 after stage 1 stays at d/d betas 9.86e-6, d/d log scales 3.64e-5 off the float64
// oracle, as with the float32 running sum (profiles/r6_gpu_tests.log, profiles/r6_eval_fixture_tables.txt).
// Batches of 8 frames and 32 column-block partials per thread: one batch each at 64 frames of the SMAL mesh (as a plain loop,
// every few additions waited for their own trip to memory: ten trips in a role that is one chain of latencies).
constexpr int kAsmFr = 8, kAsmPa = 32, kAsmLs = 4;
struct BetaOperands { float fv[kAsmFr], pv[kAsmPa], prior; };
__device__ __forceinline__ void asm_beta_fetch(const AssembleArgs& a, int s, int b0, BetaOperands& o) {
  const int t = threadIdx.x, slice = min(t / 20, 11), b = min(b0 + t % 20, a.nb - 1);
  const int nlo = a.betas_shared ? 0 : s, nhi = a.betas_shared ? a.M : s + 1, nparts = a.nblk_beta * a.ngrp_beta;
  const float* pj = a.dbetaJ + b;
  const float* pp = a.dbeta_part + (size_t)s * nparts * a.nb + b;
#pragma unroll
  for (int u = 0; u < kAsmFr; ++u) o.fv[u] = pj[(size_t)min(nlo + slice + 12 * u, nhi - 1) * a.NBall];
#pragma unroll
  for (int u = 0; u < kAsmPa; ++u) o.pv[u] = pp[(size_t)min(slice + 12 * u, nparts - 1) * a.nb];
  o.prior = (a.gb_prior && s == 0) ? a.gb_prior[min(b0 + min(t, 19), a.nb - 1)] : 0.f;     // thread t < 20: the prior's share of direction b0 + t
}
__device__ __forceinline__ void asm_beta_slices(const AssembleArgs& a, int s, int b0, BetaOperands& o, double (*bsum)[32]) {
  const int t = threadIdx.x, bl = t % 20, slice = t / 20, b = b0 + bl;
  if (slice < 12 && b < a.nb) {
    const int nlo = a.betas_shared ? 0 : s, nhi = a.betas_shared ? a.M : s + 1, nparts = a.nblk_beta * a.ngrp_beta;
    const float* pj = a.dbetaJ + b;
    const float* pp = a.dbeta_part + (size_t)s * nparts * a.nb + b;
    double acc = 0.0;
    for (int n0 = nlo + slice; n0 < nhi; n0 += 12 * kAsmFr) {
#pragma unroll
      for (int u = 0; u < kAsmFr; ++u)
        if (n0 + 12 * u < nhi) acc += (double)o.fv[u];
      if (n0 + 12 * kAsmFr < nhi) {
#pragma unroll
        for (int u = 0; u < kAsmFr; ++u) o.fv[u] = pj[(size_t)min(n0 + 12 * (kAsmFr + u), nhi - 1) * a.NBall];
      }
    }
    for (int k0 = slice; k0 < nparts; k0 += 12 * kAsmPa) {
#pragma unroll
      for (int u = 0; u < kAsmPa; ++u)
        if (k0 + 12 * u < nparts) acc += (double)o.pv[u];
      if (k0 + 12 * kAsmPa < nparts) {
#pragma unroll
        for (int u = 0; u < kAsmPa; ++u) o.pv[u] = pp[(size_t)min(k0 + 12 * (kAsmPa + u), nparts - 1) * a.nb];
      }
    }
    bsum[slice][bl] = acc;
  }
}
// ... behind the barrier: thread t < 20 returns direction b0 + t (valid where b0 + t < a.nb)
__device__ __forceinline__ float asm_beta_total(const AssembleArgs& a, int s, int b0, const BetaOperands& o, double (*bsum)[32]) {
  const int t = threadIdx.x;
  double tot = 0.0;
  if (t < 20 && b0 + t < a.nb) {
    for (int sl = 0; sl < 12; ++sl) tot += bsum[sl][t];
    if (a.gb_prior && s == 0) tot += (double)o.prior;
  }
  return (float)tot;
}
// d loss / d shared limb scales, likewise: 6 scales x 32 frame slices (in double, like the shape gradient), then thread t < 6
// adds the 32 slices of scale t in a fixed order
struct LsOperands { float lv[kAsmLs], prior; };
__device__ __forceinline__ void asm_ls_fetch(const AssembleArgs& a, LsOperands& o) {
  const int t = threadIdx.x, e = min(t & 7, 5), sl = t >> 3;
#pragma unroll
  for (int u = 0; u < kAsmLs; ++u) o.lv[u] = a.dls[(size_t)min(sl + 32 * u, a.M - 1) * 6 + e];
  o.prior = a.gls_prior ? a.gls_prior[min(t, 5)] : 0.f;
}
__device__ __forceinline__ void asm_ls_slices(const AssembleArgs& a, LsOperands& o, double (*dpart)[8]) {
  const int t = threadIdx.x, e = t & 7, sl = t >> 3;
  double acc = 0.0;
  if (e < 6)
    for (int n0 = sl; n0 < a.M; n0 += 32 * kAsmLs) {
#pragma unroll
      for (int u = 0; u < kAsmLs; ++u)
        if (n0 + 32 * u < a.M) acc += (double)o.lv[u];
      if (n0 + 32 * kAsmLs < a.M) {
#pragma unroll
        for (int u = 0; u < kAsmLs; ++u) o.lv[u] = a.dls[(size_t)min(n0 + 32 * (kAsmLs + u), a.M - 1) * 6 + e];
      }
    }
  dpart[sl][e] = acc;
}
__device__ __forceinline__ float asm_ls_total(const AssembleArgs& a, const LsOperands& o, double (*dpart)[8]) {
  const int t = threadIdx.x;
  double tot = 0.0;
  if (t < 6) {
    for (int i = 0; i < 32; ++i) tot += dpart[i][t];
    if (a.gls_prior) tot += (double)o.prior;
  }
  return (float)tot;
}
// per-frame elements: masks on the axis-angle adjoint (component l of the frame's 105: the global rotation, then the joints);
// the translation's direct part + the vertex blocks' partials
__device__ __forceinline__ float asm_theta_elem(const AssembleArgs& a, int n, int l) {
  const float* mk = (l < 3) ? a.gmask + l : a.rmask + max(l - 3, 0);
  return a.dtheta[(size_t)n * 105 + l] * *mk;
}
__device__ __forceinline__ float asm_grot_elem(const AssembleArgs& a, int n, int e) { return asm_theta_elem(a, n, e); }
__device__ __forceinline__ float asm_jrot_elem(const AssembleArgs& a, int n, int e) { return asm_theta_elem(a, n, 3 + e); }
__device__ __forceinline__ float asm_trans_elem(const AssembleArgs& a, int n, int e) {
  double acc = a.dtr_direct ? (double)a.dtr_direct[n * 3 + e] : 0.0;     // (the vertex blocks' partials cancel too: in double)
#pragma unroll 16
  for (int vt = 0; vt < a.nvt; ++vt) acc += (double)a.dtr_part[((size_t)vt * a.M + n) * 3 + e];
  return (float)acc;
}

// ------------------------------------------------------------------------------------------------
// K0: shape blend + rest joints
// ------------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------------
// K1: per-frame pose: Rodrigues, limb scales, kinematic chain, skinning transforms, pose feature
// ------------------------------------------------------------------------------------------------
// K0+K1a in one launch: per-frame pose blocks (masked axis-angles -> Rodrigues -> limb scales -> kinematic chain by
// tree depth -> A_j and the pose feature; the rest joints J = Jt + JS beta are formed in place), the shape-blend
// blocks (v_shaped = v_template + shapedirs beta) and, for the fitter, the shape-prior block.  The three parts are
// independent and each is latency-bound: one launch instead of four.
struct HeadArgs {
  int M, Mp, nb, betas_stride, ls_stride, nshape_x, nshape, prior_D, prior_use_ls;
  const float* betas;        // [nbs][betas_stride]
  const float* theta_in;     // [M][105] ready-made (component API) or null
  const float* grot;         // [M][3], jrot [M][102], masks: used when theta_in is null
  const float* jrot;
  const float* gmask;
  const float* rmask;
  const float* logscale;     // [.][6] or null
  float* theta;              // [M][105] out (masked axis-angles)
  float* Jrest;              // [nbs][105] out
  float* v_shaped;           // [nbs][3][Vp] out
  float *Rm, *Gm, *scm, *Am, *pfT;
  const float* prior_prec;   // shape prior (null: none)
  const float* prior_mean;
  float prior_w;
  float *prior_loss, *prior_gb, *prior_gls;
  // SMAL.__call__ options of the component API (smal_torch.py:99-122,132-133)
  const float* Rs_in;        // [M][35][9] rotation matrices given instead of axis-angles, or null
  const float* joff;         // [M][joff_stride] rest-joint offsets = J_regressor^T (per-frame template offset), or null
  int joff_stride;
  const float* voff;         // [M][3][Vp] per-frame template offset (del_v + v_template override), or null
};

// The pending optimiser step (PendingStep, smalfit_fit_run): what assemble_kernel + adam_segments_kernel would have done behind the
// previous evaluation, done here by the first -- and, for the per-frame tensors, the only -- reader of the stepped values.
// A block requests everything the step reads in one go (pending_shared_fetch, pending_jrot_fetch, the caller's own operands),
// computes, and meets at two barriers: slices of the shared gradients | their totals and Adam | the stepped values in LDS.
constexpr int kPendingNb = 20;    // shape directions of the fitter (smalfit_fit_eval); the pending path holds a thread's operands in registers
// LDS the stepped / staged shared parameters are handed over in: betas, then the (shared or this frame's) limb scales
struct HeadShared {
  float beta[kPendingNb], ls[8], grot[4];
  double bsum[12][32], dpart[32][8];
};
struct AdamOperands { float p, m, v; };     // element i of a tensor as the step finds it
__device__ __forceinline__ AdamOperands pending_load(const PendingStep& p, const PendingTensor& T, int i) {
  return AdamOperands{T.p_in[i], p.fresh ? 0.f : T.m_in[i], p.fresh ? 0.f : T.v_in[i]};
}
__device__ __forceinline__ float pending_adam(const PendingStep& p, const PendingTensor& T, int i, const AdamOperands& o, float gi, bool store) {
  float mi, vi, pv = o.p;
  adam_update(gi, o.m, o.v, p.b1, p.b2, p.eps, p.step_size, p.bc2_sqrt, mi, vi, pv);
  if (store) { T.m[i] = mi; T.v[i] = vi; T.p[i] = pv; T.g[i] = gi; }
  return pv;
}
// the shared tensors (every block of the launch, redundantly): operands of the gradients' slices and, in the threads that will
// step them, the parameters as they are
struct SharedOperands { AdamOperands beta, ls; BetaOperands bo; LsOperands lo; };
// (an untrained tensor's PendingTensor names the tensor itself as p_in / m_in / v_in: the same loads fetch it as it is.  n: the
// frame whose limb scales are staged when they are per frame -- their step, if any, is pending_frame_extras')
__device__ __forceinline__ void pending_shared_fetch(const PendingStep& p, const HeadArgs& a, int n, SharedOperands& o) {
  const int t = threadIdx.x;
  o.beta = pending_load(p, p.betas, min(t, 19));
  if (p.betas.train) asm_beta_fetch(p.g, 0, 0, o.bo);
  if (a.logscale) {
    if (p.g.ls_shared) o.ls = pending_load(p, p.ls, min(t, 5));
    else if (!p.ls.train) o.ls.p = a.logscale[(size_t)n * a.ls_stride + min(t, 5)];
    if (p.ls.train && p.g.ls_shared) asm_ls_fetch(p.g, o.lo);
  }
}
__device__ __forceinline__ void pending_shared_slices(const PendingStep& p, SharedOperands& o, HeadShared& sh) {
  if (p.betas.train) asm_beta_slices(p.g, 0, 0, o.bo, sh.bsum);
  if (p.ls.train && p.g.ls_shared) asm_ls_slices(p.g, o.lo, sh.dpart);
}
// behind the first barrier: totals, Adam, and the values every thread of the block reads from LDS after one more barrier; block
// 0 stores
__device__ __forceinline__ void pending_shared_step(const PendingStep& p, const HeadArgs& a, const SharedOperands& o, HeadShared& sh) {
  const int t = threadIdx.x;
  const bool store = blockIdx.x == 0;
  if (p.betas.train) {
    const float gi = asm_beta_total(p.g, 0, 0, o.bo, sh.bsum);
    if (t < 20) sh.beta[t] = pending_adam(p, p.betas, t, o.beta, gi, store);
  } else if (t < 20) {
    sh.beta[t] = o.beta.p;
  }
  if (a.logscale && (p.g.ls_shared || !p.ls.train)) {
    if (p.ls.train) {
      const float gi = asm_ls_total(p.g, o.lo, sh.dpart);
      if (t < 6) sh.ls[t] = pending_adam(p, p.ls, t, o.ls, gi, store);
    } else if (t < 6) {
      sh.ls[t] = o.ls.p;
    }
  }
}
// frame n's own parameters.  Thread 3 <= l < 105 owns joint-rotation component l - 3: its operands, requested unconditionally
// (an untrained tensor's PendingTensor names the tensor itself as p_in / m_in / v_in: readable) ...
struct ThetaOperands { AdamOperands ao; float gi; };
__device__ __forceinline__ void pending_jrot_fetch(const PendingStep& p, int n, ThetaOperands& o) {
  const int l = max(min((int)threadIdx.x, 104), 3);
  o.ao = pending_load(p, p.jrot, n * 102 + (l - 3));
  o.gi = asm_theta_elem(p.g, n, l);
}
// ... and its step: returns the component (unmasked) as the pose block goes on with it
__device__ __forceinline__ float pending_jrot_step(const PendingStep& p, int n, const ThetaOperands& o) {
  const int l = threadIdx.x;
  if (l >= 3 && l < 105 && p.jrot.train) return pending_adam(p, p.jrot, n * 102 + (l - 3), o.ao, o.gi, true);
  return o.ao.p;
}
// the frame's small tensors, three or six threads each in the waves that own no joint rotation: the translation in the third, the
// global rotation (handed to threads l < 3 through LDS: they meet two barriers before they need it) and the frame's limb scales,
// when those are per frame, in the fourth
__device__ __forceinline__ void pending_frame_extras(const PendingStep& p, int n, HeadShared& sh) {
  const int l = threadIdx.x;
  if (l >= 128 && l < 131) {
    const int i = n * 3 + (l - 128);
    if (p.trans.train) pending_adam(p, p.trans, i, pending_load(p, p.trans, i), asm_trans_elem(p.g, n, l - 128), true);
  } else if (l >= 224 && l < 227) {
    const int i = n * 3 + (l - 224);
    const AdamOperands ao = pending_load(p, p.grot, i);
    sh.grot[l - 224] = p.grot.train ? pending_adam(p, p.grot, i, ao, asm_theta_elem(p.g, n, l - 224), true) : ao.p;
  } else if (l >= 192 && l < 198) {
    if (p.ls.train && !p.g.ls_shared) { const int i = n * 6 + (l - 192); sh.ls[l - 192] = pending_adam(p, p.ls, i, pending_load(p, p.ls, i), p.g.dls[i], true); }
  }
}

template <bool kPending>
__device__ __forceinline__ void
pose_block(const ModelDev& m, const HeadArgs& a, int n, const PendingStep* pend, HeadShared* sh) {
  __shared__ float th[105];
  __shared__ float R[35][9];
  __shared__ float sc[35][3], isc[35][3];
  __shared__ __attribute__((aligned(16))) float G[35][12];
  __shared__ float J[35][3];
  __shared__ unsigned char t_lvl_off[36], t_lvl_joint[36], t_par[36];
  __shared__ unsigned char t_pj[kTreeMaxPass][8], t_pp[kTreeMaxPass][8];
  const int l = threadIdx.x, M = a.M;
  PHASE_MARK(ph0);
  const TreeLevels& tl = m.tree;
  if (l < 36) {
    t_lvl_off[l] = tl.lvl_off[l];
    if (l < 35) { t_lvl_joint[l] = tl.lvl_joint[l]; t_par[l] = (unsigned char)max(m.parents[l], 0); }
  }
  if (l >= 128 && l < 128 + kTreeMaxPass * 8) { const int q = l - 128; t_pj[q >> 3][q & 7] = tl.pass_joint[q >> 3][q & 7]; t_pp[q >> 3][q & 7] = tl.pass_parent[q >> 3][q & 7]; }
  const int nlev = tl.nlev;
  float tv_pend = 0.f, js_pre[kPendingNb], jt_pre = 0.f, mv_pre = 0.f;
  int idx_pre = 0;
  if constexpr (kPending) {
    // the pending step (fitter path: parameters given as grot / jrot, shared betas of kPendingNb directions).  What the thread
    // reads of the model and the masks is requested first: behind the step's barriers it would be a second trip to memory.
    // Then the slices of the shared gradients and this frame's own elements before the barrier, the shared totals behind it,
    // and one more barrier before anyone reads the stepped values
    const int lc = min(l, 104);
    idx_pre = m.scale_idx[lc]; jt_pre = m.Jt[lc];
    mv_pre = (lc < 3) ? a.gmask[lc] : a.rmask[max(lc - 3, 0)];
#pragma unroll
    for (int b = 0; b < kPendingNb; ++b) js_pre[b] = m.JS[lc * m.NBall + b];
    SharedOperands so;
    ThetaOperands to;
    pending_shared_fetch(*pend, a, n, so);
    pending_jrot_fetch(*pend, n, to);
    pending_frame_extras(*pend, n, *sh);
    tv_pend = pending_jrot_step(*pend, n, to);
    pending_shared_slices(*pend, so, *sh);
    PHASE_MARK(pp1);                    // everything fetched, the frame's own step taken, slices of the shared gradients in LDS
    __syncthreads();
    pending_shared_step(*pend, a, so, *sh);
    PHASE_MARK(pp2);                    // shared totals and their step
    __syncthreads();
    if (l < 3) tv_pend = sh->grot[l];
    PHASE_MARK(pp3);
    PHASE_ADD(PH_HEAD_POSE, 4, ph0, pp1); PHASE_ADD(PH_HEAD_POSE, 5, pp1, pp2); PHASE_ADD(PH_HEAD_POSE, 6, pp2, pp3);   // (parts of phase 0)
  }
  if (l < 105) {
    // operands whose address depends on nothing loaded are requested together, through pointers selected without a branch
    // (a load inside a per-lane condition is a branch plus a wait for everything in flight: tools/isa_loads.py)
    const int lj = max(l - 3, 0);
    const float* tsrc = a.theta_in ? a.theta_in + (size_t)n * 105 + l : ((l < 3) ? a.grot + n * 3 + l : a.jrot + (size_t)n * 102 + lj);
    const float* msrc = a.theta_in ? tsrc : ((l < 3) ? a.gmask + l : a.rmask + lj);
    int idx;
    float tv0, mv, lsv, acc;
    if constexpr (kPending) {
      idx = idx_pre; tv0 = tv_pend; mv = mv_pre; acc = jt_pre;
      lsv = a.logscale ? sh->ls[max(idx, 0)] : 0.f;
    } else {
      idx = m.scale_idx[l];
      tv0 = *tsrc; mv = *msrc;
      acc = m.Jt[l];
      lsv = a.logscale ? a.logscale[(size_t)n * a.ls_stride + max(idx, 0)] : 0.f;   // (its address needs idx: second trip)
    }
    const float tv = a.theta_in ? tv0 : tv0 * mv;
    th[l] = tv;
    a.theta[(size_t)n * 105 + l] = tv;
    // rest joint coordinate l of this frame's shape
    if constexpr (kPending) {
#pragma unroll
      for (int b = 0; b < kPendingNb; ++b) acc = fmaf(js_pre[b], sh->beta[b], acc);
    } else {
      const float* beta = a.betas + (size_t)(a.betas_stride ? n : 0) * a.betas_stride;
#pragma unroll 10
      for (int b = 0; b < a.nb; ++b) acc = fmaf(m.JS[l * m.NBall + b], beta[b], acc);
    }
    if (a.joff) acc += a.joff[(size_t)n * a.joff_stride + l];
    J[l / 3][l % 3] = acc;
    if (a.betas_stride || n == 0) a.Jrest[(size_t)(a.betas_stride ? n : 0) * 105 + l] = acc;
    const float sv = (a.logscale != nullptr && idx >= 0) ? expf(lsv) : 1.0f;
    sc[l / 3][l % 3] = sv; isc[l / 3][l % 3] = 1.0f / sv;
    a.scm[(size_t)n * 105 + l] = sv;
  }
  __syncthreads();
  PHASE_MARK(ph1);                      // operands in LDS
  if (l < 35) {
    const float t3[3] = {th[l * 3], th[l * 3 + 1], th[l * 3 + 2]};
    float r[9];
    if (a.Rs_in) {
#pragma unroll
      for (int e = 0; e < 9; ++e) r[e] = a.Rs_in[((size_t)n * 35 + l) * 9 + e];
    } else {
      rodrigues_fwd(t3, r);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) { R[l][e] = r[e]; a.Rm[((size_t)n * 35 + l) * 9 + e] = r[e]; }
  }
  __syncthreads();
  PHASE_MARK(ph2);                      // Rodrigues
  for (int idx = l; idx < 306; idx += 256) {
    const int j = idx / 9 + 1, e = idx % 9;
    a.pfT[(size_t)idx * a.Mp + n] = R[j][e] - ((e & 3) == 0 ? 1.0f : 0.0f);
  }
  if (l < 12) {
    const int r = l >> 2, c = l & 3;
    G[0][l] = (c < 3) ? R[0][r * 3 + c] : J[0][r];
  }
  // the tree by depth: 12 lanes per joint of the level, first wave only (its LDS operations complete in order)
  if (l < 64 && tl.fast) {
    // Round 6: the walk is a chain of dependent LDS trips, so everything that does not depend on the walk itself is read a pass
    // AHEAD -- the lane's joint and parent of the next pass (TreeLevels::pass_*: one byte pair per pass and slot) and the three
    // factors its element multiplies the parent's row with (a column of S_p^-1 R_i S_i, or J_i - J_p) -- and a pass is one
    // 16-byte read of the parent's row, three multiply-adds and one write (until then: level offsets -> joint -> parent ->
    // operands, five dependent trips per pass; 8.2 k cycles of the block's 14.5 k, profiles/r6_lbs_phase_breakdown.txt).  The loop
    // stays rolled: one wave running straight-line code once pays an instruction-cache miss per line (the unrolled form of this
    // walk was slower than the table-driven one).  The two walks share no code: this one forms the factors (a column of S_p^-1 R_i S_i,
    // or J_i - J_p) a pass ahead and a pass is three multiply-adds on the parent's row, the table-driven loop below forms them in place.
    // Written out they are the same products folded in the same order, but nothing enforces that and no test compares the two walks'
    // bits (a tree takes one or the other, smalfit_plan.h: tree_levels) -- each is held to the float64 oracle on trees that reach it,
    // this one at exactly kTreeMaxPass passes too (tests/test_gpu_model_forms.py).
    const int slot_c = min(l / 12, 7), e = l % 12, r = e >> 2, c = e & 3, cc = min(c, 2);
    const int npass = tl.npass;
    auto fetch = [&](int k, int& ijp, float (&kc)[3]) {
      // (branch-free: idle slots -- columns 5..7 of the table -- read 255; every operand comes from a clamped index)
      const int i = t_pj[k][slot_c], p = t_pp[k][slot_c];
      const bool live = i != 255;
      ijp = live ? (i | (p << 8)) : -1;
      const int ii = live ? i : 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float rot = R[ii][q * 3 + cc] * sc[ii][cc] * isc[p][q], dj = J[ii][q] - J[p][q];
        kc[q] = (c < 3) ? rot : dj;
      }
    };
    int ijp_n;
    float kc_n[3];
    fetch(0, ijp_n, kc_n);
#pragma unroll 1
    for (int k = 0; k < npass; ++k) {
      const int ijp = ijp_n;
      const float k0 = kc_n[0], k1 = kc_n[1], k2 = kc_n[2];
      fetch(min(k + 1, kTreeMaxPass - 1), ijp_n, kc_n);          // the next pass's operands travel while this one computes
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (ijp >= 0) {
        const int i = ijp & 255, p = ijp >> 8;
        const float4 g = *reinterpret_cast<const float4*>(&G[p][r * 4]);
        float acc = (c < 3) ? 0.f : g.w;
        acc = fmaf(g.x, k0, acc);
        acc = fmaf(g.y, k1, acc);
        acc = fmaf(g.z, k2, acc);
        G[i][e] = acc;
      }
    }
  } else if (l < 64) {
    const int slot = l / 12, e = l % 12;
    for (int L = 1; L < nlev; ++L) {
      const int j0 = t_lvl_off[L], nj = t_lvl_off[L + 1] - j0;
      for (int base = 0; base < nj; base += 5) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (slot < 5 && base + slot < nj) {
          const int i = t_lvl_joint[j0 + base + slot], p = t_par[i];
          const int r = e >> 2, c = e & 3;
          float acc;
          if (c < 3) {
            acc = 0.f;
#pragma unroll
            for (int q = 0; q < 3; ++q) acc = fmaf(G[p][r * 4 + q], R[i][q * 3 + c] * sc[i][c] * isc[p][q], acc);
          } else {
            acc = G[p][r * 4 + 3];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc = fmaf(G[p][r * 4 + q], J[i][q] - J[p][q], acc);
          }
          G[i][e] = acc;
        }
      }
    }
  }
  __syncthreads();
  PHASE_MARK(ph3);                      // tree walk
  for (int idx = l; idx < 35 * 12; idx += 256) {
    const int j = idx / 12, e = idx % 12, r = e >> 2, c = e & 3;
    float val = G[j][e];
    if (c == 3) {
#pragma unroll
      for (int q = 0; q < 3; ++q) val = fmaf(-G[j][r * 4 + q], J[j][q], val);
    }
    a.Am[(size_t)n * 420 + idx] = val;
    a.Gm[(size_t)n * 420 + idx] = G[j][e];
  }
  (void)M;
  PHASE_MARK(ph4);
  PHASE_ADD(PH_HEAD_POSE, 0, ph0, ph1); PHASE_ADD(PH_HEAD_POSE, 1, ph1, ph2); PHASE_ADD(PH_HEAD_POSE, 2, ph2, ph3); PHASE_ADD(PH_HEAD_POSE, 3, ph3, ph4);
  PHASE_END(PH_HEAD_POSE, ph0, ph4);
}

// One shape-prior term by one wave: loss = w mean_c(r_c^2) with r = (x - mean) prec, and its gradient 2 w / D (prec r) wrt x
// (entries 0..19 of x are betas, the rest log scales).  xm is lane's x - mean (lanes >= D: unused), xs / rs two LDS rows of 32 the
// wave owns.  prec is read through a pointer (global memory or an LDS copy; loops rolled to D), or -- kHeld -- from the lane's
// column pcol[r] = prec[r][lane] and row prow[c] = prec[lane][c] held in registers (26 entries, loops unrolled and guarded by D).
// The shared prior of lbs_head_kernel, the step kernel's and the per-image terms of prior_frames_block are all this function,
// so one image gives the bits a one-frame shared fit gives.
template <bool kHeld>
__device__ __forceinline__ void shape_prior_term(float xm, int lane, int D, float* xs, float* rs, const float* prec, const float* pcol,
                                                 const float* prow, float w, bool use_ls, float* loss, float* gb, float* gls) {
  if (lane < D) xs[lane] = xm;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  float lv = 0.f;
  if (lane < D) {
    float acc = 0.f;
    if constexpr (kHeld) {
#pragma unroll
      for (int r = 0; r < 26; ++r) if (r < D) acc = fmaf(xs[r], pcol[r], acc);
    } else {
      for (int r = 0; r < D; ++r) acc = fmaf(xs[r], prec[r * D + lane], acc);
    }
    rs[lane] = acc;
    lv = acc * acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  lv = wave_sum(lv);
  if (lane == 0) *loss = w * lv / (float)D;
  if (lane < D) {
    float acc = 0.f;
    if constexpr (kHeld) {
#pragma unroll
      for (int c = 0; c < 26; ++c) if (c < D) acc = fmaf(rs[c], prow[c], acc);
    } else {
      for (int c = 0; c < D; ++c) acc = fmaf(rs[c], prec[lane * D + c], acc);
    }
    acc *= 2.0f * w / (float)D;
    if (lane < 20) gb[lane] = acc; else if (use_ls) gls[lane - 20] = acc;
  }
}

// Shape prior of independent images: w mean_c(((x_n - mean) prec)_c ^2) with x_n = [betas_n | log scales_n], one term per frame.
// A block takes kPriorFrames frames, one wave every fourth of them; prec and mean are staged in LDS once per block (2.7 KB; the
// shared-shape block below reads them from memory once, here that would be once per frame).  Each frame's term is the shared
// block's shape_prior_term, so one image gives the bits a one-frame shared fit gives.  Each frame's loss is a plain store; who
// adds them up (assemble_kernel) does so in a fixed order.
// Its arguments travel beside HeadArgs (lbs_head_kernel only): the step kernel's argument block stays what it is.
constexpr int kPriorFrames = 16;
struct PriorFrames {
  int on, gb_stride, gls_stride;   // on: ceil(M / kPriorFrames) blocks behind the shape blocks evaluate one prior term per frame
  float* loss;                     // [M]: frame n's term
  float *gb, *gls;                 // rows of gb_stride / gls_stride floats: its gradient wrt betas_n / log scales_n
};
__device__ __forceinline__ void prior_frames_block(const HeadArgs& a, const PriorFrames& pf, int pb) {
  __shared__ float prec[26 * 26], mean[32], xs[4][32], rs[4][32];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, D = a.prior_D;
  for (int i = t; i < D * D; i += 256) prec[i] = a.prior_prec[i];
  if (t < D) mean[t] = a.prior_mean[t];
  __syncthreads();
  const int n_end = min((pb + 1) * kPriorFrames, a.M);
  for (int n = pb * kPriorFrames + w; n < n_end; n += 4) {       // (n is uniform over the wave)
    float xm = 0.f;
    if (lane < D)
      xm = ((lane < 20) ? a.betas[(size_t)n * a.betas_stride + lane] : a.logscale[(size_t)n * a.ls_stride + lane - 20]) - mean[lane];
    shape_prior_term<false>(xm, lane, D, xs[w], rs[w], prec, nullptr, nullptr, a.prior_w, a.prior_use_ls, pf.loss + n,
                            pf.gb + (size_t)n * pf.gb_stride, pf.gls + (size_t)n * pf.gls_stride);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the next frame of this wave overwrites xs / rs
    __builtin_amdgcn_wave_barrier();
  }
}

template <bool kPending>
__device__ __forceinline__ void
head_block(const ModelDev& m, const HeadArgs& a, const PendingStep* pend, HeadShared* sh, const PriorFrames* pf = nullptr) {
  int blk = blockIdx.x;
  if (blk < a.M) { pose_block<kPending>(m, a, blk, pend, sh); return; }
  blk -= a.M;
  if constexpr (kPending) {
    // shape and prior blocks read the shared parameters: they take the shared part of the pending step too (bit-equal copies),
    // with their own operands requested before its barriers (shared betas: one shape set, a.nshape == a.nshape_x)
    const int Vp = m.Vp, v = min(blk, a.nshape_x - 1) * 256 + threadIdx.x, t = threadIdx.x, D = a.prior_D;
    const bool shape = blk < a.nshape;
    float vt_pre[3], sd_pre[3][kPendingNb], pcol[26], prow[26];
    if (shape) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        vt_pre[c] = m.vt[c * Vp + v];
#pragma unroll
        for (int b = 0; b < kPendingNb; ++b) sd_pre[c][b] = m.sd[((size_t)b * 3 + c) * Vp + v];
      }
    } else if (a.prior_prec) {
      const int tc = min(t, D - 1);
#pragma unroll
      for (int r = 0; r < 26; ++r) { const int rc = min(r, D - 1); pcol[r] = a.prior_prec[rc * D + tc]; prow[r] = a.prior_prec[tc * D + rc]; }
    }
    const float pmean = (!shape && a.prior_prec) ? a.prior_mean[min(t, D - 1)] : 0.f;
    SharedOperands so;
    pending_shared_fetch(*pend, a, 0, so);
    pending_shared_slices(*pend, so, *sh);
    __syncthreads();
    pending_shared_step(*pend, a, so, *sh);
    __syncthreads();
    if (shape) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = vt_pre[c];
#pragma unroll
        for (int b = 0; b < kPendingNb; ++b) acc = fmaf(sh->beta[b], sd_pre[c][b], acc);
        if (a.voff) acc += a.voff[(size_t)c * Vp + v];
        a.v_shaped[(size_t)c * Vp + v] = acc;
      }
      return;
    }
    // shape prior, as below with the operands held
    if (a.prior_prec && t < 64) {
      __shared__ float x[32], res[32];
      float xm = 0.f;
      if (t < D) xm = ((t < 20) ? sh->beta[t] : sh->ls[t - 20]) - pmean;
      shape_prior_term<true>(xm, t, D, x, res, nullptr, pcol, prow, a.prior_w, a.prior_use_ls, a.prior_loss, a.prior_gb, a.prior_gls);
    }
    return;
  }
  if (blk < a.nshape) {
    PHASE_MARK(ps0);
    const int s = blk / a.nshape_x;
    const float* beta = a.betas + (size_t)s * a.betas_stride;
    const int v = (blk % a.nshape_x) * 256 + threadIdx.x;
    const int Vp = m.Vp;
    if (v < Vp) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = m.vt[c * Vp + v];
#pragma unroll 10
        for (int b = 0; b < a.nb; ++b) acc = fmaf(beta[b], m.sd[((size_t)b * 3 + c) * Vp + v], acc);
        if (a.voff) acc += a.voff[((size_t)s * 3 + c) * Vp + v];
        a.v_shaped[((size_t)s * 3 + c) * Vp + v] = acc;
      }
    }
    PHASE_MARK(ps1);
    PHASE_END(PH_HEAD_SHAPE, ps0, ps1);
    return;
  }
  if (pf && pf->on) { prior_frames_block(a, *pf, blk - a.nshape); return; }
  // shape prior: w_eff * mean_c( ((x - mean) prec)_c ^2 ), x = [betas | log scales]
  if (a.prior_prec && threadIdx.x < 64) {
    __shared__ float x[32], res[32];
    const int t = threadIdx.x, D = a.prior_D;
    float xm = 0.f;
    if (t < D) xm = ((t < 20) ? a.betas[t] : a.logscale[t - 20]) - a.prior_mean[t];
    shape_prior_term<false>(xm, t, D, x, res, a.prior_prec, nullptr, nullptr, a.prior_w, a.prior_use_ls, a.prior_loss, a.prior_gb, a.prior_gls);
  }
}

__global__ void __launch_bounds__(256)
lbs_head_kernel(ModelDev m, HeadArgs a) { head_block<false>(m, a, nullptr, nullptr); }

// ... for independent images: the prior blocks evaluate one term per frame (prior_frames_block)
__global__ void __launch_bounds__(256)
lbs_head_images_kernel(ModelDev m, HeadArgs a, PriorFrames pf) { head_block<false>(m, a, nullptr, nullptr, &pf); }

// ... carrying the optimiser step the previous evaluation left pending (smalfit_fit_run)
__global__ void __launch_bounds__(256)
lbs_head_step_kernel(ModelDev m, HeadArgs a, PendingStep p) {
  __shared__ HeadShared sh;
  head_block<true>(m, a, &p, &sh);
}

// theta[n][0] = global_rotation[n] * gmask ; theta[n][1+j] = joint_rotations[n][j] * rmask[j]
__global__ void build_theta_kernel(int M, const float* __restrict__ grot, const float* __restrict__ jrot,
                                   const float* __restrict__ gmask, const float* __restrict__ rmask,
                                   float* __restrict__ theta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * 105) return;
  const int n = i / 105, e = i % 105;
  theta[i] = (e < 3) ? grot[n * 3 + e] * gmask[e] : jrot[n * 102 + (e - 3)] * rmask[e - 3];
}

// ------------------------------------------------------------------------------------------------
// K2: pose blend + skinning + camera transform.  block = 64 vertices x FR frames, 4 waves split K=306
// ------------------------------------------------------------------------------------------------
// K1b (MFMA form): pose blend as a skinny GEMM on the matrix cores, then skinning + camera.
//   blend[n][c] = sum_k pf[n][k] * pd[k][c]   (n: 16 frames, c: 16 vertices x {x,y,z}, k: 306 pose features)
// One wave owns 16 vertices x 16 frames; v_mfma_f32_16x16x4_f32 (exact f32: an fmaf chain) takes
// A[i = lane & 15][k = lane >> 4] = pfT[k][n0 + i] and B[k = lane >> 4][j = lane & 15] = pd[k][a][v0 + j], both read
// straight from global memory as 64-byte segments; D[row = 4 (lane >> 4) + r][col = lane & 15], so a lane ends up with
// x, y, z of ONE vertex for FOUR frames -- exactly what the skinning step needs.  77 k-steps x 3 MFMAs per wave.
typedef float f32x4 __attribute__((ext_vector_type(4)));
// Round 6, the SPLIT form for evaluations of few frames (a rank of a multi-GPU fit): the K = 306 contraction is split over four
// waves (in the wide form below a wave owns 16 vertices and walks all 77 k-steps: 231 dependent matrix instructions behind seven
// batches of operand loads -- 5.9 us of a workgroup's 10.4, and only 64 workgroups at 8 frames: profiles/r6_lbs_phase_breakdown.txt).
// What the two matrix-core forms request at their top besides the GEMM operands, for a workgroup of kThreads threads: the 16
// frames' skinning transforms (one contiguous run of A as float4: clamped reads in fetch, zero fill of frames past M in stage)
// and the first min(Kw, 8) ELL weights of the lane's vertex (clamped: entries past Kw repeat the last and are never used).
template <int kThreads>
struct SkinSide {
  static constexpr int kStage = (16 * 105 + kThreads - 1) / kThreads;    // float4 words of the transforms a thread stages
  float4 a_stage[kStage];
  int wj[8], Kw, nvalid;
  float wv[8];
  __device__ __forceinline__ void fetch(const ModelDev& m, int M, int n0, int v, const float* __restrict__ Am) {
    nvalid = min(16, M - n0) * 105;                   // float4 words of A that exist
    const float4* src = reinterpret_cast<const float4*>(Am + (size_t)n0 * 420);
#pragma unroll
    for (int r = 0; r < kStage; ++r) a_stage[r] = src[min((int)threadIdx.x + kThreads * r, nvalid - 1)];
    Kw = min(m.Kw, 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ee = max(min(e, Kw - 1), 0);
      wj[e] = m.w_j[ee * m.Vp + v];
      wv[e] = m.w_val[ee * m.Vp + v];
    }
  }
  __device__ __forceinline__ void stage(float (*As)[420]) const {
    float4* dst = reinterpret_cast<float4*>(&As[0][0]);
#pragma unroll
    for (int r = 0; r < kStage; ++r) {
      const int i4 = threadIdx.x + kThreads * r;
      if (i4 < 16 * 105) dst[i4] = (i4 < nvalid) ? a_stage[r] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
};

// The finish of one (vertex v, frame n) pair, the same in all three skin forms: store the posed rest vertex vp, blend the 12
// entries of the transform from the ELL weights and the frame's staged transforms Af = As[f], apply it and store verts, project
// (+ tr) and store proj.  The first min(Kw, kHeld) weights are the caller's registers (wj, wv; Kw_held = min(Kw, kHeld)), the
// rest are read from memory: kHeld = 8 in the matrix-core forms, 0 in the plain one.
template <int kHeld>
__device__ __forceinline__ void skin_finish(const ModelDev& m, int v, int n, const float (&vp)[3], const float* Af, const int* wj,
                                            const float* wv, int Kw_held, const float* tr, float* __restrict__ vposed,
                                            float* __restrict__ verts, float* __restrict__ proj) {
  const int Vp = m.Vp;
#pragma unroll
  for (int a = 0; a < 3; ++a) vposed[((size_t)n * 3 + a) * Vp + v] = vp[a];
  float T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = 0.f;
  auto blend = [&](int j, float wx) {
    const float* A = Af + j * 12;
#pragma unroll
    for (int c = 0; c < 12; ++c) T[c] = fmaf(wx, A[c], T[c]);
  };
#pragma unroll
  for (int e = 0; e < kHeld; ++e)
    if (e < Kw_held) blend(wj[e], wv[e]);
  for (int e = kHeld; e < m.Kw; ++e) blend(m.w_j[e * Vp + v], m.w_val[e * Vp + v]);     // (models with more weights per vertex than are held)
  float o[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = fmaf(T[a * 4], vp[0], fmaf(T[a * 4 + 1], vp[1], fmaf(T[a * 4 + 2], vp[2], T[a * 4 + 3])));
    verts[((size_t)n * 3 + a) * Vp + v] = o[a];
  }
  float xn, yn, zv;
  world_to_ndc(o[0] + tr[0], o[1] + tr[1], o[2] + tr[2], xn, yn, zv);
  proj[((size_t)n * 3 + 0) * Vp + v] = xn;
  proj[((size_t)n * 3 + 1) * Vp + v] = yn;
  proj[((size_t)n * 3 + 2) * Vp + v] = zv;
}

// Four waves own 16 vertices x 16 frames (kSkinGroups such groups per workgroup share the frames' staged transforms);
// wave w takes k-steps [20 w, 20 w + 20) -- ONE batch of operand loads, 60 matrix instructions -- the four partial tiles meet in LDS
// and are added in wave order (fixed: deterministic), and wave w finishes frame 4 (lane >> 4) + w of its lanes' vertices: one
// (vertex, frame) pair per lane for the skinning instead of four.  Four times the workgroups, a quarter of the chain each.
// (kSkinGroups, kSkinVerts, kSkinThreads: smalfit_plan.h, which sizes the launch by them)
__global__ void __launch_bounds__(kSkinThreads)
skin_mfma_split_kernel(ModelDev m, int M, int Mp, const float* __restrict__ v_shaped, int vs_stride /*0 | 3*Vp*/,
                 const float* __restrict__ pfT, const float* __restrict__ Am, const float* __restrict__ trans,
                 float* __restrict__ vposed, float* __restrict__ verts, float* __restrict__ proj) {
  __shared__ __attribute__((aligned(16))) float As[16][420];
  __shared__ float red[4 * kSkinGroups][12][64];   // [wave][3 planes x 4 rows of the 16 x 16 tile][lane]
  const int Vp = m.Vp;
  PHASE_MARK(pk0);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, w = wid & 3, grp = wid >> 2;
  const int n0 = blockIdx.y * 16;
  const int v = blockIdx.x * kSkinVerts + grp * 16 + (lane & 15);
  const int kq = lane >> 4;
  // everything besides the GEMM operands is requested here, unconditionally (clamped indices, masked where it is used): the 16
  // frames' skinning transforms (one contiguous run of A, as float4), the lane's skinning weights, the rest vertex and the
  // translation of ITS frame
  SkinSide<kSkinThreads> sd;
  sd.fetch(m, M, n0, v, Am);
  const int f = 4 * kq + w, n = n0 + f, nn = min(n, M - 1);  // this lane's frame after the reduction
  float vs_r[3], tr_r[3];
  {
    const float* vs = v_shaped + (size_t)nn * vs_stride;
#pragma unroll
    for (int a = 0; a < 3; ++a) { vs_r[a] = vs[a * Vp + v]; tr_r[a] = trans[nn * 3 + a]; }
  }
  // the wave's share of the contraction: 20 k-steps of 4 pose features (the last wave 17; features 306, 307 do not exist: pfT has
  // two zero rows there and the pd row is clamped, 0 * finite = 0), all operands in flight at once
  constexpr int U = 20;
  const int st0 = w * U;
  const float* pa = pfT + (size_t)kq * Mp + n0 + (lane & 15);
  const float* pb = m.pd + (size_t)kq * 3 * Vp + v;
  float xa[U], x0[U], x1[U], x2[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int st = min(st0 + u, 76);
    xa[u] = pa[(size_t)st * 4 * Mp];
    const float* b = pb + (size_t)(min(st * 4 + kq, 305) - kq) * 3 * Vp;
    x0[u] = b[0]; x1[u] = b[Vp]; x2[u] = b[2 * Vp];
  }
  sd.stage(As);
  PHASE_MARK(pk1);                      // side operands requested and staged
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (st0 + u < 77) {                   // (uniform over the wave)
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u], x0[u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u], x1[u], acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[u], x2[u], acc2, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) { red[wid][r][lane] = acc0[r]; red[wid][4 + r][lane] = acc1[r]; red[wid][8 + r][lane] = acc2[r]; }
  __syncthreads();
  PHASE_MARK(pk2);                      // pose-blend GEMM
  if (n < M) {
    // D[row = 4 (lane >> 4) + r][col = lane & 15]: row r = w of this lane is frame f; the four waves' partials in wave order
    float bl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) bl[a] = ((red[grp * 4][a * 4 + w][lane] + red[grp * 4 + 1][a * 4 + w][lane]) + red[grp * 4 + 2][a * 4 + w][lane]) + red[grp * 4 + 3][a * 4 + w][lane];
    const float vp[3] = {vs_r[0] + bl[0], vs_r[1] + bl[1], vs_r[2] + bl[2]};
    skin_finish<8>(m, v, n, vp, As[f], sd.wj, sd.wv, sd.Kw, tr_r, vposed, verts, proj);
  }
  PHASE_MARK(pk3);
  PHASE_ADD(PH_SKIN, 0, pk0, pk1); PHASE_ADD(PH_SKIN, 1, pk1, pk2); PHASE_ADD(PH_SKIN, 2, pk2, pk3);
  PHASE_END(PH_SKIN, pk0, pk3);
}

// The wide form (rounds 2-5): a workgroup owns 64 vertices x 16 frames, a wave 16 vertices and the whole contraction.  One workgroup
// per CU at 64 frames, where it beats the split form by 2 us (the split form's four-fold workgroups fetch the frames' pose features
// and transforms four times as often); the host picks by the number of workgroups (skin_form of smalfit_plan.h).
__global__ void __launch_bounds__(256)
skin_mfma_kernel(ModelDev m, int M, int Mp, const float* __restrict__ v_shaped, int vs_stride /*0 | 3*Vp*/,
                 const float* __restrict__ pfT, const float* __restrict__ Am, const float* __restrict__ trans,
                 float* __restrict__ vposed, float* __restrict__ verts, float* __restrict__ proj) {
  __shared__ __attribute__((aligned(16))) float As[16][420];
  const int Vp = m.Vp;
  PHASE_MARK(pk0);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = blockIdx.y * 16;
  const int v = blockIdx.x * 64 + w * 16 + (lane & 15);
  const int kq = lane >> 4;
  // Everything the kernel reads besides the GEMM operands is requested HERE, unconditionally (clamped indices, masked where it
  // is used): the 16 frames' skinning transforms (one contiguous run of A, as float4), the lane's skinning weights, and the
  // rest vertex / translation of its four frames.  As conditional loads each of them was compiled into a branch with an
  // s_waitcnt vmcnt(0) behind it -- 7 dependent trips before the first matrix instruction and ~16 after the last
  // (tools/isa_loads.py); now they are in flight together, underneath the GEMM's own operand stream.
  SkinSide<256> sd;
  sd.fetch(m, M, n0, v, Am);
  float vs_r[4][3], tr_r[4][3];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int nn = min(n0 + 4 * kq + r, M - 1);
    const float* vs = v_shaped + (size_t)nn * vs_stride;
#pragma unroll
    for (int a = 0; a < 3; ++a) { vs_r[r][a] = vs[a * Vp + v]; tr_r[r][a] = trans[nn * 3 + a]; }
  }
  sd.stage(As);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0;
  const float* pa = pfT + (size_t)kq * Mp + n0 + (lane & 15);
  const float* pb = m.pd + (size_t)kq * 3 * Vp + v;
  // 77 k-steps of 4 pose features (features 306, 307 do not exist: pfT has two zero rows there and the pd row is
  // clamped, 0 * finite = 0).  With about one wave per SIMD nothing hides a load but the wave itself: operands are
  // fetched a batch of 11 steps ahead (44 loads in flight) into two register sets used alternately.
  constexpr int U = 11, NBATCH = 7;
  static_assert(U * NBATCH == 77, "306 pose features in steps of 4");
  float xa[U], x0[U], x1[U], x2[U], ya[U], y0[U], y1[U], y2[U];
  auto load_batch = [&](int bt, float* A, float* B0, float* B1, float* B2) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int st = bt * U + u;
      A[u] = pa[(size_t)st * 4 * Mp];
      const float* b = pb + (size_t)(min(st * 4 + kq, 305) - kq) * 3 * Vp;
      B0[u] = b[0]; B1[u] = b[Vp]; B2[u] = b[2 * Vp];
    }
  };
  auto mfma_batch = [&](const float* A, const float* B0, const float* B1, const float* B2) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u], B0[u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u], B1[u], acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(A[u], B2[u], acc2, 0, 0, 0);
    }
  };
  PHASE_MARK(pk1);                      // side operands requested and staged
  load_batch(0, xa, x0, x1, x2);
  for (int bt = 0; bt < NBATCH - 1; bt += 2) {
    load_batch(bt + 1, ya, y0, y1, y2);
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(xa, x0, x1, x2);
    __builtin_amdgcn_sched_barrier(0);
    load_batch(bt + 2, xa, x0, x1, x2);
    __builtin_amdgcn_sched_barrier(0);
    mfma_batch(ya, y0, y1, y2);
    __builtin_amdgcn_sched_barrier(0);
  }
  mfma_batch(xa, x0, x1, x2);
  __syncthreads();
  PHASE_MARK(pk2);                      // pose-blend GEMM
  // skinning of this lane's vertex (ELL weights, fetched at the top) for its four frames
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int f = 4 * kq + r, n = n0 + f;
    if (n >= M) break;
    const float vp[3] = {vs_r[r][0] + acc0[r], vs_r[r][1] + acc1[r], vs_r[r][2] + acc2[r]};
    skin_finish<8>(m, v, n, vp, As[f], sd.wj, sd.wv, sd.Kw, tr_r[r], vposed, verts, proj);
  }
  PHASE_MARK(pk3);
  PHASE_ADD(PH_SKIN, 0, pk0, pk1); PHASE_ADD(PH_SKIN, 1, pk1, pk2); PHASE_ADD(PH_SKIN, 2, pk2, pk3);
  PHASE_END(PH_SKIN, pk0, pk3);
}

template <int FR>
__global__ void __launch_bounds__(256)
skin_kernel(ModelDev m, int M, int Mp, const float* __restrict__ v_shaped, int vs_stride /*0 | 3*Vp*/,
            const float* __restrict__ pfT, const float* __restrict__ Am, const float* __restrict__ trans,
            float* __restrict__ vposed, float* __restrict__ verts, float* __restrict__ proj) {
  __shared__ float red[4][FR * 3][64];
  __shared__ float As[FR][420];
  const int Vp = m.Vp;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int v = blockIdx.x * 64 + lane;
  const int n0 = blockIdx.y * FR;
  for (int i = threadIdx.x; i < FR * 420; i += 256) {
    const int f = i / 420;
    As[f][i % 420] = (n0 + f < M) ? Am[(size_t)(n0 + f) * 420 + (i % 420)] : 0.f;
  }
  float acc[FR][3];
#pragma unroll
  for (int f = 0; f < FR; ++f) acc[f][0] = acc[f][1] = acc[f][2] = 0.f;
  const int k0 = (w * 306) / 4, k1 = ((w + 1) * 306) / 4;
  for (int k = k0; k < k1; ++k) {
    const float p0 = m.pd[((size_t)k * 3 + 0) * Vp + v];
    const float p1 = m.pd[((size_t)k * 3 + 1) * Vp + v];
    const float p2 = m.pd[((size_t)k * 3 + 2) * Vp + v];
    const float* pf = pfT + (size_t)k * Mp + n0;     // wave-uniform -> scalar loads
#pragma unroll
    for (int f = 0; f < FR; ++f) {
      const float c = pf[f];
      acc[f][0] = fmaf(c, p0, acc[f][0]);
      acc[f][1] = fmaf(c, p1, acc[f][1]);
      acc[f][2] = fmaf(c, p2, acc[f][2]);
    }
  }
#pragma unroll
  for (int f = 0; f < FR; ++f) {
    red[w][f * 3 + 0][lane] = acc[f][0];
    red[w][f * 3 + 1][lane] = acc[f][1];
    red[w][f * 3 + 2][lane] = acc[f][2];
  }
  __syncthreads();
  // phase 2: wave w finishes frames f = w, w+4, ...
  for (int f = w; f < FR; f += 4) {
    const int n = n0 + f;
    if (n >= M) break;
    const float* vs = v_shaped + (size_t)n * vs_stride;
    float vp[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
      vp[a] = vs[a * Vp + v] + ((red[0][f * 3 + a][lane] + red[1][f * 3 + a][lane]) +
                                (red[2][f * 3 + a][lane] + red[3][f * 3 + a][lane]));
    skin_finish<0>(m, v, n, vp, As[f], nullptr, nullptr, 0, trans + n * 3, vposed, verts, proj);
  }
}

// camera transform only (Renderer called with externally supplied vertices): vin (M,V,3) interleaved
__global__ void project_verts_kernel(int M, int V, int Vp, const float* __restrict__ vin,
                                     float* __restrict__ proj) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
  if (v >= Vp) return;
  float xn = 0.f, yn = 0.f, zv = 1.f;
  if (v < V) {
    const float* p = vin + ((size_t)n * V + v) * 3;
    world_to_ndc(p[0], p[1], p[2], xn, yn, zv);
  }
  proj[((size_t)n * 3 + 0) * Vp + v] = xn;
  proj[((size_t)n * 3 + 1) * Vp + v] = yn;
  proj[((size_t)n * 3 + 2) * Vp + v] = zv;
}

// planar [n][3][Vp] -> interleaved (M,V,3), optionally + per-frame offset
__global__ void planar_to_interleaved_kernel(int M, int V, int Vp, const float* __restrict__ src, int src_stride,
                                             const float* __restrict__ offs, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
  if (i >= V * 3) return;
  const int v = i / 3, a = i % 3;
  float val = src[(size_t)n * src_stride + a * Vp + v];
  if (offs) val += offs[n * 3 + a];
  dst[(size_t)n * V * 3 + i] = val;
}

__global__ void interleaved_to_planar_kernel(int M, int V, int Vp, const float* __restrict__ src,
                                             float* __restrict__ dst) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
  if (v >= Vp) return;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    dst[((size_t)n * 3 + a) * Vp + v] = (v < V) ? src[((size_t)n * V + v) * 3 + a] : 0.f;
}

// ------------------------------------------------------------------------------------------------
// batch_global_rigid_transformation as a free-standing function (component API; the fitting path uses the pose blocks of
// lbs_head_kernel): one thread per frame walks the 35 joints -- a utility, not a hot kernel
// ------------------------------------------------------------------------------------------------
struct Parents35 {
  int p[kJoints];
};

__global__ void global_rigid_kernel(int count, const float* __restrict__ Rs, const float* __restrict__ Js, Parents35 parents,
                                    const float* __restrict__ logscale /* [count][6] or null */,
                                    float* __restrict__ newJ, float* __restrict__ A) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= count) return;
  global_rigid_frame(Rs + (size_t)n * 315, Js + (size_t)n * 105, parents.p, logscale ? logscale + (size_t)n * 6 : nullptr,
                     newJ + (size_t)n * 105, A + (size_t)n * 560);
}

// adjoint of the above, one thread per frame (component entry point, not on the fitting path: the fused chain adjoint is
// chain_bwd_kernel).  scratch: [count][2][35][12] floats
__global__ void global_rigid_bwd_kernel(int count, const float* __restrict__ Rs, const float* __restrict__ Js, Parents35 parents,
                                        const float* __restrict__ logscale, const float* __restrict__ dnewJ,
                                        const float* __restrict__ dA, float* __restrict__ scratch, float* __restrict__ dRs,
                                        float* __restrict__ dJs, float* __restrict__ dlogscale) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= count) return;
  global_rigid_frame_bwd(Rs + (size_t)n * 315, Js + (size_t)n * 105, parents.p, logscale ? logscale + (size_t)n * 6 : nullptr,
                         dnewJ + (size_t)n * 105, dA + (size_t)n * 560, scratch + (size_t)n * 840, scratch + (size_t)n * 840 + 420,
                         dRs + (size_t)n * 315, dJs + (size_t)n * 105, dlogscale ? dlogscale + (size_t)n * 6 : nullptr);
}

// ------------------------------------------------------------------------------------------------
// K3: posed joints (35 regressed through the sparse regressor + 6 landmark vertices)
// ------------------------------------------------------------------------------------------------
// body for joint j of frame n: the first 128 threads of the block do the work (the same split of the regressor row,
// hence the same bits, whether the block has 128 or 256 threads); called by every thread of the block
__device__ __forceinline__ void joints_block(const ModelDev& m, const float* __restrict__ verts, float* __restrict__ joints /*[M][41][3]*/,
                                             int j, int n, float* red /*16 floats of LDS*/) {
  const int Vp = m.Vp;
  const float* vx = verts + (size_t)n * 3 * Vp;
  if (j >= 35) {
    if (threadIdx.x < 3) joints[((size_t)n * 41 + j) * 3 + threadIdx.x] = vx[threadIdx.x * Vp + m.landmarks[j - 35]];
    return;
  }
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  if (threadIdx.x < 128) {
#pragma unroll 4
    for (int i = m.jr_off[j] + threadIdx.x; i < m.jr_off[j + 1]; i += 128) {
      const int v = m.jr_v[i];
      const float c = m.jr_val[i];
      a0 = fmaf(c, vx[v], a0);
      a1 = fmaf(c, vx[Vp + v], a1);
      a2 = fmaf(c, vx[2 * Vp + v], a2);
    }
  }
  a0 = block_sum(a0, red);
  a1 = block_sum(a1, red);
  a2 = block_sum(a2, red);
  if (threadIdx.x == 0) {
    float* o = joints + ((size_t)n * 41 + j) * 3;
    o[0] = a0; o[1] = a1; o[2] = a2;
  }
}

__global__ void __launch_bounds__(128)
joints_kernel(ModelDev m, const float* __restrict__ verts, float* __restrict__ joints /*[M][41][3]*/) {
  __shared__ float red[16];
  joints_block(m, verts, joints, blockIdx.x, blockIdx.y, red);
}

// ------------------------------------------------------------------------------------------------
// K4: per-frame losses with their direct adjoints: keypoints, pose prior, splay, temporal
// ------------------------------------------------------------------------------------------------
// body for frame n.  Written for 128 threads; a 256-thread block may call it too (every loop starts at the thread id and
// ends below 128, so the upper half only takes part in the barriers and adds zeros to the block sums: the same bits)
__device__ __forceinline__ void loss_block(const LossArgs& a, int n) {
  __shared__ float th[105], x[105], res[105], dth[105];
  __shared__ float dJ[41 * 3];
  __shared__ float red[16];
  const int t = threadIdx.x;
  const int Bn = frame_window_size(n, a.win);
  for (int i = t; i < 105; i += 128) { th[i] = a.theta[n * 105 + i]; dth[i] = 0.f; }
  for (int i = t; i < 123; i += 128) dJ[i] = 0.f;
  __syncthreads();
  const float tx = a.trans[n * 3], ty = a.trans[n * 3 + 1], tz = a.trans[n * 3 + 2];
  float l_joint = 0.f, l_pose = 0.f, l_splay = 0.f, l_tj = 0.f, l_tg = 0.f, l_tt = 0.f, l_limit = 0.f;
  // ---- keypoints (smal_fitter.py:129-144, p3d_renderer.py:67-68) --------------------------------
  if (t < 25) {
    const int cj = a.canon[t];
    const float* jp = a.joints + ((size_t)n * 41 + cj) * 3;
    float xn, yn, zv;
    world_to_ndc(jp[0] + tx, jp[1] + ty, jp[2] + tz, xn, yn, zv);
    const float half = 0.5f * (float)(a.S - 1);
    const float row = half * (1.0f - yn), col = half * (1.0f - xn);
    if (a.proj_out) { a.proj_out[(n * 25 + t) * 2] = row; a.proj_out[(n * 25 + t) * 2 + 1] = col; }
    if (a.w_j2d > 0.f && a.vis[n * 25 + t] != 0.f) {
      const float dr = row - a.tj[(n * 25 + t) * 2], dc = col - a.tj[(n * 25 + t) * 2 + 1];
      l_joint = dr * dr + dc * dc;
      const float k = 2.0f * a.w_j2d / (50.0f * (float)Bn);
      // row = half (1 - yn), col = half (1 - xn)
      float gx, gy, gz;
      world_to_ndc_bwd(xn, yn, zv, -half * k * dc, -half * k * dr, gx, gy, gz);
      atomicAdd(&dJ[cj * 3 + 0], gx);
      atomicAdd(&dJ[cj * 3 + 1], gy);
      atomicAdd(&dJ[cj * 3 + 2], gz);
    }
  }
  // ---- pose prior (pose_prior_35.py:117-124) ------------------------------------------------------
  if (a.w_pose > 0.f) {
    if (t < 105) x[t] = th[t] - a.pose_mean[t];
    __syncthreads();
    if (t < 105) {
      float acc = 0.f;
#pragma unroll 15
      for (int r = 0; r < 105; ++r) acc = fmaf(x[r], a.pose_prec[r * 105 + t], acc);
      acc *= a.pose_mask[t];
      res[t] = acc * a.pose_mask[t];        // d(res^2)/d(pre-mask) = 2 res mask
      l_pose = acc * acc;
    }
    __syncthreads();
    if (t < 105) {
      float acc = 0.f;
#pragma unroll 15
      for (int c = 0; c < 105; ++c) acc = fmaf(res[c], a.pose_prec[t * 105 + c], acc);
      dth[t] += acc * (2.0f * a.w_pose / (105.0f * (float)Bn));
    }
  }
  // ---- joint limits (smal_fitter.py:146-151, disabled upstream): w * mean(max(x - hi, 0) + max(lo - x, 0)) over the
  // window's (B, 34, 3) joint rotations; flat inside the limits, unit slope outside
  if (a.w_limit > 0.f && t >= 3 && t < 105) {
    const float x = th[t], hi = a.lim_max[t - 3], lo = a.lim_min[t - 3];
    l_limit = fmaxf(x - hi, 0.f) + fmaxf(lo - x, 0.f);
    const float slope = (x > hi) ? 1.0f : ((x < lo) ? -1.0f : 0.0f);
    dth[t] += slope * (a.w_limit / (102.0f * (float)Bn));
  }
  // ---- splay (smal_fitter.py:159-160) --------------------------------------------------------------
  if (a.w_splay > 0.f && t >= 3 && t < 105 && ((t % 3) != 1)) {
    l_splay = th[t] * th[t];
    dth[t] += 2.0f * a.w_splay * th[t];
  }
  // ---- temporal smoothness (smal_fitter.py:177-190); pair (i, i+1) is owned by frame i ------------
  float dtr = 0.f;
  if (a.w_temp > 0.f && t < 108) {
    const bool is_tr = t >= 105;
    const int e = is_tr ? t - 105 : t;
    const float D = is_tr ? 3.0f : (e < 3 ? 3.0f : 102.0f);
    const float cur = is_tr ? a.trans[n * 3 + e] : th[e];
    float g = 0.f;
    // next neighbour (owned pair)
    bool has_next = (n + 1 < a.M) || (a.halo_next != nullptr);
    if (has_next) {
      const float nxt = (n + 1 < a.M) ? (is_tr ? a.trans[(n + 1) * 3 + e] : a.theta[(n + 1) * 105 + e])
                                      : a.halo_next[is_tr ? 105 + e : e];
      const float d = cur - nxt;
      const float term = d * d * (a.w_temp / D);
      if (is_tr) l_tt = term; else if (e < 3) l_tg = term; else l_tj = term;
      g += d;
    }
    bool has_prev = (n > 0) || (a.halo_prev != nullptr);
    if (has_prev) {
      const float prv = (n > 0) ? (is_tr ? a.trans[(n - 1) * 3 + e] : a.theta[(n - 1) * 105 + e])
                                : a.halo_prev[is_tr ? 105 + e : e];
      g += cur - prv;
    }
    g *= 2.0f * a.w_temp / D;
    if (is_tr) dtr = g; else dth[e] += g;
  }
  __syncthreads();
  // ---- outputs ---------------------------------------------------------------------------------------
  for (int i = t; i < 105; i += 128) a.dth_direct[n * 105 + i] = dth[i];
  for (int i = t; i < 123; i += 128) a.dJ41[n * 123 + i] = dJ[i];
  if (t >= 105 && t < 108) {
    // d trans: temporal part + sum over the 41 joint adjoints (joints = regress(verts) + trans)
    float s = dtr;
    const int e = t - 105;
    for (int j = 0; j < 41; ++j) s += dJ[j * 3 + e];
    a.dtr_direct[n * 3 + e] = s;
  }
  const float nj = 1.0f / (50.0f * (float)Bn), np_ = 1.0f / (105.0f * (float)Bn);
  l_joint = block_sum(l_joint, red);
  l_pose = block_sum(l_pose, red);
  l_splay = block_sum(l_splay, red);
  l_tj = block_sum(l_tj, red);
  l_tg = block_sum(l_tg, red);
  l_tt = block_sum(l_tt, red);
  l_limit = block_sum(l_limit, red);
  if (t == 0) {
    float* o = a.loss_part + n * 8;
    o[0] = a.w_j2d * nj * l_joint;
    o[1] = a.w_pose * np_ * l_pose;
    o[2] = a.w_splay * l_splay;
    o[3] = a.w_limit * l_limit / (102.0f * (float)Bn);   // joint limits (the betas term comes from the prior block of lbs_head_kernel)
    o[4] = 0.f;                // silhouette (tile partials)
    o[5] = l_tj; o[6] = l_tg; o[7] = l_tt;
  }
}

__global__ void __launch_bounds__(128)
loss_kernel(LossArgs a) { loss_block(a, blockIdx.x); }

// shape prior (smal_fitter.py:162-171): loss = w * mean(((b|ls) - mu) P)^2 counted once per window.
// single block; betas/logscale shared across frames (fitter) -> grads are for the shared vectors.


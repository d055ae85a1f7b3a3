// Internal declarations shared by the kernels and the host-side engine. Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "smalfit_math.h"
#include "smalfit_plan.h"   // TreeLevels, WinMap, the constants the launches are sized by

#define SMALFIT_STATUS_BIN_OVERFLOW 1   // a frame's candidate-list pool overflowed

namespace smalfit {

// device-resident model constants (pointers into one allocation owned by smalfit_model)
struct ModelDev {
  int V, Vp, F, NBall;
  const float* vt;        // [3][Vp]
  const float* sd;        // [NBall][3][Vp]
  const float* pd;        // [306][3][Vp]
  int Kw;                 // skin weights, ELL by vertex
  const int* w_j;         // [Kw][Vp]
  const float* w_val;     // [Kw][Vp]
  const int* wc_off;      // skin weights, CSC by joint [36]
  const int* wc_v;
  const float* wc_val;
  const int* jr_off;      // joint regressor, CSC by joint [36]
  const int* jr_v;
  const float* jr_val;
  int Kj;                 // joint regressor, ELL by vertex
  const int* jrv_j;       // [Kj][Vp]
  const float* jrv_val;   // [Kj][Vp]
  const float* Jt;        // [105]  rest joints at beta = 0
  const float* JS;        // [105][NBall]  d(rest joints)/d(beta)
  const int* parents;     // [35]
  const int* faces;       // [F][3]
  const int* vf_off;      // [V+1] vertex -> incident (face*3+corner)
  const int* vf_idx;
  const int* scale_idx;   // [105] log-scale index per (joint, axis) or -1
  int landmarks[6];
  TreeLevels tree;
};

struct LossArgs {
  int M, S;
  WinMap win;
  const float* theta;      // [M][105] masked
  const float* trans;      // [M][3]
  const float* joints;     // [M][41][3] (untranslated)
  const int* canon;        // [25]
  const float* tj;         // [M][25][2] (row, col)
  const float* vis;        // [M][25]
  float w_j2d, w_pose, w_splay, w_temp;
  float w_limit;           // joint-limit hinge (smal_fitter.py:146-151)
  const float* lim_min;    // [102] lower / upper limit per joint-rotation component
  const float* lim_max;
  const float* pose_prec;  // [105][105]
  const float* pose_mean;  // [105]
  const float* pose_mask;  // [105]
  const float* halo_prev;  // [108] neighbour frame before frame 0 (theta 105 | trans 3) or null
  const float* halo_next;  // [108] neighbour frame after frame M-1 or null
  float* proj_out;         // [M][25][2] or null
  float* dth_direct;       // [M][105]
  float* dJ41;             // [M][41][3]
  float* dtr_direct;       // [M][3]
  float* loss_part;        // [M][8]
};

struct AssembleArgs {
  int M, S, T, nb, NBall, nblk_beta, nvt;
  WinMap win;
  int betas_shared, ls_shared;
  float w_sil;
  const float* dbeta_part;
  const float* dJrest;
  const float* dbetaJ;     // [M][NBall] d beta through the rest joints (chain_bwd_kernel)
  int ngrp_beta;           // frame groups of the shape-blend adjoint (dbeta_block)
  const float* JS;
  const float* gb_prior;
  const float* gls_prior;
  const float* dls;
  const float* dtheta;
  const float* gmask;
  const float* rmask;
  const float* dtr_direct;
  const float* dtr_part;
  const float* loss_part;
  const float* loss_betas;
  const float* tile_loss;
  const long long* qloss;  // weighted silhouette loss of the queued pixels, one 2^-40 fixed-point partial per band / select block
  int nqblk;
  float* lpart;            // [kAsmLoss] partial sums of the silhouette loss (assemble_kernel)
  long long* qpart;        // [kAsmLoss] integer partial sums of the queue kernels' loss
  int* counter;            // arrival counter of assemble_kernel's blocks (zero between launches)
  float* g_betas;
  float* g_ls;
  float* g_grot;
  float* g_jrot;
  float* g_trans;
  float* losses;
};

// What assemble_kernel and frame_loss_rows_kernel take beside AssembleArgs (which the pending step carries into lbs_head_step_kernel
// and therefore stays what it is): independent images and one row of loss terms per frame.  All zero: neither.
struct AssembleExt {
  // independent images (one shape set per frame): the prior's gradient as one row per shape set, its loss as one term per frame
  const float* gb_prior_pf;                // rows of gb_stride floats, or null
  const float* gls_prior_pf;               // rows of gls_stride floats, or null
  int gb_stride, gls_stride;
  const float* prior_loss_pf;              // [M] or null
  // one row of loss terms per frame (smalfit_fit_args.losses_per_frame), written by frame_loss_rows_kernel
  float* losses_pf;                        // [M][9] or null
  unsigned long long* frame_qloss;         // [M][kFrameLossStride]: the queue kernels' 2^-40 fixed-point loss per frame; cleared by its reader
  int prior_windows;                       // one subject: windows whose prior term this evaluation owns (their sum is *loss_betas)
};

// What window_rows_kernel takes beside AssembleArgs / AssembleExt (smalfit_fit_eval_windows): one row per window of the sequence.
struct WindowRowsDev {
  int W;                    // rows
  int clear_qloss;          // this kernel is the last reader of frame_qloss (no frame_loss_rows_kernel behind it): clear it
  float* losses;            // [W][9]
  float* g_betas;           // [W][nb] or null
  float* g_ls;              // [W][6] or null
  float* row_betas;         // workspace [W][kWindowRowBetas]: the rows as the block that arrives last adds them up; null: no shape gradient
  float* row_ls;            // workspace [W][kWindowRowScales]; null: no shared limb-scale gradient
  float* tot_betas;         // [nb] the rows added in window order (smalfit_fit_args.g_betas) or null
  float* tot_ls;            // [6] likewise or null
  int* counter;             // arrival counter of the kernel's blocks (zero between launches)
};

// One optimiser step that has not been taken yet, carried by the NEXT evaluation's lbs_head_kernel (smalfit_fit_run): the raw
// partials of the previous evaluation's backward pass as assemble_kernel would read them, and per parameter tensor where its
// value / moments are read and where value / moments / gradient go.  Per-frame tensors are stepped in place by their frame's
// block.  The shared ones (betas, shared limb scales) are stepped by EVERY block from the same operands in the same order, so
// all copies agree bitwise, and stored by one block only -- to other addresses than they are read from, because the other
// blocks of the launch are still reading.
struct PendingTensor {
  int train;                       // stepped by this launch (else the tensor is read through HeadArgs as ever)
  const float *p_in, *m_in, *v_in;
  float *p, *m, *v, *g;
};
struct PendingStep {
  AssembleArgs g;                  // partials, masks, shape of the previous evaluation (output pointers unused)
  PendingTensor betas, ls, grot, jrot, trans;
  float step_size, b1, b2, eps, bc2_sqrt;   // adam_bias_terms of the pending step
  int fresh;                       // first step of a stage: moments taken as zero
};

}  // namespace smalfit

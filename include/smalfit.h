/* smalfit.h — C-ABI of the MI355X-native SMAL fitting engine (libsmalfit.so, built by hipcc for gfx950).
 *
 * The reference (benjiebob/SMALify @ /root/reference) has no FFI layer: its hot path is Python calling
 * torch / pytorch3d.  The boundary a maintainer would bind is therefore the set of Python call sites
 * listed in SURVEY.md §8b; every entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - every tensor argument is a DEVICE pointer to contiguous row-major float32 (int32 for indices)
 *     unless the parameter is documented as "host"
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     except smalfit_engine_status()
 *   - functions return 0 on success, non-zero on failure; smalfit_last_error() describes the failure
 *   - handles are thread-compatible, not thread-safe; no ownership of caller buffers is taken
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails
 */
#ifndef SMALFIT_H_
#define SMALFIT_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smalfit_model smalfit_model;
typedef struct smalfit_engine smalfit_engine;

#define SMALFIT_NUM_JOINTS 35
#define SMALFIT_NUM_MODEL_JOINTS 41
#define SMALFIT_NUM_KEYPOINTS 25
#define SMALFIT_NUM_LOSS_TERMS 9 /* joint, pose, splay, betas, sil_reproj, temp_joint, temp_global, temp_trans, limit */

#define SMALFIT_STATUS_BIN_OVERFLOW 1 /* reserved */

/* ABI version of this header.  smalfit_version() returns the version the library was built from; a caller compares the
 * two once at load time (smalify_amd/_lib.py does) -- the argument structs below are passed by pointer and grow at the
 * tail from version to version.  History: 1 = round 1; 2 = 9 loss terms (losses must hold SMALFIT_NUM_LOSS_TERMS floats),
 * smalfit_fit_args gained target_sil_u8 / w_limit; 3 = smalfit_fit_args.struct_size (first field), frame_offset,
 * total_frames; smalfit_engine_clear_joint_limits, smalfit_shard_local_step; 4 = smalfit_shard_run (the sharded loop of a
 * whole stage in one call, the collective supplied by the host as a function pointer), smalfit_rccl_allgather;
 * 5 = smalfit_engine_set_option; 6 = smalfit_fit_args.subject_frames / losses_per_frame (a batch of independent images,
 * each with its own shape; one row of loss terms per frame).  Added within version 6, no struct of it changing its layout:
 * smalfit_fit_eval_windows (smalfit_window_rows); smalfit_fit_metrics (smalfit_metrics_args: silhouette IoU counts and PCK
 * per frame); smalfit_mesh_score (smalfit_mesh_score_args: point-to-surface distances both ways, per mesh);
 * smalfit_mesh_surface_eval / smalfit_fit3d_step_surface (smalfit_surface_term_args: the same distances as a term to descend on);
 * smalfit_mesh_surface_eval_gated / smalfit_fit3d_step_gated / smalfit_mesh_targets_sample_normals (smalfit_surface_gate_args: that
 * term gated for partial scans); smalfit_mesh_objective_eval_gated / smalfit_fit3d_step_partial / smalfit_mesh_targets_sample_attrs
 * (smalfit_chamfer_gate_args: the chamfer term gated the same way); smalfit_mesh_targets_build_index /
 * smalfit_mesh_targets_index_stats (smalfit_scan_index_args: a grid over the targets that changes no result). */
#define SMALFIT_ABI_VERSION 6
int smalfit_version(void);
const char* smalfit_last_error(void);

/* ---- model constants -------------------------------------------------------------------------
 * replaces: SMAL.__init__ tensors            reference smal_model/smal_torch.py:36-96
 * All pointers are HOST arrays prepared by the caller (smalify_amd/model_io.py does the pickle
 * parsing, family mean and symmetry alignment exactly as the reference). */
typedef struct smalfit_model_desc {
  int num_verts;            /* V (3889)                                   */
  int num_faces;            /* F (7774)                                   */
  int num_betas;            /* rows of shapedirs (41)                     */
  const float* v_template;  /* (V,3)                                      */
  const float* shapedirs;   /* (num_betas, 3V), column = 3*v + axis       */
  const float* posedirs;    /* (306, 3V)                                  */
  const float* J_regressor; /* (V,35) dense                               */
  const float* weights;     /* (V,35) dense                               */
  const int* parents;       /* (35), parents[0] = -1, parents[i] < i      */
  const int* faces;         /* (F,3)                                      */
} smalfit_model_desc;

int smalfit_model_create(const smalfit_model_desc* desc, smalfit_model** out);
void smalfit_model_destroy(smalfit_model* model);

/* ---- engine = workspace in HBM for up to max_frames frames at image_size^2 ----------------------
 * image_size <= 1024 (the reference renders 256 or 512, config.py IMG_RES; larger sizes are rejected: the rasteriser's
 * pixel walk is exact in float32 up to there) */
int smalfit_engine_create(smalfit_model* model, int max_frames, int image_size, smalfit_engine** out);
void smalfit_engine_destroy(smalfit_engine* engine);
/* synchronises `stream`, returns and clears the sticky status bits (SMALFIT_STATUS_*) */
int smalfit_engine_status(smalfit_engine* engine, void* stream, int* status_bits);
/* The rasteriser keeps, per pixel, the depth bounds of its last exact K-nearest selection and re-proves them from
 * counts at every evaluation (results never depend on that state, only the time does).  This call forgets the
 * bounds, e.g. before fitting an unrelated sequence with the same engine.  No counterpart in the reference. */
int smalfit_engine_reset_raster_cache(smalfit_engine* engine, void* stream);

/* optional: time sections of smalfit_fit_eval with HIP events recorded on the caller's stream.
 * profile_begin arms up to max_evals timed evaluations, taking every `stride`-th evaluation (an event record costs
 * ~5 us of stream time on MI355X, so timing every evaluation would slow the loop it measures by several percent);
 * profile_end synchronises `stream`, and returns the summed milliseconds and the number of timed evaluations per
 * section. */
#define SMALFIT_NUM_SECTIONS 7
#define SMALFIT_SEC_LBS_FWD 0        /* lbs_head (pose, shape blend, shape prior) + skin + joints kernels */
#define SMALFIT_SEC_RASTER_SWEEP 1   /* raster_sweep_kernel alone                                  */
#define SMALFIT_SEC_RASTER_SELECT 2  /* raster_select_kernel alone (K-nearest selection)          */
#define SMALFIT_SEC_RASTER_BWD 3     /* raster_bwd_kernel alone                                   */
#define SMALFIT_SEC_LBS_BWD 4        /* vertex, mid-stage (dA, pose-blend, shape-blend) and chain adjoints */
#define SMALFIT_SEC_RASTER_RESOLVE 5 /* raster_resolve_kernel + raster_band_kernel                  */
#define SMALFIT_SEC_RASTER_BBOX 6    /* no launch any more: raster_sweep_kernel forms the boxes    */
int smalfit_engine_profile_begin(smalfit_engine* engine, int max_evals, int stride);
int smalfit_engine_profile_end(smalfit_engine* engine, void* stream, float* ms_total, int* counts);

/* replaces: Prior.__init__ data              reference smal_fitter/priors/pose_prior_35.py:51-92
 * host arrays: prec (105,105), mean (105), mask (105) */
int smalfit_engine_set_pose_prior(smalfit_engine* engine, const float* prec, const float* mean,
                                  const float* mask);
/* replaces: LimitPrior().min_values / max_values viewed as (N_POSE, 3)   reference smal_fitter/smal_fitter.py:76-79,
 * priors/joint_limits_prior.py:39-104 (commented out upstream: its table has 32 joints x 3 where view(34, 3) expects 34;
 * smalify_amd/model_io.py::joint_limit_table completes it).  host arrays: min (34,3), max (34,3), min <= max */
int smalfit_engine_set_joint_limits(smalfit_engine* engine, const float* min_values, const float* max_values);
/* back to the reference's behaviour (term commented out): w_limit is ignored again */
int smalfit_engine_clear_joint_limits(smalfit_engine* engine);
/* Engine options (no counterpart in the reference: they select between readings of pytorch3d 0.2.5 that cannot be told apart
 * without a PyTorch3D-produced vector).
 *   SMALFIT_OPT_UNCLAMPED_EDGE_T  value 0 (default) / 1.  replaces: rasterize_meshes_backward behind
 *     MeshRasterizer / SoftSilhouetteShader, reference smal_fitter/p3d_renderer.py:33-39.  0 = the exact gradient of the
 *     forward's point-segment distance (edge parameter t clamped to [0, 1]); 1 = the gradient with t left unclamped (the edge
 *     treated as an infinite line in PointLineDistanceBackward), as some 0.2.x sources are recalled to do.  The two differ only
 *     at pixels whose nearest feature of the nearest edge is a vertex.  Applies to smalfit_fit_eval / smalfit_fit_run /
 *     smalfit_shard_run / smalfit_render_backward; the forward pass is the same either way. */
#define SMALFIT_OPT_UNCLAMPED_EDGE_T 1
int smalfit_engine_set_option(smalfit_engine* engine, int option, int value);
/* replaces: betas_prec / mean_betas          reference smal_fitter/smal_fitter.py:48-69
 * host arrays: prec (dim,dim), mean (dim); dim = 26 (unity prior: betas|log scales) or <= 20 */
int smalfit_engine_set_shape_prior(smalfit_engine* engine, const float* prec, const float* mean, int dim);

/* ---- SMAL.__call__ ------------------------------------------------------------------------------
 * replaces: SMAL.__call__(beta, theta, betas_logscale=...)   reference smal_model/smal_torch.py:99-189
 * beta (M,nb) theta (M,35,3) logscale (M,6) or NULL -> verts (M,V,3) joints (M,41,3)
 * optional outputs (NULL to skip): Rs (M,35,3,3), v_shaped (M,V,3) */
int smalfit_lbs_forward(smalfit_engine* engine, void* stream, int M, int nb, const float* beta,
                        const float* theta, const float* logscale, float* verts, float* joints,
                        float* Rs, float* v_shaped);
/* adjoint of the above for upstream gradients dverts (M,V,3) and/or djoints (M,41,3) (either may be
 * NULL): dbeta (M,nb), dtheta (M,35,3), dlogscale (M,6) or NULL.  Recomputes the forward internally. */
int smalfit_lbs_backward(smalfit_engine* engine, void* stream, int M, int nb, const float* beta,
                         const float* theta, const float* logscale, const float* dverts,
                         const float* djoints, float* dbeta, float* dtheta, float* dlogscale);

/* the same call with every option of the reference's signature (smal_torch.py:99):
 *   SMAL.__call__(beta, theta, trans=None, del_v=None, betas_logscale=None, get_skin=True, v_template=None)
 * theta as (M,35,3) axis-angles OR Rs as (M,35,3,3) rotation matrices (:132-133, `len(theta.shape) == 4`);
 * v_offset (M,V,3) is added to the shaped template: del_v, plus (v_template - the model's template) for a per-call
 * template (:107-122).  trans is a plain addition after the call.  Forward reads the inputs and writes verts / joints
 * (+ Rs_out, v_shaped when not NULL); backward recomputes the forward and reads dverts / djoints (either may be NULL),
 * writing whichever of dbeta, dtheta (axis-angle input) or dRs (matrix input), dlogscale, dv_offset is not NULL. */
typedef struct smalfit_lbs_args {
  int num_frames, num_betas;
  const float* beta;       /* (M,nb)                          */
  const float* theta;      /* (M,35,3) or NULL when Rs given  */
  const float* Rs;         /* (M,35,3,3) or NULL              */
  const float* logscale;   /* (M,6) or NULL                   */
  const float* v_offset;   /* (M,V,3) or NULL                 */
  float *verts, *joints, *Rs_out, *v_shaped;            /* forward outputs: (M,V,3), (M,41,3), (M,35,3,3), (M,V,3) */
  const float *dverts, *djoints;                        /* backward inputs                                          */
  float *dbeta, *dtheta, *dRs, *dlogscale, *dv_offset;  /* backward outputs                                         */
} smalfit_lbs_args;
int smalfit_lbs_forward_ex(smalfit_engine* engine, void* stream, const smalfit_lbs_args* args);
int smalfit_lbs_backward_ex(smalfit_engine* engine, void* stream, const smalfit_lbs_args* args);

/* ---- batch_rodrigues ----------------------------------------------------------------------------
 * replaces: batch_rodrigues(theta)                           reference smal_model/batch_lbs.py:33-52 */
int smalfit_rodrigues(void* stream, int count, const float* theta, float* R);
int smalfit_rodrigues_backward(void* stream, int count, const float* theta, const float* dR, float* dtheta);

/* replaces: batch_global_rigid_transformation(Rs, Js, parent, betas_logscale=...)   reference smal_model/batch_lbs.py:75-170
 * Rs (count,35,3,3)  Js (count,35,3)  parents: host int[35] with parents[i] < i (parents[0] ignored)
 * logscale (count,6) or NULL -> new_J (count,35,3), A (count,35,4,4).  (Inside the fitting path the chain and its
 * adjoint are part of smalfit_lbs_forward / _backward and smalfit_fit_eval.) */
int smalfit_global_rigid_transformation(void* stream, int count, const float* Rs, const float* Js,
                                        const int* parents /*host*/, const float* logscale, float* new_J, float* A);
/* its adjoint (autograd of the reference's function): d_new_J (count,35,3), d_A (count,35,4,4) -> dRs (count,35,3,3),
 * dJs (count,35,3), dlogscale (count,6) (ignored when logscale is NULL); scratch: count * 840 floats of device memory */
int smalfit_global_rigid_transformation_backward(void* stream, int count, const float* Rs, const float* Js,
                                                 const int* parents /*host*/, const float* logscale, const float* d_new_J,
                                                 const float* d_A, float* scratch, float* dRs, float* dJs, float* dlogscale);

/* ---- Renderer.forward ---------------------------------------------------------------------------
 * replaces: Renderer.forward(vertices, points, faces)        reference smal_fitter/p3d_renderer.py:61-74
 * verts (M,V,3) world space -> sil (M,S,S) soft silhouette (sigma 1e-4, blur log(9999)*1e-4, K=100)
 * points (M,P,3) -> proj_points (M,P,2) as (row, col) screen coordinates; points may be NULL */
int smalfit_render_forward(smalfit_engine* engine, void* stream, int M, const float* verts,
                           const float* points, int P, float* sil, float* proj_points);
/* Renderer.forward(render_texture=True), colour branch (p3d_renderer.py:41-59,70-72): hard rasterisation
 * (blur_radius 0, faces_per_pixel 1) + HardPhongShader, one point light at (0,0,3), constant vertex colour `rgb`
 * (host, 3 floats in [0,1]; the reference uses config.MESH_COLOR / 255), white background.  Visualisation only: no
 * gradient.  verts [M][V][3] world space with the translation applied; image [M][3][S][S]. */
int smalfit_render_color(smalfit_engine* engine, void* stream, int num_frames, const float* verts, const float* rgb /*host*/,
                         float* image);

/* adjoint wrt verts given the saved silhouette and dL/dsil (M,S,S) */
int smalfit_render_backward(smalfit_engine* engine, void* stream, int M, const float* verts,
                            const float* sil, const float* dsil, float* dverts);
/* diagnostics: the hand-off of the last silhouette forward (smalfit_render_forward / _backward, an evaluation) to the backward
 * gather, one byte per face: the length of the face's candidate list (0..128), 254 = candidate masks, 255 = the whole pixel box is
 * walked.  lengths: device, (M,F) bytes.  Results never depend on which form a face takes; the tests of the gather do */
int smalfit_engine_face_list_lengths(smalfit_engine* engine, void* stream, int M, unsigned char* lengths);
int smalfit_project_points_backward(void* stream, int count, int image_size, const float* points,
                                    const float* dproj, float* dpoints);

/* ---- SMALFitter.forward + get_temporal + backward, fused ------------------------------------------
 * replaces: SMALFitter.forward / get_temporal and the autograd backward of their sum
 *           reference smal_fitter/smal_fitter.py:107-190, smal_fitter/optimize_to_joints.py:117-136
 * Evaluates M consecutive frames, grouped into windows of `window` frames (the last may be ragged),
 * with the reference's per-window normalisers, and writes every loss term plus the gradient of
 * their sum with respect to each parameter tensor. */
typedef struct smalfit_fit_args {
  unsigned struct_size;           /* sizeof(smalfit_fit_args) of the caller's header; checked by the library */
  int num_frames;                 /* M                                                          */
  int window;                     /* WINDOW_SIZE; normalisers use the size of each frame's window (see frame_offset) */
  int logscale_mode;              /* 0: no limb scales, 1: shared (6,), 2: per frame (M,6)       */
  int temporal;                   /* include the temporal term over these M frames              */
  int shape_prior_dim;            /* 0 = use the dim given to set_shape_prior                    */
  float w_j2d, w_sil, w_betas, w_pose, w_splay, w_temp;
  const float* betas;             /* (20,) shared                                               */
  const float* log_beta_scales;   /* (6,) or (M,6) or NULL                                      */
  const float* global_rotation;   /* (M,3)                                                      */
  const float* joint_rotations;   /* (M,34,3)                                                   */
  const float* trans;             /* (M,3)                                                      */
  const float* global_mask;       /* (3,)   or NULL (= ones)                                    */
  const float* rotation_mask;     /* (34,3) or NULL (= ones)                                    */
  const float* target_joints;     /* (M,25,2) (row, col)                                        */
  const float* target_visibility; /* (M,25) float {0,1}                                         */
  const float* target_sil;        /* (M,S,S); may be NULL when w_sil == 0                       */
  const float* halo_prev;         /* (108,) masked theta(105)|trans(3) of the frame before frame 0, or NULL */
  const float* halo_next;         /* (108,) of the frame after frame M-1, or NULL               */
  float* losses;                  /* (9,) see SMALFIT_NUM_LOSS_TERMS                            */
  float* g_betas;                 /* (20,)           or NULL                                    */
  float* g_log_beta_scales;       /* (6,) / (M,6)    or NULL                                    */
  float* g_global_rotation;       /* (M,3)           or NULL                                    */
  float* g_joint_rotations;       /* (M,34,3)        or NULL                                    */
  float* g_trans;                 /* (M,3)           or NULL                                    */
  float* sil_out;                 /* (M,S,S) rendered silhouettes or NULL                       */
  float* proj_out;                /* (M,25,2) projected keypoints or NULL                       */
  float* verts_out;               /* (M,V,3) translated vertices or NULL                        */
  const unsigned char* target_sil_u8; /* (M,S,S) target silhouettes as bytes, t = b / 255 (what the 8-bit masks of
                                     data_loader.py:43 hold); used instead of target_sil when not NULL          */
  float w_limit;                  /* joint-limit hinge weight (OPT_WEIGHTS row 5).  Ignored -- like the reference, whose
                                     term is commented out while its weight table says 100 -- until
                                     smalfit_engine_set_joint_limits has been called                          */
  /* Position of these M frames in their sequence.  The reference groups the frames of a SEQUENCE into consecutive windows
   * of WINDOW_SIZE (optimize_to_joints.py:119-120, last one ragged) and normalises each window's terms by its size
   * (smal_fitter.py:144,157,173).  An evaluation may hold any contiguous part of the sequence -- a shard, or ONE frame of
   * an 8-frame window (one frame per GPU): local frame n is sequence frame frame_offset + n, its window is
   * [w, min(w + window, total_frames)) with w = ((frame_offset + n) / window) * window.  The shape-prior term (once per
   * window in the reference) is owned by the evaluation that holds the window's first frame.
   * Zeros = the M frames are the whole sequence. */
  int frame_offset;               /* index of local frame 0 in the sequence                     */
  int total_frames;               /* frames in the whole sequence; 0 = frame_offset + num_frames */
  /* Whose frames these are.  0 (default): the M frames are ONE subject -- one shape, everything above as documented.
   * 1: every frame is its own subject, an unrelated image (the reference fits those one image per SMALFitter,
   * optimize_to_joints.py with BASELINE config 1): betas (M,20), g_betas (M,20); logscale_mode 0 or 2 (1 is refused:
   * nothing is shared); window must be 1, frame_offset / total_frames / temporal 0 and halo_* NULL (refused otherwise);
   * the shape prior (20-dim, or 26-dim over [betas_n | log_beta_scales_n] with logscale_mode 2) is evaluated once per
   * frame with weight w_betas, its gradient going to row n of g_betas / g_log_beta_scales; losses[3] is the sum over
   * frames.  smalfit_fit_eval and smalfit_fit_run accept it (the run keeps the plain chain: nothing is folded);
   * smalfit_shard_* and the graph replay refuse it.  Any other value is refused: clips of K > 1 frames per subject in one
   * batch are not implemented. */
  int subject_frames;
  /* (M, SMALFIT_NUM_LOSS_TERMS) or NULL, either mode: row n = frame n's contribution to each term of `losses`, same
   * weights and normalisers, so that every column sums to `losses` (up to float32 re-ordering).  The temporal columns of
   * row n are the terms of the pair (n, n+1), zero for the last frame without a halo and for independent images.  The
   * betas column: frame n's own prior term for independent images; for one subject the window's term in the row of the
   * window's first frame when this evaluation owns that window, zero elsewhere.  Asking for it changes no other output. */
  float* losses_per_frame;
} smalfit_fit_args;

int smalfit_fit_eval(smalfit_engine* engine, void* stream, const smalfit_fit_args* args);

/* ---- the same evaluation, with every window's loss terms and its share of the shared gradients ------------------------
 * replaces: the per-window calls of SMALFitter.forward inside one epoch and the backward of their (weighted) sum
 *           reference smal_fitter/smal_fitter.py:107-175, smal_fitter/optimize_to_joints.py:119-122
 * The reference's driver calls forward() once per window and backward() once per epoch on the sum.  One evaluation of the
 * whole sequence serves that loop exactly when each window's loss and each window's gradient can be handed out on their own:
 * the gradients of global_rotation, joint_rotations, trans and per-frame limb scales are per frame already; the rows below
 * are the missing part, the shared parameters.
 *   row w of losses            the nine terms restricted to the frames of window w (same weights and normalisers); the shape
 *                              prior's term in the rows of the windows this evaluation owns; the temporal columns of the pair
 *                              (n, n+1) in the row of frame n's window
 *   row w of g_betas /         gradient of row w's total: the shape-blend adjoint of the window's frames, their rest-joint
 *     g_log_beta_scales        path, and the prior's gradient once per owned window
 * args->losses, the per-frame gradients and args->losses_per_frame are what smalfit_fit_eval writes for the same block, bit
 * for bit; args->g_betas / args->g_log_beta_scales (shared, logscale_mode 1), when not NULL, are the rows added in window
 * order in double and rounded once.  One subject only (args->subject_frames 0: independent images already have one row per
 * image). */
typedef struct smalfit_window_rows {
  unsigned struct_size;          /* sizeof(smalfit_window_rows) of the caller's header; checked before any other field */
  int num_windows;               /* W = windows of the SEQUENCE holding at least one of the M frames:
                                    (frame_offset + M - 1) / window - frame_offset / window + 1; any other value is refused */
  float* losses;                 /* (W, 9), required */
  float* g_betas;                /* (W, 20) or NULL */
  float* g_log_beta_scales;      /* (W, 6) or NULL; logscale_mode 1 only, refused when non-NULL in modes 0 / 2 */
} smalfit_window_rows;
int smalfit_fit_eval_windows(smalfit_engine* engine, void* stream, const smalfit_fit_args* args, const smalfit_window_rows* rows);

/* ---- how good a fit is: silhouette intersection / union and PCK per frame -------------------------------------------
 * No counterpart in the reference, which contains no evaluation code: the definitions below are THIS PROJECT'S.  (The PCK
 * normaliser -- the square root of the ground-truth silhouette's area -- is the convention the BADJA / StanfordExtra results
 * are recalled to use; no parity with anyone's evaluation script is claimed.)
 *   covered        a pixel is covered exactly when smalfit_render_color on the same vertices would not leave it white (the
 *                  hard rasterisation of p3d_renderer.py:41-59: blur_radius 0, one face per pixel; the same per-face record,
 *                  the same clipped pixel box, the same inclusion test -- one device function serves both entry points)
 *   target on      a float target pixel t is on when t > 0.5f, a byte target pixel b when b >= 128
 *   sil_counts     row n = pixels of frame n in: covered AND on | covered OR on | covered | on.  Integer counts: no quotient is
 *                  formed on the device (IoU = sil_counts[n][0] / sil_counts[n][1] is the host's, as is what an empty union means)
 *   keypoint_dist  [n][k] = hypot(proj - target) / sqrtf((float)sil_counts[n][3]) in float32, for all 25 keypoints whether
 *                  visible or not; +inf for every keypoint of a frame whose target is empty
 *   visible        target_visibility > 0
 *   pck_counts     row n = visible keypoints, then for each t the visible keypoints with keypoint_dist <= thresholds[t]
 * Everything is enqueued on `stream`; nothing synchronises.  A refused block launches nothing and leaves every output alone.
 * The call uses the engine's projection workspace, as smalfit_render_color does: it must not overlap another call on the same
 * engine (calls enqueued on one stream never do). */
#define SMALFIT_MAX_PCK_THRESHOLDS 8
typedef struct smalfit_metrics_args {
  unsigned struct_size;                /* sizeof(smalfit_metrics_args) of the caller's header; checked before any other field */
  int num_frames;                      /* M <= the engine's max_frames */
  const float* verts;                  /* (M,V,3) world, translation applied: verts_out of smalfit_fit_eval */
  const float* target_sil;             /* (M,S,S) float, or NULL */
  const unsigned char* target_sil_u8;  /* (M,S,S) bytes, used when not NULL (as in smalfit_fit_args) */
  unsigned* sil_counts;                /* (M,4): intersection, union, rendered, target -- pixels */
  unsigned char* mask_out;             /* (M,S,S) 0/1 hard coverage, or NULL */
  /* keypoints: all of the next three given, or all NULL (silhouette only; the outputs below must then be NULL too) */
  const float* proj_joints;            /* (M,25,2) (row, col): proj_out of smalfit_fit_eval */
  const float* target_joints;          /* (M,25,2) */
  const float* target_visibility;      /* (M,25) */
  int num_thresholds;                  /* T in 1..8 when keypoints are given */
  float thresholds[SMALFIT_MAX_PCK_THRESHOLDS];   /* host values, each finite and > 0 */
  float* keypoint_dist;                /* (M,25) or NULL: distance / sqrt(target pixels) of EVERY keypoint */
  int* pck_counts;                     /* (M,1+T) or NULL: visible keypoints, then those with dist <= thresholds[t] */
} smalfit_metrics_args;
int smalfit_fit_metrics(smalfit_engine* engine, void* stream, const smalfit_metrics_args* args);

/* ---- the epoch loop: loss + backward + optimizer.step(), `iterations` times in one call ---------------------------
 * replaces: the body of the epoch loop                        reference smal_fitter/optimize_to_joints.py:113-137
 *   optimizer.zero_grad(); acc_loss = sum over windows of model(...) + temporal; acc_loss.backward(); optimizer.step()
 * with optimizer = torch.optim.Adam(model.parameters(), lr, betas=(0.5, 0.999)) created per stage (:96).
 * The fit parameters, their gradient and the two Adam moments are four flat device buffers of one layout (the caller
 * chooses it; the pointers inside smalfit_fit_args point into `param` / `grad`); the trainable tensors of the stage are
 * up to four [begin, end) ranges of that layout and are updated by ONE kernel launch per iteration -- or by none: when the
 * ranges are exactly whole parameter tensors of `args` with their gradients at the same offsets of `grad`, the step of every
 * iteration but the last is taken by the next iteration's first launch (same results, bit for bit; on return parameters,
 * moments, gradients and losses are those of the last iteration either way).
 * step = optimiser steps already taken in this stage; when it is 0 the moments are taken as zero and not read, so a new
 * stage needs no fill.  Everything is enqueued on `stream`; nothing synchronises. */
typedef struct smalfit_adam_args {
  float* param;        /* flat parameters                                   */
  float* grad;         /* their gradient (written by the evaluation)        */
  float* exp_avg;      /* Adam first moment                                 */
  float* exp_avg_sq;   /* Adam second moment                                */
  int num_segments;    /* 0..4 trainable ranges of the flat layout          */
  int seg_begin[4];
  int seg_end[4];
  float lr, beta1, beta2, eps;
  int step;            /* steps already taken by this stage's optimiser     */
} smalfit_adam_args;
int smalfit_fit_run(smalfit_engine* engine, void* stream, const smalfit_fit_args* args, const smalfit_adam_args* adam,
                    int iterations);
/* enable != 0: smalfit_fit_run captures one iteration (the evaluation's kernels + the Adam launch) into a HIP graph the
 * first time it sees a set of arguments on a (non-default) stream and replays it `iterations` times; the Adam step count
 * then lives in a device counter and the bias corrections are formed on the device.  Off by default. */
int smalfit_engine_set_graph(smalfit_engine* engine, int enable);
/* optimizer.step() alone on the ranges (t = adam->step + 1) */
int smalfit_adam_segments(void* stream, const smalfit_adam_args* adam);

/* ---- frame-sharded fitting (one process per GPU; no counterpart in the reference) --------------------
 * Per iteration a rank evaluates its frames, steps its per-frame parameters, and contributes one record to an
 * all-gather: record = [partial gradient of the shared parameters (num_shared) | masked theta(105)|trans(3) of its first
 * frame | of its last frame] -- the partial shape gradient and the neighbours' temporal halo of the next iteration. */
/* one rank's side of an iteration up to the collective, in ONE call: the evaluation (smalfit_fit_eval), Adam on the
 * per-frame ranges (`adam_local`, t = step + 1) and the record (smalfit_shard_record with the parameters / masks of `args`)
 * written straight into the collective's send buffer */
int smalfit_shard_local_step(smalfit_engine* engine, void* stream, const smalfit_fit_args* args,
                             const smalfit_adam_args* adam_local, int num_shared, const float* shared_grad,
                             float* record /*(num_shared + 216)*/);
int smalfit_shard_record(void* stream, int num_shared, const float* shared_grad, int num_frames,
                         const float* global_rotation, const float* joint_rotations, const float* trans,
                         const float* global_mask /*(3,)*/, const float* rotation_mask /*(34,3)*/,
                         float* record /*(num_shared + 216)*/);
/* after the all-gather: grad[0:num_shared] = sum over ranks (in rank order: the same bits on every rank) of the gathered
 * partial gradients, then Adam (t = adam->step + 1) on the first num_trainable of them.  gathered: (world_size, record_stride) */
int smalfit_shard_reduce_step(void* stream, int world_size, int record_stride, const float* gathered, int num_shared,
                              int num_trainable, const smalfit_adam_args* adam);

/* The sharded loop of a whole stage in ONE call (round 4; until then a host loop made one call before and one after the
 * collective of every iteration): `iterations` x [ smalfit_shard_local_step -> all-gather of the record -> smalfit_shard_reduce_step ],
 * everything enqueued on `stream`, nothing synchronises, no host code between two iterations.  The library links against no
 * communication library: the collective is the caller's, handed over as a function that enqueues
 *     all-gather of `count` floats per rank:  send (count) -> recv (world_size x count, rank-major)   on `stream`
 * and returns 0 on success.  With RCCL that is smalfit_rccl_allgather below on the process group's own communicator (same
 * stream as the kernels: no event hand-over per iteration); any other transport (gloo in the tests) is a host callback.
 * `gathered` is persistent: args->halo_prev / halo_next point INTO it (row rank-1, floats [num_shared+108, num_shared+216) and
 * row rank+1, floats [num_shared, num_shared+108)), so the all-gather of iteration i delivers the temporal halo of iteration
 * i+1 in place; the caller fills it once before the first iteration (one stand-alone all-gather of the boundary records).
 * adam_local: the per-frame ranges; adam_shared: the same flat buffers (its ranges are ignored: the first
 * num_trainable_shared floats are stepped from the rank-ordered sum); both with the same `step`. */
typedef int (*smalfit_allgather_fn)(void* ctx, const float* send, float* recv, int count, void* stream);
typedef struct smalfit_shard_args {
  unsigned struct_size;        /* sizeof(smalfit_shard_args) of the caller's header */
  int world_size, rank;
  int num_shared;              /* shared floats at the head of the flat gradient (20, or 26 with shared limb scales) */
  int num_trainable_shared;    /* how many of them this stage trains (0 in stage 0) */
  const float* shared_grad;    /* this rank's partial gradient of the shared parameters (num_shared), written by the evaluation */
  float* record;               /* (num_shared + 216): the collective's send buffer */
  float* gathered;             /* (world_size, num_shared + 216): its receive buffer */
  smalfit_allgather_fn allgather;
  void* allgather_ctx;
} smalfit_shard_args;
int smalfit_shard_run(smalfit_engine* engine, void* stream, const smalfit_fit_args* args, const smalfit_adam_args* adam_local,
                      const smalfit_adam_args* adam_shared, const smalfit_shard_args* shard, int iterations);
/* a smalfit_allgather_fn over RCCL without linking it: ctx points at {ncclComm_t comm; address of ncclAllGather} -- both
 * belong to the caller's process (torch.distributed's communicator and the librccl.so it loaded) */
typedef struct smalfit_rccl_ctx {
  void* comm;                  /* ncclComm_t */
  void* nccl_all_gather;       /* ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) */
} smalfit_rccl_ctx;
int smalfit_rccl_allgather(void* ctx, const float* send, float* recv, int count, void* stream);

/* ---- Prior.__call__ ---------------------------------------------------------------------------------
 * replaces: Prior.__call__(x)                                 reference smal_fitter/priors/pose_prior_35.py:112-124
 * x (N,105) -> out (N,105) = (((x - mean) prec) * mask)^2 with the prior given to set_pose_prior */
int smalfit_pose_prior(smalfit_engine* engine, void* stream, int N, const float* x, float* out);
int smalfit_pose_prior_backward(smalfit_engine* engine, void* stream, int N, const float* x, const float* dout,
                                float* dx);

/* ---- SMALFitter.get_temporal ----------------------------------------------------------------------------
 * replaces: SMALFitter.get_temporal(w_temp) and its backward    reference smal_fitter/smal_fitter.py:177-190
 * losses (3,) = joint, global, trans; gradients wrt the raw (unmasked) parameters; any g_* may be NULL */
int smalfit_temporal(smalfit_engine* engine, void* stream, int N, float w_temp, const float* global_rotation,
                     const float* joint_rotations, const float* trans, const float* global_mask,
                     const float* rotation_mask, float* losses, float* g_global_rotation,
                     float* g_joint_rotations, float* g_trans);

/* ---- fitter_3d: SMAL-to-mesh objective -----------------------------------------
 * replaces: Stage.forward / Stage.step                       reference fitter_3d/trainer.py:205-241
 * and the PyTorch3D v0.2.5 calls inside it (sample_points_from_meshes, chamfer_distance, mesh_edge_loss,
 * mesh_normal_consistency, mesh_laplacian_smoothing("uniform")) together with their autograd.
 *
 * smalfit_mesh_objective: the deforming source meshes, all of one topology (faces: host, (F,3) int32; every face
 * must have 3 distinct vertices).  Holds the edge / one-ring / face-pair tables and the work buffers for up to
 * max_meshes meshes and max_points target points per mesh. */
typedef struct smalfit_mesh_objective smalfit_mesh_objective;
typedef struct smalfit_mesh_targets smalfit_mesh_targets;
#define SMALFIT_NUM_MESH_LOSS_TERMS 5 /* chamfer, edge, normal, laplacian (unweighted), weighted total */

int smalfit_mesh_objective_create(int num_verts, int num_faces, const int* faces /*host*/, int max_meshes,
                                  int max_points, smalfit_mesh_objective** out);
void smalfit_mesh_objective_destroy(smalfit_mesh_objective* objective);
/* unique edges and pairs of faces sharing an edge (Meshes.edges_packed; the pair table of mesh_normal_consistency) */
int smalfit_mesh_objective_counts(const smalfit_mesh_objective* objective, int* num_edges, int* num_face_pairs);
/* verts = lbs_verts + trans + deform_verts (SMAL3DFitter.forward, trainer.py:94-108; deform_verts may be NULL), then
 * losses[0..3] = chamfer(points, verts), edge, normal, laplacian; losses[4] = sum of weights[i] * term over the terms
 * with weights[i] > 0 (weights: host, order w_chamfer, w_edge, w_normal, w_laplacian; trainer.py:31,203).
 * lbs_verts (N,V,3)  trans (N,3)  deform_verts (N,V,3)  points (N,S,3) (ignored when w_chamfer <= 0)
 * -> verts_out (N,V,3) or NULL, losses (5, device), dverts (N,V,3) = d total / d verts (also the gradient of
 * deform_verts), dtrans (N,3).  Chain dverts through smalfit_lbs_backward for the SMAL parameters.
 * Units and place: nothing is normalised.  The chamfer, edge and Laplacian terms and every gradient are built from differences
 * of coordinates: a translation that is exact in float32 changes no bit of them, and at a unit of length 2^k times another they are
 * the exact multiples (4^k, 4^k, 2^k) of their bits while no squared difference underflows and |n|^2 |n'|^2 of no face pair
 * overflows (k of about -45 ... 35 on a mesh of extent 1).  The normal term is cos = <n, n'> / sqrt(max(|n|^2 |n'|^2, 1e-16)), torch's
 * clamp on a length^8: it depends on the unit.  Between two units in which no pair is under the clamp it keeps its bits (its
 * gradient times 2^-k); a pair with a zero normal reads 1 - cos = 1 exactly, a collapsed face included. */
int smalfit_mesh_objective_eval(smalfit_mesh_objective* objective, void* stream, int num_meshes,
                                const float* lbs_verts, const float* trans, const float* deform_verts,
                                const float* points, int num_points, const float* weights /*host*/,
                                float* verts_out, float* losses, float* dverts, float* dtrans);

/* smalfit_mesh_targets: the target meshes, packed (all arguments host): vert_counts / face_counts (num_meshes),
 * verts (sum V,3), faces (sum F,3) with indices local to each mesh.
 * replaces: the Meshes object of fitter_3d/utils.py:253 as far as sample_points_from_meshes needs it */
int smalfit_mesh_targets_create(int num_meshes, const int* vert_counts, const int* face_counts, const float* verts,
                                const int* faces, smalfit_mesh_targets** out);
void smalfit_mesh_targets_destroy(smalfit_mesh_targets* targets);
/* replaces: sample_points_from_meshes(target_meshes, num_points)   trainer.py:209
 * face ~ area, barycentric (1 - sqrt u, sqrt u (1 - v), sqrt u v); Philox-4x32-10 keyed by `seed`, counter
 * (sample, mesh, iteration): the same (seed, iteration) always gives the same points.  points (N,S,3) device. */
int smalfit_mesh_targets_sample(smalfit_mesh_targets* targets, void* stream, int num_points,
                                unsigned long long seed, unsigned int iteration, float* points);
/* the same points, bit for bit (the same Philox draws, the same face), and with every point the unit normal of the face it was
 * sampled on: that face's (b - a) x (c - a) over its length, the zero vector for a degenerate face.  normals (N,S,3) device. */
int smalfit_mesh_targets_sample_normals(smalfit_mesh_targets* targets, void* stream, int num_points,
                                        unsigned long long seed, unsigned int iteration, float* points, float* normals);
/* ... and, beside them, one boundary byte per point: 1 when the face it was sampled on has a boundary edge (an edge no other face
 * of its mesh uses) or a corner that ends one, else 0.  normals (N,S,3) and boundary (N,S bytes) may each be NULL; the two
 * samplers above ARE this call with NULLs, and the points are theirs bit for bit. */
int smalfit_mesh_targets_sample_attrs(smalfit_mesh_targets* targets, void* stream, int num_points, unsigned long long seed,
                                      unsigned int iteration, float* points, float* normals, unsigned char* boundary);

/* ---- the scan index: a grid over every target mesh, for dense scans --------------------------------------------------------
 * The vertex -> surface direction of the surface term (smalfit_mesh_surface_eval*, smalfit_fit3d_step_surface and later) and of
 * smalfit_mesh_score tests every fitted vertex against every target triangle.  With an index on the targets it walks, per
 * vertex, the cells of a uniform grid over the target's bounding box outwards from the vertex's own cell -- a triangle is listed
 * in every cell its bounding box overlaps, a triangle overlapping more than 64 cells on a short list every vertex tests first --
 * and stops when no triangle it has not tested can be as near as the nearest it has: the distance to the unvisited part of the
 * box, less 256 ulp of the largest coordinate, exceeds it.  A vertex that is not done once the cells it has walked number twice the
 * mesh's faces (or after 48 rings) scans the whole mesh as before.  THE INDEX NEVER CHANGES A RESULT: the match of a vertex is the least float32 d^2 over all triangles of its
 * target, the lowest face among equal values, by the same arithmetic on the same records; every output of every call is bit for
 * bit what it is without the index (with max_dist_vert on, a vertex whose match lies beyond it may be dropped before its match
 * is known: it is dropped either way).  Off until asked for; built on the host from the handle's meshes, which are read back
 * once; all or nothing, every mesh of the handle gets a grid; calling it again rebuilds; a refusal (a non-finite target vertex,
 * a bad block) leaves the handle as it was and returns 1.  smalfit_mesh_targets_destroy frees it.
 * The point -> surface direction, the chamfer scans and the sampler do not read it. */
typedef struct smalfit_scan_index_args {
  unsigned int struct_size; /* sizeof(smalfit_scan_index_args) */
  float cell_scale;         /* cell edge = cell_scale * sqrt(surface area / faces); 0 = the library's own (2).  For tests and
                               tuning: the results do not depend on it */
} smalfit_scan_index_args;
typedef struct smalfit_scan_index_stats {
  unsigned int struct_size; /* sizeof(smalfit_scan_index_stats), set by the caller */
  int dims[3];              /* cells along x, y, z */
  int cells;                /* their product */
  int occupied_cells;       /* cells that list a triangle */
  int entries;              /* (cell, triangle) pairs listed */
  int oversize;             /* triangles on the oversize list */
  int largest_cell;         /* most triangles listed in one cell */
  unsigned long long bytes; /* device bytes of this mesh's share of the index */
} smalfit_scan_index_stats;
int smalfit_mesh_targets_build_index(smalfit_mesh_targets* targets, const smalfit_scan_index_args* args);
/* the grid of target mesh `mesh`; returns 1 with a message when the handle has no index */
int smalfit_mesh_targets_index_stats(const smalfit_mesh_targets* targets, int mesh, smalfit_scan_index_stats* out);

/* ---- the chamfer term gated for partial scans ---------------------------------------------------------------------------
 * The chamfer term matches every target point to its nearest fitted vertex and every fitted vertex to its nearest target point,
 * whatever that is: on a target with a hole the vertices over the hole are pulled to its rim.  Three opt-in gates per direction
 * decide which matches count; THIS PROJECT'S definitions (the reference has none).  Per mesh: target points x_s, s < S, each with
 * a unit normal m_s and a boundary byte b_s; fitted (composed) vertices y_v, v < V, each with a unit normal u_v.
 *   u_v            the fitted vertex normal of the gated surface term above (sum of the incident faces' normals over its length).
 *   m_s, b_s       the unit normal of the target face the point was sampled on, and 1 when that face has a boundary edge or a
 *                  corner that ends one, else 0 (smalfit_mesh_targets_sample_attrs); for the caller's points the caller's.
 *   d^2            the term's own float32 expression fma(dz, dz, fma(dy, dy, dx dx)); nearest = the lowest index among equal d^2.
 *   compatible     <a, b> >= c for the two unit normals, in float32; a zero normal gives 0 on the left, a NaN compares false.
 *                  c <= -1 switches the test off for its direction: no normal is read, staged or computed for it.  c <= 1.
 *   point -> vertex   nn(s) = the nearest vertex among those compatible with m_s under min_cos_point.  Point s is KEPT when such a
 *                  vertex exists and (max_dist_point is off or d^2 <= tau^2); tau^2 is formed once on the host in float32; tau <= 0
 *                  or not finite: off.  A dropped point has nn = -1.  No boundary rule here: a rim point is real data.
 *   vertex -> point   nn'(v) = the nearest point among those compatible with u_v under min_cos_vert.  Vertex v is KEPT when such a
 *                  point exists, (max_dist_vert is off or d^2 <= tau^2), and not (reject_boundary and b of nn'(v) != 0).  The
 *                  boundary rule judges the WINNER; it does not filter candidates (that would only match the vertex to the next
 *                  ring of points inwards).
 *   loss           chamfer = 1/(N S) sum over kept s of d^2 + 1/(N V) sum over kept v of d^2.  The denominators stay N S and N V:
 *                  a kept match's gradient is what it is ungated, and the loss does not jump with a count.
 *   gradient       d chamfer / d y_v = 2/(N V) [v kept] (y_v - x_nn'(v)) + 2/(N S) sum over kept s with nn(s) = v of (y_v - x_s),
 *                  times w_chamfer.  No gate and no normal is differentiated through.
 *   kept           kept[n] = (kept points, kept vertices) lets a caller renormalise.
 * gate == NULL, or every gate off and no mask asked for: exactly the ungated call, launch for launch and bit for bit; `kept` then
 * reads (S, V) without anything being counted.  With w_chamfer <= 0 a gate block is accepted and ignored, and `kept` reads (0, 0).
 * Not here: gates for the edge, normal or Laplacian terms or for smalfit_mesh_score, spatial acceleration.  The soft robust kernel
 * is smalfit_robust_args below. */
typedef struct smalfit_chamfer_gate_args {
  unsigned struct_size;       /* sizeof(smalfit_chamfer_gate_args) of the caller's header; checked before any other field */
  float max_dist_point;       /* tau of point -> vertex; <= 0 or not finite: off */
  float max_dist_vert;        /* tau of vertex -> point */
  float min_cos_point;        /* c of point -> vertex, <= 1; <= -1: off */
  float min_cos_vert;         /* c of vertex -> point */
  int reject_boundary;        /* != 0: the boundary rule (vertex -> point) */
  const float* point_normals; /* (N,S,3) m_s of the caller's points: needed when a min_cos gate is on and the points are the caller's;
                                 must be NULL in a step that samples its points (it draws them with the points) */
  const unsigned char* point_boundary; /* (N,S) b_s of the caller's points: needed with reject_boundary; NULL in a sampling step */
  int* kept;                  /* (N,2): kept points | kept vertices of every mesh */
  unsigned char* point_kept;  /* optional (N,S): 1 kept, 0 dropped */
  unsigned char* vert_kept;   /* optional (N,V) */
  int* point_nn;              /* optional (N,S): nn(s), -1 for a dropped point */
  int* vert_nn;               /* optional (N,V): nn'(v), -1 when no compatible point was found */
} smalfit_chamfer_gate_args;
/* smalfit_mesh_objective_eval with the gates; that call IS this one with gate = NULL.  targets may be NULL (the points, their normals
 * and boundary bytes are the caller's); when given, its mesh count must be num_meshes.  A refused block launches nothing and
 * leaves every output alone */
int smalfit_mesh_objective_eval_gated(smalfit_mesh_objective* objective, void* stream, int num_meshes,
                                      const float* lbs_verts, const float* trans, const float* deform_verts,
                                      const float* points, int num_points, const float* weights /*host*/,
                                      float* verts_out, float* losses, float* dverts, float* dtrans,
                                      smalfit_mesh_targets* targets, const smalfit_chamfer_gate_args* gate);

/* ---- how good a 3-D fit is: exact surface distances both ways, per mesh -------------------------------------------------
 * No counterpart in the reference, whose fitter_3d contains no evaluation code: the definitions below are THIS PROJECT'S.
 *   distance       from a point p to the closed triangle (a, b, c): the square root of the minimum of
 *                    - the three squared point-to-segment distances, the segment's parameter clamped to [0, 1] (a segment of
 *                      zero length is its end point), and
 *                    - the squared distance to the plane, when the normal n = (b - a) x (c - a) is not zero and p projects
 *                      inside: <(b - a) x (p - a), n>, <(c - b) x (p - b), n> and <(a - c) x (p - c), n> are all >= 0.
 *                  A degenerate triangle (collinear or coincident corners) is exactly its three segments.  float32 throughout.
 *                  Every term is a difference of coordinates: an exact translation changes no bit, and at a unit of length 2^k
 *                  times another the distances are the exact multiple 2^k of their bits while the plane product (distance x
 *                  twice the face's area, squared: a length^6) and |n|^2 stay normal -- k of about -16 ... 22 at extent 1.
 *   vert_dist      [n][v] = the least distance from fitted vertex v of mesh n to the triangles of TARGET mesh n
 *   point_dist     [n][s] = the least distance from points[n][s] to the triangles of the FITTED mesh n (verts[n] with the
 *                  faces given to the objective's create call)
 *                  Both are minima over float32 values: bit-reproducible, whatever order the triangles are scanned in.  No
 *                  face index is returned: on a shared edge or vertex several faces are equally near.
 *   sums           [n][dir] = sum d, sum d^2, max d over the queries of direction dir (0: the V fitted vertices, 1: the S
 *                  points), float32 sums in a fixed order
 *   within         [n][dir][t] = queries of that direction with d <= thresholds[t]
 * Quotients are the host's: mean = sum d / count, RMS = sqrt(sum d^2 / count), Hausdorff = the larger of the two maxima,
 * precision / recall / F-score at t from `within` (smalify_amd/metrics.py::summarise_mesh_score forms them in float64).
 * Without points only direction 0 is scored; the rows of direction 1 are zero.
 * Everything is enqueued on `stream`; nothing synchronises.  A refused block launches nothing and leaves every output alone.
 * The call uses the objective's work buffers: it must not overlap another call on the same objective (calls enqueued on one
 * stream never do). */
#define SMALFIT_MAX_SCORE_THRESHOLDS 8
typedef struct smalfit_mesh_score_args {
  unsigned struct_size;       /* sizeof(smalfit_mesh_score_args) of the caller's header; checked before any other field */
  int num_meshes;             /* N <= the objective's max_meshes, == the targets' mesh count */
  const float* verts;         /* (N,V,3) fitted vertices: verts_out of smalfit_mesh_objective_eval / smalfit_fit3d_step */
  const float* points;        /* (N,S,3) points on the target surfaces (smalfit_mesh_targets_sample), or NULL: one direction only */
  int num_points;             /* S <= the objective's max_points; 0 when points is NULL */
  int num_thresholds;         /* T in 0..8 */
  float thresholds[SMALFIT_MAX_SCORE_THRESHOLDS];  /* host values, each finite and > 0, in the model's units */
  float* vert_dist;           /* (N,V) or NULL: fitted vertex -> target surface */
  float* point_dist;          /* (N,S) or NULL: target point -> fitted surface; must be NULL without points */
  float* sums;                /* (N,2,3): per direction sum d, sum d^2, max d; the rows of direction 1 are zero without points */
  int* within;                /* (N,2,T) or NULL; must be NULL when T == 0 */
} smalfit_mesh_score_args;
int smalfit_mesh_score(smalfit_mesh_objective* objective, smalfit_mesh_targets* targets, void* stream,
                       const smalfit_mesh_score_args* args);

/* ---- an opt-in point-to-surface term, both ways, with its gradient -----------------------------------------------------
 * No counterpart in the reference (PyTorch3D grew point_mesh_face_distance after the 0.2.5 it pins): THIS PROJECT'S definition.
 * With d(p, T) the distance of smalfit_mesh_score above from a point to a closed triangle and d(p, M) its minimum over the
 * faces of the mesh M:
 *   L_ps = 1/(N S) sum_n sum_s d^2(points[n][s], fitted mesh n)      "point -> surface"
 *   L_vs = 1/(N V) sum_n sum_v d^2(verts[n][v],  target mesh n)      "vertex -> surface"
 *   term = w_point_surface L_ps + w_vert_surface L_vs                 (a weight <= 0 skips its direction: its loss reads 0)
 * the normalisation of the chamfer term.  Unlike that term it is zero for a perfect fit.
 *   nearest face   the lowest face index among equal float32 d^2.  The closest point q is the one of the candidate that
 *                  reaches the minimum, the first in the order (segment ab, bc, ca, plane): a segment's clamped parameter t
 *                  gives the barycentrics (1 - t, t, 0) on that edge; the plane gives (s1, s2, s0) / (s0 + s1 + s2) with the
 *                  three edge functions of smalfit_mesh_score (their sum is |n|^2 up to rounding: over the sum, the weights add
 *                  up to 1).  The residual r = p - q is formed from the winner's own intermediates.
 *   gradient       by the envelope theorem, nothing is differentiated through the barycentrics:
 *                    vertex -> surface:  d term / d verts[n][v] += w_vert_surface 2/(N V) r
 *                    point -> surface:   the corners i of the winning fitted face each receive -w_point_surface 2/(N S) b_i r
 *                  A degenerate triangle remains its three segments.
 * Every minimum is unique (distance, then face index) and every sum has a fixed order: the same call gives the same bits.
 * Cost: linear in the scanned faces (V F_target + S F pair tests per mesh), no acceleration structure.
 * A refused block launches nothing and leaves every output alone.  The call uses the objective's work buffers. */
typedef struct smalfit_surface_term_args {
  unsigned struct_size;       /* sizeof(smalfit_surface_term_args) of the caller's header; checked before any other field */
  int num_meshes;             /* N <= the objective's max_meshes (in a step: the step's num_meshes) */
  float w_point_surface;      /* <= 0: the direction is skipped, its targets' points are not read */
  float w_vert_surface;       /* <= 0: skipped; > 0 needs the targets, one per mesh */
  const float* verts;         /* (N,V,3) fitted vertices; must be NULL in a step (its composed vertices are used) */
  const float* points;        /* (N,S,3) points on the target surfaces; must be NULL in a step (its own points are used) */
  int num_points;             /* S <= the objective's max_points; not read in a step */
  float* losses;              /* (3, device): L_ps, L_vs, the weighted term */
  float* rows;                /* optional (N,2): per mesh sum d^2 of the points | of the vertices, not normalised */
  float* dverts;              /* optional (N,V,3): d term / d verts, written, not accumulated */
  float* dtrans;              /* optional (N,3): its sum over the vertices of a mesh */
  int* point_face;            /* optional (N,S): face of the fitted topology nearest to every point */
  float* point_bary;          /* optional (N,S,3), only with point_face: where on it */
  int* vert_face;             /* optional (N,V): face of TARGET mesh n (index within that mesh) nearest to every vertex */
  float* vert_bary;           /* optional (N,V,3), only with vert_face */
  float* point_residual;      /* optional (N,S,3), only with point_face: r = point - (its closest point), as the gradient uses it */
  float* vert_residual;       /* optional (N,V,3), only with vert_face */
  float* step_total;          /* optional (1), a step only: args->losses[4] + the weighted term, what the step descends on;
                                 smalfit_mesh_surface_eval does not write it */
} smalfit_surface_term_args;
/* the term alone.  `targets` may be NULL when w_vert_surface <= 0.  The correspondences of a skipped direction are not written */
int smalfit_mesh_surface_eval(smalfit_mesh_objective* objective, smalfit_mesh_targets* targets, void* stream,
                              const smalfit_surface_term_args* args);

/* ---- Stage.step in one call ------------------------------------------------------------------------------------
 * replaces: one iteration of Stage.run                      reference fitter_3d/trainer.py:229-241,257-262
 *   new_src_verts = smal_3d_fitter(); loss = forward(...); loss.backward(); optimizer.step()
 * = SMAL forward on [global_rot | joint_rot], target points sampled (or taken from `points`), the four-term objective,
 * its gradient back through the SMAL model, torch.optim.Adam on every parameter whose learning rate is > 0 (the
 * parameter groups of trainer.py:113-119 with their custom learning rates) -- 14 kernel launches, no host
 * synchronisation.  All pointers are device pointers unless noted.  log_beta_scales is read, never trained
 * (requires_grad=False in the reference, trainer.py:64-65). */
typedef struct smalfit_fit3d_args {
  int num_meshes;                  /* N */
  int num_betas;                   /* columns of betas (20) */
  int num_points;                  /* S target points per mesh (3000 in the reference) */
  float* betas;                    /* (N,num_betas) */
  const float* log_beta_scales;    /* (N,6) or NULL */
  float* global_rot;               /* (N,3) */
  float* joint_rot;                /* (N,34,3) */
  float* trans;                    /* (N,3) */
  float* deform_verts;             /* (N,V,3) or NULL (then treated as zero and not trainable) */
  /* Adam: learning rate per parameter (<= 0: frozen in this stage) and its state (exp_avg, exp_avg_sq), same shapes */
  float lr_betas, lr_global_rot, lr_joint_rot, lr_trans, lr_deform_verts;
  float *m_betas, *v_betas, *m_global_rot, *v_global_rot, *m_joint_rot, *v_joint_rot, *m_trans, *v_trans,
        *m_deform_verts, *v_deform_verts;
  float beta1, beta2, eps;         /* torch defaults 0.9, 0.999, 1e-8 (trainer.py:194) */
  int adam_t;                      /* 1-based step count of this stage's optimiser */
  float weights[4];                /* w_chamfer, w_edge, w_normal, w_laplacian; <= 0 skips the term */
  const float* points;             /* (N,S,3) target points, or NULL: sample them from the target meshes */
  unsigned long long seed;         /* sampler key and counter, see smalfit_mesh_targets_sample */
  unsigned int iteration;
  float* points_out;               /* optional (N,S,3): the target points this step used */
  float* losses;                   /* (5): chamfer, edge, normal, laplacian, weighted total -- before the update */
  float* verts_out;                /* optional (N,V,3): the vertices the loss was evaluated at */
} smalfit_fit3d_args;
/* `targets` may be NULL when args->points is given or w_chamfer <= 0 */
int smalfit_fit3d_step(smalfit_engine* engine, smalfit_mesh_objective* objective, smalfit_mesh_targets* targets,
                       void* stream, const smalfit_fit3d_args* args);
/* smalfit_fit3d_step with the surface term added to what the step descends on.  surface == NULL, or both of its weights <= 0:
 * exactly smalfit_fit3d_step, launch for launch and bit for bit (which IS this call with surface = NULL).  Otherwise the term is
 * evaluated at the step's composed vertices against the step's own points -- sampled or taken from the caller as before, also
 * when w_chamfer <= 0 -- and its vertex gradient is added to the step's (one float32 addition per coordinate, as a caller of
 * smalfit_mesh_surface_eval would add it) before the SMAL adjoint and Adam read it, so trans, deform_verts and the SMAL
 * parameters all descend on the sum.  args->losses keeps its five entries WITHOUT the term; surface->losses (3) carries the
 * term, and the caller adds the two (or asks for surface->step_total).  `targets` is needed when w_vert_surface > 0 or points are to be sampled. */
int smalfit_fit3d_step_surface(smalfit_engine* engine, smalfit_mesh_objective* objective, smalfit_mesh_targets* targets,
                               void* stream, const smalfit_fit3d_args* args, const smalfit_surface_term_args* surface);

/* ---- the surface term gated for partial scans ---------------------------------------------------------------------------
 * A target with holes, an unseen side or thin sheets pulls the fitted surface to whatever is nearest.  Three opt-in gates decide
 * which matches count; THIS PROJECT'S definitions.  d(p, T), the candidate order (ab, bc, ca, plane), the lowest-face tie rule
 * and the residual r are those of the term above and do not change.  Both meshes are taken to be wound consistently outward.
 *   compatibility  A query carries a unit normal u, a scanned triangle its record normal n = (b - a) x (c - a), unnormalised.
 *                  With g = <u, n> the pair is compatible with threshold c when  g |g| / |n|^2 >= c |c|  (the signed squared
 *                  cosine, monotone in the cosine).  A degenerate triangle or a zero u gives 0 on the left: compatible exactly
 *                  when c <= 0.  c <= -1 switches the test off for its direction: no normals are read or computed.
 *   gated nearest  the nearest face among the compatible ones, by the same (d^2 bits, face index) key; a query with no
 *                  compatible face finds none.
 *   query normals  fitted vertex: the sum over its incident faces, in ascending face index, of their unnormalised normals n,
 *                  over its length (a zero length gives the zero vector).  Target point: the unit normal of the target face it
 *                  was sampled on (smalfit_mesh_targets_sample_normals); for the caller's points the caller supplies them.
 *   truncation     a query is dropped when d^2 > tau^2, tau^2 formed once on the host in float32; tau <= 0 or not finite
 *                  switches truncation off for its direction.
 *   boundary       vertex -> target only.  A target's boundary edges are the undirected vertex pairs used by exactly one of its
 *                  faces, its boundary vertices their end points.  A vertex is dropped when the winning candidate of its nearest
 *                  face is a segment and that segment is a boundary edge, or its clamped parameter is exactly 0 and the start
 *                  corner is a boundary vertex, or exactly 1 and the end corner is one.
 *   kept           a query is kept when it found a face and no gate dropped it.  A dropped query contributes 0 to L_ps / L_vs
 *                  and to `rows`; its residual and barycentrics are 0, so it contributes nothing to any gradient; its optional
 *                  face output is -1.  The denominators stay N S and N V, not the kept counts: a kept query's gradient is what
 *                  it is ungated, and the loss does not jump when a count changes.  `kept` lets a caller renormalise.
 * No gate is differentiated through (they are piecewise constant, as the envelope theorem already assumes).  gate == NULL, or
 * every gate off: exactly the ungated call, launch for launch and bit for bit; with a block whose gates are all off `kept` reads
 * (S, V) for the directions that ran (0 for a skipped one) without anything being counted.
 * Not here: gates for smalfit_mesh_score, any spatial acceleration.  The soft robust kernel is smalfit_robust_args below. */
typedef struct smalfit_surface_gate_args {
  unsigned struct_size;       /* sizeof(smalfit_surface_gate_args) of the caller's header; checked before any other field */
  float max_dist_point;       /* tau of point -> surface; <= 0 or not finite: off */
  float max_dist_vert;        /* tau of vertex -> surface */
  float min_cos_point;        /* c of point -> surface, <= 1; <= -1: off */
  float min_cos_vert;         /* c of vertex -> surface */
  int reject_boundary;        /* != 0: the boundary rule */
  const float* point_normals; /* (N,S,3) unit normals of the caller's points, needed when min_cos_point is on and the points are
                                 the caller's; must be NULL in a step that samples its points (it draws the normals with them) */
  int* kept;                  /* (N,2): kept points | kept vertices of every mesh (0 for a skipped direction) */
  unsigned char* point_kept;  /* optional (N,S): 1 kept, 0 dropped */
  unsigned char* vert_kept;   /* optional (N,V) */
  float* vert_normals;        /* optional (N,V,3), only with min_cos_vert on: the fitted normals the gate used */
} smalfit_surface_gate_args;
/* smalfit_mesh_surface_eval / smalfit_fit3d_step_surface with the gates; those two ARE these calls with gate = NULL.  A refused
 * block launches nothing and leaves every output alone */
int smalfit_mesh_surface_eval_gated(smalfit_mesh_objective* objective, smalfit_mesh_targets* targets, void* stream,
                                    const smalfit_surface_term_args* args, const smalfit_surface_gate_args* gate);
int smalfit_fit3d_step_gated(smalfit_engine* engine, smalfit_mesh_objective* objective, smalfit_mesh_targets* targets,
                             void* stream, const smalfit_fit3d_args* args, const smalfit_surface_term_args* surface,
                             const smalfit_surface_gate_args* gate);
/* ... and with the gates of the chamfer term; smalfit_fit3d_step_gated IS this call with chamfer_gate = NULL.  A chamfer gate block
 * needs no surface block.  Where both gate sets want the fitted vertex normals or the sampled normals, they are produced once */
int smalfit_fit3d_step_partial(smalfit_engine* engine, smalfit_mesh_objective* objective, smalfit_mesh_targets* targets,
                               void* stream, const smalfit_fit3d_args* args, const smalfit_surface_term_args* surface,
                               const smalfit_surface_gate_args* surface_gate, const smalfit_chamfer_gate_args* chamfer_gate);

/* ---- a Geman-McClure robust kernel on both data terms -------------------------------------------------------------------
 * A hard cap leaves a match in or out: it jumps when a query crosses tau and leaves a dropped vertex to the regularisers.  The
 * robust kernel keeps every match, is quadratic near the surface and lets the pull of a far match fade smoothly to nothing --
 * stray clusters (a floor, a stand) and a second animal show neither a rim nor a flipped normal.  THIS PROJECT'S definitions.
 * For a KEPT match with float32 squared distance d^2 (the term's own bits) and its direction's scale sigma, the host forms
 * s^2 = sigma sigma once, in float32; then, in float32,
 *   u   = s^2 / (s^2 + d^2)      one add, one correctly rounded divide
 *   rho = d^2 u                  what the sums take in place of d^2: sigma^2 d^2 / (sigma^2 + d^2), -> sigma^2 far away
 *   w   = u u                    = d rho / d (d^2): what the match's gradient is multiplied by
 * d^2 = 0 gives u = 1, rho = 0, w = 1.
 *   matching       untouched: rho is monotone in d^2, so the nearest vertex / point / face, the compatibility tests, the tie rule,
 *                  truncation, the boundary rule, `kept`, nn, faces, barycentrics and residuals are those of the same call
 *                  without the block.  With the gates the kernel applies to the matches they keep.
 *   normalisation  the denominators stay N S and N V.
 *   chamfer        loss = 1/(N S) sum over kept s of rho(d^2_s) + 1/(N V) sum over kept v of rho(d^2_v);
 *                  d chamfer / d y_v = 2/(N V) [v kept] w(d^2_v) (y_v - x_nn'(v)) + 2/(N S) sum over kept s with nn(s) = v of
 *                  w(d^2_s) (y_v - x_s), times w_chamfer.  sigma_chamfer_point governs the sum over the points (both its loss
 *                  and the second gradient sum), sigma_chamfer_vert the vertices' own matches.
 *   surface term   L_ps and L_vs (and `rows`) sum rho; a vertex receives w_vert_surface 2/(N V) w r, the corners of a point's
 *                  face -w_point_surface 2/(N S) w b_i r.  The optional vert_residual / point_residual stay the geometric r.
 *   w              is not differentiated through beyond what it is: w is exactly the derivative of rho.
 *   scales         four, independent.  A scale is OFF when sigma <= 0 or sigma is not finite, and for a direction that is
 *                  skipped; it is REFUSED when sigma > 0 is finite but its float32 square is not a normal number.
 *   losses         with a scale on, args->losses (chamfer, and through it the total) and surface->losses carry the robust values.
 *   weight sums    chamfer_weight_sums / surface_weight_sums [n] = (sum of w over the kept points, over the kept vertices) of
 *                  mesh n: float32 sums of per-block partials in block order, the way `kept` is counted; how much of the data
 *                  still pulls.  A direction that ran with its scale off reads its kept count as a float (every weight is 1), a
 *                  skipped direction 0.
 *   weights        the four optional per-query outputs hold w, 0 for a dropped query; one given for a direction whose scale is
 *                  off is refused.
 * robust == NULL, or every scale off and no output asked for: the launches and the bits of the call without the block.  A
 * refused block launches nothing and leaves every output alone.  Non-finite coordinates stay in bounds, value unspecified.
 * Not here: other kernels (Huber, Cauchy), annealing sigma, robust forms of the edge, normal or Laplacian terms or of
 * smalfit_mesh_score. */
typedef struct smalfit_robust_args {
  unsigned struct_size;          /* sizeof(smalfit_robust_args) of the caller's header; checked before any other field */
  float sigma_chamfer_point;     /* sigma of chamfer point -> vertex; <= 0 or not finite: off */
  float sigma_chamfer_vert;      /* sigma of chamfer vertex -> point */
  float sigma_surface_point;     /* sigma of point -> surface */
  float sigma_surface_vert;      /* sigma of vertex -> surface */
  float* chamfer_weight_sums;    /* optional (N,2): sum of w over the kept points | kept vertices of the chamfer term */
  float* surface_weight_sums;    /* optional (N,2): ... of the surface term */
  float* chamfer_point_weights;  /* optional (N,S): w of every point's chamfer match, 0 for a dropped point */
  float* chamfer_vert_weights;   /* optional (N,V) */
  float* surface_point_weights;  /* optional (N,S) */
  float* surface_vert_weights;   /* optional (N,V) */
} smalfit_robust_args;
/* the gated calls with the robust kernel; smalfit_mesh_objective_eval_gated, smalfit_mesh_surface_eval_gated and
 * smalfit_fit3d_step_partial ARE these calls with robust = NULL.  Any of the gate blocks may be NULL as before.  The chamfer
 * call reads the two chamfer scales and outputs, the surface call the two surface ones (outputs of the other term are refused);
 * a step reads all of them, the surface ones only with a surface block */
int smalfit_mesh_objective_eval_robust(smalfit_mesh_objective* objective, void* stream, int num_meshes,
                                       const float* lbs_verts, const float* trans, const float* deform_verts,
                                       const float* points, int num_points, const float* weights /*host*/,
                                       float* verts_out, float* losses, float* dverts, float* dtrans,
                                       smalfit_mesh_targets* targets, const smalfit_chamfer_gate_args* gate,
                                       const smalfit_robust_args* robust);
int smalfit_mesh_surface_eval_robust(smalfit_mesh_objective* objective, smalfit_mesh_targets* targets, void* stream,
                                     const smalfit_surface_term_args* args, const smalfit_surface_gate_args* gate,
                                     const smalfit_robust_args* robust);
int smalfit_fit3d_step_robust(smalfit_engine* engine, smalfit_mesh_objective* objective, smalfit_mesh_targets* targets,
                              void* stream, const smalfit_fit3d_args* args, const smalfit_surface_term_args* surface,
                              const smalfit_surface_gate_args* surface_gate, const smalfit_chamfer_gate_args* chamfer_gate,
                              const smalfit_robust_args* robust);

/* ---- rigid pre-alignment: multi-start iterative closest point ----------------------------------------------------------------
 * Every term above assumes that the fitted mesh already stands roughly where its target stands and faces the same way; the
 * chamfer term is a local descent and settles back to front when it does not.  This call finds the rigid motion [R | t] that
 * carries vertices x_v, v < V, onto points p_s, s < S, by ICP from K starting orientations at once, and says which start ended
 * best.  THIS PROJECT'S definitions (the reference has none).  A handle of its own: no engine, no objective, no targets; any
 * (N,V,3) vertices against any (N,S,3) points.  Everything is per mesh n and per start k, in float32.
 *   transform      12 floats, three rows [R_i0 R_i1 R_i2 t_i].  z = R x + t is formed, per coordinate i, by the one chain
 *                  fma(R_i2, x_2, fma(R_i1, x_1, fma(R_i0, x_0, t_i))).
 *   means          c_X, c_P: the means of the vertices and of the points of mesh n.  Each coordinate is summed by 256 lanes, lane l
 *                  taking the elements l, l + 256, ... in ascending order; the 64 lanes of a wave are added by a butterfly
 *                  (xor 32, 16, ... 1), the four waves in wave order; one float32 divide by the count.
 *   start          with `starts`: R = R_k, t_i = c_P_i - (R_k c_X)_i, the product by the chain fma(R_i2, c_2, fma(R_i1, c_1,
 *                  R_i0 c_0)): z = R_k (x - c_X) + c_P.  With `start_transforms`: the given 12 floats as they are.
 *   built-in starts   starts == NULL: the 24 rotations of the cube, the signed permutation matrices of determinant +1, in this
 *                  order: the permutations (a, b, c) of (0, 1, 2) in lexicographic order (012, 021, 102, 120, 201, 210), within
 *                  each the sign triples (s_0, s_1, s_2) in the order +++, ++-, +-+, +--, -++, -+-, --+, ---, keeping those for
 *                  which the matrix with R[0][a] = s_0, R[1][b] = s_1, R[2][c] = s_2 (zero elsewhere) has determinant +1.  Start
 *                  0 is the identity.
 *   one iteration  1. z_v = R x_v + t.
 *                  2. nn'(v) = the point nearest to z_v, nn(s) = the z nearest to p_s.  d^2 and the tie rule are the chamfer
 *                     term's: fma(dz, dz, fma(dy, dy, dx dx)), the lowest index among equal d^2.
 *                  3. the pairs (x_v, p_nn'(v)), each of weight w_vert / V, and (x_nn(s), p_s), each of weight w_point / S.  A
 *                     direction of weight 0 is not scanned.
 *                  4. R, t = argmin sum w |R x + t - p|^2 by Horn's closed form: on coordinates centred at c_X and c_P every
 *                     block of 64 queries sums 1, x, p, x p^T, |x|^2, |p|^2 and d^2 over its pairs (a wave butterfly); the
 *                     blocks are added in block order, then the two directions as fma(w_point / S, point sum, (w_vert / V)
 *                     vertex sum).  With W the sum of the weights, the weighted means mx, mp and H = sum w x p^T - W mx mp^T, the
 *                     unit quaternion of R is the eigenvector of Horn's symmetric 4x4 matrix of H with the largest eigenvalue,
 *                     found by 8 cyclic Jacobi sweeps (6 rotations each, pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)); the largest
 *                     diagonal entry wins, the lowest index among equal ones.  The quaternion is normalised and R formed from
 *                     it: det R = +1 always, a reflection is never returned.  t = (c_P + mp) - R (c_X + mx).
 *                  5. rank test: with l1 >= l2 the two largest eigenvalues found, the rotation is DETERMINED when
 *                       l1 - l2 > 1e-5 sqrt(sum w |x|^2) sqrt(sum w |p|^2)
 *                     in float32 (the centred sums of 4.; a NaN compares false).  The right-hand side is the product of the two
 *                     roots, never the root of the product: every intermediate of the iteration is then of degree 2 at most
 *                     in the lengths, and the test holds wherever the sums themselves are normal float32 numbers.  Coincident or
 *                     collinear points or vertices fail it: the previous R is kept, only t is updated by the line above, and
 *                     kept_rotation counts the event.
 *                     Every output stays finite for finite input whose d^2 and unweighted sums of d^2 stay below float32's
 *                     largest number: a set of unit extent times up to about 2^60.  Beyond that d^2 is +inf: no match, a +inf
 *                     cost.  While, besides, the smallest d^2 that is not 0 stays a normal number (a unit extent times 2^-16
 *                     or more where correspondences are exact and d^2 is rounding alone), a call on inputs times 2^k gives R,
 *                     best, kept_rotation and the matches of the unscaled call, t times 2^k, scores and history times 2^2k,
 *                     bit for bit; far below, every d^2 is 0, every match is index 0 and no rotation is determined.
 *   place          a transform is about the origin, not about the centroid: t = c_P - R c_X is rounded at the size of the largest
 *                  coordinate, so z is accurate to about one ulp of that coordinate, however small the mesh.  A scan that lies far
 *                  from the origin should be re-centred first (the 3-D fitter's mesh loader does).
 *   cost, score    w_point / S sum_s d^2 + w_vert / V sum_v d^2 of a pair of scans, by the sums of 4.  `history` holds the cost
 *                  before every solve and after the last; `scores` is the cost under the final transform: one more pair of
 *                  scans after the last solve.  A skipped direction adds nothing.
 *   best           the lowest score, the lowest k among equal bits; a NaN score never wins (all NaN: 0).
 *   determinism    no atomics, every sum in a fixed order: the same call gives the same bits, and I iterations in one call give
 *                  the bits of I one-iteration calls chained through transforms -> start_transforms.
 * Everything is enqueued on `stream`; nothing synchronises.  A refused block launches nothing and leaves every output alone.  The
 * call uses the handle's work buffers: it must not overlap another call on the same handle.  Non-finite coordinates stay in
 * bounds, value unspecified.
 * The handle holds the work buffers for up to max_meshes (at most 65535) meshes of up to max_verts vertices and max_points points
 * and up to max_starts (at most 64) starts; a call may be smaller in every one of them and gives the same bits on a larger handle.
 * The two weights reach the device as the float32 quotients w_vert / V and w_point / S, one divide each on the host.
 * Not here: scale (similarity) estimation, robust weights, normals, the scan index.  Trimming: smalfit_trimmed_rigid_align below. */
typedef struct smalfit_rigid_aligner smalfit_rigid_aligner;
#define SMALFIT_MAX_RIGID_STARTS 64
#define SMALFIT_NUM_CUBE_ROTATIONS 24
typedef struct smalfit_rigid_align_args {
  unsigned struct_size;          /* sizeof(smalfit_rigid_align_args) of the caller's header; checked before any other field */
  int num_meshes;                /* N in 1 .. the handle's max_meshes */
  int num_verts;                 /* V in 1 .. the handle's max_verts */
  int num_points;                /* S in 1 .. the handle's max_points */
  const float* verts;            /* (N,V,3) device: x_v */
  const float* points;           /* (N,S,3) device: p_s */
  int num_starts;                /* K in 1 .. min(64, the handle's max_starts) */
  int iterations;                /* I in 0 .. 1000; 0 scores the starts only */
  const float* starts;           /* HOST (K,3,3) row-major proper rotations (finite, orthonormal with determinant +1 to within 1e-4),
                                    or NULL: the 24 built-in ones, and K must be 24 (unless start_transforms is given) */
  const float* start_transforms; /* optional, device (N,K,12): used as they are; `starts` must then be NULL */
  float w_point;                 /* weight of the pairs (x_nn(s), p_s); >= 0 and finite */
  float w_vert;                  /* weight of the pairs (x_v, p_nn'(v)); >= 0 and finite; not both 0 */
  float* transforms;             /* (N,K,12): the transform of every start after I iterations */
  float* scores;                 /* (N,K): the cost of every start under its final transform */
  int* best;                     /* (N) */
  float* best_transform;         /* (N,12): transforms[n][best[n]] */
  int* kept_rotation;            /* (N,K): how many of a start's I solves kept the previous rotation */
  float* history;                /* optional (N,K,I+1) */
  int* vert_nn;                  /* optional (N,K,V): nn'(v) of the score's scans; left alone when w_vert == 0 */
  int* point_nn;                 /* optional (N,K,S): nn(s) of the score's scans; left alone when w_point == 0 */
} smalfit_rigid_align_args;
int smalfit_rigid_aligner_create(int max_meshes, int max_verts, int max_points, int max_starts, smalfit_rigid_aligner** out);
void smalfit_rigid_aligner_destroy(smalfit_rigid_aligner* aligner);
int smalfit_rigid_align(smalfit_rigid_aligner* aligner, void* stream, const smalfit_rigid_align_args* args);

/* ---- trimmed rigid pre-alignment: partial, cluttered scans -----------------------------------------------------------------------
 * smalfit_rigid_align matches every vertex and every point and solves on all of the pairs: a scan that shows one side of the
 * animal, or that holds a floor, pulls every start off.  Trimmed ICP (Chetverikov's TrICP) keeps, per iteration and per direction,
 * only the pairs of smallest d^2.  THIS PROJECT'S definitions, per mesh n, start k and direction, in float32, on top of the ones
 * above.
 *   key            of query q: the pair (bits of its d^2 read as uint32, q).  d^2 is fma(dz, dz, fma(dy, dy, dx dx)) >= 0, so its
 *                  bits order as the value does.  A query without a match (non-finite input) has no key and is never kept.
 *                  A mesh with a non-finite coordinate has non-finite means, no query of it has a key, nothing is kept and every cost
 *                  of it is 0, not +inf as in smalfit_rigid_align: its score, its best and its transforms mean nothing.
 *   kept           the `keep` queries of the lowest keys, compared lexicographically: the lowest d^2, the lowest query index among
 *                  bit-equal d^2.  keep_vert in 1..V counts vertices, keep_point in 1..S points: integers, no float rounding
 *                  decides a count.  keep == the count: the direction is untrimmed.  Fewer keys than keep: all of them are kept.
 *   threshold      the highest kept key: a query is kept iff its key <= the threshold.  The one fact the selection produces.
 *   one iteration  the one above with step 3's pair set restricted to the kept pairs: a dropped query adds 0 in place of each of
 *                  its 19 sums (d^2 among them: it is not in the cost either), in the same blocks of 64 queries, the same wave
 *                  butterfly and the same block order.  The weights stay w_vert / V and w_point / S: denominators do not move
 *                  with a count, so the combination, the solve, the rank test and kept_rotation are unchanged.
 *   cost, score, history, best   as above, over the kept pairs.  keep is the same for every start: scores stay comparable.
 *   determinism    as above: no float atomics, every float sum in a fixed order (the selection counts keys with integer counters in
 *                  LDS, whose result does not depend on order).  The same call gives the same bits, I iterations give the bits of
 *                  I chained one-iteration calls.
 *   off            trim == NULL, or every direction of positive weight has keep == its count: exactly smalfit_rigid_align, launch
 *                  for launch and bit for bit; vert_kept / point_kept, where given, are set to 1 (of the directions that are on)
 *                  and trim_d2 to 0: nothing is computed for them.
 * A keep given for a direction of weight 0 is accepted and ignored.  A refused block launches nothing and writes nothing.
 * The FIRST trimmed call of a handle ALLOCATES (and so synchronises): 8 bytes per query of every (mesh, start) at the handle's
 * capacities, (max_verts + max_points) 8 max_meshes max_starts bytes, freed with the handle.  Later calls only enqueue.
 * Not here: estimating the overlap fraction (TrICP's search), scale, normal-compatible matching, translation starts (a scan cut
 * along the body's long axis moves the centroid too far: give start_transforms), the scan index, a stage that re-aligns. */
typedef struct smalfit_rigid_trim_args {
  unsigned struct_size;          /* sizeof(smalfit_rigid_trim_args) of the caller's header; checked before any other field */
  int keep_vert;                 /* vertices kept per iteration, 1 .. V (ignored when w_vert == 0) */
  int keep_point;                /* points kept per iteration, 1 .. S (ignored when w_point == 0) */
  unsigned char* vert_kept;      /* optional (N,K,V): 1 where vertex v was kept in the score's round, else 0; left alone when w_vert == 0 */
  unsigned char* point_kept;     /* optional (N,K,S); left alone when w_point == 0 */
  float* trim_d2;                /* optional (N,K,2): the d^2 of the threshold of the score's round, [0] vertices [1] points; 0 for a
                                    skipped direction and for one that kept nothing */
} smalfit_rigid_trim_args;
int smalfit_trimmed_rigid_align(smalfit_rigid_aligner* aligner, void* stream, const smalfit_rigid_align_args* args,
                                const smalfit_rigid_trim_args* trim);

/* ---- scan sequences: one shape per clip, temporal smoothness ---------------------------------------------------------------------
 * A depth camera or a multi-view rig delivers a SEQUENCE of partial scans of ONE animal moving.  A single partial scan does not
 * determine the shape; many of the same animal do, when the fitter knows that they are the same animal.  A sequence handle makes
 * the N meshes of a batch a set of CLIPS: within a clip the shape is one shape and consecutive poses are tied by the temporal terms
 * of the 2-D fitter (reference smal_fitter/smal_fitter.py:177-190, get_temporal).  THIS PROJECT'S definitions.
 *   clips          clip_lengths holds G positive integers with sum N.  Clip c is the contiguous run of meshes start_c ..
 *                  start_c + len_c - 1 in batch order, start_0 = 0, start_(c+1) = start_c + len_c.  Batch order within a clip is
 *                  temporal order.  A clip of length 1 is an unrelated mesh: nothing below touches it.
 *   shared shape   share_shape != 0: behind the step's betas gradient rows g_n (N x num_betas) every row of clip c is replaced by
 *                  the float32 sum of the clip's rows, taken in ascending n: the first row, then one addition per further row.
 *                  Adam then runs unchanged on all N rows.  Rows of betas and of their two Adam moments that are bit-equal within
 *                  a clip before a step are bit-equal after it, so betas keeps its (N, num_betas) shape for every reader.  This is
 *                  Adam on one shared parameter whose gradient is the sum over its users (the batch-mean chamfer term already
 *                  puts 1/N on every row).  In a step it applies only while lr_betas > 0.
 *   temporal terms three weights; a weight <= 0 skips its term.  x is joint_rot (L = 102 elements per mesh), global_rot (L = 3) or
 *                  trans (L = 3).  For every pair (n, n+1) inside one clip the reference adds mse_loss(x[n], x[n+1]) w; no pair
 *                  spans a clip boundary, and the sum over the pairs is NOT divided by N.  With S the float32 sum over all pairs
 *                  and elements of d d, d = x[n+1][k] - x[n][k], accumulated by fused multiply-adds, a term's loss is
 *                    w (S / L)         one divide by the float L, one multiply
 *                  so a case whose sums are exact in float32 has one result whatever order the reduction runs in.  The device
 *                  sums S by 256 lanes, lane l taking the elements l, l + 256, ... of the flat (N, L) array in ascending order
 *                  (an element of the last mesh of a clip adds nothing), the 64 lanes of a wave by a butterfly (xor 32, 16, ...
 *                  1), the four waves in wave order: the same bits every run.
 *   gradient       with c = (2 w) / L formed once on the host in float32, element k of mesh n receives
 *                    g <- fma(c, (x - prev) + (x - next), g)     prev = x[n-1][k], next = x[n+1][k], x = x[n][k]
 *                  where the first mesh of a clip takes fma(c, x - next, g), the last fma(c, x - prev, g), and a mesh alone in
 *                  its clip keeps g.  In a step the gradient of a term is added before Adam reads it and only where that
 *                  parameter is trained (its lr > 0); the loss is reported either way.
 *   losses         (4): the joint, global and trans terms as defined above (0 for a skipped term), then [3] = (joint + global) +
 *                  trans.  args->losses of the step keeps its five entries WITHOUT these.
 *   step_total     optional (1), a step only: (args->losses[4] + the surface block's weighted term, when that block is on) +
 *                  losses[3]: what the step descends on.
 *   off            a block that couples nothing -- every clip of length 1, or share_shape off (or betas not trained) and every
 *                  weight <= 0 -- launches nothing: `losses` reads 0 and the step is the step without the block, launch for launch
 *                  and bit for bit.
 * One extra launch between the betas assembly and Adam, no atomics, one thread per output element; nothing synchronises.  A
 * refused block launches nothing and leaves every output alone.  The handle owns the device clip tables; it is built for one N
 * and one list of lengths, and may be used with any engine and objective.
 * VERTEX TERMS  (velocity and acceleration on the posed vertices; the vertex block and the two vertex entry points below).  The
 * terms above tie PARAMETERS: in axis-angle two poses a full turn apart look far apart, a change near the root of the kinematic
 * tree looks as small as one at a paw, standing still is the only motion that costs nothing, and deform_verts is not tied at all.
 * These tie the SURFACE.  x[n][v][k] is the float32 array (N, V, 3) the mesh objective composes -- LBS output + trans +
 * deform_verts; in a step args->verts_out when given, else the objective's own buffer.  Clips are the handle's.
 *   velocity       for every pair (n, n+1) inside one clip d = x[n+1] - x[n]; S_vel is the sum of d d over pairs, vertices and
 *                  coordinates.  No pair spans a clip boundary.
 *   acceleration   for every triple whose centre n lies strictly inside its clip a[n] = (x[n-1] - x[n]) + (x[n+1] - x[n]); S_acc
 *                  is the sum of a a.  A clip shorter than 3 adds nothing.
 *   loss           w (S / L) with L = 3 V as a float: the form of the terms above (a mean over the elements, summed over the pairs
 *                  and NOT divided by N).  losses (3): velocity, acceleration, velocity + acceleration.
 *   gradient       c = (2 w) / L per term, formed once on the host.  Element (n, v, k) has
 *                    D = (x - prev) + (x - next)                  the one-neighbour forms at the ends of a clip
 *                    A = (a[n-1] - a[n]) + (a[n+1] - a[n])        a = 0 where the mesh is no centre: five frames at most
 *                    t = fma(c_acc, A, c_vel D)                   an absent part contributes nothing
 *                  t is ADDED to the vertex gradient behind the objective's and the surface term's contributions, the bits are
 *                  (objective + surface) + t, and the float32 sum of t over the vertices of mesh n is added to d trans [n].
 *   destinations   in a step t joins a destination only where that destination feeds a trained parameter: the planar copy the
 *                  LBS adjoint reads while pose or betas are trained, the interleaved gradient while deform_verts is, d trans
 *                  while trans is.  The loss is reported either way.
 *   reductions     no atomics.  One thread owns vertex (n, v) and its three coordinates; mesh n owns the pair (n, n+1), a centre
 *                  owns its triple.  A block of 256 threads adds its lanes by the butterfly (xor 32 .. 1) and its four waves in
 *                  wave order; the partials [N][blocks] of S_vel, S_acc and the three columns of d trans are added by one block
 *                  in ascending mesh, then ascending block order: the same bits every run.
 *   step_total     optional (1), a step only: ((args->losses[4] + the surface block's weighted term, when that block is on) +
 *                  losses[3] of the parameter terms) + losses[2] of these.  The sequence block's own step_total keeps its meaning.
 *   off            both weights <= 0, or no clip long enough for an enabled term (2 for velocity, 3 for acceleration): nothing is
 *                  launched, `losses` is cleared by a 12-byte fill and the step is the sequence step, launch for launch and bit
 *                  for bit (the stand-alone call then fills the gradients it was given with zeros).
 * Two launches between the surface term and the LBS adjoint.  The handle owns the partials, allocated by the first call that needs
 * them and regrown only when V grows.
 * Not here: sharing deform_verts (it is added after posing), robust forms of the vertex terms, weights per vertex or per body
 * part, propagating a fitted frame to the next as its start, clips that are not contiguous in the batch, sequences sharded
 * across GPUs. */
typedef struct smalfit_scan_sequence smalfit_scan_sequence;
typedef struct smalfit_sequence_args {
  int share_shape;               /* != 0: one betas gradient per clip, see above */
  float w_temp_joint;            /* weight of the term on joint_rot; <= 0: skipped; must be finite */
  float w_temp_global;           /* ... on global_rot */
  float w_temp_trans;            /* ... on trans */
  float* losses;                 /* (4, device): joint, global, trans, their sum */
  float* step_total;             /* optional (1, device), a step only */
} smalfit_sequence_args;
/* clip_lengths: HOST, num_clips positive integers with sum num_meshes */
int smalfit_scan_sequence_create(int num_meshes, int num_clips, const int* clip_lengths, smalfit_scan_sequence** out);
void smalfit_scan_sequence_destroy(smalfit_scan_sequence* sequence);
/* the coupling alone, on the caller's gradients of the handle's N meshes (the unfused path).  global_rot (N,3), joint_rot (N,34,3)
 * and trans (N,3) are read, each needed only while its weight is > 0.  g_betas (N,num_betas), g_theta (N,105: columns 0..2 global_rot,
 * 3..104 joint_rot) and g_trans (N,3) are updated in place; any of them may be NULL, and its gradient is then not formed (share_shape
 * applies when g_betas is given; num_betas is read only then).  step_total must be NULL. */
int smalfit_scan_sequence_couple(smalfit_scan_sequence* sequence, void* stream, const smalfit_sequence_args* args, int num_betas,
                                 const float* global_rot, const float* joint_rot, const float* trans, float* g_betas,
                                 float* g_theta, float* g_trans);
/* smalfit_fit3d_step_robust with the sequence block; any of the four opt-in blocks may be NULL as there.  args->num_meshes must be
 * the handle's N. */
int smalfit_scan_sequence_step(smalfit_scan_sequence* sequence, smalfit_engine* engine, smalfit_mesh_objective* objective,
                               smalfit_mesh_targets* targets, void* stream, const smalfit_fit3d_args* args,
                               const smalfit_surface_term_args* surface, const smalfit_surface_gate_args* surface_gate,
                               const smalfit_chamfer_gate_args* chamfer_gate, const smalfit_robust_args* robust,
                               const smalfit_sequence_args* sequence_args);

typedef struct smalfit_sequence_vertex_args {
  float w_temp_vert_vel;         /* weight of the velocity term on the posed vertices; <= 0: skipped; must be finite */
  float w_temp_vert_acc;         /* ... of the acceleration term */
  float* losses;                 /* (3, device): velocity, acceleration, their sum */
  float* step_total;             /* optional (1, device), a step only */
} smalfit_sequence_vertex_args;
/* the vertex terms alone at the caller's vertices of the handle's N meshes (the unfused path).  verts (N,num_verts,3) is read;
 * dverts (N,num_verts,3) and dtrans (N,3) are WRITTEN (t and its sum over a mesh's vertices), either may be NULL.  step_total must
 * be NULL. */
int smalfit_scan_sequence_vertex_term(smalfit_scan_sequence* sequence, void* stream, const smalfit_sequence_vertex_args* args,
                                      int num_verts, const float* verts, float* dverts, float* dtrans);
/* smalfit_scan_sequence_step with the vertex block behind the sequence block; both are required (a sequence block with share_shape
 * 0 and every weight 0 couples nothing). */
int smalfit_scan_sequence_vertex_step(smalfit_scan_sequence* sequence, smalfit_engine* engine, smalfit_mesh_objective* objective,
                                      smalfit_mesh_targets* targets, void* stream, const smalfit_fit3d_args* args,
                                      const smalfit_surface_term_args* surface, const smalfit_surface_gate_args* surface_gate,
                                      const smalfit_chamfer_gate_args* chamfer_gate, const smalfit_robust_args* robust,
                                      const smalfit_sequence_args* sequence_args, const smalfit_sequence_vertex_args* vertex_args);

/* ---- torch.optim.Adam.step -----------------------------------------------------------------------
 * replaces: torch.optim.Adam(lr, betas=(0.5, 0.999)).step()  reference smal_fitter/optimize_to_joints.py:96,137
 * t = 1-based step count; eps outside the bias-corrected sqrt, as torch does */
int smalfit_adam_step(void* stream, int count, float* param, const float* grad, float* exp_avg,
                      float* exp_avg_sq, float lr, float beta1, float beta2, float eps, int t);

#ifdef __cplusplus
}
#endif
#endif /* SMALFIT_H_ */

/*
 * eigentraj.h -- C ABI of libetamd.so, the MI355X (gfx950) implementation of the
 * EigenTrajectory SVD-descriptor hot path.
 *
 * The reference (InhwanBae/EigenTrajectory) is pure Python/PyTorch and has no FFI
 * of its own; the entry points below are what a binding for
 * this path has to cover, one per reference call site:
 *
 *   et_norm_project            EigenTrajectory/descriptor.py:144-160 (projection)
 *                              + normalizer.py:17-51, fused with the moving/static
 *                              routing of EigenTrajectory/model.py:73-90
 *   et_anchor_reconstruct_fwd  EigenTrajectory/anchor.py:76-88 + descriptor.py:162-176
 *                              + normalizer.py:53-62, routed like model.py:98-105
 *   et_anchor_reconstruct_bwd  autograd of the above w.r.t. C_pred (training)
 *   et_fit_gram, et_eigh_topk  descriptor.py:91-114 truncated_SVD via the 2T x 2T Gram
 *                              matrix (parameter_initialization, descriptor.py:116-142)
 *   et_kmeans_*                EigenTrajectory/kmeans.py:59-272 (BatchKMeans); used for
 *                              anchor generation (anchor.py:54-74)
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *  - tensors are contiguous fp32; obs (N,T_obs,2), pred (N,T_pred,2) row-major "NTC";
 *    coefficients are k-major: C (k,N) and C (k,N,S); labels are int64;
 *  - the caller owns every buffer; the library never allocates device memory.
 *    Scratch is passed in as a workspace whose size comes from *_workspace_bytes().  The only memory the library
 *    keeps is host-side and private: per host thread and device a 4-slot pinned staging ring (4 x 96 B + a 64-byte
 *    progress mailbox the single-GPU Lloyd kernel writes into) + 4 events
 *    for the non-blocking convergence polling of the Lloyd loops (csrc/et_hostring.h), and the timing events of
 *    et_kmeans_fit when timing is requested -- created on first use, released when that host thread ends;
 *  - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work and
 *    never synchronise unless documented;
 *  - return value: ET_OK or an ET_ERR_* code; no exceptions cross this boundary;
 *    N == 0 is valid and a no-op; NaN/Inf in the data propagate like in the reference
 *    (normalizer.py:28-29) and are not errors, except in k-means (see below).
 *
 * mode (which descriptor a row uses; the reference keeps two ETDescriptor objects,
 * model.py:29-30):
 *   ET_MODE_STATIC 0  every row: norm_sca=False descriptor (U_*_s, A_s)
 *   ET_MODE_MOVING 1  every row: norm_sca=True  descriptor (U_*_m, A_m)
 *   ET_MODE_SPLIT  2  per row: moving iff ||(obs[-1]-obs[-3])/2|| > static_dist (model.py:46,73)
 *   ET_MODE_IDENTITY 3 rows are used as they are (already normalised input / normalised output)
 */
#ifndef EIGENTRAJ_H
#define EIGENTRAJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ET_ABI_VERSION 3  /* 2: et_kmeans_timing grew `iterations` (32 bytes); 3: et_set_option replaces the ET_* environment switches */

#define ET_OK 0
#define ET_ERR_INVALID_ARG 1  /* bad shape / null pointer / misaligned buffer */
#define ET_ERR_HIP 2          /* a HIP runtime call or launch failed */
#define ET_ERR_UNSUPPORTED 3  /* dimensions outside the compiled range */
#define ET_ERR_WORKSPACE 4    /* workspace too small */
#define ET_ERR_BAD_DATA 5     /* k-means input contains NaN/Inf */
#define ET_ERR_RCCL 6         /* RCCL could not be loaded, or a collective / communicator call failed */

#define ET_MODE_STATIC 0
#define ET_MODE_MOVING 1
#define ET_MODE_SPLIT 2
#define ET_MODE_IDENTITY 3 /* no normalisation at all: bare to_ET_space / to_Euclidean_space
                              (descriptor.py:59-89) with the U_*_s / A_s operands */

#define ET_MAX_T 32  /* max T_obs, T_pred (2T <= 64 rows for the one-wavefront eigensolver) */
#define ET_MAX_K 32  /* max descriptor rank k */
#define ET_KMEANS_MAX_D 32
#define ET_KMEANS_MAX_CLUSTERS 255

typedef void *et_stream_t;
typedef void *et_comm_t; /* an ncclComm_t (RCCL); NULL = a single shard, no collective is enqueued */

int et_abi_version(void);
const char *et_status_string(int status);
/* name of the GPU arch the kernels were compiled for ("gfx950") */
const char *et_compiled_arch(void);

/* ---- tuning switches -----------------------------------------------------------------------------
 * The data path keeps no state between calls and reads nothing from the environment.  The ONE piece of process-wide
 * mutable configuration is this table of measurement aids / test levers (csrc/et_options.hip): every setting selects
 * between forms that are tested to give the same bits, the defaults are the shipped configuration, and a switch is read
 * once at the start of the call it affects (set it before the call, from one thread).  Keys (value as text):
 *   kmeans_packed_min      >= 1024: shards with at least this many points iterate on the packed f16 copy (default 131072 = 2^17)
 *   kmeans_packed          0: trace-less fits keep the fp32 filter body              (default 1)
 *   kmeans_pack_fused      0: the packed copy is written by a pass of its own         (default 1: inside iteration 0)
 *   kmeans_argmax          f: matrix-core filter + exact certification (default) | v: the exact scan only
 *   kmeans_init_tiles      0: farthest-first steps look at every point                (default 1: 256-point tile summaries)
 *   kmeans_filter_threads  256..1024, multiple of 64: workgroup size of the Lloyd kernels (default 0: chosen per shard)
 *   kmeans_chain_copies    1 / 2 / 4 / 8 copies of the per-iteration delta table in a single-GPU fit's one-launch-per-iteration loop (default 2;
 *                          a sharded fit always uses one: its wire format)
 *   kmeans_loop_grid       > 0: at most this many workgroups for the one-launch-per-iteration Lloyd kernel (default 0)
 *   kmeans_loop            a: auto (default) | c: one launch per iteration | p: one persistent launch per fit
 *   reforder_filter_min_lp 4..9: the reference-order Lloyd kernel certifies labels with the matrix-core filter from this cascade level
 *                          power on (L = 2^lp; 4: always, 5: N > 4.2e6, 9: never = default -- built and tested equal, but at 1e7 points
 *                          the launch is bound by its vector instructions either way and the filter's registers halve the
 *                          wavefronts per CU: 138 against 119 us per iteration)
 *   reforder_init_skip_min points (default 2^21): from this shard size on the reference-order farthest-first tests a point's running
 *                          similarity and nearest centroid (5 bytes) before it reads its coordinates (28); same picks
 *   reforder_single_update 1 (default): reference-order fits of at most 8 level-2 blocks update in one 1024-thread workgroup | 0: grid form
 *   metrics_form           a: auto (default) | t: vector-ALU tile kernel for every S | f: fp32 matrix instructions only
 * et_set_option returns ET_ERR_INVALID_ARG for an unknown key or a value the key does not take; et_get_option writes the
 * current value as text.  (The Python binding forwards environment variables ET_OPT_<KEY> once, at load.) */
int et_set_option(const char *key, const char *value);
int et_get_option(const char *key, char *value, size_t value_bytes);

/* ---- TrajNorm (EigenTrajectory/normalizer.py) -------------------------------------------
 * et_norm_params   normalizer.py:17-29: ori (N,1,2), rot (N,2,2) = [[c,-s],[s,c]], sca (N,1,1)
 *                  = 2/||obs[-1]-obs[-3]||; any output may be NULL (flag off).
 * et_normalize     normalizer.py:42-51: ((traj - ori) @ rot) * sca, each step skipped when its
 *                  pointer is NULL.  traj/out (N,T,2); in-place allowed.
 * et_denormalize   normalizer.py:53-62: (traj / sca) @ rot^T + ori. */
int et_norm_params(const float *obs, int64_t N, int T, float *ori, float *rot, float *sca, et_stream_t stream);
/* the same tensors from the compact state nrm (4,N) = ox, oy, dx, dy cached by et_norm_project */
int et_norm_params_from_nrm(const float *nrm, int64_t N, float *ori, float *rot, float *sca, et_stream_t stream);
int et_normalize(const float *traj, int64_t N, int T, const float *ori, const float *rot, const float *sca,
                 float *out, et_stream_t stream);
int et_denormalize(const float *traj, int64_t N, int T, const float *ori, const float *rot, const float *sca,
                   float *out, et_stream_t stream);

/* ---- projection -------------------------------------------------------------------
 * C_obs[j][n]  = sum_f U_obs[f][j]  * normalize(obs[n])[f]      (k,N)
 * C_pred[j][n] = sum_f U_pred[f][j] * normalize(pred[n])[f]     (k,N), if pred != NULL
 * nrm (4,N)    = ox, oy, dx, dy with (ox,oy)=obs[n,-1], (dx,dy)=obs[n,-1]-obs[n,-3]: the
 *                state TrajNorm caches between projection and reconstruction
 *                (normalizer.py:15,20-28); rows 0-1 are model.py:86-87's obs_ori.
 * flag (N)     = 1 for rows routed to the moving descriptor.
 * U_* are (2T,k) row-major like the reference's nn.Parameter (descriptor.py:26-27);
 * the pair a mode does not use may be NULL.  C_pred, nrm, flag may be NULL. */
int et_norm_project(const float *obs, const float *pred, int64_t N, int T_obs, int T_pred, int k,
                    const float *U_obs_m, const float *U_pred_m, const float *U_obs_s, const float *U_pred_s,
                    int mode, float static_dist,
                    float *C_obs, float *C_pred, float *nrm, uint8_t *flag, et_stream_t stream);
/* ... with one more optional output, pose (5,N) = ox, oy, c sca, s sca, +-1/sca: the normaliser of a row in the form the
 * fused error metric consumes (et_anchor_reconstruct_metrics_pose) -- origin, the heading rotation (normalizer.py:24-26)
 * already multiplied by the scale (:28), and 1 / scale with the row's moving (sign bit set) / static decision
 * (model.py:46,73).  20 B per row on top of the projection's 224; pose == NULL is et_norm_project. */
int et_norm_project_pose(const float *obs, const float *pred, int64_t N, int T_obs, int T_pred, int k,
                         const float *U_obs_m, const float *U_pred_m, const float *U_obs_s, const float *U_pred_s,
                         int mode, float static_dist,
                         float *C_obs, float *C_pred, float *nrm, uint8_t *flag, float *pose, et_stream_t stream);

/* Scene form of the projection (one scene batch of model.py:73-90, obs only, N <= ET_SCENE_MAX_N): ONE single-workgroup
 * launch that also produces obs_ori (2,N) = last observed positions minus their mean over the scene (model.py:86-89) --
 * the reference's real workload is N <= 57 pedestrians per forward, i.e. launch-bound.  flag may be NULL. */
#define ET_SCENE_MAX_N 16384
int et_scene_project(const float *obs, int64_t N, int T_obs, int k, const float *U_obs_m, const float *U_obs_s,
                     int mode, float static_dist, float *C_obs, float *nrm, float *obs_ori, uint8_t *flag,
                     et_stream_t stream);

/* ---- training form of a wrapper call on one scene (model.py:58-125 with pred_traj; utils/trainer.py:126-152) ----------
 * N <= ET_SCENE_MAX_N, single-workgroup launches (the work is microseconds; what costs is launches and framework
 * operators).  mode: ET_MODE_STATIC / MOVING / SPLIT.
 *   et_scene_project_train  et_scene_project + C_gt (k,N): the ground truth `pred` (N,T_pred,2) projected with the
 *                           observation's normaliser and its row's U_pred (descriptor.py:144-160, model.py:73-83).
 *   et_wrapper_losses_fwd   recon (S,N,T_pred,2) as et_anchor_reconstruct_fwd, and in the same launch
 *                             losses[0] loss_eigentraj     = mean_n min_s ||A[:,s] + C[:,n,s] - C_gt[:,n]||   (model.py:119)
 *                             losses[1] loss_euclidean_ade = mean_n min_s mean_t ||recon[s,n,t] - gt[n,t]||   (model.py:120-121)
 *                             losses[2] loss_euclidean_fde = mean_n min_s ||recon[s,n,-1] - gt[n,-1]||        (model.py:122-123)
 *                           best (3,N): the per-pedestrian minima, arg (3,N) int32: the sample attaining each.
 *   et_wrapper_losses_bwd   dC (k,N,S) = sum_i g_i * d losses[i] / d C (g_*: the upstream gradient of each loss, a device
 *                           scalar, NULL = not differentiated); each term reaches only its arg-min sample, on an exact
 *                           tie the first one (the gradient of the reference's .min(dim)[0]).  A distance that is exactly
 *                           0 contributes 0; one that is NaN makes that sample's dC NaN, as the reference's autograd does
 *                           (also under a non-NULL g_* whose value is 0: 0 * NaN; only a NULL g_* leaves its term out).
 *                           Needs the U_pred of every descriptor the mode uses, like et_wrapper_losses_fwd. */
int et_scene_project_train(const float *obs, const float *pred, int64_t N, int T_obs, int T_pred, int k,
                           const float *U_obs_m, const float *U_obs_s, const float *U_pred_m, const float *U_pred_s,
                           int mode, float static_dist, float *C_obs, float *nrm, float *obs_ori, float *C_gt,
                           uint8_t *flag, et_stream_t stream);
int et_wrapper_losses_fwd(const float *C, int64_t N, int S, int k, int T_pred, const float *nrm, const float *A_m,
                          const float *A_s, const float *U_pred_m, const float *U_pred_s, int mode, float static_dist,
                          const float *C_gt, const float *gt, float *recon, float *best, int32_t *arg, float *losses,
                          et_stream_t stream);
int et_wrapper_losses_bwd(const float *g_eigentraj, const float *g_ade, const float *g_fde, const float *C, int64_t N, int S,
                          int k, int T_pred, const float *nrm,
                          const float *A_m, const float *A_s, const float *U_pred_m, const float *U_pred_s, int mode,
                          float static_dist, const float *C_gt, const float *gt, const float *recon, const int32_t *arg,
                          float *dC, et_stream_t stream);

/* ---- anchor refinement + reconstruction -------------------------------------------
 * out[s][n] = denormalize( reshape( U_pred . (C[:,n,s] + A[:,s]) ) )      (S,N,T_pred,2)
 * C (k,N,S); A_m/A_s (k,S) or NULL (no anchor add); normaliser state comes from `nrm`
 * (4,N) as written by et_norm_project, or, when nrm == NULL, is recomputed from obs. */
int et_anchor_reconstruct_fwd(const float *C, int64_t N, int S, int k, int T_obs, int T_pred,
                              const float *obs, const float *nrm,
                              const float *A_m, const float *A_s, const float *U_pred_m, const float *U_pred_s,
                              int mode, float static_dist, float *out, et_stream_t stream);

/* Fused evaluation form (no counterpart in the reference, which materialises recon_traj and calls
 * utils/metrics.py:73-102): best-of-S displacement errors against gt (N,T_pred,2) without writing the
 * trajectories:  ade[n] = min_s mean_t ||out[s][n][t] - gt[n][t]||,  fde[n] = min_s ||out[s][n][T-1] - gt[n][T-1]||.
 * A NaN anywhere in a trajectory's samples makes its two results NaN (torch.min's propagation).  For T_pred = 12, k = 6,
 * 12 <= S <= 64 the contraction runs on the matrix cores from two-term f16 splits of both operands: results within 1e-6
 * (relative to the largest) of et_anchor_reconstruct_fwd + the metrics; operands beyond f16's range take fp32 instructions. */
int et_anchor_reconstruct_metrics(const float *C, int64_t N, int S, int k, int T_obs, int T_pred,
                                  const float *obs, const float *nrm,
                                  const float *A_m, const float *A_s, const float *U_pred_m, const float *U_pred_s,
                                  int mode, float static_dist, const float *gt, float *ade, float *fde,
                                  et_stream_t stream);
/* ... with the normaliser from `pose` (5,N) as written by et_norm_project_pose under the same mode and static_dist: the
 * matrix-core kernel (T_pred = 12, k = 6, 12 <= S <= 64) then re-derives nothing per pass (no square root, reciprocal or
 * selects for the rotation and the scale: ~11 % of its vector instructions).  Shapes that kernel does not take fall back to
 * nrm / obs exactly as et_anchor_reconstruct_metrics (so pass them too unless the shape is known); pose == NULL is that call. */
int et_anchor_reconstruct_metrics_pose(const float *C, int64_t N, int S, int k, int T_obs, int T_pred,
                                       const float *obs, const float *nrm, const float *pose,
                                       const float *A_m, const float *A_s, const float *U_pred_m, const float *U_pred_s,
                                       int mode, float static_dist, const float *gt, float *ade, float *fde,
                                       et_stream_t stream);

/* ---- the reference's test metrics (utils/metrics.py:30-155; utils/trainer.py:173-195) --------------------------------
 * Per pedestrian of pred (S,N,T,2) against gt (N,T,2), 2 <= T <= ET_MAX_T:
 *   ade, fde  best-of-S displacement errors (as et_anchor_reconstruct_metrics)
 *   best      int32 arg-min over samples of the final displacement (first index on ties, the first NaN wins)
 *   tcc       temporal correlation coefficient of the best sample (:105-130): per coordinate the Pearson correlation over
 *             the T steps (covariance factor 1/(T-1)), clamped to [-1, 1], NaN -> 0, mean of the two coordinates
 *   col       collision rate in percent (:133-155): 100 * (samples in which the pedestrian comes closer than 0.2 to another
 *             pedestrian of its scene at one of the first min(14, 1 + 4 (T-1)) instants of the path densified 4x) / S
 * Scenes: scene_offsets (n_scenes + 1) int32 device array, 0 = off[0] <= ... <= off[n_scenes] = N (N <= INT32_MAX);
 * NULL = one scene of N rows (the reference called on the whole tensor).  Only pairs within a scene are compared; a whole
 * split is one launch.  Any output may be NULL; col == NULL skips the pair pass.  pred, gt: 8-byte aligned. */
int et_traj_metrics(const float *pred, int64_t N, int S, int T, const float *gt,
                    const int32_t *scene_offsets, int n_scenes,
                    float *ade, float *fde, float *tcc, float *col, int32_t *best, et_stream_t stream);
/* The same from the coefficients (fused: nothing of size (S,N,T_pred,2) is written): every (sample, pedestrian) is
 * reconstructed in registers with et_anchor_reconstruct_fwd's arithmetic, so the results equal et_traj_metrics applied to
 * that call's output.  The normaliser comes from nrm or obs when given, else from pose (5,N) of et_norm_project_pose (its
 * rotation is then recovered as (c sca) / sca: within an ulp or two of the nrm form for moving rows). */
int et_anchor_reconstruct_metrics_scenes(const float *C, int64_t N, int S, int k, int T_obs, int T_pred,
                                         const float *obs, const float *nrm, const float *pose,
                                         const float *A_m, const float *A_s, const float *U_pred_m, const float *U_pred_s,
                                         int mode, float static_dist, const float *gt,
                                         const int32_t *scene_offsets, int n_scenes,
                                         float *ade, float *fde, float *tcc, float *col, int32_t *best,
                                         et_stream_t stream);

/* dC[j][n][s] = sum_f U_pred[f][j] * ((dtraj[s][n] @ R_n) / sca_n)[f]          (k,N,S) */
int et_anchor_reconstruct_bwd(const float *dtraj, int64_t N, int S, int k, int T_obs, int T_pred,
                              const float *obs, const float *nrm,
                              const float *U_pred_m, const float *U_pred_s,
                              int mode, float static_dist, float *dC, et_stream_t stream);

/* ---- curve-fitting baselines (CurveModel/curve_fitting.py; script/descriptor_evaluation.py:38-85) -----------------------
 * A batch of n_fits independent fits, one launch per pass.  Fit f is a row of fits_host (HOST array, n_fits x 6 int64):
 *   (N, T, ncp, traj_off, basis_off, cp_off)   1 <= N <= INT32_MAX, 2 <= T <= 32, 2 <= ncp <= 8
 * its trajectories are traj[traj_off ..] (N,T,2) (already normalised), its basis basis[basis_off ..] (T,ncp), its recon goes
 * to recon[traj_off ..] (N,T,2) and its control points to cp[cp_off ..] (N,ncp,2) (offsets in floats).  Per pedestrian:
 *   cp[0] = traj[0], cp[i] = cp[i-1] + (traj[T-1] - traj[0]) / (ncp-1);  recon[t] = sum_i basis[t][i] cp[i]
 *   loss = mean over the fit's N T points of ||recon - traj||_2, minimised by Adam(lr, (beta1, beta2), eps) for n_steps
 * (fp32, torch.optim.Adam's single-tensor order, the norm's gradient 0 at a zero residual; as in the reference, which never
 * zeroes .grad, Adam is fed the running sum of the step gradients).  The loss of a step is summed
 * in fixed point (per pedestrian the fp64 sum of its T norms rounded to a multiple of 2^-28, clamped to 2^26), so it and
 * the best step do not depend on the launch geometry.  Outputs:
 *   recon      the recon of the fit's best step = the first step of minimum loss (the parameters BEFORE that step's
 *              update: step 0 is the initial guess)
 *   cp         (may be NULL) the control points of that step
 *   loss       (may be NULL) n_fits x n_steps fp64: the per-step mean loss (fixed-point sum * 2^-28 / (N T))
 *   best_step  (may be NULL) n_fits int32
 * 1 <= n_steps <= INT32_MAX; 0 < lr; 0 <= beta1, beta2 < 1; 0 <= eps.  The sum of a fit's T N norms must stay below 2^35
 * (far beyond trajectories in metres).  Pass 2 replays every pedestrian to its best step, so a call costs up to 2 n_steps
 * steps.  Bad shapes / arguments: ET_ERR_INVALID_ARG before any work is enqueued. */
#define ET_CURVE_MAX_FITS 64
size_t et_curve_fit_batch_workspace_bytes(int n_fits, int64_t n_steps); /* 0: arguments not taken */
int et_curve_fit_batch(const float *traj, const float *basis, const int64_t *fits_host, int n_fits, int64_t n_steps,
                       double lr, double beta1, double beta2, double eps, float *recon, float *cp, double *loss,
                       int32_t *best_step, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- t-SNE of descriptor coefficients (script/plot_coeff_tsne.py: sklearn.manifold.TSNE, Barnes-Hut) ------------------
 * sklearn's pipeline with exact repulsion, n_components = 2.  X (N,d) fp32 row-major, 2 <= N, 1 <= d <= 32; Y (N,2) fp32.
 * et_tsne_neighbors: k = min(N-1, floor(3 perplexity + 1)) (0: arguments not taken).
 * et_tsne_affinities: the k nearest other rows of every row by (squared distance, index) -- the squared distance summed
 *   in fp64 from fp32 differences, rounded through sqrt and squared again to fp32 -- written in column order:
 *   knn_idx / knn_dist (N,k); p_cond (N,k) fp64 the perplexity search's conditional P; the symmetric
 *   P = (P_cond + P_cond^T) / total as canonical CSR: indptr (N+1), indices / P (capacity 2 N k; nnz = indptr[N]);
 *   p_total (device, may be NULL) the total.  Synchronises the stream once.  Non-finite X or N < 2: ET_ERR_BAD_DATA.
 * et_tsne_kl_grad: grad (N,2) = 4 (sum_j p_ij q_ij (y_i - y_j) - sum_{j ~ i} q_ij^2 (y_i - y_j) / Z) with
 *   q_ij = 1 / (1 + |y_i - y_j|^2), Z = max(sum_{i ~ j} q_ij, DBL_EPSILON), P fp32 CSR; j ~ i: y_j differs from y_i in
 *   a coordinate (as sklearn's quadtree as compiled, which skips exactly coincident points; j = i included; all points
 *   coincident: grad = 0); kl (device, may be NULL) the KL divergence over the CSR entries.  Bit-identical from run to run (the summation order depends on N only).  The
 *   workspace holds ceil(N / 1024) x N x 8 bytes of partial sums (grows as N^2; 7 MB at N = 3e4, 78 MB at 1e5);
 *   N <= 65 535 x 1 024.  Synchronises the stream once.  Non-finite Y: ET_ERR_BAD_DATA.
 * et_tsne_update: one step of sklearn's _gradient_descent on n coordinates in place (gains, update fp64, p; grad is
 *   scaled by the new gains).
 * et_tsne_optimize: TSNE._tsne from Y (in/out): 250 iterations with P x early_exaggeration and momentum 0.5, then up to
 *   max_iter with momentum 0.8; KL and the gradient norm every 50 iterations, sklearn's stop rules.  P is the fp64 CSR
 *   of et_tsne_affinities.  kl_out / n_iter_out (host) = sklearn's kl_divergence_ / n_iter_ (at max_iter = 250, as
 *   sklearn: the second phase runs no iteration and returns 250 and DBL_MAX; max_iter < 250, not an sklearn setting,
 *   ends the first phase early).  Workspace as et_tsne_kl_grad's plus O(N + nnz).  Synchronises the stream twice
 *   (after each phase).  Non-finite Y: ET_ERR_BAD_DATA.
 * et_tsne_pca_init: sklearn's init="pca": the top two eigenvectors of the centred X's covariance (et_eigh_topk), signs by
 *   svd_flip(u_based_decision=False), Y = (X - mean) V / std(Y[:,0]) * 1e-4.  2 <= d <= 32.  Synchronises the
 *   stream once.  Non-finite X: ET_ERR_BAD_DATA. */
int et_tsne_neighbors(int64_t N, double perplexity);
size_t et_tsne_affinities_workspace_bytes(int64_t N, int d, int k); /* 0: arguments not taken */
int et_tsne_affinities(const float *X, int64_t N, int d, double perplexity, int k, int32_t *knn_idx, float *knn_dist,
                       double *p_cond, int32_t *indptr, int32_t *indices, double *P, double *p_total, void *workspace,
                       size_t workspace_bytes, et_stream_t stream);
size_t et_tsne_kl_grad_workspace_bytes(int64_t N);
int et_tsne_kl_grad(const float *Y, int64_t N, const int32_t *indptr, const int32_t *indices, const float *P,
                    float *grad, double *kl, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_tsne_update(float *p, double *update, float *gains, float *grad, int64_t n, double momentum,
                   double learning_rate, et_stream_t stream);
size_t et_tsne_optimize_workspace_bytes(int64_t N, int64_t nnz);
int et_tsne_optimize(float *Y, int64_t N, const int32_t *indptr, const int32_t *indices, const double *P, int64_t nnz,
                     double early_exaggeration, double learning_rate, int max_iter, double *kl_out, int *n_iter_out,
                     void *workspace, size_t workspace_bytes, et_stream_t stream);
size_t et_tsne_pca_init_workspace_bytes(int64_t N, int d);
int et_tsne_pca_init(const float *X, int64_t N, int d, float *Y, void *workspace, size_t workspace_bytes,
                     et_stream_t stream);

/* ---- Social-STGCNN predictor, inference (baseline/stgcnn: bridge.py pre-hook + social_stgcnn.forward + post-hook) ---
 * Eval mode only: every BatchNorm2d uses its running statistics, dropout is off.  The parameters are read in place from
 * the module's own tensors through the pointer table below (fp32, contiguous); the BatchNorm transform
 * (x - running_mean) / sqrt(running_var + bn_eps) * weight + bias is formed inside the kernel.  Field <-> state_dict name
 * (i = st_gcn layer, j = tpcnn index):
 *   st_gcns[i].gcn_w / gcn_b         st_gcns.{i}.gcn.conv.weight (S K, C_in, 1, 1) / .bias (S K)
 *   st_gcns[i].bn1_*                 st_gcns.{i}.tcn.0.weight / bias / running_mean / running_var (S)
 *   st_gcns[i].prelu1                st_gcns.{i}.tcn.1.weight (1)
 *   st_gcns[i].tcn_w / tcn_b         st_gcns.{i}.tcn.2.weight (S, S, 3, 1) / .bias (S)
 *   st_gcns[i].bn2_*                 st_gcns.{i}.tcn.3.weight / bias / running_mean / running_var (S)
 *   st_gcns[i].res_w / res_b         st_gcns.{i}.residual.0.weight (S, C_in, 1, 1) / .bias (S); NULL when C_in == S
 *   st_gcns[i].res_bn_*              st_gcns.{i}.residual.1.weight / bias / running_mean / running_var (S)
 *   st_gcns[i].prelu                 st_gcns.{i}.prelu.weight (1)
 *   tpcnn_w[j] / tpcnn_b[j]          tpcnns.{j}.weight (k, j ? k : K, 3, 3) / .bias (k)
 *   prelus[j]                        prelus.{j}.weight (1)
 *   out_w / out_b                    tpcnn_ouput.weight (k, k, 3, 3) / .bias (k)
 * with K = seq_len, k = pred_seq_len, S = output_feat.  tpcnns[j] / prelus[j] are read for j < max(1, n_txpcnn - 1)
 * only (the reference's loop leaves the last pair unused); the others may be NULL.
 * Supported: input_feat = 1, kernel_size = 3, seq_len = pred_seq_len + 2, 1 <= pred_seq_len <= ET_MAX_K,
 * 1 <= output_feat <= 64, 1 <= n_stgcnn, n_txpcnn <= ET_STGCNN_MAX_LAYERS; anything else: ET_ERR_UNSUPPORTED.
 *
 * The adjacency of "time" row t of v (bridge.py:4-21): a_inv = 1 / |v[t,i] - v[t,j]| (0 where the distance is 0),
 * a_hat = a_inv + I, D = rowsum(a_hat)^-1/2, L = I - D a_hat D.
 *   et_stgcnn_forward_graph   one scene as the bridge hands it over: v (1,1,K,N), a = L (K,N,N) -> out (1,S,k,N), the
 *                             network's raw output.  N <= ET_SCENE_MAX_N.
 *   et_stgcnn_forward_scenes  a whole split: C_obs (k,N), nrm (4,N) of et_norm_project (rows 0-1: last observed position);
 *                             per scene v = [C_obs; nrm[0:2] - their mean over the scene] (model.py:86-90), L formed on
 *                             the fly from v, -> C_pred_refine (k,N,S) (the post-hook's layout).  scene_offsets as
 *                             et_traj_metrics (NULL = one scene of N rows); n_scenes = 0 takes N = 0 only.  One launch.
 * Workspace: a scene whose activations fit a workgroup's LDS arena (at S = 20, k = 6: up to 33 pedestrians) needs none;
 * larger ones use workspace rows [off[s], off[s+1]) of et_stgcnn_workspace_bytes(p, N, max_scene_n) bytes (0 when a
 * scene of max_scene_n pedestrians fits the arena).  A scene larger than ET_SCENE_MAX_N, or one that fits neither, is
 * not computed: its outputs are NaN.  No host synchronisation, no allocation: the calls can be captured in a graph. */
#define ET_STGCNN_MAX_LAYERS 8
typedef struct et_stgcnn_layer {
    const float *gcn_w, *gcn_b;
    const float *bn1_w, *bn1_b, *bn1_mean, *bn1_var;
    const float *prelu1;
    const float *tcn_w, *tcn_b;
    const float *bn2_w, *bn2_b, *bn2_mean, *bn2_var;
    const float *res_w, *res_b;
    const float *res_bn_w, *res_bn_b, *res_bn_mean, *res_bn_var;
    const float *prelu;
} et_stgcnn_layer;
typedef struct et_stgcnn_params {
    int n_stgcnn, n_txpcnn, input_feat, output_feat, seq_len, pred_seq_len, kernel_size;
    float bn_eps;
    et_stgcnn_layer st_gcns[ET_STGCNN_MAX_LAYERS];
    const float *tpcnn_w[ET_STGCNN_MAX_LAYERS];
    const float *tpcnn_b[ET_STGCNN_MAX_LAYERS];
    const float *prelus[ET_STGCNN_MAX_LAYERS];
    const float *out_w, *out_b;
} et_stgcnn_params;
size_t et_stgcnn_workspace_bytes(const et_stgcnn_params *params, int64_t N, int64_t max_scene_n);
int et_stgcnn_forward_scenes(const et_stgcnn_params *params, const float *C_obs, const float *nrm, int64_t N,
                             const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, void *workspace,
                             size_t workspace_bytes, et_stream_t stream);
int et_stgcnn_forward_graph(const et_stgcnn_params *params, const float *v, const float *a, int64_t N, float *out,
                            void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- SGCN predictor, inference (baseline/sgcn: bridge.py pre-hook + TrajectoryModel.forward + post-hook) -------------
 * Eval mode, dropout = 0, fp32.  The parameters are read in place from the module's own tensors through the pointer table
 * below (fp32, contiguous).  Field <-> state_dict name (SWA = sparse_weighted_adjacency_matrices, j = layer index):
 *   att[0] / att[1]                  SWA.spatial_attention / SWA.temporal_attention: embedding.weight (64, 1) / .bias,
 *                                    query.weight (64, 64) / .bias, key.weight (64, 64) / .bias
 *   fus_w / fus_b / fus_a            SWA.spa_fusion.conv.0.weight (T, T, 1, 1) / .bias (T), conv.1.weight (1)
 *   asym_s[j] / asym_t[j]            SWA.interaction_mask.{spatial,temporal}_asymmetric_convolutions.{j}: conv1.weight
 *                                    (4, 4, 3, 1), conv2.weight (4, 4, 1, 3) / .bias (4), activation.weight (1)
 *   gcn[0..3]                        stsgcn.spatial_temporal_sparse_gcn.{0,1}, stsgcn.temporal_spatial_sparse_gcn.{0,1}:
 *                                    embedding.weight (16, 1 or 16), activation.weight (1)
 *   fusion_w                         fusion_.weight (4, 4, 1, 1)
 *   tcn_w[j] / tcn_b[j] / tcn_a[j]   tcns.{j}.0.weight (k, j ? k : T, 3, 3) / .bias (k), tcns.{j}.1.weight (1)
 *   out_w / out_b                    output.weight (S, 16) / .bias (S)
 * with T = obs_len, k = pred_len, S = out_dims.  Supported: in_dims = 1, num_heads = 4, embedding_dims = 64, dropout = 0,
 * 1 <= number_asymmetric_conv_layer, n_tcn <= ET_SGCN_MAX_LAYERS, 1 <= pred_len <= ET_MAX_K, obs_len = pred_len + 2,
 * 1 <= out_dims <= 64; anything else: ET_ERR_UNSUPPORTED.  A scene has at most ET_SGCN_MAX_N pedestrians.
 *
 *   et_sgcn_forward_graph   one scene as the bridge hands it over: v (1,T,N,1), identity_s (1 or T, N, N) (id_s_t = its
 *                           first dimension), identity_t (N, 1, 1) or (N, T, T) (id_t_t = 1 or T) -> out (k, N, S).
 *                           The identities are read as given (the bridge's temporal one is all ones, not eye(T)).
 *   et_sgcn_forward_scenes  a whole split: C_obs (k,N), nrm (4,N) of et_norm_project (rows 0-1: last observed position);
 *                           per scene v = [C_obs; nrm[0:2] - their mean over the scene], spatial identity eye(n), temporal
 *                           identity all ones (what the bridge builds) -> C_pred_refine (k,N,S).  scene_offsets as
 *                           et_traj_metrics (NULL = one scene of N rows); n_scenes = 0 takes N = 0 only.  sum_n2 = the sum
 *                           of the scenes' squared sizes (sizes the dense stacks), max_scene_n the largest scene (sizes
 *                           the grid).  A scene that is larger than ET_SGCN_MAX_N or does not fit the stacks is not
 *                           computed: its outputs are NaN.
 * logit_s / logit_t (may be NULL): the values that enter the interaction mask's two sigmoids, per scene (T,4,n,n) and
 * (n,4,T,T), packed scene after scene (scene s at 4 T sum_{s'<s} n_s'^2 and at 4 T T off[s]).
 * Layered form: the dense (T,4,n,n) stacks live in the caller's workspace (two of them, ping-pong); 6 +
 * number_asymmetric_conv_layer launches for any number of scenes, no host synchronisation, no allocation (the calls can be
 * captured in a graph).  Every sum has a fixed order: results are bit-identical from run to run, and a scene's result does
 * not depend on the scenes around it. */
#define ET_SGCN_MAX_LAYERS 8
#define ET_SGCN_MAX_N 512
typedef struct et_sgcn_attention {
    const float *emb_w, *emb_b, *q_w, *q_b, *k_w, *k_b;
} et_sgcn_attention;
typedef struct et_sgcn_asym {
    const float *conv1_w, *conv2_w, *conv2_b, *act;
} et_sgcn_asym;
typedef struct et_sgcn_gcn {
    const float *w, *act;
} et_sgcn_gcn;
typedef struct et_sgcn_params {
    int n_asym, embedding_dims, n_gcn_layers, obs_len, pred_len, n_tcn, in_dims, out_dims, num_heads;
    float dropout;
    et_sgcn_attention att[2];
    const float *fus_w, *fus_b, *fus_a;
    et_sgcn_asym asym_s[ET_SGCN_MAX_LAYERS];
    et_sgcn_asym asym_t[ET_SGCN_MAX_LAYERS];
    et_sgcn_gcn gcn[4];
    const float *fusion_w;
    const float *tcn_w[ET_SGCN_MAX_LAYERS];
    const float *tcn_b[ET_SGCN_MAX_LAYERS];
    const float *tcn_a[ET_SGCN_MAX_LAYERS];
    const float *out_w, *out_b;
} et_sgcn_params;
size_t et_sgcn_workspace_bytes(const et_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes);
int et_sgcn_forward_scenes(const et_sgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                           const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                           float *C_pred_refine, float *logit_s, float *logit_t, void *workspace, size_t workspace_bytes,
                           et_stream_t stream);
int et_sgcn_forward_graph(const et_sgcn_params *params, const float *v, const float *identity_s, int id_s_t,
                          const float *identity_t, int id_t_t, int64_t N, float *out, float *logit_s, float *logit_t,
                          void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- SGCN predictor, training (the family above; dropout = 0 makes the training-mode forward the eval forward) ---------
 * Gradients of what et_sgcn_forward_graph computes with respect to every parameter; no input gradient (the bridge detaches v).
 *   et_sgcn_train_workspace_bytes   the training workspace: the eval workspace's values, n_asym + 1 kept stacks of each
 *                                   kind instead of the two ping-pong ones, the tail's activations, and the backward's
 *                                   gradient stacks (one per kept stack) and partial sums.  0: outside the family, or N <= 0.
 *   et_sgcn_train_forward_graph /   et_sgcn_forward_graph / _scenes with the kept layout: the same kernels, the same
 *   et_sgcn_train_forward_scenes    number of launches, an output that is bit-equal to theirs.  logit_s / logit_t (may be
 *                                   NULL) are copies of the last kept stacks.
 *   et_sgcn_backward_graph /        d_out (k, N, S), the gradient at the forward's output, and the workspace as that forward
 *   et_sgcn_backward_scenes         left it (same parameters, same N, scene_offsets, sum_n2; the graph form also the same
 *                                   identities) -> grads, grads_floats >= et_sgcn_grad_floats floats: every parameter's
 *                                   gradient in state_dict order (att[0], att[1]: embedding.weight, .bias, query.weight,
 *                                   .bias, key.weight, .bias; fus_w, fus_b, fus_a; asym_s[j], then asym_t[j]: conv1.weight,
 *                                   conv2.weight, conv2.bias, activation.weight; gcn[0..3]: embedding.weight,
 *                                   activation.weight; fusion_w; tcns j: weight, bias, PReLU weight; out_w, out_b).
 *                                   number_asymmetric_conv_layer + 8 launches for any number of scenes.
 * A scene that the forward does not compute (larger than ET_SGCN_MAX_N, or one that does not fit the stacks) contributes
 * nothing: its rows of d_out are not read.  key.bias of both attentions gets an exact +0.0: it shifts a softmax row by a
 * constant (autograd leaves rounding noise there).
 * No atomics.  A weight gradient is the sum of per-workgroup partials over chunks of ET_SGCN_BWD_CHUNK pedestrians (the
 * tail), ET_SGCN_BWD_ROWS softmax rows or ET_SGCN_BWD_ITEMS stack positions of one scene: ascending inside a chunk (per
 * lane, then the lanes by a fixed butterfly, then the wavefronts), then the chunks ascending, then the scenes ascending.
 * Results are bit-identical from run to run.  Host-side checks answer ET_ERR_INVALID_ARG / ET_ERR_WORKSPACE /
 * ET_ERR_UNSUPPORTED before any launch. */
#define ET_SGCN_BWD_CHUNK 4
#define ET_SGCN_BWD_ROWS 1024
#define ET_SGCN_BWD_ITEMS 4096
size_t et_sgcn_train_workspace_bytes(const et_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes);
int64_t et_sgcn_grad_floats(const et_sgcn_params *params);
/* where the training workspace keeps what (host only, no launch), in floats from its start: v, rows_s, rows_t, stack_s,
 * its stride, stack_t, its stride, at, f2, f1, ts, tail, its floats per row, d_at (the tail's part), d_f1, d_ts, d_f2, the
 * per-spatial-row record (ZeroSoftmax's denominator and d (A_s f2): 17 floats), g_s, g_t (n_asym + 1 gradient stacks each, the strides of
 * stack_s / stack_t: d stack j stays for a layer-by-layer check), the direct parts of d dense_s and d dense_t, d dense_s,
 * the total.  A scene's block starts at T x its first row (v), 4 T x its packed n^2 offset (stack_s, g_s, dense_s parts) or
 * 4 T T / 64 T x its first row (the rest). */
#define ET_SGCN_TRAIN_LAYOUT_FIELDS 24
int et_sgcn_train_layout(const et_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes, int64_t *offsets, int n_offsets);
int et_sgcn_train_forward_scenes(const et_sgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                 const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                                 float *C_pred_refine, float *logit_s, float *logit_t, void *workspace,
                                 size_t workspace_bytes, et_stream_t stream);
int et_sgcn_train_forward_graph(const et_sgcn_params *params, const float *v, const float *identity_s, int id_s_t,
                                const float *identity_t, int id_t_t, int64_t N, float *out, float *logit_s, float *logit_t,
                                void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_sgcn_backward_scenes(const et_sgcn_params *params, int64_t N, const int32_t *scene_offsets, int n_scenes,
                            int64_t sum_n2, int64_t max_scene_n, const float *d_out, float *grads, int64_t grads_floats,
                            void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_sgcn_backward_graph(const et_sgcn_params *params, const float *identity_s, int id_s_t, const float *identity_t,
                           int id_t_t, int64_t N, const float *d_out, float *grads, int64_t grads_floats, void *workspace,
                           size_t workspace_bytes, et_stream_t stream);

/* ---- Social-STGCNN predictor, training (the inference family above with n_stgcnn = 1; anything else: ET_ERR_UNSUPPORTED;
 * deeper stacks would send a gradient through the Laplacian contraction and are out of scope) -------------------------------
 * The training-mode forward is NOT the eval forward: st_gcns.0.tcn.0, .tcn.3 and .residual.1 (the last only when
 * output_feat != 1; at output_feat = 1 the residual is the identity) normalise with the statistics of the scene -- mean and
 * biased variance per channel over its K n values -- and update their running statistics as torch does:
 * running_mean = (1 - m) running_mean + m mean, running_var = (1 - m) running_var + m var cnt / (cnt - 1), cnt = K n,
 * num_batches_tracked += 1, per scene, the scenes in ascending order (an empty scene is no batch), whether or not a backward
 * call follows.  et_stgcnn_params' running statistics are not read.  et_stgcnn_train carries what training adds: the
 * momentum, the writable running statistics (S floats each) and the three num_batches_tracked (one int64_t each); the
 * res_bn_* three are NULL exactly when output_feat = 1.
 *   et_stgcnn_train_workspace_bytes  the training workspace for N pedestrians in n_scenes scenes (graph form: 1): every
 *                                    intermediate of both passes, the scenes' statistics and gradient partials.  0: outside
 *                                    the family, N <= 0 or n_scenes < 1.
 *   et_stgcnn_train_forward_graph /  arguments as et_stgcnn_forward_graph / _scenes, plus `train`; 2 launches (the scene
 *   et_stgcnn_train_forward_scenes   kernel, one workgroup per scene; the running-statistics kernel) for any N and any
 *                                    number of scenes.
 *   et_stgcnn_backward_graph /       d_out laid out as the forward's output ((1,S,k,N) / (k,N,S)) and the workspace as that
 *   et_stgcnn_backward_scenes        forward left it (same parameters, N, scene_offsets) -> grads, grads_floats >=
 *                                    et_stgcnn_grad_floats floats: every parameter's gradient in state_dict order
 *                                    (st_gcns.0: gcn.conv.weight, .bias, tcn.0.weight, .bias, tcn.1.weight, tcn.2.weight,
 *                                    .bias, tcn.3.weight, .bias, [residual.0.weight, .bias, residual.1.weight, .bias,]
 *                                    prelu.weight; tpcnns.j.weight, .bias for every j; tpcnn_ouput.weight, .bias;
 *                                    prelus.j.weight for every j).  2 launches (the scene kernel; the reduction over the
 *                                    scenes) for any N and any number of scenes.
 * tcn.2.bias and residual.0.bias feed a training-mode BatchNorm directly: their gradient is an exact +0.0 (autograd leaves
 * rounding noise there), and so is that of tpcnns[n_txpcnn-1] / prelus[n_txpcnn-1], which the forward never reads when
 * n_txpcnn >= 2.  No gradient with respect to the input.  No atomics: every per-channel statistic and every gradient element
 * of a scene is one wavefront's sum over the element's positions (lane l adds positions l, l + 64, ... in ascending order,
 * then the lanes by the xor butterfly 32, 16, ..., 1), and the scenes' partials are added in ascending order; results are
 * bit-identical from run to run, and a one-scene scenes call equals the graph call.  A scene of more than ET_SCENE_MAX_N
 * pedestrians is not computed (NaN outputs, no batch, no gradient).  Host-side checks answer ET_ERR_UNSUPPORTED /
 * ET_ERR_INVALID_ARG / ET_ERR_WORKSPACE before any launch.  A single scene occupies one CU. */
typedef struct et_stgcnn_train {
    float momentum;
    float *bn1_mean, *bn1_var;
    float *bn2_mean, *bn2_var;
    float *res_bn_mean, *res_bn_var;
    int64_t *bn1_batches, *bn2_batches, *res_bn_batches;
} et_stgcnn_train;
size_t et_stgcnn_train_workspace_bytes(const et_stgcnn_params *params, int64_t N, int n_scenes);
int64_t et_stgcnn_grad_floats(const et_stgcnn_params *params);
/* where the training workspace keeps what (host only, no launch), in floats.  Per-pedestrian fields first (scene s's block
 * starts at off[s] x [20]; field f of it at + offsets[f] x the scene's n): u (K,n), d (K,n), P (K,K+1,n), g, a1, y, t, r,
 * s, x (S,K,n each: gcn output, tcn.1's input and output, tcn.2's output, residual.0's output, the pre-residual sum, the
 * block's output), tp (per applied tpcnn j < max(1, n_txpcnn - 1): pre-activation, output, (k,S,n) each), dfin (k,S,n), then
 * the gradients at tp, x, s, t, r, y, a1, g; [20] floats per pedestrian; [21] the statistics (scene s at + s x [22]: per
 * BatchNorm tcn.0, tcn.3, residual.1 five rows of S: mean, variance, 1/sqrt(var + eps), mean(dy), mean(dy x^)); [23] the
 * scenes' gradient partials, [24] = et_stgcnn_grad_floats each; [25] the total. */
#define ET_STGCNN_TRAIN_LAYOUT_FIELDS 26
int et_stgcnn_train_layout(const et_stgcnn_params *params, int64_t N, int n_scenes, int64_t *offsets, int n_offsets);
int et_stgcnn_train_forward_scenes(const et_stgcnn_params *params, const et_stgcnn_train *train, const float *C_obs,
                                   const float *nrm, int64_t N, const int32_t *scene_offsets, int n_scenes,
                                   float *C_pred_refine, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_stgcnn_train_forward_graph(const et_stgcnn_params *params, const et_stgcnn_train *train, const float *v,
                                  const float *a, int64_t N, float *out, void *workspace, size_t workspace_bytes,
                                  et_stream_t stream);
int et_stgcnn_backward_scenes(const et_stgcnn_params *params, int64_t N, const int32_t *scene_offsets, int n_scenes,
                              const float *d_out, float *grads, int64_t grads_floats, void *workspace,
                              size_t workspace_bytes, et_stream_t stream);
int et_stgcnn_backward_graph(const et_stgcnn_params *params, int64_t N, const float *d_out, float *grads,
                             int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- GP-Graph-SGCN predictor, inference (baseline/gpgraphsgcn: bridge.py pre-hook + GPGraph.forward around the
 * two-channel SGCN of model_baseline.py + post-hook) --------------------------------------------------------------------
 * The ET configuration: d_type 'learned_l2norm', learned threshold, mix_type 'mlp', all three graphs, shared weights,
 * eval mode, dropout = 0, fp32.  `base` is the SGCN table above with ONE difference: att[1].emb_w, the temporal
 * attention's embedding.weight, is (64, 2) -- column 0 the position channel, column 1 the coefficient channel.
 *   group_w / group_b   group_gen.group_cnn.0.weight (8, 1, 3, 1) / .bias (8)
 *   th                  group_gen.th (1), read on the device at every call;  tau: the sigmoid's temperature (0.1)
 *   mix_a               group_mix.st_gcns_mix.0.weight (1), the PReLU slope
 *   mix_w / mix_b       group_mix.st_gcns_mix.1.weight (S k, 3 S k, 1, 1) / .bias (S k)
 * Per scene: d[i][j] = mean over t of the L2 norm over the 8 channels of conv(v_abs)[:, t, i] - conv(v_abs)[:, t, j]; the
 * pairs (r, c), c < r, d[r][c] <= th, in row-major order, each relabel every pedestrian that carries r's label with c (the
 * reference's loop: the LAST close column of a row wins -- not connected components); labels made compact in the order of
 * the surviving values.  v' = (v_rel - v_soft) + v_soft with v_soft = v_rel @ (sig / sig.sum(0)), sig = sigmoid(-(d - th) /
 * tau).  The base runs on v_rel, on the group means of v' (G nodes, unpooled by gather) and on v' with the spatial mask
 * times the same-group matrix, identities eye(n) and eye(T); out = mean of the three + mix(PReLU(cat of the three)).
 *
 *   et_gpgraph_sgcn_forward_graph   one scene as the bridge hands it over: v_abs (1,1,T,N), v_rel (1,2,T,N) (channel 0 the
 *                                   position) -> out (1,S,k,N)
 *   et_gpgraph_sgcn_forward_scenes  a whole split: C_obs (k,N), nrm (4,N), scene_offsets, sum_n2, max_scene_n as
 *                                   et_sgcn_forward_scenes (v_abs = [C_obs; nrm[0:2] - their mean over the scene], position
 *                                   t + 1) -> C_pred_refine (k,N,S).  A scene larger than ET_SGCN_MAX_N or one that does
 *                                   not fit the stacks is not computed: its outputs are NaN (a scene larger than
 *                                   ET_SGCN_MAX_N takes no room in the stacks: leave it out of sum_n2, and of the packed
 *                                   dist / logit_s offsets).  n_scenes = 0 takes N = 0 only.
 * Optional outputs (may be NULL): group_index int32 (N), the scene-local compact label; dist, n x n per scene, scene s at
 * sum_{s'<s} n_s'^2; logit_s / logit_t of the three passes: pass m (0 pedestrian, 1 pooled, 2 intra-group) of scene s at
 * 4 T (m sum_n2 + sum_{s'<s} n_s'^2) as (T,4,n_m,n_m) and at 4 T T (m N + off[s]) as (n_m,4,T,T), n_m = G for the pooled pass.
 * The three passes of all scenes are 3 n_scenes virtual scenes of ONE run of the layered SGCN kernels (node counts from a
 * device table): 8 + number_asymmetric_conv_layer launches for any number of scenes (prep, group, input, fuse, the
 * asymmetric layers, tadj, sadj, tail, mix), no host synchronisation, no allocation (capturable in a graph); every sum has
 * a fixed order: bit-identical from run to run, and a scene's result does not depend on the scenes around it. */
typedef struct et_gpgraph_sgcn_params {
    et_sgcn_params base;
    const float *group_w, *group_b, *th;
    float tau;
    const float *mix_a, *mix_w, *mix_b;
} et_gpgraph_sgcn_params;
size_t et_gpgraph_sgcn_workspace_bytes(const et_gpgraph_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes);
int et_gpgraph_sgcn_forward_graph(const et_gpgraph_sgcn_params *params, const float *v_abs, const float *v_rel, int64_t N,
                                  float *out, int32_t *group_index, float *dist, float *logit_s, float *logit_t,
                                  void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_gpgraph_sgcn_forward_scenes(const et_gpgraph_sgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                   const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                                   float *C_pred_refine, int32_t *group_index, float *dist, float *logit_s,
                                   float *logit_t, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- GP-Graph-SGCN predictor, training (the configuration above; dropout = 0 makes the training-mode forward the eval
 * forward) ---------------------------------------------------------------------------------------------------------------
 * Gradients of what et_gpgraph_sgcn_forward_graph computes with respect to every parameter of the wrapper and of its base;
 * no gradient for v_abs / v_rel (the bridge builds them from detached tensors).  group_index is not differentiable; the
 * grouping reaches the output through v' = (v_rel - v_soft).detach() + v_soft alone (the straight-through estimator).
 *   et_gpgraph_sgcn_train_workspace_bytes  the training workspace: the base's (et_sgcn_train_workspace_bytes' layout for the
 *                                          3 N virtual rows, 3 sum_n2 entries and 3 n_scenes virtual scenes of the three
 *                                          passes), the wrapper's eval values, sig, its column sums and the group sizes, and
 *                                          the backward's intermediate gradients and partial sums.  0: outside the family.
 *   et_gpgraph_sgcn_train_forward_graph /  et_gpgraph_sgcn_forward_graph / _scenes with the kept layout: the same kernels, the
 *   et_gpgraph_sgcn_train_forward_scenes   same 8 + number_asymmetric_conv_layer launches, bit-equal outputs.
 *   et_gpgraph_sgcn_backward_graph /       d_out, laid out as the forward's output ((1,S,k,N) / (k,N,S)), and the workspace as
 *   et_gpgraph_sgcn_backward_scenes        that forward left it (same parameters, N, scene_offsets, sum_n2) -> grads,
 *                                          grads_floats >= et_gpgraph_sgcn_grad_floats floats, in the state_dict order of the
 *                                          whole GPGraph: baseline_model.* as et_sgcn_backward_graph lists them (the temporal
 *                                          attention's embedding.weight is (64, 2)), group_gen.th, group_gen.group_cnn.0.weight,
 *                                          .bias, group_mix.st_gcns_mix.0.weight, .1.weight, .1.bias.
 *                                          number_asymmetric_conv_layer + 13 launches for any number of scenes and any n:
 *                                          mix_bwd, mixw_bwd, unpool, the base's number_asymmetric_conv_layer + 7 on the
 *                                          virtual scenes, dx (the base's input gradient of passes 1 and 2), group_bwd, reduce.
 * The order: mix (d o_m = g / 3 + (W^T g)_m (z > 0 ? 1 : a)), unpool (a group's row: its members' d o_1, ascending), the
 * base's backward of the three virtual scenes (weight gradients: chunks ascending, then virtual scenes ascending), its input
 * gradient for passes 1 and 2, pool (d v' = d v'_intra + d pooled[group] / |group|), straight-through (d v_soft = d v'),
 * d P[i][j] = sum_{c,t} v_rel[c,t,i] d v_soft[c,t,j], d sig = (d P - sum_i' P d P) / colsum, d u = d sig sig (1 - sig),
 * d d = -d u / tau, d th = sum d u / tau, d f_i = sum_j (d d[i][j] + d d[j][i]) / T (f_i - f_j) / |f_i - f_j| (0 where the norm
 * is 0: the diagonal and coincident pedestrians), and group_cnn's weight and bias from d f.
 * A scene that the forward does not compute contributes nothing.  key.bias of both attentions gets an exact +0.0.  No
 * atomics: the base's partial sums as above; d (mix_a, mix_w, mix_b) per chunk of ET_GPGRAPH_BWD_ROWS pedestrians (rows
 * ascending), then the chunks ascending; d (th, group_cnn) per scene (a lane's items ascending, the lanes by a fixed
 * butterfly, the wavefronts ascending), then the scenes ascending.  Bit-identical from run to run. */
#define ET_GPGRAPH_BWD_ROWS 64
size_t et_gpgraph_sgcn_train_workspace_bytes(const et_gpgraph_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes);
int64_t et_gpgraph_sgcn_grad_floats(const et_gpgraph_sgcn_params *params);
/* where the training workspace keeps what (host only, no launch), in floats from its start.  The first 23 fields are
 * et_sgcn_train_layout's without its total, for the virtual rows (pass m of a scene at rows m N + off[s], at m sum_n2 + its
 * packed offset in the n^2 stacks); then the position channel (T, 3 N), the virtual scenes' node counts (int32), the group
 * index (int32 N), per spatial row d (A_s x), per spatial row (sum dense d dense, d t_i), per temporal row (sum dense d
 * dense, d a, d b), per temporal row d (A_t x), A_s^T d (A_s x) (n,4,T), the input gradient's position and coefficient
 * channel (T, n_m blocks at T x the virtual row); then the wrapper's: v_abs, f = group_cnn(v_abs) (8,T,n at 8 T off[s]),
 * dist, sig / colsum, the passes' outputs (k, 3 N, S), sig, its column sums, the group sizes (int32), d o_m per pedestrian
 * (k, 3 N, S), the base's upstream gradient (k, 3 N, S; pass 1 pooled), d v' (2,T,n at 2 T off[s]), d P, d sig, d d (n,n at
 * the packed offset), d f (8,T,n), the total. */
#define ET_GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS 49
int et_gpgraph_sgcn_train_layout(const et_gpgraph_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes,
                                 int64_t *offsets, int n_offsets);
int et_gpgraph_sgcn_train_forward_scenes(const et_gpgraph_sgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                         const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                                         float *C_pred_refine, int32_t *group_index, float *dist, float *logit_s,
                                         float *logit_t, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_gpgraph_sgcn_train_forward_graph(const et_gpgraph_sgcn_params *params, const float *v_abs, const float *v_rel,
                                        int64_t N, float *out, int32_t *group_index, float *dist, float *logit_s,
                                        float *logit_t, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_gpgraph_sgcn_backward_scenes(const et_gpgraph_sgcn_params *params, int64_t N, const int32_t *scene_offsets,
                                    int n_scenes, int64_t sum_n2, int64_t max_scene_n, const float *d_out, float *grads,
                                    int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_gpgraph_sgcn_backward_graph(const et_gpgraph_sgcn_params *params, int64_t N, const float *d_out, float *grads,
                                   int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- GP-Graph-STGCNN predictor, inference (baseline/gpgraphstgcnn: bridge.py pre-hook + GPGraph.forward around the
 * social_stgcnn of model_baseline.py + post-hook) ------------------------------------------------------------------------
 * The ET configuration, as for GP-Graph-SGCN; group_w .. mix_b as there.  `base` is the Social-STGCNN table above with ONE
 * difference: the base is the ORIGINAL Social-STGCNN, whose gcn convolves to S channels and contracts time row t with its
 * own Laplacian (einsum 'nctv,tvw->nctw'), so st_gcns[i].gcn_w is (S, C_in, 1, 1) and gcn_b (S).  The bridge hands over
 * v_abs = v_rel = v (1,1,T,N), v = [C_obs; obs_ori].  Per scene: the grouping of GP-Graph-SGCN on one channel; the base runs
 * on v with L = laplacian(v), on the group means of v' (G nodes, unpooled by gather) and on v' with a_inv multiplied by the
 * same-group matrix BEFORE + I (so the mask enters the degree); laplacian: a = |v_i - v_j| per time row, a_inv = 1 / a (0
 * where a == 0), a_hat = a_inv + I, L = I - D^-1/2 a_hat D^-1/2, formed where it is used, never stored.
 *
 *   et_gpgraph_stgcnn_forward_graph   one scene as the bridge hands it over -> out (1,S,k,N)
 *   et_gpgraph_stgcnn_forward_scenes  a whole split, arguments as et_gpgraph_sgcn_forward_scenes -> C_pred_refine (k,N,S);
 *                                     a scene larger than ET_SGCN_MAX_N or one that does not fit the workspace: NaN rows
 * Optional outputs (may be NULL): group_index int32 (N); dist, packed as for GP-Graph-SGCN; graph_inputs (3, T N) float: the
 * three passes' inputs exactly as the second kernel reads them, pass m of scene s a (T, n_m) block at T (m N + off[s]),
 * n_m = n, G, n (the rest of a pass-1 block is not written).
 * Three launches for any number of scenes (group, the 3 n_scenes virtual scenes, mix), no host synchronisation, no
 * allocation; a virtual scene's arena is in LDS when it fits (n_m <= 33 at S = 20, k = 6), else in the workspace.  Every
 * sum has a fixed order: bit-identical from run to run, and a scene's result does not depend on the scenes around it. */
typedef struct et_gpgraph_stgcnn_params {
    et_stgcnn_params base;
    const float *group_w, *group_b, *th;
    float tau;
    const float *mix_a, *mix_w, *mix_b;
} et_gpgraph_stgcnn_params;
size_t et_gpgraph_stgcnn_workspace_bytes(const et_gpgraph_stgcnn_params *params, int64_t N, int64_t sum_n2, int n_scenes);
int et_gpgraph_stgcnn_forward_graph(const et_gpgraph_stgcnn_params *params, const float *v_abs, const float *v_rel, int64_t N,
                                    float *out, int32_t *group_index, float *dist, float *graph_inputs, void *workspace,
                                    size_t workspace_bytes, et_stream_t stream);
int et_gpgraph_stgcnn_forward_scenes(const et_gpgraph_stgcnn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                     const int32_t *scene_offsets, int n_scenes, int64_t sum_n2, int64_t max_scene_n,
                                     float *C_pred_refine, int32_t *group_index, float *dist, float *graph_inputs,
                                     void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- DMRGCN predictor, inference (baseline/dmrgcn: bridge.py pre-hook + social_dmrgcn.forward + post-hook) -------------
 * Eval mode only (no drop_edge, no dropout); the network has no BatchNorm.  The parameters are read in place from the
 * module's own tensors through the pointer tables below (fp32, contiguous).  Field <-> state_dict name (i = st_dmrgcn
 * block, r = relation 0 displacement / 1 distance, j = tpcnn block, m = 0, 1):
 *   st_dmrgcns[i].gcn_w[r] / gcn_b[r]   st_dmrgcns.{i}.gcns.{r}.conv.weight (5 S, C_in, 1, 1) / .bias (5 S): channel b S + c
 *   st_dmrgcns[i].tcn_prelu             st_dmrgcns.{i}.tcn.0.weight (1)
 *   st_dmrgcns[i].tcn_w / tcn_b         st_dmrgcns.{i}.tcn.1.weight (S, S, 3, 1) / .bias (S)
 *   st_dmrgcns[i].res_w / res_b         st_dmrgcns.{i}.residual.0.weight (S, C_in, 1, 1) / .bias (S); NULL when C_in == S
 *   st_dmrgcns[i].prelu                 st_dmrgcns.{i}.prelu.weight (1)
 *   tpcnns[j].conv_w[m] / conv_b[m]     tpcnns.{j}.tpcn.{m}.0.weight (k, m == 0 && j == 0 ? K : k, 3, 3) / .bias (k)
 *   tpcnns[j].conv_a[m]                 tpcnns.{j}.tpcn.{m}.1.weight (1)
 *   tpcnns[j].gta_w / gta_b / gta_a     tpcnns.{j}.gtacn.0.0.weight (S, S, k, 1) / .bias (S), gtacn.0.1.weight (1)
 *   tpcnns[j].res_w / res_b             tpcnns.0.residual.0.weight (k, K, 1, 1) / .bias (k); NULL for j > 0 (identity)
 * with K = seq_len, k = pred_seq_len, S = output_feat, C_in = 1 in block 0 and S afterwards.  `split` holds the two
 * disentangling scale sets, which the reference keeps as constructor constants ([0, 1/4, 2/4, 3/4, 1] for the
 * displacement relation, [0, 1/2, 1, 2, 4] for the distance relation); 1e10 closes the last bin.
 * Supported: input_feat = 1, kernel_size = 3, seq_len = pred_seq_len + 2, 1 <= pred_seq_len <= ET_MAX_K,
 * 1 <= output_feat <= 64, 1 <= n_stgcn <= ET_DMRGCN_MAX_STGCN, 1 <= n_tpcnn <= ET_DMRGCN_MAX_TPCNN, ET_DMRGCN_BINS
 * bins per relation with 0 <= split[r][0] < split[r][1] < ... < 1e10; anything else: ET_ERR_UNSUPPORTED.  A missing
 * pointer: ET_ERR_INVALID_ARG.
 *
 * The graphs (bridge.py:4-19, dmrgcn.py:12-35): A_dist[t,i,j] = |v[t,i] - v[t,j]|, A_disp the same on v_rel (v_rel[0] = 0,
 * v_rel[t] = v[t] - v[t-1]); bin b of relation r is the indicator of the OPEN interval split[r][b] < A < split[r][b+1] --
 * a distance equal to a split value is in no bin, nor is 0 (the diagonal); per (r, b, t): L = I - D^-1/2 (A_b + I) D^-1/2
 * with D = rowsum(A_b + I) >= 1.  The decisions are fp32 comparisons of fp32 distances: exactly the reference's.
 *   et_dmrgcn_forward_graph   one scene as the bridge hands it over: v (1,1,K,N), a (1,2,K,N,N) = [A_disp, A_dist], read
 *                             as given -> out (1,S,k,N), the network's raw output v.  N <= ET_SCENE_MAX_N.
 *   et_dmrgcn_forward_scenes  a whole split: C_obs (k,N), nrm (4,N) of et_norm_project; per scene v = [C_obs; nrm[0:2] -
 *                             their mean over the scene], summed in et_scene_project's order; v_rel and the distances
 *                             are formed where they are used, the (2,5,K,n,n) stacks are never stored -> C_pred_refine
 *                             (k,N,S).  scene_offsets as et_traj_metrics (NULL = one scene of N rows); n_scenes = 0
 *                             takes N = 0 only.  Optional output graph_inputs (K,N) float (may be NULL): the fp32 v the
 *                             kernel used, scene s at columns [off[s], off[s+1]).  One launch.
 * Workspace: a scene whose activations fit a workgroup's LDS arena (at S = 20, k = 6: up to 26 pedestrians) needs none;
 * larger ones use workspace rows [off[s], off[s+1]) of et_dmrgcn_workspace_bytes(p, N, max_scene_n) bytes (0 when a
 * scene of max_scene_n pedestrians fits the arena).  A scene larger than ET_SCENE_MAX_N, or one that fits neither, is
 * not computed: its outputs are NaN.  No host synchronisation, no allocation: the calls can be captured in a graph.
 * Every sum has a fixed order: a scene's result does not depend on the scenes around it or on where its arena lies.
 * A NaN or inf in a scene's v (C_obs, nrm) makes that scene's outputs NaN, as the reference's dense einsum does. */
#define ET_DMRGCN_MAX_STGCN 4
#define ET_DMRGCN_MAX_TPCNN 8
#define ET_DMRGCN_BINS 5
typedef struct et_dmrgcn_layer {
    const float *gcn_w[2], *gcn_b[2];
    const float *tcn_prelu;
    const float *tcn_w, *tcn_b;
    const float *res_w, *res_b;
    const float *prelu;
} et_dmrgcn_layer;
typedef struct et_dmrgcn_tpcnn {
    const float *conv_w[2], *conv_b[2], *conv_a[2];
    const float *gta_w, *gta_b, *gta_a;
    const float *res_w, *res_b;
} et_dmrgcn_tpcnn;
typedef struct et_dmrgcn_params {
    int n_stgcn, n_tpcnn, input_feat, output_feat, seq_len, pred_seq_len, kernel_size;
    float split[2][ET_DMRGCN_BINS];
    et_dmrgcn_layer st_dmrgcns[ET_DMRGCN_MAX_STGCN];
    et_dmrgcn_tpcnn tpcnns[ET_DMRGCN_MAX_TPCNN];
} et_dmrgcn_params;
size_t et_dmrgcn_workspace_bytes(const et_dmrgcn_params *params, int64_t N, int64_t max_scene_n);
int et_dmrgcn_forward_graph(const et_dmrgcn_params *params, const float *v, const float *a, int64_t N, float *out,
                            void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_dmrgcn_forward_scenes(const et_dmrgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                             const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *graph_inputs,
                             void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- DMRGCN predictor, training (social_dmrgcn.forward in training mode + its backward pass) ---------------------------
 * The training-mode forward is NOT the eval forward: every MultiRelationalGCN applies drop_edge(A_, 0.8) to the clipped 0/1
 * bin tensor (dropedge.py), so every (relation, bin, time row) graph loses entries independently per direction and is no
 * longer symmetric.  The draw is the caller's: `keep`, uint8, (2,5,K,N,N) indexed [r,b,t,w,v] (graph form), entry != 0
 * keeps A_b[w,v]; scenes form: scene s's own (2,5,K,n,n) block starts at 10 K keep_offsets[s], keep_offsets (device,
 * n_scenes + 1 int64_t) the running sum of n^2 over the scenes (a scene above the cap takes no room); keep = NULL keeps
 * everything.  cnt[r,b,t,w] = the kept entries of row w, d_w = 1/sqrt(1 + cnt), L[w,v] = [v==w] - (d_w (A'[w,v] + [v==w]))
 * d_v with d_v the column pedestrian's own row degree; every other statement is et_dmrgcn_forward_*'s in its order, so with
 * keep = NULL or all ones the output is bit-equal to the inference entry's.
 * Trained natively: the inference family with n_stgcn = 1 (the only depth the reference builds; deeper stacks send a
 * gradient through the Laplacians: ET_ERR_UNSUPPORTED) and scenes of at most ET_DMRGCN_TRAIN_MAX_N pedestrians (a larger
 * scene of the scenes form is not computed: NaN outputs, no gradient; graph form: ET_ERR_INVALID_ARG).
 *   et_dmrgcn_train_workspace_bytes  the training workspace for N pedestrians in n_scenes scenes (graph form: 1): what the
 *                                    forward keeps, the activation gradients, an arena for scenes that do not fit LDS and
 *                                    the scenes' gradient partials.  0: outside the family, N <= 0 or n_scenes < 1.
 *   et_dmrgcn_train_forward_graph /  arguments as et_dmrgcn_forward_graph / _scenes plus the mask.  ONE launch, one
 *   et_dmrgcn_train_forward_scenes   workgroup per scene, the live operands in the LDS arena when the scene fits it (at
 *                                    S = 20, k = 6: up to 24 pedestrians), else in the workspace's arena rows.
 *   et_dmrgcn_backward_graph /       d_out laid out as the forward's output ((1,S,k,N) / (k,N,S)) and the workspace as that
 *   et_dmrgcn_backward_scenes        forward left it (same parameters, N, scene_offsets) -> grads, grads_floats >=
 *                                    et_dmrgcn_grad_floats floats: every parameter's gradient in state_dict order
 *                                    (st_dmrgcns.0: gcns.0.conv.weight, .bias, gcns.1.conv.weight, .bias, tcn.0.weight,
 *                                    tcn.1.weight, .bias, [residual.0.weight, .bias,] prelu.weight; tpcnns.j: tpcn.0.0.weight,
 *                                    .bias, tpcn.0.1.weight, tpcn.1.0.weight, .bias, tpcn.1.1.weight, gtacn.0.0.weight, .bias,
 *                                    gtacn.0.1.weight, [residual.0.weight, .bias]).  THREE launches for any N and any number
 *                                    of scenes: the activation gradients (one workgroup per scene, the dependent chain in
 *                                    the arena), the parameter gradients (16 workgroups per scene: every element is one
 *                                    wavefront's sum, the scene's 64 wavefronts take them round robin), the reduction.
 * No gradient with respect to the input.  No atomics: a gradient element of a scene is one wavefront's sum over the
 * element's positions (lane l adds positions l, l + 64, ... in ascending order, then the lanes by the xor butterfly 32, 16,
 * ..., 1), and the scenes' partials are added in ascending order, the first one copied; results are bit-identical from run
 * to run, and a one-scene scenes call equals the graph call.  Host-side checks answer ET_ERR_UNSUPPORTED /
 * ET_ERR_INVALID_ARG / ET_ERR_WORKSPACE before any launch. */
#define ET_DMRGCN_TRAIN_MAX_N 512
size_t et_dmrgcn_train_workspace_bytes(const et_dmrgcn_params *params, int64_t N, int n_scenes);
int64_t et_dmrgcn_grad_floats(const et_dmrgcn_params *params);
/* where the training workspace keeps what (host only, no launch), in floats.  Per-pedestrian fields first (scene s's block
 * starts at off[s] x [10]; field f of it at + offsets[f] x the scene's n): [0] u (K,n), [1] P (2,5,2,K,n) the contraction
 * rows (j = 0 from u, j = 1 from the ones row), [2] yp (S,K,n) the tcn PReLU's input, [3] s (S,K,n) the block PReLU's
 * input, [4] x (K,S,n) the block's output, [5] per tpcnn block j at + j x [11]: c0, y, c1, q, o (k,S,n each: tpcn.0's
 * pre-activation and output, tpcn.1's, the block's output), z (S,n) the GTA pre-activation, [6] per tpcnn block at + j x
 * [12]: dq, dy (k,S,n), dg (S,n) the gradients at q, y and the GTA row, [7] dx (K,S,n), [8] dy (S,K,n) the gradient at
 * PReLU(yp), [9] the arena; [10] floats per pedestrian; [13] the scenes' gradient partials, [14] = et_dmrgcn_grad_floats
 * each; [15] the total. */
#define ET_DMRGCN_TRAIN_LAYOUT_FIELDS 16
int et_dmrgcn_train_layout(const et_dmrgcn_params *params, int64_t N, int n_scenes, int64_t *offsets, int n_offsets);
int et_dmrgcn_train_forward_graph(const et_dmrgcn_params *params, const float *v, const float *a, int64_t N,
                                  const uint8_t *keep, float *out, void *workspace, size_t workspace_bytes,
                                  et_stream_t stream);
int et_dmrgcn_train_forward_scenes(const et_dmrgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                   const int32_t *scene_offsets, int n_scenes, const uint8_t *keep,
                                   const int64_t *keep_offsets, float *C_pred_refine, void *workspace,
                                   size_t workspace_bytes, et_stream_t stream);
int et_dmrgcn_backward_graph(const et_dmrgcn_params *params, int64_t N, const float *d_out, float *grads,
                             int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_dmrgcn_backward_scenes(const et_dmrgcn_params *params, int64_t N, const int32_t *scene_offsets, int n_scenes,
                              const float *d_out, float *grads, int64_t grads_floats, void *workspace,
                              size_t workspace_bytes, et_stream_t stream);

/* ---- Social-Implicit predictor, inference (baseline/implicit: bridge.py pre-hook + SocialImplicitLight.forward + post-hook)
 * Eval mode, the Light form (its noise is identically zero, so the noise_w term is not computed; noise_w is carried so
 * that the table is complete).  The parameters are read in place from the module's tensors (fp32, contiguous).  Per cell
 * i = zone, global_t[j] / local_t[j] with j = 0..7 are, of implicit_cells.{i}. and implicit_cells.{i}.ped.:
 *   0, 1  feat.weight (S,1,3,3) / (S,1,3), .bias (S)          2, 3  highway_input.weight (S,1,1,1) / (S,1,1), .bias (S)
 *   4, 5  highway.weight (T_out,T,1,1) / (T_out,T,1), .bias   6, 7  tpcnn.weight (T_out,T,3,3) / (T_out,T,3), .bias (T_out)
 * and noise_w, global_w, local_w the cell's three scalars; S = spatial_output, T = temporal_input, T_out =
 * temporal_output.  `bins` are the n_bins ascending zone bounds ([0, 0.01, 0.1, 1.2] in the reference's configuration).
 * Supported: spatial_input = 1, 1 <= S <= 64, 1 <= T, T_out <= 16, 1 <= n_bins <= ET_IMPLICIT_MAX_BINS, bins[b] <=
 * bins[b+1]; anything else: ET_ERR_UNSUPPORTED.  A missing pointer: ET_ERR_INVALID_ARG.
 *
 * The network (model.py:9-88,126-159): zone[n] = (number of bins b with bins[b] <= |v[0,n]|) - 1, an exact fp32
 * comparison (a NaN lands in the last zone; a norm below bins[0] is in no zone and its output is 0).  Each zone's cell
 * runs on the zone's pedestrians COMPACTED in scene order.  Global stream: u = relu(feat(v)) + highway_input(v) (S,T,n_z),
 * then with T as channels highway(u) + tpcnn(u), tpcnn's 3x3 over the (S, n_z) plane zero-padding u; local stream, per
 * pedestrian: the same with 1-d convolutions, whose (T_out,S) result is reinterpreted (reshape, no transpose) as
 * (S,T_out); out = global_w global + local_w local, written at the pedestrian's own column.
 *   et_implicit_forward_graph   one scene as the bridge hands it over: v (1,1,T,N) -> out (1,S,T_out,N).
 *                               N <= ET_SCENE_MAX_N.
 *   et_implicit_forward_scenes  a whole split: C_obs (T-2,N), nrm (4,N) of et_norm_project; per scene v = [C_obs;
 *                               nrm[0:2] - their mean over the scene], summed in et_scene_project's order ->
 *                               C_pred_refine (T_out,N,S), the post-hook's permute.  T >= 3.  scene_offsets as
 *                               et_traj_metrics (NULL = one scene of N <= ET_SCENE_MAX_N rows); n_scenes = 0 takes N = 0
 *                               only.  Optional outputs (may be NULL): graph_inputs (T,N) float, the fp32 v used, scene
 *                               s at columns [off[s], off[s+1]); zone (N,) int32.  A scene larger than
 *                               ET_SCENE_MAX_N is not computed: its outputs are NaN and its zones -2.
 *                               (Its rows of the workspace's table keep, in their spare eighth entry, the zone each
 *                               pedestrian would have had: read by et_implicit_backward_scenes alone.)
 * Two launches per call whatever the number of scenes: one finds every pedestrian's zone and its two predecessors and two
 * successors of the same zone within its scene, one computes every pedestrian on its own from those five columns.
 * Workspace: et_implicit_workspace_bytes(p, N) bytes (0 for N = 0 or parameters outside the family).  No host
 * synchronisation, no allocation: the calls can be captured in a graph.  Every sum has a fixed order: a pedestrian's
 * result depends on its scene alone, not on the scenes around it, the launch size or the tiling. */
#define ET_IMPLICIT_MAX_BINS 8
typedef struct et_implicit_cell {
    const float *global_t[8];
    const float *local_t[8];
    const float *noise_w, *global_w, *local_w;
} et_implicit_cell;
typedef struct et_implicit_params {
    int spatial_input, spatial_output, temporal_input, temporal_output, n_bins;
    float bins[ET_IMPLICIT_MAX_BINS];
    et_implicit_cell cells[ET_IMPLICIT_MAX_BINS];
} et_implicit_params;
size_t et_implicit_workspace_bytes(const et_implicit_params *params, int64_t N);
int et_implicit_forward_graph(const et_implicit_params *params, const float *v, int64_t N, float *out, void *workspace,
                              size_t workspace_bytes, et_stream_t stream);
int et_implicit_forward_scenes(const et_implicit_params *params, const float *C_obs, const float *nrm, int64_t N,
                               const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *graph_inputs,
                               int32_t *zone, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- Social-Implicit predictor, training: the backward pass of the two calls above (their forward is the training-mode
 * forward: the Light form has no dropout, no BatchNorm, no sampling).  `grads` (n_bins, G) fp32 with G = 18 S + 14 T_out T
 * + 4 T_out + 2, the sizes of the 18 tensors below together (1058 in the reference's configuration): per cell, in et_implicit_cell's field order,
 * the gradients of global_t[0..7], local_t[0..7], global_w, local_w (noise_w multiplies the zero noise: its gradient is
 * an exact zero and is not stored).  The block is fully overwritten; a cell no pedestrian is in gets +0.0 everywhere (the
 * reference leaves its .grad None); the cell of a pedestrian of a scene larger than ET_SCENE_MAX_N gets NaN.  No input
 * gradient is formed (the bridge detaches v).
 *   et_implicit_backward_graph   one scene: v (T,N) and forward_workspace as et_implicit_forward_graph read / filled them,
 *                                g_out the gradient at its out: g_layout ET_IMPLICIT_G_STN (1,S,T_out,N), or
 *                                ET_IMPLICIT_G_TNS the same values as (T_out,N,S), the implicit bridge's post-hook's
 *                                permute undone by autograd; another value: ET_ERR_INVALID_ARG.
 *   et_implicit_backward_scenes  a whole batch: forward_workspace as et_implicit_forward_scenes filled it (the table and
 *                                every scene's v), g (T_out,N,S) the gradient at C_pred_refine.
 * Two launches whatever N and the number of scenes, no atomics: an element's terms are added rows ascending (within a row
 * ascending over the element's own inner index) inside chunks of ET_IMPLICIT_BWD_CHUNK rows, then the chunks ascending.
 * Workspace: et_implicit_backward_workspace_bytes(p, N) (0 for N = 0 or outside the family).  Errors as the forward
 * entries; N = 0: ET_OK, the block zeroed.  No host synchronisation, no allocation. */
#define ET_IMPLICIT_BWD_CHUNK 8
#define ET_IMPLICIT_G_STN 0
#define ET_IMPLICIT_G_TNS 1
size_t et_implicit_backward_workspace_bytes(const et_implicit_params *params, int64_t N);
int et_implicit_backward_graph(const et_implicit_params *params, const float *v, int64_t N, const void *forward_workspace,
                               size_t forward_workspace_bytes, const float *g_out, int g_layout, float *grads,
                               void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_implicit_backward_scenes(const et_implicit_params *params, int64_t N, const void *forward_workspace,
                                size_t forward_workspace_bytes, const float *g, float *grads, void *workspace,
                                size_t workspace_bytes, et_stream_t stream);

/* ---- PECNet / LBEBM predictors, inference (baseline/pecnet, baseline/lbebm: bridge.py hooks + predict) ---------------
 * Both predict bodies are chains of Linear + ReLU (no activation after a chain's last layer) in exact fp32: every product
 * on the f32-input MFMA, accumulated in fp32 ascending in k, the bias added last.  The weights are read in place from the
 * module's tensors: chain.w[i] is <chain>.layers.{i}.weight (widths[i+1], widths[i]) row-major, chain.b[i] its bias.
 *   LBEBM.predict    predictor(encoder_past(past) | encoder_dest(dest))                                  2 launches
 *   PECNet.predict   the same with initial_pos appended (pos_width = 2) and nonlocal_pools rounds of non-local social
 *                    pooling in between: feat <- normalize_1(softmax(theta(feat) phi(feat)^T) * mask) g(feat) + feat,
 *                    the softmax over every column of the row's range BEFORE the mask, normalize_1 the division by
 *                    max(sum |w|, 1e-12) (an all-zero mask row gives feat back).      2 + 2 nonlocal_pools launches
 * A launch takes 16 rows per workgroup through ALL layers of a chain (activations in LDS) and runs up to three chains side
 * by side (encoder_past + encoder_dest; theta + phi + g); the concatenated inputs are gathered, never stored.  An output
 * element's summation order depends on the layer's shape only: a row's result does not depend on the rows around it.
 *   et_*_predict          the module form: past (N, encoder_past.widths[0]), dest (N, encoder_dest.widths[0]),
 *                         initial_pos (N, 2), mask (N, N) float or NULL (all ones), one range of N rows -> out (N, out_width)
 *   et_*_forward_scenes   a whole split: C_obs (k, N), nrm (4, N) of et_norm_project; past = C_obs^T, dest = initial_pos =
 *                         obs_ori = nrm[0:2] - their mean over the scene (summed in et_scene_project's order), one softmax
 *                         range per scene (the reference's test loader: one scene per call, all-ones mask), the post-hook's
 *                         layout -> C_pred_refine (k, N, out_width / k).  scene_offsets as et_traj_metrics (NULL = one
 *                         scene); n_scenes = 0 takes N = 0 only.  Optional net_inputs (k + 2, N): the fp32 [C_obs; obs_ori]
 *                         the call used.  k = encoder_past.widths[0], dest width 2.
 * Supported: 2 to ET_MLP_MAX_LAYERS Linear layers per chain (1 to 4 hidden), widths 1 to ET_MLP_MAX_WIDTH, nonlocal_pools
 * 0 to ET_MLP_MAX_POOLS, a softmax range of up to ET_MLP_MAX_RANGE rows (a longer scene's rows are NaN; the module form
 * with pooling and N beyond it: ET_ERR_UNSUPPORTED); anything else ET_ERR_UNSUPPORTED, before any launch.  The workspace
 * (et_*_workspace_bytes) holds the activations between launches.  No host synchronisation, no allocation. */
#define ET_MLP_MAX_LAYERS 5
#define ET_MLP_MAX_WIDTH 1024
#define ET_MLP_MAX_POOLS 8
#define ET_MLP_MAX_RANGE 4096
typedef struct et_mlp_chain {
    int n_layers;
    int widths[ET_MLP_MAX_LAYERS + 1];
    const float *w[ET_MLP_MAX_LAYERS], *b[ET_MLP_MAX_LAYERS];
} et_mlp_chain;
typedef struct et_mlp_params {
    int fdim, nonlocal_pools, non_local_dim, out_width, pos_width;
    et_mlp_chain encoder_past, encoder_dest, non_local_theta, non_local_phi, non_local_g, predictor;
} et_mlp_params;
size_t et_pecnet_workspace_bytes(const et_mlp_params *params, int64_t N);
int et_pecnet_predict(const et_mlp_params *params, const float *past, const float *dest, const float *mask,
                      const float *initial_pos, int64_t N, float *out, void *workspace, size_t workspace_bytes,
                      et_stream_t stream);
int et_pecnet_forward_scenes(const et_mlp_params *params, const float *C_obs, const float *nrm, int64_t N,
                             const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *net_inputs,
                             void *workspace, size_t workspace_bytes, et_stream_t stream);
size_t et_lbebm_workspace_bytes(const et_mlp_params *params, int64_t N);
int et_lbebm_predict(const et_mlp_params *params, const float *past, const float *dest, int64_t N, float *out,
                     void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_lbebm_forward_scenes(const et_mlp_params *params, const float *C_obs, const float *nrm, int64_t N,
                            const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *net_inputs,
                            void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- LBEBM predictor, training (what the lbebm bridge runs in training too: LBEBM.predict) -------------------------------
 * Forward with the activations kept, and the backward pass, of predictor(encoder_past(past) | encoder_dest(dest)).  Notation
 * for a chain of L layers: a_0 the input, z_i = a_{i-1} W_i^T + b_i, a_i = relu(z_i) for i < L, the output z_L.
 *   et_lbebm_train_fwd   out (N, out_width) = et_lbebm_predict's, bit for bit, in the same 2 launches; `saved` receives the
 *                        two encoders' outputs and every a_i, 0 < i < L.  The workspace is not used (NULL / 0 are fine).
 *   et_lbebm_train_bwd   from g_out (N, out_width), the gradient at `out`: every dW_i (widths[i], widths[i-1]) = g_z(i)^T
 *                        a_{i-1} and db_i = the column sums of g_z(i), with g_z(L) = g_out, g_a(i-1) = g_z(i) W_i and
 *                        g_z(i-1) = g_a(i-1) where a_{i-1} > 0, else 0 (an activation of exactly 0 passes nothing); the
 *                        predictor's input gradient splits at column fdim into the two encoders' output gradients.
 *                        `grads` names where they go: the buffers are OVERWRITTEN (accumulation is the caller's).  g_past /
 *                        g_dest (may be NULL: not computed) receive the input gradients, element (row, c) at the input's
 *                        own offset row * rs + c * cs.  3 launches whatever N and the widths: the
 *                        predictor's rows, both encoders' rows, every dW / db.
 * past / dest are read in place through their strides (in elements; element (row, c) at p[row * rs + c * cs], both >= 0):
 * the bridge hands over transposed views.  `saved` and the workspace have ONE layout and ONE size,
 * et_lbebm_train_workspace_bytes(params, N) bytes each (0 for parameters outside the family), in floats, every block
 * starting on a multiple of 4 floats (a block of (N, w) takes N w rounded up to 4):
 *   encoder_past's output (N, fdim) | encoder_dest's output (N, fdim) | encoder_past a_1 .. a_{L-1}, each (N, widths[i]) |
 *   encoder_dest a_1 .. a_{L-1} | predictor a_1 .. a_{L-1}
 * the workspace holding, at the same places, the gradients at those values (g_z(i) for an a_i).  Every dot product is one
 * fp32 fmaf chain on the f32-input MFMA from a zero accumulator: over a layer's outputs ascending for g_a, over ALL rows 0
 * .. N-1 ascending for dW and db -- no atomics, no partial sums, so a value is a function of the data alone, two runs agree
 * bit for bit, and a row's g_z and input gradients do not depend on the other rows or on N.  Rows past N and columns past a
 * width are taken as zeros; nothing uninitialised is read.  Supported: et_lbebm_predict's family (2 to ET_MLP_MAX_LAYERS
 * layers, widths 1 to ET_MLP_MAX_WIDTH); anything else ET_ERR_UNSUPPORTED before any launch; a missing pointer
 * ET_ERR_INVALID_ARG; a short workspace ET_ERR_WORKSPACE.  N = 0: the forward does nothing, the backward writes zeros.  No
 * host synchronisation, no allocation. */
typedef struct et_mlp_chain_grads {
    float *dw[ET_MLP_MAX_LAYERS], *db[ET_MLP_MAX_LAYERS];
} et_mlp_chain_grads;
typedef struct et_lbebm_grads {
    et_mlp_chain_grads encoder_past, encoder_dest, predictor;
} et_lbebm_grads;
size_t et_lbebm_train_workspace_bytes(const et_mlp_params *params, int64_t N);
int et_lbebm_train_fwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                       int64_t dest_rs, int64_t dest_cs, int64_t N, float *out, float *saved, void *workspace,
                       size_t workspace_bytes, et_stream_t stream);
int et_lbebm_train_bwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                       int64_t dest_rs, int64_t dest_cs, int64_t N, const float *saved, const float *g_out,
                       const et_lbebm_grads *grads, float *g_past, float *g_dest, void *workspace, size_t workspace_bytes,
                       et_stream_t stream);

/* ---- PECNet predictor, training (what the pecnet bridge runs in training too: PECNet.predict) -----------------------------
 * Forward with everything the backward needs kept, and the backward pass, of et_pecnet_predict: the six chains (notation as
 * above) and nonlocal_pools rounds of pooling with the SAME theta / phi / g weights.  One round, feat (N, F) -> out (N, F):
 * f = theta(feat) phi(feat)^T, s = softmax(f) over all N columns, w = s * mask, den = max(sum_j |w_ij|, 1e-12), p = w / den,
 * out = p g(feat) + feat.  Its backward from G, the gradient at out:  d feat += G;  dp_ij = G_i . g_j;  dw_ij = (dp_ij -
 * sign(w_ij) sum_k dp_ik p_ik) / den where sum |w| > 1e-12, else dp_ij / 1e-12 (clamp_min's convention);  ds_ij = dw_ij
 * mask_ij, exactly 0 where mask_ij = 0;  df_ij = s_ij (ds_ij - sum_k ds_ik s_ik);  d theta_i = sum_j df_ij phi_j;  d phi_j =
 * sum_i df_ij theta_i;  d g_j = sum_i p_ij G_i.  The mask gets no gradient.
 *   et_pecnet_train_fwd   out (N, out_width) = et_pecnet_predict's, bit for bit, in the same 2 + 2 nonlocal_pools launches;
 *                         `saved` (et_pecnet_train_saved_bytes) receives the two encoders' outputs, every hidden activation
 *                         of every chain in every round, theta / phi / g of every round and the features entering every
 *                         round and the predictor (round 0's [ftraj | dfeat | initial_pos] stored as one block).  The
 *                         attention weights are NOT kept.  The workspace is not used (NULL / 0 are fine).
 *   et_pecnet_train_bwd   from g_out (N, out_width): every dW / db of the six chains (`grads`; OVERWRITTEN; with
 *                         nonlocal_pools = 0 the three non-local chains are neither checked nor written), and, where the
 *                         pointer is not NULL, the gradients of past, dest and initial_pos at the inputs' own strides.
 *                         3 + 3 nonlocal_pools launches whatever N: the predictor's rows; per round, last to first: the
 *                         pooling's rows (one wavefront per row forms s again with the forward's own statements, so with
 *                         its bits, then p, df and d theta_i), the column sums d phi and d g, then theta, phi and g
 *                         backward side by side; both encoders' rows; every dW / db.
 * The gradient at a round's input features is summed in ONE order: the residual G, then the input gradients of theta, of
 * phi and of g.  After round 0 it splits at columns fdim and 2 fdim into the two encoders' output gradients and g_pos.  A dW
 * / db element of theta / phi / g is one fp32 fmaf chain over round 0's rows 0 .. N-1, then round 1's, and so on; d phi_j and
 * d g_j are one chain over i = 0 .. N-1; the row sums (softmax, sum |w|, the two sums over k) are formed by one wavefront,
 * lane l taking j = l, l + 64, ... ascending, then a fixed butterfly over the 64 lanes.  No atomics, nothing depends on the
 * grid: two runs agree bit for bit.  A row whose mask row is all zeros has p = 0 and contributes exactly 0 to d theta, d phi
 * and d g.  past / dest / initial_pos are read in place through their strides (in elements, >= 0); mask (N, N) float32
 * row-major or NULL (all ones).  The workspace (et_pecnet_train_workspace_bytes) holds the gradients at the kept values and,
 * with pooling, p and df of ONE round, 2 N^2 floats (128 MB at N = 4096); all sizes are 0 for parameters outside the family.
 * Supported: et_pecnet_predict's family, N <= ET_MLP_MAX_RANGE with pooling; anything else ET_ERR_UNSUPPORTED before any
 * launch; a missing pointer ET_ERR_INVALID_ARG; a short workspace ET_ERR_WORKSPACE.  N = 0: the forward does nothing, the
 * backward writes zeros.  No host synchronisation, no allocation. */
typedef struct et_pecnet_grads {
    et_mlp_chain_grads encoder_past, encoder_dest, non_local_theta, non_local_phi, non_local_g, predictor;
} et_pecnet_grads;
size_t et_pecnet_train_saved_bytes(const et_mlp_params *params, int64_t N);
size_t et_pecnet_train_workspace_bytes(const et_mlp_params *params, int64_t N);
int et_pecnet_train_fwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                        int64_t dest_rs, int64_t dest_cs, const float *initial_pos, int64_t pos_rs, int64_t pos_cs,
                        const float *mask, int64_t N, float *out, float *saved, void *workspace, size_t workspace_bytes,
                        et_stream_t stream);
int et_pecnet_train_bwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                        int64_t dest_rs, int64_t dest_cs, const float *initial_pos, int64_t pos_rs, int64_t pos_cs,
                        const float *mask, int64_t N, const float *saved, const float *g_out, const et_pecnet_grads *grads,
                        float *g_past, float *g_dest, float *g_pos, void *workspace, size_t workspace_bytes,
                        et_stream_t stream);

/* ---- AgentFormer predictor, inference (baseline/agentformer: bridge.py hooks + AgentFormerLight.forward) -------------
 * Eval mode, the ET configuration family: input_type = ['pos'], pred_type = 'pos', nz = 0, no learnt prior, pos_concat,
 * no agent encoding, dot-product scores (gaussian_kernel off) with separate same-agent projections (sep_attn on), an
 * all-zero agent mask (conn_dist >= 1000), out_fc straight after the decoder.  Exact fp32: every Linear on the f32-input
 * MFMA, accumulated ascending in k, the bias added last.  The parameters are read in place from the module's tensors
 * (fp32, contiguous).  Field <-> state_dict name (E = context_encoder, F = future_decoder, i = layer):
 *   enc_embed / dec_embed .input_fc_weight / _bias   E|F.input_fc.weight (D, 1) / .bias (D)
 *                         .fc_weight / _bias         E|F.pos_encoder.fc.weight (D, 2 D) / .bias (D)
 *                         .pe                        E|F.pos_encoder.pe (max_t_len, 1, D), the buffer; rows 0 .. T-1 are read
 *   enc[i] / dec[i]       .self_attn                 E.tf_encoder.layers.{i}.self_attn. | F.tf_decoder.layers.{i}.self_attn.
 *                         .multihead_attn            F.tf_decoder.layers.{i}.multihead_attn. (decoder only; unused in enc[])
 *      an attention's     .in_proj_weight / _bias             (3 D, D) / (3 D): q | k | v
 *                         .in_proj_weight_self / _bias_self   (2 D, D) / (2 D): q_self | k_self
 *                         .out_proj_weight / _bias            out_proj.weight (D, D) / out_proj.bias (D)
 *                         .linear1_weight / _bias    layers.{i}.linear1.weight (ff, D) / .bias (ff)
 *                         .linear2_weight / _bias    layers.{i}.linear2.weight (D, ff) / .bias (D)
 *                         .norm_weight[j] / norm_bias[j]   layers.{i}.norm{j+1}.weight / .bias (D); j = 0, 1 and, decoder, 2
 *   out_fc_weight / _bias                            F.out_fc.weight (S, D) / .bias (S)
 * with D = model_dim, ff = ff_dim, T = past_frames, k = future_frames, S = forecast_dim.
 * Supported: motion_dim = 1, model_dim a multiple of 16 up to 256, nhead dividing model_dim with head_dim a multiple of 4,
 * 1 <= ff_dim <= 512, 1 to ET_AGENTFORMER_MAX_LAYERS layers each side, 1 <= T, k <= 16, 1 <= S <= 64; anything else:
 * ET_ERR_UNSUPPORTED.  A missing pointer: ET_ERR_INVALID_ARG.
 *
 * The network: a scene of n pedestrians is T n encoder tokens (token t n + a = frame t of pedestrian a), x =
 * fc(cat[input_fc(u[t, a]), pe[t]]); post-norm layers LN(x + attn(x)), LN(x + linear2(relu(linear1(x)))).  The decoder's
 * k-pass loop feeds the same input every pass under a block-causal mask, so ONE pass over k n tokens (token t n + a, input
 * u[T-1, a], positional row pe[t]) gives what its last pass gives; decoder layers add LN(x + cross-attn(x, memory))
 * between the two; out_fc maps D -> S.  Agent-aware scores: score(i, j) = q_self_i . k_self_j when i % n == j % n, else
 * q_i . k_j, both q scaled by head_dim^-0.5 after the bias; decoder self-attention masks keys of a later frame; softmax
 * over the scene's keys; cross-attention takes q, q_self from the decoder rows and k, v, k_self from the encoder output.
 *   et_agentformer_forward_graph   one scene as the bridge hands it over: pre_motion (T, N[, 1]) -> seq_out (k, N, S)
 *                                  (_dec_motion is its (N, k, S) transpose).  N <= ET_AGENTFORMER_MAX_SCENE_N.
 *   et_agentformer_forward_scenes  a whole split: C_obs (k, N), nrm (4, N) of et_norm_project; per scene u = [C_obs;
 *                                  nrm[0:2] - their mean over the scene], summed in et_scene_project's order (T = k + 2)
 *                                  -> C_pred_refine (k, N, S).  scene_offsets as et_implicit_forward_scenes (NULL = one
 *                                  scene of N <= ET_AGENTFORMER_MAX_SCENE_N rows; n_scenes = 0 takes N = 0 only).
 *                                  Optional output graph_inputs (k + 2, N) (may be NULL): the fp32 u used, scene s at
 *                                  columns [off[s], off[s+1]).  A scene of more than ET_AGENTFORMER_MAX_SCENE_N
 *                                  pedestrians (the reference's max_agent_len) is not computed: its outputs and its
 *                                  graph_inputs are NaN.
 * Launches: 2 + 2 n_enc + 4 n_dec whatever N and the number of scenes (14 for 2 + 2 layers; the graph form one fewer).
 * Workspace: et_agentformer_workspace_bytes(p, N_total, max_scene_n) bytes, linear in N_total (max_scene_n is accepted
 * for symmetry with the other predictors and does not change the size); 0 for N_total = 0 or parameters outside the
 * family.  No host synchronisation, no allocation: the calls can be captured in a graph.  Every reduction (softmax
 * maximum and sum, P V, LayerNorm mean and variance) has a fixed order that depends on the scene and the layer shape only:
 * a token's result does not depend on the scenes around it, the tile it landed in or the launch size. */
#define ET_AGENTFORMER_MAX_LAYERS 4
#define ET_AGENTFORMER_MAX_SCENE_N 128
typedef struct et_agentformer_attn {
    const float *in_proj_weight, *in_proj_bias;
    const float *in_proj_weight_self, *in_proj_bias_self;
    const float *out_proj_weight, *out_proj_bias;
} et_agentformer_attn;
typedef struct et_agentformer_layer {
    et_agentformer_attn self_attn, multihead_attn;
    const float *linear1_weight, *linear1_bias, *linear2_weight, *linear2_bias;
    const float *norm_weight[3], *norm_bias[3];
} et_agentformer_layer;
typedef struct et_agentformer_embed {
    const float *input_fc_weight, *input_fc_bias, *fc_weight, *fc_bias, *pe;
} et_agentformer_embed;
typedef struct et_agentformer_params {
    int motion_dim, model_dim, ff_dim, nhead, forecast_dim, past_frames, future_frames, n_enc, n_dec;
    et_agentformer_embed enc_embed, dec_embed;
    const float *out_fc_weight, *out_fc_bias;
    et_agentformer_layer enc[ET_AGENTFORMER_MAX_LAYERS], dec[ET_AGENTFORMER_MAX_LAYERS];
} et_agentformer_params;
size_t et_agentformer_workspace_bytes(const et_agentformer_params *params, int64_t N_total, int64_t max_scene_n);
int et_agentformer_forward_graph(const et_agentformer_params *params, const float *pre_motion, int64_t N, float *seq_out,
                                 void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_agentformer_forward_scenes(const et_agentformer_params *params, const float *C_obs, const float *nrm, int64_t N,
                                  const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *graph_inputs,
                                  void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- Graph-TERN predictor, inference (baseline/graphtern: bridge.py pre-hook + graph_tern_light.forward + post-hook) ----
 * Eval mode only (no drop_edge, no dropout); the network has no BatchNorm.  The parameters are read in place from the
 * module's own tensors through the pointer tables below (fp32, contiguous).  Field <-> state_dict name (i = st_mrgcn
 * block, j = epcnn block):
 *   tp_mrgcns[i].gcn_w / gcn_b      tp_mrgcns.{i}.gcn.conv.weight (64, C_in, 1, 1) / .bias (64): relation r on channel r 16 + c
 *   tp_mrgcns[i].tcn_prelu          tp_mrgcns.{i}.tcn.0.weight (1)
 *   tp_mrgcns[i].tcn_w / tcn_b      tp_mrgcns.{i}.tcn.1.weight (16, 16, 3, 1) / .bias (16)
 *   tp_mrgcns[i].res_w / res_b      tp_mrgcns.{i}.residual.0.weight (16, C_in, 1, 1) / .bias (16); NULL when C_in == 16
 *   tp_mrgcns[i].prelu              tp_mrgcns.{i}.prelu.weight (1): carried so that the table is complete; the network
 *                                   (use_mdn) never applies it and the kernel never reads it
 *   tpcnns[j].tpcn_w / tpcn_b       tpcnns.{j}.tpcns.0.0.weight (k, j == 0 ? T : k, 3, 3) / .bias (k)
 *   tpcnns[j].tpcn_a                tpcnns.{j}.tpcns.0.1.weight (1)
 *   tpcnns[j].cpcn_w / cpcn_b       tpcnns.{j}.cpcns.0.0.weight (C_out, 16, 3, 3) / .bias (C_out)
 *   tpcnns[j].cpcn_a                tpcnns.{j}.cpcns.0.1.weight (1)
 *   tpcnns[j].rest_w / rest_b       tpcnns.0.restconv.0.weight (k, T, 1, 1) / .bias (k); NULL for j > 0
 *   tpcnns[j].resc_w / resc_b       tpcnns.{n_epcnn-1}.rescconv.0.weight (S, 16, 1, 1) / .bias (S); NULL for the other
 *                                   blocks, and for the last one too when S == 16 (identity)
 * with T = seq_len, k = pred_seq_len, S = n_smpl, C_in = 1 in block 0 and 16 afterwards, C_out = S in the last epcnn block
 * and 16 before it.
 * Supported: input_feat = 1, hidden_feat = 16, seq_len = pred_seq_len + 2, 1 <= pred_seq_len <= ET_MAX_K, 1 <= n_smpl <= 64,
 * 1 <= n_epgcn <= ET_GRAPHTERN_MAX_EPGCN, 2 <= n_epcnn <= ET_GRAPHTERN_MAX_EPCNN; anything else: ET_ERR_UNSUPPORTED.  A
 * missing pointer (or a residual table that does not fit the shapes): ET_ERR_INVALID_ARG.
 *
 * The graphs (model.py:7-15): per time row four relations [A_abs, A_rel, 1 / A_abs, 1 / A_rel], A_abs[i,j] = |u[t,i] -
 * u[t,j]|, A_rel the same on rel (rel[0] = 0, rel[t] = u[t] - u[t-1]); an inverse is 0 where the distance is EXACTLY 0 (an
 * fp32 comparison of the fp32 distance, the reference's own decision, no tolerance band); per (r, t): D^-1/2 (A + I)
 * D^-1/2 with D = rowsum(A + I), in the reference's (D (A + I)) D order.  Division and square root are IEEE.  The epcnn
 * blocks' 3x3 convolutions pad by replication, clamped at the scene's own first and last pedestrian.
 *   et_graphtern_forward_graph   one scene as the bridge hands it over: S_obs (1,2,T,N,1) = [abs, rel], both read as given
 *                                -> out (1,k,N,S), the network's raw output.  N <= ET_SCENE_MAX_N.
 *   et_graphtern_forward_scenes  a whole split: C_obs (k,N), nrm (4,N) of et_norm_project; per scene u = [C_obs; nrm[0:2] -
 *                                their mean over the scene], summed in et_scene_project's order; rel, the distances and
 *                                their inverses are formed where they are used, the (4,T,n,n) stack is never stored ->
 *                                C_pred_refine (k,N,S).  scene_offsets as et_traj_metrics (NULL = one scene of N rows);
 *                                n_scenes = 0 takes N = 0 only.  Optional output graph_inputs (T,N) float (may be NULL):
 *                                the fp32 u the kernel used, scene s at columns [off[s], off[s+1]).  One launch.
 * Workspace: a scene whose activations fit a workgroup's LDS arena (at S = 20, k = 6: up to 35 pedestrians) needs none;
 * larger ones use workspace rows [off[s], off[s+1]) of et_graphtern_workspace_bytes(p, N, max_scene_n) bytes (0 when a
 * scene of max_scene_n pedestrians fits the arena).  A scene larger than ET_SCENE_MAX_N, or one that fits neither, is
 * not computed: its outputs are NaN.  No host synchronisation, no allocation: the calls can be captured in a graph.
 * Every sum has a fixed order: a scene's result does not depend on the scenes around it or on where its arena lies. */
#define ET_GRAPHTERN_MAX_EPGCN 4
#define ET_GRAPHTERN_MAX_EPCNN 8
typedef struct et_graphtern_layer {
    const float *gcn_w, *gcn_b;
    const float *tcn_prelu;
    const float *tcn_w, *tcn_b;
    const float *res_w, *res_b;
    const float *prelu;
} et_graphtern_layer;
typedef struct et_graphtern_epcnn {
    const float *tpcn_w, *tpcn_b, *tpcn_a;
    const float *cpcn_w, *cpcn_b, *cpcn_a;
    const float *rest_w, *rest_b;
    const float *resc_w, *resc_b;
} et_graphtern_epcnn;
typedef struct et_graphtern_params {
    int n_epgcn, n_epcnn, input_feat, hidden_feat, seq_len, pred_seq_len, n_smpl;
    et_graphtern_layer tp_mrgcns[ET_GRAPHTERN_MAX_EPGCN];
    et_graphtern_epcnn tpcnns[ET_GRAPHTERN_MAX_EPCNN];
} et_graphtern_params;
size_t et_graphtern_workspace_bytes(const et_graphtern_params *params, int64_t N, int64_t max_scene_n);
int et_graphtern_forward_graph(const et_graphtern_params *params, const float *S_obs, int64_t N, float *out,
                               void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_graphtern_forward_scenes(const et_graphtern_params *params, const float *C_obs, const float *nrm, int64_t N,
                                const int32_t *scene_offsets, int n_scenes, float *C_pred_refine, float *graph_inputs,
                                void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- Graph-TERN predictor, training (graph_tern_light.forward in training mode + its backward pass) -------------------
 * The training-mode forward is NOT the eval forward: MultiRelationalGCN applies drop_edge(A, 0.8) (stmrgcn.py:22) to the
 * float tensor A (1,4,T,N,N) = [A_abs, A_rel, 1/A_abs, 1/A_rel] before + I and before the normalisation, one draw per
 * st_mrgcn block.  The draw is the caller's: `keep`, uint8, (4,T,N,N) indexed [r,t,w,v] (graph form), entry != 0 keeps
 * A_r[w,v]; scenes form: scene s's own (4,T,n,n) block starts at 4 T keep_offsets[s], keep_offsets (device, n_scenes + 1
 * int64_t) the running sum of n^2 over the scenes (a scene above the cap takes no room); keep = NULL keeps everything.
 * s[r,t,w] = sum_v (keep ? A_r[w,v] : 0) + [v==w], d = 1/sqrt(s) with inf set to 0, L[r,t,w,v] = (d_w ((keep ? A_r[w,v] :
 * 0) + [v==w])) d_v with d_v the column pedestrian's own row degree: the degrees change with the mask and L is no longer
 * symmetric.  A's diagonal is exactly 0, so the mask's diagonal has no effect.  Every other statement is
 * et_graphtern_forward_*'s in its order, so with keep = NULL or all ones the output is bit-equal to the inference entry's.
 * Trained natively: the inference family with n_epgcn = 1 (the only depth ET builds; a deeper stack needs a gradient
 * through the contraction, L^T: ET_ERR_UNSUPPORTED) and scenes of at most ET_GRAPHTERN_TRAIN_MAX_N pedestrians (a larger
 * scene of the scenes form is not computed: NaN outputs, no gradient; graph form: ET_ERR_INVALID_ARG).  The graphs are
 * detached by the reference (model.py:244) and the bridge detaches the input: no gradient passes through a graph.
 *   et_graphtern_train_workspace_bytes  the training workspace for N pedestrians in n_scenes scenes (graph form: 1): what
 *                                       the forward keeps, the activation gradients, an arena for scenes that do not fit
 *                                       LDS and the scenes' gradient partials.  0: outside the family, N <= 0 or
 *                                       n_scenes < 1.
 *   et_graphtern_train_forward_graph /  arguments as et_graphtern_forward_graph / _scenes (no graph_inputs) plus the mask.
 *   et_graphtern_train_forward_scenes   ONE launch, one workgroup per scene, the live operands in the LDS arena when the
 *                                       scene fits it (at S = 20, k = 6: up to 35 pedestrians), else in the workspace's
 *                                       arena rows.
 *   et_graphtern_backward_graph /       d_out laid out as the forward's output ((1,k,N,S) / (k,N,S)) and the workspace as
 *   et_graphtern_backward_scenes        that forward left it (same parameters, N, scene_offsets) -> grads, grads_floats >=
 *                                       et_graphtern_grad_floats floats: every parameter's gradient in state_dict order
 *                                       (tp_mrgcns.0: prelu.weight, gcn.conv.weight, .bias, tcn.0.weight, tcn.1.weight,
 *                                       .bias, residual.0.weight, .bias; tpcnns.j: tpcns.0.0.weight, .bias, tpcns.0.1.weight,
 *                                       cpcns.0.0.weight, .bias, cpcns.0.1.weight, [rescconv.0.weight, .bias,]
 *                                       [restconv.0.weight, .bias]).  tp_mrgcns.0.prelu.weight is never applied by the
 *                                       forward: its slot is always +0 (torch leaves its .grad None).  THREE launches for
 *                                       any N and any number of scenes: the activation gradients (one workgroup per scene,
 *                                       the dependent chain in the arena), the parameter gradients (16 workgroups per
 *                                       scene: every element is one wavefront's sum, the scene's 64 wavefronts take them
 *                                       round robin), the reduction.
 * The transposed 3x3 convolutions under replicate padding are gathers: an input cell sums the outputs whose clamped taps
 * land on it, in a fixed order; the convolution weight gradients read the input through the same clamps.
 * No gradient with respect to the input.  No atomics: a gradient element of a scene is one wavefront's sum over the
 * element's positions (lane l adds positions l, l + 64, ... in ascending order, then the lanes by the xor butterfly 32, 16,
 * ..., 1), and the scenes' partials are added in ascending order, the first one copied; results are bit-identical from run
 * to run, and a one-scene scenes call equals the graph call.  Host-side checks answer ET_ERR_UNSUPPORTED /
 * ET_ERR_INVALID_ARG / ET_ERR_WORKSPACE before any launch. */
#define ET_GRAPHTERN_TRAIN_MAX_N 512
size_t et_graphtern_train_workspace_bytes(const et_graphtern_params *params, int64_t N, int n_scenes);
int64_t et_graphtern_grad_floats(const et_graphtern_params *params);
/* where the training workspace keeps what (host only, no launch), in floats.  Per-pedestrian fields first (scene s's block
 * starts at off[s] x [10]; field f of it at + offsets[f] x the scene's n): [0] u (T,n), [1] d (4,T,n) the D^-1/2 of the
 * masked graphs, [2] P (4,2,T,n) the contracted rows (j = 0 from u, j = 1 from the ones row), [3] yp (16,T,n) the tcn
 * PReLU's input, [4] x0 (T,16,n) the st_mrgcn block's output, [5] per epcnn block j at + j x [11]: c0, y (k,16,n each:
 * tpcns.0's pre-activation and output), then c1, o (k,C,n each with C = max(16, S) floats of room, (k,C_out,n) used:
 * cpcns.0's pre-activation, the block's output); block j's input is x0 (j = 0) or block j-1's o, [6] per epcnn block at +
 * j x [12]: do (room (k,C,n), used (k,C_out,n)) the gradient at the block's output, dy (k,16,n) the gradient at y, [7] dx0
 * (T,16,n), [8] dy (16,T,n) the gradient at PReLU(yp), [9] the arena; [10] floats per pedestrian; [13] the scenes'
 * gradient partials, [14] = et_graphtern_grad_floats each; [15] the total. */
#define ET_GRAPHTERN_TRAIN_LAYOUT_FIELDS 16
int et_graphtern_train_layout(const et_graphtern_params *params, int64_t N, int n_scenes, int64_t *offsets, int n_offsets);
int et_graphtern_train_forward_graph(const et_graphtern_params *params, const float *S_obs, int64_t N, const uint8_t *keep,
                                     float *out, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_graphtern_train_forward_scenes(const et_graphtern_params *params, const float *C_obs, const float *nrm, int64_t N,
                                      const int32_t *scene_offsets, int n_scenes, const uint8_t *keep,
                                      const int64_t *keep_offsets, float *C_pred_refine, void *workspace,
                                      size_t workspace_bytes, et_stream_t stream);
int et_graphtern_backward_graph(const et_graphtern_params *params, int64_t N, const float *d_out, float *grads,
                                int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream);
int et_graphtern_backward_scenes(const et_graphtern_params *params, int64_t N, const int32_t *scene_offsets, int n_scenes,
                                 const float *d_out, float *grads, int64_t grads_floats, void *workspace,
                                 size_t workspace_bytes, et_stream_t stream);

/* ---- fit ----------------------------------------------------------------------------
 * Gram matrices of the normalised trajectories routed to descriptor `which`
 * (1 moving / 0 static) under `mode`:  G_obs (2T_obs,2T_obs), G_pred (2T_pred,2T_pred)
 * fp64, full symmetric; *count = rows used (int64, device).  A data-sharded fit sums
 * G_obs, G_pred and count over ranks (RCCL all-reduce) before et_eigh_topk. */
size_t et_fit_gram_workspace_bytes(int64_t N, int T_obs, int T_pred);
int et_fit_gram(const float *obs, const float *pred, int64_t N, int T_obs, int T_pred,
                int mode, float static_dist, int which,
                double *G_obs, double *G_pred, int64_t *count,
                void *workspace, size_t workspace_bytes, et_stream_t stream);

/* The fit of ONE descriptor in a single call (descriptor.py:116-142 parameter_initialization = normalise -> SVD of the obs
 * rows + SVD of the pred rows): et_fit_gram followed by the eigensolve of both matrices, the matrix assembly folded into
 * the eigensolver's launch (three launches in all).  U_obs (2T_obs,k), U_pred (2T_pred,k),
 * sigma_obs / sigma_pred (k) as et_eigh_topk writes them; G_obs, G_pred, count: optional outputs (may be NULL), the same
 * bits et_fit_gram returns.  Any (T_obs, T_pred) and N = 0 are accepted (they run the two calls one after the other). */
size_t et_fit_descriptor_workspace_bytes(int64_t N, int T_obs, int T_pred);
int et_fit_descriptor(const float *obs, const float *pred, int64_t N, int T_obs, int T_pred, int k,
                      int mode, float static_dist, int which,
                      float *U_obs, float *U_pred, float *sigma_obs, float *sigma_pred,
                      double *G_obs, double *G_pred, int64_t *count,
                      void *workspace, size_t workspace_bytes, et_stream_t stream);

/* Top-k eigenpairs of a symmetric n x n fp64 matrix (n <= 64), parallel-order (round-robin) Jacobi in one
 * workgroup: U (n,k) fp32 = eigenvectors by descending eigenvalue, each signed so its
 * largest-|.| component is positive; sigma[k] = sqrt(max(lambda,0)) -- U[:, :k], S[:k]
 * of torch.linalg.svd at descriptor.py:110-113 up to sign. */
int et_eigh_topk(const double *G, int n, int k, float *U, float *sigma, et_stream_t stream);

/* The same for `batch` (<= ET_EIGH_MAX_BATCH) independent matrices in ONE launch, one workgroup each:
 * G[i] (n[i] x n[i]) -> U[i] (n[i], k[i]), sigma[i] (k[i]).  The arrays themselves are host memory, the
 * matrices and outputs device memory.  A fit solves its obs / pred (x moving / static) Gram matrices
 * side by side this way (the reference runs its torch.linalg.svd calls one after the other,
 * model.py:50-52). */
#define ET_EIGH_MAX_BATCH 8
int et_eigh_topk_batch(int batch, const double *const *G, const int *n, const int *k, float *const *U,
                       float *const *sigma, et_stream_t stream);

/* ---- BatchKMeans ----------------------------------------------------------------------
 * X (d,N) d-major points (= C_pred (k,N)); centroids (d,K); labels int64 (N).
 * Similarity is kmeans.py:71-74 in the reference's operation order; the argmax takes
 * the first maximum and lets NaN win (torch.max).  Per-cluster sums are exact 64-bit
 * fixed-point integers (state.frac fractional bits), hence identical for any
 * partition of the points over workgroups or GPUs. */
typedef struct et_kmeans_state {
    double max_abs_x;   /* max |x| over ALL shards (all-reduce MAX before et_kmeans_begin) */
    double max_abs_c;   /* max |centroid| of the current centroids (NaN ignored)           */
    int64_t n_total;    /* number of points over all shards                                */
    int64_t frac;       /* fractional bits of the coordinate accumulators                   */
    int64_t sim_frac;   /* fractional bits of the similarity (inertia) accumulator          */
    int64_t iter;       /* Lloyd iterations executed                                       */
    int64_t done;       /* 1 once error <= tol (kmeans.py:239); later steps are no-ops     */
    int64_t bad_input;  /* 1 if X holds NaN/Inf (all-reduce MAX)                           */
    double error;       /* kmeans.py:45-51 of the last update                              */
    double inertia;     /* kmeans.py:53-57 of the last assignment                          */
    int64_t fast_ok;    /* 0/1/2: which arg-max kernel the next assignment may use          */
    int64_t min_nz_x_bits; /* fp32 bit pattern of the smallest non-zero |x| (all-reduce MIN) */
} et_kmeans_state;

/* kmeans.py:59-76 euc_sim for one batch element: a (d,m), b (d,n) -> y (m,n) */
int et_euc_sim(const float *a, const float *b, int d, int64_t m, int64_t n, float *y, et_stream_t stream);
/* ... and for the reference's leading batch dimensions in one launch: contiguous a (B,d,m), b (B,d,n) -> y (B,m,n) */
int et_euc_sim_batch(const float *a, const float *b, int64_t batch, int d, int64_t m, int64_t n, float *y,
                     et_stream_t stream);

/* number of int64 in a partials block: d*K sums (d-major), K counts, sim_sum, nan_count */
size_t et_kmeans_partials_len(int d, int K);
/* scratch of every k-means call on a shard of N points: ~5 B per point (labels, running best similarity) + O(d K); for
 * d = 6, 3 <= K <= 32, N >= 131072 (2^17) and N % 4 == 0 another 46 B per point: the packed copy of the points that the trace-less
 * Lloyd iterations of et_kmeans_fit / et_kmeans_fit_sharded read instead of X (csrc/et_kmeans.hip: kmeans_pack_kernel) */
size_t et_kmeans_workspace_bytes(int64_t N, int d, int K);

/* max |x| and non-finite flag of this shard -> state->max_abs_x, state->bad_input
 * (the rest of *state is zeroed). */
int et_kmeans_scan(const float *X, int64_t N, int d, et_kmeans_state *state, et_stream_t stream);
/* fix frac / sim_frac from the (all-reduced) max_abs_x, n_total and the initial centroids
 * (d,K); reset iter/done (done = 1 straight away when bad_input is set). */
int et_kmeans_begin(et_kmeans_state *state, int64_t n_total, const float *centroids, int d, int K,
                    et_stream_t stream);

/* ABI limit: the farthest-first keys and the filter kernel's queue carry 32-bit GLOBAL point indices, so the number
 * of points over all shards of one k-means problem must be < 2^32 (checked: ET_ERR_INVALID_ARG).
 * farthest-first initialisation (kmeans.py:78-112).  best (N) fp32 scratch.
 *   step i (1 <= i < K): similarity of every local point to centroid column i-1 of C0,
 *   running max into best, local arg-min -> cand: {uint64 key, d floats} where
 *   key = orderable(best) << 32 | (index_base + local index); smaller key wins and a
 *   sharded run picks the minimum key over ranks.  cand must hold 8 + 4*d bytes.
 * et_kmeans_init_set copies a point (device, d floats) into column `col` of C0 (d,K). */
int et_kmeans_init_step(const float *X, int64_t N, int d, int K, int i, const float *C0, float *best,
                        int64_t index_base, void *cand, void *workspace, size_t workspace_bytes,
                        et_stream_t stream);
int et_kmeans_init_set(float *C0, int d, int K, int col, const float *point, et_stream_t stream);
/* sharded step, after the all-gather of the ranks' candidate records (n_cands records, stride_bytes apart,
 * 8-byte aligned): the record with the smallest key becomes column `col` of C0 -- the same on every rank. */
int et_kmeans_init_select(const void *cands, int n_cands, int stride_bytes, int d, int K, int col, float *C0,
                          et_stream_t stream);
/* gather X[:, local_index] -> point (d floats, device) */
int et_kmeans_gather_point(const float *X, int64_t N, int d, int64_t local_index, float *point,
                           et_stream_t stream);
/* single-GPU convenience: the whole initialisation, first centroid = X[:, first_index] */
int et_kmeans_init_farthest(const float *X, int64_t N, int d, int K, int64_t first_index, float *C0,
                            void *workspace, size_t workspace_bytes, et_stream_t stream);

/* one Lloyd half-step on a shard (kmeans.py:230 + the sums of :231, :234): labels_u8 (N)
 * and this shard's exact partials; no-op when state->done.  From the second iteration on only
 * the points whose label changed update the sums (exact integer deltas) -- for d = 6, K <= 32 a
 * matrix-core filter first proves, per point, that the label cannot change (bit-identical results) --
 * so `labels_u8` and `workspace` (which holds the running totals) must be the buffers of the previous
 * iteration of the same fit, unmodified; `partials` receives a copy of the totals and is the caller's to
 * overwrite (e.g. all-reduce in place).  With given_labels != NULL (int64, N) the labels are taken as they are instead of
 * computed (compute_centroids, kmeans.py:160-198, as a public method). */
int et_kmeans_assign_accumulate(const float *X, int64_t N, int d, int K, const et_kmeans_state *state,
                                const float *centroids, const int64_t *given_labels, uint8_t *labels_u8,
                                int64_t *partials, void *workspace, size_t workspace_bytes, et_stream_t stream);
/* centroid update + error/inertia/convergence from (all-reduced) partials
 * (kmeans.py:180-182, 45-57, 239).  centroids updated in place; trace (max_iter,2) fp32
 * receives (error, inertia) at row state->iter when not NULL. */
int et_kmeans_update(et_kmeans_state *state, const int64_t *partials, int d, int K, float tol,
                     float *centroids, float *trace, et_stream_t stream);
/* BatchKMeans.fit with l > 1 problems stops them TOGETHER, on the sum of their errors (kmeans.py:228-240: `error` is one
 * sum over the (l, d, K) centroid tensors).  Step-API driver: run et_kmeans_update of every problem with a negative
 * tolerance (no error meets it), then this: states = device array of the n_problems state-block pointers; sets every
 * state's `done` to (sum of the states' errors <= tol).  Later steps of all problems are then no-ops. */
int et_kmeans_joint_done(et_kmeans_state *const *states, int n_problems, float tol, et_stream_t stream);
/* widen the uint8 labels of the last assignment to the reference's int64 */
int et_kmeans_labels_i64(const uint8_t *labels_u8, int64_t N, int64_t *labels, et_stream_t stream);

/* optional kernel timing of et_kmeans_fit: HIP events recorded on `stream` around the dominant kernel of the path.
 * Default (all iterations of the fit in ONE persistent launch, kmeans_lloyd_persist_kernel): the duration of that
 * launch, assign_launches = 1, iterations = the Lloyd iterations it ran.  One launch per iteration (ET_KMEANS_LOOP=chain,
 * shapes the persistent kernel does not take): a sample of the launches -- the first one separately, then of every eight
 * launches a run of four between one pair of events (an event record between two kernels costs a dispatch gap on both
 * sides; assign_launches counts the launches inside the pairs).  Filled after the final sync. */
typedef struct et_kmeans_timing {
    double assign_ms;        /* summed duration of the timed launches                                                 */
    int64_t assign_launches; /* number of launches in assign_ms                                                       */
    double first_assign_ms;  /* per-iteration form only: launch 0 (plain exact scan + full accumulation), else 0      */
    int64_t iterations;      /* Lloyd iterations (24 B of coordinates per point each) that assign_ms covers           */
} et_kmeans_timing;

/* single-GPU fit of one batch element from given initial centroids (kmeans.py:228-240):
 * centroids (d,K) in/out, labels int64 (N) out (NULL: not wanted), trace (max_iter,2) fp32 (error, inertia) per iteration or NULL:
 * without a trace the per-iteration inertia is not evaluated (the reference only prints it, kmeans.py:236) and
 * state.inertia -- the inertia of the last assignment -- comes from one extra pass after the loop (same bits).
 * *state_host receives the final state,
 * *timing_host (may be NULL) the assign-kernel timing.  Synchronises the stream once, at the
 * end (the reference syncs every iteration at kmeans.py:239; here the convergence flag is polled
 * without blocking, a few iterations behind the launches). */
int et_kmeans_fit(const float *X, int64_t N, int d, int K, int max_iter, float tol, float *centroids,
                  int64_t *labels, float *trace, et_kmeans_state *state_host, et_kmeans_timing *timing_host,
                  void *workspace, size_t workspace_bytes, et_stream_t stream);

/* `batch` independent fits in one call (each stops on its own error, unlike BatchKMeans' joint stop): the n_init
 * initialisations of the reference's sklearn anchor clustering (anchor.py:65-71).  X: problem b's points at X + b *
 * x_stride floats (x_stride = 0: all problems cluster the same points); centroids (batch,d,K) in/out; labels
 * (batch,N) int64 or NULL; states_host[batch].  For d = 6, 3 <= K <= 32 and shards that leave room for at least two
 * problems on the device the problems run side by side as the y dimension of ONE persistent launch
 * (csrc/et_kmeans.hip), in chunks when they do not all fit; any other shape: one et_kmeans_fit after the other.
 * workspace: et_kmeans_batch_workspace_bytes (= batch x et_kmeans_workspace_bytes).  Synchronises the stream. */
size_t et_kmeans_batch_workspace_bytes(int64_t N, int d, int K, int64_t batch);
int et_kmeans_fit_batch(const float *X, int64_t x_stride, int64_t N, int d, int K, int64_t batch, int max_iter, float tol,
                        float *centroids, int64_t *labels, et_kmeans_state *states_host, void *workspace,
                        size_t workspace_bytes, et_stream_t stream);

/* ---- opt-in: BatchKMeans in the REFERENCE's own fp32 summation orders (csrc/et_kmeans_reforder.hip) ----------
 * et_kmeans_fit sums the per-cluster coordinates exactly, which makes the result independent of launch geometry and GPU
 * count but lets a whole run drift away from the reference's (kmeans.py:180-182 sums fp32 in ATen's cascade order; whole-run
 * label equality with the imported reference: 96/96 runs here against 76/96 with exact sums).  These entry
 * points restate ATen's CPU orders for kmeans.py:73-74 (norms), :180-182 (cluster sums) and :45-51 (error) literally.
 * Single GPU, any d <= 32, K <= 255.  d = 6, K <= 32, 1024 <= N < 2^29 (the anchor clustering's shape): ONE launch per
 * Lloyd iteration -- ATen's cascade is a fixed tree over index ranges, so its levels are evaluated in parallel without
 * changing an addition (level 0: one work item per chunk lane and coordinate; level 1: inside a workgroup; levels 2, 3,
 * the centroid update and the stop flag: by the workgroups that arrive last) --, no host synchronisation inside the loop.
 * Any other shape: plain kernels, serial where the reference's order is serial, one synchronisation per iteration.
 * workspace: et_kmeans_reforder_workspace_bytes (~ 25 B per point for the fast form's permuted copy). */
size_t et_kmeans_reforder_workspace_bytes(int64_t N, int d, int K);
/* kmeans.py:59-76 with both norms in torch's order: every bit of the reference's euc_sim. a (d,m), b (d,n) -> y (m,n) */
int et_euc_sim_reforder(const float *a, const float *b, int d, int64_t m, int64_t n, float *y, et_stream_t stream);
/* kmeans.py:78-112, re-evaluating euc_sim against all current centroids at every step like the reference */
int et_kmeans_init_farthest_reforder(const float *X, int64_t N, int d, int K, int64_t first_index, float *C0,
                                     void *workspace, size_t workspace_bytes, et_stream_t stream);
/* kmeans.py:143-158 get_labels: labels int64 (N), maxsims (N) (either may be NULL) */
int et_kmeans_predict_reforder(const float *X, int64_t N, int d, const float *centroids, int K, int64_t *labels,
                               float *maxsims, void *workspace, size_t workspace_bytes, et_stream_t stream);
/* kmeans.py:228-240 from given initial centroids: centroids (d,K) in/out, labels int64 (N) or NULL, trace (max_iter,2) or
 * NULL, *state_host: iter, done, error, inertia (the inertia is this build's fp64 sum: the reference only prints it).
 * The fast form synchronises the stream once, at the end; the plain kernels every iteration (kmeans.py:239). */
int et_kmeans_fit_reforder(const float *X, int64_t N, int d, int K, int max_iter, float tol, float *centroids,
                           int64_t *labels, float *trace, et_kmeans_state *state_host, void *workspace,
                           size_t workspace_bytes, et_stream_t stream);
/* BatchKMeans.fit's own loop for `batch` (= l) problems (kmeans.py:228-240): all problems iterate together and stop
 * TOGETHER on the error summed over the whole contiguous (l, d, K) centroid tensor in ATen's inner-sum order.  X: problem
 * b's points at X + b * x_stride floats; centroids (batch, d, K) in/out; labels (batch, N) int64 or NULL; trace (batch,
 * max_iter, 2) or NULL (row = joint error, this problem's inertia); states_host[batch]; *timing_host (may be NULL):
 * assign_ms = the whole loop between two events, assign_launches = launches enqueued.  batch > 1 takes the fast form's
 * shapes only (d = 6, K <= 32, 1024 <= N < 2^29, batch <= 64; the workspace query returns 0 otherwise). */
size_t et_kmeans_reforder_batch_workspace_bytes(int64_t N, int d, int K, int64_t batch);
int et_kmeans_fit_reforder_batch(const float *X, int64_t x_stride, int64_t N, int d, int K, int64_t batch, int max_iter,
                                 float tol, float *centroids, int64_t *labels, float *trace, et_kmeans_state *states_host,
                                 et_kmeans_timing *timing_host, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* kmeans.py:261-272 predict: labels int64 (N); maxsims (N) optional */
int et_kmeans_predict(const float *X, int64_t N, int d, const float *centroids, int K, int64_t *labels,
                      float *maxsims, et_stream_t stream);
/* kmeans.py:143-158 get_labels on a batch in one launch: element b's points at X + b * x_stride floats (d N for a
 * contiguous (B,d,N) tensor, 0: the same points for every element), centroids (B,d,K) -> labels / maxsims (B,N) */
int et_kmeans_predict_batch(const float *X, int64_t x_stride, int64_t batch, int64_t N, int d, const float *centroids,
                            int K, int64_t *labels, float *maxsims, et_stream_t stream);

/* ---- anchor clustering as the reference runs it: sklearn KMeans(init='k-means++', n_init=10) ----------
 * EigenTrajectory/anchor.py:65-71 hands the coefficients to sklearn.cluster.KMeans (third-party; its published
 * algorithm is restated, see csrc/et_kmeanspp.hip).  The Lloyd iterations are et_kmeans_fit; these two entry
 * points are the parts sklearn does around them, in the arithmetic of its float32 code path.
 *
 * et_center_columns   KMeans.fit's pre-processing, in place on X (d,N): mean[j] = fp32 sum over the points in
 *                     index order / N (numpy's add.reduce(axis=0) order), X[j] -= mean[j], and
 *                     *tol = rel_tol * mean_j(var_j) (sklearn `_tolerance`).  mean (d), tol (1): device.
 *                     workspace >= 2 * 4 * ET_KMEANS_MAX_D bytes.
 * et_kmeanspp_seed    greedy k-means++ (n_trials = 2 + floor(ln K) candidates per centre): centers (d,K) fp32 and
 *                     indices (K) int64 of the chosen points.  `uniforms` (device, float64) holds the
 *                     1 + (K-1)*n_trials draws of the seeding in the order sklearn consumes its RandomState:
 *                     [0] picks the first centre (index floor(u*N)), then n_trials thresholds per centre.
 *                     Enqueues 4K-1 launches, no synchronisation. */
int et_center_columns(float *X, int64_t N, int d, float rel_tol, float *mean, float *tol,
                      void *workspace, size_t workspace_bytes, et_stream_t stream);
size_t et_kmeanspp_workspace_bytes(int64_t N, int d, int n_trials);
int et_kmeanspp_seed(const float *X, int64_t N, int d, int K, int n_trials, const double *uniforms,
                     float *centers, int64_t *indices, void *workspace, size_t workspace_bytes, et_stream_t stream);
/* `batch` seedings of the SAME points side by side (the n_init initialisations), as the y dimension of the same 4K-1
 * launches: uniforms (batch, 1+(K-1)*n_trials), centers (batch,d,K), indices (batch,K);
 * workspace = batch x et_kmeanspp_workspace_bytes. */
size_t et_kmeanspp_batch_workspace_bytes(int64_t N, int d, int n_trials, int64_t batch);
int et_kmeanspp_seed_batch(const float *X, int64_t N, int d, int K, int n_trials, const double *uniforms, int64_t batch,
                           float *centers, int64_t *indices, void *workspace, size_t workspace_bytes, et_stream_t stream);

/* ---- data-sharded fit and k-means: one process per GPU, RCCL over xGMI (csrc/et_sharded.hip) ------------------------
 * The reference has no distributed code; these are the entry points of SURVEY.md §8(b) "with an optional
 * ncclComm_t for the sharded variants".  `comm` is an ncclComm_t -- the caller's own, or one made with et_comm_* below
 * (ncclGetUniqueId on rank 0, the 128 bytes handed to the other ranks by any side channel, ncclCommInitRank everywhere).
 * RCCL is bound at run time with dlopen: an RCCL the process has already mapped (PyTorch's) is reused, otherwise
 * librccl.so.1 is searched; et_comm_load(path) forces a specific library.  Every rank must make the same calls in the
 * same order; all collectives are enqueued on `stream` (a few KB each, latency-bound).  comm == NULL: single shard. */
#define ET_COMM_UNIQUE_ID_BYTES 128
int et_comm_load(const char *librccl_path_or_null);
int et_comm_unique_id(void *id128_host);
int et_comm_init_rank(const void *id128_host, int nranks, int rank, et_comm_t *comm); /* on the CURRENT device */
int et_comm_destroy(et_comm_t comm);
int et_comm_info(et_comm_t comm, int *nranks, int *rank);

/* et_fit_gram over all ranks' rows: the local pass + one grouped all-reduce(SUM) of G_obs, G_pred (fp64) and count. */
int et_fit_gram_sharded(const float *obs, const float *pred, int64_t N_local, int T_obs, int T_pred,
                        int mode, float static_dist, int which,
                        double *G_obs, double *G_pred, int64_t *count,
                        void *workspace, size_t workspace_bytes, et_comm_t comm, et_stream_t stream);

/* workspace of the two calls below (>= et_kmeans_workspace_bytes + the gathered candidate records) */
size_t et_kmeans_sharded_workspace_bytes(int64_t N_local, int d, int K, int nranks);
/* farthest-first initialisation over all ranks' points (kmeans.py:78-112): C0 (d,K) identical on every rank.
 * first_index is GLOBAL; this rank's points are the global indices [index_base, index_base + N_local); best (N_local)
 * fp32 scratch.  One all-gather of an (8 + 4d)-byte record per rank and new centroid. */
int et_kmeans_init_farthest_sharded(const float *X, int64_t N_local, int d, int K, int64_t first_index,
                                    int64_t index_base, float *C0, float *best,
                                    void *workspace, size_t workspace_bytes, et_comm_t comm, et_stream_t stream);
/* Lloyd iterations over all ranks' points from given centroids (identical on every rank; updated in place):
 * per iteration ONE kernel launch (the previous iteration's update in its prologue, then the assignment) and ONE
 * in-place all-reduce(SUM) of the exact int64 delta table (16 (d K + K + 2) values, 18 KB for d = 6, K = 20), all on
 * `stream`, no host round trip inside the loop (the convergence flag is looked at a few iterations late, on the same
 * copy on every rank).  Shards that form does not take (d != 6, K > 32, N_local < 1024 or not a multiple of 4 on ANY
 * rank -- decided together, one all-reduce(MIN) and one stream synchronisation before the loop) run assignment kernels,
 * an all-reduce of d K + K + 2 values and an update kernel instead.  state / labels_u8 (N_local + 3) / partials
 * (et_kmeans_partials_len) are caller-owned device buffers; labels (N_local) int64 may be NULL.  Synchronises the
 * stream at the end; *state_host receives the final state. */
int et_kmeans_fit_sharded(const float *X, int64_t N_local, int64_t N_total, int d, int K, int max_iter, float tol,
                          float *centroids, int64_t *labels, float *trace,
                          et_kmeans_state *state, uint8_t *labels_u8, int64_t *partials,
                          et_kmeans_state *state_host, void *workspace, size_t workspace_bytes,
                          et_comm_t comm, et_stream_t stream);

/* The REFERENCE-ORDER Lloyd iterations (et_kmeans_fit_reforder above) over shards, d = 6, K <= 32, 1024 <= N_total < 2^29.
 * The order of ATen's cascade sum is a property of the whole array, but its tree is made of index ranges: rank r holds the
 * points [sum of n_locals[0..r), + n_locals[r]) and every rank before the last non-empty one holds a whole number of
 * level-2 blocks (n_locals[r] a multiple of et_kmeans_reforder_shard_block(N_total, d, K) = 4 L^3 points, L the level
 * step of N_total: 16 384 / 131 072 / 1 048 576 points for L = 16 / 32 / 64; zero is a multiple); ranks after it are empty.  Each rank runs
 * levels 0 .. 2 over its own blocks; per iteration ONE all-gather of a record per rank (a row of d K sums + K counts per
 * block, the end of the array's partial sums) and the same sequential level 3 on every rank: centroids, labels, error and
 * iteration count equal et_kmeans_fit_reforder on the whole array bit for bit (inertia: to fp32 rounding).  n_locals is a
 * HOST array of nranks sizes, identical on every rank; labels (n_locals[rank]) int64 or NULL; *state_host the final
 * state.  comm == NULL: nranks must be 1.  Anything else than the shapes above: ET_ERR_UNSUPPORTED / ET_ERR_INVALID_ARG. */
#define ET_REFORDER_MAX_RANKS 64
int64_t et_kmeans_reforder_shard_block(int64_t N_total, int d, int K); /* 0: shape not taken */
size_t et_kmeans_reforder_sharded_workspace_bytes(const int64_t *n_locals, int nranks, int rank, int d, int K);
int et_kmeans_fit_reforder_sharded(const float *X, const int64_t *n_locals, int nranks, int rank, int d, int K, int max_iter,
                                   float tol, float *centroids, int64_t *labels, float *trace,
                                   et_kmeans_state *state_host, void *workspace, size_t workspace_bytes,
                                   et_comm_t comm, et_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EIGENTRAJ_H */

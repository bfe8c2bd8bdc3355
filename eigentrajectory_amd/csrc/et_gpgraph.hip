// et_gpgraph.hip -- GP-Graph-SGCN inference (baseline/gpgraphsgcn: bridge.py pre-hook, model_groupwrapper.py GPGraph.forward
// around model_baseline.py's two-channel SGCN in eval mode with dropout 0, bridge.py post-hook) for the ET configuration
// (include/eigentraj.h "GP-Graph-SGCN predictor").
//
// GP-Graph runs the SAME SGCN three times with shared weights -- on the pedestrian graph, on the graph of group means and
// on the pedestrian graph with the spatial mask cut down to pairs of one group -- so the three graphs of S scenes are 3 S
// virtual scenes of ONE run of the layered kernels of et_sgcn_core.inl (their GP = true instantiations).  Per call, for any
// number of scenes, 8 + number_asymmetric_conv_layer launches:
//   prep    1 workgroup     the two attentions collapsed: 2 coefficients per head for the spatial one, 6 for the temporal
//   group   per scene       conv features of v_abs, the n x n distance matrix (workspace), the decisions d <= th, the
//                           reference's merge, compact labels, group sizes, sig / sig.sum(0), v' = (v_rel - v_soft) + v_soft,
//                           the group means; the three virtual scenes' inputs, node counts and stack offsets
//   input, fuse, asym x layers, tadj, sadj, tail   et_sgcn_core.inl on the 3 S virtual scenes -> (k, 3 N, S) in the workspace
//   mix     per pedestrian  unpool by gather, mean of the three, PReLU, the (S k) x (3 S k) product, -> (k, N, S)
// The group steps and the mix kernel are et_gpgraph_core.inl, shared with et_gpgraph_stgcnn.hip.
// The merge.  The reference walks the close pairs (r, c), c < r, in row-major order and gives every pedestrian that carries
// r's label the label c -- c itself, not c's label, so the result is NOT the connected components.  Within row r with close
// columns c1 < .. < cm the walk moves label[r]'s carriers to c1, then c1's carriers (those included) to c2, ..: at the end
// every pedestrian whose label was in {label[r], c1, .., c(m-1)} carries cm.  That is one parallel step per row, n serial
// steps per scene (rows without a close column are skipped without a barrier).
// Every sum runs in a fixed order inside one lane, so results are bit-identical from run to run and a scene's result does
// not depend on the scenes around it.  Training (the kept-layout forward and the backward pass to every parameter of the
// wrapper and of the base) is et_gpgraph_train.inl, on the base's backward of et_sgcn_train.inl.
#include "et_common.h"

namespace et {
namespace {

#include "et_sgcn_core.inl"

#include "et_gpgraph_core.inl"

struct WLay {  // the workspace behind the base's (floats): v_abs (T,N), conv features (8,T,N), dist and sig_norm (sum n^2),
    int64_t va, feat, dist, sn, po, total;  // the base's output for the 3 N virtual rows (k, 3 N, S)
};

struct GpKeep {  // where the training forward keeps sig (sum n^2), its column sums (N) and the group sizes (int32 N); -1: not kept
    int64_t sig, cs, cnt;
};

__host__ __device__ inline WLay wlay_of(const Lay &L, int T, int k, int S, int64_t N, int64_t n2) {
    WLay G;
    G.va = L.total;
    G.feat = up4(G.va + T * N);
    G.dist = up4(G.feat + (int64_t)kGpHid * T * N);
    G.sn = up4(G.dist + n2);
    G.po = up4(G.sn + n2);
    G.total = up4(G.po + (int64_t)k * 3 * N * S);
    return G;
}

static GpTab tab_of(const Ctx &c) {
    return GpTab{c.off, c.Nr, c.Sr, reinterpret_cast<int64_t *>(c.ws + c.L.sq), reinterpret_cast<int32_t *>(c.ws + c.L.vn),
                 reinterpret_cast<int32_t *>(c.ws + c.L.gidx)};
}

static GpWeights weights_of(const et_gpgraph_sgcn_params &p) {
    return GpWeights{p.group_w, p.group_b, p.th, p.tau, p.mix_a, p.mix_w, p.mix_b, p.base.pred_len, p.base.out_dims};
}

// ---- group: one workgroup per real scene (the steps: et_gpgraph_core.inl)
__global__ __launch_bounds__(kSnThreads) void gp_group(Ctx c, GpTab tab, GpWeights p, WLay G, GpKeep K, int64_t n2real,
                                                       const float *__restrict__ g_abs, const float *__restrict__ g_rel,
                                                       const float *__restrict__ C_obs, const float *__restrict__ nrm,
                                                       int32_t *__restrict__ group_index, float *__restrict__ dist_out) {
    __shared__ int64_t part[kSnThreads];
    const int s = blockIdx.x, tid = threadIdx.x, T = c.T, Sr = c.Sr;
    const int64_t Nr = c.Nr;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    if (e <= b) return;
    const int64_t sq = scene_sq_before(c.off, s, part, ET_SGCN_MAX_N);  // (a larger scene takes no room)
    const int64_t nn = e - b;
    const bool ok = nn <= ET_SGCN_MAX_N && sq + nn * nn <= n2real;
    if (tid == 0) {
        int64_t *sqt = tab.sq;
        for (int m = 0; m < 3; ++m) sqt[m * Sr + s] = ok ? m * n2real + sq : -1;
    }
    if (!ok) return;
    GpScene gs;
    gs.va = c.ws + G.va + T * b;
    gs.feat = c.ws + G.feat + (int64_t)kGpHid * T * b;
    gs.D = c.ws + G.dist + sq;
    gs.sn = c.ws + G.sn + sq;
    if (K.sig >= 0) {
        gs.sig = c.ws + K.sig + sq;
        gs.cs = c.ws + K.cs + b;
        gs.cnt = reinterpret_cast<int32_t *>(c.ws + K.cnt) + b;
    }
    for (int m = 0; m < 3; ++m) {  // the three virtual scenes' rows: pass m at m Nr + b
        gs.in[m][0] = c.ws + c.L.vp + T * (m * Nr + b);
        gs.in[m][1] = c.ws + c.L.v + T * (m * Nr + b);
    }
    gp_group_scene<2>(tab, gs, p, s, b, (int)nn, T, sq, g_abs, g_rel, C_obs, nrm, group_index, dist_out);
}

static int check_gp(const et_gpgraph_sgcn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    const int rc = check_params(&p->base);
    if (rc != ET_OK) return rc;
    if (!p->group_w || !p->group_b || !p->th || !p->mix_a || !p->mix_w || !p->mix_b) return ET_ERR_INVALID_ARG;
    if (!(p->tau > 0.f)) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

static int64_t gp_total(const et_sgcn_params &b, int64_t N, int64_t sum_n2, int n_scenes) {
    const Lay L = lay_of(b.obs_len, 3 * N, 3 * sum_n2, 3 * (int64_t)n_scenes, true);
    return wlay_of(L, b.obs_len, b.pred_len, b.out_dims, N, sum_n2).total;
}

static int gp_run(const et_gpgraph_sgcn_params &p, const float *g_abs, const float *g_rel, const float *C_obs,
                  const float *nrm, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2, int64_t max_n, float *out,
                  int graph_layout, int32_t *group_index, float *dist, float *logit_s, float *logit_t, void *workspace,
                  size_t workspace_bytes, hipStream_t st) {
    const et_sgcn_params &bp = p.base;
    const int T = bp.obs_len;
    Ctx c;
    c.off = off;
    c.N = 3 * N;
    c.n2cap = 3 * sum_n2;
    c.S = 3 * n_scenes;
    c.T = T;
    c.ws = (float *)workspace;
    c.L = lay_of(T, 3 * N, 3 * sum_n2, 3 * (int64_t)n_scenes, true);
    c.Nr = N;
    c.Sr = n_scenes;
    const WLay G = wlay_of(c.L, T, bp.pred_len, bp.out_dims, N, sum_n2);
    if (!workspace || workspace_bytes < (size_t)G.total * 4) return ET_ERR_WORKSPACE;
    const Ident I{nullptr, nullptr, 1, -1};  // eye(n) and eye(T): generate_identity_matrix
    hipLaunchKernelGGL(sgcn_prep<true>, dim3(1), dim3(kSnThreads), 0, st, bp, c.ws);
    const GpTab tab = tab_of(c);
    const GpWeights w = weights_of(p);
    hipLaunchKernelGGL(gp_group, dim3((unsigned)n_scenes), dim3(kSnThreads), 0, st, c, tab, w, G, GpKeep{-1, -1, -1}, sum_n2,
                       g_abs, g_rel, C_obs, nrm, group_index, dist);
    float *po = c.ws + G.po;
    run_layers<true>(bp, c, nullptr, I, nullptr, nullptr, max_n, po, logit_s, logit_t, st);
    hipLaunchKernelGGL(gp_mix, dim3((unsigned)N), dim3(kMixThreads), 6 * bp.out_dims * bp.pred_len * sizeof(float), st, tab, w,
                       po, out, graph_layout);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

#include "et_sgcn_train.inl"

#include "et_gpgraph_train.inl"

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_gpgraph_sgcn_workspace_bytes(const et_gpgraph_sgcn_params *params, int64_t N, int64_t sum_n2,
                                                  int n_scenes) {
    if (check_gp(params) != ET_OK || N <= 0 || sum_n2 < 0 || n_scenes < 0) return 0;
    return (size_t)gp_total(params->base, N, sum_n2, n_scenes) * 4;
}

extern "C" int et_gpgraph_sgcn_forward_scenes(const et_gpgraph_sgcn_params *params, const float *C_obs, const float *nrm,
                                              int64_t N, const int32_t *scene_offsets, int n_scenes, int64_t sum_n2,
                                              int64_t max_scene_n, float *C_pred_refine, int32_t *group_index, float *dist,
                                              float *logit_s, float *logit_t, void *workspace, size_t workspace_bytes,
                                              et_stream_t stream) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    // (the three passes are scenes and rows of their own: 3 N and 3 n_scenes are what has to fit 32 bits)
    if (3 * N > INT32_MAX || 3 * (int64_t)n_scenes > INT32_MAX || sum_n2 < 0 || max_scene_n < 0) return ET_ERR_INVALID_ARG;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SGCN_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
        max_scene_n = N;
    }
    if (max_scene_n > ET_SGCN_MAX_N) max_scene_n = ET_SGCN_MAX_N;  // larger scenes are not computed
    return gp_run(*params, nullptr, nullptr, C_obs, nrm, N, scene_offsets, n_scenes, sum_n2, max_scene_n, C_pred_refine, 0,
                  group_index, dist, logit_s, logit_t, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_gpgraph_sgcn_forward_graph(const et_gpgraph_sgcn_params *params, const float *v_abs, const float *v_rel,
                                             int64_t N, float *out, int32_t *group_index, float *dist, float *logit_s,
                                             float *logit_t, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SGCN_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v_abs || !v_rel || !out) return ET_ERR_INVALID_ARG;
    return gp_run(*params, v_abs, v_rel, nullptr, nullptr, N, nullptr, 1, N * N, N, out, 1, group_index, dist, logit_s,
                  logit_t, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- training (et_gpgraph_train.inl)
extern "C" size_t et_gpgraph_sgcn_train_workspace_bytes(const et_gpgraph_sgcn_params *params, int64_t N, int64_t sum_n2,
                                                        int n_scenes) {
    if (check_gp(params) != ET_OK || N <= 0 || sum_n2 < 0 || n_scenes < 0) return 0;
    return (size_t)gtlay_of(params->base, N, sum_n2, n_scenes).total * 4;
}

extern "C" int64_t et_gpgraph_sgcn_grad_floats(const et_gpgraph_sgcn_params *params) {
    if (check_gp(params) != ET_OK) return 0;
    return gp_grad_floats(params->base);
}

extern "C" int et_gpgraph_sgcn_train_layout(const et_gpgraph_sgcn_params *params, int64_t N, int64_t sum_n2, int n_scenes,
                                            int64_t *offsets, int n_offsets) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    if (N <= 0 || sum_n2 < 0 || n_scenes < 0 || !offsets || n_offsets != ET_GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS)
        return ET_ERR_INVALID_ARG;
    const GTLay g = gtlay_of(params->base, N, sum_n2, n_scenes);
    const TLay &t = g.t;
    const int64_t f[ET_GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS] = {
        t.L.v, t.L.rs_s, t.L.rs_t, t.xs, t.xs_stride, t.xt, t.xt_stride, t.L.at, t.L.f2, t.L.f1, t.L.ts, t.keep,
        tail_keep_floats(params->base), t.dat, t.df1, t.dts, t.df2, t.rrec, t.gs, t.gt, t.dir_s, t.dir_t, t.dd_s,
        t.L.vp, t.L.vn, t.L.gidx, t.dax, t.srec, t.trec, t.dacc_t, t.dx_as, t.dxp, t.dxv,
        g.W.va, g.W.feat, g.W.dist, g.W.sn, g.W.po, g.sig, g.cs, g.cnt, g.dmix, g.dpo, g.dvp, g.dP, g.dsig, g.dd, g.df, g.total};
    for (int i = 0; i < ET_GPGRAPH_SGCN_TRAIN_LAYOUT_FIELDS; ++i) offsets[i] = f[i];
    return ET_OK;
}

extern "C" int et_gpgraph_sgcn_train_forward_scenes(const et_gpgraph_sgcn_params *params, const float *C_obs, const float *nrm,
                                                    int64_t N, const int32_t *scene_offsets, int n_scenes, int64_t sum_n2,
                                                    int64_t max_scene_n, float *C_pred_refine, int32_t *group_index,
                                                    float *dist, float *logit_s, float *logit_t, void *workspace,
                                                    size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    if (3 * N > INT32_MAX || 3 * (int64_t)n_scenes > INT32_MAX || sum_n2 < 0 || max_scene_n < 0) return ET_ERR_INVALID_ARG;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SGCN_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
        max_scene_n = N;
    }
    if (max_scene_n > ET_SGCN_MAX_N) max_scene_n = ET_SGCN_MAX_N;  // larger scenes are not computed
    return gp_run_train(*params, nullptr, nullptr, C_obs, nrm, N, scene_offsets, n_scenes, sum_n2, max_scene_n, C_pred_refine,
                        0, group_index, dist, logit_s, logit_t, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_gpgraph_sgcn_train_forward_graph(const et_gpgraph_sgcn_params *params, const float *v_abs,
                                                   const float *v_rel, int64_t N, float *out, int32_t *group_index,
                                                   float *dist, float *logit_s, float *logit_t, void *workspace,
                                                   size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SGCN_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v_abs || !v_rel || !out) return ET_ERR_INVALID_ARG;
    return gp_run_train(*params, v_abs, v_rel, nullptr, nullptr, N, nullptr, 1, N * N, N, out, 1, group_index, dist, logit_s,
                        logit_t, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_gpgraph_sgcn_backward_scenes(const et_gpgraph_sgcn_params *params, int64_t N, const int32_t *scene_offsets,
                                               int n_scenes, int64_t sum_n2, int64_t max_scene_n, const float *d_out,
                                               float *grads, int64_t grads_floats, void *workspace, size_t workspace_bytes,
                                               et_stream_t stream) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    if (sum_n2 < 0 || max_scene_n < 0 || !grads || grads_floats < gp_grad_floats(params->base)) return ET_ERR_INVALID_ARG;
    if (N < 0 || 3 * N > INT32_MAX || n_scenes < 0 || 3 * (int64_t)n_scenes > INT32_MAX ||
        (scene_offsets && n_scenes == 0 && N != 0) || (!scene_offsets && N > ET_SGCN_MAX_N) || (N > 0 && !d_out))
        return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
        max_scene_n = N;
    }
    if (max_scene_n > ET_SGCN_MAX_N) max_scene_n = ET_SGCN_MAX_N;
    if (N == 0) {  // no scene: every gradient is zero
        if (hipMemsetAsync(grads, 0, (size_t)gp_grad_floats(params->base) * 4, (hipStream_t)stream) != hipSuccess)
            return ET_ERR_HIP;
        return ET_OK;
    }
    return gp_run_backward(*params, N, scene_offsets, n_scenes, sum_n2, max_scene_n, d_out, 0, grads, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

extern "C" int et_gpgraph_sgcn_backward_graph(const et_gpgraph_sgcn_params *params, int64_t N, const float *d_out, float *grads,
                                              int64_t grads_floats, void *workspace, size_t workspace_bytes,
                                              et_stream_t stream) {
    const int rc = check_gp(params);
    if (rc != ET_OK) return rc;
    if (N <= 0 || N > ET_SGCN_MAX_N || !d_out || !grads || grads_floats < gp_grad_floats(params->base))
        return ET_ERR_INVALID_ARG;
    return gp_run_backward(*params, N, nullptr, 1, N * N, N, d_out, 1, grads, workspace, workspace_bytes, (hipStream_t)stream);
}

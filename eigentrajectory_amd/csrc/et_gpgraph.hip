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
// The merge.  The reference walks the close pairs (r, c), c < r, in row-major order and gives every pedestrian that carries
// r's label the label c -- c itself, not c's label, so the result is NOT the connected components.  Within row r with close
// columns c1 < .. < cm the walk moves label[r]'s carriers to c1, then c1's carriers (those included) to c2, ..: at the end
// every pedestrian whose label was in {label[r], c1, .., c(m-1)} carries cm.  That is one parallel step per row, n serial
// steps per scene (rows without a close column are skipped without a barrier).
// Every sum runs in a fixed order inside one lane, so results are bit-identical from run to run and a scene's result does
// not depend on the scenes around it.
#include "et_common.h"

namespace et {
namespace {

#include "et_sgcn_core.inl"

constexpr int kGpHid = 8;  // group_cnn's output channels
constexpr int kMixThreads = 128;

struct GLay {  // the workspace behind the base's (floats): v_abs (T,N), conv features (8,T,N), dist and sig_norm (sum n^2),
    int64_t va, feat, dist, sn, po, total;  // the base's output for the 3 N virtual rows (k, 3 N, S)
};

__host__ __device__ inline GLay glay_of(const Lay &L, int T, int k, int S, int64_t N, int64_t n2) {
    GLay G;
    G.va = L.total;
    G.feat = up4(G.va + T * N);
    G.dist = up4(G.feat + (int64_t)kGpHid * T * N);
    G.sn = up4(G.dist + n2);
    G.po = up4(G.sn + n2);
    G.total = up4(G.po + (int64_t)k * 3 * N * S);
    return G;
}

__device__ __forceinline__ float sig_of(float d, float th, float tau) { return 1.0f / (1.0f + expf(-(-(d - th) / tau))); }

// ---- group: one workgroup per real scene
__global__ __launch_bounds__(kSnThreads) void gp_group(Ctx c, et_gpgraph_sgcn_params p, GLay G, int64_t n2real,
                                                       const float *__restrict__ g_abs, const float *__restrict__ g_rel,
                                                       const float *__restrict__ C_obs, const float *__restrict__ nrm,
                                                       int32_t *__restrict__ group_index, float *__restrict__ dist_out) {
    __shared__ int64_t part[kSnThreads];
    __shared__ float red[2 * kSnThreads / kWave];
    __shared__ int lab[ET_SGCN_MAX_N], cmx[ET_SGCN_MAX_N], idx[ET_SGCN_MAX_N], cnt[ET_SGCN_MAX_N];
    __shared__ unsigned char hit[ET_SGCN_MAX_N];
    __shared__ float cs[ET_SGCN_MAX_N];
    __shared__ int n_groups;
    const int s = blockIdx.x, tid = threadIdx.x, T = c.T, Sr = c.Sr;
    const int64_t Nr = c.Nr;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    if (e <= b) return;
    const int64_t sq = scene_sq_before(c.off, s, part, ET_SGCN_MAX_N);  // (a larger scene takes no room)
    const int64_t nn = e - b;
    const bool ok = nn <= ET_SGCN_MAX_N && sq + nn * nn <= n2real;
    if (tid == 0) {
        int64_t *sqt = reinterpret_cast<int64_t *>(c.ws + c.L.sq);
        for (int m = 0; m < 3; ++m) sqt[m * Sr + s] = ok ? m * n2real + sq : -1;
    }
    if (!ok) return;
    const int n = (int)nn;
    float *va = c.ws + G.va + T * b;
    float *feat = c.ws + G.feat + (int64_t)kGpHid * T * b;
    float *D = c.ws + G.dist + sq, *sn = c.ws + G.sn + sq;
    float *v0 = c.ws + c.L.v + T * b, *p0 = c.ws + c.L.vp + T * b;
    float *v1 = v0 + T * Nr, *p1 = p0 + T * Nr, *v2 = v1 + T * Nr, *p2 = p1 + T * Nr;
    const float th = p.th[0], tau = p.tau;

    // v_abs, and the pedestrian graph v_rel = [position; coefficients]
    scene_v(va, g_abs, C_obs, nrm, Nr, b, n, T, red);
    for (int q = tid; q < T * n; q += kSnThreads) {
        p0[q] = g_rel ? g_rel[q] : (float)(q / n + 1);
        if (g_rel) v0[q] = g_rel[T * n + q];
    }
    __syncthreads();
    if (!g_rel)
        for (int q = tid; q < T * n; q += kSnThreads) v0[q] = va[q];
    // group_cnn: Conv2d(1, 8, (3, 1), padding (1, 0)) along t
    for (int q = tid; q < kGpHid * T * n; q += kSnThreads) {
        const int i = q % n, t = (q / n) % T, ch = q / (n * T);
        float acc = p.group_b[ch];
        for (int d = 0; d < 3; ++d) {
            const int tt = t + d - 1;
            if (tt >= 0 && tt < T) acc = fmaf(p.group_w[ch * 3 + d], va[tt * n + i], acc);
        }
        feat[q] = acc;
    }
    __syncthreads();
    // d[i][j]: the mean over t of the L2 norm over the channels (symmetric bit for bit: (a - b)^2 = (b - a)^2, one order)
    for (int q = tid; q < n * n; q += kSnThreads) {
        const int i = q / n, j = q % n;
        float tot = 0.f;
        for (int t = 0; t < T; ++t) {
            float ss = 0.f;
            for (int ch = 0; ch < kGpHid; ++ch) {
                const float df = feat[(ch * T + t) * n + i] - feat[(ch * T + t) * n + j];
                ss = fmaf(df, df, ss);
            }
            tot += sqrtf(ss);
        }
        const float d = tot / (float)T;
        D[q] = d;
        if (dist_out) dist_out[sq + q] = d;
    }
    __syncthreads();
    // the last close column of every row (-1: none), and the labels' start
    for (int r = tid; r < n; r += kSnThreads) {
        int cm = -1;
        for (int cc = 0; cc < r; ++cc)
            if (D[r * n + cc] <= th) cm = cc;
        cmx[r] = cm;
        lab[r] = r;
    }
    __syncthreads();
    for (int r = 1; r < n; ++r) {
        const int cm = cmx[r];
        if (cm < 0) continue;  // (uniform)
        const int lr = lab[r];
        for (int cc = tid; cc < n; cc += kSnThreads) hit[cc] = cc < r && D[r * n + cc] <= th;
        __syncthreads();
        for (int i = tid; i < n; i += kSnThreads) {
            const int l = lab[i];
            if (hit[l] || l == lr) lab[i] = cm;
        }
        __syncthreads();
    }
    // compact labels in the order of the surviving values; group sizes
    for (int i = tid; i < n; i += kSnThreads) {
        hit[i] = 0;
        cnt[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kSnThreads) hit[lab[i]] = 1;
    __syncthreads();
    for (int i = tid; i < n; i += kSnThreads) {
        int rank = 0;
        for (int l = 0; l < lab[i]; ++l) rank += hit[l];
        idx[i] = rank;
        atomicAdd(&cnt[rank], 1);
    }
    if (tid == 0) {
        int g = 0;
        for (int l = 0; l < n; ++l) g += hit[l];
        n_groups = g;
    }
    __syncthreads();
    const int ng = n_groups;
    if (tid == 0) {
        int32_t *vn = reinterpret_cast<int32_t *>(c.ws + c.L.vn);
        vn[s] = n;
        vn[Sr + s] = ng;
        vn[2 * Sr + s] = n;
    }
    int32_t *gi = reinterpret_cast<int32_t *>(c.ws + c.L.gidx) + b;
    for (int i = tid; i < n; i += kSnThreads) {
        gi[i] = idx[i];
        if (group_index) group_index[b + i] = idx[i];
    }
    // sig / sig.sum(dim = 0)
    for (int j = tid; j < n; j += kSnThreads) {
        float sum = 0.f;
        for (int i = 0; i < n; ++i) sum += sig_of(D[i * n + j], th, tau);
        cs[j] = sum;
    }
    __syncthreads();
    for (int q = tid; q < n * n; q += kSnThreads) sn[q] = sig_of(D[q], th, tau) / cs[q % n];
    __syncthreads();
    // v' = (v_rel - v_soft) + v_soft, v_soft = v_rel @ sig_norm: both channels
    for (int q = tid; q < 2 * T * n; q += kSnThreads) {
        const int j = q % n, t = (q / n) % T, ch = q / (n * T);
        const float *x = (ch ? v0 : p0) + t * n;
        float soft = 0.f;
        for (int i = 0; i < n; ++i) soft = fmaf(x[i], sn[i * n + j], soft);
        (ch ? v2 : p2)[t * n + j] = (x[j] - soft) + soft;
    }
    __syncthreads();
    // the group means of v', pedestrians in ascending order
    for (int q = tid; q < 2 * T * ng; q += kSnThreads) {
        const int g = q % ng, t = (q / ng) % T, ch = q / (ng * T);
        const float *x = (ch ? v2 : p2) + t * n;
        float sum = 0.f;
        for (int i = 0; i < n; ++i)
            if (idx[i] == g) sum += x[i];
        (ch ? v1 : p1)[t * ng + g] = sum / (float)cnt[g];
    }
}

// ---- mix: one workgroup per pedestrian
__global__ __launch_bounds__(kMixThreads) void gp_mix(Ctx c, et_gpgraph_sgcn_params p, const float *__restrict__ po,
                                                      float *__restrict__ out, int graph_layout) {
    extern __shared__ float mix_lds[];  // the three passes' (S, k) as they are, and after the PReLU
    const int k = p.base.pred_len, S = p.base.out_dims, Sk = S * k, tid = threadIdx.x;
    float *raw = mix_lds, *act = mix_lds + 3 * Sk;
    const int64_t r = blockIdx.x, Nr = c.Nr;
    const int s = c.off ? scene_of_row(c.off, c.Sr, r) : 0;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    const bool ok = r >= b && r < e && reinterpret_cast<const int64_t *>(c.ws + c.L.sq)[s] >= 0;
    int64_t row[3] = {r, r, 2 * Nr + r};
    if (ok) row[1] = Nr + b + reinterpret_cast<const int32_t *>(c.ws + c.L.gidx)[r];  // unpool: the group's row
    const float a = p.mix_a[0];
    for (int q = tid; q < 3 * Sk; q += kMixThreads) {
        const int m = q / Sk, ss = (q % Sk) / k, t = q % k;
        const float x = ok ? po[((int64_t)t * 3 * Nr + row[m]) * S + ss] : __builtin_nanf("");
        raw[q] = x;
        act[q] = prelu(x, a);
    }
    __syncthreads();
    for (int o = tid; o < Sk; o += kMixThreads) {
        const float *w = p.mix_w + (int64_t)o * 3 * Sk;
        float acc = p.mix_b[o];
        for (int q = 0; q < 3 * Sk; ++q) acc = fmaf(w[q], act[q], acc);
        const float y = ((raw[o] + raw[Sk + o]) + raw[2 * Sk + o]) / 3.0f + acc;
        const int ss = o / k, t = o % k;
        if (graph_layout)
            out[((int64_t)ss * k + t) * Nr + r] = y;
        else
            out[((int64_t)t * Nr + r) * S + ss] = y;
    }
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
    return glay_of(L, b.obs_len, b.pred_len, b.out_dims, N, sum_n2).total;
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
    const GLay G = glay_of(c.L, T, bp.pred_len, bp.out_dims, N, sum_n2);
    if (!workspace || workspace_bytes < (size_t)G.total * 4) return ET_ERR_WORKSPACE;
    const Ident I{nullptr, nullptr, 1, -1};  // eye(n) and eye(T): generate_identity_matrix
    hipLaunchKernelGGL(sgcn_prep<true>, dim3(1), dim3(kSnThreads), 0, st, bp, c.ws);
    hipLaunchKernelGGL(gp_group, dim3((unsigned)n_scenes), dim3(kSnThreads), 0, st, c, p, G, sum_n2, g_abs, g_rel, C_obs, nrm,
                       group_index, dist);
    float *po = c.ws + G.po;
    run_layers<true>(bp, c, nullptr, I, nullptr, nullptr, max_n, po, logit_s, logit_t, st);
    hipLaunchKernelGGL(gp_mix, dim3((unsigned)N), dim3(kMixThreads), 6 * bp.out_dims * bp.pred_len * sizeof(float), st, c, p,
                       po, out, graph_layout);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

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
    if (N < 0 || 3 * N > INT32_MAX || n_scenes < 0 || 3 * (int64_t)n_scenes > INT32_MAX || sum_n2 < 0 || max_scene_n < 0)
        return ET_ERR_INVALID_ARG;
    if (scene_offsets && n_scenes == 0) return N == 0 ? ET_OK : ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        if (N > ET_SGCN_MAX_N) return ET_ERR_INVALID_ARG;
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

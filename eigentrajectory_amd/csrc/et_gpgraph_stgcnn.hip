// et_gpgraph_stgcnn.hip -- GP-Graph-STGCNN inference (baseline/gpgraphstgcnn: bridge.py pre-hook, model_groupwrapper.py
// GPGraph.forward around model_baseline.py's social_stgcnn in eval mode, bridge.py post-hook) for the ET configuration
// (include/eigentraj.h "GP-Graph-STGCNN predictor").
//
// GP-Graph runs the SAME Social-STGCNN three times with shared weights -- on the pedestrian graph, on the graph of group
// means and on the pedestrian graph with the inverse-distance kernel cut down to pairs of one group -- so the three graphs of
// S scenes are 3 S virtual scenes of ONE launch of the scene body of et_stgcnn_core.inl.  Per call, for any number of
// scenes, three launches:
//   group   per scene          et_gpgraph_core.inl's steps on one channel: distances, decisions d <= th, the reference's
//                              merge, compact labels, sig / sig.sum(0), v' = (v - v_soft) + v_soft, the group means; the three
//                              virtual scenes' inputs as (T, n_m) blocks, their node counts (n, G, n)
//   passes  per virtual scene  run_scene with the Laplacian formed from u and d where it is used (pass 2: the same-group
//                              predicate on a_inv, in the degree as well), output through the reference's view into
//                              (k, 3 N, S); the arena in LDS when the virtual scene fits, else in the workspace -- the three
//                              passes of one scene may sit in different places (a scene of 34 pedestrians in 33 groups)
//   mix     per pedestrian     et_gpgraph_core.inl's kernel: unpool by gather, mean of the three, PReLU, the product
// The base is the ORIGINAL Social-STGCNN gcn (a 1x1 conv to S channels, time row t contracted with its own Laplacian), not
// ET-STGCNN's (S K channels, contracted over all rows): Src::kPerRow of the scene body.
// Every sum runs in a fixed order inside one lane, so results are bit-identical from run to run and a scene's result does
// not depend on the scenes around it.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"
#include "et_stgcnn_core.inl"
#include "et_gpgraph_core.inl"

static_assert(kSgThreads == kSnThreads, "the group steps and the scene body share one workgroup size");

struct GsLay {  // the workspace, in floats: the tables (sq int64 [3 S], vn int32 [3 S], gidx int32 [N]), v_abs (T, N), conv
    int64_t sq, vn, gidx, va, feat, dist, sn, in, po, arena, total;  // features (8, T, N), dist and sig_norm (sum n^2), the
    int64_t arena_floats;                                            // passes' inputs (3, T N), their outputs (k, 3 N, S),
};                                                                   // the arenas of scenes too large for LDS (3 N rows)

__host__ __device__ inline GsLay gslay_of(const Dims &D, int64_t N, int64_t n2, int64_t S) {
    GsLay G;
    const int T = D.K;
    G.sq = 0;
    G.vn = up4(G.sq + 2 * 3 * S);
    G.gidx = up4(G.vn + 3 * S);
    G.va = up4(G.gidx + N);
    G.feat = up4(G.va + T * N);
    G.dist = up4(G.feat + (int64_t)kGpHid * T * N);
    G.sn = up4(G.dist + n2);
    G.in = up4(G.sn + n2);
    G.po = up4(G.in + 3 * (int64_t)T * N);
    G.arena = up4(G.po + (int64_t)D.k * 3 * N * D.S);
    // the largest scene the caller may have: at most N rows, ET_SGCN_MAX_N, and n^2 <= sum n^2
    int64_t cap = N < ET_SGCN_MAX_N ? N : ET_SGCN_MAX_N;
    while (cap > 0 && cap * cap > n2) --cap;
    G.arena_floats = arena_per_ped(D) * cap * 4 <= kSgLdsBytes ? 0 : arena_per_ped(D) * 3 * N;
    G.total = up4(G.arena + G.arena_floats);
    return G;
}

// ---- group: one workgroup per real scene
__global__ __launch_bounds__(kSnThreads) void gps_group(GpTab tab, GpWeights p, GsLay G, float *ws, int T, int64_t n2real,
                                                        const float *__restrict__ g_abs, const float *__restrict__ g_rel,
                                                        const float *__restrict__ C_obs, const float *__restrict__ nrm,
                                                        int32_t *__restrict__ group_index, float *__restrict__ dist_out,
                                                        float *__restrict__ graph_inputs) {
    __shared__ int64_t part[kSnThreads];
    const int s = blockIdx.x, tid = threadIdx.x, Sr = tab.Sr;
    const int64_t Nr = tab.Nr;
    const int64_t b = tab.off ? tab.off[s] : 0;
    const int64_t e = tab.off ? tab.off[s + 1] : Nr;
    if (e <= b) return;
    const int64_t sq = scene_sq_before(tab.off, s, part, ET_SGCN_MAX_N);  // (a larger scene takes no room)
    const int64_t nn = e - b;
    const bool ok = nn <= ET_SGCN_MAX_N && sq + nn * nn <= n2real;
    if (tid == 0)
        for (int m = 0; m < 3; ++m) tab.sq[m * Sr + s] = ok ? sq : -1;
    if (!ok) return;
    const int n = (int)nn;
    GpScene gs;
    gs.va = ws + G.va + T * b;
    gs.feat = ws + G.feat + (int64_t)kGpHid * T * b;
    gs.D = ws + G.dist + sq;
    gs.sn = ws + G.sn + sq;
    for (int m = 0; m < 3; ++m) gs.in[m][0] = gs.in[m][1] = ws + G.in + T * (m * Nr + b);
    gp_group_scene<1>(tab, gs, p, s, b, n, T, sq, g_abs, g_rel, C_obs, nrm, group_index, dist_out);
    if (!graph_inputs) return;
    __syncthreads();
    const int ng = tab.vn[Sr + s];
    for (int m = 0; m < 3; ++m) {
        const int nm = m == 1 ? ng : n;
        for (int q = tid; q < T * nm; q += kSnThreads) graph_inputs[T * (m * Nr + b) + q] = gs.in[m][0][q];
    }
}

// pass m of a real scene: the input block the group kernel wrote, L formed from u and d, the output in the stack of the
// three passes (k, 3 N, S) at rows m N + b ..
struct GpSrc {
    static constexpr bool kComputed = true, kPerRow = true;
    const float *in;     // (T, n)
    const int32_t *gi;   // the scene's group indices (in LDS): a_inv stays where they are equal; NULL: everywhere
    float *po;
    int64_t N3, row0;
    __device__ void load(float *u, int64_t, int n, int K, float *) const {
        for (int i = threadIdx.x; i < K * n; i += kSgThreads) u[i] = in[i];
    }
    __device__ int key(int w) const { return gi ? gi[w] : 0; }  // (read once per lane, outside the loops over vv)
    __device__ bool keep(int vv, int kw) const { return !gi || gi[vv] == kw; }
    // L[kk,vv,w] = [vv == w] - (d_v a_hat[vv,w]) d_w, a_hat = a_inv * mask + I (generate_adjacency_matrix)
    __device__ float lap(int kk, int vv, int w, int n, const float *u, const float *d, float uw, float dw, int kw) const {
        const float dist = fabsf(u[kk * n + vv] - uw);
        const float ainv = dist == 0.f || !keep(vv, kw) ? 0.f : 1.0f / dist;
        const float eye = vv == w ? 1.f : 0.f;
        return eye - (d[kk * n + vv] * (ainv + eye)) * dw;
    }
    // tpcnn_ouput's output (o, h, w) -> view (S,k,n) (model_baseline.py:147) -> (k, rows, S)
    __device__ void store(int o, int h, int w, int k, int S, int, int64_t, float val) const {
        const int r = o * S + h;
        const int s = r / k, t = r - s * k;
        po[((int64_t)t * N3 + row0 + w) * S + s] = val;
    }
};

// ---- passes: one workgroup per virtual scene (pass m, scene s) = blockIdx m Sr + s
__global__ __launch_bounds__(kSgThreads) void gps_passes(et_stgcnn_params p, GpTab tab, const float *__restrict__ in,
                                                         float *__restrict__ po, float *arena, int64_t arena_floats,
                                                         int lds_floats) {
    extern __shared__ float lds[];
    __shared__ int32_t gi[ET_SGCN_MAX_N];  // pass 2: the scene's group indices, read once per pedestrian in every Laplacian entry
    const int Sr = tab.Sr;
    const int m = blockIdx.x / Sr, s = blockIdx.x - m * Sr;
    const int64_t Nr = tab.Nr;
    const int64_t b = tab.off ? tab.off[s] : 0;
    const int64_t e = tab.off ? tab.off[s + 1] : Nr;
    if (e <= b || tab.sq[s] < 0) return;  // (a scene that was not grouped: the mix kernel answers NaN)
    const int n = tab.vn[m * Sr + s];
    if (n <= 0 || n > e - b) return;
    const Dims D = dims_of(p, true);
    const int64_t per = arena_per_ped(D);
    const int64_t row0 = m * Nr + b;
    if (m == 2) {  // (uniform)
        for (int i = threadIdx.x; i < n; i += kSgThreads) gi[i] = tab.gidx[b + i];
        __syncthreads();
    }
    const GpSrc src{in + D.K * row0, m == 2 ? gi : nullptr, po, 3 * Nr, row0};
    if (per * n <= lds_floats) {
        run_scene(src, p, D, b, n, lds, nullptr);
    } else if ((row0 + n) * per <= arena_floats) {
        run_scene(src, p, D, b, n, arena + row0 * per, nullptr);
    } else {  // fits nowhere: NaN, never an access outside the buffers
        const float nan = __builtin_nanf("");
        for (int i = threadIdx.x; i < D.k * D.S * n; i += kSgThreads) {
            const int w = i % n, oh = i / n;
            src.store(oh / D.S, oh % D.S, w, D.k, D.S, n, b, nan);
        }
    }
}

static int check_gps(const et_gpgraph_stgcnn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    const int rc = check_params(&p->base);
    if (rc != ET_OK) return rc;
    if (!p->group_w || !p->group_b || !p->th || !p->mix_a || !p->mix_w || !p->mix_b) return ET_ERR_INVALID_ARG;
    if (!(p->tau > 0.f)) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

static int gps_run(const et_gpgraph_stgcnn_params &p, const float *g_abs, const float *g_rel, const float *C_obs,
                   const float *nrm, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2, float *out,
                   int graph_layout, int32_t *group_index, float *dist, float *graph_inputs, void *workspace,
                   size_t workspace_bytes, hipStream_t st) {
    const Dims D = dims_of(p.base, true);
    const GsLay G = gslay_of(D, N, sum_n2, n_scenes);
    if (!workspace || workspace_bytes < (size_t)G.total * 4) return ET_ERR_WORKSPACE;
    float *ws = (float *)workspace;
    const GpTab tab{off, N, n_scenes, reinterpret_cast<int64_t *>(ws + G.sq), reinterpret_cast<int32_t *>(ws + G.vn),
                    reinterpret_cast<int32_t *>(ws + G.gidx)};
    const GpWeights w{p.group_w, p.group_b, p.th, p.tau, p.mix_a, p.mix_w, p.mix_b, D.k, D.S};
    hipLaunchKernelGGL(gps_group, dim3((unsigned)n_scenes), dim3(kSnThreads), 0, st, tab, w, G, ws, D.K, sum_n2, g_abs, g_rel,
                       C_obs, nrm, group_index, dist, graph_inputs);
    float *po = ws + G.po;
    hipLaunchKernelGGL(gps_passes, dim3(3u * (unsigned)n_scenes), dim3(kSgThreads), kSgLdsBytes, st, p.base, tab, ws + G.in, po,
                       ws + G.arena, G.arena_floats, kSgLdsBytes / 4);
    hipLaunchKernelGGL(gp_mix, dim3((unsigned)N), dim3(kMixThreads), 6 * D.S * D.k * sizeof(float), st, tab, w, po, out,
                       graph_layout);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_gpgraph_stgcnn_workspace_bytes(const et_gpgraph_stgcnn_params *params, int64_t N, int64_t sum_n2,
                                                    int n_scenes) {
    if (check_gps(params) != ET_OK || N <= 0 || sum_n2 < 0 || n_scenes < 0) return 0;
    return (size_t)gslay_of(dims_of(params->base, true), N, sum_n2, n_scenes).total * 4;
}

extern "C" int et_gpgraph_stgcnn_forward_scenes(const et_gpgraph_stgcnn_params *params, const float *C_obs, const float *nrm,
                                                int64_t N, const int32_t *scene_offsets, int n_scenes, int64_t sum_n2,
                                                int64_t max_scene_n, float *C_pred_refine, int32_t *group_index, float *dist,
                                                float *graph_inputs, void *workspace, size_t workspace_bytes,
                                                et_stream_t stream) {
    const int rc = check_gps(params);
    if (rc != ET_OK) return rc;
    // (the three passes are scenes and rows of their own: 3 N and 3 n_scenes are what has to fit 32 bits)
    if (3 * N > INT32_MAX || 3 * (int64_t)n_scenes > INT32_MAX || sum_n2 < 0 || max_scene_n < 0) return ET_ERR_INVALID_ARG;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SGCN_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!scene_offsets) {
        n_scenes = 1;
        sum_n2 = N * N;
    }
    return gps_run(*params, nullptr, nullptr, C_obs, nrm, N, scene_offsets, n_scenes, sum_n2, C_pred_refine, 0, group_index,
                   dist, graph_inputs, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int et_gpgraph_stgcnn_forward_graph(const et_gpgraph_stgcnn_params *params, const float *v_abs, const float *v_rel,
                                               int64_t N, float *out, int32_t *group_index, float *dist, float *graph_inputs,
                                               void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_gps(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SGCN_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v_abs || !v_rel || !out) return ET_ERR_INVALID_ARG;
    return gps_run(*params, v_abs, v_rel, nullptr, nullptr, N, nullptr, 1, N * N, out, 1, group_index, dist, graph_inputs,
                   workspace, workspace_bytes, (hipStream_t)stream);
}

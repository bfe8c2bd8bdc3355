// et_stgcnn.hip -- Social-STGCNN inference (baseline/stgcnn: bridge.py pre-hook, model.py social_stgcnn.forward in eval
// mode, bridge.py post-hook) for the ET configuration family (include/eigentraj.h "Social-STGCNN predictor").
//
// One workgroup per scene; the scene's activations live in an arena of (2K + 2SK + Q) floats per pedestrian:
//   u (K,n)   the input v = [C_obs; obs_ori]: one channel, K = k+2 "time" rows
//   d (K,n)   D = rowsum(a_hat)^-1/2 of every time row (scene form only)
//   x (S,K,n) st_gcn activations; viewed (K,S,n) (model.py:136) they are the tpcnn input
//   y (S,K,n) gcn output -> BN -> PReLU; the tpcnn ping buffer (k,S,n)
//   q (Q n)   the Laplacian contraction of a chunk of time rows; the tpcnn pong buffer (k,S,n)
// in LDS when it fits kSgLdsBytes (S = 20, k = 6: 1824 B per pedestrian, n <= 33 -- the real scenes), else in the
// caller's workspace at the scene's rows.  The scene form never stores the (K,n,n) Laplacian: each entry is formed from u
// and d where it is used.  The st_gcn contraction einsum('nkctv,kvw->nctw', conv1x1(x), L) is regrouped as
//   y[c,t,w] = sum_kk ( sum_ci W[kk S + c, ci] P[kk,ci K + t,w] + b[kk S + c] P[kk,C_in K,w] ),
//   P[kk,j,w] = sum_v X_j[v] L[kk,v,w]    (X_j = x[ci,t,:], and the ones row for the conv bias)
// so the O(K^2 n^2) part runs over C_in K + 1 rows instead of S K: 9 rather than 160 in the first layer (C_in = 1).
// Lanes take (time row, pedestrian) pairs in the contraction and (channel, row, pedestrian) triples in the convolutions:
// K n and k S n lanes, so a scene of 8 pedestrians already fills a wavefront.
// The scene body (run_scene and what it needs) is et_stgcnn_core.inl, shared with et_gpgraph_stgcnn.hip; this file holds the
// two sources of ET-STGCNN and the C entry points.
#include "et_common.h"

namespace et {
namespace {

#include "et_stgcnn_core.inl"

// one scene as the bridge hands it over: v (1,1,K,N), L (K,N,N) given
struct GraphSrc {
    static constexpr bool kComputed = false, kPerRow = false;
    const float *v, *a;
    float *out;  // (1,S,k,N) raw network output
    __device__ void load(float *u, int64_t, int n, int K, float *) const {
        for (int i = threadIdx.x; i < K * n; i += kSgThreads) u[i] = v[i];
    }
    __device__ int key(int) const { return 0; }
    __device__ bool keep(int, int) const { return true; }
    __device__ float lap(int kk, int vv, int w, int n, const float *, const float *, float, float, int) const {
        return a[((int64_t)kk * n + vv) * n + w];
    }
    // tpcnn_ouput's output (o, h, w) viewed (1,S,k,N) is the raw output: the same memory
    __device__ void store(int o, int h, int w, int, int S, int n, int64_t, float val) const {
        out[((int64_t)o * S + h) * n + w] = val;
    }
};

// a split: C_obs (k,N), nrm (4,N), scenes by offsets; L formed from u and d
struct ScenesSrc {
    static constexpr bool kComputed = true, kPerRow = false;
    const float *C_obs, *nrm;
    int64_t N;
    float *out;  // (k,N,S) C_pred_refine
    // (= scene_v of et_scene_helpers.inl, word for word; calling it instead changes this kernel's --digest: leave it)
    __device__ void load(float *u, int64_t b, int n, int K, float *red) const {
        const int k = K - 2;
        for (int i = threadIdx.x; i < k * n; i += kSgThreads) u[i] = C_obs[(int64_t)(i / n) * N + b + (i % n)];
        // obs_ori = last observed position - its mean over the scene (model.py:86-90), summed in et_scene_project's order
        float sx = 0.f, sy = 0.f;
        for (int w = threadIdx.x; w < n; w += kSgThreads) {
            sx += nrm[b + w];
            sy += nrm[N + b + w];
        }
        for (int o = 32; o > 0; o >>= 1) {
            sx += __shfl_xor(sx, o);
            sy += __shfl_xor(sy, o);
        }
        if ((threadIdx.x & (kWave - 1)) == 0) {
            red[threadIdx.x / kWave] = sx;
            red[kSgThreads / kWave + threadIdx.x / kWave] = sy;
        }
        __syncthreads();
        float mx = 0.f, my = 0.f;
        for (int w = 0; w < kSgThreads / kWave; ++w) {
            mx += red[w];
            my += red[kSgThreads / kWave + w];
        }
        mx = mx / (float)n;
        my = my / (float)n;
        for (int w = threadIdx.x; w < n; w += kSgThreads) {
            u[k * n + w] = nrm[b + w] - mx;
            u[(k + 1) * n + w] = nrm[N + b + w] - my;
        }
    }
    __device__ int key(int) const { return 0; }
    __device__ bool keep(int, int) const { return true; }
    // L[kk,vv,w] = [vv == w] - (d_v a_hat[vv,w]) d_w  (bridge.py:10-20: D a_hat D with D diagonal)
    __device__ float lap(int kk, int vv, int w, int n, const float *u, const float *d, float uw, float dw, int kw) const {
        const float dist = fabsf(u[kk * n + vv] - uw);
        const float ainv = dist == 0.f || !keep(vv, kw) ? 0.f : 1.0f / dist;
        const float eye = vv == w ? 1.f : 0.f;
        return eye - (d[kk * n + vv] * (ainv + eye)) * dw;
    }
    // tpcnn_ouput's output (o, h, w) -> view (S,k,n) (model.py:144) -> permute(0,2,3,1) (bridge.py:42): (k,N,S)
    __device__ void store(int o, int h, int w, int k, int S, int, int64_t b, float val) const {
        const int r = o * S + h;
        const int s = r / k, t = r - s * k;
        out[((int64_t)t * N + b + w) * S + s] = val;
    }
};

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_stgcnn_workspace_bytes(const et_stgcnn_params *params, int64_t N, int64_t max_scene_n) {
    if (check_params(params) != ET_OK || N < 0 || max_scene_n < 0) return 0;
    return arena_workspace_bytes(arena_per_ped(dims_of(*params)), N, max_scene_n);
}

extern "C" int et_stgcnn_forward_scenes(const et_stgcnn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                        const int32_t *scene_offsets, int n_scenes, float *C_pred_refine,
                                        void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SCENE_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    const ScenesSrc src{C_obs, nrm, N, C_pred_refine};
    const unsigned grid = scene_offsets ? (unsigned)n_scenes : 1u;
    hipLaunchKernelGGL((stgcnn_kernel<ScenesSrc>), dim3(grid), dim3(kSgThreads), kSgLdsBytes, (hipStream_t)stream, src,
                       *params, scene_offsets, N, (float *)workspace, (int64_t)(workspace ? workspace_bytes / 4 : 0),
                       kSgLdsBytes / 4);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

extern "C" int et_stgcnn_forward_graph(const et_stgcnn_params *params, const float *v, const float *a, int64_t N,
                                       float *out, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SCENE_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v || !a || !out) return ET_ERR_INVALID_ARG;
    const ArenaPlace place = arena_place_scene(arena_per_ped(dims_of(*params)), N, workspace, workspace_bytes);
    if (place.status != ET_OK) return place.status;
    const GraphSrc src{v, a, out};
    hipLaunchKernelGGL((stgcnn_kernel<GraphSrc>), dim3(1), dim3(kSgThreads), place.lds_bytes,
                       (hipStream_t)stream, src, *params, nullptr, N, (float *)workspace,
                       (int64_t)(workspace ? workspace_bytes / 4 : 0), place.lds_floats);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

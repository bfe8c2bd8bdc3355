// et_graphtern.hip -- Graph-TERN inference (baseline/graphtern: bridge.py pre-hook, model.py graph_tern_light.forward in eval
// mode with the blocks of stmrgcn.py, bridge.py post-hook) for the ET configuration family (include/eigentraj.h "Graph-TERN
// predictor").
//
// One workgroup per scene; the scene's activations live in an arena of (6T + 3Q) floats per pedestrian:
//   u   (T,n)    the input [C_obs; obs_ori] (S_obs[:, 0]): one channel, T = k+2 "time" rows
//   rel (T,n)    S_obs[:, 1]: rel[0] = 0, rel[t] = u[t] - u[t-1] (read as given in the graph form)
//   d   (4,T,n)  D^-1/2 = 1/sqrt(rowsum(A_r + I)) of every (relation, time row, pedestrian); relations
//                [A_abs, A_rel, 1/A_abs, 1/A_rel] (model.py:7-15), A_abs = |u_i - u_j|, A_rel the same on rel
//   three buffers of Q n floats, Q >= 16 T, that take turns: a block's input x, the gcn output y (16,T,n) after the tcn's
//   PReLU, the contracted rows q; then the epcnn blocks' (rows, channels, n) planes
// in LDS when it fits kSgLdsBytes (S = 20, k = 6: 1728 B per pedestrian, n <= 35), else in the caller's workspace at the
// scene's rows.  The 4 T n^2 graphs are never stored: the O(T n^2) loops form the two distances of a pair and their
// inverses where they are used.  MultiRelationalGCN's einsum('nrtwv,nrctv->nctw', L, conv1x1(x)) is regrouped as in
// et_dmrgcn.hip:
//   y[c,t,w] = sum_r ( sum_ci W[r 16 + c, ci] P[r,ci,t,w] + bias[r 16 + c] P[r,C_in,t,w] ),
//   P[r,j,t,w] = sum_v L[r,t,w,v] X_j[t,v]    (X_j = x[j,t,:], and the ones row j = C_in for the conv bias)
// so with C_in = 1 the pair loop carries eight sums per (t,w) instead of 64.  L[r,t,w,v] = (d_w (A_r[w,v] + [v == w])) d_v,
// the reference's D (A + I) D order (normalizer.py:7-21; its diagonal matrices contribute exact zeros elsewhere).
// A == 0 -> A_inv = 0 is an exact comparison of the fp32 distance, as the reference decides on the same fp32 number; the
// division and the square root are the plain IEEE forms (the build sets no fast-math flag).
// The epcnn convolutions pad by REPLICATION (stmrgcn.py:70, 80), clamped at the scene's own first and last pedestrian.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_v: a scene's input, obs_ori summed in et_scene_project's order
#include "et_stgcnn_core.inl"    // prelu, kSgThreads, kSgLdsBytes, kSgMaxS
#include "et_graphtern_core.inl" // GtDims, the sources, conv33_replicate, gt_relations, gt_check_params

template <class Src>
__device__ __forceinline__ void gt_run_scene(const Src &src, const et_graphtern_params &p, const GtDims &D, int64_t b, int n,
                                             float *ar, float *red, float *out, float *gin, int64_t N) {
    const int T = D.T, k = D.k, S = D.S, H = kGtHidden;
    const int tid = threadIdx.x;
    float *u = ar, *rel = u + T * n, *d = rel + T * n;
    float *x = d + (int64_t)kGtRel * T * n, *y = x + (int64_t)D.qpp * n, *q = y + (int64_t)D.qpp * n;

    src.load(u, rel, b, n, T, red);
    __syncthreads();
    if (Src::kComputed) {
        for (int i = tid; i < T * n; i += kSgThreads) {
            rel[i] = i < n ? 0.f : u[i] - u[i - n];
            if (gin) gin[(int64_t)(i / n) * N + b + (i % n)] = u[i];
        }
        __syncthreads();
    }
    // degrees: the row sums of A_r + I, per relation and time row (>= 1; an overflowed sum gives D^-1/2 = 0)
    for (int i = tid; i < T * n; i += kSgThreads) {
        const int t = i / n, w = i - t * n;
        const float *ut = u + t * n, *rt = rel + t * n;
        const float uw = ut[w], rw = rt[w];
        float s[kGtRel] = {0.f, 0.f, 0.f, 0.f};
        for (int vv = 0; vv < n; ++vv) {
            float A[kGtRel];
            gt_relations(fabsf(uw - ut[vv]), fabsf(rw - rt[vv]), A);
            const float diag = vv == w ? 1.f : 0.f;
#pragma unroll
            for (int r = 0; r < kGtRel; ++r) s[r] += A[r] + diag;
        }
#pragma unroll
        for (int r = 0; r < kGtRel; ++r) {
            const float di = 1.0f / sqrtf(s[r]);
            d[(r * T + t) * n + w] = isinf(di) ? 0.f : di;  // normalizer.py:12
        }
    }
    __syncthreads();

    for (int l = 0; l < D.n_gcn; ++l) {
        const et_graphtern_layer &Ly = p.tp_mrgcns[l];
        const int Cin = l == 0 ? 1 : H;
        const float *xin = l == 0 ? u : x;  // (Cin,T,n)
        const int J = Cin + 1;              // contracted rows per graph: x[ci,t,:] and the ones row (the conv's bias)
        const int ngroups = (J + kGtRows - 1) / kGtRows;
        const int nt = min(T, D.qpp / (kGtRel * J));  // time rows per chunk of q
        for (int t0 = 0; t0 < T; t0 += nt) {
            const int tn = min(nt, T - t0);
            for (int it = tid; it < tn * ngroups * n; it += kSgThreads) {
                const int w = it % n;
                const int rest = it / n;
                const int g = rest % ngroups, tq = rest / ngroups;
                const int t = t0 + tq, j0 = g * kGtRows;
                const float *ut = u + t * n, *rt = rel + t * n;
                const float uw = ut[w], rw = rt[w];
                float dw[kGtRel], acc[kGtRel][kGtRows];
#pragma unroll
                for (int r = 0; r < kGtRel; ++r) {
                    dw[r] = d[(r * T + t) * n + w];
#pragma unroll
                    for (int jj = 0; jj < kGtRows; ++jj) acc[r][jj] = 0.f;
                }
                for (int vv = 0; vv < n; ++vv) {
                    float A[kGtRel], xv[kGtRows];
                    gt_relations(fabsf(uw - ut[vv]), fabsf(rw - rt[vv]), A);
                    const float diag = vv == w ? 1.f : 0.f;
#pragma unroll
                    for (int jj = 0; jj < kGtRows; ++jj) {
                        const int j = j0 + jj;
                        xv[jj] = j < Cin ? xin[(j * T + t) * n + vv] : j == Cin ? 1.f : 0.f;
                    }
#pragma unroll
                    for (int r = 0; r < kGtRel; ++r) {
                        const float lv = (dw[r] * (A[r] + diag)) * d[(r * T + t) * n + vv];
#pragma unroll
                        for (int jj = 0; jj < kGtRows; ++jj) acc[r][jj] = fmaf(xv[jj], lv, acc[r][jj]);
                    }
                }
#pragma unroll
                for (int r = 0; r < kGtRel; ++r)
#pragma unroll
                    for (int jj = 0; jj < kGtRows; ++jj)
                        if (j0 + jj < J) q[((tq * kGtRel + r) * J + j0 + jj) * n + w] = acc[r][jj];
            }
            __syncthreads();
            // the 1x1 convolution on the contracted rows (relation r on channels r 16 + c), then the tcn's PReLU
            for (int it = tid; it < H * tn * n; it += kSgThreads) {
                const int w = it % n;
                const int ct = it / n;
                const int c = ct / tn, tq = ct - c * tn;
                float acc = 0.f;
                for (int r = 0; r < kGtRel; ++r) {
                    const int o = r * H + c;  // stmrgcn.py:21's view
                    const float *qb = q + (int64_t)(tq * kGtRel + r) * J * n;
                    for (int ci = 0; ci < Cin; ++ci) acc = fmaf(Ly.gcn_w[o * Cin + ci], qb[ci * n + w], acc);
                    acc = fmaf(Ly.gcn_b[o], qb[Cin * n + w], acc);
                }
                y[(c * T + t0 + tq) * n + w] = prelu(acc, Ly.tcn_prelu);
            }
            __syncthreads();
        }
        // tcn: (3,1) conv over time (zero padding), + residual -> q; use_mdn: the block's own PReLU is not applied
        // (stmrgcn.py:54).  The last block writes (T,16,n), the permute of model.py:256
        const bool last = l + 1 == D.n_gcn;
        for (int it = tid; it < H * T * n; it += kSgThreads) {
            const int w = it % n;
            const int ct = it / n;
            const int c = ct / T, t = ct - c * T;
            float acc = Ly.tcn_b[c];
            for (int ci = 0; ci < H; ++ci) {
                const float *wc = Ly.tcn_w + ((int64_t)c * H + ci) * 3;
                const float *yc = y + (int64_t)ci * T * n;
                if (t > 0) acc = fmaf(wc[0], yc[(t - 1) * n + w], acc);
                acc = fmaf(wc[1], yc[t * n + w], acc);
                if (t + 1 < T) acc = fmaf(wc[2], yc[(t + 1) * n + w], acc);
            }
            float res;
            if (Ly.res_w) {
                res = Ly.res_b[c];
                for (int ci = 0; ci < Cin; ++ci) res = fmaf(Ly.res_w[c * Cin + ci], xin[(ci * T + t) * n + w], res);
            } else {
                res = xin[it];
            }
            q[last ? (t * H + c) * n + w : it] = acc + res;
        }
        __syncthreads();
        float *tmp = x;
        x = q;
        q = tmp;
    }

    // epcnn blocks over x (rows, 16, n): rows = T into the first block, k afterwards; the last block's channels are S
    for (int j = 0; j < D.n_cnn; ++j) {
        const et_graphtern_epcnn &Ep = p.tpcnns[j];
        const bool last = j + 1 == D.n_cnn;
        const int Rin = j == 0 ? T : k, Cout = last ? S : H;
        for (int it = tid; it < k * H * n; it += kSgThreads) {  // tpcns[0]: the rows as channels, over the (16, n) plane
            const int w = it % n, oh = it / n;
            const int o = oh / H, h = oh - o * H;
            y[it] = prelu(conv33_replicate(x, Rin, H, H, 1, n, Ep.tpcn_w, Ep.tpcn_b, o, h, w), Ep.tpcn_a);
        }
        __syncthreads();
        for (int it = tid; it < k * Cout * n; it += kSgThreads) {  // cpcns[0]: the channels, over the (k, n) plane; + residual
            const int w = it % n, to = it / n;
            const int t = to / Cout, o = to - t * Cout;
            float res;
            if (Ep.rest_w) {  // restconv: 1x1 over the rows (stmrgcn.py:92)
                res = Ep.rest_b[t];
                for (int i = 0; i < Rin; ++i) res = fmaf(Ep.rest_w[t * Rin + i], x[(i * H + o) * n + w], res);
            } else if (Ep.resc_w) {  // rescconv: 1x1 over the channels (stmrgcn.py:89)
                res = Ep.resc_b[o];
                for (int c = 0; c < H; ++c) res = fmaf(Ep.resc_w[o * H + c], x[(t * H + c) * n + w], res);
            } else {
                res = x[it];
            }
            const float val = prelu(conv33_replicate(y, H, 1, k, H, n, Ep.cpcn_w, Ep.cpcn_b, o, t, w), Ep.cpcn_a) + res;
            // (t, o, w) -> transpose(2, 3) (model.py:262) -> (1,k,N,S), which the post-hook squeezes
            if (last) out[((int64_t)t * N + b + w) * S + o] = val;
            else q[it] = val;
        }
        __syncthreads();
        float *tmp = x;
        x = q;
        q = tmp;
    }
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void graphtern_kernel(Src src, et_graphtern_params p, const int32_t *__restrict__ off,
                                                               int64_t N, float *out, float *gin, float *ws,
                                                               int64_t ws_floats, int lds_floats) {
    extern __shared__ float lds[];
    __shared__ float red[2 * kSgThreads / kWave];
    const int64_t b = off ? off[blockIdx.x] : 0;
    const int64_t e = off ? off[blockIdx.x + 1] : N;
    if (e <= b) return;
    const GtDims D = gt_dims_of(p);
    const int64_t per = gt_arena_per_ped(D);
    const int64_t n = e - b;
    if (n <= ET_SCENE_MAX_N && per * n <= lds_floats) {
        gt_run_scene(src, p, D, b, (int)n, lds, red, out, gin, N);
    } else if (n <= ET_SCENE_MAX_N && e * per <= ws_floats) {
        gt_run_scene(src, p, D, b, (int)n, ws + b * per, red, out, gin, N);
    } else {  // fits nowhere: NaN, never an access outside the buffers
        const float nan = __builtin_nanf("");
        for (int64_t t = 0; t < D.k; ++t)
            for (int64_t i = threadIdx.x; i < n * D.S; i += kSgThreads) out[(t * N + b) * D.S + i] = nan;
        if (gin)
            for (int64_t i = threadIdx.x; i < (int64_t)D.T * n; i += kSgThreads) gin[(i / n) * N + b + (i % n)] = nan;
    }
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_graphtern_workspace_bytes(const et_graphtern_params *params, int64_t N, int64_t max_scene_n) {
    if (gt_check_params(params) != ET_OK || N < 0 || max_scene_n < 0) return 0;
    return arena_workspace_bytes(gt_arena_per_ped(gt_dims_of(*params)), N, max_scene_n);
}

extern "C" int et_graphtern_forward_graph(const et_graphtern_params *params, const float *S_obs, int64_t N, float *out,
                                          void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = gt_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SCENE_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!S_obs || !out) return ET_ERR_INVALID_ARG;
    const ArenaPlace place = arena_place_scene(gt_arena_per_ped(gt_dims_of(*params)), N, workspace, workspace_bytes);
    if (place.status != ET_OK) return place.status;
    const GraphSrc src{S_obs};
    hipLaunchKernelGGL((graphtern_kernel<GraphSrc>), dim3(1), dim3(kSgThreads), place.lds_bytes,
                       (hipStream_t)stream, src, *params, nullptr, N, out, nullptr, (float *)workspace,
                       (int64_t)(workspace ? workspace_bytes / 4 : 0), place.lds_floats);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

extern "C" int et_graphtern_forward_scenes(const et_graphtern_params *params, const float *C_obs, const float *nrm, int64_t N,
                                           const int32_t *scene_offsets, int n_scenes, float *C_pred_refine,
                                           float *graph_inputs, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = gt_check_params(params);
    if (rc != ET_OK) return rc;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SCENE_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    const ScenesSrc src{C_obs, nrm, N};
    const unsigned grid = scene_offsets ? (unsigned)n_scenes : 1u;
    hipLaunchKernelGGL((graphtern_kernel<ScenesSrc>), dim3(grid), dim3(kSgThreads), kSgLdsBytes, (hipStream_t)stream, src,
                       *params, scene_offsets, N, C_pred_refine, graph_inputs, (float *)workspace,
                       (int64_t)(workspace ? workspace_bytes / 4 : 0), kSgLdsBytes / 4);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

// et_dmrgcn.hip -- DMRGCN inference (baseline/dmrgcn: bridge.py pre-hook, predictor.py social_dmrgcn.forward in eval mode,
// bridge.py post-hook) for the ET configuration family (include/eigentraj.h "DMRGCN predictor").
//
// One workgroup per scene; the scene's activations live in an arena of (2K + 10K + 3Q) floats per pedestrian:
//   u   (K,n)      the input v = [C_obs; obs_ori]: one channel, K = k+2 "time" rows
//   rel (K,n)      v_rel: rel[0] = 0, rel[t] = u[t] - u[t-1] (scene form only)
//   d   (2,5,K,n)  D^-1/2 = 1/sqrt(1 + count) of every (relation, bin, time row, pedestrian)
//   three buffers of Q n floats, Q >= S K, that take turns: a block's input x (S,K,n), the gcn output y (S,K,n) after the
//   tcn's PReLU, the contracted rows q; then the tpcnn blocks' (k,S,n) planes
// in LDS when it fits kSgLdsBytes (S = 20, k = 6: 2304 B per pedestrian, n <= 26), else in the caller's workspace at the
// scene's rows.  Neither form stores a Laplacian: a pair is in at most ONE bin per relation (the bins are disjoint open
// intervals), so the O(K n^2) loops form the two distances of a pair, find the bin of each and add into that bin's
// accumulator only.  MultiRelationalGCN's einsum('nrtwv,nrctv->nctw', L, conv1x1(x)) summed over both relations is regrouped
//   y[c,t,w] = sum_{r,b} ( sum_ci W_r[b S + c, ci] P[r,b,ci,t,w] + bias_r[b S + c] P[r,b,C_in,t,w] ),
//   P[r,b,j,t,w] = sum_v L[r,b,t,w,v] X_j[t,v]    (X_j = x[j,t,:], and the ones row j = C_in for the conv bias)
// so the pair loop runs over 10 (C_in + 1) rows per (t,w) instead of 10 S: 20 rather than 200 in the first block.
// A pair outside a graph's bin is skipped, where the reference's dense einsum adds 0 x[v]; that product is kept once per
// contracted row (`zero`), so a NaN or inf in one pedestrian's row reaches every pedestrian of its time row as it does there.
// L[r,b,t,w,v] = [v == w] - (d_w (A_b[w,v] + [v == w])) d_v, the reference's D (A + I) D order.
// The bin of a distance is two fp32 comparisons against the split values: the reference's clip_adjacency_matrix decides
// the same way on the same fp32 number, so there is no tolerance band around a split value.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_v: a scene's input, obs_ori summed in et_scene_project's order
#include "et_stgcnn_core.inl"    // conv33, prelu, kSgThreads, kSgLdsBytes, kSgMaxS

#include "et_dmrgcn_core.inl"   // DmDims, bin_of, GraphSrc, ScenesSrc, dm_check_params (shared with et_dmrgcn_train.hip)

template <class Src>
__device__ __forceinline__ void dm_run_scene(const Src &src, const et_dmrgcn_params &p, const DmDims &D, int64_t b, int n,
                                             float *ar, float *red, float *gin, int64_t N) {
    const int K = D.K, k = D.k, S = D.S;
    const int tid = threadIdx.x;
    float *u = ar, *rel = u + K * n, *d = rel + K * n;
    float *x = d + (int64_t)kDmRB * K * n, *y = x + (int64_t)D.qpp * n, *q = y + (int64_t)D.qpp * n;

    src.load(u, b, n, K, red);
    __syncthreads();
    if (Src::kComputed) {
        for (int i = tid; i < K * n; i += kSgThreads) {
            rel[i] = i < n ? 0.f : u[i] - u[i - n];
            if (gin) gin[(int64_t)(i / n) * N + b + (i % n)] = u[i];
        }
        __syncthreads();
    }
    // degrees: 1 + the pairs of row w in bin b, per relation and time row (never 0)
    for (int i = tid; i < K * n; i += kSgThreads) {
        const int t = i / n, w = i - t * n;
        const float uw = u[i], rw = Src::kComputed ? rel[i] : 0.f;
        int cnt[2][kDmBins];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int bb = 0; bb < kDmBins; ++bb) cnt[r][bb] = 0;
        for (int vv = 0; vv < n; ++vv) {
            float dist[2];
            src.pair(t, w, vv, n, K, u, rel, uw, rw, dist);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int bin = bin_of(dist[r], p.split[r]);
#pragma unroll
                for (int bb = 0; bb < kDmBins; ++bb) cnt[r][bb] += bin == bb ? 1 : 0;
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int bb = 0; bb < kDmBins; ++bb) d[((r * kDmBins + bb) * K + t) * n + w] = 1.0f / sqrtf(1.0f + (float)cnt[r][bb]);
    }
    __syncthreads();

    for (int l = 0; l < D.n_st; ++l) {
        const et_dmrgcn_layer &Ly = p.st_dmrgcns[l];
        const int Cin = l == 0 ? 1 : S;
        const float *xin = l == 0 ? u : x;  // (Cin,K,n)
        const int J = Cin + 1;              // contracted rows per graph: x[ci,t,:] and the ones row (the conv's bias)
        const int ngroups = (J + kDmRows - 1) / kDmRows;
        const int nt = min(K, D.qpp / (kDmRB * J));  // time rows per chunk of q
        for (int t0 = 0; t0 < K; t0 += nt) {
            const int tn = min(nt, K - t0);
            for (int it = tid; it < tn * ngroups * n; it += kSgThreads) {
                const int w = it % n;
                const int rest = it / n;
                const int g = rest % ngroups, tq = rest / ngroups;
                const int t = t0 + tq, j0 = g * kDmRows;
                const float uw = u[t * n + w], rw = Src::kComputed ? rel[t * n + w] : 0.f;
                float dw[2][kDmBins], acc[2][kDmBins][kDmRows];
                float zero[kDmRows];  // 0 x[j,t,v] over all v: the einsum multiplies every column by its (mostly zero) entry
#pragma unroll
                for (int jj = 0; jj < kDmRows; ++jj) zero[jj] = 0.f;
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int bb = 0; bb < kDmBins; ++bb) {
                        dw[r][bb] = d[((r * kDmBins + bb) * K + t) * n + w];
#pragma unroll
                        for (int jj = 0; jj < kDmRows; ++jj) acc[r][bb][jj] = 0.f;
                    }
                for (int vv = 0; vv < n; ++vv) {
                    float dist[2], xv[kDmRows];
                    src.pair(t, w, vv, n, K, u, rel, uw, rw, dist);
#pragma unroll
                    for (int jj = 0; jj < kDmRows; ++jj) {
                        const int j = j0 + jj;
                        xv[jj] = j < Cin ? xin[(j * K + t) * n + vv] : j == Cin ? 1.f : 0.f;
                        zero[jj] = fmaf(xv[jj], 0.f, zero[jj]);  // +0 while x is finite; NaN once a column is not
                    }
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const int bin = bin_of(dist[r], p.split[r]);
                        if (vv == w) {  // the diagonal is in every graph: 1 - (d_w (A + 1)) d_w
#pragma unroll
                            for (int bb = 0; bb < kDmBins; ++bb) {
                                const float lv = 1.f - (dw[r][bb] * ((bin == bb ? 1.f : 0.f) + 1.f)) * dw[r][bb];
#pragma unroll
                                for (int jj = 0; jj < kDmRows; ++jj) acc[r][bb][jj] = fmaf(xv[jj], lv, acc[r][bb][jj]);
                            }
                        } else if (bin >= 0) {  // off the diagonal only the pair's own bin has an entry
                            const float dv = d[((r * kDmBins + bin) * K + t) * n + vv];
#pragma unroll
                            for (int bb = 0; bb < kDmBins; ++bb) {
                                const float lv = 0.f - (dw[r][bb] * 1.f) * dv;
#pragma unroll
                                for (int jj = 0; jj < kDmRows; ++jj)
                                    acc[r][bb][jj] = bin == bb ? fmaf(xv[jj], lv, acc[r][bb][jj]) : acc[r][bb][jj];
                            }
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int bb = 0; bb < kDmBins; ++bb)
#pragma unroll
                        for (int jj = 0; jj < kDmRows; ++jj)
                            if (j0 + jj < J)
                                q[((tq * kDmRB + r * kDmBins + bb) * J + j0 + jj) * n + w] = acc[r][bb][jj] + zero[jj];
            }
            __syncthreads();
            // the 1x1 convolutions of both relations on the contracted rows, then the tcn's PReLU
            for (int it = tid; it < S * tn * n; it += kSgThreads) {
                const int w = it % n;
                const int ct = it / n;
                const int c = ct / tn, tq = ct - c * tn;
                float acc = 0.f;
                for (int r = 0; r < 2; ++r) {
                    const float *W = Ly.gcn_w[r], *B = Ly.gcn_b[r];
                    for (int bb = 0; bb < kDmBins; ++bb) {
                        const int o = bb * S + c;  // dmrgcn.py:67's view: channel b S + c
                        const float *qb = q + (int64_t)(tq * kDmRB + r * kDmBins + bb) * J * n;
                        for (int ci = 0; ci < Cin; ++ci) acc = fmaf(W[o * Cin + ci], qb[ci * n + w], acc);
                        acc = fmaf(B[o], qb[Cin * n + w], acc);
                    }
                }
                y[(c * K + t0 + tq) * n + w] = prelu(acc, Ly.tcn_prelu);
            }
            __syncthreads();
        }
        // tcn: (3,1) conv over time, + residual, PReLU -> q; the last block writes (K,S,n), the permute of predictor.py:89
        const bool last = l + 1 == D.n_st;
        for (int it = tid; it < S * K * n; it += kSgThreads) {
            const int w = it % n;
            const int ct = it / n;
            const int c = ct / K, t = ct - c * K;
            float acc = Ly.tcn_b[c];
            for (int ci = 0; ci < S; ++ci) {
                const float *wc = Ly.tcn_w + ((int64_t)c * S + ci) * 3;
                const float *yc = y + (int64_t)ci * K * n;
                if (t > 0) acc = fmaf(wc[0], yc[(t - 1) * n + w], acc);
                acc = fmaf(wc[1], yc[t * n + w], acc);
                if (t + 1 < K) acc = fmaf(wc[2], yc[(t + 1) * n + w], acc);
            }
            float res;
            if (Ly.res_w) {
                res = Ly.res_b[c];
                for (int ci = 0; ci < Cin; ++ci) res = fmaf(Ly.res_w[c * Cin + ci], xin[(ci * K + t) * n + w], res);
            } else {
                res = xin[it];
            }
            q[last ? (t * S + c) * n + w : it] = prelu(acc + res, Ly.prelu);
        }
        __syncthreads();
        float *tmp = x;
        x = q;
        q = tmp;
    }

    // tpcnn blocks over x (K,S,n); planes (k,S,n) from the second convolution on
    const int ko = k * S * n;
    for (int j = 0; j < D.n_tp; ++j) {
        const et_dmrgcn_tpcnn &Tp = p.tpcnns[j];
        const int Cin = j == 0 ? K : k;
        for (int it = tid; it < ko; it += kSgThreads) {  // tpcn[0] + residual
            const int w = it % n, oh = it / n;
            const int o = oh / S, h = oh - o * S;
            float res;
            if (Tp.res_w) {
                res = Tp.res_b[o];
                for (int i = 0; i < Cin; ++i) res = fmaf(Tp.res_w[o * Cin + i], x[(i * S + h) * n + w], res);
            } else {
                res = x[it];
            }
            y[it] = prelu(conv33(x, Cin, S, n, Tp.conv_w[0], Tp.conv_b[0], o, h, w), Tp.conv_a[0]) + res;
        }
        __syncthreads();
        for (int it = tid; it < ko; it += kSgThreads) {  // tpcn[1](x) + x
            const int w = it % n, oh = it / n;
            const int o = oh / S, h = oh - o * S;
            q[it] = prelu(conv33(y, k, S, n, Tp.conv_w[1], Tp.conv_b[1], o, h, w), Tp.conv_a[1]) + y[it];
        }
        __syncthreads();
        for (int it = tid; it < S * n; it += kSgThreads) {  // GTA: Conv2d(S, S, (k,1)) on the (S,k,n) permute: one row
            const int w = it % n, so = it / n;
            float acc = Tp.gta_b[so];
            for (int s = 0; s < S; ++s) {
                const float *wg = Tp.gta_w + ((int64_t)so * S + s) * k;
                for (int t = 0; t < k; ++t) acc = fmaf(wg[t], q[(t * S + s) * n + w], acc);
            }
            y[it] = prelu(acc, Tp.gta_a);
        }
        __syncthreads();
        const bool last = j + 1 == D.n_tp;
        for (int it = tid; it < ko; it += kSgThreads) {  // + x broadcasts the row over the k rows
            const int w = it % n, oh = it / n;
            const int t = oh / S, s = oh - t * S;
            const float val = y[s * n + w] + q[it];
            if (last) src.store(t, s, w, k, S, n, b, val);
            else x[it] = val;
        }
        __syncthreads();
    }
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void dmrgcn_kernel(Src src, et_dmrgcn_params p, const int32_t *__restrict__ off,
                                                            int64_t N, float *gin, float *ws, int64_t ws_floats,
                                                            int lds_floats) {
    extern __shared__ float lds[];
    __shared__ float red[2 * kSgThreads / kWave];
    const int64_t b = off ? off[blockIdx.x] : 0;
    const int64_t e = off ? off[blockIdx.x + 1] : N;
    if (e <= b) return;
    const DmDims D = dm_dims_of(p);
    const int64_t per = dm_arena_per_ped(D);
    const int64_t n = e - b;
    if (n <= ET_SCENE_MAX_N && per * n <= lds_floats) {
        dm_run_scene(src, p, D, b, (int)n, lds, red, gin, N);
    } else if (n <= ET_SCENE_MAX_N && e * per <= ws_floats) {
        dm_run_scene(src, p, D, b, (int)n, ws + b * per, red, gin, N);
    } else {  // fits nowhere: NaN, never an access outside the buffers
        const float nan = __builtin_nanf("");
        for (int64_t i = threadIdx.x; i < (int64_t)D.k * D.S * n; i += kSgThreads) {
            const int w = (int)(i % n), ts = (int)(i / n);
            src.store(ts / D.S, ts % D.S, w, D.k, D.S, (int)n, b, nan);
        }
        if (gin)
            for (int64_t i = threadIdx.x; i < (int64_t)D.K * n; i += kSgThreads) gin[(i / n) * N + b + (i % n)] = nan;
    }
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_dmrgcn_workspace_bytes(const et_dmrgcn_params *params, int64_t N, int64_t max_scene_n) {
    if (dm_check_params(params) != ET_OK || N < 0 || max_scene_n < 0) return 0;
    return arena_workspace_bytes(dm_arena_per_ped(dm_dims_of(*params)), N, max_scene_n);
}

extern "C" int et_dmrgcn_forward_graph(const et_dmrgcn_params *params, const float *v, const float *a, int64_t N,
                                       float *out, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = dm_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SCENE_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v || !a || !out) return ET_ERR_INVALID_ARG;
    const ArenaPlace place = arena_place_scene(dm_arena_per_ped(dm_dims_of(*params)), N, workspace, workspace_bytes);
    if (place.status != ET_OK) return place.status;
    const GraphSrc src{v, a, out};
    hipLaunchKernelGGL((dmrgcn_kernel<GraphSrc>), dim3(1), dim3(kSgThreads), place.lds_bytes,
                       (hipStream_t)stream, src, *params, nullptr, N, nullptr, (float *)workspace,
                       (int64_t)(workspace ? workspace_bytes / 4 : 0), place.lds_floats);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

extern "C" int et_dmrgcn_forward_scenes(const et_dmrgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                        const int32_t *scene_offsets, int n_scenes, float *C_pred_refine,
                                        float *graph_inputs, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = dm_check_params(params);
    if (rc != ET_OK) return rc;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SCENE_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    const ScenesSrc src{C_obs, nrm, N, C_pred_refine};
    const unsigned grid = scene_offsets ? (unsigned)n_scenes : 1u;
    hipLaunchKernelGGL((dmrgcn_kernel<ScenesSrc>), dim3(grid), dim3(kSgThreads), kSgLdsBytes, (hipStream_t)stream, src,
                       *params, scene_offsets, N, graph_inputs, (float *)workspace,
                       (int64_t)(workspace ? workspace_bytes / 4 : 0), kSgLdsBytes / 4);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

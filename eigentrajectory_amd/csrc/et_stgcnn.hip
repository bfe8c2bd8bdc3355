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
#include "et_common.h"

namespace et {
namespace {

constexpr int kSgThreads = 256;         // = et_scene_project's workgroup: the same obs_ori reduction order
constexpr int kSgLdsBytes = 60 * 1024;  // LDS arena of one workgroup (two workgroups per CU)
constexpr int kSgGroup = 16;            // contraction rows per lane
constexpr int kSgMaxS = 64;

struct Dims {
    int K, k, S, n_st, n_tp;
    int qpp;  // floats per pedestrian of q
};

__host__ __device__ inline Dims dims_of(const et_stgcnn_params &p) {
    Dims d{p.seq_len, p.pred_seq_len, p.output_feat, p.n_stgcnn, p.n_txpcnn, 0};
    int q = d.K + 1;  // first layer: one input channel + the ones row
    if (d.n_st > 1 && d.S * d.K + 1 > q) q = d.S * d.K + 1;
    if (d.n_tp >= 3 && d.k * d.S > q) q = d.k * d.S;  // tpcnn residual loop: pong buffer
    d.qpp = q;
    return d;
}

__host__ __device__ inline int64_t arena_per_ped(const Dims &d) { return 2 * d.K + 2 * (int64_t)d.S * d.K + d.qpp; }

// BatchNorm2d in eval mode: (x - mean) / sqrt(var + eps) * w + b, as x * alpha + beta
__device__ __forceinline__ float bn_eval(float x, const float *w, const float *b, const float *m, const float *v, int c,
                                         float eps) {
    const float inv = 1.0f / sqrtf(v[c] + eps);
    const float alpha = w[c] * inv;
    const float beta = b[c] - m[c] * alpha;
    return fmaf(x, alpha, beta);
}

__device__ __forceinline__ float prelu(float x, const float *a) { return x > 0.f ? x : a[0] * x; }

// one scene as the bridge hands it over: v (1,1,K,N), L (K,N,N) given
struct GraphSrc {
    static constexpr bool kComputed = false;
    const float *v, *a;
    float *out;  // (1,S,k,N) raw network output
    __device__ void load(float *u, int64_t, int n, int K, float *) const {
        for (int i = threadIdx.x; i < K * n; i += kSgThreads) u[i] = v[i];
    }
    __device__ float lap(int kk, int vv, int w, int n, const float *, const float *, float, float) const {
        return a[((int64_t)kk * n + vv) * n + w];
    }
    // tpcnn_ouput's output (o, h, w) viewed (1,S,k,N) is the raw output: the same memory
    __device__ void store(int o, int h, int w, int, int S, int n, int64_t, float val) const {
        out[((int64_t)o * S + h) * n + w] = val;
    }
};

// a split: C_obs (k,N), nrm (4,N), scenes by offsets; L formed from u and d
struct ScenesSrc {
    static constexpr bool kComputed = true;
    const float *C_obs, *nrm;
    int64_t N;
    float *out;  // (k,N,S) C_pred_refine
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
    // L[kk,vv,w] = [vv == w] - (d_v a_hat[vv,w]) d_w  (bridge.py:10-20: D a_hat D with D diagonal)
    __device__ float lap(int kk, int vv, int w, int n, const float *u, const float *d, float uw, float dw) const {
        const float dist = fabsf(u[kk * n + vv] - uw);
        const float ainv = dist == 0.f ? 0.f : 1.0f / dist;
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

// 3x3 convolution with padding 1 over the (H = S, W = n) plane: in (Cin,S,n) -> output channel o at (h, w)
__device__ __forceinline__ float conv33(const float *in, int Cin, int S, int n, const float *W, const float *bias, int o,
                                        int h, int w) {
    float acc = bias[o];
    for (int i = 0; i < Cin; ++i) {
        const float *wi = W + ((int64_t)o * Cin + i) * 9;
        const float *pi = in + (int64_t)i * S * n;
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            const int hh = h + dh - 1;
            if (hh < 0 || hh >= S) continue;
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
                const int ww = w + dw - 1;
                if (ww < 0 || ww >= n) continue;
                acc = fmaf(wi[dh * 3 + dw], pi[hh * n + ww], acc);
            }
        }
    }
    return acc;
}

template <class Src>
__device__ __forceinline__ void run_scene(const Src &src, const et_stgcnn_params &p, const Dims &D, int64_t b, int n,
                                          float *ar, float *red) {
    const int K = D.K, k = D.k, S = D.S;
    const int tid = threadIdx.x;
    float *u = ar, *d = u + K * n, *x = d + K * n, *y = x + S * K * n, *q = y + S * K * n;
    const float eps = p.bn_eps;

    src.load(u, b, n, K, red);
    __syncthreads();
    if (Src::kComputed) {  // D = rowsum(a_hat)^-1/2; a_hat = a_inv + I, so every row sums to >= 1 (never the inf case)
        for (int i = tid; i < K * n; i += kSgThreads) {
            const int kk = i / n, vv = i - kk * n;
            const float *ur = u + kk * n;
            const float uv = ur[vv];
            float s = 0.f;
            for (int w = 0; w < n; ++w) {
                const float dist = fabsf(uv - ur[w]);
                const float ainv = dist == 0.f ? 0.f : 1.0f / dist;
                s += ainv + (w == vv ? 1.f : 0.f);
            }
            d[i] = 1.0f / sqrtf(s);
        }
        __syncthreads();
    }

    for (int l = 0; l < D.n_st; ++l) {
        const et_stgcnn_layer &Ly = p.st_gcns[l];
        const int Cin = l == 0 ? 1 : S;
        const float *xin = l == 0 ? u : x;
        const int J = Cin * K + 1;  // contraction rows: x[ci,t,:] and the ones row (the gcn conv's bias)
        const int ngroups = (J + kSgGroup - 1) / kSgGroup;
        const int nkk = min(K, D.qpp / J);  // time rows per chunk
        for (int k0 = 0; k0 < K; k0 += nkk) {
            const int kn = min(nkk, K - k0);
            const int items = kn * ngroups * n;
            for (int it = tid; it < items; it += kSgThreads) {
                const int w = it % n;
                const int rest = it / n;
                const int g = rest % ngroups, kq = rest / ngroups;
                const int kk = k0 + kq;
                const int j0 = g * kSgGroup;
                const float uw = Src::kComputed ? u[kk * n + w] : 0.f;
                const float dw = Src::kComputed ? d[kk * n + w] : 0.f;
                float acc[kSgGroup];
#pragma unroll
                for (int jj = 0; jj < kSgGroup; ++jj) acc[jj] = 0.f;
                for (int vv = 0; vv < n; ++vv) {
                    const float lv = src.lap(kk, vv, w, n, u, d, uw, dw);
#pragma unroll
                    for (int jj = 0; jj < kSgGroup; ++jj) {
                        const int j = j0 + jj;
                        if (j < J) acc[jj] = fmaf(j < J - 1 ? xin[j * n + vv] : 1.f, lv, acc[jj]);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < kSgGroup; ++jj)
                    if (j0 + jj < J) q[((int64_t)kq * J + j0 + jj) * n + w] = acc[jj];
            }
            __syncthreads();
            const bool last = k0 + kn >= K;
            for (int it = tid; it < S * K * n; it += kSgThreads) {
                const int w = it % n;
                const int ct = it / n;
                const int c = ct / K, t = ct - c * K;
                float acc = k0 == 0 ? 0.f : y[it];
                for (int kq = 0; kq < kn; ++kq) {
                    const int o = (k0 + kq) * S + c;  // gcn channel o = kk S + c (model.py:44's view)
                    const float *qk = q + (int64_t)kq * J * n;
                    for (int ci = 0; ci < Cin; ++ci) acc = fmaf(Ly.gcn_w[o * Cin + ci], qk[(ci * K + t) * n + w], acc);
                    acc = fmaf(Ly.gcn_b[o], qk[(J - 1) * n + w], acc);
                }
                if (last) acc = prelu(bn_eval(acc, Ly.bn1_w, Ly.bn1_b, Ly.bn1_mean, Ly.bn1_var, c, eps), Ly.prelu1);
                y[it] = acc;
            }
            __syncthreads();
        }
        // tcn: (3,1) conv over time, BN, + residual, PReLU -> x (in place when the residual is the identity)
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
            acc = bn_eval(acc, Ly.bn2_w, Ly.bn2_b, Ly.bn2_mean, Ly.bn2_var, c, eps);
            float res;
            if (Ly.res_w) {
                res = Ly.res_b[c];
                for (int ci = 0; ci < Cin; ++ci) res = fmaf(Ly.res_w[c * Cin + ci], xin[(ci * K + t) * n + w], res);
                res = bn_eval(res, Ly.res_bn_w, Ly.res_bn_b, Ly.res_bn_mean, Ly.res_bn_var, c, eps);
            } else {
                res = xin[it];
            }
            x[it] = prelu(acc + res, Ly.prelu);
        }
        __syncthreads();
    }

    // tpcnns over x viewed (K, S, n) (model.py:136: a reshape, not a permute)
    const int ko = k * S * n;
    for (int it = tid; it < ko; it += kSgThreads) {
        const int w = it % n, oh = it / n;
        const int o = oh / S, h = oh - o * S;
        y[it] = prelu(conv33(x, K, S, n, p.tpcnn_w[0], p.tpcnn_b[0], o, h, w), p.prelus[0]);
    }
    __syncthreads();
    float *cur = y, *nxt = q;
    for (int j = 1; j < D.n_tp - 1; ++j) {  // model.py:140-141: tpcnns[n_txpcnn - 1] is never used
        for (int it = tid; it < ko; it += kSgThreads) {
            const int w = it % n, oh = it / n;
            const int o = oh / S, h = oh - o * S;
            nxt[it] = prelu(conv33(cur, k, S, n, p.tpcnn_w[j], p.tpcnn_b[j], o, h, w), p.prelus[j]) + cur[it];
        }
        __syncthreads();
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
    for (int it = tid; it < ko; it += kSgThreads) {
        const int w = it % n, oh = it / n;
        const int o = oh / S, h = oh - o * S;
        src.store(o, h, w, k, S, n, b, conv33(cur, k, S, n, p.out_w, p.out_b, o, h, w));
    }
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void stgcnn_kernel(Src src, et_stgcnn_params p, const int32_t *__restrict__ off,
                                                            int64_t N, float *ws, int64_t ws_floats, int lds_floats) {
    extern __shared__ float lds[];
    __shared__ float red[2 * kSgThreads / kWave];
    const int64_t b = off ? off[blockIdx.x] : 0;
    const int64_t e = off ? off[blockIdx.x + 1] : N;
    if (e <= b) return;
    const Dims D = dims_of(p);
    const int64_t per = arena_per_ped(D);
    const int64_t n = e - b;
    if (n <= ET_SCENE_MAX_N && per * n <= lds_floats) {
        run_scene(src, p, D, b, (int)n, lds, red);
    } else if (n <= ET_SCENE_MAX_N && e * per <= ws_floats) {
        run_scene(src, p, D, b, (int)n, ws + b * per, red);
    } else {  // fits nowhere: NaN, never an access outside the buffers
        const float nan = __builtin_nanf("");
        for (int64_t i = threadIdx.x; i < (int64_t)D.k * D.S * n; i += kSgThreads) {
            const int w = (int)(i % n), oh = (int)(i / n);
            src.store(oh / D.S, oh % D.S, w, D.k, D.S, (int)n, b, nan);
        }
    }
}

static int check_params(const et_stgcnn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->input_feat != 1 || p->kernel_size != 3 || p->pred_seq_len < 1 || p->pred_seq_len > ET_MAX_K ||
        p->seq_len != p->pred_seq_len + 2 || p->output_feat < 1 || p->output_feat > kSgMaxS || p->n_stgcnn < 1 ||
        p->n_stgcnn > ET_STGCNN_MAX_LAYERS || p->n_txpcnn < 1 || p->n_txpcnn > ET_STGCNN_MAX_LAYERS)
        return ET_ERR_UNSUPPORTED;
    if (!(p->bn_eps >= 0.f)) return ET_ERR_INVALID_ARG;
    for (int i = 0; i < p->n_stgcnn; ++i) {
        const et_stgcnn_layer &l = p->st_gcns[i];
        if (!l.gcn_w || !l.gcn_b || !l.bn1_w || !l.bn1_b || !l.bn1_mean || !l.bn1_var || !l.prelu1 || !l.tcn_w ||
            !l.tcn_b || !l.bn2_w || !l.bn2_b || !l.bn2_mean || !l.bn2_var || !l.prelu)
            return ET_ERR_INVALID_ARG;
        const int cin = i == 0 ? p->input_feat : p->output_feat;
        const bool res = cin != p->output_feat;  // model.py:90-95: a 1x1 conv + BN only when the widths differ
        if (res != (l.res_w != nullptr)) return ET_ERR_INVALID_ARG;
        if (res && (!l.res_b || !l.res_bn_w || !l.res_bn_b || !l.res_bn_mean || !l.res_bn_var)) return ET_ERR_INVALID_ARG;
    }
    const int used = p->n_txpcnn - 1 > 1 ? p->n_txpcnn - 1 : 1;
    for (int j = 0; j < used; ++j)
        if (!p->tpcnn_w[j] || !p->tpcnn_b[j] || !p->prelus[j]) return ET_ERR_INVALID_ARG;
    if (!p->out_w || !p->out_b) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_stgcnn_workspace_bytes(const et_stgcnn_params *params, int64_t N, int64_t max_scene_n) {
    if (check_params(params) != ET_OK || N < 0 || max_scene_n < 0) return 0;
    const int64_t per = arena_per_ped(dims_of(*params));
    if (per * max_scene_n * 4 <= kSgLdsBytes) return 0;
    return (size_t)(per * N * 4);
}

extern "C" int et_stgcnn_forward_scenes(const et_stgcnn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                        const int32_t *scene_offsets, int n_scenes, float *C_pred_refine,
                                        void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > INT32_MAX || n_scenes < 0) return ET_ERR_INVALID_ARG;
    if (scene_offsets && n_scenes == 0) return N == 0 ? ET_OK : ET_ERR_INVALID_ARG;
    if (!scene_offsets && N > ET_SCENE_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
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
    const int64_t per = arena_per_ped(dims_of(*params));
    const bool in_lds = per * N * 4 <= kSgLdsBytes;
    if (!in_lds && (!workspace || workspace_bytes < (size_t)(per * N * 4))) return ET_ERR_WORKSPACE;
    const GraphSrc src{v, a, out};
    hipLaunchKernelGGL((stgcnn_kernel<GraphSrc>), dim3(1), dim3(kSgThreads), in_lds ? (unsigned)(per * N * 4) : 0u,
                       (hipStream_t)stream, src, *params, nullptr, N, (float *)workspace,
                       (int64_t)(workspace ? workspace_bytes / 4 : 0), in_lds ? (int)(per * N) : 0);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

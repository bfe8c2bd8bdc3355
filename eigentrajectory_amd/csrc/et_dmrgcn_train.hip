// et_dmrgcn_train.hip -- DMRGCN in training mode (include/eigentraj.h "DMRGCN predictor, training"): the forward with
// DropEdge (dropedge.py: every entry of the clipped 0/1 bin tensor kept or zeroed by the caller's keep mask, so the graph is
// no longer symmetric) and the backward pass to every parameter, for the inference family of dm_check_params with
// n_stgcn = 1 (C_in = 1: no gradient passes through a Laplacian) and scenes of at most ET_DMRGCN_TRAIN_MAX_N pedestrians.
// The eval kernel (et_dmrgcn.hip) is untouched; both units take DmDims / bin_of / the sources from et_dmrgcn_core.inl.
//
// Keep mask: uint8 (2,5,K,n,n) indexed [r,b,t,w,v] per scene (scenes form: scene s at 10 K keep_offsets[s], the packed sum of
// n^2); entry != 0 keeps A_b[w,v]; NULL keeps everything.  It is applied where the eval kernel decides "the pair is in bin b":
// in the degree loop (cnt[r,b,t,w] = kept entries of row w, d_w = 1/sqrt(1 + cnt)) and in the contraction loop
// (L[w,v] = [v==w] - (d_w (A'[w,v] + [v==w])) d_v, d_v the column pedestrian's own row degree).  Every other statement of
// the forward, the `zero` term included, is dm_run_scene's in its order: with a NULL or an all-ones mask the output is
// bit-equal to et_dmrgcn_forward_graph / _scenes.
//
// Forward: ONE launch, one workgroup of 256 lanes per scene.  The live operands (u, rel, d, the three rotating buffers) are
// in the LDS arena when the scene fits it (dt_arena_per_ped floats per pedestrian; S = 20, k = 6: n <= 24), else in the
// scene's arena rows of the workspace; what the backward reads is written on the side into the workspace:
//   u (K), P (2,5,2,K) the contraction rows (j = 0: u's row, j = 1: the ones row), yp (S,K) the gcn sum = the tcn PReLU's
//   input, s (S,K) the block PReLU's input, x (K,S) the block's output after the permute, and per tpcnn block j: c0, y, c1, q,
//   o (k,S each: tpcn.0's pre-activation and output, tpcn.1's, the block's output) and z (S) the GTA pre-activation.
// Backward: THREE launches for any N and any number of scenes:
//   1. dmrgcn_train_bwd_kernel     one workgroup per scene walks the dependent chain d out -> ... -> d y with its operands in
//                                  the same arena (three buffers + two GTA rows) and leaves per tpcnn block dq, dy (k,S) and
//                                  dg (S), then dx (K,S) and dy (S,K), in the workspace
//   2. dmrgcn_train_wgrad_kernel   grid (scenes, kDtChunks): every parameter-gradient element of a scene is one wavefront's
//                                  sum; the scene's 64 wavefronts take the elements round robin -> the scene's partial
//   3. scene_grad_reduce_kernel    grads[e] = the scenes' partials in ascending order, the first one copied
//                                  (et_train_sums.inl, which the three scene training units share)
// Fixed orders (no atomics; two runs agree bit for bit, a one-scene scenes call equals the graph call): wave_sum of
// et_train_sums.inl (lane l adds positions l, l + 64, ... ascending from +0, then the xor butterfly 32 .. 1); every other
// sum is one lane's ascending fmaf chain.  Every PReLU branches on the kept fp32 word in both passes.
// A scene of more than ET_DMRGCN_TRAIN_MAX_N pedestrians is not computed: NaN outputs, no gradient.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"
#include "et_stgcnn_core.inl"
#include "et_dmrgcn_core.inl"

enum {
    F_U, F_P, F_YP, F_S, F_X, F_TP, F_DTP, F_DX, F_DY, F_ARENA, F_PER, F_TP_STRIDE, F_DTP_STRIDE, F_PARTIALS, F_GRADS, F_TOTAL,
    F_COUNT
};
static_assert(F_COUNT == ET_DMRGCN_TRAIN_LAYOUT_FIELDS, "et_dmrgcn_train_layout's field count");

#include "et_train_sums.inl"

constexpr int kDtMaxN = ET_DMRGCN_TRAIN_MAX_N;
constexpr int kDtChunks = 16;                     // weight-gradient workgroups per scene
constexpr int kDtWaves = kDtChunks * kTrWaves;    // ... and its wavefronts

// where every parameter's gradient starts in the flat buffer (state_dict order)
struct DtGradOff {
    int gcn_w[2], gcn_b[2], tcn_a, tcn_w, tcn_b, res_w, res_b, prelu;
    struct {
        int w[2], b[2], a[2], gta_w, gta_b, gta_a, res_w, res_b;
    } tp[ET_DMRGCN_MAX_TPCNN];
    int total;
};

__host__ __device__ inline DtGradOff dt_grad_off(const DmDims &D) {
    DtGradOff g{};
    const int S = D.S, K = D.K, k = D.k;
    int at = 0;
    auto take = [&](int cnt) {
        const int o = at;
        at += cnt;
        return o;
    };
    for (int r = 0; r < 2; ++r) g.gcn_w[r] = take(kDmBins * S), g.gcn_b[r] = take(kDmBins * S);
    g.tcn_a = take(1), g.tcn_w = take(S * S * 3), g.tcn_b = take(S);
    if (S != 1) g.res_w = take(S), g.res_b = take(S);
    g.prelu = take(1);
    for (int j = 0; j < D.n_tp; ++j) {
        for (int m = 0; m < 2; ++m)
            g.tp[j].w[m] = take(k * (j == 0 && m == 0 ? K : k) * 9), g.tp[j].b[m] = take(k), g.tp[j].a[m] = take(1);
        g.tp[j].gta_w = take(S * S * k), g.tp[j].gta_b = take(S), g.tp[j].gta_a = take(1);
        if (j == 0) g.tp[j].res_w = take(k * K), g.tp[j].res_b = take(k);
    }
    g.total = at;
    return g;
}

// the arena of both passes: dm_run_scene's, and room for the backward's two GTA rows behind its three buffers
__host__ __device__ inline int64_t dt_arena_per_ped(const DmDims &D) { return dm_arena_per_ped(D) + 2 * D.S; }

__host__ __device__ inline TrainLayout dt_layout(const DmDims &D, int64_t N, int64_t n_scenes) {
    TrainLayout L{};
    const int64_t SK = (int64_t)D.S * D.K, kS = (int64_t)D.k * D.S;
    int64_t at = 0;
    auto take = [&](int f, int64_t cnt) {
        L.o[f] = at;
        at += cnt;
    };
    L.o[F_TP_STRIDE] = 5 * kS + D.S;
    L.o[F_DTP_STRIDE] = 2 * kS + D.S;
    take(F_U, D.K), take(F_P, (int64_t)kDmRB * 2 * D.K), take(F_YP, SK), take(F_S, SK), take(F_X, SK);
    take(F_TP, D.n_tp * L.o[F_TP_STRIDE]), take(F_DTP, D.n_tp * L.o[F_DTP_STRIDE]);
    take(F_DX, SK), take(F_DY, SK), take(F_ARENA, dt_arena_per_ped(D));
    layout_tail(L, at, N * at, dt_grad_off(D).total, n_scenes);
    return L;
}

// a scene's fields in the workspace
struct DtScene : TrainScene {
    int64_t tp_stride, dtp_stride;  // x n: one tpcnn block's kept values / gradients
};

__device__ __forceinline__ DtScene dt_scene(float *ws, const TrainLayout &L, int64_t b, int n, int scene) {
    return {train_scene(ws, L, b, n, scene), L.o[F_TP_STRIDE] * n, L.o[F_DTP_STRIDE] * n};
}

// block j's kept values: c0, y, c1, q, o (k,S,n each), z (S,n); its gradients: dq, dy (k,S,n), dg (S,n)
struct DtBlock {
    float *c0, *y, *c1, *q, *o, *z, *dq, *dy, *dg;
};

__device__ __forceinline__ DtBlock dt_block(const DtScene &W, int j, int ko) {
    DtBlock B;
    float *t = W.f[F_TP] + j * W.tp_stride, *d = W.f[F_DTP] + j * W.dtp_stride;
    const int64_t p = ko;
    B.c0 = t, B.y = t + p, B.c1 = t + 2 * p, B.q = t + 3 * p, B.o = t + 4 * p, B.z = t + 5 * p;
    B.dq = d, B.dy = d + p, B.dg = d + 2 * p;
    return B;
}

// the training sources: the eval unit's, with where an output / d_out entry (t, s, w) lies
struct TrainGraphSrc : GraphSrc {
    const float *d_out;
    __device__ int64_t at(int t, int s, int w, int k, int, int n, int64_t) const { return ((int64_t)s * k + t) * n + w; }
};
struct TrainScenesSrc : ScenesSrc {
    const float *d_out;
    __device__ int64_t at(int t, int s, int w, int, int S, int, int64_t b) const { return ((int64_t)t * N + b + w) * S + s; }
};

// the forward of one scene: dm_run_scene's statements for n_stgcn = 1 with the keep mask, every kept value written on the side
template <class Src>
__device__ __forceinline__ void dt_forward_scene(const Src &src, const et_dmrgcn_params &p, const DmDims &D, int64_t b, int n,
                                                 float *ar, float *red, const DtScene &W, const uint8_t *keep) {
    const int K = D.K, k = D.k, S = D.S;
    const int tid = threadIdx.x;
    float *u = ar, *rel = u + K * n, *d = rel + K * n;
    float *x = d + (int64_t)kDmRB * K * n, *y = x + (int64_t)D.qpp * n, *q = y + (int64_t)D.qpp * n;
    // keep[r,bin,t,w,vv]; a NULL mask keeps everything
    auto kept = [&](int r, int bin, int t, int w, int vv) {
        return !keep || keep[(((int64_t)(r * kDmBins + bin) * K + t) * n + w) * n + vv] != 0;
    };

    src.load(u, b, n, K, red);
    __syncthreads();
    for (int i = tid; i < K * n; i += kSgThreads) {
        if (Src::kComputed) rel[i] = i < n ? 0.f : u[i] - u[i - n];
        W.f[F_U][i] = u[i];
    }
    __syncthreads();
    // degrees: 1 + the KEPT pairs of row w in bin b, per relation and time row (never 0)
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
                int bin = bin_of(dist[r], p.split[r]);
                if (bin >= 0 && !kept(r, bin, t, w, vv)) bin = -1;
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

    const et_dmrgcn_layer &Ly = p.st_dmrgcns[0];
    {
        constexpr int Cin = 1, J = 2;
        const float *xin = u;
        const int nt = min(K, D.qpp / (kDmRB * J));  // time rows per chunk of q
        float *Pk = W.f[F_P], *ypk = W.f[F_YP];
        for (int t0 = 0; t0 < K; t0 += nt) {
            const int tn = min(nt, K - t0);
            for (int it = tid; it < tn * n; it += kSgThreads) {
                const int w = it % n;
                const int tq = it / n;
                const int t = t0 + tq;
                const float uw = u[t * n + w], rw = Src::kComputed ? rel[t * n + w] : 0.f;
                float dw[2][kDmBins], acc[2][kDmBins][kDmRows];
                float zero[kDmRows];  // 0 x[j,t,v] over all v, the dropped and the out-of-bin ones as well
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
                    xv[0] = xin[t * n + vv];
                    xv[1] = 1.f;
#pragma unroll
                    for (int jj = 0; jj < kDmRows; ++jj) zero[jj] = fmaf(xv[jj], 0.f, zero[jj]);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        int bin = bin_of(dist[r], p.split[r]);
                        if (bin >= 0 && !kept(r, bin, t, w, vv)) bin = -1;
                        if (vv == w) {  // the diagonal is in every graph, + I after the draw: 1 - (d_w (A' + 1)) d_w
#pragma unroll
                            for (int bb = 0; bb < kDmBins; ++bb) {
                                const float lv = 1.f - (dw[r][bb] * ((bin == bb ? 1.f : 0.f) + 1.f)) * dw[r][bb];
#pragma unroll
                                for (int jj = 0; jj < kDmRows; ++jj) acc[r][bb][jj] = fmaf(xv[jj], lv, acc[r][bb][jj]);
                            }
                        } else if (bin >= 0) {  // off the diagonal only the pair's own bin has an entry, if it is kept
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
                        for (int jj = 0; jj < kDmRows; ++jj) {
                            const float pv = acc[r][bb][jj] + zero[jj];
                            q[((tq * kDmRB + r * kDmBins + bb) * J + jj) * n + w] = pv;
                            Pk[(((int64_t)(r * kDmBins + bb) * J + jj) * K + t) * n + w] = pv;
                        }
            }
            __syncthreads();
            // the 1x1 convolutions of both relations on the contracted rows, then the tcn's PReLU
            for (int it = tid; it < S * tn * n; it += kSgThreads) {
                const int w = it % n;
                const int ct = it / n;
                const int c = ct / tn, tq = ct - c * tn;
                float acc = 0.f;
                for (int r = 0; r < 2; ++r) {
                    const float *Wr = Ly.gcn_w[r], *Br = Ly.gcn_b[r];
                    for (int bb = 0; bb < kDmBins; ++bb) {
                        const int o = bb * S + c;
                        const float *qb = q + (int64_t)(tq * kDmRB + r * kDmBins + bb) * J * n;
                        for (int ci = 0; ci < Cin; ++ci) acc = fmaf(Wr[o * Cin + ci], qb[ci * n + w], acc);
                        acc = fmaf(Br[o], qb[Cin * n + w], acc);
                    }
                }
                ypk[(c * K + t0 + tq) * n + w] = acc;
                y[(c * K + t0 + tq) * n + w] = prelu(acc, Ly.tcn_prelu);
            }
            __syncthreads();
        }
        // tcn: (3,1) conv over time, + residual, PReLU -> q as (K,S,n), the permute of predictor.py:89
        float *sk = W.f[F_S], *xk = W.f[F_X];
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
            const float sv = acc + res;
            const float xv = prelu(sv, Ly.prelu);
            sk[it] = sv;
            q[(t * S + c) * n + w] = xv;
            xk[(t * S + c) * n + w] = xv;
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
        const DtBlock B = dt_block(W, j, ko);
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
            const float cv = conv33(x, Cin, S, n, Tp.conv_w[0], Tp.conv_b[0], o, h, w);
            const float yv = prelu(cv, Tp.conv_a[0]) + res;
            B.c0[it] = cv;
            B.y[it] = yv;
            y[it] = yv;
        }
        __syncthreads();
        for (int it = tid; it < ko; it += kSgThreads) {  // tpcn[1](x) + x
            const int w = it % n, oh = it / n;
            const int o = oh / S, h = oh - o * S;
            const float cv = conv33(y, k, S, n, Tp.conv_w[1], Tp.conv_b[1], o, h, w);
            const float qv = prelu(cv, Tp.conv_a[1]) + y[it];
            B.c1[it] = cv;
            B.q[it] = qv;
            q[it] = qv;
        }
        __syncthreads();
        for (int it = tid; it < S * n; it += kSgThreads) {  // GTA: Conv2d(S, S, (k,1)) on the (S,k,n) permute: one row
            const int w = it % n, so = it / n;
            float acc = Tp.gta_b[so];
            for (int s = 0; s < S; ++s) {
                const float *wg = Tp.gta_w + ((int64_t)so * S + s) * k;
                for (int t = 0; t < k; ++t) acc = fmaf(wg[t], q[(t * S + s) * n + w], acc);
            }
            B.z[it] = acc;
            y[it] = prelu(acc, Tp.gta_a);
        }
        __syncthreads();
        const bool last = j + 1 == D.n_tp;
        for (int it = tid; it < ko; it += kSgThreads) {  // + x broadcasts the row over the k rows
            const int w = it % n, oh = it / n;
            const int t = oh / S, s = oh - t * S;
            const float val = y[s * n + w] + q[it];
            B.o[it] = val;
            if (last) src.store(t, s, w, k, S, n, b, val);
            else x[it] = val;
        }
        __syncthreads();
    }
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void dmrgcn_train_fwd_kernel(Src src, et_dmrgcn_params p,
                                                                      const int32_t *__restrict__ off, int64_t N,
                                                                      const uint8_t *__restrict__ keep,
                                                                      const int64_t *__restrict__ keep_off, float *ws,
                                                                      TrainLayout L) {
    extern __shared__ float lds[];
    __shared__ float red[2 * kSgThreads / kWave];
    const SceneRows R = scene_rows(off, N);
    if (R.empty()) return;
    const DmDims D = dm_dims_of(p);
    const int64_t b = R.b, n = R.n();
    if (n > kDtMaxN) {  // not computed: NaN
        nan_scene(D.k, D.S, n, [&](int t, int s, int w, float nan) { src.store(t, s, w, D.k, D.S, (int)n, b, nan); });
        return;
    }
    const DtScene W = dt_scene(ws, L, b, (int)n, blockIdx.x);
    const uint8_t *kp = keep ? keep + (keep_off ? keep_off[blockIdx.x] : 0) * kDmRB * D.K : nullptr;
    float *ar = dt_arena_per_ped(D) * n * 4 <= kSgLdsBytes ? lds : W.f[F_ARENA];
    dt_forward_scene(src, p, D, b, (int)n, ar, red, W, kp);
}

// launch 1 of the backward: the activation gradients of one scene
template <class Src>
__global__ __launch_bounds__(kSgThreads) void dmrgcn_train_bwd_kernel(Src src, et_dmrgcn_params p,
                                                                      const int32_t *__restrict__ off, int64_t N, float *ws,
                                                                      TrainLayout L) {
    extern __shared__ float lds[];
    const SceneRows R = scene_rows(off, N);
    if (R.empty() || R.n() > kDtMaxN) return;
    const int64_t b = R.b;
    const int n = (int)R.n();
    const DmDims D = dm_dims_of(p);
    const int K = D.K, k = D.k, S = D.S, tid = threadIdx.x;
    const DtScene W = dt_scene(ws, L, b, n, blockIdx.x);
    float *ar = dt_arena_per_ped(D) * n * 4 <= kSgLdsBytes ? lds : W.f[F_ARENA];
    float *A = ar, *Bf = A + (int64_t)D.qpp * n, *C = Bf + (int64_t)D.qpp * n;
    float *dg = C + (int64_t)D.qpp * n, *dz = dg + S * n;
    const int ko = k * S * n;

    for (int it = tid; it < ko; it += kSgThreads) {
        const int w = it % n, oh = it / n;
        const int t = oh / S, s = oh - t * S;
        A[it] = src.d_out[src.at(t, s, w, k, S, n, b)];
    }
    __syncthreads();
    for (int j = D.n_tp - 1; j >= 0; --j) {  // o = g(q) + q, q = prelu(c1(y)) + y, y = prelu(c0(x)) + res(x); A = d o
        const et_dmrgcn_tpcnn &Tp = p.tpcnns[j];
        const DtBlock B = dt_block(W, j, ko);
        const int Cin = j == 0 ? K : k;
        for (int it = tid; it < S * n; it += kSgThreads) {  // the GTA row was added to all k time rows
            const int w = it % n, s = it / n;
            float acc = 0.f;
            for (int t = 0; t < k; ++t) acc += A[(t * S + s) * n + w];
            dg[it] = acc;
            B.dg[it] = acc;
            dz[it] = acc * slope(B.z[it], Tp.gta_a);
        }
        __syncthreads();
        for (int it = tid; it < ko; it += kSgThreads) {  // d q = d o + Wg^T d z;  d c1
            const int w = it % n, oh = it / n;
            const int t = oh / S, s = oh - t * S;
            float acc = A[it];
            for (int so = 0; so < S; ++so) acc = fmaf(Tp.gta_w[((int64_t)so * S + s) * k + t], dz[so * n + w], acc);
            Bf[it] = acc;
            B.dq[it] = acc;
            C[it] = acc * slope(B.c1[it], Tp.conv_a[1]);
        }
        __syncthreads();
        for (int it = tid; it < ko; it += kSgThreads) {  // d y = d q + conv1^T d c1;  d c0 (over d q's own entry)
            const int w = it % n, ih = it / n;
            const int i = ih / S, h = ih - i * S;
            const float v = Bf[it] + conv33_dx(C, k, k, S, n, Tp.conv_w[1], i, h, w);
            A[it] = v;
            B.dy[it] = v;
            Bf[it] = v * slope(B.c0[it], Tp.conv_a[0]);
        }
        __syncthreads();
        float *dxk = W.f[F_DX];
        for (int it = tid; it < Cin * S * n; it += kSgThreads) {  // d x = conv0^T d c0 + res^T d y
            const int w = it % n, ih = it / n;
            const int i = ih / S, h = ih - i * S;
            const float v = conv33_dx(Bf, k, Cin, S, n, Tp.conv_w[0], i, h, w);
            float r;
            if (Tp.res_w) {
                r = 0.f;
                for (int o = 0; o < k; ++o) r = fmaf(Tp.res_w[o * Cin + i], A[(o * S + h) * n + w], r);
            } else {
                r = A[it];
            }
            C[it] = r + v;
            if (j == 0) dxk[it] = r + v;
        }
        __syncthreads();
        float *tmp = A;
        A = C;
        C = tmp;
    }
    // A = d x (K,S,n).  The block's PReLU on s (S,K,n), then the (3,1) conv's transpose -> d y
    const et_dmrgcn_layer &Ly = p.st_dmrgcns[0];
    const float *sk = W.f[F_S];
    for (int it = tid; it < S * K * n; it += kSgThreads) {
        const int w = it % n;
        const int ct = it / n;
        const int c = ct / K, t = ct - c * K;
        Bf[it] = A[(t * S + c) * n + w] * slope(sk[it], Ly.prelu);
    }
    __syncthreads();
    float *dyk = W.f[F_DY];
    const int cnt = K * n;
    for (int it = tid; it < S * K * n; it += kSgThreads) {
        const int w = it % n;
        const int ct = it / n;
        const int ci = ct / K, t = ct - ci * K;
        float acc = 0.f;
        for (int c = 0; c < S; ++c) {
            const float *wc = Ly.tcn_w + ((int64_t)c * S + ci) * 3;
            const float *dc = Bf + (int64_t)c * cnt;
            if (t + 1 < K) acc = fmaf(wc[0], dc[(t + 1) * n + w], acc);
            acc = fmaf(wc[1], dc[t * n + w], acc);
            if (t > 0) acc = fmaf(wc[2], dc[(t - 1) * n + w], acc);
        }
        dyk[it] = acc;
    }
}

// d W (Cout,Cin,3,3) of out = conv33(in) with d out = dsrc slope(pre): item oi = one (o, i) pair, its nine taps in one pass
__device__ __forceinline__ void dt_conv33_dw(float *dst, int oi, const float *dsrc, const float *pre, const float *a,
                                             const float *in, int Cin, int S, int n) {
    const int i = oi % Cin, o = oi / Cin;
    const float *dyo = dsrc + (int64_t)o * S * n, *pro = pre + (int64_t)o * S * n, *ini = in + (int64_t)i * S * n;
    wave_sum_taps<9>(dst + (int64_t)oi * 9, S * n, [&](int pp, int tap) {
        const int h = pp / n, w = pp - h * n;
        const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
        if (hh < 0 || hh >= S || ww < 0 || ww >= n) return 0.f;
        return (dyo[pp] * slope(pro[pp], a)) * ini[hh * n + ww];
    });
}

// launch 2 of the backward: the parameter gradients of one scene, grid (scenes, kDtChunks)
__global__ __launch_bounds__(kSgThreads) void dmrgcn_train_wgrad_kernel(et_dmrgcn_params p, const int32_t *__restrict__ off,
                                                                        int64_t N, float *ws, TrainLayout L) {
    const SceneRows R = scene_rows(off, N);
    if (R.empty() || R.n() > kDtMaxN) return;
    const int64_t b = R.b;
    const int n = (int)R.n();
    const DmDims D = dm_dims_of(p);
    const int K = D.K, k = D.k, S = D.S;
    const DtScene W = dt_scene(ws, L, b, n, blockIdx.x);
    const int wv = blockIdx.y * kTrWaves + threadIdx.x / kWave;
    const int cnt = K * n, SKn = S * K * n, Sn = S * n, ko = k * S * n;
    const et_dmrgcn_layer &Ly = p.st_dmrgcns[0];
    float *gr = W.part;
    const float *u = W.f[F_U], *Pk = W.f[F_P], *yp = W.f[F_YP], *sk = W.f[F_S], *xk = W.f[F_X], *dx = W.f[F_DX], *dy = W.f[F_DY];
    int start = 0;  // items so far (the round robin's phase)
    int at = 0;     // gradient floats so far: the segments below come in dt_grad_off's (the state_dict's) order
    auto take = [&](int cnt) {
        float *dst = gr + at;
        at += cnt;
        return dst;
    };

    // d s[c,(t,w)] = d x[t,c,w] slope(s);  d yp = d y slope(yp)
    auto ds = [&](int c, int pp) {
        const int t = pp / n, w = pp - t * n;
        return dx[(t * S + c) * n + w] * slope(sk[(int64_t)c * cnt + pp], Ly.prelu);
    };
    auto dyp = [&](int c, int pp) { return dy[(int64_t)c * cnt + pp] * slope(yp[(int64_t)c * cnt + pp], Ly.tcn_prelu); };
    // the gcn through the kept contraction rows: channel o = b S + c reads P[r,b,0] (weight) and P[r,b,1] (bias)
    for (int r = 0; r < 2; ++r)
        for (int jj = 0; jj < 2; ++jj) {
            float *dst = take(kDmBins * S);
            segment<kDtWaves>(start, kDmBins * S, wv, [&](int o) {
                const int bb = o / S, c = o - bb * S;
                const float *Pr = Pk + ((int64_t)(r * kDmBins + bb) * 2 + jj) * cnt;
                sum_to(dst + o, cnt, [&](int pp) { return dyp(c, pp) * Pr[pp]; });
            });
        }
    float *d_tcn_a = take(1), *d_tcn_w = take(S * S * 3), *d_tcn_b = take(S);
    float *d_res_w = S != 1 ? take(S) : nullptr, *d_res_b = S != 1 ? take(S) : nullptr;
    float *d_prelu = take(1);
    segment<kDtWaves>(start, 1, wv, [&](int) { sum_to(d_tcn_a, SKn, [&](int pp) { return dy[pp] * neg_part(yp[pp]); }); });
    segment<kDtWaves>(start, S * S, wv, [&](int cc) {  // the (3,1) conv on y = prelu(yp)
        const int ci = cc % S, c = cc / S;
        const float *yc = yp + (int64_t)ci * cnt;
        wave_sum_taps<3>(d_tcn_w + cc * 3, cnt, [&](int pp, int tap) {
            const int tt = pp / n + tap - 1;
            if (tt < 0 || tt >= K) return 0.f;
            return ds(c, pp) * prelu(yc[pp + (tap - 1) * n], Ly.tcn_prelu);
        });
    });
    segment<kDtWaves>(start, S, wv, [&](int c) { sum_to(d_tcn_b + c, cnt, [&](int pp) { return ds(c, pp); }); });
    if (S != 1) {  // the residual 1x1 conv from u
        segment<kDtWaves>(start, S, wv, [&](int c) { sum_to(d_res_w + c, cnt, [&](int pp) { return ds(c, pp) * u[pp]; }); });
        segment<kDtWaves>(start, S, wv, [&](int c) { sum_to(d_res_b + c, cnt, [&](int pp) { return ds(c, pp); }); });
    }
    segment<kDtWaves>(start, 1, wv, [&](int) {
        sum_to(d_prelu, SKn, [&](int pp) {
            const int w = pp % n, ct = pp / n;
            const int c = ct / K, t = ct - c * K;
            return dx[(t * S + c) * n + w] * neg_part(sk[pp]);
        });
    });
    for (int j = 0; j < D.n_tp; ++j) {
        const et_dmrgcn_tpcnn &Tp = p.tpcnns[j];
        const DtBlock B = dt_block(W, j, ko);
        const int Cin = j == 0 ? K : k;
        const float *xin = j == 0 ? xk : dt_block(W, j - 1, ko).o;
        for (int m = 0; m < 2; ++m) {  // tpcn.m: d pre = d out slope(pre), out = prelu(pre) + ...
            const float *dsrc = m ? B.dq : B.dy, *pre = m ? B.c1 : B.c0, *in = m ? B.y : xin;
            const float *a = Tp.conv_a[m];
            const int Ci = m ? k : Cin;
            float *d_w = take(k * Ci * 9), *d_b = take(k), *d_a = take(1);
            segment<kDtWaves>(start, k * Ci, wv, [&](int oi) { dt_conv33_dw(d_w, oi, dsrc, pre, a, in, Ci, S, n); });
            segment<kDtWaves>(start, k, wv, [&](int o) {
                sum_to(d_b + o, Sn, [&](int pp) { return dsrc[(int64_t)o * Sn + pp] * slope(pre[(int64_t)o * Sn + pp], a); });
            });
            segment<kDtWaves>(start, 1, wv,
                              [&](int) { sum_to(d_a, ko, [&](int pp) { return dsrc[pp] * neg_part(pre[pp]); }); });
        }
        float *d_gw = take(S * S * k), *d_gb = take(S), *d_ga = take(1);
        segment<kDtWaves>(start, S * S * k, wv, [&](int el) {  // d Wg[so,s,t] = sum_w d z[so,w] q[t,s,w]
            const int t = el % k, ss = el / k;
            const int s = ss % S, so = ss / S;
            const float *dgo = B.dg + (int64_t)so * n, *zo = B.z + (int64_t)so * n, *qr = B.q + (int64_t)(t * S + s) * n;
            sum_to(d_gw + el, n, [&](int w) { return (dgo[w] * slope(zo[w], Tp.gta_a)) * qr[w]; });
        });
        segment<kDtWaves>(start, S, wv, [&](int so) {
            sum_to(d_gb + so, n, [&](int w) { return B.dg[(int64_t)so * n + w] * slope(B.z[(int64_t)so * n + w], Tp.gta_a); });
        });
        segment<kDtWaves>(start, 1, wv, [&](int) { sum_to(d_ga, Sn, [&](int pp) { return B.dg[pp] * neg_part(B.z[pp]); }); });
        if (j == 0) {  // the residual 1x1 conv (K -> k) sees d y
            float *d_rw = take(k * K), *d_rb = take(k);
            segment<kDtWaves>(start, k * K, wv, [&](int oi) {
                const int i = oi % K, o = oi / K;
                sum_to(d_rw + oi, Sn, [&](int pp) { return B.dy[(int64_t)o * Sn + pp] * xin[(int64_t)i * Sn + pp]; });
            });
            segment<kDtWaves>(start, k, wv,
                              [&](int o) { sum_to(d_rb + o, Sn, [&](int pp) { return B.dy[(int64_t)o * Sn + pp]; }); });
        }
    }
}

static int dt_check_params(const et_dmrgcn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->n_stgcn != 1) return ET_ERR_UNSUPPORTED;  // deeper stacks send a gradient through the Laplacians
    return dm_check_params(p);
}

template <class Src>
static int dt_forward(const Src &src, const et_dmrgcn_params *p, const int32_t *off, int ns, int64_t N, const uint8_t *keep,
                      const int64_t *keep_off, void *workspace, const TrainLayout &L, et_stream_t stream) {
    hipLaunchKernelGGL((dmrgcn_train_fwd_kernel<Src>), dim3((unsigned)ns), dim3(kSgThreads), kSgLdsBytes, (hipStream_t)stream,
                       src, *p, off, N, keep, keep_off, (float *)workspace, L);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

template <class Src>
static int dt_backward(const Src &src, const et_dmrgcn_params *p, const int32_t *off, int ns, int64_t N, float *grads,
                       void *workspace, const TrainLayout &L, et_stream_t stream) {
    if (N > 0) {
        hipLaunchKernelGGL((dmrgcn_train_bwd_kernel<Src>), dim3((unsigned)ns), dim3(kSgThreads), kSgLdsBytes,
                           (hipStream_t)stream, src, *p, off, N, (float *)workspace, L);
        ET_LAUNCH_CHECK();
        hipLaunchKernelGGL(dmrgcn_train_wgrad_kernel, dim3((unsigned)ns, kDtChunks), dim3(kSgThreads), 0, (hipStream_t)stream,
                           *p, off, N, (float *)workspace, L);
        ET_LAUNCH_CHECK();
    }
    return scene_grad_reduce((const float *)workspace + L.o[F_PARTIALS], L.o[F_GRADS], kDtMaxN, off, ns, N, grads, stream);
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_dmrgcn_train_workspace_bytes(const et_dmrgcn_params *params, int64_t N, int n_scenes) {
    if (dt_check_params(params) != ET_OK || N <= 0 || n_scenes < 1) return 0;
    return (size_t)dt_layout(dm_dims_of(*params), N, n_scenes).o[F_TOTAL] * 4;
}

extern "C" int64_t et_dmrgcn_grad_floats(const et_dmrgcn_params *params) {
    if (dt_check_params(params) != ET_OK) return 0;
    return dt_grad_off(dm_dims_of(*params)).total;
}

extern "C" int et_dmrgcn_train_layout(const et_dmrgcn_params *params, int64_t N, int n_scenes, int64_t *offsets,
                                      int n_offsets) {
    const int rc = dt_check_params(params);
    if (rc != ET_OK) return rc;
    return layout_out(N, n_scenes, offsets, n_offsets, [&] { return dt_layout(dm_dims_of(*params), N, n_scenes); });
}

extern "C" int et_dmrgcn_train_forward_scenes(const et_dmrgcn_params *params, const float *C_obs, const float *nrm, int64_t N,
                                              const int32_t *scene_offsets, int n_scenes, const uint8_t *keep,
                                              const int64_t *keep_offsets, float *C_pred_refine, void *workspace,
                                              size_t workspace_bytes, et_stream_t stream) {
    const int rc = dt_check_params(params);
    if (rc != ET_OK) return rc;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, kDtMaxN);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (keep && scene_offsets && !keep_offsets) return ET_ERR_INVALID_ARG;  // where each scene's block of the mask starts
    const int ns = scene_offsets ? n_scenes : 1;
    const TrainLayout L = dt_layout(dm_dims_of(*params), N, ns);
    if (!train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return dt_forward(TrainScenesSrc{{C_obs, nrm, N, C_pred_refine}, nullptr}, params, scene_offsets, ns, N, keep,
                      scene_offsets ? keep_offsets : nullptr, workspace, L, stream);
}

extern "C" int et_dmrgcn_train_forward_graph(const et_dmrgcn_params *params, const float *v, const float *a, int64_t N,
                                             const uint8_t *keep, float *out, void *workspace, size_t workspace_bytes,
                                             et_stream_t stream) {
    const int rc = dt_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > kDtMaxN) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v || !a || !out) return ET_ERR_INVALID_ARG;
    const TrainLayout L = dt_layout(dm_dims_of(*params), N, 1);
    if (!train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return dt_forward(TrainGraphSrc{{v, a, out}, nullptr}, params, nullptr, 1, N, keep, nullptr, workspace, L, stream);
}

extern "C" int et_dmrgcn_backward_scenes(const et_dmrgcn_params *params, int64_t N, const int32_t *scene_offsets,
                                         int n_scenes, const float *d_out, float *grads, int64_t grads_floats,
                                         void *workspace, size_t workspace_bytes, et_stream_t stream) {
    int rc = dt_check_params(params);
    if (rc != ET_OK) return rc;
    const DmDims D = dm_dims_of(*params);
    rc = backward_args_status(N, scene_offsets, n_scenes, kDtMaxN, d_out, grads, grads_floats, dt_grad_off(D).total);
    if (rc != ET_OK) return rc;
    const int ns = scene_offsets ? n_scenes : 1;
    const TrainLayout L = dt_layout(D, N, ns);
    if (N > 0 && !train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return dt_backward(TrainScenesSrc{{nullptr, nullptr, N, nullptr}, d_out}, params, scene_offsets, ns, N, grads, workspace, L,
                       stream);
}

extern "C" int et_dmrgcn_backward_graph(const et_dmrgcn_params *params, int64_t N, const float *d_out, float *grads,
                                        int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    int rc = dt_check_params(params);
    if (rc != ET_OK) return rc;
    const DmDims D = dm_dims_of(*params);
    rc = backward_args_status(N, nullptr, 0, kDtMaxN, d_out, grads, grads_floats, dt_grad_off(D).total);
    if (rc != ET_OK) return rc;
    const TrainLayout L = dt_layout(D, N, 1);
    if (N > 0 && !train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return dt_backward(TrainGraphSrc{{nullptr, nullptr, nullptr}, d_out}, params, nullptr, 1, N, grads, workspace, L, stream);
}

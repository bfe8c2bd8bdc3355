// et_stgcnn_train.hip -- Social-STGCNN in training mode (include/eigentraj.h "Social-STGCNN predictor, training"): the
// forward with BatchNorm batch statistics, the running-statistics update, and the backward pass to every parameter, for
// the inference family of et_stgcnn_core.inl's check_params with n_stgcnn = 1 (no gradient flows through the Laplacian).
// The eval kernels (et_stgcnn.hip) are untouched: this translation unit takes dims_of / conv33 / prelu / check_params from
// et_stgcnn_core.inl and holds its own scene bodies beside run_scene's.
//
// One workgroup of 256 lanes per scene, forward and backward; everything a scene computes stays in the caller's workspace
// (no LDS arena: the backward and the tests read every intermediate).  Workspace, in floats:
//   [0, N per)                           per-pedestrian fields: scene s's block starts at off[s] per, field f of it at
//                                        + o[f] n (n = the scene's pedestrians), o[] = et_stgcnn_train_layout's
//   [o[STATS], + n_scenes 15 S)          per scene, BatchNorm b = 0 tcn.0, 1 tcn.3, 2 residual.1: 5 rows of S floats each,
//                                        mean, biased variance, 1/sqrt(var + eps), mean(dy), mean(dy x^) (the last two
//                                        after the backward)
//   [o[PARTIALS], + n_scenes G)          per scene, its parameter gradients in state_dict order (G = et_stgcnn_grad_floats)
// Fields per pedestrian: u (K), d (K; scene form), P (K, K+1: the contraction rows of run_scene, ones row last), g (S,K)
// the gcn output, a1 (S,K) tcn.0's output = tcn.1's input, y (S,K) tcn.1's output, t (S,K) tcn.2's output, r (S,K)
// residual.0's output, s (S,K) the pre-residual sum BN(t) + residual = the block PReLU's input, x (S,K), tp: for every
// applied tpcnn j < max(1, n_txpcnn - 1) its pre-activation and its output (k,S) each, dfin (k,S) d_out in the output
// conv's own (o, h, w) order; then the gradient at each: dtp, dx, ds, dt, dr, dy, da1, dg.
//
// Launches: forward 2 (the scene kernel; the running-statistics kernel), backward 2 (the scene kernel; the reduction over
// the scenes) -- for any N and any number of scenes, graph form and scenes form alike.
//
// Fixed orders (no atomics; two runs agree bit for bit):
//   wave_sum   every per-channel mean, variance and every parameter-gradient element of a scene is ONE wavefront's sum over
//              the element's positions p = 0 .. count-1 (row-major over the value's own (row, pedestrian) plane): lane l
//              adds p = l, l + 64, l + 128, ... in ascending order into its own accumulator that starts at +0, then the 64
//              lanes are added by the xor butterfly with strides 32, 16, 8, 4, 2, 1.
//   BatchNorm  mean = wave_sum(x) / cnt; var = wave_sum((x - mean)^2) / cnt (two passes, biased), cnt = K n.
//   scenes     grads[e] = partial[s0][e] + partial[s1][e] + ... over the non-empty scenes in ascending order, one lane per
//              element; running statistics: one lane per channel applies the recurrence scene after scene, ascending.
// st_gcns.0.tcn.2.bias and st_gcns.0.residual.0.bias feed a training-mode BatchNorm directly: their gradient is analytically
// zero and is written as an exact +0.0; so is every element of the unused tail tpcnns[n_txpcnn-1] / prelus[n_txpcnn-1]
// (n_txpcnn >= 2; model.py:140).  Every PReLU branches on the kept fp32 word in both passes.
// A single scene occupies one CU, and its four wavefronts walk some twenty dependent phases whose operands are all in
// global memory: the body is bound by memory latency (measured: about 2 ms of kernel time per scene of 34 pedestrians at the
// ET shape, DESIGN section 4 "STGCNN training"), not by the launches.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"
#include "et_stgcnn_core.inl"

enum {
    F_U, F_D, F_P, F_G, F_A1, F_Y, F_T, F_R, F_S, F_X, F_TP, F_DFIN, F_DTP, F_DX, F_DS, F_DT, F_DR, F_DY, F_DA1, F_DG,
    F_PER, F_STATS, F_STAT_STRIDE, F_PARTIALS, F_GRADS, F_TOTAL, F_COUNT
};
static_assert(F_COUNT == ET_STGCNN_TRAIN_LAYOUT_FIELDS, "et_stgcnn_train_layout's field count");

#include "et_train_sums.inl"

// where every parameter's gradient starts in the flat buffer (state_dict order)
struct GradOff {
    int gcn_w, gcn_b, bn1_w, bn1_b, prelu1, tcn_w, tcn_b, bn2_w, bn2_b, res_w, res_b, rbn_w, rbn_b, prelu;
    int tp_w[ET_STGCNN_MAX_LAYERS], tp_b[ET_STGCNN_MAX_LAYERS], out_w, out_b, prelus[ET_STGCNN_MAX_LAYERS];
    int total;
};

__host__ __device__ inline int applied_tpcnns(const Dims &D) { return D.n_tp - 1 > 1 ? D.n_tp - 1 : 1; }

__host__ __device__ inline GradOff grad_off(const Dims &D) {
    GradOff g{};
    const int S = D.S, K = D.K, k = D.k;
    int at = 0;
    auto take = [&](int cnt) {
        const int o = at;
        at += cnt;
        return o;
    };
    g.gcn_w = take(S * K), g.gcn_b = take(S * K);
    g.bn1_w = take(S), g.bn1_b = take(S), g.prelu1 = take(1);
    g.tcn_w = take(S * S * 3), g.tcn_b = take(S);
    g.bn2_w = take(S), g.bn2_b = take(S);
    if (S != 1) g.res_w = take(S), g.res_b = take(S), g.rbn_w = take(S), g.rbn_b = take(S);
    g.prelu = take(1);
    for (int j = 0; j < D.n_tp; ++j) g.tp_w[j] = take(k * (j ? k : K) * 9), g.tp_b[j] = take(k);
    g.out_w = take(k * k * 9), g.out_b = take(k);
    for (int j = 0; j < D.n_tp; ++j) g.prelus[j] = take(1);
    g.total = at;
    return g;
}

__host__ __device__ inline TrainLayout train_layout(const Dims &D, int64_t N, int64_t n_scenes) {
    TrainLayout L{};
    const int64_t SK = (int64_t)D.S * D.K, kS = (int64_t)D.k * D.S, tp = 2 * applied_tpcnns(D) * kS;
    int64_t at = 0;
    auto take = [&](int f, int64_t cnt) {
        L.o[f] = at;
        at += cnt;
    };
    take(F_U, D.K), take(F_D, D.K), take(F_P, (int64_t)D.K * (D.K + 1));
    take(F_G, SK), take(F_A1, SK), take(F_Y, SK), take(F_T, SK), take(F_R, SK), take(F_S, SK), take(F_X, SK);
    take(F_TP, tp), take(F_DFIN, kS), take(F_DTP, tp);
    take(F_DX, SK), take(F_DS, SK), take(F_DT, SK), take(F_DR, SK), take(F_DY, SK), take(F_DA1, SK), take(F_DG, SK);
    L.o[F_STATS] = N * at;
    L.o[F_STAT_STRIDE] = 15 * D.S;
    layout_tail(L, at, L.o[F_STATS] + n_scenes * L.o[F_STAT_STRIDE], grad_off(D).total, n_scenes);
    return L;
}

// one scene as the bridge hands it over: v (1,1,K,N), L (K,N,N) given; out / d_out (1,S,k,N) = the output conv's (o,h,w)
struct TrainGraphSrc {
    static constexpr bool kComputed = false;
    const float *v, *a;
    float *out;
    const float *d_out;
    __device__ void load(float *u, int64_t, int n, int K, float *red) const { scene_v(u, v, nullptr, nullptr, 0, 0, n, K, red); }
    __device__ float lap(int kk, int vv, int w, int n, const float *, const float *, float, float) const {
        return a[((int64_t)kk * n + vv) * n + w];
    }
    __device__ int64_t at(int o, int h, int w, int, int S, int n, int64_t) const { return ((int64_t)o * S + h) * n + w; }
};

// a split: C_obs (k,N), nrm (4,N), scenes by offsets; L formed from u and d (et_stgcnn.hip: ScenesSrc); out / d_out (k,N,S)
struct TrainScenesSrc {
    static constexpr bool kComputed = true;
    const float *C_obs, *nrm;
    int64_t N;
    float *out;
    const float *d_out;
    __device__ void load(float *u, int64_t b, int n, int K, float *red) const { scene_v(u, nullptr, C_obs, nrm, N, b, n, K, red); }
    __device__ float lap(int kk, int vv, int w, int n, const float *u, const float *d, float uw, float dw) const {
        const float dist = fabsf(u[kk * n + vv] - uw);
        const float ainv = dist == 0.f ? 0.f : 1.0f / dist;
        const float eye = vv == w ? 1.f : 0.f;
        return eye - (d[kk * n + vv] * (ainv + eye)) * dw;
    }
    __device__ int64_t at(int o, int h, int w, int k, int S, int, int64_t b) const {
        const int r = o * S + h;
        const int s = r / k, t = r - s * k;
        return ((int64_t)t * N + b + w) * S + s;
    }
};

struct SceneWs {
    float *f[F_PER];  // the scene's fields
    float *stat;      // its 15 S statistics
    float *part;      // its gradient partial
};

__device__ __forceinline__ SceneWs scene_ws(float *ws, const TrainLayout &L, int64_t b, int n, int scene) {
    SceneWs w;
    scene_fields(w.f, ws, L, b, n);
    w.stat = ws + L.o[F_STATS] + scene * L.o[F_STAT_STRIDE];
    w.part = ws + L.o[F_PARTIALS] + scene * L.o[F_GRADS];
    return w;
}

// batch statistics of x (S, cnt) -> stat rows 0-2 of BatchNorm `bn` (header comment: "BatchNorm")
__device__ __forceinline__ void bn_stats(const float *x, int S, int cnt, float eps, float *stat, int bn) {
    const int lane = threadIdx.x & (kWave - 1);
    float *st = stat + bn * 5 * S;
    for (int c = threadIdx.x / kWave; c < S; c += kTrWaves) {
        const float *xc = x + (int64_t)c * cnt;
        const float mean = wave_sum(cnt, [&](int p) { return xc[p]; }) / (float)cnt;
        const float var = wave_sum(cnt, [&](int p) { return (xc[p] - mean) * (xc[p] - mean); }) / (float)cnt;
        if (lane == 0) {
            st[c] = mean;
            st[S + c] = var;
            st[2 * S + c] = 1.0f / sqrtf(var + eps);
        }
    }
}

__device__ __forceinline__ float bn_apply(float x, const float *st, int S, int c, const float *w, const float *b) {
    return fmaf((x - st[c]) * st[2 * S + c], w[c], b[c]);
}

// BatchNorm-training backward, the sums: d beta = sum dy, d gamma = sum dy x^, and stat rows 3-4 = their means
__device__ __forceinline__ void bn_bwd_sums(const float *dy, const float *x, int S, int cnt, float *stat, int bn, float *d_w,
                                            float *d_b) {
    const int lane = threadIdx.x & (kWave - 1);
    float *st = stat + bn * 5 * S;
    for (int c = threadIdx.x / kWave; c < S; c += kTrWaves) {
        const float *dc = dy + (int64_t)c * cnt, *xc = x + (int64_t)c * cnt;
        const float mean = st[c], inv = st[2 * S + c];
        const float sb = wave_sum(cnt, [&](int p) { return dc[p]; });
        const float sg = wave_sum(cnt, [&](int p) { return dc[p] * ((xc[p] - mean) * inv); });
        if (lane == 0) {
            d_b[c] = sb;
            d_w[c] = sg;
            st[3 * S + c] = sb / (float)cnt;
            st[4 * S + c] = sg / (float)cnt;
        }
    }
}

// ... and dx = gamma invstd (dy - mean(dy) - x^ mean(dy x^))
__device__ __forceinline__ float bn_bwd_dx(float dy, float x, const float *st, int S, int c, const float *w) {
    const float xh = (x - st[c]) * st[2 * S + c];
    return (w[c] * st[2 * S + c]) * ((dy - st[3 * S + c]) - xh * st[4 * S + c]);
}

// d W (Cout,Cin,3,3) and d bias (Cout) of out = conv33(in): one wave_sum over the (S, n) plane per element, the nine taps
// of an (o, i) pair in one pass
__device__ __forceinline__ void conv33_dw(const float *dY, const float *in, int Cout, int Cin, int S, int n, float *d_w,
                                          float *d_b) {
    for (int oi = threadIdx.x / kWave; oi < Cout * Cin; oi += kTrWaves) {
        const int i = oi % Cin, o = oi / Cin;
        const float *dyo = dY + (int64_t)o * S * n, *ini = in + (int64_t)i * S * n;
        wave_sum_taps<9>(d_w + (int64_t)oi * 9, S * n, [&](int p, int tap) {
            const int h = p / n, w = p - h * n;
            const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
            if (hh < 0 || hh >= S || ww < 0 || ww >= n) return 0.f;
            return dyo[p] * ini[hh * n + ww];
        });
    }
    wave_sums(d_b, Cout, S * n, [&](int o, int p) { return dY[(int64_t)o * S * n + p]; });
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void stgcnn_train_fwd_kernel(Src src, et_stgcnn_params p,
                                                                      const int32_t *__restrict__ off, int64_t N, float *ws,
                                                                      TrainLayout L) {
    __shared__ float red[2 * kSgThreads / kWave];
    const SceneRows R = scene_rows(off, N);
    if (R.empty()) return;
    const Dims D = dims_of(p);
    const int K = D.K, k = D.k, S = D.S, tid = threadIdx.x;
    const int64_t b = R.b, rows = R.n();
    if (rows > ET_SCENE_MAX_N) {  // not computed: NaN (et_stgcnn_forward_scenes' rule)
        nan_scene(k, S, rows, [&](int o, int h, int w, float nan) { src.out[src.at(o, h, w, k, S, (int)rows, b)] = nan; });
        return;
    }
    const int n = (int)rows;
    const SceneWs W = scene_ws(ws, L, b, n, blockIdx.x);
    const et_stgcnn_layer &Ly = p.st_gcns[0];
    float *u = W.f[F_U], *d = W.f[F_D], *q = W.f[F_P], *g = W.f[F_G], *a1 = W.f[F_A1], *y = W.f[F_Y], *t1 = W.f[F_T];
    float *r = W.f[F_R], *s = W.f[F_S], *x = W.f[F_X];
    const int cnt = K * n, SKn = S * K * n;

    src.load(u, b, n, K, red);
    __syncthreads();
    if (Src::kComputed) {  // run_scene's statement
        for (int i = tid; i < K * n; i += kSgThreads) {
            const int kk = i / n, vv = i - kk * n;
            const float *ur = u + kk * n;
            const float uv = ur[vv];
            float sum = 0.f;
            for (int w = 0; w < n; ++w) {
                const float dist = fabsf(uv - ur[w]);
                const float ainv = dist == 0.f ? 0.f : 1.0f / dist;
                sum += ainv + (w == vv ? 1.f : 0.f);
            }
            d[i] = 1.0f / sqrtf(sum);
        }
        __syncthreads();
    }
    // P[kk,j,w] = sum_v X_j[v] L[kk,v,w], X_j = u[j,:] (j < K) and the ones row (j = K): run_scene's statements, all rows kept
    const int J = K + 1;
    const int ngroups = (J + kSgGroup - 1) / kSgGroup;
    for (int it = tid; it < K * ngroups * n; it += kSgThreads) {
        const int w = it % n;
        const int rest = it / n;
        const int gq = rest % ngroups, kk = rest / ngroups;
        const int j0 = gq * kSgGroup;
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
                if (j < J) acc[jj] = fmaf(j < J - 1 ? u[j * n + vv] : 1.f, lv, acc[jj]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < kSgGroup; ++jj)
            if (j0 + jj < J) q[((int64_t)kk * J + j0 + jj) * n + w] = acc[jj];
    }
    __syncthreads();
    for (int it = tid; it < SKn; it += kSgThreads) {
        const int w = it % n;
        const int ct = it / n;
        const int c = ct / K, t = ct - c * K;
        float acc = 0.f;
        for (int kk = 0; kk < K; ++kk) {
            const int o = kk * S + c;  // gcn channel o = kk S + c (model.py:44's view)
            const float *qk = q + (int64_t)kk * J * n;
            acc = fmaf(Ly.gcn_w[o], qk[t * n + w], acc);
            acc = fmaf(Ly.gcn_b[o], qk[(J - 1) * n + w], acc);
        }
        g[it] = acc;
    }
    __syncthreads();
    bn_stats(g, S, cnt, p.bn_eps, W.stat, 0);
    __syncthreads();
    for (int it = tid; it < SKn; it += kSgThreads) {
        const int c = it / cnt;
        const float v1 = bn_apply(g[it], W.stat, S, c, Ly.bn1_w, Ly.bn1_b);
        a1[it] = v1;
        y[it] = prelu(v1, Ly.prelu1);
    }
    __syncthreads();
    for (int it = tid; it < SKn; it += kSgThreads) {  // run_scene's (3,1) conv and residual conv, before their BatchNorms
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
        t1[it] = acc;
        if (Ly.res_w) r[it] = fmaf(Ly.res_w[c], u[t * n + w], Ly.res_b[c]);
    }
    __syncthreads();
    bn_stats(t1, S, cnt, p.bn_eps, W.stat, 1);
    if (Ly.res_w) bn_stats(r, S, cnt, p.bn_eps, W.stat, 2);
    __syncthreads();
    for (int it = tid; it < SKn; it += kSgThreads) {
        const int c = it / cnt;
        const float tb = bn_apply(t1[it], W.stat + 5 * S, S, c, Ly.bn2_w, Ly.bn2_b);
        // (S = 1: the identity residual; then x[it] = x[t, w] and u has the same index)
        const float res = Ly.res_w ? bn_apply(r[it], W.stat + 10 * S, S, c, Ly.res_bn_w, Ly.res_bn_b) : u[it];
        const float sv = tb + res;
        s[it] = sv;
        x[it] = prelu(sv, Ly.prelu);
    }
    __syncthreads();

    // tpcnns over x viewed (K, S, n), every pre-activation and output kept
    const int ko = k * S * n, A = applied_tpcnns(D);
    float *tp = W.f[F_TP];
    for (int j = 0; j < A; ++j) {
        const float *cur = j ? tp + (int64_t)(2 * j - 1) * ko : x;
        float *pre = tp + (int64_t)(2 * j) * ko, *outj = pre + ko;
        for (int it = tid; it < ko; it += kSgThreads) {
            const int w = it % n, oh = it / n;
            const int o = oh / S, h = oh - o * S;
            const float pv = conv33(cur, j ? k : K, S, n, p.tpcnn_w[j], p.tpcnn_b[j], o, h, w);
            pre[it] = pv;
            outj[it] = j ? prelu(pv, p.prelus[j]) + cur[it] : prelu(pv, p.prelus[0]);
        }
        __syncthreads();
    }
    const float *cur = tp + (int64_t)(2 * A - 1) * ko;
    for (int it = tid; it < ko; it += kSgThreads) {
        const int w = it % n, oh = it / n;
        const int o = oh / S, h = oh - o * S;
        src.out[src.at(o, h, w, k, S, n, b)] = conv33(cur, k, S, n, p.out_w, p.out_b, o, h, w);
    }
}

// running statistics, as torch updates them: one lane per (BatchNorm, channel), the scenes in ascending order;
// an empty scene (and one that is not computed) is no batch
__global__ __launch_bounds__(kSgThreads) void stgcnn_train_stats_kernel(et_stgcnn_train tr, const int32_t *__restrict__ off,
                                                                        int n_scenes, int64_t N, int S, int K, const float *ws,
                                                                        TrainLayout L) {
    const int i = blockIdx.x * kSgThreads + threadIdx.x;
    if (i >= 3 * S) return;
    const int bn = i / S, c = i - bn * S;
    float *rm = bn == 0 ? tr.bn1_mean : bn == 1 ? tr.bn2_mean : tr.res_bn_mean;
    float *rv = bn == 0 ? tr.bn1_var : bn == 1 ? tr.bn2_var : tr.res_bn_var;
    int64_t *nb = bn == 0 ? tr.bn1_batches : bn == 1 ? tr.bn2_batches : tr.res_bn_batches;
    if (!rm) return;  // S = 1: no residual.1
    const float m = tr.momentum;
    float mean = rm[c], var = rv[c];
    int64_t batches = 0;
    for (int s = 0; s < n_scenes; ++s) {
        const int64_t n = off ? (int64_t)off[s + 1] - off[s] : N;
        if (n < 1 || n > ET_SCENE_MAX_N) continue;
        const float *st = ws + L.o[F_STATS] + s * L.o[F_STAT_STRIDE] + bn * 5 * S;
        const float cnt = (float)(K * n);
        mean = (1.f - m) * mean + m * st[c];
        var = (1.f - m) * var + m * (st[S + c] * cnt / (cnt - 1.f));
        ++batches;
    }
    rm[c] = mean;
    rv[c] = var;
    if (c == 0) nb[0] += batches;
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void stgcnn_train_bwd_kernel(Src src, et_stgcnn_params p,
                                                                      const int32_t *__restrict__ off, int64_t N, float *ws,
                                                                      TrainLayout L) {
    const SceneRows R = scene_rows(off, N);
    if (R.empty() || R.n() > ET_SCENE_MAX_N) return;
    const Dims D = dims_of(p);
    const GradOff G = grad_off(D);
    const int K = D.K, k = D.k, S = D.S, tid = threadIdx.x;
    const int64_t b = R.b;
    const int n = (int)R.n();
    const SceneWs W = scene_ws(ws, L, b, n, blockIdx.x);
    const et_stgcnn_layer &Ly = p.st_gcns[0];
    const int cnt = K * n, SKn = S * K * n, ko = k * S * n, A = applied_tpcnns(D);
    float *gr = W.part;
    const float *u = W.f[F_U], *q = W.f[F_P], *g = W.f[F_G], *a1 = W.f[F_A1], *y = W.f[F_Y], *t1 = W.f[F_T], *r = W.f[F_R];
    const float *s = W.f[F_S], *x = W.f[F_X], *tp = W.f[F_TP];
    float *dfin = W.f[F_DFIN], *dtp = W.f[F_DTP], *dx = W.f[F_DX], *ds = W.f[F_DS], *dt = W.f[F_DT], *dr = W.f[F_DR];
    float *dy = W.f[F_DY], *da1 = W.f[F_DA1], *dg = W.f[F_DG];

    // exact zeros: the two biases in front of a BatchNorm, and the tail the forward never reads
    for (int i = tid; i < S; i += kSgThreads) {
        gr[G.tcn_b + i] = 0.f;
        if (S != 1) gr[G.res_b + i] = 0.f;
    }
    for (int j = A; j < D.n_tp; ++j) {
        for (int i = tid; i < k * k * 9; i += kSgThreads) gr[G.tp_w[j] + i] = 0.f;
        for (int i = tid; i < k; i += kSgThreads) gr[G.tp_b[j] + i] = 0.f;
        if (tid == 0) gr[G.prelus[j]] = 0.f;
    }
    for (int it = tid; it < ko; it += kSgThreads) {
        const int w = it % n, oh = it / n;
        const int o = oh / S, h = oh - o * S;
        dfin[it] = src.d_out[src.at(o, h, w, k, S, n, b)];
    }
    __syncthreads();

    // the output conv
    {
        const float *cur = tp + (int64_t)(2 * A - 1) * ko;
        float *dcur = dtp + (int64_t)(2 * A - 1) * ko;
        conv33_dw(dfin, cur, k, k, S, n, gr + G.out_w, gr + G.out_b);
        for (int it = tid; it < ko; it += kSgThreads) {
            const int w = it % n, ih = it / n;
            const int i = ih / S, h = ih - i * S;
            dcur[it] = conv33_dx(dfin, k, k, S, n, p.out_w, i, h, w);
        }
        __syncthreads();
    }
    // the tpcnn residual loop, then tpcnns[0]: out_j = prelu(pre_j) (+ out_{j-1})
    for (int j = A - 1; j >= 0; --j) {
        const float *pre = tp + (int64_t)(2 * j) * ko;
        const float *dout = dtp + (int64_t)(2 * j + 1) * ko;
        float *dpre = dtp + (int64_t)(2 * j) * ko;
        for (int it = tid; it < ko; it += kSgThreads) dpre[it] = dout[it] * slope(pre[it], p.prelus[j]);
        __syncthreads();
        const float *in = j ? tp + (int64_t)(2 * j - 1) * ko : x;
        const int Cin = j ? k : K;
        wave_sums(gr + G.prelus[j], 1, ko, [&](int, int pp) { return dout[pp] * neg_part(pre[pp]); });
        conv33_dw(dpre, in, k, Cin, S, n, gr + G.tp_w[j], gr + G.tp_b[j]);
        float *din = j ? dtp + (int64_t)(2 * j - 1) * ko : dx;
        for (int it = tid; it < Cin * S * n; it += kSgThreads) {
            const int w = it % n, ih = it / n;
            const int i = ih / S, h = ih - i * S;
            const float v = conv33_dx(dpre, k, Cin, S, n, p.tpcnn_w[j], i, h, w);
            din[it] = j ? dout[it] + v : v;
        }
        __syncthreads();
    }
    // dx is d x in x's own (S, K, n) order as well: the (K,S,n) view is a reshape.  The block's PReLU:
    for (int it = tid; it < SKn; it += kSgThreads) ds[it] = dx[it] * slope(s[it], Ly.prelu);
    __syncthreads();
    wave_sums(gr + G.prelu, 1, SKn, [&](int, int pp) { return dx[pp] * neg_part(s[pp]); });
    // tcn.3 and residual.1 see the same dy = ds
    bn_bwd_sums(ds, t1, S, cnt, W.stat, 1, gr + G.bn2_w, gr + G.bn2_b);
    if (Ly.res_w) bn_bwd_sums(ds, r, S, cnt, W.stat, 2, gr + G.rbn_w, gr + G.rbn_b);
    __syncthreads();
    for (int it = tid; it < SKn; it += kSgThreads) {
        const int c = it / cnt;
        dt[it] = bn_bwd_dx(ds[it], t1[it], W.stat + 5 * S, S, c, Ly.bn2_w);
        if (Ly.res_w) dr[it] = bn_bwd_dx(ds[it], r[it], W.stat + 10 * S, S, c, Ly.res_bn_w);
    }
    __syncthreads();
    if (Ly.res_w)  // r[c,t,w] = res_w[c] u[t,w] + res_b[c]
        wave_sums(gr + G.res_w, S, cnt, [&](int c, int pp) { return dr[(int64_t)c * cnt + pp] * u[pp]; });
    // the (3,1) conv: t[c,t,w] = b[c] + sum_ci sum_tap W[c,ci,tap] y[ci,t+tap-1,w]
    for (int cc = tid / kWave; cc < S * S; cc += kTrWaves) {
        const int ci = cc % S, c = cc / S;
        const float *dc = dt + (int64_t)c * cnt, *yc = y + (int64_t)ci * cnt;
        wave_sum_taps<3>(gr + G.tcn_w + cc * 3, cnt, [&](int pp, int tap) {
            const int tt = pp / n + tap - 1;
            if (tt < 0 || tt >= K) return 0.f;
            return dc[pp] * yc[pp + (tap - 1) * n];
        });
    }
    for (int it = tid; it < SKn; it += kSgThreads) {
        const int w = it % n;
        const int ct = it / n;
        const int ci = ct / K, t = ct - ci * K;
        float acc = 0.f;
        for (int c = 0; c < S; ++c) {
            const float *wc = Ly.tcn_w + ((int64_t)c * S + ci) * 3;
            const float *dc = dt + (int64_t)c * cnt;
            if (t + 1 < K) acc = fmaf(wc[0], dc[(t + 1) * n + w], acc);
            acc = fmaf(wc[1], dc[t * n + w], acc);
            if (t > 0) acc = fmaf(wc[2], dc[(t - 1) * n + w], acc);
        }
        dy[it] = acc;
        da1[it] = acc * slope(a1[it], Ly.prelu1);
    }
    __syncthreads();
    wave_sums(gr + G.prelu1, 1, SKn, [&](int, int pp) { return dy[pp] * neg_part(a1[pp]); });
    bn_bwd_sums(da1, g, S, cnt, W.stat, 0, gr + G.bn1_w, gr + G.bn1_b);
    __syncthreads();
    for (int it = tid; it < SKn; it += kSgThreads) dg[it] = bn_bwd_dx(da1[it], g[it], W.stat, S, it / cnt, Ly.bn1_w);
    __syncthreads();
    // the gcn conv through the kept contraction rows: g[c,t,w] = sum_kk W[kk S + c] P[kk,t,w] + b[kk S + c] P[kk,K,w]
    const int J = K + 1;
    wave_sums(gr + G.gcn_w, S * K, cnt, [&](int o, int pp) {
        const int kk = o / S, c = o - kk * S;
        return dg[(int64_t)c * cnt + pp] * q[(int64_t)kk * J * n + pp];
    });
    wave_sums(gr + G.gcn_b, S * K, cnt, [&](int o, int pp) {
        const int kk = o / S, c = o - kk * S;
        return dg[(int64_t)c * cnt + pp] * q[((int64_t)kk * J + K) * n + pp % n];
    });
}

static int check_train_params(const et_stgcnn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->n_stgcnn != 1) return ET_ERR_UNSUPPORTED;  // deeper stacks send a gradient through the contraction
    return check_params(p);
}

static int check_train_state(const et_stgcnn_params *p, const et_stgcnn_train *t) {
    if (!t || !(t->momentum >= 0.f && t->momentum <= 1.f)) return ET_ERR_INVALID_ARG;
    if (!t->bn1_mean || !t->bn1_var || !t->bn1_batches || !t->bn2_mean || !t->bn2_var || !t->bn2_batches)
        return ET_ERR_INVALID_ARG;
    const bool res = p->output_feat != 1;
    if (res != (t->res_bn_mean != nullptr) || res != (t->res_bn_var != nullptr) || res != (t->res_bn_batches != nullptr))
        return ET_ERR_INVALID_ARG;
    return ET_OK;
}

template <class Src>
static int train_forward(const Src &src, const et_stgcnn_params *p, const et_stgcnn_train *t, const int32_t *off, int ns,
                         int64_t N, void *workspace, const TrainLayout &L, et_stream_t stream) {
    const Dims D = dims_of(*p);
    hipLaunchKernelGGL((stgcnn_train_fwd_kernel<Src>), dim3((unsigned)ns), dim3(kSgThreads), 0, (hipStream_t)stream, src, *p,
                       off, N, (float *)workspace, L);
    ET_LAUNCH_CHECK();
    hipLaunchKernelGGL(stgcnn_train_stats_kernel, dim3((unsigned)ceil_div(3 * D.S, kSgThreads)), dim3(kSgThreads), 0,
                       (hipStream_t)stream, *t, off, ns, N, D.S, D.K, (const float *)workspace, L);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

template <class Src>
static int train_backward(const Src &src, const et_stgcnn_params *p, const int32_t *off, int ns, int64_t N, float *grads,
                          void *workspace, const TrainLayout &L, et_stream_t stream) {
    if (N > 0) {
        hipLaunchKernelGGL((stgcnn_train_bwd_kernel<Src>), dim3((unsigned)ns), dim3(kSgThreads), 0, (hipStream_t)stream, src,
                           *p, off, N, (float *)workspace, L);
        ET_LAUNCH_CHECK();
    }
    return scene_grad_reduce((const float *)workspace + L.o[F_PARTIALS], L.o[F_GRADS], ET_SCENE_MAX_N, off, ns, N, grads,
                             stream);
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_stgcnn_train_workspace_bytes(const et_stgcnn_params *params, int64_t N, int n_scenes) {
    if (check_train_params(params) != ET_OK || N <= 0 || n_scenes < 1) return 0;
    return (size_t)train_layout(dims_of(*params), N, n_scenes).o[F_TOTAL] * 4;
}

extern "C" int64_t et_stgcnn_grad_floats(const et_stgcnn_params *params) {
    if (check_train_params(params) != ET_OK) return 0;
    return grad_off(dims_of(*params)).total;
}

extern "C" int et_stgcnn_train_layout(const et_stgcnn_params *params, int64_t N, int n_scenes, int64_t *offsets,
                                      int n_offsets) {
    const int rc = check_train_params(params);
    if (rc != ET_OK) return rc;
    return layout_out(N, n_scenes, offsets, n_offsets, [&] { return train_layout(dims_of(*params), N, n_scenes); });
}

extern "C" int et_stgcnn_train_forward_scenes(const et_stgcnn_params *params, const et_stgcnn_train *train,
                                              const float *C_obs, const float *nrm, int64_t N, const int32_t *scene_offsets,
                                              int n_scenes, float *C_pred_refine, void *workspace, size_t workspace_bytes,
                                              et_stream_t stream) {
    int rc = check_train_params(params);
    if (rc != ET_OK) return rc;
    if ((rc = check_train_state(params, train)) != ET_OK) return rc;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, ET_SCENE_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    const int ns = scene_offsets ? n_scenes : 1;
    const TrainLayout L = train_layout(dims_of(*params), N, ns);
    if (!train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return train_forward(TrainScenesSrc{C_obs, nrm, N, C_pred_refine, nullptr}, params, train, scene_offsets, ns, N, workspace,
                         L, stream);
}

extern "C" int et_stgcnn_train_forward_graph(const et_stgcnn_params *params, const et_stgcnn_train *train, const float *v,
                                             const float *a, int64_t N, float *out, void *workspace, size_t workspace_bytes,
                                             et_stream_t stream) {
    int rc = check_train_params(params);
    if (rc != ET_OK) return rc;
    if ((rc = check_train_state(params, train)) != ET_OK) return rc;
    if (N < 0 || N > ET_SCENE_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v || !a || !out) return ET_ERR_INVALID_ARG;
    const TrainLayout L = train_layout(dims_of(*params), N, 1);
    if (!train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return train_forward(TrainGraphSrc{v, a, out, nullptr}, params, train, nullptr, 1, N, workspace, L, stream);
}

extern "C" int et_stgcnn_backward_scenes(const et_stgcnn_params *params, int64_t N, const int32_t *scene_offsets,
                                         int n_scenes, const float *d_out, float *grads, int64_t grads_floats,
                                         void *workspace, size_t workspace_bytes, et_stream_t stream) {
    int rc = check_train_params(params);
    if (rc != ET_OK) return rc;
    const Dims D = dims_of(*params);
    rc = backward_args_status(N, scene_offsets, n_scenes, ET_SCENE_MAX_N, d_out, grads, grads_floats, grad_off(D).total);
    if (rc != ET_OK) return rc;
    const int ns = scene_offsets ? n_scenes : 1;
    const TrainLayout L = train_layout(D, N, ns);
    if (N > 0 && !train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return train_backward(TrainScenesSrc{nullptr, nullptr, N, nullptr, d_out}, params, scene_offsets, ns, N, grads, workspace,
                          L, stream);
}

extern "C" int et_stgcnn_backward_graph(const et_stgcnn_params *params, int64_t N, const float *d_out, float *grads,
                                        int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    int rc = check_train_params(params);
    if (rc != ET_OK) return rc;
    const Dims D = dims_of(*params);
    rc = backward_args_status(N, nullptr, 0, ET_SCENE_MAX_N, d_out, grads, grads_floats, grad_off(D).total);
    if (rc != ET_OK) return rc;
    const TrainLayout L = train_layout(D, N, 1);
    if (N > 0 && !train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return train_backward(TrainGraphSrc{nullptr, nullptr, nullptr, d_out}, params, nullptr, 1, N, grads, workspace, L, stream);
}

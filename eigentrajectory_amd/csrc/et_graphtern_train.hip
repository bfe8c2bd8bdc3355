// et_graphtern_train.hip -- Graph-TERN in training mode (include/eigentraj.h "Graph-TERN predictor, training"): the forward
// with DropEdge (stmrgcn.py:22: drop_edge(A, 0.8, self.training) on the float tensor A (1,4,T,N,N) before + I and before the
// normalisation, so the degrees change with the mask and the normalised graph is no longer symmetric) and the backward pass to
// every parameter, for the inference family of gt_check_params with n_epgcn = 1 (C_in = 1 and detached graphs: no gradient
// passes through a normalised graph) and scenes of at most ET_GRAPHTERN_TRAIN_MAX_N pedestrians.  The eval kernel
// (et_graphtern.hip) is untouched; both units take GtDims / gt_relations / conv33_replicate / the sources from
// et_graphtern_core.inl.
//
// Keep mask: uint8 (4,T,n,n) indexed [r,t,w,v] per scene (scenes form: scene s at 4 T keep_offsets[s], the packed sum of
// n^2); entry != 0 keeps A_r[w,v]; NULL keeps everything.  It is applied where the eval kernel reads A_r[w,v]: in the degree
// loop (s[r,t,w] = sum_v (keep ? A_r[w,v] : 0) + [v==w], d = 1/sqrt(s), inf -> 0) and in the contraction loop
// (L[w,v] = (d_w ((keep ? A_r[w,v] : 0) + [v==w])) d_v, d_v the column pedestrian's own row degree).  A's diagonal is exactly
// 0, so the mask's diagonal has no effect.  Every other statement of the forward is gt_run_scene's in its order: with a NULL
// or an all-ones mask the output is bit-equal to et_graphtern_forward_graph / _scenes.
//
// Forward: ONE launch, one workgroup of 256 lanes per scene.  The live operands (u, rel, d, the three rotating buffers) are
// in the LDS arena when the scene fits it (gt_arena_per_ped floats per pedestrian; S = 20, k = 6: n <= 35), else in the
// scene's arena rows of the workspace; what the backward reads is written on the side into the workspace:
//   u (T), d (4,T), P (4,2,T) the contracted rows (j = 0: u's row, j = 1: the ones row), yp (16,T) the gcn sum = the tcn
//   PReLU's input, x0 (T,16) the st_mrgcn block's output after the permute, and per epcnn block j: c0, y (k,16: tpcns.0's
//   pre-activation and output), c1, o (k,C_out: cpcns.0's pre-activation, the block's output); block j's input is x0 (j = 0)
//   or block j-1's o.
// Backward: THREE launches for any N and any number of scenes:
//   1. graphtern_train_bwd_kernel    one workgroup per scene walks the dependent chain d out -> ... -> d y with its operands
//                                    in the same arena (three buffers) and leaves per epcnn block do (k,C_out) and dy (k,16),
//                                    then dx0 (T,16) and dy (16,T), in the workspace
//   2. graphtern_train_wgrad_kernel  grid (scenes, kGttChunks): every parameter-gradient element of a scene is one wavefront's
//                                    sum; the scene's 64 wavefronts take the elements round robin -> the scene's partial
//   3. scene_grad_reduce_kernel      grads[e] = the scenes' partials in ascending order, the first one copied
//                                    (et_train_sums.inl, which the three scene training units share)
// The transposed 3x3 convolution under REPLICATE padding is written in gather form (conv33_replicate_dx): an input cell sums
// the outputs whose clamped taps land on it -- exactly three (output row, row tap) pairs and three (output column, column
// tap) pairs for every cell and every plane size (at n = 1 all three column taps of output column 0, at n = 2 two taps of the
// cell's own column and one of the other) -- over o ascending, then the row pairs, then the column pairs, each by ascending
// output index, then ascending tap.  The convolution weight gradients read the input through the same clamps.
// Fixed orders (no atomics; two runs agree bit for bit, a one-scene scenes call equals the graph call): wave_sum of
// et_train_sums.inl (lane l adds positions l, l + 64, ... ascending from +0, then the xor butterfly 32 .. 1); every other
// sum is one lane's ascending fmaf chain.  Every PReLU branches on the kept fp32 word in both passes.
// tp_mrgcns.0.prelu.weight, which the forward never applies, has a slot of the gradient buffer that is always +0.
// A scene of more than ET_GRAPHTERN_TRAIN_MAX_N pedestrians is not computed: NaN outputs, no gradient.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"
#include "et_stgcnn_core.inl"
#include "et_graphtern_core.inl"

enum {
    F_U, F_D, F_P, F_YP, F_X0, F_TP, F_DTP, F_DX0, F_DY, F_ARENA, F_PER, F_TP_STRIDE, F_DTP_STRIDE, F_PARTIALS, F_GRADS, F_TOTAL,
    F_COUNT
};
static_assert(F_COUNT == ET_GRAPHTERN_TRAIN_LAYOUT_FIELDS, "et_graphtern_train_layout's field count");

#include "et_train_sums.inl"

constexpr int kGttMaxN = ET_GRAPHTERN_TRAIN_MAX_N;
constexpr int kGttChunks = 16;                     // weight-gradient workgroups per scene
constexpr int kGttWaves = kGttChunks * kTrWaves;   // ... and its wavefronts

__host__ __device__ inline int gtt_cmax(const GtDims &D) { return D.S > kGtHidden ? D.S : kGtHidden; }

// the number of gradient floats (state_dict order: header comment of include/eigentraj.h)
__host__ __device__ inline int gtt_grad_total(const GtDims &D) {
    const int H = kGtHidden, T = D.T, k = D.k, S = D.S;
    int at = 1 + 2 * kGtRel * H + 1 + H * H * 3 + H + 2 * H;
    for (int j = 0; j < D.n_cnn; ++j) {
        const bool last = j + 1 == D.n_cnn;
        const int Rin = j == 0 ? T : k, Cout = last ? S : H;
        at += k * Rin * 9 + k + 1 + Cout * H * 9 + Cout + 1;
        if (last && S != H) at += S * H + S;
        if (j == 0) at += k * T + k;
    }
    return at;
}

__host__ __device__ inline TrainLayout gtt_layout(const GtDims &D, int64_t N, int64_t n_scenes) {
    TrainLayout L{};
    const int64_t HT = (int64_t)kGtHidden * D.T, kH = (int64_t)D.k * kGtHidden, kC = (int64_t)D.k * gtt_cmax(D);
    int64_t at = 0;
    auto take = [&](int f, int64_t cnt) {
        L.o[f] = at;
        at += cnt;
    };
    L.o[F_TP_STRIDE] = 2 * kH + 2 * kC;
    L.o[F_DTP_STRIDE] = kC + kH;
    take(F_U, D.T), take(F_D, (int64_t)kGtRel * D.T), take(F_P, (int64_t)kGtRel * 2 * D.T), take(F_YP, HT), take(F_X0, HT);
    take(F_TP, D.n_cnn * L.o[F_TP_STRIDE]), take(F_DTP, D.n_cnn * L.o[F_DTP_STRIDE]);
    take(F_DX0, HT), take(F_DY, HT), take(F_ARENA, gt_arena_per_ped(D));
    layout_tail(L, at, N * at, gtt_grad_total(D), n_scenes);
    return L;
}

// a scene's fields in the workspace
struct GttScene : TrainScene {
    int64_t tp_stride, dtp_stride;  // x n: one epcnn block's kept values / gradients
};

__device__ __forceinline__ GttScene gtt_scene(float *ws, const TrainLayout &L, int64_t b, int n, int scene) {
    return {train_scene(ws, L, b, n, scene), L.o[F_TP_STRIDE] * n, L.o[F_DTP_STRIDE] * n};
}

// block j's kept values: c0, y (k,16,n), c1, o (k,C_out,n); its gradients: d_o (k,C_out,n) at the block's output, dy (k,16,n)
struct GttBlock {
    float *c0, *y, *c1, *o, *d_o, *dy;
};

__device__ __forceinline__ GttBlock gtt_block(const GttScene &W, const GtDims &D, int j) {
    GttBlock B;
    float *t = W.f[F_TP] + j * W.tp_stride, *d = W.f[F_DTP] + j * W.dtp_stride;
    const int64_t kH = (int64_t)D.k * kGtHidden * W.n, kC = (int64_t)D.k * gtt_cmax(D) * W.n;
    B.c0 = t, B.y = t + kH, B.c1 = t + 2 * kH, B.o = t + 2 * kH + kC;
    B.d_o = d, B.dy = d + kC;
    return B;
}

// where an output / d_out entry (t, o, w) of the scene at row b lies: (1,k,N,S) in the graph form (b = 0), (k,N,S) otherwise
__device__ __forceinline__ int64_t gtt_out_at(int t, int o, int w, int S, int64_t b, int64_t N) {
    return ((int64_t)t * N + b + w) * S + o;
}

// the forward of one scene: gt_run_scene's statements for n_epgcn = 1 with the keep mask, every kept value written on the side
template <class Src>
__device__ __forceinline__ void gtt_forward_scene(const Src &src, const et_graphtern_params &p, const GtDims &D, int64_t b,
                                                  int n, float *ar, float *red, float *out, int64_t N, const GttScene &W,
                                                  const uint8_t *keep) {
    const int T = D.T, k = D.k, S = D.S, H = kGtHidden;
    const int tid = threadIdx.x;
    float *u = ar, *rel = u + T * n, *d = rel + T * n;
    float *x = d + (int64_t)kGtRel * T * n, *y = x + (int64_t)D.qpp * n, *q = y + (int64_t)D.qpp * n;
    // keep[r,t,w,vv]; a NULL mask keeps everything
    auto kept = [&](int r, int t, int w, int vv) { return !keep || keep[(((int64_t)r * T + t) * n + w) * n + vv] != 0; };

    src.load(u, rel, b, n, T, red);
    __syncthreads();
    if (Src::kComputed) {
        for (int i = tid; i < T * n; i += kSgThreads) rel[i] = i < n ? 0.f : u[i] - u[i - n];
        __syncthreads();
    }
    // degrees: the row sums of A'_r + I, per relation and time row (>= 1; an overflowed sum gives D^-1/2 = 0)
    float *dk = W.f[F_D];
    for (int i = tid; i < T * n; i += kSgThreads) {
        const int t = i / n, w = i - t * n;
        const float *ut = u + t * n, *rt = rel + t * n;
        const float uw = ut[w], rw = rt[w];
        W.f[F_U][i] = u[i];
        float s[kGtRel] = {0.f, 0.f, 0.f, 0.f};
        for (int vv = 0; vv < n; ++vv) {
            float A[kGtRel];
            gt_relations(fabsf(uw - ut[vv]), fabsf(rw - rt[vv]), A);
            const float diag = vv == w ? 1.f : 0.f;
#pragma unroll
            for (int r = 0; r < kGtRel; ++r) s[r] += (kept(r, t, w, vv) ? A[r] : 0.f) + diag;
        }
#pragma unroll
        for (int r = 0; r < kGtRel; ++r) {
            const float di = 1.0f / sqrtf(s[r]);
            const float dv = isinf(di) ? 0.f : di;  // normalizer.py:12
            d[(r * T + t) * n + w] = dv;
            dk[(r * T + t) * n + w] = dv;
        }
    }
    __syncthreads();

    const et_graphtern_layer &Ly = p.tp_mrgcns[0];
    {
        constexpr int Cin = 1, J = 2;  // contracted rows per graph: u[t,:] and the ones row (the conv's bias)
        const float *xin = u;
        float *Pk = W.f[F_P], *ypk = W.f[F_YP], *xk = W.f[F_X0];
        // qpp >= 16 T >= 4 J T: all time rows in one chunk of q
        for (int it = tid; it < T * n; it += kSgThreads) {
            const int w = it % n;
            const int t = it / n;
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
                xv[0] = xin[t * n + vv];
                xv[1] = 1.f;
#pragma unroll
                for (int r = 0; r < kGtRel; ++r) {
                    const float lv = (dw[r] * ((kept(r, t, w, vv) ? A[r] : 0.f) + diag)) * d[(r * T + t) * n + vv];
#pragma unroll
                    for (int jj = 0; jj < kGtRows; ++jj) acc[r][jj] = fmaf(xv[jj], lv, acc[r][jj]);
                }
            }
#pragma unroll
            for (int r = 0; r < kGtRel; ++r)
#pragma unroll
                for (int jj = 0; jj < kGtRows; ++jj) {
                    q[((t * kGtRel + r) * J + jj) * n + w] = acc[r][jj];
                    Pk[((int64_t)(r * J + jj) * T + t) * n + w] = acc[r][jj];
                }
        }
        __syncthreads();
        // the 1x1 convolution on the contracted rows (relation r on channels r 16 + c), then the tcn's PReLU
        for (int it = tid; it < H * T * n; it += kSgThreads) {
            const int w = it % n;
            const int ct = it / n;
            const int c = ct / T, t = ct - c * T;
            float acc = 0.f;
            for (int r = 0; r < kGtRel; ++r) {
                const int o = r * H + c;  // stmrgcn.py:21's view
                const float *qb = q + (int64_t)(t * kGtRel + r) * J * n;
                for (int ci = 0; ci < Cin; ++ci) acc = fmaf(Ly.gcn_w[o * Cin + ci], qb[ci * n + w], acc);
                acc = fmaf(Ly.gcn_b[o], qb[Cin * n + w], acc);
            }
            ypk[it] = acc;
            y[it] = prelu(acc, Ly.tcn_prelu);
        }
        __syncthreads();
        // tcn: (3,1) conv over time (zero padding), + residual -> q as (T,16,n), the permute of model.py:256; use_mdn: the
        // block's own PReLU is not applied (stmrgcn.py:54)
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
            float res = Ly.res_b[c];
            for (int ci = 0; ci < Cin; ++ci) res = fmaf(Ly.res_w[c * Cin + ci], xin[(ci * T + t) * n + w], res);
            const float xv = acc + res;
            q[(t * H + c) * n + w] = xv;
            xk[(t * H + c) * n + w] = xv;
        }
        __syncthreads();
        float *tmp = x;
        x = q;
        q = tmp;
    }

    // epcnn blocks over x (rows, 16, n): rows = T into the first block, k afterwards; the last block's channels are S
    for (int j = 0; j < D.n_cnn; ++j) {
        const et_graphtern_epcnn &Ep = p.tpcnns[j];
        const GttBlock B = gtt_block(W, D, j);
        const bool last = j + 1 == D.n_cnn;
        const int Rin = j == 0 ? T : k, Cout = last ? S : H;
        for (int it = tid; it < k * H * n; it += kSgThreads) {  // tpcns[0]: the rows as channels, over the (16, n) plane
            const int w = it % n, oh = it / n;
            const int o = oh / H, h = oh - o * H;
            const float cv = conv33_replicate(x, Rin, H, H, 1, n, Ep.tpcn_w, Ep.tpcn_b, o, h, w);
            const float yv = prelu(cv, Ep.tpcn_a);
            B.c0[it] = cv;
            B.y[it] = yv;
            y[it] = yv;
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
            const float cv = conv33_replicate(y, H, 1, k, H, n, Ep.cpcn_w, Ep.cpcn_b, o, t, w);
            const float val = prelu(cv, Ep.cpcn_a) + res;
            B.c1[it] = cv;
            B.o[it] = val;
            // (t, o, w) -> transpose(2, 3) (model.py:262) -> (1,k,N,S), which the post-hook squeezes
            if (last) out[gtt_out_at(t, o, w, S, b, N)] = val;
            else q[it] = val;
        }
        __syncthreads();
        float *tmp = x;
        x = q;
        q = tmp;
    }
}

template <class Src>
__global__ __launch_bounds__(kSgThreads) void graphtern_train_fwd_kernel(Src src, et_graphtern_params p,
                                                                         const int32_t *__restrict__ off, int64_t N,
                                                                         const uint8_t *__restrict__ keep,
                                                                         const int64_t *__restrict__ keep_off, float *out,
                                                                         float *ws, TrainLayout L) {
    extern __shared__ float lds[];
    __shared__ float red[2 * kSgThreads / kWave];
    const SceneRows R = scene_rows(off, N);
    if (R.empty()) return;
    const GtDims D = gt_dims_of(p);
    const int64_t b = R.b, n = R.n();
    if (n > kGttMaxN) {  // not computed: NaN, the scene's n S floats of every output row at a stretch
        const float nan = __builtin_nanf("");
        for (int64_t t = 0; t < D.k; ++t)
            for (int64_t i = threadIdx.x; i < n * D.S; i += kSgThreads) out[(t * N + b) * D.S + i] = nan;
        return;
    }
    const GttScene W = gtt_scene(ws, L, b, (int)n, blockIdx.x);
    const uint8_t *kp = keep ? keep + (keep_off ? keep_off[blockIdx.x] : 0) * kGtRel * D.T : nullptr;
    float *ar = gt_arena_per_ped(D) * n * 4 <= kSgLdsBytes ? lds : W.f[F_ARENA];
    gtt_forward_scene(src, p, D, b, (int)n, ar, red, out, N, W, kp);
}

// d in[i,h,w] of out = conv33_replicate(in) (H rows, n columns): the outputs whose clamped taps land on the cell, over o
// ascending, then the (output row, tap) pairs, then the (output column, tap) pairs, each by ascending output index and tap.
// Output entry (o, h', w') of dY is at dY[(o co + h' ho) n + w'].
__device__ __forceinline__ float conv33_replicate_dx(const float *dY, int Cout, int co, int ho, int H, int n, const float *W,
                                                     int Cin, int i, int h, int w) {
    int hp[3], ht[3], wp[3], wt[3];  // exactly three pairs each (header comment); the guards keep the arrays' bounds
    int nh = 0, nw = 0;
    for (int a = max(h - 1, 0); a <= min(h + 1, H - 1); ++a)
        for (int dd = 0; dd < 3; ++dd)
            if (min(max(a + dd - 1, 0), H - 1) == h && nh < 3) hp[nh] = a * ho, ht[nh] = dd * 3, ++nh;
    for (int a = max(w - 1, 0); a <= min(w + 1, n - 1); ++a)
        for (int dd = 0; dd < 3; ++dd)
            if (min(max(a + dd - 1, 0), n - 1) == w && nw < 3) wp[nw] = a, wt[nw] = dd, ++nw;
    float acc = 0.f;
    for (int o = 0; o < Cout; ++o) {
        const float *wi = W + ((int64_t)o * Cin + i) * 9;
        const float *po = dY + (int64_t)o * co * n;
        for (int a = 0; a < nh; ++a)
            for (int c = 0; c < nw; ++c) acc = fmaf(wi[ht[a] + wt[c]], po[(int64_t)hp[a] * n + wp[c]], acc);
    }
    return acc;
}

// launch 1 of the backward: the activation gradients of one scene
__global__ __launch_bounds__(kSgThreads) void graphtern_train_bwd_kernel(et_graphtern_params p,
                                                                         const int32_t *__restrict__ off, int64_t N,
                                                                         const float *__restrict__ d_out, float *ws,
                                                                         TrainLayout L) {
    extern __shared__ float lds[];
    const SceneRows R = scene_rows(off, N);
    if (R.empty() || R.n() > kGttMaxN) return;
    const int64_t b = R.b;
    const int n = (int)R.n();
    const GtDims D = gt_dims_of(p);
    const int T = D.T, k = D.k, S = D.S, H = kGtHidden, tid = threadIdx.x;
    const GttScene W = gtt_scene(ws, L, b, n, blockIdx.x);
    float *ar = gt_arena_per_ped(D) * n * 4 <= kSgLdsBytes ? lds : W.f[F_ARENA];
    float *A = ar, *Bf = A + (int64_t)D.qpp * n, *C = Bf + (int64_t)D.qpp * n;

    for (int it = tid; it < k * S * n; it += kSgThreads) {
        const int w = it % n, to = it / n;
        const int t = to / S, o = to - t * S;
        A[it] = d_out[gtt_out_at(t, o, w, S, b, N)];
    }
    __syncthreads();
    for (int j = D.n_cnn - 1; j >= 0; --j) {  // o = prelu(c1(y)) + res(x), y = prelu(c0(x)); A = d o (k,C_out,n)
        const et_graphtern_epcnn &Ep = p.tpcnns[j];
        const GttBlock B = gtt_block(W, D, j);
        const bool last = j + 1 == D.n_cnn;
        const int Rin = j == 0 ? T : k, Cout = last ? S : H;
        for (int it = tid; it < k * Cout * n; it += kSgThreads) {  // d c1
            const float g = A[it];
            B.d_o[it] = g;
            Bf[it] = g * slope(B.c1[it], Ep.cpcn_a);
        }
        __syncthreads();
        for (int it = tid; it < k * H * n; it += kSgThreads) {  // d y = cpcn^T d c1 over the (k, n) plane;  d c0
            const int w = it % n, tc = it / n;
            const int t = tc / H, c = tc - t * H;
            const float v = conv33_replicate_dx(Bf, Cout, 1, Cout, k, n, Ep.cpcn_w, H, c, t, w);
            B.dy[it] = v;
            C[it] = v * slope(B.c0[it], Ep.tpcn_a);
        }
        __syncthreads();
        for (int it = tid; it < Rin * H * n; it += kSgThreads) {  // d x = tpcn^T d c0 over the (16, n) plane + res^T d o
            const int w = it % n, ih = it / n;
            const int i = ih / H, h = ih - i * H;
            const float v = conv33_replicate_dx(C, k, H, 1, H, n, Ep.tpcn_w, Rin, i, h, w);
            float r;
            if (Ep.rest_w) {  // x (T,16,n) -> rows t
                r = 0.f;
                for (int t = 0; t < k; ++t) r = fmaf(Ep.rest_w[t * Rin + i], A[(t * H + h) * n + w], r);
            } else if (Ep.resc_w) {  // x (k,16,n) -> channels o
                r = 0.f;
                for (int o = 0; o < S; ++o) r = fmaf(Ep.resc_w[o * H + h], A[(i * S + o) * n + w], r);
            } else {
                r = A[it];
            }
            Bf[it] = r + v;
        }
        __syncthreads();
        float *tmp = A;
        A = Bf;
        Bf = tmp;
    }
    // A = d x0 (T,16,n); x0[t,c] = tcn(prelu(yp))[c,t] + res(u)[c,t]: the (3,1) conv's transpose -> d y (16,T,n)
    const et_graphtern_layer &Ly = p.tp_mrgcns[0];
    float *dxk = W.f[F_DX0], *dyk = W.f[F_DY];
    for (int it = tid; it < H * T * n; it += kSgThreads) {
        const int w = it % n;
        const int ct = it / n;
        const int ci = ct / T, t = ct - ci * T;
        dxk[it] = A[it];
        float acc = 0.f;
        for (int c = 0; c < H; ++c) {
            const float *wc = Ly.tcn_w + ((int64_t)c * H + ci) * 3;
            if (t + 1 < T) acc = fmaf(wc[0], A[((t + 1) * H + c) * n + w], acc);
            acc = fmaf(wc[1], A[(t * H + c) * n + w], acc);
            if (t > 0) acc = fmaf(wc[2], A[((t - 1) * H + c) * n + w], acc);
        }
        dyk[it] = acc;
    }
}

// d W (Cout,Cin,3,3) of out = conv33_replicate(in) with d out = dsrc slope(pre): item oi = one (o, i) pair, its nine taps in
// one pass over the R n output positions, the input read through the forward's clamps.  Entry (o, h, w) of dsrc / pre is at
// [(o co + h ho) n + w], entry (i, h, w) of in at [(i ci + h ch) n + w]
__device__ __forceinline__ void gtt_conv33_dw(float *dst, int oi, const float *dsrc, const float *pre, const float *a, int co,
                                              int ho, const float *in, int Cin, int ci, int ch, int R, int n) {
    const int i = oi % Cin, o = oi / Cin;
    wave_sum_taps<9>(dst + (int64_t)oi * 9, R * n, [&](int pp, int tap) {
        const int h = pp / n, w = pp - h * n;
        const int hh = min(max(h + tap / 3 - 1, 0), R - 1), ww = min(max(w + tap % 3 - 1, 0), n - 1);
        const int64_t at = ((int64_t)o * co + (int64_t)h * ho) * n + w;
        return (dsrc[at] * slope(pre[at], a)) * in[((int64_t)i * ci + (int64_t)hh * ch) * n + ww];
    });
}

// launch 2 of the backward: the parameter gradients of one scene, grid (scenes, kGttChunks)
__global__ __launch_bounds__(kSgThreads) void graphtern_train_wgrad_kernel(et_graphtern_params p,
                                                                           const int32_t *__restrict__ off, int64_t N,
                                                                           float *ws, TrainLayout L) {
    const SceneRows R = scene_rows(off, N);
    if (R.empty() || R.n() > kGttMaxN) return;
    const int64_t b = R.b;
    const int n = (int)R.n();
    const GtDims D = gt_dims_of(p);
    const int T = D.T, k = D.k, S = D.S, H = kGtHidden;
    const GttScene W = gtt_scene(ws, L, b, n, blockIdx.x);
    const int wv = blockIdx.y * kTrWaves + threadIdx.x / kWave;
    const int cnt = T * n, HTn = H * T * n, Hn = H * n, kn = k * n;
    const et_graphtern_layer &Ly = p.tp_mrgcns[0];
    float *gr = W.part;
    const float *u = W.f[F_U], *Pk = W.f[F_P], *yp = W.f[F_YP], *xk = W.f[F_X0], *dx = W.f[F_DX0], *dy = W.f[F_DY];
    int start = 0;  // items so far (the round robin's phase)
    int at = 0;     // gradient floats so far: the segments below come in gtt_grad_total's (the state_dict's) order
    auto take = [&](int c) {
        float *dst = gr + at;
        at += c;
        return dst;
    };

    // d s[c,(t,w)] = d x0[t,c,w] (the block applies no PReLU of its own);  d yp = d y slope(yp)
    auto ds = [&](int c, int pp) {
        const int t = pp / n, w = pp - t * n;
        return dx[(t * H + c) * n + w];
    };
    auto dyp = [&](int c, int pp) { return dy[(int64_t)c * cnt + pp] * slope(yp[(int64_t)c * cnt + pp], Ly.tcn_prelu); };
    float *d_prelu = take(1);  // never applied by the forward: +0
    segment<kGttWaves>(start, 1, wv, [&](int) {
        if ((threadIdx.x & (kWave - 1)) == 0) d_prelu[0] = 0.f;
    });
    // the gcn through the kept contracted rows: channel o = r 16 + c reads P[r,0] (weight) and P[r,1] (bias)
    for (int jj = 0; jj < 2; ++jj) {
        float *dst = take(kGtRel * H);
        segment<kGttWaves>(start, kGtRel * H, wv, [&](int o) {
            const int r = o / H, c = o - r * H;
            const float *Pr = Pk + (int64_t)(r * 2 + jj) * cnt;
            sum_to(dst + o, cnt, [&](int pp) { return dyp(c, pp) * Pr[pp]; });
        });
    }
    float *d_tcn_a = take(1), *d_tcn_w = take(H * H * 3), *d_tcn_b = take(H), *d_res_w = take(H), *d_res_b = take(H);
    segment<kGttWaves>(start, 1, wv, [&](int) { sum_to(d_tcn_a, HTn, [&](int pp) { return dy[pp] * neg_part(yp[pp]); }); });
    segment<kGttWaves>(start, H * H, wv, [&](int cc) {  // the (3,1) conv on y = prelu(yp)
        const int ci = cc % H, c = cc / H;
        const float *yc = yp + (int64_t)ci * cnt;
        wave_sum_taps<3>(d_tcn_w + cc * 3, cnt, [&](int pp, int tap) {
            const int tt = pp / n + tap - 1;
            if (tt < 0 || tt >= T) return 0.f;
            return ds(c, pp) * prelu(yc[pp + (tap - 1) * n], Ly.tcn_prelu);
        });
    });
    segment<kGttWaves>(start, H, wv, [&](int c) { sum_to(d_tcn_b + c, cnt, [&](int pp) { return ds(c, pp); }); });
    // the residual 1x1 conv from u
    segment<kGttWaves>(start, H, wv, [&](int c) { sum_to(d_res_w + c, cnt, [&](int pp) { return ds(c, pp) * u[pp]; }); });
    segment<kGttWaves>(start, H, wv, [&](int c) { sum_to(d_res_b + c, cnt, [&](int pp) { return ds(c, pp); }); });
    for (int j = 0; j < D.n_cnn; ++j) {
        const et_graphtern_epcnn &Ep = p.tpcnns[j];
        const GttBlock B = gtt_block(W, D, j);
        const bool last = j + 1 == D.n_cnn;
        const int Rin = j == 0 ? T : k, Cout = last ? S : H;
        const float *xin = j == 0 ? xk : gtt_block(W, D, j - 1).o;
        {  // tpcns.0: d c0 = d y slope(c0); output (o,h,w) at (o 16 + h) n + w over the (16, n) plane, input (i,h,w) likewise
            float *d_w = take(k * Rin * 9), *d_b = take(k), *d_a = take(1);
            segment<kGttWaves>(start, k * Rin, wv,
                        [&](int oi) { gtt_conv33_dw(d_w, oi, B.dy, B.c0, Ep.tpcn_a, H, 1, xin, Rin, H, 1, H, n); });
            segment<kGttWaves>(start, k, wv, [&](int o) {
                sum_to(d_b + o, Hn, [&](int pp) {
                    return B.dy[(int64_t)o * Hn + pp] * slope(B.c0[(int64_t)o * Hn + pp], Ep.tpcn_a);
                });
            });
            segment<kGttWaves>(start, 1, wv,
                               [&](int) { sum_to(d_a, k * Hn, [&](int pp) { return B.dy[pp] * neg_part(B.c0[pp]); }); });
        }
        {  // cpcns.0: d c1 = d o slope(c1); output (o,t,w) at (t C_out + o) n + w over the (k, n) plane, input (c,t,w) at (t 16 + c) n + w
            float *d_w = take(Cout * H * 9), *d_b = take(Cout), *d_a = take(1);
            segment<kGttWaves>(start, Cout * H, wv,
                        [&](int oi) { gtt_conv33_dw(d_w, oi, B.d_o, B.c1, Ep.cpcn_a, 1, Cout, B.y, H, 1, H, k, n); });
            segment<kGttWaves>(start, Cout, wv, [&](int o) {
                sum_to(d_b + o, kn, [&](int pp) {
                    const int t = pp / n, w = pp - t * n;
                    const int64_t idx = ((int64_t)t * Cout + o) * n + w;
                    return B.d_o[idx] * slope(B.c1[idx], Ep.cpcn_a);
                });
            });
            segment<kGttWaves>(start, 1, wv,
                        [&](int) { sum_to(d_a, k * Cout * n, [&](int pp) { return B.d_o[pp] * neg_part(B.c1[pp]); }); });
        }
        if (last && S != H) {  // rescconv: the residual 1x1 conv over the channels sees d o
            float *d_rw = take(S * H), *d_rb = take(S);
            segment<kGttWaves>(start, S * H, wv, [&](int oc) {
                const int c = oc % H, o = oc / H;
                sum_to(d_rw + oc, kn, [&](int pp) {
                    const int t = pp / n, w = pp - t * n;
                    return B.d_o[((int64_t)t * S + o) * n + w] * xin[((int64_t)t * H + c) * n + w];
                });
            });
            segment<kGttWaves>(start, S, wv, [&](int o) {
                sum_to(d_rb + o, kn, [&](int pp) {
                    const int t = pp / n, w = pp - t * n;
                    return B.d_o[((int64_t)t * S + o) * n + w];
                });
            });
        }
        if (j == 0) {  // restconv: the residual 1x1 conv over the rows (T -> k) sees d o (k,16,n)
            float *d_rw = take(k * T), *d_rb = take(k);
            segment<kGttWaves>(start, k * T, wv, [&](int ti) {
                const int i = ti % T, t = ti / T;
                sum_to(d_rw + ti, Hn, [&](int pp) { return B.d_o[(int64_t)t * Hn + pp] * xin[(int64_t)i * Hn + pp]; });
            });
            segment<kGttWaves>(start, k, wv,
                               [&](int t) { sum_to(d_rb + t, Hn, [&](int pp) { return B.d_o[(int64_t)t * Hn + pp]; }); });
        }
    }
}

static int gtt_check_params(const et_graphtern_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->n_epgcn != 1) return ET_ERR_UNSUPPORTED;  // deeper stacks send a gradient through the contraction (L^T)
    return gt_check_params(p);
}

template <class Src>
static int gtt_forward(const Src &src, const et_graphtern_params *p, const int32_t *off, int ns, int64_t N,
                       const uint8_t *keep, const int64_t *keep_off, float *out, void *workspace, const TrainLayout &L,
                       et_stream_t stream) {
    hipLaunchKernelGGL((graphtern_train_fwd_kernel<Src>), dim3((unsigned)ns), dim3(kSgThreads), kSgLdsBytes,
                       (hipStream_t)stream, src, *p, off, N, keep, keep_off, out, (float *)workspace, L);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

static int gtt_backward(const et_graphtern_params *p, const int32_t *off, int ns, int64_t N, const float *d_out, float *grads,
                        void *workspace, const TrainLayout &L, et_stream_t stream) {
    if (N > 0) {
        hipLaunchKernelGGL(graphtern_train_bwd_kernel, dim3((unsigned)ns), dim3(kSgThreads), kSgLdsBytes, (hipStream_t)stream,
                           *p, off, N, d_out, (float *)workspace, L);
        ET_LAUNCH_CHECK();
        hipLaunchKernelGGL(graphtern_train_wgrad_kernel, dim3((unsigned)ns, kGttChunks), dim3(kSgThreads), 0,
                           (hipStream_t)stream, *p, off, N, (float *)workspace, L);
        ET_LAUNCH_CHECK();
    }
    return scene_grad_reduce((const float *)workspace + L.o[F_PARTIALS], L.o[F_GRADS], kGttMaxN, off, ns, N, grads, stream);
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_graphtern_train_workspace_bytes(const et_graphtern_params *params, int64_t N, int n_scenes) {
    if (gtt_check_params(params) != ET_OK || N <= 0 || n_scenes < 1) return 0;
    return (size_t)gtt_layout(gt_dims_of(*params), N, n_scenes).o[F_TOTAL] * 4;
}

extern "C" int64_t et_graphtern_grad_floats(const et_graphtern_params *params) {
    if (gtt_check_params(params) != ET_OK) return 0;
    return gtt_grad_total(gt_dims_of(*params));
}

extern "C" int et_graphtern_train_layout(const et_graphtern_params *params, int64_t N, int n_scenes, int64_t *offsets,
                                         int n_offsets) {
    const int rc = gtt_check_params(params);
    if (rc != ET_OK) return rc;
    return layout_out(N, n_scenes, offsets, n_offsets, [&] { return gtt_layout(gt_dims_of(*params), N, n_scenes); });
}

extern "C" int et_graphtern_train_forward_scenes(const et_graphtern_params *params, const float *C_obs, const float *nrm,
                                                 int64_t N, const int32_t *scene_offsets, int n_scenes, const uint8_t *keep,
                                                 const int64_t *keep_offsets, float *C_pred_refine, void *workspace,
                                                 size_t workspace_bytes, et_stream_t stream) {
    const int rc = gtt_check_params(params);
    if (rc != ET_OK) return rc;
    const int early = scene_args_status(N, INT32_MAX, scene_offsets, n_scenes, kGttMaxN);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (keep && scene_offsets && !keep_offsets) return ET_ERR_INVALID_ARG;  // where each scene's block of the mask starts
    const int ns = scene_offsets ? n_scenes : 1;
    const TrainLayout L = gtt_layout(gt_dims_of(*params), N, ns);
    if (!train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return gtt_forward(ScenesSrc{C_obs, nrm, N}, params, scene_offsets, ns, N, keep, scene_offsets ? keep_offsets : nullptr,
                       C_pred_refine, workspace, L, stream);
}

extern "C" int et_graphtern_train_forward_graph(const et_graphtern_params *params, const float *S_obs, int64_t N,
                                                const uint8_t *keep, float *out, void *workspace, size_t workspace_bytes,
                                                et_stream_t stream) {
    const int rc = gtt_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > kGttMaxN) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!S_obs || !out) return ET_ERR_INVALID_ARG;
    const TrainLayout L = gtt_layout(gt_dims_of(*params), N, 1);
    if (!train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return gtt_forward(GraphSrc{S_obs}, params, nullptr, 1, N, keep, nullptr, out, workspace, L, stream);
}

extern "C" int et_graphtern_backward_scenes(const et_graphtern_params *params, int64_t N, const int32_t *scene_offsets,
                                            int n_scenes, const float *d_out, float *grads, int64_t grads_floats,
                                            void *workspace, size_t workspace_bytes, et_stream_t stream) {
    int rc = gtt_check_params(params);
    if (rc != ET_OK) return rc;
    const GtDims D = gt_dims_of(*params);
    rc = backward_args_status(N, scene_offsets, n_scenes, kGttMaxN, d_out, grads, grads_floats, gtt_grad_total(D));
    if (rc != ET_OK) return rc;
    const int ns = scene_offsets ? n_scenes : 1;
    const TrainLayout L = gtt_layout(D, N, ns);
    if (N > 0 && !train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return gtt_backward(params, scene_offsets, ns, N, d_out, grads, workspace, L, stream);
}

extern "C" int et_graphtern_backward_graph(const et_graphtern_params *params, int64_t N, const float *d_out, float *grads,
                                           int64_t grads_floats, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    int rc = gtt_check_params(params);
    if (rc != ET_OK) return rc;
    const GtDims D = gt_dims_of(*params);
    rc = backward_args_status(N, nullptr, 0, kGttMaxN, d_out, grads, grads_floats, gtt_grad_total(D));
    if (rc != ET_OK) return rc;
    const TrainLayout L = gtt_layout(D, N, 1);
    if (N > 0 && !train_ws_fits(L.o[F_TOTAL], workspace, workspace_bytes)) return ET_ERR_WORKSPACE;
    return gtt_backward(params, nullptr, 1, N, d_out, grads, workspace, L, stream);
}

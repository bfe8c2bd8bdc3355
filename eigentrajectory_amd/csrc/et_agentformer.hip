// et_agentformer.hip -- AgentFormer inference (baseline/agentformer: bridge.py hooks, model.py AgentFormerLight.forward,
// agentformer_lib.py agent_aware_attention) for the ET configuration family (include/eigentraj.h "AgentFormer predictor").
//
// The decoder "loop" of decode_traj_batch re-appends the SAME input row every step (nz = 0) under a block-causal mask, so
// its last iteration alone yields every output: ONE decoder pass over k N tokens (DESIGN "AgentFormer").  A scene of n
// pedestrians is T n encoder tokens and k n decoder tokens (token t n + a: frame t, pedestrian a); scene s's tokens lie at
// rows [off[s] T, off[s+1] T) / [off[s] k, off[s+1] k) of every token buffer.  Three kernels:
//   af_prep_kernel   (scene form only) one workgroup per scene: u = [C_obs; obs_ori], obs_ori summed in
//                    et_scene_project's order
//   af_rows_kernel   a workgroup takes 16 token rows, the model_dim-wide row resident in LDS, through a fixed list of
//                    token-wise stages: [embedding: fc(cat[input_fc(u), pe[t]])] -> [out_proj of an attention + residual +
//                    LayerNorm] -> [linear2(relu(linear1)) + residual + LayerNorm] -> store -> [up to two projections of
//                    the row: the next attention's q | k | v and q_self | k_self, or out_fc].  blockIdx.y picks one of two
//                    jobs (encoder / decoder tokens).  Every Linear is v_mfma_f32_16x16x4_f32 in ascending k from a zero
//                    accumulator with the bias added last (the idiom of et_mlp.hip): exact fp32, and an output element
//                    depends on its own row and the layer's shape only.
//   af_attn_kernel   a workgroup takes 16 query rows and four heads (one per wavefront).  Per scene among its rows: the
//                    scores against the scene's keys 16 at a time by MFMA, the entries of the same pedestrian
//                    (i % n == j % n) overwritten with q_self . k_self (an ascending fmaf chain), keys of a later frame
//                    set to -inf (decoder self-attention); TWO passes: the row maximum first, then exp, the row sum and
//                    P V (MFMA, keys ascending) with the scores formed again by the same instructions; the division by
//                    the sum comes last.  Nothing is rescaled on the way, so a row's sums run over the scene's keys in
//                    key order whatever the tile.
// Launches: 1 (prep, scene form) + 1 (both embeddings + layer 0's projections) + 2 per encoder layer (attention; out_proj
// + LN + FFN + LN + the next projections) + 4 per decoder layer (self-attention; out_proj + LN + cross q next to the
// memory's k | v | k_self; cross-attention; out_proj + LN + FFN + LN + the next projections or out_fc):
// 2 + 2 n_enc + 4 n_dec, 14 for ET (2 + 2); the module form runs one fewer (no prep).  No host synchronisation.
// A scene of more than ET_AGENTFORMER_MAX_SCENE_N pedestrians is not computed: its attention rows are NaN, hence its
// outputs.
#include "et_common.h"

#include <math.h>

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_v, scene_of_row, kSnThreads

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAfThreads = kSnThreads;
constexpr int kAfWaves = kAfThreads / kWave;
constexpr int kAfRows = 16;
constexpr int kAfMaxD = 256, kAfMaxFF = 512, kAfMaxT = 16, kAfMaxS = 64;
constexpr int kAfMaxN = ET_AGENTFORMER_MAX_SCENE_N;
constexpr int kAfXStride = kAfMaxD + 4;   // row r of an image starts at bank 4 r
constexpr int kAfBStride = kAfMaxFF + 4;  // the wide image: cat[x, pe] (2 model_dim), an attention's output, the FFN's hidden row
constexpr int kAfPStride = 20;            // a wavefront's 16 x 16 tile of exp(scores)
constexpr float kAfLnEps = 1e-5f;

struct AfScenes {
    const int32_t *off;
    int n_scenes;
    int64_t N;
};

// the scene of pedestrian `ped`: its first row b and its size n (offsets clamped to [0, N])
__device__ __forceinline__ void af_scene(const AfScenes &S, int64_t ped, int64_t &b, int &n) {
    if (!S.off) {
        b = 0, n = (int)S.N;
        return;
    }
    const int s = scene_of_row(S.off, S.n_scenes, ped);
    const int64_t lo = min((int64_t)max(S.off[s], 0), S.N);
    int64_t hi = min((int64_t)max(S.off[s + 1], 0), S.N);
    if (hi < lo) hi = lo;
    b = lo, n = (int)(hi - lo);
}

// u of scene s at ubuf + off[s] T, (T, n); a scene beyond the limit: NaN
__global__ __launch_bounds__(kAfThreads) void af_prep_kernel(const float *__restrict__ C_obs, const float *__restrict__ nrm,
                                                             AfScenes S, int T, float *ubuf, float *gin) {
    __shared__ float red[2 * kAfThreads / kWave];
    int64_t b;
    int n;
    if (S.off) {
        const int64_t lo = min((int64_t)max(S.off[blockIdx.x], 0), S.N);
        int64_t hi = min((int64_t)max(S.off[blockIdx.x + 1], 0), S.N);
        if (hi < lo) hi = lo;
        b = lo, n = (int)(hi - lo);
    } else {
        b = 0, n = (int)S.N;
    }
    if (n <= 0) return;
    const int tid = threadIdx.x;
    const int64_t N = S.N;
    float *vb = ubuf + b * T;
    if (n > kAfMaxN) {
        for (int i = tid; i < T * n; i += kAfThreads) {
            vb[i] = __builtin_nanf("");
            if (gin) gin[(int64_t)(i / n) * N + b + (i % n)] = __builtin_nanf("");
        }
        return;
    }
    scene_v(vb, nullptr, C_obs, nrm, N, b, n, T, red);
    if (gin) {
        __syncthreads();
        for (int i = tid; i < T * n; i += kAfThreads) gin[(int64_t)(i / n) * N + b + (i % n)] = vb[i];
    }
}

// out (16, out) = A (16, in; LDS image of row stride `as`, zeros in columns in .. up4(in)) W^T + B, W (out, in) read in
// place.  epi(i, j, ok, v): row i of the tile, column j (ok: j < out), v = the sum + bias.  No barrier inside.
template <class Epi>
__device__ __forceinline__ void af_linear(const float *A, int as, int in, const float *__restrict__ W,
                                          const float *__restrict__ B, int out, Epi epi) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int col = lane & 15, kq = lane >> 4;
    const int nblk = (out + 15) / 16;
    const float *ar = A + col * as + kq;  // A: row `col` of the tile, k = k0 + kq
    for (int blk = wave; blk < nblk; blk += 2 * kAfWaves) {
        const int j0 = blk * 16 + col, j1 = (blk + kAfWaves) * 16 + col;
        const bool ok0 = j0 < out, ok1 = j1 < out;
        const float *w0 = W + (int64_t)(ok0 ? j0 : 0) * in + kq, *w1 = W + (int64_t)(ok1 ? j1 : 0) * in + kq;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const int inm = in & ~3;
        int k0 = 0;
        for (; k0 + 16 <= inm; k0 += 16) {  // four steps' operands in flight, then the products in k order
            float a[4], t0[4], t1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = ar[k0 + 4 * u], t0[u] = w0[k0 + 4 * u], t1[u] = w1[k0 + 4 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], ok0 ? t0[u] : 0.f, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], ok1 ? t1[u] : 0.f, acc1, 0, 0, 0);
            }
        }
        for (; k0 < inm; k0 += 4) {
            const float a = ar[k0], t0 = w0[k0], t1 = w1[k0];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok0 ? t0 : 0.f, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok1 ? t1 : 0.f, acc1, 0, 0, 0);
        }
        if (inm < in) {  // the last, partial step: the image holds zeros in columns in .. up4(in)
            const bool kok = inm + kq < in;
            const float a = ar[inm];
            const float b0 = (ok0 && kok) ? w0[inm] : 0.f, b1 = (ok1 && kok) ? w1[inm] : 0.f;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((h ? blk + kAfWaves : blk) >= nblk) continue;
            const int j = h ? j1 : j0;
            const bool ok = h ? ok1 : ok0;
            const f32x4 acc = h ? acc1 : acc0;
            const float bias = ok ? B[j] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(4 * kq + r, j, ok, acc[r] + bias);
        }
    }
}

// LayerNorm of the 16 rows of X in place, a wavefront per row: mean, then the biased variance about it, each a per-lane
// sum over columns lane, lane + 64, .. followed by the xor butterfly -- an order that depends on D alone
__device__ __forceinline__ void af_layer_norm(float *X, int D, const float *__restrict__ w, const float *__restrict__ b) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int i = wave; i < kAfRows; i += kAfWaves) {
        float *x = X + i * kAfXStride;
        float s = 0.f;
        for (int c = lane; c < D; c += kWave) s += x[c];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)D;
        float v = 0.f;
        for (int c = lane; c < D; c += kWave) {
            const float d = x[c] - mean;
            v = fmaf(d, d, v);
        }
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        const float rstd = 1.f / sqrtf(v / (float)D + kAfLnEps);
        for (int c = lane; c < D; c += kWave) x[c] = (x[c] - mean) * rstd * w[c] + b[c];
    }
}

struct AfSeg {
    const float *W, *B;  // (n_out, D), (n_out)
    int n_out, n_scaled, dst_col;  // the first n_scaled columns are multiplied by head_dim^-0.5 after the bias
};

struct AfRowsJob {
    int64_t M;  // token rows
    int T;      // token rows per pedestrian (past_frames / future_frames)
    // embedding (fcw set): u holds scene s's (uT, n) block at off[s] uT; dec: every frame's input is the block's last row
    const float *u;
    int uT, dec;
    const float *ifw, *ifb, *fcw, *fcb, *pe;
    const float *xin;                            // else the rows (M, D)
    const float *attn, *ow, *ob, *lnaw, *lnab;   // out_proj of an attention's output (M, D) + residual + LayerNorm
    const float *w1, *b1, *w2, *b2, *lnfw, *lnfb;  // the feed-forward block + residual + LayerNorm
    float *xout;                                 // (M, D)
    int n_seg, final;  // final: segment 0 is out_fc, row (scene, t, a) -> pout[((t N + b + a) pstride + j]
    AfSeg seg[2];
    float *pout;
    int pstride;
};

struct AfRowsLaunch {
    AfRowsJob job[2];
    AfScenes sc;
    int D, ff;
    float scaling;
};

__global__ __launch_bounds__(kAfThreads) void af_rows_kernel(AfRowsLaunch L) {
    __shared__ float X[kAfRows * kAfXStride];
    __shared__ float Bi[kAfRows * kAfBStride];
    __shared__ int64_t sb[kAfRows];
    __shared__ int sn[kAfRows];
    const AfRowsJob &J = L.job[blockIdx.y];
    const int64_t M = J.M, row0 = (int64_t)blockIdx.x * kAfRows;
    if (row0 >= M) return;
    const int tid = threadIdx.x, D = L.D, ff = L.ff;

    if ((J.fcw || J.final) && tid < kAfRows) {
        int64_t b = 0;
        int n = 1;
        if (row0 + tid < M) af_scene(L.sc, (row0 + tid) / J.T, b, n);
        sb[tid] = b, sn[tid] = n < 1 ? 1 : n;
    }
    __syncthreads();
    if (J.fcw) {
        for (int idx = tid; idx < kAfRows * 2 * D; idx += kAfThreads) {
            const int i = idx / (2 * D), c = idx - i * 2 * D;
            const int64_t row = row0 + i;
            float v = 0.f;
            if (row < M) {
                const int64_t b = sb[i];
                const int n = sn[i];
                int64_t local = row - b * J.T;
                if (local < 0 || local >= (int64_t)n * J.T) local = 0;  // (offsets that do not cover the row)
                const int t = (int)(local / n), a = (int)(local - (int64_t)t * n);
                if (c < D) {
                    const float uu = J.u[b * J.uT + (J.dec ? (int64_t)(J.uT - 1) * n + a : local)];
                    v = uu * J.ifw[c] + J.ifb[c];
                } else {
                    v = J.pe[(int64_t)t * D + (c - D)];
                }
            }
            Bi[i * kAfBStride + c] = v;
        }
        __syncthreads();
        af_linear(Bi, kAfBStride, 2 * D, J.fcw, J.fcb, D, [&](int i, int j, bool, float v) { X[i * kAfXStride + j] = v; });
    } else {
        for (int idx = tid; idx < kAfRows * D; idx += kAfThreads) {
            const int i = idx / D, c = idx - i * D;
            X[i * kAfXStride + c] = row0 + i < M ? J.xin[(row0 + i) * D + c] : 0.f;
        }
    }
    __syncthreads();
    if (J.ow) {
        for (int idx = tid; idx < kAfRows * D; idx += kAfThreads) {
            const int i = idx / D, c = idx - i * D;
            Bi[i * kAfBStride + c] = row0 + i < M ? J.attn[(row0 + i) * D + c] : 0.f;
        }
        __syncthreads();
        af_linear(Bi, kAfBStride, D, J.ow, J.ob, D, [&](int i, int j, bool, float v) { X[i * kAfXStride + j] += v; });
        __syncthreads();
        af_layer_norm(X, D, J.lnaw, J.lnab);
        __syncthreads();
    }
    if (J.w1) {
        af_linear(X, kAfXStride, D, J.w1, J.b1, ff, [&](int i, int j, bool ok, float v) {
            Bi[i * kAfBStride + j] = ok ? (v < 0.f ? 0.f : v) : 0.f;  // ReLU; a NaN stays a NaN.  j < 16 ceil(ff / 16) <= 512
        });
        __syncthreads();
        af_linear(Bi, kAfBStride, ff, J.w2, J.b2, D, [&](int i, int j, bool, float v) { X[i * kAfXStride + j] += v; });
        __syncthreads();
        af_layer_norm(X, D, J.lnfw, J.lnfb);
        __syncthreads();
    }
    if (J.xout)
        for (int idx = tid; idx < kAfRows * D; idx += kAfThreads) {
            const int i = idx / D, c = idx - i * D;
            if (row0 + i < M) J.xout[(row0 + i) * D + c] = X[i * kAfXStride + c];
        }
    for (int s = 0; s < J.n_seg; ++s) {
        const AfSeg &G = J.seg[s];
        const bool fin = J.final != 0;
        af_linear(X, kAfXStride, D, G.W, G.B, G.n_out, [&](int i, int j, bool ok, float v) {
            const int64_t row = row0 + i;
            if (!ok || row >= M) return;
            if (j < G.n_scaled) v = v * L.scaling;
            if (fin) {
                const int64_t b = sb[i];
                const int n = sn[i];
                const int64_t local = row - b * J.T;
                if (local < 0 || local >= (int64_t)n * J.T) return;  // (offsets that do not cover the row)
                const int64_t t = local / n, a = local - t * n;
                J.pout[(t * L.sc.N + b + a) * J.pstride + j] = v;
            } else {
                J.pout[row * J.pstride + G.dst_col + j] = v;
            }
        });
    }
}

struct AfAttn {
    const float *q;  // (Mq, qs): q at column q_col, q_self at qself_col (both already scaled)
    int qs, q_col, qself_col;
    const float *kv;  // (Mk, ks): k, v, k_self
    int ks, k_col, v_col, kself_col;
    int Tq, Tk, causal, D, nhead, hd;
    int64_t Mq;
    AfScenes sc;
    float *out;  // (Mq, D)
};

__global__ __launch_bounds__(kAfThreads) void af_attn_kernel(AfAttn P) {
    __shared__ float Pt[kAfWaves][2][kAfRows * kAfPStride];
    __shared__ int64_t sb[kAfRows];
    __shared__ int sn[kAfRows];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int col = lane & 15, kq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * kAfRows;
    const int head = blockIdx.y * kAfWaves + wave;
    const bool live = head < P.nhead;  // an idle wavefront walks the same loops (the barriers) on head 0 and stores nothing
    const int hd = P.hd, hoff = (live ? head : 0) * hd;
    if (tid < kAfRows) {
        int64_t b = -1;
        int n = 0;
        if (row0 + tid < P.Mq) af_scene(P.sc, (row0 + tid) / P.Tq, b, n);
        sb[tid] = b, sn[tid] = n;
    }
    __syncthreads();
    const float ninf = -INFINITY;
    int64_t prev_b = -1;
    for (int i0 = 0; i0 < kAfRows; ++i0) {
        const int64_t b = sb[i0];
        const int n = sn[i0];
        if (b < 0 || b == prev_b || n <= 0) continue;  // (the same for every thread of the workgroup)
        prev_b = b;
        if (n > kAfMaxN) {
            for (int idx = lane; idx < kAfRows * hd; idx += kWave) {
                const int i = idx / hd, d = idx - i * hd;
                if (live && sb[i] == b) P.out[(row0 + i) * P.D + hoff + d] = __builtin_nanf("");
            }
            continue;
        }
        const int Lk = P.Tk * n, nchunk = (Lk + 15) / 16;
        const int64_t qbase = b * P.Tq, kbase = b * P.Tk;
        const int64_t arow = min(row0 + col, P.Mq - 1);  // the A operand's row; a row of another scene is formed and dropped
        const float *qa = P.q + arow * P.qs + P.q_col + hoff + kq;
        bool inr[4];
        int qt[4], qag[4];
        int64_t ri[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * kq + r;
            ri[r] = row0 + i;
            inr[r] = sb[i] == b;
            const int64_t local = inr[r] ? ri[r] - qbase : 0;
            qt[r] = (int)(local / n);
            qag[r] = (int)(local - (int64_t)qt[r] * n);
        }
        // the scores of the tile's rows against keys 16 c .. 16 c + 15: lane (col, kq) holds rows 4 kq + r, key 16 c + col
        auto scores = [&](int c, float *s) {
            const int key = c * 16 + col;
            const bool kvalid = key < Lk;
            const int64_t krow = kbase + (kvalid ? key : 0);
            const float *kb = P.kv + krow * P.ks + P.k_col + hoff + kq;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < hd; k0 += 4) {
                const float kval = kb[k0];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[k0], kvalid ? kval : 0.f, acc, 0, 0, 0);
            }
            const int tk = key / n, ak = key - tk * n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[r];
                if (!kvalid) {
                    v = ninf;
                } else if (inr[r]) {
                    if (ak == qag[r]) {  // the same pedestrian: q_self . k_self
                        const float *qsf = P.q + ri[r] * P.qs + P.qself_col + hoff;
                        const float *ksf = P.kv + krow * P.ks + P.kself_col + hoff;
                        float d = 0.f;
                        for (int e = 0; e < hd; ++e) d = fmaf(qsf[e], ksf[e], d);
                        v = d;
                    }
                    if (P.causal && tk > qt[r]) v = ninf;
                }
                s[r] = v;
            }
        };
        float m[4] = {ninf, ninf, ninf, ninf};
        for (int c = 0; c < nchunk; ++c) {
            float s[4];
            scores(c, s);
#pragma unroll
            for (int r = 0; r < 4; ++r) m[r] = fmaxf(m[r], s[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            for (int o = 8; o > 0; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o));
        for (int g0 = 0; g0 < hd; g0 += 64) {  // 64 columns of the head at a time (one round for head_dim <= 64)
            f32x4 acc[4];
            float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < nchunk; ++c) {
                float s[4];
                scores(c, s);
                float *pt = Pt[wave][c & 1];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = expf(s[r] - m[r]);
                    z[r] += e;
                    pt[(4 * kq + r) * kAfPStride + col] = e;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < 16; kk += 4) {
                    const float a = pt[col * kAfPStride + kk + kq];
                    const int key = c * 16 + kk + kq;
                    const bool kvalid = key < Lk;
                    const float *vb = P.kv + (kbase + (kvalid ? key : 0)) * P.ks + P.v_col + hoff;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int d = g0 + q * 16 + col;
                        if (g0 + q * 16 < hd) {
                            const float bv = (kvalid && d < hd) ? vb[d] : 0.f;
                            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[q], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                for (int o = 8; o > 0; o >>= 1) z[r] += __shfl_xor(z[r], o);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = g0 + q * 16 + col;
                if (g0 + q * 16 >= hd || d >= hd || !live) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (inr[r]) P.out[ri[r] * P.D + hoff + d] = acc[q][r] / z[r];
            }
        }
    }
}

static bool af_attn_ok(const et_agentformer_attn &a) {
    return a.in_proj_weight && a.in_proj_bias && a.in_proj_weight_self && a.in_proj_bias_self && a.out_proj_weight &&
           a.out_proj_bias;
}

static int af_check_params(const et_agentformer_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->motion_dim != 1 || p->model_dim < 16 || p->model_dim > kAfMaxD || p->model_dim % 16 != 0 || p->nhead < 1 ||
        p->model_dim % p->nhead != 0 || (p->model_dim / p->nhead) % 4 != 0 || p->ff_dim < 1 || p->ff_dim > kAfMaxFF ||
        p->n_enc < 1 || p->n_enc > ET_AGENTFORMER_MAX_LAYERS || p->n_dec < 1 || p->n_dec > ET_AGENTFORMER_MAX_LAYERS ||
        p->past_frames < 1 || p->past_frames > kAfMaxT || p->future_frames < 1 || p->future_frames > kAfMaxT ||
        p->forecast_dim < 1 || p->forecast_dim > kAfMaxS)
        return ET_ERR_UNSUPPORTED;
    for (int side = 0; side < 2; ++side) {
        const et_agentformer_embed &e = side ? p->dec_embed : p->enc_embed;
        if (!e.input_fc_weight || !e.input_fc_bias || !e.fc_weight || !e.fc_bias || !e.pe) return ET_ERR_INVALID_ARG;
        const int nl = side ? p->n_dec : p->n_enc;
        for (int l = 0; l < nl; ++l) {
            const et_agentformer_layer &y = side ? p->dec[l] : p->enc[l];
            if (!af_attn_ok(y.self_attn) || (side && !af_attn_ok(y.multihead_attn))) return ET_ERR_INVALID_ARG;
            if (!y.linear1_weight || !y.linear1_bias || !y.linear2_weight || !y.linear2_bias) return ET_ERR_INVALID_ARG;
            for (int i = 0; i < (side ? 3 : 2); ++i)
                if (!y.norm_weight[i] || !y.norm_bias[i]) return ET_ERR_INVALID_ARG;
        }
    }
    if (!p->out_fc_weight || !p->out_fc_bias) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

// the workspace, in floats (every block starts on a multiple of 4)
struct AfWs {
    int64_t u, xe, pe, ae, xd, pd, ad, pq, total;
};

static AfWs af_workspace(const et_agentformer_params &p, int64_t N) {
    AfWs w{};
    int64_t at = 0;
    auto take = [&](int64_t n) {
        const int64_t here = at;
        at += up4(n);
        return here;
    };
    const int64_t ME = N * p.past_frames, MD = N * p.future_frames, D = p.model_dim;
    w.u = take(ME);
    w.xe = take(ME * D);
    w.pe = take(ME * 5 * D);  // q | k | v | q_self | k_self of the encoder; then the memory's k | v | k_self per decoder layer
    w.ae = take(ME * D);
    w.xd = take(MD * D);
    w.pd = take(MD * 5 * D);
    w.ad = take(MD * D);
    w.pq = take(MD * 2 * D);  // the cross-attention's q | q_self
    w.total = at;
    return w;
}

static void af_self_proj(AfRowsJob &J, const et_agentformer_attn &a, int D, float *pout) {
    J.n_seg = 2;
    J.seg[0] = AfSeg{a.in_proj_weight, a.in_proj_bias, 3 * D, D, 0};
    J.seg[1] = AfSeg{a.in_proj_weight_self, a.in_proj_bias_self, 2 * D, D, 3 * D};
    J.pout = pout;
    J.pstride = 5 * D;
}

static void af_attn_stage(AfRowsJob &J, const float *attn, const et_agentformer_attn &a, const float *lw, const float *lb) {
    J.attn = attn, J.ow = a.out_proj_weight, J.ob = a.out_proj_bias, J.lnaw = lw, J.lnab = lb;
}

static void af_ffn_stage(AfRowsJob &J, const et_agentformer_layer &y, int norm) {
    J.w1 = y.linear1_weight, J.b1 = y.linear1_bias, J.w2 = y.linear2_weight, J.b2 = y.linear2_bias;
    J.lnfw = y.norm_weight[norm], J.lnfb = y.norm_bias[norm];
}

static int af_launch_rows(const AfRowsLaunch &L, int jobs, hipStream_t stream) {
    int64_t M = L.job[0].M;
    if (jobs > 1 && L.job[1].M > M) M = L.job[1].M;
    hipLaunchKernelGGL(af_rows_kernel, dim3((unsigned)ceil_div(M, kAfRows), (unsigned)jobs), dim3(kAfThreads), 0, stream, L);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

static int af_launch_attn(const AfAttn &A, hipStream_t stream) {
    hipLaunchKernelGGL(af_attn_kernel, dim3((unsigned)ceil_div(A.Mq, kAfRows), (unsigned)ceil_div(A.nhead, kAfWaves)),
                       dim3(kAfThreads), 0, stream, A);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

// u: scene s's (T, n) block at off[s] T; out (k, N, S)
static int af_run(const et_agentformer_params &p, const float *u, const AfScenes &sc, float *out, float *ws,
                  hipStream_t stream) {
    const int64_t N = sc.N;
    const AfWs W = af_workspace(p, N);
    const int D = p.model_dim, T = p.past_frames, k = p.future_frames, hd = D / p.nhead;
    const int64_t ME = N * T, MD = N * k;
    float *xe = ws + W.xe, *pe = ws + W.pe, *ae = ws + W.ae, *xd = ws + W.xd, *pd = ws + W.pd, *ad = ws + W.ad,
          *pq = ws + W.pq;
    AfRowsLaunch base{};
    base.sc = sc, base.D = D, base.ff = p.ff_dim;
    base.scaling = (float)(1.0 / sqrt((double)hd));
    AfAttn abase{};
    abase.D = D, abase.nhead = p.nhead, abase.hd = hd, abase.sc = sc;
    int rc;

    {  // both embeddings and layer 0's projections
        AfRowsLaunch L = base;
        for (int side = 0; side < 2; ++side) {
            AfRowsJob &J = L.job[side];
            const et_agentformer_embed &e = side ? p.dec_embed : p.enc_embed;
            J.M = side ? MD : ME, J.T = side ? k : T;
            J.u = u, J.uT = T, J.dec = side;
            J.ifw = e.input_fc_weight, J.ifb = e.input_fc_bias, J.fcw = e.fc_weight, J.fcb = e.fc_bias, J.pe = e.pe;
            J.xout = side ? xd : xe;
            af_self_proj(J, side ? p.dec[0].self_attn : p.enc[0].self_attn, D, side ? pd : pe);
        }
        if ((rc = af_launch_rows(L, 2, stream)) != ET_OK) return rc;
    }
    for (int l = 0; l < p.n_enc; ++l) {
        AfAttn A = abase;
        A.q = pe, A.qs = 5 * D, A.q_col = 0, A.qself_col = 3 * D;
        A.kv = pe, A.ks = 5 * D, A.k_col = D, A.v_col = 2 * D, A.kself_col = 4 * D;
        A.Tq = T, A.Tk = T, A.causal = 0, A.Mq = ME, A.out = ae;
        if ((rc = af_launch_attn(A, stream)) != ET_OK) return rc;
        AfRowsLaunch L = base;
        AfRowsJob &J = L.job[0];
        J.M = ME, J.T = T, J.xin = xe, J.xout = xe;
        af_attn_stage(J, ae, p.enc[l].self_attn, p.enc[l].norm_weight[0], p.enc[l].norm_bias[0]);
        af_ffn_stage(J, p.enc[l], 1);
        if (l + 1 < p.n_enc) af_self_proj(J, p.enc[l + 1].self_attn, D, pe);
        if ((rc = af_launch_rows(L, 1, stream)) != ET_OK) return rc;
    }
    for (int l = 0; l < p.n_dec; ++l) {
        const et_agentformer_layer &y = p.dec[l];
        AfAttn A = abase;
        A.q = pd, A.qs = 5 * D, A.q_col = 0, A.qself_col = 3 * D;
        A.kv = pd, A.ks = 5 * D, A.k_col = D, A.v_col = 2 * D, A.kself_col = 4 * D;
        A.Tq = k, A.Tk = k, A.causal = 1, A.Mq = MD, A.out = ad;
        if ((rc = af_launch_attn(A, stream)) != ET_OK) return rc;
        {  // decoder rows: out_proj + norm1, then the cross-attention's q | q_self; memory rows: its k | v | k_self
            AfRowsLaunch L = base;
            AfRowsJob &J = L.job[0];
            J.M = MD, J.T = k, J.xin = xd, J.xout = xd;
            af_attn_stage(J, ad, y.self_attn, y.norm_weight[0], y.norm_bias[0]);
            const et_agentformer_attn &c = y.multihead_attn;
            J.n_seg = 2;
            J.seg[0] = AfSeg{c.in_proj_weight, c.in_proj_bias, D, D, 0};
            J.seg[1] = AfSeg{c.in_proj_weight_self, c.in_proj_bias_self, D, D, D};
            J.pout = pq, J.pstride = 2 * D;
            AfRowsJob &Km = L.job[1];
            Km.M = ME, Km.T = T, Km.xin = xe;
            Km.n_seg = 2;
            Km.seg[0] = AfSeg{c.in_proj_weight + (int64_t)D * D, c.in_proj_bias + D, 2 * D, 0, 0};
            Km.seg[1] = AfSeg{c.in_proj_weight_self + (int64_t)D * D, c.in_proj_bias_self + D, D, 0, 2 * D};
            Km.pout = pe, Km.pstride = 3 * D;
            if ((rc = af_launch_rows(L, 2, stream)) != ET_OK) return rc;
        }
        A = abase;
        A.q = pq, A.qs = 2 * D, A.q_col = 0, A.qself_col = D;
        A.kv = pe, A.ks = 3 * D, A.k_col = 0, A.v_col = D, A.kself_col = 2 * D;
        A.Tq = k, A.Tk = T, A.causal = 0, A.Mq = MD, A.out = ad;
        if ((rc = af_launch_attn(A, stream)) != ET_OK) return rc;
        AfRowsLaunch L = base;
        AfRowsJob &J = L.job[0];
        J.M = MD, J.T = k, J.xin = xd, J.xout = xd;
        af_attn_stage(J, ad, y.multihead_attn, y.norm_weight[1], y.norm_bias[1]);
        af_ffn_stage(J, y, 2);
        if (l + 1 < p.n_dec) {
            af_self_proj(J, p.dec[l + 1].self_attn, D, pd);
        } else {
            J.n_seg = 1, J.final = 1;
            J.seg[0] = AfSeg{p.out_fc_weight, p.out_fc_bias, p.forecast_dim, 0, 0};
            J.pout = out, J.pstride = p.forecast_dim;
        }
        if ((rc = af_launch_rows(L, 1, stream)) != ET_OK) return rc;
    }
    return ET_OK;
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_agentformer_workspace_bytes(const et_agentformer_params *params, int64_t N_total, int64_t max_scene_n) {
    (void)max_scene_n;  // every buffer is per token: the size is linear in N_total whatever the scenes
    if (af_check_params(params) != ET_OK || N_total <= 0 || N_total > INT32_MAX / kAfMaxT) return 0;
    return (size_t)af_workspace(*params, N_total).total * sizeof(float);
}

extern "C" int et_agentformer_forward_graph(const et_agentformer_params *params, const float *pre_motion, int64_t N,
                                            float *seq_out, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = af_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > kAfMaxN) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!pre_motion || !seq_out) return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_agentformer_workspace_bytes(params, N, N)) return ET_ERR_WORKSPACE;
    return af_run(*params, pre_motion, AfScenes{nullptr, 0, N}, seq_out, (float *)workspace, (hipStream_t)stream);
}

extern "C" int et_agentformer_forward_scenes(const et_agentformer_params *params, const float *C_obs, const float *nrm,
                                             int64_t N, const int32_t *scene_offsets, int n_scenes, float *C_pred_refine,
                                             float *graph_inputs, void *workspace, size_t workspace_bytes,
                                             et_stream_t stream) {
    const int rc = af_check_params(params);
    if (rc != ET_OK) return rc;
    if (params->past_frames != params->future_frames + 2) return ET_ERR_UNSUPPORTED;  // u = [C_obs; obs_ori]
    const int early = scene_args_status(N, INT32_MAX / kAfMaxT, scene_offsets, n_scenes, kAfMaxN);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_agentformer_workspace_bytes(params, N, N)) return ET_ERR_WORKSPACE;
    float *ws = (float *)workspace;
    const AfScenes sc{scene_offsets, n_scenes, N};
    float *ubuf = ws + af_workspace(*params, N).u;
    hipLaunchKernelGGL(af_prep_kernel, dim3(scene_offsets ? (unsigned)n_scenes : 1u), dim3(kAfThreads), 0,
                       (hipStream_t)stream, C_obs, nrm, sc, params->past_frames, ubuf, graph_inputs);
    ET_LAUNCH_CHECK();
    return af_run(*params, ubuf, sc, C_pred_refine, ws, (hipStream_t)stream);
}

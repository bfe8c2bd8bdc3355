// et_mlp_train.hip -- training of the `predict` bodies of LBEBM and PECNet (include/eigentraj.h "LBEBM predictor, training",
// "PECNet predictor, training"): the chains of Linear + ReLU forward with their activations kept, PECNet's rounds of
// non-local pooling with theta / phi / g kept, and their backward pass.  Four kernels of its own:
//
// mlp_chain_kernel<MlTrainLaunch>   (et_mlp_chain.inl) the inference kernel's arithmetic, instruction for instruction,
//   plus a store of every hidden layer's activations.  The forward is the inference path's 2 launches.
// mlp_chain_bwd_kernel   a workgroup takes kMlRows = 16 rows of the output gradient backward through ALL layers of one
//   chain; the gradient ping-pongs between the two LDS images the forward keeps its activations in.  Layer l (in -> out):
//   g_a = g_z W_l on v_mfma_f32_16x16x4_f32 with A = g_z (lane l: row l & 15, k = k0 + (l >> 4)) and B = W_l itself (lane
//   l: k = k0 + (l >> 4), column l & 15: W_l[k][column], 16 consecutive floats per k), k0 ascending over the layer's outputs
//   from a zero accumulator; then g_z = g_a where the saved activation is > 0, else 0 (an activation of exactly 0 passes
//   nothing, as torch.relu's backward).  Every hidden g_z is stored for the weight-gradient launch; the gradient of the
//   chain's input is scattered to up to two destinations side by side (the predictor's: the output gradients of the two
//   encoders; an encoder's: the caller's strided tensor, only when asked for -- layer 0 is not run otherwise).  Rows past N,
//   the columns out .. up4(out) of every image and the weights read for them are taken as zeros; a row's gradients depend
//   on that row only.  blockIdx.y picks one of up to three chains (PECNet: theta, phi and g side by side).  A job's output
//   gradient may be the sum of up to four strided terms, added in the order given, and is then stored where asked; a job
//   of no layers does only that (PECNet: the gradient of round 0's features is G + theta's + phi's + g's input gradients,
//   split at fdim and 2 fdim into the encoders' output gradients and the gradient of initial_pos).
// mlp_wgrad_kernel   every dW and db of every layer of the three (PECNet: six) chains in ONE launch.  A wavefront owns a 16 x 32 block
//   of one layer's dW (out, in) = g_z^T a: A = g_z^T (lane l: output o0 + (l & 15), row n0 + (l >> 4)), B = a (lane l: row
//   n0 + (l >> 4), input i0 + (l & 15)), two accumulators side by side, n0 ascending over ALL rows 0 .. N-1 from a zero
//   accumulator: an element is one fp32 fmaf chain over the rows, no atomics, no partial sums, a function of the data
//   alone.  The wavefront of a block row's first block also forms db = the column sums of g_z the same way (B = 1).  The
//   first layer's a is gathered from the strided inputs (the predictor's from the two encoders' outputs).  Rows past N and
//   outputs / inputs past the widths are taken as zeros.  A job has its own row count: theta / phi / g of PECNet run once
//   per pooling round with the SAME weights, their activations and g_z are stacked round after round, and the chain simply
//   runs over nonlocal_pools N rows (round 0's first).  The up to 30 jobs share one table of sources (2.5 KB of kernel
//   arguments; the limit is 4 KB).  The same kernel forms the pooling's column sums: d phi = d f^T theta and d g = p^T G
//   are "weight gradients" of an N-wide layer (no bias), one fmaf chain over the rows i = 0 .. N-1 per element.
// nonlocal_pool_bwd_kernel   one pooling round backwards, the row-wise half, one wavefront per row as the forward: the row
//   of G is summed (in place) from G and the three input gradients of the round after, s and den are formed again with
//   nonlocal_pool_kernel's own statements (same bits; the attention weights are NOT kept by the forward: a kept (N, N)
//   matrix per round would be 64 MB per round at N = 4096), then dp_j = G_i . g_j, the two row sums, p and d f, stored as
//   (N, N) matrices of ONE round for the column sums (the workspace's 2 N^2 floats), and d theta_i = sum_j d f_ij phi_j.
//   Row sums: lane l takes j = l, l + 64, ... ascending (fmaf from zero), then a fixed xor butterfly over the 64 lanes.
//   LDS: 4 wavefronts x (4096 + 1024) floats = 80 KB.  A zero of the mask gives d s = 0 exactly whatever d w is (an
//   all-zero mask row: p = 0, d w = dp / 1e-12 finite, d s = d f = 0, nothing reaches d theta, d phi, d g).
//
// LBEBM's backward pass is 3 launches whatever N and the widths: predictor dX, both encoders' dX, all dW / db.  PECNet's is
// 3 + 3 nonlocal_pools (12 in the ET configuration) whatever N and the number of collated scenes (scenes are separated by
// the block mask only): predictor dX; per round, last to first: pooling rows, pooling column sums, theta / phi / g dX;
// both encoders' dX (+ the gradient of initial_pos); all dW / db.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_of_row, up4, kSnThreads

#include "et_mlp_chain.inl"

constexpr int kMtChains = 3;  // encoder_past, encoder_dest, predictor
constexpr int kPtChains = 6;  // ... non_local_theta, non_local_phi, non_local_g
constexpr int kMtMaxWJobs = kPtChains * ET_MLP_MAX_LAYERS;

struct MbDst {
    float *p;
    int width;
    int64_t rs, cs;  // element (row, c) = p[row * rs + c * cs]
};

// one term of a chain's output gradient: element (row, c) at p[row * rs + c0 + c]
struct MbG {
    const float *p;
    int64_t rs;
    int c0;
};

struct MbJob {
    int n_layers, n_dst;  // n_dst = 0: the input gradient is not wanted; n_layers = 0: only g_out is formed (and kept)
    int n_g;              // g_out = ((g[0] + g[1]) + g[2]) + g[3], the first n_g terms, in this order
    int widths[ET_MLP_MAX_LAYERS + 1];
    const float *w[ET_MLP_MAX_LAYERS];
    const float *act[ET_MLP_MAX_LAYERS];  // act[l], l = 1 .. n_layers-1: the input of layer l, (N, widths[l])
    float *gz[ET_MLP_MAX_LAYERS];         // gz[l], l = 1 .. n_layers-1: the gradient at the output of layer l-1 before its ReLU
    MbG g[4];                             // (N, widths[n_layers])
    MbDst keep;                           // p != null: g_out as summed is stored here
    MbDst dst[3];                         // a destination with p == null is skipped
};

struct MbLaunch {
    MbJob job[3];
    int64_t N;
};

__global__ __launch_bounds__(kMlThreads) void mlp_chain_bwd_kernel(MbLaunch L) {
    extern __shared__ float lds[];
    const MbJob &J = L.job[blockIdx.y];
    const int64_t N = L.N, row0 = (int64_t)blockIdx.x * kMlRows;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float *cur = lds, *nxt = lds + kMlRows * kMlStride;
    {
        const int out = J.widths[J.n_layers], outp = (int)up4(out);
        for (int idx = tid; idx < kMlRows * outp; idx += kMlThreads) {
            const int i = idx / outp, c = idx - i * outp;
            const int64_t row = row0 + i;
            float v = 0.f;
            if (row < N && c < out) {
                v = J.g[0].p[row * J.g[0].rs + J.g[0].c0 + c];
                for (int t = 1; t < J.n_g; ++t) v += J.g[t].p[row * J.g[t].rs + J.g[t].c0 + c];
                if (J.keep.p) J.keep.p[row * J.keep.rs + c * J.keep.cs] = v;
            }
            cur[i * kMlStride + c] = v;
        }
    }
    __syncthreads();

    const int col = lane & 15, kq = lane >> 4;
    const int lmin = J.n_dst > 0 ? 0 : 1;
    for (int l = J.n_layers - 1; l >= lmin; --l) {
        const int in = J.widths[l], out = J.widths[l + 1];  // (16, out) . W (out, in) -> (16, in)
        const float *__restrict__ W = J.w[l];
        const int nblk = (in + 15) / 16;
        const float *ar = cur + col * kMlStride + kq;  // A: row `col` of the tile, k = k0 + kq
        for (int blk = wave; blk < nblk; blk += 2 * kMlWaves) {
            const int j0 = blk * 16 + col, j1 = (blk + kMlWaves) * 16 + col;
            const bool ok0 = j0 < in, ok1 = j1 < in;
            // B: row k0 + kq of W, column j; a column past `in` reads column 0 and is dropped
            const float *w0 = W + (int64_t)kq * in + (ok0 ? j0 : 0), *w1 = W + (int64_t)kq * in + (ok1 ? j1 : 0);
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const int outm = out & ~3;  // whole k steps: rows k0 + kq < outm <= out of W
            int k0 = 0;
            for (; k0 + 16 <= outm; k0 += 16) {  // four steps' operands in flight, then the products in k order
                float a[4], t0[4], t1[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u] = ar[k0 + 4 * u];
                    t0[u] = w0[(int64_t)(k0 + 4 * u) * in];
                    t1[u] = w1[(int64_t)(k0 + 4 * u) * in];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], ok0 ? t0[u] : 0.f, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], ok1 ? t1[u] : 0.f, acc1, 0, 0, 0);
                }
            }
            for (; k0 < outm; k0 += 4) {
                const float a = ar[k0], t0 = w0[(int64_t)k0 * in], t1 = w1[(int64_t)k0 * in];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok0 ? t0 : 0.f, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok1 ? t1 : 0.f, acc1, 0, 0, 0);
            }
            if (outm < out) {  // the last, partial step: the image holds zeros in columns out .. up4(out)
                const bool kok = outm + kq < out;
                const float a = ar[outm];
                const float b0 = (ok0 && kok) ? w0[(int64_t)outm * in] : 0.f;
                const float b1 = (ok1 && kok) ? w1[(int64_t)outm * in] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = h ? j1 : j0;
                const bool ok = h ? ok1 : ok0;
                if ((h ? blk + kMlWaves : blk) >= nblk) continue;
                const f32x4 acc = h ? acc1 : acc0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 4 * kq + r;
                    const int64_t row = row0 + i;
                    const bool live = ok && row < N;
                    if (l > 0) {
                        const float a = live ? J.act[l][row * in + j] : 0.f;
                        const float v = a > 0.f ? acc[r] : 0.f;
                        nxt[i * kMlStride + j] = v;  // j < 16 nblk <= ET_MLP_MAX_WIDTH: inside the row
                        if (live) J.gz[l][row * in + j] = v;
                    } else if (live) {
                        int c = j;
                        for (int d = 0; d < J.n_dst; ++d) {
                            if (c < J.dst[d].width) {
                                if (J.dst[d].p) J.dst[d].p[row * J.dst[d].rs + c * J.dst[d].cs] = acc[r];
                                break;
                            }
                            c -= J.dst[d].width;
                        }
                    }
                }
            }
        }
        __syncthreads();
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
}

struct MwJob {
    int out, in;
    int unit0;           // this layer's wavefront units are [unit0, unit0 + ceil(out / 16) ceil(in / 32))
    short n_src, src0;   // the layer's input a, (rows, in), gathered from MwLaunch::src[src0 .. src0 + n_src)
    int64_t rows;        // the rows summed over: N, or nonlocal_pools N for a chain every pooling round runs
    const float *gz;     // (rows, out)
    float *dw, *db;      // (out, in), (out) or null
};

constexpr int kMtMaxWSrcs = kMtMaxWJobs + 2;  // one per job, the predictor's first layer up to three

struct MwLaunch {
    MwJob job[kMtMaxWJobs];
    MlSrc src[kMtMaxWSrcs];
    int n_jobs, n_units, n_srcs;
};
static_assert(sizeof(MwLaunch) <= 4096, "the kernel arguments of one launch are limited to 4 KB");

__global__ __launch_bounds__(kMlThreads) void mlp_wgrad_kernel(MwLaunch L) {
    const int lane = threadIdx.x & (kWave - 1);
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kMlWaves + threadIdx.x / kWave));
    if (unit >= L.n_units) return;  // (no barrier below)
    int jb = 0;
    while (jb + 1 < L.n_jobs && unit >= L.job[jb + 1].unit0) ++jb;
    const MwJob &J = L.job[jb];
    const int64_t N = J.rows;
    const MlSrc *src = L.src + J.src0;
    const int out = J.out, in = J.in;
    const int nip = (in + 31) / 32;
    const int u = unit - J.unit0, ot = u / nip, ip = u - ot * nip;
    const int col = lane & 15, kq = lane >> 4;
    const int o = ot * 16 + col, i0 = ip * 32 + col, i1 = i0 + 16;
    const bool oko = o < out, ok0 = i0 < in, ok1 = i1 < in;
    const bool bias = ip == 0 && J.db;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    for (int64_t n0 = 0; n0 < N; n0 += 16) {  // four steps' operands in flight, then the products in row order
        float a[4], b0[4], b1[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t n = n0 + 4 * s + kq;
            const bool okn = n < N;
            a[s] = (okn && oko) ? J.gz[n * out + o] : 0.f;
            b0[s] = (okn && ok0) ? gather(src, J.n_src, n, i0) : 0.f;
            b1[s] = (okn && ok1) ? gather(src, J.n_src, n, i1) : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {  // a step wholly past N adds 0 * 0 to every element: its value stays
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b0[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b1[s], acc1, 0, 0, 0);
            if (bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], 1.f, accb, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int orow = ot * 16 + 4 * kq + r;  // D: row 4 (l >> 4) + r, column l & 15
        if (orow >= out) continue;
        if (ok0) J.dw[(int64_t)orow * in + i0] = acc0[r];
        if (ok1) J.dw[(int64_t)orow * in + i1] = acc1[r];
        if (bias && col == 0) J.db[orow] = accb[r];
    }
}


// One pooling round backwards, the row-wise half.  G (N, F) is the gradient at the round's output; the forward was
// f = theta phi^T, s = softmax(f), w = s * mask, den = max(sum |w|, 1e-12), p = w / den, out = p g + feat.
struct PbLaunch {
    const float *theta, *phi, *g;  // the round's (N, D), (N, D), (N, F)
    const float *mask;             // (N, N) or null
    int D, F, n_add;
    int64_t N;
    float *G;             // (N, F), in and out: first G <- ((G + add[0]) + add[1]) + add[2], the first n_add terms
    const float *add[3];  // (N, F) each: the input gradients of theta, phi and g of the round after this one
    float *P, *DF;        // (N, N): p and the gradient at the logits
    float *dtheta;        // (N, D)
};

constexpr int kPbLdsBytes = kAtRows * (ET_MLP_MAX_RANGE + ET_MLP_MAX_WIDTH) * 4;

__global__ __launch_bounds__(kMlThreads) void nonlocal_pool_bwd_kernel(PbLaunch A) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t N = A.N, row = (int64_t)blockIdx.x * kAtRows + wave;
    float *lg = lds + wave * ET_MLP_MAX_RANGE;
    float *gr = lds + kAtRows * ET_MLP_MAX_RANGE + wave * ET_MLP_MAX_WIDTH;  // the row of G
    const int n = row < N ? (int)N : 0;  // (the entries refuse N > ET_MLP_MAX_RANGE)
    const int D = A.D, F = A.F;

    if (row < N) {
        for (int c = lane; c < F; c += kWave) {
            float v = A.G[row * F + c];
            for (int t = 0; t < A.n_add; ++t) v += A.add[t][row * F + c];
            A.G[row * F + c] = v;
            gr[c] = v;
        }
    }
    // s, den: nonlocal_pool_kernel's statements in its order, so the bits are the forward's
    const float *th = A.theta + row * D;
    float m = -INFINITY;
    for (int j = lane; j < n; j += kWave) {
        const float *ph = A.phi + (int64_t)j * D;
        float acc = 0.f;
        for (int c = 0; c < D; ++c) acc = fmaf(th[c], ph[c], acc);
        lg[j] = acc;
        m = fmaxf(m, acc);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float z = 0.f;
    for (int j = lane; j < n; j += kWave) {
        const float ex = expf(lg[j] - m);
        lg[j] = ex;
        z += ex;
    }
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
    float l1 = 0.f;
    for (int j = lane; j < n; j += kWave) {
        const float sj = lg[j] / z;
        float w = sj;
        if (A.mask) w = w * A.mask[row * N + j];
        lg[j] = sj;  // (the forward keeps w here; the backward needs s and forms w again, one product)
        l1 += fabsf(w);
    }
    for (int o = 32; o > 0; o >>= 1) l1 += __shfl_xor(l1, o);
    const float den = fmaxf(l1, 1e-12f);
    const bool clamped = !(l1 > 1e-12f);
    __syncthreads();  // (every wavefront gets here) the row of G is in LDS

    // dp_j = G_i . g_j (parked in DF), p_j, r1 = sum_j dp_j p_j
    float r1 = 0.f;
    for (int j = lane; j < n; j += kWave) {
        float w = lg[j];
        if (A.mask) w = w * A.mask[row * N + j];
        const float p = w / den;
        const float *gj = A.g + (int64_t)j * F;
        float dp = 0.f;
        for (int c = 0; c < F; ++c) dp = fmaf(gr[c], gj[c], dp);
        A.P[row * N + j] = p;
        A.DF[row * N + j] = dp;  // read back by this lane only
        r1 = fmaf(dp, p, r1);
    }
    for (int o = 32; o > 0; o >>= 1) r1 += __shfl_xor(r1, o);
    // ds_j = dw_j mask_j (exactly 0 under a zero of the mask, whatever dw is), r2 = sum_j ds_j s_j
    float r2 = 0.f;
    for (int j = lane; j < n; j += kWave) {
        const float sj = lg[j], mk = A.mask ? A.mask[row * N + j] : 1.f;
        const float w = A.mask ? sj * mk : sj;
        const float dp = A.DF[row * N + j];
        const float sg = w > 0.f ? 1.f : w < 0.f ? -1.f : 0.f;
        const float dw = clamped ? dp / 1e-12f : (dp - sg * r1) / den;
        const float ds = mk == 0.f ? 0.f : (A.mask ? dw * mk : dw);
        A.DF[row * N + j] = ds;
        r2 = fmaf(ds, sj, r2);
    }
    for (int o = 32; o > 0; o >>= 1) r2 += __shfl_xor(r2, o);
    for (int j = lane; j < n; j += kWave) {
        const float df = lg[j] * (A.DF[row * N + j] - r2);
        A.DF[row * N + j] = df;
        lg[j] = df;
    }
    __syncthreads();  // the row's df is in LDS
    if (row < N) {
        for (int c = lane; c < D; c += kWave) {
            float acc = 0.f;
            for (int j = 0; j < n; ++j) acc = fmaf(lg[j], A.phi[(int64_t)j * D + c], acc);
            A.dtheta[row * D + c] = acc;
        }
    }
}

// `saved` and the workspace share one layout, in floats, every block starting on a multiple of 4:
// saved:     ftraj (N, fdim) | dfeat (N, fdim) | per chain (encoder_past, encoder_dest, predictor) a_1 .. a_{L-1}
// workspace: the gradients at the same places: g_ftraj | g_dfeat | per chain g_z(1) .. g_z(L-1)
struct MtLayout {
    int64_t feat[2], act[kMtChains][ET_MLP_MAX_LAYERS], total;
};

static const et_mlp_chain *chain_of(const et_mlp_params &p, int c) {
    return c == 0 ? &p.encoder_past : c == 1 ? &p.encoder_dest : &p.predictor;
}

static MtLayout mt_layout(const et_mlp_params &p, int64_t N) {
    MtLayout w{};
    int64_t at = 0;
    auto take = [&](int64_t width) {
        const int64_t here = at;
        at += up4(N * width);
        return here;
    };
    w.feat[0] = take(p.fdim);
    w.feat[1] = take(p.fdim);
    for (int c = 0; c < kMtChains; ++c) {
        const et_mlp_chain &ch = *chain_of(p, c);
        for (int l = 1; l < ch.n_layers; ++l) w.act[c][l] = take(ch.widths[l]);
    }
    w.total = at;
    return w;
}

static int mt_attributes() {
    static PerDevice<bool> lds_set;
    bool &ok = lds_set.current();
    if (ok) return ET_OK;
    ET_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mlp_chain_kernel<MlTrainLaunch>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kMlLdsBytes));
    ET_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(mlp_chain_bwd_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kMlLdsBytes));
    ET_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(nonlocal_pool_kernel<AtTrainLaunch>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kAtLdsBytes));
    ET_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(nonlocal_pool_bwd_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kPbLdsBytes));
    ok = true;
    return ET_OK;
}

// the checks both entries share
static int mt_check(const et_mlp_params *p, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                    int64_t dest_rs, int64_t dest_cs, int64_t N) {
    const int rc = ml_check_params(p, false);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > INT32_MAX) return ET_ERR_INVALID_ARG;
    if (past_rs < 0 || past_cs < 0 || dest_rs < 0 || dest_cs < 0) return ET_ERR_INVALID_ARG;
    if (N > 0 && (!past || !dest)) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

static int mt_fwd(const et_mlp_params &p, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                  int64_t dest_rs, int64_t dest_cs, int64_t N, float *out, float *saved, hipStream_t stream) {
    const int rc = mt_attributes();
    if (rc != ET_OK) return rc;
    const MtLayout W = mt_layout(p, N);
    const unsigned tiles = (unsigned)((N + kMlRows - 1) / kMlRows);

    MlTrainLaunch L{};
    L.N = N;
    job_of(L.job[0], p.encoder_past, saved + W.feat[0], p.fdim);
    job_of(L.job[1], p.encoder_dest, saved + W.feat[1], p.fdim);
    L.job[0].n_src = L.job[1].n_src = 1;
    L.job[0].src[0] = MlSrc{past, p.encoder_past.widths[0], past_rs, past_cs};
    L.job[1].src[0] = MlSrc{dest, p.encoder_dest.widths[0], dest_rs, dest_cs};
    for (int c = 0; c < 2; ++c)
        for (int l = 1; l < chain_of(p, c)->n_layers; ++l) L.save[c][l - 1] = saved + W.act[c][l];  // layer l-1 outputs a_l
    hipLaunchKernelGGL(mlp_chain_kernel<MlTrainLaunch>, dim3(tiles, 2), dim3(kMlThreads), kMlLdsBytes, stream, L);
    ET_LAUNCH_CHECK();

    MlTrainLaunch P{};
    P.N = N;
    job_of(P.job[0], p.predictor, out, p.out_width);
    P.job[0].n_src = 2;
    P.job[0].src[0] = rows_of(saved + W.feat[0], p.fdim);
    P.job[0].src[1] = rows_of(saved + W.feat[1], p.fdim);
    for (int l = 1; l < p.predictor.n_layers; ++l) P.save[0][l - 1] = saved + W.act[2][l];
    hipLaunchKernelGGL(mlp_chain_kernel<MlTrainLaunch>, dim3(tiles, 1), dim3(kMlThreads), kMlLdsBytes, stream, P);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

// saved_at / at: the offsets of the chain's activation blocks in `saved` / of their gradients in the workspace; skip_rows:
// the rows before a pooling round's in the stacked blocks
static void bwd_job_of(MbJob &j, const et_mlp_chain &c, const float *saved, const int64_t *saved_at, float *ws,
                       const int64_t *at, const float *g_out, int64_t skip_rows = 0) {
    j.n_layers = c.n_layers;
    for (int i = 0; i <= c.n_layers; ++i) j.widths[i] = c.widths[i];
    for (int i = 0; i < c.n_layers; ++i) j.w[i] = c.w[i];
    for (int l = 1; l < c.n_layers; ++l) {
        j.act[l] = saved + saved_at[l] + skip_rows * c.widths[l];
        j.gz[l] = ws + at[l] + skip_rows * c.widths[l];
    }
    j.n_g = 1;
    j.g[0] = MbG{g_out, c.widths[c.n_layers], 0};
}

// a layer's job of the weight-gradient launch; its sources follow with wgrad_src
static MwJob &wgrad_job(MwLaunch &Q, int in, int out, int64_t rows, const float *gz, float *dw, float *db) {
    MwJob &j = Q.job[Q.n_jobs++];
    j.in = in, j.out = out, j.rows = rows;
    j.unit0 = Q.n_units;
    Q.n_units += ((out + 15) / 16) * ((in + 31) / 32);
    j.n_src = 0, j.src0 = (short)Q.n_srcs;
    j.gz = gz, j.dw = dw, j.db = db;
    return j;
}

static void wgrad_src(MwLaunch &Q, MwJob &j, const MlSrc &s) {
    Q.src[Q.n_srcs++] = s;
    ++j.n_src;
}

static void wgrad_launch(const MwLaunch &Q, hipStream_t stream) {
    hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((unsigned)((Q.n_units + kMlWaves - 1) / kMlWaves)), dim3(kMlThreads), 0, stream,
                       Q);
}

static int mt_bwd(const et_mlp_params &p, const float *past, int64_t past_rs, int64_t past_cs, const float *dest,
                  int64_t dest_rs, int64_t dest_cs, int64_t N, const float *saved, const float *g_out,
                  const et_lbebm_grads &G, float *g_past, float *g_dest, float *ws, hipStream_t stream) {
    const int rc = mt_attributes();
    if (rc != ET_OK) return rc;
    const MtLayout W = mt_layout(p, N);
    const unsigned tiles = (unsigned)((N + kMlRows - 1) / kMlRows);
    const int kp = p.encoder_past.widths[0], kd = p.encoder_dest.widths[0];

    if (tiles > 0) {
        MbLaunch P{};
        P.N = N;
        bwd_job_of(P.job[0], p.predictor, saved, W.act[2], ws, W.act[2], g_out);
        P.job[0].n_dst = 2;
        P.job[0].dst[0] = MbDst{ws + W.feat[0], p.fdim, p.fdim, 1};
        P.job[0].dst[1] = MbDst{ws + W.feat[1], p.fdim, p.fdim, 1};
        hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, 1), dim3(kMlThreads), kMlLdsBytes, stream, P);
        ET_LAUNCH_CHECK();

        MbLaunch E{};
        E.N = N;
        bwd_job_of(E.job[0], p.encoder_past, saved, W.act[0], ws, W.act[0], ws + W.feat[0]);
        bwd_job_of(E.job[1], p.encoder_dest, saved, W.act[1], ws, W.act[1], ws + W.feat[1]);
        if (g_past) E.job[0].n_dst = 1, E.job[0].dst[0] = MbDst{g_past, kp, past_rs, past_cs};
        if (g_dest) E.job[1].n_dst = 1, E.job[1].dst[0] = MbDst{g_dest, kd, dest_rs, dest_cs};
        hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, 2), dim3(kMlThreads), kMlLdsBytes, stream, E);
        ET_LAUNCH_CHECK();
    }

    MwLaunch Q{};
    for (int c = 0; c < kMtChains; ++c) {
        const et_mlp_chain &ch = *chain_of(p, c);
        const et_mlp_chain_grads &g = c == 0 ? G.encoder_past : c == 1 ? G.encoder_dest : G.predictor;
        for (int l = 0; l < ch.n_layers; ++l) {
            const float *gz = l + 1 < ch.n_layers ? ws + W.act[c][l + 1] : c == 2 ? g_out : ws + W.feat[c];
            MwJob &j = wgrad_job(Q, ch.widths[l], ch.widths[l + 1], N, gz, g.dw[l], g.db[l]);
            if (l > 0) {
                wgrad_src(Q, j, rows_of(saved + W.act[c][l], j.in));
            } else if (c == 2) {
                wgrad_src(Q, j, rows_of(saved + W.feat[0], p.fdim));
                wgrad_src(Q, j, rows_of(saved + W.feat[1], p.fdim));
            } else {
                wgrad_src(Q, j, c == 0 ? MlSrc{past, kp, past_rs, past_cs} : MlSrc{dest, kd, dest_rs, dest_cs});
            }
        }
    }
    wgrad_launch(Q, stream);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

// ---- PECNet: the six chains of `predict` and nonlocal_pools rounds of pooling.  Chain c: 0 .. 2 as above, 3 .. 5
// non_local_theta, non_local_phi, non_local_g.  Both buffers, in floats, every block starting on a multiple of 4; a block
// "stacked" holds the rounds one after the other, round r at rows r N .. (r + 1) N:
// saved:     ftraj | dfeat | chains 0 .. 2: a_1 .. a_{L-1} | [pools > 0:] the features entering round 0 .. pools-1 and the
//            predictor ((pools + 1) N, F) | theta, phi (pools N, D), g (pools N, F) stacked | chains 3 .. 5: a_1 .. a_{L-1}
//            stacked
// workspace: g_ftraj | g_dfeat | chains 0 .. 2: g_z(1) .. g_z(L-1) | [pools > 0:] G (N, F) | the input gradients of theta,
//            phi, g of one round, 3 (N, F) | d theta, d phi (pools N, D), d g (pools N, F) stacked | chains 3 .. 5: g_z
//            stacked | p (N, N) | d f (N, N)
struct PtLayout {
    int64_t feat[2], act[kPtChains][ET_MLP_MAX_LAYERS], stack, part[3], out[3], pmat, dfmat, total;
};

static const et_mlp_chain *pt_chain(const et_mlp_params &p, int c) {
    return c < kMtChains ? chain_of(p, c) : c == 3 ? &p.non_local_theta : c == 4 ? &p.non_local_phi : &p.non_local_g;
}

static const et_mlp_chain_grads &pt_grads(const et_pecnet_grads &G, int c) {
    return c == 0   ? G.encoder_past
           : c == 1 ? G.encoder_dest
           : c == 2 ? G.predictor
           : c == 3 ? G.non_local_theta
           : c == 4 ? G.non_local_phi
                    : G.non_local_g;
}

static PtLayout pt_layout(const et_mlp_params &p, int64_t N, bool workspace) {
    PtLayout w{};
    int64_t at = 0;
    auto take = [&](int64_t rows, int64_t width) {
        const int64_t here = at;
        at += up4(rows * width);
        return here;
    };
    const int F = feat_width(p), R = p.nonlocal_pools;
    w.feat[0] = take(N, p.fdim);
    w.feat[1] = take(N, p.fdim);
    for (int c = 0; c < kMtChains; ++c)
        for (int l = 1; l < pt_chain(p, c)->n_layers; ++l) w.act[c][l] = take(N, pt_chain(p, c)->widths[l]);
    if (R > 0) {
        if (workspace) {
            w.stack = take(N, F);
            for (int k = 0; k < 3; ++k) w.part[k] = take(N, F);
        } else {
            w.stack = take((R + 1) * N, F);
        }
        w.out[0] = take(R * N, p.non_local_dim);
        w.out[1] = take(R * N, p.non_local_dim);
        w.out[2] = take(R * N, F);
        for (int c = kMtChains; c < kPtChains; ++c)
            for (int l = 1; l < pt_chain(p, c)->n_layers; ++l) w.act[c][l] = take(R * N, pt_chain(p, c)->widths[l]);
        if (workspace) {
            w.pmat = take(N, N);
            w.dfmat = take(N, N);
        }
    }
    w.total = at;
    return w;
}

struct PtIn {
    const float *past, *dest, *pos;
    int64_t past_rs, past_cs, dest_rs, dest_cs, pos_rs, pos_cs;
    const float *mask;
};

// the checks both entries share
static int pt_check(const et_mlp_params *p, const PtIn &in, int64_t N) {
    const int rc = ml_check_params(p, true);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > INT32_MAX) return ET_ERR_INVALID_ARG;
    if (p->nonlocal_pools > 0 && N > ET_MLP_MAX_RANGE) return ET_ERR_UNSUPPORTED;
    if (in.past_rs < 0 || in.past_cs < 0 || in.dest_rs < 0 || in.dest_cs < 0 || in.pos_rs < 0 || in.pos_cs < 0)
        return ET_ERR_INVALID_ARG;
    if (N > 0 && (!in.past || !in.dest || !in.pos)) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

// 2 + 2 nonlocal_pools launches: et_pecnet_predict's, with everything the backward needs kept
static int pt_fwd(const et_mlp_params &p, const PtIn &in, int64_t N, float *out, float *saved, hipStream_t stream) {
    const int rc = mt_attributes();
    if (rc != ET_OK) return rc;
    const PtLayout S = pt_layout(p, N, false);
    const unsigned tiles = (unsigned)((N + kMlRows - 1) / kMlRows);
    const int F = feat_width(p), D = p.non_local_dim;

    MlTrainLaunch L{};
    L.N = N;
    job_of(L.job[0], p.encoder_past, saved + S.feat[0], p.fdim);
    job_of(L.job[1], p.encoder_dest, saved + S.feat[1], p.fdim);
    L.job[0].n_src = L.job[1].n_src = 1;
    L.job[0].src[0] = MlSrc{in.past, p.encoder_past.widths[0], in.past_rs, in.past_cs};
    L.job[1].src[0] = MlSrc{in.dest, p.encoder_dest.widths[0], in.dest_rs, in.dest_cs};
    for (int c = 0; c < 2; ++c)
        for (int l = 1; l < pt_chain(p, c)->n_layers; ++l) L.save[c][l - 1] = saved + S.act[c][l];
    hipLaunchKernelGGL(mlp_chain_kernel<MlTrainLaunch>, dim3(tiles, 2), dim3(kMlThreads), kMlLdsBytes, stream, L);
    ET_LAUNCH_CHECK();

    MlSrc feat[3] = {rows_of(saved + S.feat[0], p.fdim), rows_of(saved + S.feat[1], p.fdim),
                     MlSrc{in.pos, p.pos_width, in.pos_rs, in.pos_cs}};
    int n_feat = 3;
    for (int r = 0; r < p.nonlocal_pools; ++r) {
        float *theta = saved + S.out[0] + r * N * D, *phi = saved + S.out[1] + r * N * D, *g = saved + S.out[2] + r * N * F;
        MlTrainLaunch Q{};
        Q.N = N;
        job_of(Q.job[0], p.non_local_theta, theta, D);
        job_of(Q.job[1], p.non_local_phi, phi, D);
        job_of(Q.job[2], p.non_local_g, g, F);
        for (int j = 0; j < 3; ++j) {
            const et_mlp_chain &ch = *pt_chain(p, kMtChains + j);
            Q.job[j].n_src = n_feat;
            for (int s = 0; s < n_feat; ++s) Q.job[j].src[s] = feat[s];
            for (int l = 1; l < ch.n_layers; ++l) Q.save[j][l - 1] = saved + S.act[kMtChains + j][l] + r * N * ch.widths[l];
        }
        hipLaunchKernelGGL(mlp_chain_kernel<MlTrainLaunch>, dim3(tiles, 3), dim3(kMlThreads), kMlLdsBytes, stream, Q);
        ET_LAUNCH_CHECK();
        AtTrainLaunch A{};
        A.theta = theta, A.phi = phi, A.g = g;
        A.D = D, A.F = F, A.n_src = n_feat;
        for (int s = 0; s < n_feat; ++s) A.src[s] = feat[s];
        A.mask = in.mask, A.off = nullptr, A.n_scenes = 0, A.N = N;
        A.out = saved + S.stack + (r + 1) * N * F;
        A.feat_keep = r == 0 ? saved + S.stack : nullptr;
        hipLaunchKernelGGL(nonlocal_pool_kernel<AtTrainLaunch>, dim3((unsigned)((N + kAtRows - 1) / kAtRows)),
                           dim3(kMlThreads), kAtLdsBytes, stream, A);
        ET_LAUNCH_CHECK();
        feat[0] = rows_of(A.out, F);
        n_feat = 1;
    }

    MlTrainLaunch P{};
    P.N = N;
    job_of(P.job[0], p.predictor, out, p.out_width);
    P.job[0].n_src = n_feat;
    for (int s = 0; s < n_feat; ++s) P.job[0].src[s] = feat[s];
    for (int l = 1; l < p.predictor.n_layers; ++l) P.save[0][l - 1] = saved + S.act[2][l];
    hipLaunchKernelGGL(mlp_chain_kernel<MlTrainLaunch>, dim3(tiles, 1), dim3(kMlThreads), kMlLdsBytes, stream, P);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

// 3 + 3 nonlocal_pools launches: the predictor's rows; per round, last to first, the pooling's rows, its column sums (d phi,
// d g: the weight-gradient kernel, a column of p / d f in the place of a layer's output), theta, phi and g side by side;
// both encoders' rows (with the gradient of initial_pos); every dW / db.
static int pt_bwd(const et_mlp_params &p, const PtIn &in, int64_t N, const float *saved, const float *g_out,
                  const et_pecnet_grads &G, float *g_past, float *g_dest, float *g_pos, float *ws, hipStream_t stream) {
    const int rc = mt_attributes();
    if (rc != ET_OK) return rc;
    const PtLayout S = pt_layout(p, N, false), W = pt_layout(p, N, true);
    const unsigned tiles = (unsigned)((N + kMlRows - 1) / kMlRows);
    const int F = feat_width(p), D = p.non_local_dim, R = p.nonlocal_pools;
    const int kp = p.encoder_past.widths[0], kd = p.encoder_dest.widths[0];
    float *Gf = ws + W.stack;

    if (tiles > 0) {
        MbLaunch P{};
        P.N = N;
        bwd_job_of(P.job[0], p.predictor, saved, S.act[2], ws, W.act[2], g_out);
        if (R > 0) {
            P.job[0].n_dst = 1;
            P.job[0].dst[0] = MbDst{Gf, F, F, 1};
        } else {
            P.job[0].n_dst = 3;
            P.job[0].dst[0] = MbDst{ws + W.feat[0], p.fdim, p.fdim, 1};
            P.job[0].dst[1] = MbDst{ws + W.feat[1], p.fdim, p.fdim, 1};
            P.job[0].dst[2] = MbDst{g_pos, p.pos_width, in.pos_rs, in.pos_cs};
        }
        hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, 1), dim3(kMlThreads), kMlLdsBytes, stream, P);
        ET_LAUNCH_CHECK();

        for (int r = R - 1; r >= 0; --r) {
            const float *theta = saved + S.out[0] + r * N * D, *phi = saved + S.out[1] + r * N * D;
            const float *g = saved + S.out[2] + r * N * F;
            float *d_theta = ws + W.out[0] + r * N * D, *d_phi = ws + W.out[1] + r * N * D, *d_g = ws + W.out[2] + r * N * F;
            PbLaunch A{};
            A.theta = theta, A.phi = phi, A.g = g, A.mask = in.mask;
            A.D = D, A.F = F, A.N = N;
            A.G = Gf;
            A.n_add = r == R - 1 ? 0 : 3;
            for (int k = 0; k < 3; ++k) A.add[k] = ws + W.part[k];
            A.P = ws + W.pmat, A.DF = ws + W.dfmat, A.dtheta = d_theta;
            hipLaunchKernelGGL(nonlocal_pool_bwd_kernel, dim3((unsigned)((N + kAtRows - 1) / kAtRows)), dim3(kMlThreads),
                               kPbLdsBytes, stream, A);
            ET_LAUNCH_CHECK();

            MwLaunch C{};  // d phi = d f^T theta, d g = p^T G: over the rows i ascending
            wgrad_src(C, wgrad_job(C, D, (int)N, N, ws + W.dfmat, d_phi, nullptr), rows_of(theta, D));
            wgrad_src(C, wgrad_job(C, F, (int)N, N, ws + W.pmat, d_g, nullptr), rows_of(Gf, F));
            wgrad_launch(C, stream);
            ET_LAUNCH_CHECK();

            MbLaunch Q{};
            Q.N = N;
            for (int j = 0; j < 3; ++j) {
                bwd_job_of(Q.job[j], *pt_chain(p, kMtChains + j), saved, S.act[kMtChains + j], ws, W.act[kMtChains + j],
                           j == 0 ? d_theta : j == 1 ? d_phi : d_g, r * N);
                Q.job[j].n_dst = 1;
                Q.job[j].dst[0] = MbDst{ws + W.part[j], F, F, 1};
            }
            hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, 3), dim3(kMlThreads), kMlLdsBytes, stream, Q);
            ET_LAUNCH_CHECK();
        }

        MbLaunch E{};
        E.N = N;
        bwd_job_of(E.job[0], p.encoder_past, saved, S.act[0], ws, W.act[0], ws + W.feat[0]);
        bwd_job_of(E.job[1], p.encoder_dest, saved, S.act[1], ws, W.act[1], ws + W.feat[1]);
        if (g_past) E.job[0].n_dst = 1, E.job[0].dst[0] = MbDst{g_past, kp, in.past_rs, in.past_cs};
        if (g_dest) E.job[1].n_dst = 1, E.job[1].dst[0] = MbDst{g_dest, kd, in.dest_rs, in.dest_cs};
        unsigned jobs = 2;
        if (R > 0) {
            // the gradient of round 0's features: G, then the input gradients of theta, phi and g; it splits at fdim, 2 fdim
            E.job[2].n_layers = 0;
            E.job[2].widths[0] = p.pos_width;
            for (int j = 0; j < 3; ++j) {
                MbJob &J = E.job[j];
                J.n_g = 4;
                J.g[0] = MbG{Gf, F, j * p.fdim};
                for (int k = 0; k < 3; ++k) J.g[k + 1] = MbG{ws + W.part[k], F, j * p.fdim};
            }
            E.job[0].keep = MbDst{ws + W.feat[0], p.fdim, p.fdim, 1};
            E.job[1].keep = MbDst{ws + W.feat[1], p.fdim, p.fdim, 1};
            if (g_pos) E.job[2].keep = MbDst{g_pos, p.pos_width, in.pos_rs, in.pos_cs}, jobs = 3;
        }
        hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, jobs), dim3(kMlThreads), kMlLdsBytes, stream, E);
        ET_LAUNCH_CHECK();
    }

    MwLaunch Q{};
    for (int c = 0; c < (R > 0 ? kPtChains : kMtChains); ++c) {
        const et_mlp_chain &ch = *pt_chain(p, c);
        const et_mlp_chain_grads &g = pt_grads(G, c);
        const bool pooled = c >= kMtChains;
        for (int l = 0; l < ch.n_layers; ++l) {
            const float *gz = l + 1 < ch.n_layers ? ws + W.act[c][l + 1]
                              : c == 2            ? g_out
                              : pooled            ? ws + W.out[c - kMtChains]
                                                  : ws + W.feat[c];
            MwJob &j = wgrad_job(Q, ch.widths[l], ch.widths[l + 1], pooled ? R * N : N, gz, g.dw[l], g.db[l]);
            if (l > 0) {
                wgrad_src(Q, j, rows_of(saved + S.act[c][l], j.in));
            } else if (pooled) {
                wgrad_src(Q, j, rows_of(saved + S.stack, F));
            } else if (c == 2 && R > 0) {
                wgrad_src(Q, j, rows_of(saved + S.stack + R * N * F, F));
            } else if (c == 2) {
                wgrad_src(Q, j, rows_of(saved + S.feat[0], p.fdim));
                wgrad_src(Q, j, rows_of(saved + S.feat[1], p.fdim));
                wgrad_src(Q, j, MlSrc{in.pos, p.pos_width, in.pos_rs, in.pos_cs});
            } else {
                wgrad_src(Q, j, c == 0 ? MlSrc{in.past, kp, in.past_rs, in.past_cs} : MlSrc{in.dest, kd, in.dest_rs, in.dest_cs});
            }
        }
    }
    wgrad_launch(Q, stream);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_lbebm_train_workspace_bytes(const et_mlp_params *params, int64_t N) {
    if (ml_check_params(params, false) != ET_OK || N < 0) return 0;
    return (size_t)mt_layout(*params, N).total * 4;
}

extern "C" int et_lbebm_train_fwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs,
                                  const float *dest, int64_t dest_rs, int64_t dest_cs, int64_t N, float *out, float *saved,
                                  void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = mt_check(params, past, past_rs, past_cs, dest, dest_rs, dest_cs, N);
    if (rc != ET_OK) return rc;
    if (N == 0) return ET_OK;
    if (!out || !saved) return ET_ERR_INVALID_ARG;
    (void)workspace, (void)workspace_bytes;  // the forward needs none
    return mt_fwd(*params, past, past_rs, past_cs, dest, dest_rs, dest_cs, N, out, saved, (hipStream_t)stream);
}

extern "C" int et_lbebm_train_bwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs,
                                  const float *dest, int64_t dest_rs, int64_t dest_cs, int64_t N, const float *saved,
                                  const float *g_out, const et_lbebm_grads *grads, float *g_past, float *g_dest,
                                  void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = mt_check(params, past, past_rs, past_cs, dest, dest_rs, dest_cs, N);
    if (rc != ET_OK) return rc;
    if (!grads) return ET_ERR_INVALID_ARG;
    for (int c = 0; c < kMtChains; ++c) {
        const et_mlp_chain_grads &g = c == 0 ? grads->encoder_past : c == 1 ? grads->encoder_dest : grads->predictor;
        for (int l = 0; l < chain_of(*params, c)->n_layers; ++l)
            if (!g.dw[l] || !g.db[l]) return ET_ERR_INVALID_ARG;
    }
    if (N > 0 && (!saved || !g_out)) return ET_ERR_INVALID_ARG;
    if (N > 0 && (!workspace || workspace_bytes < (size_t)mt_layout(*params, N).total * 4)) return ET_ERR_WORKSPACE;
    return mt_bwd(*params, past, past_rs, past_cs, dest, dest_rs, dest_cs, N, saved, g_out, *grads, g_past, g_dest,
                  (float *)workspace, (hipStream_t)stream);
}

extern "C" size_t et_pecnet_train_saved_bytes(const et_mlp_params *params, int64_t N) {
    if (ml_check_params(params, true) != ET_OK || N < 0) return 0;
    return (size_t)pt_layout(*params, N, false).total * 4;
}

extern "C" size_t et_pecnet_train_workspace_bytes(const et_mlp_params *params, int64_t N) {
    if (ml_check_params(params, true) != ET_OK || N < 0) return 0;
    return (size_t)pt_layout(*params, N, true).total * 4;
}

extern "C" int et_pecnet_train_fwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs,
                                   const float *dest, int64_t dest_rs, int64_t dest_cs, const float *initial_pos,
                                   int64_t pos_rs, int64_t pos_cs, const float *mask, int64_t N, float *out, float *saved,
                                   void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const PtIn in{past, dest, initial_pos, past_rs, past_cs, dest_rs, dest_cs, pos_rs, pos_cs, mask};
    const int rc = pt_check(params, in, N);
    if (rc != ET_OK) return rc;
    if (N == 0) return ET_OK;
    if (!out || !saved) return ET_ERR_INVALID_ARG;
    (void)workspace, (void)workspace_bytes;  // the forward needs none
    return pt_fwd(*params, in, N, out, saved, (hipStream_t)stream);
}

extern "C" int et_pecnet_train_bwd(const et_mlp_params *params, const float *past, int64_t past_rs, int64_t past_cs,
                                   const float *dest, int64_t dest_rs, int64_t dest_cs, const float *initial_pos,
                                   int64_t pos_rs, int64_t pos_cs, const float *mask, int64_t N, const float *saved,
                                   const float *g_out, const et_pecnet_grads *grads, float *g_past, float *g_dest,
                                   float *g_pos, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const PtIn in{past, dest, initial_pos, past_rs, past_cs, dest_rs, dest_cs, pos_rs, pos_cs, mask};
    const int rc = pt_check(params, in, N);
    if (rc != ET_OK) return rc;
    if (!grads) return ET_ERR_INVALID_ARG;
    for (int c = 0; c < (params->nonlocal_pools > 0 ? kPtChains : kMtChains); ++c) {
        const et_mlp_chain_grads &g = pt_grads(*grads, c);
        for (int l = 0; l < pt_chain(*params, c)->n_layers; ++l)
            if (!g.dw[l] || !g.db[l]) return ET_ERR_INVALID_ARG;
    }
    if (N > 0 && (!saved || !g_out)) return ET_ERR_INVALID_ARG;
    if (N > 0 && (!workspace || workspace_bytes < (size_t)pt_layout(*params, N, true).total * 4)) return ET_ERR_WORKSPACE;
    return pt_bwd(*params, in, N, saved, g_out, *grads, g_past, g_dest, g_pos, (float *)workspace, (hipStream_t)stream);
}

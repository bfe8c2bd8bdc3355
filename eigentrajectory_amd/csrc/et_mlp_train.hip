// et_mlp_train.hip -- training of the LBEBM predictor's `predict` body (include/eigentraj.h "LBEBM predictor, training"):
// the three chains of Linear + ReLU forward with their activations kept, and their backward pass.  Three kernels:
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
//   on that row only.  blockIdx.y picks one of up to two chains.
// mlp_wgrad_kernel   every dW and db of every layer of the three chains in ONE launch.  A wavefront owns a 16 x 32 block
//   of one layer's dW (out, in) = g_z^T a: A = g_z^T (lane l: output o0 + (l & 15), row n0 + (l >> 4)), B = a (lane l: row
//   n0 + (l >> 4), input i0 + (l & 15)), two accumulators side by side, n0 ascending over ALL rows 0 .. N-1 from a zero
//   accumulator: an element is one fp32 fmaf chain over the rows, no atomics, no partial sums, a function of the data
//   alone.  The wavefront of a block row's first block also forms db = the column sums of g_z the same way (B = 1).  The
//   first layer's a is gathered from the strided inputs (the predictor's from the two encoders' outputs).  Rows past N and
//   outputs / inputs past the widths are taken as zeros.
//
// The backward pass is 3 launches whatever N and the widths: predictor dX, both encoders' dX, all dW / db.
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_of_row, up4, kSnThreads

#include "et_mlp_chain.inl"

constexpr int kMtChains = 3;  // encoder_past, encoder_dest, predictor
constexpr int kMtMaxWJobs = kMtChains * ET_MLP_MAX_LAYERS;

struct MbDst {
    float *p;
    int width;
    int64_t rs, cs;  // element (row, c) = p[row * rs + c * cs]
};

struct MbJob {
    int n_layers, n_dst;  // n_dst = 0: the input gradient is not wanted
    int widths[ET_MLP_MAX_LAYERS + 1];
    const float *w[ET_MLP_MAX_LAYERS];
    const float *act[ET_MLP_MAX_LAYERS];  // act[l], l = 1 .. n_layers-1: the input of layer l, (N, widths[l])
    float *gz[ET_MLP_MAX_LAYERS];         // gz[l], l = 1 .. n_layers-1: the gradient at the output of layer l-1 before its ReLU
    const float *g_out;                   // (N, widths[n_layers])
    MbDst dst[2];
};

struct MbLaunch {
    MbJob job[2];
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
            cur[i * kMlStride + c] = (row < N && c < out) ? J.g_out[row * out + c] : 0.f;
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
                                J.dst[d].p[row * J.dst[d].rs + c * J.dst[d].cs] = acc[r];
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
    int out, in, n_src;
    int unit0;         // this layer's wavefront units are [unit0, unit0 + ceil(out / 16) ceil(in / 32))
    MlSrc src[2];      // the layer's input a, (N, in), gathered
    const float *gz;   // (N, out)
    float *dw, *db;    // (out, in), (out)
};

struct MwLaunch {
    MwJob job[kMtMaxWJobs];
    int n_jobs, n_units;
    int64_t N;
};

__global__ __launch_bounds__(kMlThreads) void mlp_wgrad_kernel(MwLaunch L) {
    const int lane = threadIdx.x & (kWave - 1);
    const int unit = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kMlWaves + threadIdx.x / kWave));
    if (unit >= L.n_units) return;  // (no barrier below)
    int jb = 0;
    while (jb + 1 < L.n_jobs && unit >= L.job[jb + 1].unit0) ++jb;
    const MwJob &J = L.job[jb];
    const int64_t N = L.N;
    const int out = J.out, in = J.in;
    const int nip = (in + 31) / 32;
    const int u = unit - J.unit0, ot = u / nip, ip = u - ot * nip;
    const int col = lane & 15, kq = lane >> 4;
    const int o = ot * 16 + col, i0 = ip * 32 + col, i1 = i0 + 16;
    const bool oko = o < out, ok0 = i0 < in, ok1 = i1 < in;
    const bool bias = ip == 0;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    for (int64_t n0 = 0; n0 < N; n0 += 16) {  // four steps' operands in flight, then the products in row order
        float a[4], b0[4], b1[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t n = n0 + 4 * s + kq;
            const bool okn = n < N;
            a[s] = (okn && oko) ? J.gz[n * out + o] : 0.f;
            b0[s] = (okn && ok0) ? gather(J.src, J.n_src, n, i0) : 0.f;
            b1[s] = (okn && ok1) ? gather(J.src, J.n_src, n, i1) : 0.f;
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

static void bwd_job_of(MbJob &j, const et_mlp_chain &c, const float *saved, float *ws, const int64_t *at,
                       const float *g_out) {
    j.n_layers = c.n_layers;
    for (int i = 0; i <= c.n_layers; ++i) j.widths[i] = c.widths[i];
    for (int i = 0; i < c.n_layers; ++i) j.w[i] = c.w[i];
    for (int l = 1; l < c.n_layers; ++l) j.act[l] = saved + at[l], j.gz[l] = ws + at[l];
    j.g_out = g_out;
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
        bwd_job_of(P.job[0], p.predictor, saved, ws, W.act[2], g_out);
        P.job[0].n_dst = 2;
        P.job[0].dst[0] = MbDst{ws + W.feat[0], p.fdim, p.fdim, 1};
        P.job[0].dst[1] = MbDst{ws + W.feat[1], p.fdim, p.fdim, 1};
        hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, 1), dim3(kMlThreads), kMlLdsBytes, stream, P);
        ET_LAUNCH_CHECK();

        MbLaunch E{};
        E.N = N;
        bwd_job_of(E.job[0], p.encoder_past, saved, ws, W.act[0], ws + W.feat[0]);
        bwd_job_of(E.job[1], p.encoder_dest, saved, ws, W.act[1], ws + W.feat[1]);
        if (g_past) E.job[0].n_dst = 1, E.job[0].dst[0] = MbDst{g_past, kp, past_rs, past_cs};
        if (g_dest) E.job[1].n_dst = 1, E.job[1].dst[0] = MbDst{g_dest, kd, dest_rs, dest_cs};
        hipLaunchKernelGGL(mlp_chain_bwd_kernel, dim3(tiles, 2), dim3(kMlThreads), kMlLdsBytes, stream, E);
        ET_LAUNCH_CHECK();
    }

    MwLaunch Q{};
    Q.N = N;
    int units = 0;
    for (int c = 0; c < kMtChains; ++c) {
        const et_mlp_chain &ch = *chain_of(p, c);
        const et_mlp_chain_grads &g = c == 0 ? G.encoder_past : c == 1 ? G.encoder_dest : G.predictor;
        for (int l = 0; l < ch.n_layers; ++l) {
            MwJob &j = Q.job[Q.n_jobs++];
            j.in = ch.widths[l], j.out = ch.widths[l + 1];
            j.unit0 = units;
            units += ((j.out + 15) / 16) * ((j.in + 31) / 32);
            if (l > 0) {
                j.n_src = 1, j.src[0] = rows_of(saved + W.act[c][l], j.in);
            } else if (c == 2) {
                j.n_src = 2, j.src[0] = rows_of(saved + W.feat[0], p.fdim), j.src[1] = rows_of(saved + W.feat[1], p.fdim);
            } else {
                j.n_src = 1, j.src[0] = c == 0 ? MlSrc{past, kp, past_rs, past_cs} : MlSrc{dest, kd, dest_rs, dest_cs};
            }
            j.gz = l + 1 < ch.n_layers ? ws + W.act[c][l + 1] : c == 2 ? g_out : ws + W.feat[c];
            j.dw = g.dw[l], j.db = g.db[l];
        }
    }
    Q.n_units = units;
    hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((unsigned)((units + kMlWaves - 1) / kMlWaves)), dim3(kMlThreads), 0, stream, Q);
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

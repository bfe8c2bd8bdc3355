// et_metrics.hip -- the reference's four test metrics per pedestrian (utils/metrics.py:30-155, utils/trainer.py:173-195):
// best-of-S ADE / FDE, the best sample's index, TCC (temporal correlation coefficient) and COL (collision rate), batched
// over scenes in one launch.
//
// Semantics (utils/metrics.py):
//   best  argmin over samples of the final-step displacement (:114-115); first index on ties, the first NaN wins
//   TCC   per coordinate the Pearson correlation over the T steps of the best sample and gt, covariance factor 1/(T-1),
//         clamped to [-1, 1], NaN -> 0, mean of the two coordinates (:116-129).  The means are pairwise (binary-counter)
//         tree sums / T: for a motionless coordinate that equals ATen's mean bit for bit, so the rows where the reference
//         gets exactly 0 get exactly 0 here.
//   COL   the densified path p0 + cumsum of each step's increment / 4, four times (:145-149; the sum runs in fp64 and is
//         rounded per instant, as ATen's CPU cumsum does), its first min(14, 1 + 4 (T-1)) instants; a pair of pedestrians
//         of the same scene collides when its minimum same-instant distance is strictly below 0.2 (:150-152; a NaN
//         instant makes the minimum NaN: no collision); COL = 100 * (samples with a collision) / S (:153).
//
// Layout: lane = pedestrian, 256 consecutive rows per workgroup -- scenes are contiguous row ranges, so small scenes pack
// into one workgroup by construction.  Per sample, the densified paths of the rows the workgroup's scenes span are staged
// in LDS tiles of 256 rows (14 float2 = 112 B per row); each lane scans the rows of its own scene in the tile.  Scenes
// larger than a tile loop over tiles.  ADE / FDE / arg-min stream over the samples; TCC re-reads the best sample (two
// passes: means, then the covariances).
//
// Sample sources: TensorSrc reads pred (S,N,T,2); CoefSrc reconstructs each (sample, pedestrian) in registers from the
// coefficients with the arithmetic of et_anchor_reconstruct_fwd (reconstruct_tile_kernel / reconstruct_generic_kernel:
// anchor add, the j-ordered fmaf chain, denormalize_point), so that the fused form equals the tensor form applied to that
// call's output.
#include "et_common.h"

namespace et {

constexpr int kMtThreads = 256;                 // rows per workgroup = rows per LDS tile
constexpr int kColInstants = 14;                // 3 * num_interp + 2 (utils/metrics.py:150)
constexpr int kColPitch = 2 * kColInstants;     // floats per staged row
constexpr int kColSteps = 5;                    // trajectory points the 14 instants depend on
constexpr int kTreeLevels = 6;                  // binary-counter tree over T <= ET_MAX_T = 32 terms

struct TensorSrc {
    const float *pred;
    int64_t N;
    int T;
    struct Row {};
    struct Sample {
        const float2 *p;
    };
    __device__ Row row(int64_t) const { return {}; }
    __device__ Sample sample(const Row &, int64_t n, int s) const {
        return {reinterpret_cast<const float2 *>(pred + ((int64_t)s * N + n) * 2 * T)};
    }
    __device__ float2 point(const Row &, const Sample &q, int t) const { return q.p[t]; }
};

// pose (5,N) = ox, oy, c sca, s sca, +-1/sca (store_pose in et_descriptor.hip): c and s are recovered as (c sca) / sca,
// exact for static rows (sca = 1), within an ulp or two for moving rows
__device__ __forceinline__ RowNorm pose_row_norm(const float *__restrict__ pose, int64_t N, int64_t n) {
    RowNorm p;
    const float w = pose[4 * N + n];
    p.ox = pose[n];
    p.oy = pose[N + n];
    p.mv = (__float_as_uint(w) >> 31) ? 1 : 0;
    p.inv = fabsf(w);
    p.sca = p.mv ? 1.0f / p.inv : 1.0f;
    p.c = p.mv ? pose[2 * N + n] * p.inv : pose[2 * N + n];
    p.s = p.mv ? pose[3 * N + n] * p.inv : pose[3 * N + n];
    return p;
}

template <int KMAX>
struct CoefSrc {
    const float *C;
    int64_t N;
    int S, k, T_obs;
    const float *obs, *nrm, *pose, *A_m, *A_s, *U_m, *U_s;
    int mode;
    float static_dist;
    struct Row {
        RowNorm p;
        const float *U, *A;
    };
    // KMAX > 0: the k <= KMAX anchored coefficients of a sample in registers; KMAX == 0 (any k): re-read per point
    struct Sample {
        float c[KMAX > 0 ? KMAX : 1];
        int64_t n;
        int s;
    };
    __device__ Row row(int64_t n) const {
        Row r;
        r.p = (mode == ET_MODE_IDENTITY || nrm || obs) ? load_row_norm(nrm, obs, N, n, T_obs, mode, static_dist)
                                                        : pose_row_norm(pose, N, n);
        r.U = r.p.mv ? U_m : U_s;
        r.A = r.p.mv ? A_m : A_s;
        return r;
    }
    __device__ float coef(const Row &r, int64_t n, int s, int j) const {
        const float cj = C[((int64_t)j * N + n) * S + s];
        return r.A ? r.A[j * S + s] + cj : cj;  // anchor.py:87
    }
    __device__ Sample sample(const Row &r, int64_t n, int s) const {
        Sample q;
        q.n = n;
        q.s = s;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) q.c[j] = j < k ? coef(r, n, s, j) : 0.f;
        return q;
    }
    __device__ float2 point(const Row &r, const Sample &q, int t) const {
        float vx = 0.f, vy = 0.f;
        if constexpr (KMAX > 0) {
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < k) vx = fmaf(r.U[(2 * t) * k + j], q.c[j], vx);  // descriptor.py:87
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < k) vy = fmaf(r.U[(2 * t + 1) * k + j], q.c[j], vy);
        } else {
            for (int j = 0; j < k; ++j) vx = fmaf(r.U[(2 * t) * k + j], coef(r, q.n, q.s, j), vx);
            for (int j = 0; j < k; ++j) vy = fmaf(r.U[(2 * t + 1) * k + j], coef(r, q.n, q.s, j), vy);
        }
        float2 o;
        denormalize_point(r.p, vx, vy, o.x, o.y);
        return o;
    }
};

// [lo, hi): the scene of row n (offsets NULL: one scene of N).  Rows outside every scene of malformed offsets are scenes
// of their own; callers clamp every row index they derive to [0, N).
__device__ __forceinline__ void scene_of(const int32_t *__restrict__ off, int n_scenes, int64_t N, int64_t n, int64_t &lo,
                                         int64_t &hi) {
    if (!off) {
        lo = 0;
        hi = N;
        return;
    }
    int a = 0, b = n_scenes;  // largest a < n_scenes with off[a] <= n
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (off[m] <= n) a = m;
        else b = m;
    }
    lo = off[a];
    hi = off[a + 1];
    if (!(lo <= n && n < hi)) {
        lo = n;
        hi = n + 1;
    }
}

// utils/metrics.py:145-149: p0, then each step's increment / 4 added four times; the running sum in fp64, every instant
// rounded to fp32 (ATen's CPU cumsum accumulates float in double).  Instants >= M are left at 0.
template <class Src>
__device__ __forceinline__ void dense_path(const Src &src, const typename Src::Row &r, const typename Src::Sample &q, int T,
                                           float2 (&d)[kColInstants]) {
    float2 prev = src.point(r, q, 0);
    d[0] = prev;
    double ax = prev.x, ay = prev.y;
#pragma unroll
    for (int t = 1; t < kColSteps; ++t) {
        if (t < T) {
            const float2 v = src.point(r, q, t);
            const float rx = (v.x - prev.x) / 4.0f, ry = (v.y - prev.y) / 4.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = 4 * (t - 1) + 1 + e;
                if (m < kColInstants) {
                    ax = ax + (double)rx;
                    ay = ay + (double)ry;
                    d[m] = make_float2((float)ax, (float)ay);
                }
            }
            prev = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = 4 * (t - 1) + 1 + e;
                if (m < kColInstants) d[m] = make_float2(0.f, 0.f);
            }
        }
    }
}

// pairwise sum as a binary counter: term t merges with the partial sums of the completed power-of-two blocks before it
// (12 terms: ((0..7) + (8..11)), every block summed by halves); static register indices only
__device__ __forceinline__ void tree_push(float (&st)[kTreeLevels], int t, float x) {
    bool done = false;
#pragma unroll
    for (int l = 0; l < kTreeLevels; ++l) {
        if (!done) {
            if ((t >> l) & 1) {
                x = st[l] + x;
            } else {
                st[l] = x;
                done = true;
            }
        }
    }
}
__device__ __forceinline__ float tree_total(const float (&st)[kTreeLevels], int T) {
    float acc = 0.f;
    bool any = false;
#pragma unroll
    for (int l = 0; l < kTreeLevels; ++l) {
        if ((T >> l) & 1) {
            acc = any ? st[l] + acc : st[l];
            any = true;
        }
    }
    return acc;
}

// utils/metrics.py:120-128 for one coordinate: cov[0][1] / std[0] / std[1], clamped, NaN -> 0
__device__ __forceinline__ float corr_coef(float cpg, float cpp, float cgg) {
    const float r = (cpg / sqrtf(cpp)) / sqrtf(cgg);
    return isnan(r) ? 0.f : fminf(fmaxf(r, -1.f), 1.f);
}

template <class Src>
__global__ __launch_bounds__(kMtThreads) void traj_metrics_kernel(Src src, int64_t N, int S, int T,
                                                                  const float *__restrict__ gt,
                                                                  const int32_t *__restrict__ off, int n_scenes,
                                                                  float *__restrict__ ade, float *__restrict__ fde,
                                                                  float *__restrict__ tcc, float *__restrict__ col,
                                                                  int32_t *__restrict__ best) {
    __shared__ __attribute__((aligned(16))) float sDense[kMtThreads * kColPitch];  // 28 KB
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kMtThreads;
    const int64_t i = r0 + tid;
    const bool live = i < N;
    const float2 *gt2 = reinterpret_cast<const float2 *>(gt);
    const int M = min(kColInstants, 1 + 4 * (T - 1));

    // the rows this workgroup's scenes span: [scene start of its first row, scene end of its last row)
    int64_t blo, bhi, lo, hi, unused;
    scene_of(off, n_scenes, N, r0, blo, unused);
    scene_of(off, n_scenes, N, min(r0 + kMtThreads, N) - 1, unused, bhi);
    blo = max(blo, (int64_t)0);
    bhi = min(bhi, N);
    scene_of(off, n_scenes, N, live ? i : r0, lo, hi);
    lo = max(lo, blo);
    hi = min(hi, bhi);
    const int tiles = bhi > blo ? (int)ceil_div(bhi - blo, kMtThreads) : 0;

    const typename Src::Row row = src.row(live ? i : r0);
    float best_a = 0.f, best_f = 0.f;
    int best_s = 0, ncol = 0;
    for (int s = 0; s < S; ++s) {
        float2 own[kColInstants];
        if (live) {
            const typename Src::Sample q = src.sample(row, i, s);
            float sum = 0.f, last = 0.f;
            for (int t = 0; t < T; ++t) {
                const float2 v = src.point(row, q, t), g = gt2[i * T + t];
                const float ex = v.x - g.x, ey = v.y - g.y;
                last = sqrtf(fmaf(ey, ey, ex * ex));  // utils/metrics.py:84 (ATen's 2-norm of a pair)
                sum = sum + last;
            }
            const float va = sum / (float)T;
            if (s == 0 || va < best_a || isnan(va)) best_a = va;  // torch.min propagates NaN
            if (s == 0 || (!isnan(best_f) && (last < best_f || isnan(last)))) {  // argmin: first minimum / first NaN
                best_f = last;
                best_s = s;
            }
            if (col) dense_path(src, row, q, T, own);
        }
        if (!col) continue;
        bool hit = false;
        for (int tl = 0; tl < tiles; ++tl) {
            const int64_t t0 = blo + (int64_t)tl * kMtThreads;
            const int rows = (int)min((int64_t)kMtThreads, bhi - t0);
            __syncthreads();  // the previous tile's scan is done
            if (tid < rows) {
                const int64_t j = t0 + tid;
                const typename Src::Row rj = src.row(j);
                float2 d[kColInstants];
                dense_path(src, rj, src.sample(rj, j, s), T, d);
                float4 *dst = reinterpret_cast<float4 *>(sDense + tid * kColPitch);
#pragma unroll
                for (int m = 0; m < kColInstants / 2; ++m)
                    dst[m] = make_float4(d[2 * m].x, d[2 * m].y, d[2 * m + 1].x, d[2 * m + 1].y);
            }
            __syncthreads();
            if (!live || hit) continue;
            const int64_t jb = max(lo, t0), je = min(hi, t0 + rows);
            for (int64_t j = jb; j < je && !hit; ++j) {
                if (j == i) continue;  // the +eye of :152: a pedestrian never collides with itself
                const float4 *rj = reinterpret_cast<const float4 *>(sDense + (int)(j - t0) * kColPitch);
                float qmin = 0.f;
#pragma unroll
                for (int m2 = 0; m2 < kColInstants / 2; ++m2) {
                    const float4 v = rj[m2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int m = 2 * m2 + e;
                        const float dx = own[m].x - (e ? v.z : v.x), dy = own[m].y - (e ? v.w : v.y);
                        const float qq = fmaf(dy, dy, dx * dx);
                        if (m < M && (m == 0 || qq < qmin || isnan(qq))) qmin = qq;  // NaN-propagating minimum
                    }
                }
                // sqrt is monotonic: min_m sqrt(q_m) = sqrt(min_m q_m), NaN included
                hit = sqrtf(qmin) < 0.2f;
            }
        }
        ncol += hit ? 1 : 0;
    }
    if (!live) return;
    if (ade) ade[i] = best_a;
    if (fde) fde[i] = best_f;
    if (best) best[i] = best_s;
    if (col) col[i] = ((float)ncol / (float)S) * 100.0f;  // utils/metrics.py:153
    if (!tcc) return;
    const typename Src::Sample q = src.sample(row, i, best_s);
    float spx[kTreeLevels], spy[kTreeLevels], sgx[kTreeLevels], sgy[kTreeLevels];
#pragma unroll
    for (int l = 0; l < kTreeLevels; ++l) spx[l] = spy[l] = sgx[l] = sgy[l] = 0.f;
    for (int t = 0; t < T; ++t) {
        const float2 v = src.point(row, q, t), g = gt2[i * T + t];
        tree_push(spx, t, v.x);
        tree_push(spy, t, v.y);
        tree_push(sgx, t, g.x);
        tree_push(sgy, t, g.y);
    }
    const float mpx = tree_total(spx, T) / (float)T, mpy = tree_total(spy, T) / (float)T;
    const float mgx = tree_total(sgx, T) / (float)T, mgy = tree_total(sgy, T) / (float)T;
    const float factor = (float)(1.0 / (double)(T - 1));  // :121, applied to the first factor of :122's product
    float xpg = 0.f, xpp = 0.f, xgg = 0.f, ypg = 0.f, ypp = 0.f, ygg = 0.f;
    for (int t = 0; t < T; ++t) {
        const float2 v = src.point(row, q, t), g = gt2[i * T + t];
        const float ax = v.x - mpx, bx = g.x - mgx, ay = v.y - mpy, by = g.y - mgy;
        const float fax = factor * ax, fbx = factor * bx, fay = factor * ay, fby = factor * by;
        xpg = fmaf(fax, bx, xpg);
        xpp = fmaf(fax, ax, xpp);
        xgg = fmaf(fbx, bx, xgg);
        ypg = fmaf(fay, by, ypg);
        ypp = fmaf(fay, ay, ypp);
        ygg = fmaf(fby, by, ygg);
    }
    tcc[i] = (corr_coef(xpg, xpp, xgg) + corr_coef(ypg, ypp, ygg)) / 2.0f;  // :129 mean over the coordinates
}

template <class Src>
static int launch(const Src &src, int64_t N, int S, int T, const float *gt, const int32_t *off, int n_scenes, float *ade,
                  float *fde, float *tcc, float *col, int32_t *best, et_stream_t stream) {
    hipLaunchKernelGGL((traj_metrics_kernel<Src>), dim3((unsigned)ceil_div(N, kMtThreads)), dim3(kMtThreads), 0,
                       (hipStream_t)stream, src, N, S, T, gt, off, n_scenes, ade, fde, tcc, col, best);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

static bool common_args_ok(int64_t N, int S, int T, const float *gt, const int32_t *off, int n_scenes) {
    if (N < 0 || S < 1 || T < 2 || T > ET_MAX_T) return false;
    if (off && (n_scenes < 1 || N > INT32_MAX)) return false;
    if (N > 0 && (!gt || (reinterpret_cast<uintptr_t>(gt) & 7u))) return false;
    return ceil_div(N, kMtThreads) <= INT32_MAX;
}

}  // namespace et

using namespace et;

extern "C" int et_traj_metrics(const float *pred, int64_t N, int S, int T, const float *gt, const int32_t *scene_offsets,
                               int n_scenes, float *ade, float *fde, float *tcc, float *col, int32_t *best,
                               et_stream_t stream) {
    if (!common_args_ok(N, S, T, gt, scene_offsets, n_scenes)) return ET_ERR_INVALID_ARG;
    if (N > 0 && (!pred || (reinterpret_cast<uintptr_t>(pred) & 7u))) return ET_ERR_INVALID_ARG;
    if (N == 0 || !(ade || fde || tcc || col || best)) return ET_OK;
    const TensorSrc src{pred, N, T};
    return launch(src, N, S, T, gt, scene_offsets, n_scenes, ade, fde, tcc, col, best, stream);
}

extern "C" int et_anchor_reconstruct_metrics_scenes(const float *C, int64_t N, int S, int k, int T_obs, int T_pred,
                                                    const float *obs, const float *nrm, const float *pose,
                                                    const float *A_m, const float *A_s, const float *U_pred_m,
                                                    const float *U_pred_s, int mode, float static_dist, const float *gt,
                                                    const int32_t *scene_offsets, int n_scenes, float *ade, float *fde,
                                                    float *tcc, float *col, int32_t *best, et_stream_t stream) {
    if (!common_args_ok(N, S, T_pred, gt, scene_offsets, n_scenes)) return ET_ERR_INVALID_ARG;
    if (k < 1 || k > ET_MAX_K || mode < 0 || mode > 3) return ET_ERR_INVALID_ARG;
    if (obs && (T_obs < 3 || T_obs > ET_MAX_T)) return ET_ERR_INVALID_ARG;
    if (N == 0 || !(ade || fde || tcc || col || best)) return ET_OK;
    if (!C || (mode != ET_MODE_IDENTITY && !obs && !nrm && !pose)) return ET_ERR_INVALID_ARG;
    const bool need_m = mode == ET_MODE_MOVING || mode == ET_MODE_SPLIT, need_s = mode != ET_MODE_MOVING;
    if ((need_m && !U_pred_m) || (need_s && !U_pred_s)) return ET_ERR_INVALID_ARG;
    if (k <= 8) {
        const CoefSrc<8> src{C, N, S, k, T_obs, obs, nrm, pose, A_m, A_s, U_pred_m, U_pred_s, mode, static_dist};
        return launch(src, N, S, T_pred, gt, scene_offsets, n_scenes, ade, fde, tcc, col, best, stream);
    }
    const CoefSrc<0> src{C, N, S, k, T_obs, obs, nrm, pose, A_m, A_s, U_pred_m, U_pred_s, mode, static_dist};
    return launch(src, N, S, T_pred, gt, scene_offsets, n_scenes, ade, fde, tcc, col, best, stream);
}

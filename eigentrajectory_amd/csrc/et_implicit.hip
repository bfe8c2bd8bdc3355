// et_implicit.hip -- Social-Implicit inference (baseline/implicit: bridge.py pre-hook, model.py SocialImplicitLight.forward,
// bridge.py post-hook) for the ET configuration family (include/eigentraj.h "Social-Implicit predictor").
//
// The network sorts a scene's pedestrians into Social-Zones by |first coefficient| and runs each zone's own cell on the
// zone's pedestrians COMPACTED in scene order, so every convolution over the pedestrian axis sees the neighbours in the
// compacted list.  The receptive field of one output column is its compacted neighbours -2 .. +2, so nothing is compacted
// here.  Two launches, whatever the number of scenes:
//   implicit_prep_kernel  one workgroup per scene: the scene's v = [C_obs; obs_ori] (scene form), and per pedestrian a
//                         row of kImTab int32: its zone, the rows of its two predecessors and two successors of the same
//                         zone within the scene (-1: none), the scene's first row and size; the eighth entry is 0, or in
//                         a skipped scene the zone the pedestrian would have had (the backward pass reads it)
//   implicit_main_kernel  tiles of pedestrians, each pedestrian on its own from its five gathered columns of v:
//                         u = relu(feat(v)) + highway_input(v) at the compacted positions -1, 0, +1 (S, T each), the local
//                         stream's (S, T) plane, then the S x T_out outputs.  The zero padding of tpcnn pads u: u of a
//                         missing neighbour is 0, not feat of a zero column.
// All cells' weights are staged in LDS when they fit next to one pedestrian's planes (ET: 4 cells, 4.2k floats); otherwise
// they are read where they are.  Every output is one chain of fmaf in a fixed order over its own pedestrian's planes: it
// does not depend on the tile, on the launch size or on where the scene lies in the split.
// The noise term of SocialCellGlobal is noise_w * noise_weights[i] * 0 in the Light form and is left out.  For a finite
// noise_w it is a zero: adding it could only turn a -0.0 of v into +0.0, i.e. change the sign of a zero product.  A
// non-finite noise_w (NaN everywhere in the reference) is not reproduced.
// Training: the forward above is the training-mode forward too; its backward pass (two launches more, the gradients of every
// cell's tensors) is the second half of this file, "backward".
#include "et_common.h"

namespace et {
namespace {

#include "et_scene_helpers.inl"  // scene_v: a scene's input, obs_ori summed in et_scene_project's order

constexpr int kImThreads = kSnThreads;
constexpr int kImLdsBytes = 60 * 1024;  // dynamic LDS of one workgroup
constexpr int kImMaxS = 64;
constexpr int kImMaxT = 16;
constexpr int kImMaxBins = ET_IMPLICIT_MAX_BINS;
constexpr int kImMaxTile = 8;    // pedestrians of one tile
constexpr int kImMaxGrid = 1024;  // workgroups of the main kernel (they stride over the tiles)
constexpr int kImTab = 8;  // int32 per pedestrian: zone, rows of the neighbours -2, -1, +1, +2, scene begin, scene size, 0
                           // (of a skipped scene: the zone it would have had)
constexpr int kImSkipped = -2;  // zone of a pedestrian whose scene is larger than ET_SCENE_MAX_N (-1: in no zone)

// float offsets of one cell's tensors in the LDS copy (field order of et_implicit_cell)
struct ImLayout {
    int g[8], l[8], gw, lw, size;
};

__host__ __device__ inline ImLayout im_layout(int S, int T, int To) {
    const int gs[8] = {9 * S, S, S, S, To * T, To, 9 * To * T, To};
    const int ls[8] = {3 * S, S, S, S, To * T, To, 3 * To * T, To};
    ImLayout L;
    int at = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        L.g[i] = at;
        at += gs[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        L.l[i] = at;
        at += ls[i];
    }
    L.gw = at++;
    L.lw = at++;
    L.size = at;
    return L;
}

__host__ __device__ inline int im_floats_per_ped(int S, int T) { return 5 * T + 4 * T * S + kImTab; }

struct ImPlan {
    bool weights_in_lds;
    int tile, lds_bytes;
};

inline ImPlan im_plan(const et_implicit_params &p) {
    const int S = p.spatial_output, T = p.temporal_input;
    const int per = im_floats_per_ped(S, T);
    const int wf = p.n_bins * im_layout(S, T, p.temporal_output).size;
    ImPlan pl;
    pl.weights_in_lds = (wf + per) * 4 <= kImLdsBytes;
    const int left = kImLdsBytes / 4 - (pl.weights_in_lds ? wf : 0);
    pl.tile = left / per < kImMaxTile ? left / per : kImMaxTile;
    pl.lds_bytes = ((pl.weights_in_lds ? wf : 0) + pl.tile * per) * 4;
    return pl;
}

// bucketize(|first|, bins, right=True) - 1: the bins that are not greater than the norm, minus one (a NaN norm is greater
// than no bin and lands in the last zone, as the reference's upper-bound search leaves it); -1 below bins[0]
__device__ __forceinline__ int zone_of(float first, const et_implicit_params &p) {
    const float norm = fabsf(first);
    int cnt = 0;
#pragma unroll
    for (int b = 0; b < kImMaxBins; ++b) cnt += (b < p.n_bins && !(p.bins[b] > norm)) ? 1 : 0;
    return cnt - 1;
}

// gv: one scene as the bridge built it, (T,N); else C_obs (T-2,N), nrm (4,N) and the scene's v written to vbuf at b T
__global__ __launch_bounds__(kImThreads) void implicit_prep_kernel(et_implicit_params p, const float *__restrict__ gv,
                                                                   const float *__restrict__ C_obs,
                                                                   const float *__restrict__ nrm,
                                                                   const int32_t *__restrict__ off, int64_t N, float *vbuf,
                                                                   float *gin, int32_t *tab, int32_t *zone_out) {
    __shared__ float red[2 * kImThreads / kWave];
    const int64_t b = off ? off[blockIdx.x] : 0;
    const int64_t e = off ? off[blockIdx.x + 1] : N;
    if (e <= b) return;
    const int n = (int)(e - b);
    const int T = p.temporal_input;
    const int tid = threadIdx.x;
    if (n > ET_SCENE_MAX_N) {  // not computed (the neighbour scan is O(n) per pedestrian): zone kImSkipped, NaN rows
        for (int w = tid; w < n; w += kImThreads) {
            int32_t *t = tab + (b + w) * kImTab;
            t[0] = kImSkipped;
            for (int i = 1; i < kImTab - 1; ++i) t[i] = i < 5 ? -1 : 0;
            t[7] = zone_of(gv ? gv[w] : C_obs[b + w], p);  // read by the backward pass alone: the cell whose gradients it makes NaN
            if (zone_out) zone_out[b + w] = kImSkipped;
        }
        if (gin)
            for (int i = tid; i < T * n; i += kImThreads) gin[(int64_t)(i / n) * N + b + (i % n)] = __builtin_nanf("");
        return;
    }
    const float *row0 = gv ? gv : C_obs + b;  // the first coefficients of the scene
    if (!gv) {
        float *vb = vbuf + b * T;
        scene_v(vb, nullptr, C_obs, nrm, N, b, n, T, red);
        if (gin) {
            __syncthreads();
            for (int i = tid; i < T * n; i += kImThreads) gin[(int64_t)(i / n) * N + b + (i % n)] = vb[i];
        }
    }
    // the zones once, into the table; then every pedestrian looks for its neighbours among them
    for (int w = tid; w < n; w += kImThreads) {
        const int z = zone_of(row0[w], p);
        tab[(b + w) * kImTab] = z;
        if (zone_out) zone_out[b + w] = z;
    }
    __syncthreads();
    const int32_t *zs = tab + b * kImTab;  // zone of the scene's pedestrian j: zs[j kImTab]
    for (int w = tid; w < n; w += kImThreads) {
        const int z = zs[(int64_t)w * kImTab];
        int p1 = -1, p2 = -1, s1 = -1, s2 = -1;
        if (z >= 0) {
            for (int j = w - 1; j >= 0 && p2 < 0; --j)
                if (zs[(int64_t)j * kImTab] == z) {
                    if (p1 < 0) p1 = j; else p2 = j;
                }
            for (int j = w + 1; j < n && s2 < 0; ++j)
                if (zs[(int64_t)j * kImTab] == z) {
                    if (s1 < 0) s1 = j; else s2 = j;
                }
        }
        int32_t *t = tab + (b + w) * kImTab;
        t[1] = p2 < 0 ? -1 : (int32_t)(b + p2);
        t[2] = p1 < 0 ? -1 : (int32_t)(b + p1);
        t[3] = s1 < 0 ? -1 : (int32_t)(b + s1);
        t[4] = s2 < 0 ? -1 : (int32_t)(b + s2);
        t[5] = (int32_t)b;
        t[6] = n;
        t[7] = 0;
    }
}

// one cell's tensors, in LDS or where the module keeps them
struct ImCell {
    const float *gfw, *gfb, *ghiw, *ghib, *ghw, *ghb, *gtw, *gtb;
    const float *lfw, *lfb, *lhiw, *lhib, *lhw, *lhb, *ltw, *ltb;
    const float *gw, *lw;
};

template <bool kLds>
__device__ __forceinline__ ImCell im_cell(const et_implicit_params &p, const ImLayout &L, const float *wl, int z) {
    ImCell c;
    if (kLds) {
        const float *w = wl + z * L.size;
        c.gfw = w + L.g[0], c.gfb = w + L.g[1], c.ghiw = w + L.g[2], c.ghib = w + L.g[3];
        c.ghw = w + L.g[4], c.ghb = w + L.g[5], c.gtw = w + L.g[6], c.gtb = w + L.g[7];
        c.lfw = w + L.l[0], c.lfb = w + L.l[1], c.lhiw = w + L.l[2], c.lhib = w + L.l[3];
        c.lhw = w + L.l[4], c.lhb = w + L.l[5], c.ltw = w + L.l[6], c.ltb = w + L.l[7];
        c.gw = w + L.gw, c.lw = w + L.lw;
    } else {
        const et_implicit_cell &q = p.cells[z];
        c.gfw = q.global_t[0], c.gfb = q.global_t[1], c.ghiw = q.global_t[2], c.ghib = q.global_t[3];
        c.ghw = q.global_t[4], c.ghb = q.global_t[5], c.gtw = q.global_t[6], c.gtb = q.global_t[7];
        c.lfw = q.local_t[0], c.lfb = q.local_t[1], c.lhiw = q.local_t[2], c.lhib = q.local_t[3];
        c.lhw = q.local_t[4], c.lhb = q.local_t[5], c.ltw = q.local_t[6], c.ltb = q.local_t[7];
        c.gw = q.global_w, c.lw = q.local_w;
    }
    return c;
}

__device__ __forceinline__ float relu(float x) { return x < 0.f ? 0.f : x; }  // a NaN stays a NaN, as in torch

// src: the scenes' v, scene s (T, n_s) at float b_s T (graph form: the given (T,N), b = 0).  kScenes: out (T_out,N,S), the
// post-hook's permute; else (1,S,T_out,N), the network's raw output.
template <bool kScenes, bool kLds>
__global__ __launch_bounds__(kImThreads) void implicit_main_kernel(et_implicit_params p, const float *__restrict__ src,
                                                                   const int32_t *__restrict__ tab, int64_t N,
                                                                   float *__restrict__ out, int tile) {
    extern __shared__ float lds[];
    const int S = p.spatial_output, T = p.temporal_input, To = p.temporal_output;
    const int tid = threadIdx.x;
    const ImLayout L = im_layout(S, T, To);
    float *wl = lds;
    float *vc = lds + (kLds ? p.n_bins * L.size : 0);  // (tile, 5, T): the columns of the neighbours -2 .. +2
    float *u = vc + tile * 5 * T;                      // (tile, 3, T, S): u at the compacted positions -1, 0, +1
    float *ul = u + tile * 3 * T * S;                  // (tile, T, S): the local stream's plane
    int *meta = (int *)(ul + tile * T * S);            // (tile, kImTab)

    if (kLds) {
        for (int z = 0; z < p.n_bins; ++z) {
            const et_implicit_cell &q = p.cells[z];
            float *w = wl + z * L.size;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int gn = (i < 7 ? L.g[i + 1] : L.l[0]) - L.g[i], ln = (i < 7 ? L.l[i + 1] : L.gw) - L.l[i];
                for (int j = tid; j < gn; j += kImThreads) w[L.g[i] + j] = q.global_t[i][j];
                for (int j = tid; j < ln; j += kImThreads) w[L.l[i] + j] = q.local_t[i][j];
            }
            if (tid == 0) {
                w[L.gw] = q.global_w[0];
                w[L.lw] = q.local_w[0];
            }
        }
    }
    for (int64_t t0 = (int64_t)blockIdx.x * tile; t0 < N; t0 += (int64_t)gridDim.x * tile) {
        const int np = (int)(N - t0 < tile ? N - t0 : tile);
        for (int i = tid; i < np * kImTab; i += kImThreads) meta[i] = tab[t0 * kImTab + i];
        __syncthreads();
        for (int it = tid; it < np * 5 * T; it += kImThreads) {
            const int t = it % T, c = (it / T) % 5, pp = it / (5 * T);
            const int *m = meta + pp * kImTab;
            const int64_t idx = c == 2 ? t0 + pp : m[c < 2 ? c + 1 : c];
            vc[it] = idx >= 0 && m[0] >= 0 ? src[(int64_t)m[5] * T + (int64_t)t * m[6] + (idx - m[5])] : 0.f;
        }
        __syncthreads();
        for (int it = tid; it < np * 3 * T * S; it += kImThreads) {
            const int s = it % S, t = (it / S) % T, q = (it / (S * T)) % 3, pp = it / (3 * S * T);
            const int *m = meta + pp * kImTab;
            float val = 0.f;
            if (m[0] >= 0 && (q == 1 || m[q == 0 ? 2 : 3] >= 0)) {  // the neighbour at position q - 1 is there
                const ImCell W = im_cell<kLds>(p, L, wl, m[0]);
                const float *col = vc + (pp * 5 + q) * T;  // the columns q - 2 .. q of this position: col[dj T + t]
                float acc = W.gfb[s];
                for (int dt = 0; dt < 3; ++dt) {
                    const int tt = t + dt - 1;
                    if (tt < 0 || tt >= T) continue;
                    for (int dj = 0; dj < 3; ++dj) acc = fmaf(W.gfw[s * 9 + dt * 3 + dj], col[dj * T + tt], acc);
                }
                val = relu(acc) + (W.ghiw[s] * col[T + t] + W.ghib[s]);
            }
            u[it] = val;
        }
        for (int it = tid; it < np * T * S; it += kImThreads) {
            const int s = it % S, t = (it / S) % T, pp = it / (S * T);
            const int *m = meta + pp * kImTab;
            float val = 0.f;
            if (m[0] >= 0) {
                const ImCell W = im_cell<kLds>(p, L, wl, m[0]);
                const float *col = vc + (pp * 5 + 2) * T;
                float acc = W.lfb[s];
                for (int dt = 0; dt < 3; ++dt) {
                    const int tt = t + dt - 1;
                    if (tt >= 0 && tt < T) acc = fmaf(W.lfw[s * 3 + dt], col[tt], acc);
                }
                val = relu(acc) + (W.lhiw[s] * col[t] + W.lhib[s]);
            }
            ul[it] = val;
        }
        __syncthreads();
        for (int it = tid; it < np * To * S; it += kImThreads) {
            const int s = it % S, o = (it / S) % To, pp = it / (S * To);
            const int *m = meta + pp * kImTab;
            float val = 0.f;
            if (m[0] >= 0) {
                const ImCell W = im_cell<kLds>(p, L, wl, m[0]);
                // global stream: tpcnn over the (S, zone) plane of u with T as channels, + the 1x1 highway
                const float *up = u + (int64_t)pp * 3 * T * S;
                float acc = W.gtb[o];
                for (int t = 0; t < T; ++t)
                    for (int ds = 0; ds < 3; ++ds) {
                        const int ss = s + ds - 1;
                        if (ss < 0 || ss >= S) continue;
                        const float *wk = W.gtw + ((o * T + t) * 3 + ds) * 3;
                        for (int dj = 0; dj < 3; ++dj) acc = fmaf(wk[dj], up[(dj * T + t) * S + ss], acc);
                    }
                float res = W.ghb[o];
                for (int t = 0; t < T; ++t) res = fmaf(W.ghw[o * T + t], up[(T + t) * S + s], res);
                const float g = acc + res;
                // local stream: its (T_out, S) block is READ AS (S, T_out) (model.py:40 reshapes, it does not transpose)
                const int f = s * To + o;
                const int lo = f / S, ls = f - lo * S;
                const float *lp = ul + (int64_t)pp * T * S;
                float accl = W.ltb[lo];
                for (int t = 0; t < T; ++t)
                    for (int ds = 0; ds < 3; ++ds) {
                        const int ss = ls + ds - 1;
                        if (ss >= 0 && ss < S) accl = fmaf(W.ltw[(lo * T + t) * 3 + ds], lp[t * S + ss], accl);
                    }
                float resl = W.lhb[lo];
                for (int t = 0; t < T; ++t) resl = fmaf(W.lhw[lo * T + t], lp[t * S + ls], resl);
                const float l = accl + resl;
                val = W.gw[0] * g + W.lw[0] * l;
            } else if (m[0] == kImSkipped) {
                val = __builtin_nanf("");
            }
            const int64_t j = t0 + pp;
            if (kScenes) out[((int64_t)o * N + j) * S + s] = val;
            else out[((int64_t)s * To + o) * N + j] = val;
        }
        __syncthreads();
    }
}

static int im_check_params(const et_implicit_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->spatial_input != 1 || p->spatial_output < 1 || p->spatial_output > kImMaxS || p->temporal_input < 1 ||
        p->temporal_input > kImMaxT || p->temporal_output < 1 || p->temporal_output > kImMaxT || p->n_bins < 1 ||
        p->n_bins > kImMaxBins)
        return ET_ERR_UNSUPPORTED;
    if (!(p->bins[0] == p->bins[0])) return ET_ERR_UNSUPPORTED;
    for (int b = 0; b + 1 < p->n_bins; ++b)  // ascending, as bucketize takes them (a NaN fails the comparison)
        if (!(p->bins[b] <= p->bins[b + 1])) return ET_ERR_UNSUPPORTED;
    for (int z = 0; z < p->n_bins; ++z) {
        const et_implicit_cell &c = p->cells[z];
        for (int i = 0; i < 8; ++i)
            if (!c.global_t[i] || !c.local_t[i]) return ET_ERR_INVALID_ARG;
        if (!c.noise_w || !c.global_w || !c.local_w) return ET_ERR_INVALID_ARG;
    }
    return ET_OK;
}

static size_t im_tab_bytes(int64_t N) { return (size_t)N * kImTab * sizeof(int32_t); }

template <bool kScenes>
static int im_launch_main(const et_implicit_params &p, const float *src, const int32_t *tab, int64_t N, float *out,
                          hipStream_t stream) {
    const ImPlan pl = im_plan(p);
    const int64_t tiles = ceil_div(N, pl.tile);
    const unsigned grid = (unsigned)(tiles < kImMaxGrid ? tiles : kImMaxGrid);
    if (pl.weights_in_lds)
        hipLaunchKernelGGL((implicit_main_kernel<kScenes, true>), dim3(grid), dim3(kImThreads), (unsigned)pl.lds_bytes, stream,
                           p, src, tab, N, out, pl.tile);
    else
        hipLaunchKernelGGL((implicit_main_kernel<kScenes, false>), dim3(grid), dim3(kImThreads), (unsigned)pl.lds_bytes,
                           stream, p, src, tab, N, out, pl.tile);
    ET_LAUNCH_CHECK();
    return ET_OK;
}


// ---------------------------------------------------------------------------------------------------------- backward
// The gradients of the 18 tensors of every cell that the forward reads (noise_w has none to compute: its term is a product
// with the zero noise), one block of im_layout().size floats per cell in et_implicit_cell's field order.  A pedestrian's
// output depends on its own five gathered columns alone, so its contribution to every weight gradient is formed on its
// own, from those columns and its (S, T_out) block G of the upstream gradient; nothing of the forward is kept but the
// neighbour table.  Two launches whatever N:
//   implicit_bwd_kernel      one workgroup per (chunk of kImChunk rows, cell).  The chunk's pedestrians of that cell, one
//                            after the other in row order: u, ul, g, l again with the forward's own statements; du, dul
//                            from dg = global_w G and dl = local_w G (G read by flat index, the inverse of the local
//                            stream's reshape); dpre = du where pre > 0 (a NaN pre passes, as torch's relu backward does),
//                            +0 elsewhere.  Then every gradient element, owned by one thread, CONTINUES its accumulator:
//                            one fmaf (or addition) per term, ascending over the element's inner index (the position q,
//                            then t; or s; or the flat index of G for the two scalars).
//   implicit_bwd_sum_kernel  grad = the chunks' partial blocks added in ascending chunk order.
// So the summation order of an element is: rows ascending inside chunks of kImChunk rows from a +0 accumulator, then the
// chunks ascending; it depends on N through the number of chunks only.  No atomics.  Terms that the forward's zero padding
// of u contributes (a missing neighbour: u = 0) are formed (0 x NaN is a NaN); a missing neighbour carries no gradient to
// feat / highway_input; taps beyond the T and S edges are not terms, as in the forward.
constexpr int kImChunk = ET_IMPLICIT_BWD_CHUNK;
constexpr int kImBwdLdsBytes = 64 * 1024;

__host__ __device__ inline int im_bwd_floats_per_ped(int S, int T, int To) { return 5 * T + 3 * S * To + 12 * T * S; }

struct ImBwdPlan {
    bool lds;  // the cell's weights and its gradient block in LDS next to the planes
    int lds_bytes;
};

inline ImBwdPlan im_bwd_plan(const et_implicit_params &p) {
    const int per = im_bwd_floats_per_ped(p.spatial_output, p.temporal_input, p.temporal_output);
    const int wf = 2 * im_layout(p.spatial_output, p.temporal_input, p.temporal_output).size;
    ImBwdPlan pl;
    pl.lds = (per + wf) * 4 <= kImBwdLdsBytes - 64;
    pl.lds_bytes = (per + (pl.lds ? wf : 0)) * 4;
    return pl;
}

// src, tab as implicit_main_kernel's; gout: kTns (T_out,N,S), else (1,S,T_out,N); part (chunks, n_bins, L.size)
template <bool kTns, bool kLds>
__global__ __launch_bounds__(kImThreads) void implicit_bwd_kernel(et_implicit_params p, const float *__restrict__ src,
                                                                  const int32_t *__restrict__ tab, int64_t N,
                                                                  const float *__restrict__ gout, float *part) {
    extern __shared__ float lds[];
    const int S = p.spatial_output, T = p.temporal_input, To = p.temporal_output;
    const int tid = threadIdx.x, z = blockIdx.y;
    const ImLayout L = im_layout(S, T, To);
    const int TS = T * S, F = S * To;
    float *vc = lds;         // (5, T): the columns of the neighbours -2 .. +2
    float *G = vc + 5 * T;   // (S, T_out), flat f = s T_out + o: the upstream gradient of this pedestrian
    float *u = G + F;        // (3, T, S): u at the compacted positions -1, 0, +1
    float *du = u + 3 * TS;  // its gradient through this pedestrian's outputs
    float *dp = du + 3 * TS;  // du where feat's pre-activation passes the ReLU
    float *ul = dp + 3 * TS;  // (T, S): the local stream's plane, its gradient, the gradient behind the ReLU
    float *dul = ul + TS;
    float *dpl = dul + TS;
    float *gg = dpl + TS;  // (S, T_out) flat: g and l, for the two scalars' gradients
    float *ll = gg + F;
    float *wl = ll + F;  // kLds: the cell's weights, then its gradient block
    float *blk = part + ((int64_t)blockIdx.x * p.n_bins + z) * L.size;
    float *acc = kLds ? wl + L.size : blk;

    // the chunk's rows first (the same for all threads): a workgroup none of whose rows is in cell z -- most of them, with
    // 4 to 8 cells and 8 rows -- writes its block and is done, without staging the weights
    const int64_t r0 = (int64_t)blockIdx.x * kImChunk;
    const int rows = (int)(N - r0 < kImChunk ? N - r0 : kImChunk);
    bool poison = false, any = false;
    for (int r = 0; r < rows; ++r) {
        const int32_t *m = tab + (r0 + r) * kImTab;
        poison = poison || (m[0] == kImSkipped && m[7] == z);
        any = any || m[0] == z;
    }
    if (!any || poison) {
        for (int e = tid; e < L.size; e += kImThreads) blk[e] = poison ? __builtin_nanf("") : 0.f;
        return;
    }
    for (int e = tid; e < L.size; e += kImThreads) acc[e] = 0.f;
    if (kLds) {
        const et_implicit_cell &q = p.cells[z];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gn = (i < 7 ? L.g[i + 1] : L.l[0]) - L.g[i], ln = (i < 7 ? L.l[i + 1] : L.gw) - L.l[i];
            for (int j = tid; j < gn; j += kImThreads) wl[L.g[i] + j] = q.global_t[i][j];
            for (int j = tid; j < ln; j += kImThreads) wl[L.l[i] + j] = q.local_t[i][j];
        }
        if (tid == 0) {
            wl[L.gw] = q.global_w[0];
            wl[L.lw] = q.local_w[0];
        }
    }
    __syncthreads();
    const ImCell W = im_cell<kLds>(p, L, wl, kLds ? 0 : z);
    const float gwv = W.gw[0], lwv = W.lw[0];
    for (int r = 0; r < rows; ++r) {  // every decision below is the same for all threads
        const int64_t j = r0 + r;
        const int32_t *m = tab + j * kImTab;
        if (m[0] != z) continue;
        const int64_t b = m[5];
        const int n = m[6];
        const int has = (m[2] >= 0 ? 1 : 0) | 2 | (m[3] >= 0 ? 4 : 0);  // bit q: the neighbour at position q - 1 is there
        for (int it = tid; it < 5 * T; it += kImThreads) {
            const int t = it % T, c = it / T;
            const int64_t idx = c == 2 ? j : m[c < 2 ? c + 1 : c];
            vc[it] = idx >= 0 ? src[b * T + (int64_t)t * n + (idx - b)] : 0.f;
        }
        for (int f = tid; f < F; f += kImThreads) {
            const int s = f / To, o = f - s * To;
            G[f] = kTns ? gout[((int64_t)o * N + j) * S + s] : gout[(int64_t)f * N + j];
        }
        __syncthreads();
        for (int it = tid; it < 3 * TS; it += kImThreads) {
            const int s = it % S, t = (it / S) % T, q = it / TS;
            float val = 0.f, d = 0.f, dpre = 0.f;
            if ((has >> q) & 1) {
                const float *col = vc + q * T;
                float a = W.gfb[s];
                for (int dt = 0; dt < 3; ++dt) {
                    const int tt = t + dt - 1;
                    if (tt < 0 || tt >= T) continue;
                    for (int dj = 0; dj < 3; ++dj) a = fmaf(W.gfw[s * 9 + dt * 3 + dj], col[dj * T + tt], a);
                }
                val = relu(a) + (W.ghiw[s] * col[T + t] + W.ghib[s]);
                for (int o = 0; o < To; ++o)
                    for (int ds = 0; ds < 3; ++ds) {
                        const int sp = s - ds + 1;  // the output row that read u[t, s] through tap ds
                        if (sp < 0 || sp >= S) continue;
                        d = fmaf(W.gtw[((o * T + t) * 3 + ds) * 3 + q], gwv * G[sp * To + o], d);
                    }
                if (q == 1)
                    for (int o = 0; o < To; ++o) d = fmaf(W.ghw[o * T + t], gwv * G[s * To + o], d);
                dpre = a <= 0.f ? 0.f : d;
            }
            u[it] = val;
            du[it] = d;
            dp[it] = dpre;
        }
        for (int it = tid; it < TS; it += kImThreads) {
            const int s = it % S, t = it / S;
            const float *col = vc + 2 * T;
            float a = W.lfb[s];
            for (int dt = 0; dt < 3; ++dt) {
                const int tt = t + dt - 1;
                if (tt >= 0 && tt < T) a = fmaf(W.lfw[s * 3 + dt], col[tt], a);
            }
            float d = 0.f;
            for (int lo = 0; lo < To; ++lo)
                for (int ds = 0; ds < 3; ++ds) {
                    const int sp = s - ds + 1;
                    if (sp >= 0 && sp < S) d = fmaf(W.ltw[(lo * T + t) * 3 + ds], lwv * G[lo * S + sp], d);
                }
            for (int lo = 0; lo < To; ++lo) d = fmaf(W.lhw[lo * T + t], lwv * G[lo * S + s], d);
            ul[it] = relu(a) + (W.lhiw[s] * col[t] + W.lhib[s]);
            dul[it] = d;
            dpl[it] = a <= 0.f ? 0.f : d;
        }
        __syncthreads();
        for (int it = tid; it < F; it += kImThreads) {  // g and l: implicit_main_kernel's statements
            const int s = it % S, o = it / S;
            float a = W.gtb[o];
            for (int t = 0; t < T; ++t)
                for (int ds = 0; ds < 3; ++ds) {
                    const int ss = s + ds - 1;
                    if (ss < 0 || ss >= S) continue;
                    const float *wk = W.gtw + ((o * T + t) * 3 + ds) * 3;
                    for (int dj = 0; dj < 3; ++dj) a = fmaf(wk[dj], u[(dj * T + t) * S + ss], a);
                }
            float res = W.ghb[o];
            for (int t = 0; t < T; ++t) res = fmaf(W.ghw[o * T + t], u[(T + t) * S + s], res);
            const int f = s * To + o;
            const int lo = f / S, ls = f - lo * S;
            float al = W.ltb[lo];
            for (int t = 0; t < T; ++t)
                for (int ds = 0; ds < 3; ++ds) {
                    const int ss = ls + ds - 1;
                    if (ss >= 0 && ss < S) al = fmaf(W.ltw[(lo * T + t) * 3 + ds], ul[t * S + ss], al);
                }
            float resl = W.lhb[lo];
            for (int t = 0; t < T; ++t) resl = fmaf(W.lhw[lo * T + t], ul[t * S + ls], resl);
            gg[f] = a + res;
            ll[f] = al + resl;
        }
        __syncthreads();
        for (int e = tid; e < L.size; e += kImThreads) {
            float a = acc[e];
            if (e < L.l[0]) {
                if (e < L.g[1]) {  // feat.weight (s, dt, dj)
                    const int s = e / 9, dt = (e / 3) % 3, dj = e % 3;
                    for (int q = 0; q < 3; ++q) {
                        if (!((has >> q) & 1)) continue;
                        for (int t = 0; t < T; ++t) {
                            const int tt = t + dt - 1;
                            if (tt >= 0 && tt < T) a = fmaf(dp[(q * T + t) * S + s], vc[(q + dj) * T + tt], a);
                        }
                    }
                } else if (e < L.g[4]) {  // feat.bias, highway_input.weight, highway_input.bias (s)
                    const int k = e < L.g[2] ? 1 : e < L.g[3] ? 2 : 3, s = e - L.g[k];
                    for (int q = 0; q < 3; ++q) {
                        if (!((has >> q) & 1)) continue;
                        for (int t = 0; t < T; ++t) {
                            const int i = (q * T + t) * S + s;
                            a = k == 1 ? a + dp[i] : k == 2 ? fmaf(du[i], vc[(q + 1) * T + t], a) : a + du[i];
                        }
                    }
                } else if (e < L.g[5]) {  // highway.weight (o, t)
                    const int i = e - L.g[4], o = i / T, t = i - o * T;
                    for (int s = 0; s < S; ++s) a = fmaf(gwv * G[s * To + o], u[(T + t) * S + s], a);
                } else if (e < L.g[6] || e >= L.g[7]) {  // highway.bias, tpcnn.bias (o)
                    const int o = e - (e < L.g[6] ? L.g[5] : L.g[7]);
                    for (int s = 0; s < S; ++s) a += gwv * G[s * To + o];
                } else {  // tpcnn.weight (o, t, ds, dj)
                    const int i = e - L.g[6], dj = i % 3, ds = (i / 3) % 3, t = (i / 9) % T, o = i / (9 * T);
                    for (int s = 0; s < S; ++s) {
                        const int ss = s + ds - 1;
                        if (ss >= 0 && ss < S) a = fmaf(gwv * G[s * To + o], u[(dj * T + t) * S + ss], a);
                    }
                }
            } else if (e < L.gw) {
                if (e < L.l[1]) {  // ped.feat.weight (s, dt)
                    const int i = e - L.l[0], s = i / 3, dt = i - s * 3;
                    for (int t = 0; t < T; ++t) {
                        const int tt = t + dt - 1;
                        if (tt >= 0 && tt < T) a = fmaf(dpl[t * S + s], vc[2 * T + tt], a);
                    }
                } else if (e < L.l[4]) {  // ped.feat.bias, ped.highway_input.weight, ped.highway_input.bias (s)
                    const int k = e < L.l[2] ? 1 : e < L.l[3] ? 2 : 3, s = e - L.l[k];
                    for (int t = 0; t < T; ++t) {
                        const int i = t * S + s;
                        a = k == 1 ? a + dpl[i] : k == 2 ? fmaf(dul[i], vc[2 * T + t], a) : a + dul[i];
                    }
                } else if (e < L.l[5]) {  // ped.highway.weight (lo, t)
                    const int i = e - L.l[4], lo = i / T, t = i - lo * T;
                    for (int ls = 0; ls < S; ++ls) a = fmaf(lwv * G[lo * S + ls], ul[t * S + ls], a);
                } else if (e < L.l[6] || e >= L.l[7]) {  // ped.highway.bias, ped.tpcnn.bias (lo)
                    const int lo = e - (e < L.l[6] ? L.l[5] : L.l[7]);
                    for (int ls = 0; ls < S; ++ls) a += lwv * G[lo * S + ls];
                } else {  // ped.tpcnn.weight (lo, t, ds)
                    const int i = e - L.l[6], ds = i % 3, t = (i / 3) % T, lo = i / (3 * T);
                    for (int ls = 0; ls < S; ++ls) {
                        const int ss = ls + ds - 1;
                        if (ss >= 0 && ss < S) a = fmaf(lwv * G[lo * S + ls], ul[t * S + ss], a);
                    }
                }
            } else {  // global_w, local_w
                const float *y = e == L.gw ? gg : ll;
                for (int f = 0; f < F; ++f) a = fmaf(G[f], y[f], a);
            }
            acc[e] = a;
        }
        __syncthreads();
    }
    if (kLds)
        for (int e = tid; e < L.size; e += kImThreads) blk[e] = acc[e];
}

// grad (total) = the chunks' blocks part (chunks, total), added in ascending chunk order
__global__ __launch_bounds__(kImThreads) void implicit_bwd_sum_kernel(const float *__restrict__ part, int64_t chunks,
                                                                      int total, float *__restrict__ grad) {
    const int i = blockIdx.x * kImThreads + threadIdx.x;
    if (i >= total) return;
    float a = part[i];
    for (int64_t c = 1; c < chunks; ++c) a += part[c * total + i];
    grad[i] = a;
}

static size_t im_bwd_part_bytes(const et_implicit_params &p, int64_t N) {
    return (size_t)ceil_div(N, kImChunk) * p.n_bins * im_layout(p.spatial_output, p.temporal_input, p.temporal_output).size *
           sizeof(float);
}

template <bool kTns>
static int im_launch_bwd(const et_implicit_params &p, const float *src, const int32_t *tab, int64_t N, const float *gout,
                         float *grads, float *part, hipStream_t stream) {
    const ImBwdPlan pl = im_bwd_plan(p);
    const int64_t chunks = ceil_div(N, kImChunk);
    const int total = p.n_bins * im_layout(p.spatial_output, p.temporal_input, p.temporal_output).size;
    const dim3 grid((unsigned)chunks, (unsigned)p.n_bins);
    if (pl.lds)
        hipLaunchKernelGGL((implicit_bwd_kernel<kTns, true>), grid, dim3(kImThreads), (unsigned)pl.lds_bytes, stream, p, src,
                           tab, N, gout, part);
    else
        hipLaunchKernelGGL((implicit_bwd_kernel<kTns, false>), grid, dim3(kImThreads), (unsigned)pl.lds_bytes, stream, p,
                           src, tab, N, gout, part);
    ET_LAUNCH_CHECK();
    hipLaunchKernelGGL(implicit_bwd_sum_kernel, dim3((unsigned)ceil_div(total, kImThreads)), dim3(kImThreads), 0, stream, part,
                       chunks, total, grads);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

static int im_zero_grads(const et_implicit_params &p, float *grads, hipStream_t stream) {
    const size_t bytes =
        (size_t)p.n_bins * im_layout(p.spatial_output, p.temporal_input, p.temporal_output).size * sizeof(float);
    return hipMemsetAsync(grads, 0, bytes, stream) == hipSuccess ? ET_OK : ET_ERR_HIP;
}

}  // namespace
}  // namespace et

using namespace et;

extern "C" size_t et_implicit_workspace_bytes(const et_implicit_params *params, int64_t N) {
    if (im_check_params(params) != ET_OK || N <= 0 || N > INT32_MAX / kImMaxT) return 0;
    return im_tab_bytes(N) + (size_t)N * params->temporal_input * sizeof(float);
}

extern "C" int et_implicit_forward_graph(const et_implicit_params *params, const float *v, int64_t N, float *out,
                                         void *workspace, size_t workspace_bytes, et_stream_t stream) {
    const int rc = im_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SCENE_MAX_N) return ET_ERR_INVALID_ARG;
    if (N == 0) return ET_OK;
    if (!v || !out) return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < im_tab_bytes(N)) return ET_ERR_WORKSPACE;
    int32_t *tab = (int32_t *)workspace;
    hipLaunchKernelGGL(implicit_prep_kernel, dim3(1), dim3(kImThreads), 0, (hipStream_t)stream, *params, v, nullptr, nullptr,
                       nullptr, N, nullptr, nullptr, tab, nullptr);
    ET_LAUNCH_CHECK();
    return im_launch_main<false>(*params, v, tab, N, out, (hipStream_t)stream);
}

extern "C" int et_implicit_forward_scenes(const et_implicit_params *params, const float *C_obs, const float *nrm, int64_t N,
                                          const int32_t *scene_offsets, int n_scenes, float *C_pred_refine,
                                          float *graph_inputs, int32_t *zone, void *workspace, size_t workspace_bytes,
                                          et_stream_t stream) {
    const int rc = im_check_params(params);
    if (rc != ET_OK) return rc;
    if (params->temporal_input < 3) return ET_ERR_UNSUPPORTED;  // v = [C_obs; obs_ori]: one coefficient row at least
    const int early = scene_args_status(N, INT32_MAX / kImMaxT, scene_offsets, n_scenes, ET_SCENE_MAX_N);
    if (early != kSceneArgsGo) return early;
    if (!C_obs || !nrm || !C_pred_refine) return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_implicit_workspace_bytes(params, N)) return ET_ERR_WORKSPACE;
    int32_t *tab = (int32_t *)workspace;
    float *vbuf = (float *)((char *)workspace + im_tab_bytes(N));
    const unsigned grid = scene_offsets ? (unsigned)n_scenes : 1u;
    hipLaunchKernelGGL(implicit_prep_kernel, dim3(grid), dim3(kImThreads), 0, (hipStream_t)stream, *params, nullptr, C_obs,
                       nrm, scene_offsets, N, vbuf, graph_inputs, tab, zone);
    ET_LAUNCH_CHECK();
    return im_launch_main<true>(*params, vbuf, tab, N, C_pred_refine, (hipStream_t)stream);
}

extern "C" size_t et_implicit_backward_workspace_bytes(const et_implicit_params *params, int64_t N) {
    if (im_check_params(params) != ET_OK || N <= 0 || N > INT32_MAX / kImMaxT) return 0;
    return im_bwd_part_bytes(*params, N);
}

extern "C" int et_implicit_backward_graph(const et_implicit_params *params, const float *v, int64_t N,
                                          const void *forward_workspace, size_t forward_workspace_bytes, const float *g_out,
                                          int g_layout, float *grads, void *workspace, size_t workspace_bytes,
                                          et_stream_t stream) {
    const int rc = im_check_params(params);
    if (rc != ET_OK) return rc;
    if (N < 0 || N > ET_SCENE_MAX_N || !grads || (g_layout != ET_IMPLICIT_G_STN && g_layout != ET_IMPLICIT_G_TNS))
        return ET_ERR_INVALID_ARG;
    if (N == 0) return im_zero_grads(*params, grads, (hipStream_t)stream);
    if (!v || !g_out) return ET_ERR_INVALID_ARG;
    if (!forward_workspace || forward_workspace_bytes < im_tab_bytes(N) || !workspace ||
        workspace_bytes < im_bwd_part_bytes(*params, N))
        return ET_ERR_WORKSPACE;
    const int32_t *tab = (const int32_t *)forward_workspace;
    return g_layout == ET_IMPLICIT_G_TNS
               ? im_launch_bwd<true>(*params, v, tab, N, g_out, grads, (float *)workspace, (hipStream_t)stream)
               : im_launch_bwd<false>(*params, v, tab, N, g_out, grads, (float *)workspace, (hipStream_t)stream);
}

extern "C" int et_implicit_backward_scenes(const et_implicit_params *params, int64_t N, const void *forward_workspace,
                                           size_t forward_workspace_bytes, const float *g, float *grads, void *workspace,
                                           size_t workspace_bytes, et_stream_t stream) {
    const int rc = im_check_params(params);
    if (rc != ET_OK) return rc;
    if (params->temporal_input < 3) return ET_ERR_UNSUPPORTED;
    if (N < 0 || N > INT32_MAX / kImMaxT || !grads) return ET_ERR_INVALID_ARG;
    if (N == 0) return im_zero_grads(*params, grads, (hipStream_t)stream);
    if (!g) return ET_ERR_INVALID_ARG;
    if (!forward_workspace || forward_workspace_bytes < et_implicit_workspace_bytes(params, N) || !workspace ||
        workspace_bytes < im_bwd_part_bytes(*params, N))
        return ET_ERR_WORKSPACE;
    const float *vbuf = (const float *)((const char *)forward_workspace + im_tab_bytes(N));
    return im_launch_bwd<true>(*params, vbuf, (const int32_t *)forward_workspace, N, g, grads, (float *)workspace,
                               (hipStream_t)stream);
}

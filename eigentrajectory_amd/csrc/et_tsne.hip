// et_tsne.hip -- t-SNE of descriptor coefficients (reference: script/plot_coeff_tsne.py, which calls
// sklearn.manifold.TSNE(n_components=2, random_state=42): Barnes-Hut, perplexity 30, 1 000 iterations).  This is that
// pipeline with one change: the repulsive term is summed exactly over all pairs instead of through a quadtree.
//
//   affinities  knn_kernel            k nearest other rows by (squared distance, index); one lane per query row,
//                                     candidate tiles through LDS, the lane's sorted list in the workspace
//               perplexity_kernel     sklearn's binary search for beta per row (fp64, 100 steps)
//               indeg / scan / scatter / rev_sort / merge_count / scan / merge_fill / total / normalize
//                                     P = P_cond + P_cond^T as canonical CSR (sorted columns, zero sums dropped),
//                                     divided by its total
//   gradient    rep_kernel            grid (row block x column chunk of kChunk columns): per row and chunk the fp32 sums
//                                     of q^2 dx, q^2 dy (ceil(N / kChunk) x N x 8 bytes: the workspace grows as N^2 /
//                                     128); per (chunk, row block) the fp64 sum of the rows' fp32 sums of q
//               grad_kernel           Z = the fp64 sum of the q partials in a fixed order (every block computes it
//                                     alike), neg = the fp64 sum of a row's chunk partials in chunk order, the attraction
//                                     over the CSR row in sklearn's fp32 form, grad = 4 (pos - neg / Z); optionally the
//                                     KL terms and the optimiser update, fused
//               finish_kernel         KL and |grad| from the per-block partials; the optimiser's progress check
// The summation structure depends on N only (kChunk is fixed), there are no float atomics: results are bit-identical
// from run to run.  The optimiser runs all iterations of a phase without a host synchronisation; a device flag written
// by the check stops the remaining launches of the phase.  Positions alternate between two buffers (iteration i reads
// buffer i % 2 and writes the other), so no block reads a position another block has already moved.
#include <float.h>

#include "et_common.h"

namespace {

constexpr int kKnnBlock = 64;   // query rows per knn block (one wavefront)
constexpr int kKnnTile = 64;    // candidate rows per LDS tile
constexpr int kBlock = 256;     // rows per block of the per-row kernels
constexpr int kChunk = 1024;    // columns per repulsion chunk
constexpr int kCheckEvery = 50; // sklearn's _N_ITER_CHECK
constexpr int kMaxD = 32;

// ------------------------------------------------------------------------------------------------------------- kNN
// squared distance as sklearn's KD-tree computes it (the tree holds X as fp64): fp64 differences of the fp32 inputs,
// squared and summed in fp64 in coordinate order
template <int MD>
__global__ void __launch_bounds__(kKnnBlock) knn_kernel(const float *__restrict__ X, int64_t N, int d, int k,
                                                         double *__restrict__ kd, int32_t *__restrict__ ki,
                                                         int32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                         int *__restrict__ bad) {
    __shared__ float tile[kKnnTile * MD];
    const int64_t i = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
    const bool live = i < N;
    float xi[MD];
#pragma unroll
    for (int c = 0; c < MD; ++c) xi[c] = (live && c < d) ? X[i * d + c] : 0.f;
    if (live) {
        bool fin = true;
#pragma unroll
        for (int c = 0; c < MD; ++c) fin = fin && isfinite(xi[c]);
        if (!fin) atomicOr(bad, 1);
    }
    // the lane's list: slot s of row i at [s * N + i] (lanes of a wavefront touch adjacent words)
    int filled = 0;
    double worst = 0.0;
    for (int64_t t0 = 0; t0 < N; t0 += kKnnTile) {
        const int nt = (int)(N - t0 < kKnnTile ? N - t0 : kKnnTile);
        __syncthreads();
        for (int e = threadIdx.x; e < nt * d; e += kKnnBlock) tile[(e / d) * MD + e % d] = X[t0 * d + e];
        __syncthreads();
        if (!live) continue;
        for (int jj = 0; jj < nt; ++jj) {
            const int64_t j = t0 + jj;
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < MD; ++c) {
                if (c < d) {
                    const double t = (double)xi[c] - (double)tile[jj * MD + c];
                    s = s + t * t;
                }
            }
            if (j == i) continue;
            // candidates come in increasing index order: an equal distance never displaces a kept one
            if (filled == k && !(s < worst)) continue;
            int pos = filled < k ? filled : k - 1;
            while (pos > 0 && kd[(int64_t)(pos - 1) * N + i] > s) {
                kd[(int64_t)pos * N + i] = kd[(int64_t)(pos - 1) * N + i];
                ki[(int64_t)pos * N + i] = ki[(int64_t)(pos - 1) * N + i];
                --pos;
            }
            kd[(int64_t)pos * N + i] = s;
            ki[(int64_t)pos * N + i] = (int32_t)j;
            if (filled < k) ++filled;
            if (filled == k) worst = kd[(int64_t)(k - 1) * N + i];
        }
    }
    if (!live) return;
    // sklearn sorts the kNN graph's columns (distances.sort_indices()): reorder the list by index
    for (int a = 1; a < k; ++a) {
        const int32_t ia = ki[(int64_t)a * N + i];
        const double da = kd[(int64_t)a * N + i];
        int b = a;
        while (b > 0 && ki[(int64_t)(b - 1) * N + i] > ia) {
            ki[(int64_t)b * N + i] = ki[(int64_t)(b - 1) * N + i];
            kd[(int64_t)b * N + i] = kd[(int64_t)(b - 1) * N + i];
            --b;
        }
        ki[(int64_t)b * N + i] = ia;
        kd[(int64_t)b * N + i] = da;
    }
    for (int a = 0; a < k; ++a) {
        const double r = sqrt(kd[(int64_t)a * N + i]);  // the tree's distance, squared again (distances_nn.data **= 2)
        out_idx[i * k + a] = ki[(int64_t)a * N + i];
        out_dist[i * k + a] = (float)(r * r);
    }
}

// ------------------------------------------------------------------------------------------------ perplexity search
// sklearn.manifold._utils._binary_search_perplexity, one lane per row: fp64 beta and P, fp32 distances and constants
__global__ void __launch_bounds__(kBlock) perplexity_kernel(const float *__restrict__ dist, int64_t N, int k,
                                                            double desired_entropy, double *__restrict__ P) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const float *dr = dist + i * k;
    double *pr = P + i * k;
    const double tol = (double)1e-5f, eps_dbl = (double)1e-8f;  // PERPLEXITY_TOLERANCE, EPSILON_DBL are C floats
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    for (int l = 0; l < 100; ++l) {
        double sum_p = 0.0;
        for (int j = 0; j < k; ++j) {
            const double p = exp((double)(-dr[j]) * beta);
            pr[j] = p;
            sum_p = sum_p + p;
        }
        if (sum_p == 0.0) sum_p = eps_dbl;
        double sum_dp = 0.0;
        for (int j = 0; j < k; ++j) {
            const double p = pr[j] / sum_p;
            pr[j] = p;
            sum_dp = sum_dp + (double)dr[j] * p;
        }
        const double entropy = log(sum_p) + beta * sum_dp;
        const double diff = entropy - desired_entropy;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
}

// ------------------------------------------------------------------------------------------------- symmetrisation
__global__ void indeg_kernel(const int32_t *__restrict__ idx, int64_t nk, int *__restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < nk) atomicAdd(&cnt[idx[e]], 1);
}

// exclusive scan of n ints into off[0..n] (one block; n is at most a few million)
__global__ void __launch_bounds__(1024) scan_kernel(const int *__restrict__ cnt, int64_t n, int32_t *__restrict__ off) {
    __shared__ int64_t part[1024];
    const int64_t per = et::ceil_div(n, 1024);
    const int64_t a = threadIdx.x * per, b = a + per < n ? a + per : n;
    int64_t s = 0;
    for (int64_t e = a; e < b; ++e) s += cnt[e];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; ++t) {
            const int64_t v = part[t];
            part[t] = run;
            run += v;
        }
        off[n] = (int32_t)run;
    }
    __syncthreads();
    s = part[threadIdx.x];
    for (int64_t e = a; e < b; ++e) {
        off[e] = (int32_t)s;
        s += cnt[e];
    }
}

__global__ void scatter_kernel(const int32_t *__restrict__ idx, const double *__restrict__ pc, int64_t N, int k,
                               const int32_t *__restrict__ roff, int *__restrict__ fill, int32_t *__restrict__ rsrc,
                               double *__restrict__ rval) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= N * k) return;
    const int32_t j = idx[e];
    const int at = roff[j] + atomicAdd(&fill[j], 1);
    rsrc[at] = (int32_t)(e / k);
    rval[at] = pc[e];
}

// the reverse list of row j sorted by source row (the scatter's order is a race; each source appears once per row)
__global__ void rev_sort_kernel(const int32_t *__restrict__ roff, int64_t N, int32_t *__restrict__ rsrc,
                                double *__restrict__ rval) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= N) return;
    const int a0 = roff[j], a1 = roff[j + 1];
    for (int a = a0 + 1; a < a1; ++a) {
        const int32_t s = rsrc[a];
        const double v = rval[a];
        int b = a;
        while (b > a0 && rsrc[b - 1] > s) {
            rsrc[b] = rsrc[b - 1];
            rval[b] = rval[b - 1];
            --b;
        }
        rsrc[b] = s;
        rval[b] = v;
    }
}

// row i of P_cond + P_cond^T: merge of the forward row (k entries, sorted columns) and the reverse list; scipy's
// canonical sum drops entries whose sum is 0.  FILL = false counts, FILL = true writes columns, values and the row's
// sequential fp64 sum (csr_matvec's order, which P.sum() reduces).
template <bool FILL>
__global__ void merge_kernel(const int32_t *__restrict__ idx, const double *__restrict__ pc, int64_t N, int k,
                             const int32_t *__restrict__ roff, const int32_t *__restrict__ rsrc,
                             const double *__restrict__ rval, int *__restrict__ rowlen, const int32_t *__restrict__ indptr,
                             int32_t *__restrict__ indices, double *__restrict__ P, double *__restrict__ rowsum) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    int a = 0, b = roff[i];
    const int b1 = roff[i + 1];
    int n = 0;
    const int w0 = FILL ? indptr[i] : 0;
    double s = 0.0;
    while (a < k || b < b1) {
        const int32_t ca = a < k ? idx[i * k + a] : INT32_MAX;
        const int32_t cb = b < b1 ? rsrc[b] : INT32_MAX;
        int32_t c;
        double v;
        if (ca == cb) {
            c = ca;
            v = pc[i * k + a] + rval[b];
            ++a;
            ++b;
        } else if (ca < cb) {
            c = ca;
            v = pc[i * k + a];
            ++a;
        } else {
            c = cb;
            v = rval[b];
            ++b;
        }
        if (v == 0.0) continue;
        if (FILL) {
            indices[w0 + n] = c;
            P[w0 + n] = v;
            s = s + v;
        }
        ++n;
    }
    if (FILL)
        rowsum[i] = s;
    else
        rowlen[i] = n;
}

// numpy's pairwise summation of a contiguous fp64 array (blocks of at most 128 summed with 8 accumulators, halves split
// at a multiple of 8): P.sum() = (P @ ones).sum() reduces the row sums this way
__device__ double pairwise_block(const double *p, int64_t n) {
    if (n < 8) {
        double res = -0.0;
        for (int64_t e = 0; e < n; ++e) res = res + p[e];
        return res;
    }
    double r[8];
    for (int u = 0; u < 8; ++u) r[u] = p[u];
    int64_t e;
    for (e = 8; e < n - (n % 8); e += 8)
        for (int u = 0; u < 8; ++u) r[u] = r[u] + p[e + u];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; e < n; ++e) res = res + p[e];
    return res;
}

__device__ double pairwise_sum(const double *a, int64_t n) {
    struct Frame {
        int64_t off, n;
        int state;
    };
    Frame fr[64];
    double res[64];
    int sp = 0, nr = 0;
    fr[sp++] = Frame{0, n, 0};
    while (sp > 0) {
        Frame &f = fr[sp - 1];
        if (f.n <= 128) {
            res[nr++] = pairwise_block(a + f.off, f.n);
            --sp;
            continue;
        }
        int64_t n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) {
            f.state = 1;
            fr[sp++] = Frame{f.off, n2, 0};
        } else if (f.state == 1) {
            f.state = 2;
            fr[sp++] = Frame{f.off + n2, f.n - n2, 0};
        } else {
            res[nr - 2] = res[nr - 2] + res[nr - 1];
            --nr;
            --sp;
        }
    }
    return res[0];
}

// sum_P = max(P.sum(), DBL_EPSILON); P /= sum_P is scipy's data *= (1.0 / sum_P)
__global__ void total_kernel(const double *__restrict__ rowsum, int64_t N, double *__restrict__ total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const double t = pairwise_sum(rowsum, N);
        total[0] = t;
        total[1] = 1.0 / (t > DBL_EPSILON ? t : DBL_EPSILON);
    }
}

__global__ void normalize_kernel(double *__restrict__ P, const int32_t *__restrict__ indptr, int64_t N,
                                 const double *__restrict__ total) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < indptr[N]) P[e] = P[e] * total[1];
}

// ------------------------------------------------------------------------------------------------------- gradient
struct OptState {
    double error, best_error, grad_norm, pad;
    int32_t best_iter, stop;
    int32_t last_iter;  // the last iteration run (-1: none); its new positions are in buffer (last_iter + 1) % 2
    int32_t n_iter;     // sklearn's returned i: the last iteration run, or `it` for a phase that runs none
    int32_t bad, pad2;
};

__device__ __forceinline__ double block_sum_f64(double v, double *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// per row i and column chunk c: (nx, ny) = sum q^2 (y_i - y_j) over the chunk's j whose position differs from y_i in
// at least one coordinate (fp32, j order); zpart[c * nrb + block] = the fp64 sum of the block's rows' fp32 sums of q
// over the chunk
__global__ void __launch_bounds__(kBlock) rep_kernel(const float2 *__restrict__ Y, int64_t N, float *__restrict__ part,
                                                     double *__restrict__ zpart, const OptState *__restrict__ st) {
    if (st && st->stop) return;
    __shared__ float2 ty[kChunk];
    __shared__ double sh[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * kChunk;
    const int nc = (int)(N - c0 < kChunk ? N - c0 : kChunk);
    for (int e = threadIdx.x; e < nc; e += kBlock) ty[e] = Y[c0 + e];
    __syncthreads();
    const bool live = i < N;
    const float2 yi = live ? Y[i] : make_float2(0.f, 0.f);
    float z = 0.f, nx = 0.f, ny = 0.f;
    if (live) {
        const int self = (i >= c0 && i < c0 + nc) ? (int)(i - c0) : -1;
        for (int j = 0; j < nc; ++j) {
            const float dx = yi.x - ty[j].x, dy = yi.y - ty[j].y;
            const float d2 = fmaf(dy, dy, dx * dx);
            // like sklearn's tree as compiled, which leaves out the points exactly coincident with the query (its own
            // "self interaction": the 1e-6 its source names has no effect), not only j == i: coincident
            // points (no force, dx = dy = 0) do not inflate Z; a point 1e-7 away counts like any other
            const bool skip = j == self || (dx == 0.f && dy == 0.f);
            const float q = skip ? 0.f : 1.0f / (1.0f + d2);
            const float q2 = q * q;
            z = z + q;
            nx = fmaf(q2, dx, nx);
            ny = fmaf(q2, dy, ny);
        }
        const int64_t o = ((int64_t)blockIdx.y * N + i) * 2;
        part[o] = nx;
        part[o + 1] = ny;
    }
    const double bz = block_sum_f64((double)z, sh);
    if (threadIdx.x == 0) zpart[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = bz;
}

// sklearn's _gradient_descent update of one coordinate (numpy 2 promotion: update fp64, p / gains / grad fp32)
__device__ __forceinline__ void opt_update(float &p, double &u, float &gain, float &g, double momentum, double lr) {
    const bool inc = u * (double)g < 0.0;
    gain = inc ? gain + 0.2f : gain * 0.8f;
    gain = gain < 0.01f ? 0.01f : gain;  // np.clip(gains, min_gain, inf)
    g = g * gain;
    u = momentum * u - lr * (double)g;
    p = (float)((double)p + u);
}

struct GradArgs {
    const int32_t *indptr, *indices;
    const float *P;           // fp32 P (exaggerated in phase 1)
    const float *part;
    const double *zpart;
    int64_t N, nzp;
    float *grad;              // out (kl_grad) or NULL (optimiser)
    double *klpart, *gnpart;  // per block
    int want_kl;
    // optimiser (gains != NULL): the updated positions go to Ynext (other blocks still read Yw)
    float *Yw, *Ynext, *gains;
    double *upd;
    double momentum, lr;
    int iter;
    OptState *st;
};

__global__ void __launch_bounds__(kBlock) grad_kernel(GradArgs a) {
    if (a.st && a.st->stop) return;
    __shared__ double sh[kBlock];
    // Z: the same fixed order in every block
    double zs = 0.0;
    for (int64_t e = threadIdx.x; e < a.nzp; e += kBlock) zs = zs + a.zpart[e];
    // sklearn: sum_Q = max(sum_Q, DBL_EPSILON) -- all points coincident: Z = 0, every force 0, the gradient exactly 0
    const double zsum = block_sum_f64(zs, sh);
    const double Z = zsum > DBL_EPSILON ? zsum : DBL_EPSILON;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t N = a.N;
    double kl = 0.0, gn = 0.0;
    if (i < N) {
        const float2 *Yr = reinterpret_cast<const float2 *>(a.Yw);
        const float2 yi = Yr[i];
        const int64_t nch = et::ceil_div(N, kChunk);
        double negx = 0.0, negy = 0.0;
        for (int64_t c = 0; c < nch; ++c) {
            negx = negx + (double)a.part[(c * N + i) * 2];
            negy = negy + (double)a.part[(c * N + i) * 2 + 1];
        }
        // compute_gradient_positive: fp32, CSR order
        float px = 0.f, py = 0.f;
        for (int e = a.indptr[i]; e < a.indptr[i + 1]; ++e) {
            const float2 yj = Yr[a.indices[e]];
            const float bx = yi.x - yj.x, by = yi.y - yj.y;
            const float dij = bx * bx + by * by;
            const float q = 1.0f / (1.0f + dij);
            const float pij = a.P[e];
            const float pq = pij * q;
            if (a.want_kl) {
                const float qz = (float)((double)q / Z);
                const float num = pij > FLT_MIN ? pij : FLT_MIN, den = qz > FLT_MIN ? qz : FLT_MIN;
                kl = kl + (double)pij * log((double)(num / den));
            }
            px = px + pq * bx;
            py = py + pq * by;
        }
        float gx = (float)((double)px - negx / Z) * 4.0f;
        float gy = (float)((double)py - negy / Z) * 4.0f;
        if (a.gains) {
            float2 p = yi;
            opt_update(p.x, a.upd[2 * i], a.gains[2 * i], gx, a.momentum, a.lr);
            opt_update(p.y, a.upd[2 * i + 1], a.gains[2 * i + 1], gy, a.momentum, a.lr);
            gn = (double)gx * (double)gx + (double)gy * (double)gy;
            reinterpret_cast<float2 *>(a.Ynext)[i] = p;
        } else {
            a.grad[2 * i] = gx;
            a.grad[2 * i + 1] = gy;
        }
    }
    const double bk = block_sum_f64(kl, sh);
    const double bg = block_sum_f64(gn, sh);
    if (threadIdx.x == 0) {
        a.klpart[blockIdx.x] = bk;
        a.gnpart[blockIdx.x] = bg;
        if (a.st && blockIdx.x == 0) a.st->last_iter = a.st->n_iter = a.iter;
    }
}

// KL and |grad| from the block partials; with a state, sklearn's progress check of iteration `iter`
__global__ void __launch_bounds__(kBlock) finish_kernel(const double *__restrict__ klpart,
                                                        const double *__restrict__ gnpart, int nb, double *__restrict__ kl,
                                                        OptState *__restrict__ st, int iter, int check, int nwp) {
    if (st && st->stop) return;
    __shared__ double sh[kBlock];
    double a = 0.0, b = 0.0;
    for (int e = threadIdx.x; e < nb; e += kBlock) {
        a = a + klpart[e];
        b = b + gnpart[e];
    }
    const double err = block_sum_f64(a, sh);
    const double gn2 = block_sum_f64(b, sh);
    if (threadIdx.x != 0) return;
    if (kl) kl[0] = err;
    if (!st) return;
    st->error = err;
    st->grad_norm = sqrt(gn2);
    if (!check) return;
    if (err < st->best_error) {
        st->best_error = err;
        st->best_iter = iter;
    } else if (iter - st->best_iter > nwp) {
        st->stop = 1;
    }
    if (st->grad_norm <= 1e-7) st->stop = 1;
}

__global__ void update_kernel(float *__restrict__ p, double *__restrict__ u, float *__restrict__ gains,
                              float *__restrict__ g, int64_t n, double momentum, double lr) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    float pe = p[e], ge = g[e], ga = gains[e];
    double ue = u[e];
    opt_update(pe, ue, ga, ge, momentum, lr);
    p[e] = pe;
    u[e] = ue;
    gains[e] = ga;
    g[e] = ge;
}

// phase setup: fp32 P = fp32(P64 * ee) (phase 1) or fp32((P64 * ee) / ee) (phase 2, sklearn's P /= early_exaggeration);
// update = 0, gains = 1; the state of a _gradient_descent call: error = best_error = DBL_MAX, best_iter = i = it
__global__ void phase_kernel(const double *__restrict__ P64, int64_t nnz, double ee, int phase2, float *__restrict__ P32,
                             double *__restrict__ u, float *__restrict__ gains, int64_t n2, int it,
                             OptState *__restrict__ st) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < nnz) {
        const double x = P64[e] * ee;
        P32[e] = (float)(phase2 ? x / ee : x);
    }
    if (e < n2) {
        u[e] = 0.0;
        gains[e] = 1.0f;
    }
    if (e == 0) {
        st->error = DBL_MAX;
        st->best_error = DBL_MAX;
        st->best_iter = it;  // best_iter = i = it
        st->n_iter = it;
        if (!phase2) st->last_iter = -1;
        st->stop = 0;
    }
}

__global__ void finite_kernel(const float *__restrict__ x, int64_t n, int *__restrict__ bad) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < n && !isfinite(x[e])) atomicOr(bad, 1);
}

// ------------------------------------------------------------------------------------------------------ PCA init
// column means (fp64) and the fp64 Gram of the fp32-centred rows, one block
__global__ void __launch_bounds__(kBlock) pca_cov_kernel(const float *__restrict__ X, int64_t N, int d,
                                                         float *__restrict__ mean32, double *__restrict__ G) {
    __shared__ double sh[kBlock];
    __shared__ float m[kMaxD];
    for (int c = 0; c < d; ++c) {
        double s = 0.0;
        for (int64_t r = threadIdx.x; r < N; r += kBlock) s = s + (double)X[r * d + c];
        const double t = block_sum_f64(s, sh);
        if (threadIdx.x == 0) {
            m[c] = (float)(t / (double)N);
            mean32[c] = m[c];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < d * d; e += kBlock) {
        const int r0 = e / d, c0 = e % d;
        double s = 0.0;
        for (int64_t r = 0; r < N; ++r) {
            const double a = (double)(X[r * d + r0] - m[r0]), b = (double)(X[r * d + c0] - m[c0]);
            s = s + a * b;
        }
        G[e] = s;
    }
}

// Y = (X - mean) V with each component's largest-|.| entry positive (svd_flip, u_based_decision=False), then
// Y / std(Y[:, 0]) * 1e-4 (np.std: fp64 here)
__global__ void __launch_bounds__(kBlock) pca_project_kernel(const float *__restrict__ X, int64_t N, int d,
                                                             const float *__restrict__ mean32,
                                                             const float *__restrict__ U, float *__restrict__ Y) {
    __shared__ double sh[kBlock];
    __shared__ float v[kMaxD * 2];
    if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        int best = 0;
        for (int r = 1; r < d; ++r)
            if (fabsf(U[r * 2 + c]) > fabsf(U[best * 2 + c])) best = r;
        const float sg = U[best * 2 + c] < 0.f ? -1.f : 1.f;
        for (int r = 0; r < d; ++r) v[r * 2 + c] = U[r * 2 + c] * sg;
    }
    __syncthreads();
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < N; r += kBlock) {
        float y0 = 0.f, y1 = 0.f;
        for (int c = 0; c < d; ++c) {
            const float xc = X[r * d + c] - mean32[c];
            y0 = fmaf(xc, v[c * 2], y0);
            y1 = fmaf(xc, v[c * 2 + 1], y1);
        }
        Y[2 * r] = y0;
        Y[2 * r + 1] = y1;
        s = s + (double)y0;
    }
    const double mu = block_sum_f64(s, sh) / (double)N;
    double q = 0.0;
    for (int64_t r = threadIdx.x; r < N; r += kBlock) {
        const double t = (double)Y[2 * r] - mu;
        q = q + t * t;
    }
    const float sd = (float)sqrt(block_sum_f64(q, sh) / (double)N);
    for (int64_t r = threadIdx.x; r < N; r += kBlock) {
        Y[2 * r] = (Y[2 * r] / sd) * 1e-4f;
        Y[2 * r + 1] = (Y[2 * r + 1] / sd) * 1e-4f;
    }
}

// ----------------------------------------------------------------------------------------------------- workspace
size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct AffWs {
    size_t kd, ki, cnt, roff, fill, rsrc, rval, rowlen, rowsum, total, bad, end;
};
AffWs aff_ws(int64_t N, int k) {
    AffWs w{};
    size_t o = 0;
    const size_t nk = (size_t)N * (size_t)k;
    w.kd = o; o += al(nk * 8);
    w.ki = o; o += al(nk * 4);
    w.cnt = o; o += al((size_t)N * 4);
    w.roff = o; o += al((size_t)(N + 1) * 4);
    w.fill = o; o += al((size_t)N * 4);
    w.rsrc = o; o += al(nk * 4);
    w.rval = o; o += al(nk * 8);
    w.rowlen = o; o += al((size_t)N * 4);
    w.rowsum = o; o += al((size_t)N * 8);
    w.total = o; o += al(16);
    w.bad = o; o += al(4);
    w.end = o;
    return w;
}

struct GradWs {
    size_t part, zpart, klpart, gnpart, bad, end;
};
GradWs grad_ws(int64_t N) {
    GradWs w{};
    const int64_t nch = et::ceil_div(N, kChunk), nrb = et::ceil_div(N, kBlock);
    size_t o = 0;
    w.part = o; o += al((size_t)nch * (size_t)N * 2 * 4);
    w.zpart = o; o += al((size_t)nch * (size_t)nrb * 8);
    w.klpart = o; o += al((size_t)nrb * 8);
    w.gnpart = o; o += al((size_t)nrb * 8);
    w.bad = o; o += al(4);
    w.end = o;
    return w;
}

struct OptWs {
    GradWs g;
    size_t p32, upd, gains, ynext, st, end;
};
OptWs opt_ws(int64_t N, int64_t nnz) {
    OptWs w{};
    w.g = grad_ws(N);
    size_t o = w.g.end;
    w.p32 = o; o += al((size_t)nnz * 4);
    w.upd = o; o += al((size_t)N * 2 * 8);
    w.gains = o; o += al((size_t)N * 2 * 4);
    w.ynext = o; o += al((size_t)N * 2 * 4);
    w.st = o; o += al(sizeof(OptState));
    w.end = o;
    return w;
}

template <typename T>
T *at(void *ws, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(ws) + off); }

unsigned blocks(int64_t n) { return (unsigned)et::ceil_div(n > 0 ? n : 1, kBlock); }

// rep + grad (+ finish) for one evaluation
int launch_grad(const float *Y, float *Ynext, int64_t N, const int32_t *indptr, const int32_t *indices, const float *P32,
                float *grad, int want_kl, const GradWs &w, void *ws, double *upd, float *gains, double momentum,
                double lr, int iter, OptState *st, double *kl, int check, int nwp, hipStream_t s) {
    const int64_t nch = et::ceil_div(N, kChunk), nrb = et::ceil_div(N, kBlock);
    rep_kernel<<<dim3((unsigned)nrb, (unsigned)nch), kBlock, 0, s>>>(reinterpret_cast<const float2 *>(Y), N,
                                                                      at<float>(ws, w.part), at<double>(ws, w.zpart), st);
    ET_LAUNCH_CHECK();
    GradArgs a{};
    a.indptr = indptr;
    a.indices = indices;
    a.P = P32;
    a.part = at<float>(ws, w.part);
    a.zpart = at<double>(ws, w.zpart);
    a.N = N;
    a.nzp = nch * nrb;
    a.grad = grad;
    a.klpart = at<double>(ws, w.klpart);
    a.gnpart = at<double>(ws, w.gnpart);
    a.want_kl = want_kl;
    a.Yw = const_cast<float *>(Y);
    a.Ynext = Ynext;
    a.gains = gains;
    a.upd = upd;
    a.momentum = momentum;
    a.lr = lr;
    a.iter = iter;
    a.st = st;
    grad_kernel<<<(unsigned)nrb, kBlock, 0, s>>>(a);
    ET_LAUNCH_CHECK();
    if (want_kl) {
        finish_kernel<<<1, kBlock, 0, s>>>(at<double>(ws, w.klpart), at<double>(ws, w.gnpart), (int)nrb, kl, st, iter,
                                           check, nwp);
        ET_LAUNCH_CHECK();
    }
    return ET_OK;
}

bool aligned(const void *p, unsigned m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) == 0; }

// N the gradient takes: the chunk count is gridDim.y (at most 65 535)
bool grad_n_ok(int64_t N) { return N >= 2 && et::ceil_div(N, kChunk) <= 65535; }

// ET_ERR_BAD_DATA if any of x[0..n) is not finite (one stream synchronisation)
int check_finite(const float *x, int64_t n, int *flag, hipStream_t s) {
    ET_HIP_TRY(hipMemsetAsync(flag, 0, 4, s));
    finite_kernel<<<blocks(n), kBlock, 0, s>>>(x, n, flag);
    ET_LAUNCH_CHECK();
    int h = 0;
    ET_HIP_TRY(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, s));
    ET_HIP_TRY(hipStreamSynchronize(s));
    return h ? ET_ERR_BAD_DATA : ET_OK;
}

}  // namespace

extern "C" int et_tsne_neighbors(int64_t N, double perplexity) {
    if (N < 2 || !(perplexity > 0.0)) return 0;
    const double f = floor(3.0 * perplexity + 1.0);
    const int64_t k = f < (double)(N - 1) ? (int64_t)f : N - 1;
    return k < 1 ? 1 : (int)k;
}

extern "C" size_t et_tsne_affinities_workspace_bytes(int64_t N, int d, int k) {
    if (N < 2 || d < 1 || d > kMaxD || k < 1 || k > N - 1 || 2 * N * (int64_t)k > INT32_MAX) return 0;
    return aff_ws(N, k).end;
}

extern "C" int et_tsne_affinities(const float *X, int64_t N, int d, double perplexity, int k, int32_t *knn_idx,
                                  float *knn_dist, double *p_cond, int32_t *indptr, int32_t *indices, double *P,
                                  double *p_total, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    if (N < 2) return ET_ERR_BAD_DATA;
    if (!X || !knn_idx || !knn_dist || !p_cond || !indptr || !indices || !P || d < 1 || d > kMaxD ||
        !(perplexity > 0.0) || k < 1 || k > N - 1 || 2 * N * (int64_t)k > INT32_MAX)
        return ET_ERR_INVALID_ARG;
    if (!aligned(X, 4) || !aligned(p_cond, 8) || !aligned(P, 8)) return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_tsne_affinities_workspace_bytes(N, d, k)) return ET_ERR_WORKSPACE;
    const AffWs w = aff_ws(N, k);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    void *ws = workspace;
    int *bad = at<int>(ws, w.bad), *cnt = at<int>(ws, w.cnt), *fill = at<int>(ws, w.fill);
    ET_HIP_TRY(hipMemsetAsync(bad, 0, 4, s));
    ET_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)N * 4, s));
    ET_HIP_TRY(hipMemsetAsync(fill, 0, (size_t)N * 4, s));
    const unsigned kb = (unsigned)et::ceil_div(N, kKnnBlock);
    if (d <= 8)
        knn_kernel<8><<<kb, kKnnBlock, 0, s>>>(X, N, d, k, at<double>(ws, w.kd), at<int32_t>(ws, w.ki), knn_idx,
                                                 knn_dist, bad);
    else
        knn_kernel<kMaxD><<<kb, kKnnBlock, 0, s>>>(X, N, d, k, at<double>(ws, w.kd), at<int32_t>(ws, w.ki), knn_idx,
                                                     knn_dist, bad);
    ET_LAUNCH_CHECK();
    perplexity_kernel<<<blocks(N), kBlock, 0, s>>>(knn_dist, N, k, log((double)(float)perplexity), p_cond);
    ET_LAUNCH_CHECK();
    const int64_t nk = N * k;
    int32_t *roff = at<int32_t>(ws, w.roff), *rsrc = at<int32_t>(ws, w.rsrc);
    double *rval = at<double>(ws, w.rval), *rowsum = at<double>(ws, w.rowsum), *total = at<double>(ws, w.total);
    int *rowlen = at<int>(ws, w.rowlen);
    indeg_kernel<<<blocks(nk), kBlock, 0, s>>>(knn_idx, nk, cnt);
    ET_LAUNCH_CHECK();
    scan_kernel<<<1, 1024, 0, s>>>(cnt, N, roff);
    ET_LAUNCH_CHECK();
    scatter_kernel<<<blocks(nk), kBlock, 0, s>>>(knn_idx, p_cond, N, k, roff, fill, rsrc, rval);
    ET_LAUNCH_CHECK();
    rev_sort_kernel<<<blocks(N), kBlock, 0, s>>>(roff, N, rsrc, rval);
    ET_LAUNCH_CHECK();
    merge_kernel<false><<<blocks(N), kBlock, 0, s>>>(knn_idx, p_cond, N, k, roff, rsrc, rval, rowlen, nullptr, nullptr,
                                                     nullptr, nullptr);
    ET_LAUNCH_CHECK();
    scan_kernel<<<1, 1024, 0, s>>>(rowlen, N, indptr);
    ET_LAUNCH_CHECK();
    merge_kernel<true><<<blocks(N), kBlock, 0, s>>>(knn_idx, p_cond, N, k, roff, rsrc, rval, nullptr, indptr, indices,
                                                    P, rowsum);
    ET_LAUNCH_CHECK();
    total_kernel<<<1, 64, 0, s>>>(rowsum, N, total);
    ET_LAUNCH_CHECK();
    normalize_kernel<<<blocks(2 * nk), kBlock, 0, s>>>(P, indptr, N, total);
    ET_LAUNCH_CHECK();
    if (p_total) ET_HIP_TRY(hipMemcpyAsync(p_total, total, 8, hipMemcpyDeviceToDevice, s));
    int bad_h = 0;
    ET_HIP_TRY(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, s));
    ET_HIP_TRY(hipStreamSynchronize(s));
    return bad_h ? ET_ERR_BAD_DATA : ET_OK;
}

extern "C" size_t et_tsne_kl_grad_workspace_bytes(int64_t N) {
    if (!grad_n_ok(N)) return 0;
    return grad_ws(N).end;
}

extern "C" int et_tsne_kl_grad(const float *Y, int64_t N, const int32_t *indptr, const int32_t *indices, const float *P,
                               float *grad, double *kl, void *workspace, size_t workspace_bytes, et_stream_t stream) {
    if (N < 2) return ET_ERR_BAD_DATA;
    if (!Y || !indptr || !indices || !P || !grad || !grad_n_ok(N) || !aligned(Y, 8) || !aligned(grad, 4))
        return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_tsne_kl_grad_workspace_bytes(N)) return ET_ERR_WORKSPACE;
    const GradWs w = grad_ws(N);
    const int rc = check_finite(Y, 2 * N, at<int>(workspace, w.bad), static_cast<hipStream_t>(stream));
    if (rc) return rc;
    return launch_grad(Y, nullptr, N, indptr, indices, P, grad, kl ? 1 : 0, w, workspace, nullptr, nullptr, 0.0, 0.0, 0,
                       nullptr, kl, 0, 0, static_cast<hipStream_t>(stream));
}

extern "C" int et_tsne_update(float *p, double *update, float *gains, float *grad, int64_t n, double momentum,
                              double learning_rate, et_stream_t stream) {
    if (!p || !update || !gains || !grad || n < 1) return ET_ERR_INVALID_ARG;
    update_kernel<<<blocks(n), kBlock, 0, static_cast<hipStream_t>(stream)>>>(p, update, gains, grad, n, momentum,
                                                                               learning_rate);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

extern "C" size_t et_tsne_optimize_workspace_bytes(int64_t N, int64_t nnz) {
    if (!grad_n_ok(N) || nnz < 0 || nnz > INT32_MAX) return 0;
    return opt_ws(N, nnz).end;
}

extern "C" int et_tsne_optimize(float *Y, int64_t N, const int32_t *indptr, const int32_t *indices, const double *P,
                                int64_t nnz, double early_exaggeration, double learning_rate, int max_iter,
                                double *kl_out, int *n_iter_out, void *workspace, size_t workspace_bytes,
                                et_stream_t stream) {
    if (N < 2) return ET_ERR_BAD_DATA;
    if (!Y || !indptr || !indices || !P || !grad_n_ok(N) || nnz < 0 || nnz > INT32_MAX || !aligned(Y, 8) ||
        !(early_exaggeration > 0.0) || !(learning_rate > 0.0) || max_iter < 1)
        return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_tsne_optimize_workspace_bytes(N, nnz)) return ET_ERR_WORKSPACE;
    const OptWs w = opt_ws(N, nnz);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    void *ws = workspace;
    float *P32 = at<float>(ws, w.p32), *gains = at<float>(ws, w.gains);
    double *upd = at<double>(ws, w.upd);
    OptState *st = at<OptState>(ws, w.st);
    ET_HIP_TRY(hipMemsetAsync(st, 0, sizeof(OptState), s));
    finite_kernel<<<blocks(2 * N), kBlock, 0, s>>>(Y, 2 * N, &st->bad);
    ET_LAUNCH_CHECK();
    OptState h{};
    float *buf[2] = {Y, at<float>(ws, w.ynext)};
    // TSNE._tsne: 250 exploration iterations (P * ee, momentum 0.5), then the rest (P / ee, momentum 0.8).  max_iter
    // below 250 (not an sklearn setting) ends the first phase early.
    const int explore = 250;
    int it = 0;
    for (int ph = 0; ph < 2; ++ph) {
        const int end = ph ? max_iter : (max_iter < explore ? max_iter : explore);
        const int nwp = ph ? 300 : explore;
        const double mom = ph ? 0.8 : 0.5;
        if (ph) {
            ET_HIP_TRY(hipMemcpyAsync(&h, st, sizeof(OptState), hipMemcpyDeviceToHost, s));
            ET_HIP_TRY(hipStreamSynchronize(s));
            if (h.bad) return ET_ERR_BAD_DATA;
            // sklearn: it = the i phase 1 returned; phase 2 runs from it + 1 if it < 250 or max_iter > 250 -- always,
            // as phase 1 returns at most 249.  At max_iter = 250 it runs no iteration and returns i = 250 and
            // error = finfo(float).max, which is reproduced.
            if (!(h.n_iter < explore || max_iter - explore > 0)) break;
            it = h.n_iter + 1;
        }
        const int64_t nmax = nnz > 2 * N ? nnz : 2 * N;
        phase_kernel<<<blocks(nmax), kBlock, 0, s>>>(P, nnz, early_exaggeration, ph, P32, upd, gains, 2 * N, it, st);
        ET_LAUNCH_CHECK();
        for (int i = it; i < end; ++i) {
            const int check = (i + 1) % kCheckEvery == 0;
            const int want = check || i == end - 1;
            const int rc = launch_grad(buf[i & 1], buf[(i + 1) & 1], N, indptr, indices, P32, nullptr, want, w.g, ws, upd,
                                       gains, mom, learning_rate, i, st, nullptr, check, nwp, s);
            if (rc) return rc;
        }
    }
    ET_HIP_TRY(hipMemcpyAsync(&h, st, sizeof(OptState), hipMemcpyDeviceToHost, s));
    ET_HIP_TRY(hipStreamSynchronize(s));
    if (h.bad) return ET_ERR_BAD_DATA;
    if ((h.last_iter + 1) & 1) {  // the last positions are in the second buffer
        ET_HIP_TRY(hipMemcpyAsync(Y, buf[1], (size_t)N * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
        ET_HIP_TRY(hipStreamSynchronize(s));
    }
    if (kl_out) *kl_out = h.error;
    if (n_iter_out) *n_iter_out = h.n_iter;
    return ET_OK;
}

extern "C" size_t et_tsne_pca_init_workspace_bytes(int64_t N, int d) {
    if (N < 2 || d < 2 || d > kMaxD) return 0;
    return al((size_t)d * d * 8) + al((size_t)d * 4) + al((size_t)d * 2 * 4) + al(8) + al(4);
}

extern "C" int et_tsne_pca_init(const float *X, int64_t N, int d, float *Y, void *workspace, size_t workspace_bytes,
                                et_stream_t stream) {
    if (N < 2) return ET_ERR_BAD_DATA;
    if (!X || !Y || d < 2 || d > kMaxD) return ET_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < et_tsne_pca_init_workspace_bytes(N, d)) return ET_ERR_WORKSPACE;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    double *G = at<double>(workspace, 0);
    float *mean32 = at<float>(workspace, al((size_t)d * d * 8));
    float *U = at<float>(workspace, al((size_t)d * d * 8) + al((size_t)d * 4));
    float *sig = at<float>(workspace, al((size_t)d * d * 8) + al((size_t)d * 4) + al((size_t)d * 2 * 4));
    int *bad = at<int>(workspace, al((size_t)d * d * 8) + al((size_t)d * 4) + al((size_t)d * 2 * 4) + al(8));
    const int fr = check_finite(X, N * d, bad, s);
    if (fr) return fr;
    pca_cov_kernel<<<1, kBlock, 0, s>>>(X, N, d, mean32, G);
    ET_LAUNCH_CHECK();
    const int rc = et_eigh_topk(G, d, 2, U, sig, stream);
    if (rc) return rc;
    pca_project_kernel<<<1, kBlock, 0, s>>>(X, N, d, mean32, U, Y);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

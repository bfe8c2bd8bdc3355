// et_stgcnn_core.inl -- the Social-STGCNN scene body (header comment: et_stgcnn.hip), one fragment #included by et_stgcnn.hip
// and by et_gpgraph_stgcnn.hip inside their anonymous namespaces.  run_scene is a template on a source Src:
//   Src::load / lap / store   where a scene's input comes from, one entry of its Laplacian, where an output entry goes
//   Src::kComputed            the Laplacian is formed from u and d where it is used (never stored); then
//   Src::key(w), keep(vv, kw) keep says whether the inverse distance of the pair (vv, w) stays in a_inv, given kw = key(w), which
//                             the loops over vv read once per lane -- it multiplies a_inv BEFORE + I, so it
//                             enters the degree as well (GP-Graph's intra-group mask); constant true for ET-STGCNN
//   Src::kPerRow              false: ET-STGCNN's gcn (baseline/stgcnn/model.py: a 1x1 conv to S K channels, contracted over
//                             kk AND v with L[kk]); true: the original Social-STGCNN gcn that GP-Graph-STGCNN wraps
//                             (baseline/gpgraphstgcnn/model_baseline.py: a 1x1 conv to S channels, time row t contracted with
//                             its own L[t] only).  dims_of(p, per_row) sizes q for either.
// The kPerRow = false instantiations keep the arithmetic they had before the fragment (the build sets -ffp-contract=off).
constexpr int kSgThreads = 256;         // = et_scene_project's workgroup: the same obs_ori reduction order
constexpr int kSgLdsBytes = 60 * 1024;  // LDS arena of one workgroup (two workgroups per CU)
constexpr int kSgGroup = 16;            // contraction rows per lane
constexpr int kSgMaxS = 64;

// Host side of the arena's placement, for the three predictors that keep one of `per` floats per pedestrian (ET-STGCNN,
// DMRGCN, Graph-TERN).  *_workspace_bytes: none when the largest scene fits the LDS arena, else every scene's rows.
static inline size_t arena_workspace_bytes(int64_t per, int64_t N, int64_t max_scene_n) {
    return per * max_scene_n * 4 <= kSgLdsBytes ? 0 : (size_t)(per * N * 4);
}
// *_forward_graph's one scene: in LDS, sized for exactly its N pedestrians, else in the caller's workspace (both LDS
// figures 0), else status = ET_ERR_WORKSPACE
struct ArenaPlace {
    int status;
    unsigned lds_bytes;
    int lds_floats;
};
static inline ArenaPlace arena_place_scene(int64_t per, int64_t N, const void *workspace, size_t workspace_bytes) {
    if (per * N * 4 <= kSgLdsBytes) return {ET_OK, (unsigned)(per * N * 4), (int)(per * N)};
    const bool fits = workspace && workspace_bytes >= (size_t)(per * N * 4);
    return {fits ? ET_OK : ET_ERR_WORKSPACE, 0u, 0};
}

struct Dims {
    int K, k, S, n_st, n_tp;
    int qpp;  // floats per pedestrian of q
};

__host__ __device__ inline Dims dims_of(const et_stgcnn_params &p, bool per_row = false) {
    Dims d{p.seq_len, p.pred_seq_len, p.output_feat, p.n_stgcnn, p.n_txpcnn, 0};
    int q = d.K + 1;  // first layer: one input channel + the ones row
    if (d.n_st > 1 && d.S * d.K + 1 > q) q = d.S * d.K + 1;
    if (per_row) q = d.K * ((d.n_st > 1 ? d.S : 1) + 1);  // every time row keeps its own C_in + 1 contracted rows
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
            const int kv = src.key(vv);
            float s = 0.f;
            for (int w = 0; w < n; ++w) {
                const float dist = fabsf(uv - ur[w]);
                const float ainv = dist == 0.f ? 0.f : 1.0f / dist;
                s += (src.keep(w, kv) ? ainv : 0.f) + (w == vv ? 1.f : 0.f);
            }
            d[i] = 1.0f / sqrtf(s);
        }
        __syncthreads();
    }

    for (int l = 0; l < D.n_st; ++l) {
        const et_stgcnn_layer &Ly = p.st_gcns[l];
        const int Cin = l == 0 ? 1 : S;
        const float *xin = l == 0 ? u : x;
        if constexpr (Src::kPerRow) {
            // y[c,t,w] = sum_ci W[c,ci] P[t,ci,w] + b[c] P[t,C_in,w], P[t,j,w] = sum_v X_j[t,v] L[t,v,w] (ones row: j = C_in)
            const int J = Cin + 1;
            const int ngroups = (J + kSgGroup - 1) / kSgGroup;
            for (int it = tid; it < K * ngroups * n; it += kSgThreads) {
                const int w = it % n;
                const int rest = it / n;
                const int g = rest % ngroups, t = rest / ngroups;
                const int j0 = g * kSgGroup;
                const float uw = u[t * n + w], dw = d[t * n + w];
                const int kw = src.key(w);
                float acc[kSgGroup];
#pragma unroll
                for (int jj = 0; jj < kSgGroup; ++jj) acc[jj] = 0.f;
                for (int vv = 0; vv < n; ++vv) {
                    const float lv = src.lap(t, vv, w, n, u, d, uw, dw, kw);
#pragma unroll
                    for (int jj = 0; jj < kSgGroup; ++jj) {
                        const int j = j0 + jj;
                        if (j < J) acc[jj] = fmaf(j < J - 1 ? xin[(j * K + t) * n + vv] : 1.f, lv, acc[jj]);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < kSgGroup; ++jj)
                    if (j0 + jj < J) q[((int64_t)t * J + j0 + jj) * n + w] = acc[jj];
            }
            __syncthreads();
            for (int it = tid; it < S * K * n; it += kSgThreads) {
                const int w = it % n;
                const int ct = it / n;
                const int c = ct / K, t = ct - c * K;
                const float *qt = q + (int64_t)t * J * n;
                float acc = 0.f;
                for (int ci = 0; ci < Cin; ++ci) acc = fmaf(Ly.gcn_w[c * Cin + ci], qt[ci * n + w], acc);
                acc = fmaf(Ly.gcn_b[c], qt[(J - 1) * n + w], acc);
                y[it] = prelu(bn_eval(acc, Ly.bn1_w, Ly.bn1_b, Ly.bn1_mean, Ly.bn1_var, c, eps), Ly.prelu1);
            }
            __syncthreads();
        } else {
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
                    const int kw = src.key(w);
                    float acc[kSgGroup];
#pragma unroll
                    for (int jj = 0; jj < kSgGroup; ++jj) acc[jj] = 0.f;
                    for (int vv = 0; vv < n; ++vv) {
                        const float lv = src.lap(kk, vv, w, n, u, d, uw, dw, kw);
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

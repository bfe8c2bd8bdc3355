// et_sgcn_core.inl -- the layered SGCN kernels (header comment: et_sgcn.hip), one fragment #included by et_sgcn.hip and by
// et_gpgraph.hip inside their anonymous namespaces.  Every kernel is a template on GP:
//   GP = false  SGCN as baseline/sgcn runs it: one input channel, the scenes of `off`
//   GP = true   the base of GP-Graph-SGCN (baseline/gpgraphsgcn/model_baseline.py): the graph carries a position channel
//               next to the coefficient channel, the temporal attention reads both (six collapsed coefficients per head
//               instead of two), the spatial attention and the GCNs read the coefficient channel only, and the spatial
//               mask of the intra-group pass is multiplied by the same-group matrix.  The three passes of Sr real scenes
//               are 3 Sr *virtual scenes* of one call (pass m, scene s = virtual scene m Sr + s, rows m Nr + off[s] ..):
//               their node counts (the group count for the pooled pass) and stack offsets are read from device tables
//               that et_gpgraph.hip's group kernel writes.
// The GP = false instantiations keep the arithmetic they had before the template (the build sets -ffp-contract=off).
#include "et_scene_helpers.inl"

constexpr int kH = 4, kD = 16, kE = 64;
constexpr int kSnMaxT = ET_MAX_K + 2;
constexpr int kSnMaxS = 64;

struct Lay {  // workspace layout, in floats (vp, vn, gidx: GP only)
    int64_t hdr, sq, v, rs_s, rs_t, xa, xb, ta, tb, at, f2, f1, ts, vp, vn, gidx, total;
};

__host__ __device__ inline Lay lay_of(int T, int64_t N, int64_t n2, int64_t S, bool gp = false) {
    Lay L;
    L.hdr = 0;
    L.sq = 64;  // int64 [S]
    L.v = up4(L.sq + 2 * (S + 1));
    L.rs_s = up4(L.v + T * N);
    L.rs_t = up4(L.rs_s + 2 * (int64_t)T * kH * N);
    L.xa = up4(L.rs_t + 2 * (int64_t)T * kH * N);
    L.xb = up4(L.xa + (int64_t)T * kH * n2);
    L.ta = up4(L.xb + (int64_t)T * kH * n2);
    L.tb = up4(L.ta + N * kH * T * T);
    L.at = up4(L.tb + N * kH * T * T);
    L.f2 = up4(L.at + N * kH * T * T);
    L.f1 = up4(L.f2 + N * kH * T * kD);
    L.ts = up4(L.f1 + N * kH * T * kD);
    L.total = up4(L.ts + N * kH * T * kD);
    L.vp = L.vn = L.gidx = 0;
    if (gp) {  // the position channel (T, N), the virtual scenes' node counts int32 [S], the group index int32 [N / 3]
        L.vp = L.total;
        L.vn = up4(L.vp + T * N);
        L.gidx = up4(L.vn + S);
        L.total = up4(L.gidx + N / 3);
    }
    return L;
}

struct Ctx {
    const int32_t *off;  // scene offsets, or NULL: one scene of N rows (GP: of Nr rows)
    int64_t N, n2cap;    // GP: the virtual rows 3 Nr and 3 x the real scenes' squared sizes
    int S, T;            // GP: S = 3 Sr virtual scenes
    float *ws;
    Lay L;
    int64_t Nr;          // GP: the real rows and scenes
    int Sr;
};

// identities as handed over (graph form), or NULL: eye(n) / all ones (what the sgcn bridge builds); t NULL and t_t < 0:
// eye(T) (what GP-Graph's generate_identity_matrix builds)
struct Ident {
    const float *s, *t;
    int s_t, t_t;
};

__device__ __forceinline__ float ident_s(const Ident &I, int t, int i, int j, int n) {
    if (!I.s) return i == j ? 1.f : 0.f;
    return I.s[((int64_t)(I.s_t > 1 ? t : 0) * n + i) * n + j];
}

__device__ __forceinline__ float ident_t(const Ident &I, int i, int t, int u, int T) {
    if (!I.t) return I.t_t < 0 ? (t == u ? 1.f : 0.f) : 1.f;
    return I.t_t > 1 ? I.t[((int64_t)i * T + t) * T + u] : I.t[i];
}

template <bool GP>
__device__ __forceinline__ bool scene_at(const Ctx &c, int s, int64_t &b, int &n, int64_t &sq) {
    if constexpr (GP) {  // virtual scene s = pass m of real scene sr: rows m Nr + off[sr] .., node count from the table
        const int m = s / c.Sr, sr = s - m * c.Sr;
        const int64_t rb = c.off ? c.off[sr] : 0;
        const int64_t re = c.off ? c.off[sr + 1] : c.Nr;
        if (re <= rb) return false;
        sq = reinterpret_cast<const int64_t *>(c.ws + c.L.sq)[s];
        if (sq < 0) return false;
        n = reinterpret_cast<const int32_t *>(c.ws + c.L.vn)[s];
        b = (int64_t)m * c.Nr + rb;
        return n > 0 && n <= re - rb;
    } else {
        b = c.off ? c.off[s] : 0;
        const int64_t e = c.off ? c.off[s + 1] : c.N;
        if (e <= b) return false;
        sq = reinterpret_cast<const int64_t *>(c.ws + c.L.sq)[s];
        if (sq < 0) return false;
        n = (int)(e - b);
        return true;
    }
}

// one temporal softmax row (i, h, t): what multiplies the entries along u.  GP = false: the score of u is a x_u with
// a = x_t alpha + beta; GP = true: p_u a + c_u b with a, b affine in (p_t, c_t) -- hdr[8 + 4 q + h], q = 0..5
template <bool GP>
struct TRow {
    float a, b;
};

template <bool GP>
__device__ __forceinline__ TRow<GP> trow_of(const float *hdr, const float *v, const float *vp, int n, int t, int i, int h) {
    TRow<GP> r;
    if constexpr (GP) {
        const float pt = vp[t * n + i], ct = v[t * n + i];
        r.a = fmaf(pt, hdr[8 + h], fmaf(ct, hdr[12 + h], hdr[16 + h]));
        r.b = fmaf(pt, hdr[20 + h], fmaf(ct, hdr[24 + h], hdr[28 + h]));
    } else {
        r.a = fmaf(v[t * n + i], hdr[8 + h], hdr[12 + h]);
        r.b = 0.f;
    }
    return r;
}

template <bool GP>
__device__ __forceinline__ float tscore(const TRow<GP> &r, const float *v, const float *vp, int n, int u, int i) {
    if constexpr (GP)
        return fmaf(vp[u * n + i], r.a, v[u * n + i] * r.b);
    else
        return r.a * v[u * n + i];
}

__device__ __forceinline__ float dense(float ti, float xj, float m, float sum) { return expf(ti * xj - m) / sum; }
// where(sigmoid(l) > 0.5, sigmoid(l), 0) + identity
__device__ __forceinline__ float mask_of(float l, float ident) {
    const float sg = 1.0f / (1.0f + expf(-l));
    return (sg > 0.5f ? sg : 0.f) + ident;
}
__device__ __forceinline__ float zsm_num(float x) {
    const float e = expf(x) - 1.0f;
    return e * e;
}

// ---- prep: alpha / beta of the two attentions -> hdr[a * 8 + h], hdr[a * 8 + 4 + h]
// GP: the temporal embedding is (64, 2), column 0 the position p and column 1 the coefficient c (slot 1: c, slot 2: p).
// With x = (p, c): q_t . k_u = p_u (p_t aqp.akp + c_t aqc.akp + cq.akp) + c_u (p_t aqp.akc + c_t aqc.akc + cq.akc) + (terms
// constant along u) -> hdr[8 + 4 q + h], q = 0..5 in that order
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_prep(et_sgcn_params p, float *ws) {
    __shared__ double aq[3][kE], cq[3][kE], ak[3][kE];
    const int tid = threadIdx.x;
    if (tid < (GP ? 3 : 2) * kE) {
        const int slot = tid / kE, a = slot ? 1 : 0, c = tid % kE;
        const int stride = GP && a ? 2 : 1, col = GP && slot == 1 ? 1 : 0;
        const et_sgcn_attention &A = p.att[a];
        double s_aq = 0, s_cq = (double)A.q_b[c], s_ak = 0;
        for (int e = 0; e < kE; ++e) {
            const double we = A.emb_w[e * stride + col], be = A.emb_b[e];
            s_aq = fma((double)A.q_w[c * kE + e], we, s_aq);
            s_cq = fma((double)A.q_w[c * kE + e], be, s_cq);
            s_ak = fma((double)A.k_w[c * kE + e], we, s_ak);
        }
        aq[slot][c] = s_aq;
        cq[slot][c] = s_cq;
        ak[slot][c] = s_ak;
    }
    __syncthreads();
    auto dot = [&](const double *x, const double *y, int h) {
        double s = 0;
        for (int d = 0; d < kD; ++d) s = fma(x[h * kD + d], y[h * kD + d], s);
        return (float)(s * 0.125);  // / scaled_factor = sqrt(64)
    };
    if (tid < 2 * kH) {
        const int a = tid / kH, h = tid % kH;
        if (!GP || a == 0) {
            ws[a * 8 + h] = dot(aq[a], ak[a], h);
            ws[a * 8 + 4 + h] = dot(cq[a], ak[a], h);
        } else {
            ws[8 + h] = dot(aq[2], ak[2], h);
            ws[12 + h] = dot(aq[1], ak[2], h);
            ws[16 + h] = dot(cq[1], ak[2], h);
            ws[20 + h] = dot(aq[2], ak[1], h);
            ws[24 + h] = dot(aq[1], ak[1], h);
            ws[28 + h] = dot(cq[1], ak[1], h);
        }
    }
}

// ---- input: one workgroup per scene (GP: per virtual scene; its v and its table entries are the group kernel's)
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_input(Ctx c, const float *__restrict__ gv, const float *__restrict__ C_obs,
                                                         const float *__restrict__ nrm) {
    __shared__ int64_t part[kSnThreads];
    __shared__ float red[2 * kSnThreads / kWave];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int T = c.T;
    int64_t b, sq;
    int n;
    if constexpr (GP) {
        if (!scene_at<true>(c, s, b, n, sq)) return;
    } else {
        b = c.off ? c.off[s] : 0;
        const int64_t e = c.off ? c.off[s + 1] : c.N;
        if (e <= b) return;
        // the scene's offset into the stacks: the squared sizes of the scenes before it
        sq = scene_sq_before(c.off, s, part, INT64_MAX);
        const int64_t nn = e - b;
        const bool ok = nn <= ET_SGCN_MAX_N && sq + nn * nn <= c.n2cap;
        if (tid == 0) reinterpret_cast<int64_t *>(c.ws + c.L.sq)[s] = ok ? sq : -1;
        if (!ok) return;
        n = (int)nn;
        scene_v(c.ws + c.L.v + T * b, gv, C_obs, nrm, c.N, b, n, T, red);
        __syncthreads();
    }
    float *v = c.ws + c.L.v + T * b;
    const float *vp = c.ws + c.L.vp + T * b;
    // softmax rows: maximum and sum, spatial (t,h,i) over j and temporal (i,h,t) over u
    const float *hdr = c.ws + c.L.hdr;
    float *rs_s = c.ws + c.L.rs_s + 2 * (int64_t)T * kH * b;
    float *rs_t = c.ws + c.L.rs_t + 2 * (int64_t)T * kH * b;
    const int rows = T * kH * n;
    for (int r = tid; r < 2 * rows; r += kSnThreads) {
        const bool temporal = r >= rows;
        int t, h, i;
        if (!temporal) {
            i = r % n;
            h = (r / n) % kH;
            t = r / (n * kH);
        } else {
            const int q = r - rows;
            t = q % T;
            h = (q / T) % kH;
            i = q / (T * kH);
        }
        float *dst = temporal ? rs_t + 2 * (r - rows) : rs_s + 2 * r;
        float m = -INFINITY, sum = 0.f;
        if (GP && temporal) {
            const TRow<GP> tr = trow_of<GP>(hdr, v, vp, n, t, i, h);
            for (int u = 0; u < T; ++u) m = fmaxf(m, tscore<GP>(tr, v, vp, n, u, i));
            for (int u = 0; u < T; ++u) sum += expf(tscore<GP>(tr, v, vp, n, u, i) - m);
        } else {
            const float ti = fmaf(v[t * n + i], hdr[(temporal ? 8 : 0) + h], hdr[(temporal ? 8 : 0) + 4 + h]);
            const float *x = temporal ? v + i : v + t * n;
            const int len = temporal ? T : n, stride = temporal ? n : 1;
            for (int j = 0; j < len; ++j) m = fmaxf(m, ti * x[j * stride]);
            for (int j = 0; j < len; ++j) sum += expf(ti * x[j * stride] - m);
        }
        dst[0] = m;
        dst[1] = sum;
    }
}

// ---- fuse: spa_fusion (1x1 convolution over T, PReLU, + x) -> spatial stack; temporal stack = the attention
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_fuse(Ctx c, et_sgcn_params p) {
    int64_t b, sq;
    int n;
    if (!scene_at<GP>(c, blockIdx.x, b, n, sq)) return;
    const int T = c.T;
    const float *hdr = c.ws + c.L.hdr;
    const float *v = c.ws + c.L.v + T * b;
    const float *vp = c.ws + c.L.vp + T * b;
    const float *rs_s = c.ws + c.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *rs_t = c.ws + c.L.rs_t + 2 * (int64_t)T * kH * b;
    float *xa = c.ws + c.L.xa + (int64_t)T * kH * sq;
    float *ta = c.ws + c.L.ta + b * kH * T * T;
    const int64_t ns = (int64_t)kH * n * n, nt = (int64_t)n * kH * T * T;
    const float fa = p.fus_a[0];
    for (int64_t it = (int64_t)blockIdx.y * kSnThreads + threadIdx.x; it < ns + nt; it += (int64_t)gridDim.y * kSnThreads) {
        if (it < ns) {
            const int j = (int)(it % n), i = (int)((it / n) % n), h = (int)(it / ((int64_t)n * n));
            const float al = hdr[h], be = hdr[4 + h];
            float d[kSnMaxT];
#pragma unroll
            for (int t = 0; t < kSnMaxT; ++t) {
                d[t] = 0.f;
                if (t < T) {
                    const int r = (t * kH + h) * n + i;
                    d[t] = dense(fmaf(v[t * n + i], al, be), v[t * n + j], rs_s[2 * r], rs_s[2 * r + 1]);
                }
            }
            for (int u = 0; u < T; ++u) {
                float acc = p.fus_b[u], du = 0.f;
#pragma unroll
                for (int t = 0; t < kSnMaxT; ++t) {
                    if (t < T) {
                        acc = fmaf(p.fus_w[u * T + t], d[t], acc);
                        if (t == u) du = d[t];
                    }
                }
                xa[(((int64_t)u * kH + h) * n + i) * n + j] = prelu(acc, fa) + du;
            }
        } else {
            const int64_t q = it - ns;
            const int u = (int)(q % T), t = (int)((q / T) % T), h = (int)((q / (T * T)) % kH), i = (int)(q / (T * T * kH));
            const int r = (i * kH + h) * T + t;
            ta[q] = expf(tscore<GP>(trow_of<GP>(hdr, v, vp, n, t, i, h), v, vp, n, u, i) - rs_t[2 * r]) / rs_t[2 * r + 1];
        }
    }
}

// ---- asym: AsymmetricConvolution on (B,4,P,Q), entry `it` = (b,p,q): all four output channels
__device__ __forceinline__ void asym_entry(const float *__restrict__ in, float *__restrict__ out, int P, int Q, int64_t it,
                                           const et_sgcn_asym &A) {
    const int q = (int)(it % Q), pp = (int)((it / Q) % P);
    const int64_t bb = it / ((int64_t)P * Q);
    const float *x = in + bb * 4 * P * Q;
    float *y = out + bb * 4 * P * Q;
    float xc[4], xl[4], xr[4], xu[4], xd[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int64_t at = ((int64_t)ch * P + pp) * Q + q;
        xc[ch] = x[at];
        xl[ch] = q > 0 ? x[at - 1] : 0.f;
        xr[ch] = q + 1 < Q ? x[at + 1] : 0.f;
        xu[ch] = pp > 0 ? x[at - Q] : 0.f;
        xd[ch] = pp + 1 < P ? x[at + Q] : 0.f;
    }
    const float a = A.act[0];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float acc2 = A.conv2_b[o], acc1 = 0.f;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const float *w2 = A.conv2_w + (o * 4 + ch) * 3;  // (1,3): along q, with bias
            acc2 = fmaf(w2[0], xl[ch], acc2);
            acc2 = fmaf(w2[1], xc[ch], acc2);
            acc2 = fmaf(w2[2], xr[ch], acc2);
            const float *w1 = A.conv1_w + (o * 4 + ch) * 3;  // (3,1): along p, no bias
            acc1 = fmaf(w1[0], xu[ch], acc1);
            acc1 = fmaf(w1[1], xc[ch], acc1);
            acc1 = fmaf(w1[2], xd[ch], acc1);
        }
        y[((int64_t)o * P + pp) * Q + q] = prelu(acc2 + acc1, a) + xc[o];
    }
}

template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_asym(Ctx c, et_sgcn_asym As, et_sgcn_asym At, const float *in_s,
                                                        float *out_s, const float *in_t, float *out_t) {
    int64_t b, sq;
    int n;
    if (!scene_at<GP>(c, blockIdx.x, b, n, sq)) return;
    const int T = c.T;
    const int64_t os = (int64_t)T * kH * sq, ot = b * kH * T * T;
    const int64_t ns = (int64_t)T * n * n, nt = (int64_t)n * T * T;
    for (int64_t it = (int64_t)blockIdx.y * kSnThreads + threadIdx.x; it < ns + nt; it += (int64_t)gridDim.y * kSnThreads) {
        if (it < ns)
            asym_entry(in_s + os, out_s + os, n, n, it, As);
        else
            asym_entry(in_t + ot, out_t + ot, T, T, it - ns, At);
    }
}

// ---- tadj: temporal rows (i,h,t): mask, ZeroSoftmax -> A_t; temporal_spatial gcn 0 -> f2 (n,4,T,16)
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_tadj(Ctx c, et_sgcn_params p, Ident I, const float *__restrict__ lt) {
    int64_t b, sq;
    int n;
    if (!scene_at<GP>(c, blockIdx.x, b, n, sq)) return;
    const int T = c.T;
    const float *hdr = c.ws + c.L.hdr;
    const float *v = c.ws + c.L.v + T * b;
    const float *vp = c.ws + c.L.vp + T * b;
    const float *rs_t = c.ws + c.L.rs_t + 2 * (int64_t)T * kH * b;
    float *at = c.ws + c.L.at + b * kH * T * T;
    float *f2 = c.ws + c.L.f2 + b * kH * T * kD;
    const float *lg = lt + b * kH * T * T;
    const float a = p.gcn[2].act[0];
    const int rows = n * kH * T;
    for (int r = blockIdx.y * kSnThreads + threadIdx.x; r < rows; r += gridDim.y * kSnThreads) {
        const int t = r % T, h = (r / T) % kH, i = r / (T * kH);
        const TRow<GP> tr = trow_of<GP>(hdr, v, vp, n, t, i, h);
        const float m = rs_t[2 * r], sum = rs_t[2 * r + 1];
        float ssum = 0.f;
        for (int u = 0; u < T; ++u)
            ssum += zsm_num(expf(tscore<GP>(tr, v, vp, n, u, i) - m) / sum *
                            mask_of(lg[(int64_t)r * T + u], ident_t(I, i, t, u, T)));
        const float den = ssum + 1e-5f;
        float acc = 0.f;
        for (int u = 0; u < T; ++u) {
            const float xu = v[u * n + i];
            const float e = zsm_num(expf(tscore<GP>(tr, v, vp, n, u, i) - m) / sum *
                                    mask_of(lg[(int64_t)r * T + u], ident_t(I, i, t, u, T)));
            const float w = e / den;
            at[(int64_t)r * T + u] = w;
            acc = fmaf(w, xu, acc);
        }
        for (int d = 0; d < kD; ++d) f2[(int64_t)r * kD + d] = prelu(p.gcn[2].w[d] * acc, a);
    }
}

// ---- sadj: spatial rows (t,h,i): mask, ZeroSoftmax; spatial_temporal gcn 0 -> f1 (T,4,n,16); temporal_spatial gcn 1 ->
// ts (n,4,T,16)
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_sadj(Ctx c, et_sgcn_params p, Ident I, const float *__restrict__ ls) {
    int64_t b, sq;
    int n;
    if (!scene_at<GP>(c, blockIdx.x, b, n, sq)) return;
    const int T = c.T;
    // the intra-group pass (the third): the mask, identity added, times the same-group matrix
    const int32_t *grp = nullptr;
    if constexpr (GP)
        if ((int)blockIdx.x >= 2 * c.Sr) grp = reinterpret_cast<const int32_t *>(c.ws + c.L.gidx) + (b - 2 * c.Nr);
    const float *hdr = c.ws + c.L.hdr;
    const float *v = c.ws + c.L.v + T * b;
    const float *rs_s = c.ws + c.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *f2 = c.ws + c.L.f2 + b * kH * T * kD;
    float *f1 = c.ws + c.L.f1 + b * kH * T * kD;
    float *ts = c.ws + c.L.ts + b * kH * T * kD;
    const float *lg = ls + (int64_t)T * kH * sq;
    const float a0 = p.gcn[0].act[0], a3 = p.gcn[3].act[0];
    const int rows = T * kH * n;
    for (int r = blockIdx.y * kSnThreads + threadIdx.x; r < rows; r += gridDim.y * kSnThreads) {
        const int i = r % n, h = (r / n) % kH, t = r / (n * kH);
        const float ti = fmaf(v[t * n + i], hdr[h], hdr[4 + h]);
        const float m = rs_s[2 * r], sum = rs_s[2 * r + 1];
        const float *lrow = lg + (int64_t)r * n;
        float acc[kD];
#pragma unroll
        for (int d = 0; d < kD; ++d) acc[d] = 0.f;
        float ssum = 0.f, sx = 0.f;
        for (int j = 0; j < n; ++j) {
            const float xj = v[t * n + j];
            float mk = mask_of(lrow[j], ident_s(I, t, i, j, n));
            if constexpr (GP)
                if (grp) mk = mk * (grp[i] == grp[j] ? 1.f : 0.f);
            const float e = zsm_num(dense(ti, xj, m, sum) * mk);
            ssum += e;
            sx = fmaf(e, xj, sx);
            const float *fr = f2 + (((int64_t)j * kH + h) * T + t) * kD;
#pragma unroll
            for (int d = 0; d < kD; ++d) acc[d] = fmaf(e, fr[d], acc[d]);
        }
        const float den = ssum + 1e-5f;
        const float ax = sx / den;
#pragma unroll
        for (int d = 0; d < kD; ++d) {
            f1[(int64_t)r * kD + d] = prelu(p.gcn[0].w[d] * ax, a0);
            acc[d] = acc[d] / den;
        }
        float *dst = ts + (((int64_t)i * kH + h) * T + t) * kD;
        for (int d = 0; d < kD; ++d) {
            float o = 0.f;
#pragma unroll
            for (int q = 0; q < kD; ++q) o = fmaf(p.gcn[3].w[d * kD + q], acc[q], o);
            dst[d] = prelu(o, a3);
        }
    }
}

// ---- tail: one wavefront per pedestrian; lane = (h, d) of the (4,16) plane.  KEEP (the training forward,
// et_sgcn_train.inl): the same statements, and row r's activations are also stored at keep + r * tail_keep_floats(p)
__host__ __device__ inline int64_t tail_keep_floats(const et_sgcn_params &p) {
    return (int64_t)(2 * p.obs_len + 2 * p.n_tcn * p.pred_len) * kWave;
}

template <bool GP, bool KEEP = false>
__global__ __launch_bounds__(kWave) void sgcn_tail(Ctx c, et_sgcn_params p, float *__restrict__ out,
                                                   float *__restrict__ keep) {
    extern __shared__ float tail_lds[];  // two (T, 64) buffers
    float *bufA = tail_lds, *bufB = tail_lds + c.T * kWave;
    const int64_t r = blockIdx.x;
    const int l = threadIdx.x, h = l >> 4, d = l & 15;
    const int T = c.T, k = p.pred_len, S = p.out_dims;
    int s = 0;
    if constexpr (GP) {  // virtual row r = pass m, real row r - m Nr
        const int m = (int)(r / c.Nr);
        s = m * c.Sr + (c.off ? scene_of_row(c.off, c.Sr, r - (int64_t)m * c.Nr) : 0);
    } else {
        if (c.off) s = scene_of_row(c.off, c.S, r);
    }
    int64_t b, sq;
    int n;
    if (!scene_at<GP>(c, s, b, n, sq) || r < b || r >= b + n) {  // not computed: NaN, never an access outside the buffers
        if (l < S)
            for (int t = 0; t < k; ++t) out[((int64_t)t * c.N + r) * S + l] = __builtin_nanf("");
        return;
    }
    const int i = (int)(r - b);
    const float *at = c.ws + c.L.at + ((b + i) * kH + h) * T * T;
    const float *f1 = c.ws + c.L.f1 + b * kH * T * kD;
    const float *ts = c.ws + c.L.ts + ((b + i) * kH + h) * T * kD;
    // spatial_temporal gcn 1: A_t (T,T) of (i,h) times f1[:,h,i,:]
    for (int t = 0; t < T; ++t) {
        float g = 0.f;
        for (int u = 0; u < T; ++u) g = fmaf(at[t * T + u], f1[(((int64_t)u * kH + h) * n + i) * kD + d], g);
        bufA[t * kWave + l] = g;
    }
    __syncthreads();
    const float a1 = p.gcn[1].act[0];
    for (int t = 0; t < T; ++t) {
        float o = 0.f;
#pragma unroll
        for (int q = 0; q < kD; ++q) o = fmaf(p.gcn[1].w[d * kD + q], bufA[t * kWave + h * kD + q], o);
        bufB[t * kWave + l] = prelu(o, a1);
        if constexpr (KEEP) keep[r * tail_keep_floats(p) + t * kWave + l] = o;  // gcn 1 before its PReLU
    }
    __syncthreads();
    // fusion_ (1x1 over heads) of the spatial-temporal features + the temporal-spatial ones -> channels t, plane (h,d)
    for (int t = 0; t < T; ++t) {
        float o = 0.f;
#pragma unroll
        for (int g = 0; g < kH; ++g) o = fmaf(p.fusion_w[h * kH + g], bufB[t * kWave + g * kD + d], o);
        bufA[t * kWave + l] = o + ts[t * kD + d];
        if constexpr (KEEP) keep[r * tail_keep_floats(p) + (T + t) * kWave + l] = bufA[t * kWave + l];
    }
    __syncthreads();
    float *cur = bufA, *nxt = bufB;
    for (int j = 0; j < p.n_tcn; ++j) {  // tcns[0] without, tcns[j >= 1] with the residual
        const int Cin = j ? k : T;
        const float aj = p.tcn_a[j][0];
        // every output channel of this lane's position at once: k independent chains, the 9 taps read once per input
        // channel (each chain still runs input channel by input channel, tap by tap)
        float acc[ET_MAX_K];
#pragma unroll
        for (int o = 0; o < ET_MAX_K; ++o) acc[o] = o < k ? p.tcn_b[j][o] : 0.f;
        for (int ci = 0; ci < Cin; ++ci) {
            const float *pl = cur + ci * kWave;
            float x[9];
#pragma unroll
            for (int dh = 0; dh < 3; ++dh) {
#pragma unroll
                for (int dd = 0; dd < 3; ++dd) {
                    const int hh = h + dh - 1, d2 = d + dd - 1;
                    const bool in = hh >= 0 && hh < kH && d2 >= 0 && d2 < kD;
                    const float val = pl[in ? hh * kD + d2 : l];
                    x[dh * 3 + dd] = in ? val : 0.f;  // zero padding
                }
            }
#pragma unroll
            for (int o = 0; o < ET_MAX_K; ++o) {
                if (o < k) {
                    const float *w = p.tcn_w[j] + ((int64_t)o * Cin + ci) * 9;
#pragma unroll
                    for (int q = 0; q < 9; ++q) acc[o] = fmaf(w[q], x[q], acc[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < ET_MAX_K; ++o) {
            if (o < k) {
                float val = prelu(acc[o], aj);
                if (j) val += cur[o * kWave + l];
                nxt[o * kWave + l] = val;
                if constexpr (KEEP) {  // tcns[j] before its PReLU, then its output
                    float *kj = keep + r * tail_keep_floats(p) + (int64_t)(2 * T + 2 * j * k) * kWave;
                    kj[o * kWave + l] = acc[o];
                    kj[(k + o) * kWave + l] = val;
                }
            }
        }
        __syncthreads();
        float *tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    if (l < S) {  // output layer, mean over heads -> (k, N, S)
        float w[kD];
#pragma unroll
        for (int q = 0; q < kD; ++q) w[q] = p.out_w[l * kD + q];
        const float bias = p.out_b[l];
        for (int t = 0; t < k; ++t) {
            float tot = 0.f;
            for (int g = 0; g < kH; ++g) {
                float lin = bias;
#pragma unroll
                for (int q = 0; q < kD; ++q) lin = fmaf(w[q], cur[t * kWave + g * kD + q], lin);
                tot += lin;
            }
            out[((int64_t)t * c.N + r) * S + l] = tot * 0.25f;
        }
    }
}

static int check_params(const et_sgcn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->in_dims != 1 || p->num_heads != kH || p->embedding_dims != kE || p->dropout != 0.f || p->n_asym < 1 ||
        p->n_asym > ET_SGCN_MAX_LAYERS || p->n_tcn < 1 || p->n_tcn > ET_SGCN_MAX_LAYERS || p->pred_len < 1 ||
        p->pred_len > ET_MAX_K || p->obs_len != p->pred_len + 2 || p->out_dims < 1 || p->out_dims > kSnMaxS)
        return ET_ERR_UNSUPPORTED;
    for (int a = 0; a < 2; ++a) {
        const et_sgcn_attention &A = p->att[a];
        if (!A.emb_w || !A.emb_b || !A.q_w || !A.q_b || !A.k_w || !A.k_b) return ET_ERR_INVALID_ARG;
    }
    if (!p->fus_w || !p->fus_b || !p->fus_a || !p->fusion_w || !p->out_w || !p->out_b) return ET_ERR_INVALID_ARG;
    for (int j = 0; j < p->n_asym; ++j)
        for (const et_sgcn_asym *A : {&p->asym_s[j], &p->asym_t[j]})
            if (!A->conv1_w || !A->conv2_w || !A->conv2_b || !A->act) return ET_ERR_INVALID_ARG;
    for (int g = 0; g < 4; ++g)
        if (!p->gcn[g].w || !p->gcn[g].act) return ET_ERR_INVALID_ARG;
    for (int j = 0; j < p->n_tcn; ++j)
        if (!p->tcn_w[j] || !p->tcn_b[j] || !p->tcn_a[j]) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

// chunks per scene of the entry / row kernels: enough lanes for the largest scene, bounded over all scenes
static unsigned chunks(int64_t work_max, int n_scenes) {
    int64_t by = ceil_div(work_max, 4 * kSnThreads);
    const int64_t cap = 65536 / n_scenes > 8 ? 65536 / n_scenes : 8;
    if (by > cap) by = cap;
    if (by > 1024) by = 1024;
    return (unsigned)(by < 1 ? 1 : by);
}

// input .. tail on the c.S scenes of c (whoever calls has launched the prep, and for GP the group kernel): 5 +
// number_asymmetric_conv_layer launches.  out: (k, c.N, S).  keep (the training forward): layer j reads the
// stack at c.L.xa / c.L.ta + j x stride and writes the next one instead of the two ping-pong buffers, and the tail stores its
// activations at keep; the launches and their arithmetic are the same
template <bool GP>
static void run_layers(const et_sgcn_params &p, const Ctx &c, const float *gv, const Ident &I, const float *C_obs,
                       const float *nrm, int64_t max_n, float *out, float *logit_s, float *logit_t, hipStream_t st,
                       int64_t s_stride = 0, int64_t t_stride = 0, float *keep = nullptr) {
    const int T = c.T, n_scenes = c.S;
    const dim3 blk(kSnThreads);
    const unsigned S = (unsigned)n_scenes;
    hipLaunchKernelGGL(sgcn_input<GP>, dim3(S), blk, 0, st, c, gv, C_obs, nrm);
    const unsigned by_e = chunks((int64_t)T * kH * max_n * max_n + max_n * kH * T * T, n_scenes);
    const unsigned by_r = chunks((int64_t)T * kH * max_n * 4, n_scenes);
    hipLaunchKernelGGL(sgcn_fuse<GP>, dim3(S, by_e), blk, 0, st, c, p);
    float *xs[2] = {c.ws + c.L.xa, c.ws + c.L.xb}, *xt[2] = {c.ws + c.L.ta, c.ws + c.L.tb};
    const float *ls = xs[0], *lt = xt[0];
    for (int j = 0; j < p.n_asym; ++j) {
        const bool last = j + 1 == p.n_asym;
        float *os = keep ? xs[0] + (j + 1) * s_stride : last && logit_s ? logit_s : xs[(j + 1) & 1];
        float *ot = keep ? xt[0] + (j + 1) * t_stride : last && logit_t ? logit_t : xt[(j + 1) & 1];
        hipLaunchKernelGGL(sgcn_asym<GP>, dim3(S, by_e), blk, 0, st, c, p.asym_s[j], p.asym_t[j], ls, os, lt, ot);
        ls = os;
        lt = ot;
    }
    hipLaunchKernelGGL(sgcn_tadj<GP>, dim3(S, by_r), blk, 0, st, c, p, I, lt);
    hipLaunchKernelGGL(sgcn_sadj<GP>, dim3(S, by_r), blk, 0, st, c, p, I, ls);
    if (keep) {
        hipLaunchKernelGGL((sgcn_tail<GP, true>), dim3((unsigned)c.N), dim3(kWave), 2 * T * kWave * sizeof(float), st, c, p,
                           out, keep);
        return;
    }
    hipLaunchKernelGGL(sgcn_tail<GP>, dim3((unsigned)c.N), dim3(kWave), 2 * T * kWave * sizeof(float), st, c, p, out,
                       (float *)nullptr);
}

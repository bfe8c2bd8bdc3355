// et_sgcn_train.inl -- SGCN training for the one-channel family (include/eigentraj.h "SGCN predictor, training"): the
// training forward (the eval kernels of et_sgcn_core.inl on a layout that keeps every asymmetric layer's input and the
// tail's activations) and the backward pass with respect to every parameter.  #included by et_sgcn.hip after the core, and
// by et_gpgraph.hip: like the forward's, the kernels are templates on GP.  GP = true is the base of GP-Graph-SGCN on its
// 3 Sr virtual scenes (et_gpgraph_train.inl drives it): a pass has n_m nodes, the temporal score row carries six numbers per
// head and both channels, the spatial mask of the intra-group pass is multiplied by the same-group matrix, and the kernels
// also leave what the input gradient needs (d (A_s x) and d (A_t x) per row, A_s^T d (A_s x), the rows' sum dense d dense,
// d t_i, d a, d b).  The GP = false instantiations keep the arithmetic they had before the template.
//
// Backward, number_asymmetric_conv_layer + 8 launches for any number of scenes, in the order the gradient flows:
//   tail_bwd   per chunk of ET_SGCN_BWD_CHUNK pedestrians   output layer, tcns, fusion_, spatial_temporal gcn 1
//                                                            -> d ts, d f1, the tail's part of d A_t
//   sadj_bwd   per spatial row (t,h,i)   temporal_spatial gcn 1, spatial_temporal gcn 0, ZeroSoftmax, mask
//                                         -> d logit_s, the direct part of d dense_s, per row 1 / den and d (A_s f2)
//   sadj_f2    per (j,h,t)               d f2 = A_s^T d (A_s f2)  (a gather over the rows i; A_s is re-formed)
//   tadj_bwd   per temporal row (i,h,t)  temporal_spatial gcn 0, ZeroSoftmax, mask -> d logit_t, direct part of d dense_t
//   asym_bwd   x layers, last to first   both stacks; a position re-forms the pre-activation of its four neighbours
//   fuse_bwd   per entry (h,i,j)         spa_fusion -> d dense_s (in place of the direct part)
//   rows_bwd   per softmax row           d score -> the 16 numbers d alpha_h, d beta_h of both attentions
//   prep_bwd   1 workgroup, fp64         -> the 12 attention tensors (key.bias: an exact zero)
//   reduce     per gradient element      the fixed-order sum of the per-workgroup partials
// No atomics.  A kernel with weight gradients runs on a one-dimensional grid of *slots*: slot g is chunk c of scene s, found
// by walking the scenes (chunks of a compile-time number of items, ET_SGCN_BWD_*).  Inside a slot a thread sums its items
// ascending, the lanes of a wavefront are summed by a fixed butterfly, the wavefronts ascending; the tail sums its
// pedestrians ascending.  `reduce` sums the slots ascending, which is chunks ascending, then scenes ascending.  A slot
// without work stores zeros.
constexpr int kBwdChunk = ET_SGCN_BWD_CHUNK;   // pedestrians per tail slot
constexpr int kBwdRows = ET_SGCN_BWD_ROWS;     // softmax rows per slot
constexpr int kBwdItems = ET_SGCN_BWD_ITEMS;   // stack positions (asym) / entries (fuse) per slot
constexpr int kFuseTile = 128;
static_assert(kSnThreads == kD * kD, "tail_bwd and sadj_bwd give one thread to each element of a (16, 16) weight");
constexpr int kAsymG = 101;                    // conv1.weight 48, conv2.weight 48, conv2.bias 4, activation 1

struct TLay {  // training workspace, in floats.  L: the eval layout's names (xa / ta: stack 0)
    Lay L;
    int64_t xs, xs_stride, xt, xt_stride;  // n_asym + 1 kept stacks each
    int64_t keep;                          // tail activations, tail_keep_floats per row
    int64_t dat, df1, dts, df2, rrec;      // gradients of at / f1 / ts / f2; per spatial row 1 / den and d (A_s f2): 17
    int64_t gs, gt, dir_s, dir_t, dd_s;    // n_asym + 1 gradient stacks each (strides as xs / xt: d stack j is kept for the
                                           // tests' layer-by-layer check), the direct parts of d dense, d dense_s
    int64_t p_tail, p_sadj, p_tadj, p_asym_s, p_asym_t, p_fuse, p_rows;  // partials
    int64_t n_tail, n_rows, n_rows2, n_as, n_at, n_fuse;                 // slots
    int64_t g_tail;                                                       // floats of a tail partial block
    // GP (the base of GP-Graph-SGCN, three passes as virtual scenes): what the input gradient needs -- per spatial row
    // d (A_s x), per spatial row (sum dense d dense, d t_i), per temporal row (sum dense d dense, d a, d b), per temporal row
    // d (A_t x), A_s^T d (A_s x) per (j,h,t), and the input gradient itself, position and coefficient channel (T, n_m)
    int64_t dax, srec, trec, dacc_t, dx_as, dxp, dxv;
    int rows_g;                                                           // floats of a rows partial: 16, GP 32
    int64_t total;
};

__host__ __device__ inline int64_t tcn_floats(const et_sgcn_params &p, int j) {
    return (int64_t)p.pred_len * (j ? p.pred_len : p.obs_len) * 9 + p.pred_len + 1;
}

// the flat gradient buffer, in state_dict order
struct GLay {
    int64_t att[2], fus, asym_s, asym_t, gcn[4], fusion, tcn[ET_SGCN_MAX_LAYERS], out_w, out_b, total;
};

__host__ __device__ inline GLay glay_of(const et_sgcn_params &p, bool gp = false) {
    GLay G;
    const int T = p.obs_len;
    int64_t at = 0;
    for (int a = 0; a < 2; ++a) {
        G.att[a] = at;
        at += (gp && a ? 3 : 2) * kE + 2 * (kE * kE + kE);  // GP: the temporal embedding.weight is (64, 2)
    }
    G.fus = at;
    at += T * T + T + 1;
    G.asym_s = at;
    at += (int64_t)p.n_asym * kAsymG;
    G.asym_t = at;
    at += (int64_t)p.n_asym * kAsymG;
    for (int g = 0; g < 4; ++g) {
        G.gcn[g] = at;
        at += (g & 1 ? kD * kD : kD) + 1;
    }
    G.fusion = at;
    at += kH * kH;
    for (int j = 0; j < ET_SGCN_MAX_LAYERS; ++j) {
        G.tcn[j] = at;
        if (j < p.n_tcn) at += tcn_floats(p, j);
    }
    G.out_w = at;
    at += (int64_t)p.out_dims * kD;
    G.out_b = at;
    at += p.out_dims;
    G.total = at;
    return G;
}

__host__ __device__ inline TLay tlay_of(const et_sgcn_params &p, int64_t N, int64_t n2, int64_t S, bool gp = false) {
    TLay t;
    const int T = p.obs_len;
    t.L = lay_of(T, N, n2, S);  // (GP: N, n2, S count the virtual scenes' rows, entries and scenes)
    int64_t at = t.L.xa;
    auto take = [&](int64_t n) {
        const int64_t o = at;
        at = up4(at + n);
        return o;
    };
    const int64_t es = (int64_t)T * kH * n2, et = N * kH * T * T, ef = N * kH * T * kD;
    t.xs_stride = up4(es);
    t.xt_stride = up4(et);
    t.xs = take(t.xs_stride * (p.n_asym + 1));
    t.xt = take(t.xt_stride * (p.n_asym + 1));
    t.L.xa = t.xs;
    t.L.xb = t.xs + t.xs_stride;
    t.L.ta = t.xt;
    t.L.tb = t.xt + t.xt_stride;
    t.L.at = take(et);
    t.L.f2 = take(ef);
    t.L.f1 = take(ef);
    t.L.ts = take(ef);
    t.keep = take(N * tail_keep_floats(p));
    t.dat = take(et);
    t.df1 = take(ef);
    t.dts = take(ef);
    t.df2 = take(ef);
    t.rrec = take((int64_t)T * kH * N * 17);
    t.gs = take(t.xs_stride * (p.n_asym + 1));
    t.gt = take(t.xt_stride * (p.n_asym + 1));
    t.dir_s = take(es);
    t.dir_t = take(et);
    t.dd_s = take(es);
    t.g_tail = (kD * kD + 1) + kH * kH + (int64_t)p.out_dims * (kD + 1);
    for (int j = 0; j < p.n_tcn; ++j) t.g_tail += tcn_floats(p, j);
    t.n_tail = N / kBwdChunk + S;
    t.n_rows = (int64_t)T * kH * N / kBwdRows + S;
    t.n_rows2 = 2 * (int64_t)T * kH * N / kBwdRows + S;
    t.n_as = (int64_t)T * n2 / kBwdItems + S;
    t.n_at = N * T * T / kBwdItems + S;
    t.n_fuse = (int64_t)kH * n2 / kBwdItems + S;
    t.p_tail = take(t.n_tail * t.g_tail);
    t.p_sadj = take(t.n_rows * (kD + 1 + kD * kD + 1));
    t.p_tadj = take(t.n_rows * (kD + 1));
    t.p_asym_s = take(t.n_as * kAsymG * p.n_asym);
    t.p_asym_t = take(t.n_at * kAsymG * p.n_asym);
    t.p_fuse = take(t.n_fuse * (T * T + T + 1));
    t.rows_g = gp ? 32 : 16;
    t.p_rows = take(t.n_rows2 * t.rows_g);
    t.dax = t.srec = t.trec = t.dacc_t = t.dx_as = t.dxp = t.dxv = 0;
    if (gp) {
        t.L.vp = take(T * N);
        t.L.vn = take(S);
        t.L.gidx = take(N / 3);
        t.dax = take((int64_t)T * kH * N);
        t.srec = take(2 * (int64_t)T * kH * N);
        t.trec = take(3 * (int64_t)T * kH * N);
        t.dacc_t = take((int64_t)T * kH * N);
        t.dx_as = take((int64_t)T * kH * N);
        t.dxp = take(T * N);
        t.dxv = take(T * N);
        t.L.total = at;  // GP-Graph's wrapper values follow the base's training layout (wlay_of starts at L.total)
    }
    t.total = at;
    return t;
}

// slot g of a kernel whose scene of n pedestrians has work(n) items in chunks of `per`: -> scene, chunk (false: no work)
template <bool GP, class W>
__device__ __forceinline__ bool find_slot(const Ctx &c, int64_t g, int64_t per, W work, int64_t &chunk, int64_t &b, int &n,
                                          int64_t &sq, int *scene = nullptr) {
    for (int s = 0; s < c.S; ++s) {
        if (!scene_at<GP>(c, s, b, n, sq)) continue;
        const int64_t nch = ceil_div(work(n), per);
        if (g < nch) {
            chunk = g;
            if (scene) *scene = s;
            return true;
        }
        g -= nch;
    }
    return false;
}

__device__ __forceinline__ float wave_sum(float x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// the sum over the workgroup, wavefronts ascending (red: one float per wavefront); two barriers
__device__ __forceinline__ float block_sum(float x, float *red) {
    x = wave_sum(x);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = x;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < (int)blockDim.x / kWave; ++w) s += red[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ float sigmoid_of(float l) { return 1.0f / (1.0f + expf(-l)); }

// the spatial mask of entry (i, j), identity added; GP's intra-group pass (grp: the scene's group index, else NULL): times
// the same-group matrix, as sgcn_sadj forms it
template <bool GP>
__device__ __forceinline__ float smask_of(float l, float ident, const int32_t *grp, int i, int j) {
    float mk = mask_of(l, ident);
    if constexpr (GP)
        if (grp) mk = mk * (grp[i] == grp[j] ? 1.f : 0.f);
    return mk;
}

template <bool GP>
__device__ __forceinline__ const int32_t *group_index_of(const Ctx &c, int s, int64_t b) {
    if constexpr (GP)
        if (s >= 2 * c.Sr) return reinterpret_cast<const int32_t *>(c.ws + c.L.gidx) + (b - 2 * c.Nr);
    return nullptr;
}

// ---- tail backward
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_tail_bwd(Ctx c, TLay tl, et_sgcn_params p,
                                                            const float *__restrict__ dout) {
    __shared__ float sdo[ET_MAX_K * kSnMaxS];
    __shared__ float bA[kSnMaxT * kWave], bB[kSnMaxT * kWave], bC[kSnMaxT * kWave], bD[kSnMaxT * kWave];
    __shared__ float red[kSnThreads / kWave];
    const int tid = threadIdx.x;
    const int T = c.T, k = p.pred_len, S = p.out_dims, nt = p.n_tcn;
    float *part = c.ws + tl.p_tail + (int64_t)blockIdx.x * tl.g_tail;
    int64_t chunk, b, sq;
    int n;
    if (!find_slot<GP>(c, blockIdx.x, kBwdChunk, [](int m) { return (int64_t)m; }, chunk, b, n, sq)) {
        for (int64_t q = tid; q < tl.g_tail; q += kSnThreads) part[q] = 0.f;
        return;
    }
    // the block: gcn 1 (w 256, a 1), fusion_ 16, tcns j (w, b, a), output (w, b)
    const int64_t o_g1w = 0, o_g1a = kD * kD, o_fw = o_g1a + 1;
    int64_t o_tcn[ET_SGCN_MAX_LAYERS + 1];
    o_tcn[0] = o_fw + kH * kH;
    for (int j = 0; j < ET_SGCN_MAX_LAYERS; ++j) o_tcn[j + 1] = o_tcn[j] + (j < nt ? tcn_floats(p, j) : 0);
    const int64_t o_ow = o_tcn[nt], o_ob = o_ow + S * kD;
    const int64_t KS = tail_keep_floats(p);
    const int i0 = (int)chunk * kBwdChunk, i1 = i0 + kBwdChunk < n ? i0 + kBwdChunk : n;
    const float *f1 = c.ws + tl.L.f1 + b * kH * T * kD;
    for (int i = i0; i < i1; ++i) {
        const bool first = i == i0;
        auto put = [&](int64_t idx, float val) { part[idx] = first ? val : part[idx] + val; };
        const int64_t r = b + i;
        const float *keepr = c.ws + tl.keep + r * KS;
        for (int q = tid; q < k * S; q += kSnThreads) sdo[q] = dout[((int64_t)(q / S) * c.N + r) * S + q % S];
        const float *xN = keepr + (int64_t)(2 * T + (2 * (nt - 1) + 1) * k) * kWave;
        __syncthreads();
        for (int q = tid; q < S * kD; q += kSnThreads) {
            const int s = q / kD, qq = q % kD;
            float acc = 0.f;
            for (int t = 0; t < k; ++t) {
                const float g = 0.25f * sdo[t * S + s];
                for (int gg = 0; gg < kH; ++gg) acc = fmaf(g, xN[t * kWave + gg * kD + qq], acc);
            }
            put(o_ow + q, acc);
        }
        for (int s = tid; s < S; s += kSnThreads) {
            float acc = 0.f;
            for (int t = 0; t < k; ++t) acc += sdo[t * S + s];
            put(o_ob + s, acc);
        }
        for (int q = tid; q < k * kWave; q += kSnThreads) {
            const int t = q / kWave, qq = q & 15;
            float acc = 0.f;
            for (int s = 0; s < S; ++s) acc = fmaf(sdo[t * S + s], p.out_w[s * kD + qq], acc);
            bA[q] = 0.25f * acc;
        }
        __syncthreads();
        float *dx = bA, *dx2 = bB, *sx = bC, *sdz = bD;
        for (int j = nt - 1; j >= 0; --j) {
            const int Cin = j ? k : T;
            const float *zj = keepr + (int64_t)(2 * T + 2 * j * k) * kWave;
            const float *xj = j ? keepr + (int64_t)(2 * T + (2 * (j - 1) + 1) * k) * kWave : keepr + T * kWave;
            const float a = p.tcn_a[j][0];
            const int64_t o_w = o_tcn[j], o_b = o_w + (int64_t)k * Cin * 9, o_a = o_b + k;
            float la = 0.f;
            for (int q = tid; q < k * kWave; q += kSnThreads) {
                const float z = zj[q], g = dx[q];
                sdz[q] = z > 0.f ? g : a * g;
                la += z > 0.f ? 0.f : g * z;
            }
            for (int q = tid; q < Cin * kWave; q += kSnThreads) sx[q] = xj[q];
            const float sa = block_sum(la, red);
            if (tid == 0) put(o_a, sa);
            for (int q = tid; q < k * Cin * 9; q += kSnThreads) {
                const int o = q / (Cin * 9), ci = (q / 9) % Cin, tap = q % 9, dh = tap / 3, dd = tap % 3;
                float acc = 0.f;
                for (int l = 0; l < kWave; ++l) {
                    const int hh = (l >> 4) + dh - 1, d2 = (l & 15) + dd - 1;
                    if (hh >= 0 && hh < kH && d2 >= 0 && d2 < kD) acc = fmaf(sdz[o * kWave + l], sx[ci * kWave + hh * kD + d2], acc);
                }
                put(o_w + q, acc);
            }
            for (int o = tid; o < k; o += kSnThreads) {
                float acc = 0.f;
                for (int l = 0; l < kWave; ++l) acc += sdz[o * kWave + l];
                put(o_b + o, acc);
            }
            for (int q = tid; q < Cin * kWave; q += kSnThreads) {
                const int ci = q / kWave, l = q & (kWave - 1), h = l >> 4, d = l & 15;
                float acc = j ? dx[q] : 0.f;  // the residual of tcns[j >= 1]
                for (int o = 0; o < k; ++o) {
                    const float *w = p.tcn_w[j] + ((int64_t)o * Cin + ci) * 9;
                    for (int dh = 0; dh < 3; ++dh)
                        for (int dd = 0; dd < 3; ++dd) {
                            const int hh = h - dh + 1, d2 = d - dd + 1;
                            if (hh >= 0 && hh < kH && d2 >= 0 && d2 < kD)
                                acc = fmaf(w[dh * 3 + dd], sdz[o * kWave + hh * kD + d2], acc);
                        }
                }
                dx2[q] = acc;
            }
            __syncthreads();
            float *tmp = dx;
            dx = dx2;
            dx2 = tmp;
        }
        // dx: d (fusion_ st + ts), (T, 64)
        const float a1 = p.gcn[1].act[0];
        for (int q = tid; q < T * kWave; q += kSnThreads) {
            const int t = q / kWave, l = q & (kWave - 1), h = l >> 4, d = l & 15;
            c.ws[tl.dts + ((r * kH + h) * T + t) * kD + d] = dx[q];
            const float z = keepr[q];
            sdz[q] = z;
            sx[q] = prelu(z, a1);
        }
        __syncthreads();
        if (tid < kH * kH) {
            const int ho = tid / kH, g = tid % kH;
            float acc = 0.f;
            for (int t = 0; t < T; ++t)
                for (int d = 0; d < kD; ++d) acc = fmaf(dx[t * kWave + ho * kD + d], sx[t * kWave + g * kD + d], acc);
            put(o_fw + tid, acc);
        }
        for (int q = tid; q < T * kWave; q += kSnThreads) {
            const int t = q / kWave, l = q & (kWave - 1), g = l >> 4, d = l & 15;
            float acc = 0.f;
            for (int ho = 0; ho < kH; ++ho) acc = fmaf(p.fusion_w[ho * kH + g], dx[t * kWave + ho * kD + d], acc);
            dx2[q] = acc;
        }
        __syncthreads();
        float la = 0.f;
        for (int q = tid; q < T * kWave; q += kSnThreads) {
            const float z = sdz[q], g = dx2[q];
            dx[q] = z > 0.f ? g : a1 * g;
            la += z > 0.f ? 0.f : g * z;
        }
        const float sa1 = block_sum(la, red);
        if (tid == 0) put(o_g1a, sa1);
        const float *at_i = c.ws + tl.L.at + r * kH * T * T;
        for (int q = tid; q < T * kWave; q += kSnThreads) {  // A_t f1, as the forward forms it
            const int t = q / kWave, l = q & (kWave - 1), h = l >> 4, d = l & 15;
            float g = 0.f;
            for (int u = 0; u < T; ++u) g = fmaf(at_i[(h * T + t) * T + u], f1[(((int64_t)u * kH + h) * n + i) * kD + d], g);
            sx[q] = g;
        }
        __syncthreads();
        {
            const int d = tid / kD, qq = tid % kD;
            float acc = 0.f;
            for (int t = 0; t < T; ++t)
                for (int h = 0; h < kH; ++h) acc = fmaf(dx[t * kWave + h * kD + d], sx[t * kWave + h * kD + qq], acc);
            put(o_g1w + tid, acc);
        }
        for (int q = tid; q < T * kWave; q += kSnThreads) {
            const int t = q / kWave, l = q & (kWave - 1), h = l >> 4, qq = l & 15;
            float acc = 0.f;
            for (int d = 0; d < kD; ++d) acc = fmaf(p.gcn[1].w[d * kD + qq], dx[t * kWave + h * kD + d], acc);
            dx2[q] = acc;
        }
        __syncthreads();
        for (int q = tid; q < kH * T * T; q += kSnThreads) {
            const int u = q % T, t = (q / T) % T, h = q / (T * T);
            float acc = 0.f;
            for (int d = 0; d < kD; ++d) acc = fmaf(dx2[t * kWave + h * kD + d], f1[(((int64_t)u * kH + h) * n + i) * kD + d], acc);
            c.ws[tl.dat + r * kH * T * T + q] = acc;
        }
        for (int q = tid; q < T * kWave; q += kSnThreads) {
            const int u = q / kWave, l = q & (kWave - 1), h = l >> 4, d = l & 15;
            float acc = 0.f;
            for (int t = 0; t < T; ++t) acc = fmaf(at_i[(h * T + t) * T + u], dx2[t * kWave + l], acc);
            c.ws[tl.df1 + b * kH * T * kD + (((int64_t)u * kH + h) * n + i) * kD + d] = acc;
        }
        __syncthreads();
    }
}

// ZeroSoftmax and mask backward of one entry: dense dn, mask mk (identity included), logit l, d e -> the direct part of
// d dense and d logit
__device__ __forceinline__ void zsm_entry_bwd(float dn, float mk, float l, float de, float &direct, float &dlogit) {
    const float ex = expf(dn * mk);
    const float dx = de * (2.0f * (ex - 1.0f) * ex);
    direct = mk * dx;
    const float sg = sigmoid_of(l);
    dlogit = sg > 0.5f ? dn * dx * (sg * (1.0f - sg)) : 0.f;
}

// ---- sadj backward: spatial rows (t,h,i)
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_sadj_bwd(Ctx c, TLay tl, et_sgcn_params p, Ident I,
                                                            const float *__restrict__ ls, float *__restrict__ gout) {
    __shared__ float s_dz[kD * kSnThreads], s_ac[kD * kSnThreads];
    __shared__ float red[(kSnThreads / kWave) * (kD + 2)];
    const int tid = threadIdx.x, T = c.T;
    constexpr int G = kD + 1 + kD * kD + 1;  // gcn 0 (w 16, a), gcn 3 (w 256, a)
    float *part = c.ws + tl.p_sadj + (int64_t)blockIdx.x * G;
    int64_t chunk, b, sq;
    int n;
    int scene = 0;
    if (!find_slot<GP>(c, blockIdx.x, kBwdRows, [T](int m) { return (int64_t)T * kH * m; }, chunk, b, n, sq, &scene)) {
        for (int q = tid; q < G; q += kSnThreads) part[q] = 0.f;
        return;
    }
    const int32_t *grp = group_index_of<GP>(c, scene, b);
    const float *hdr = c.ws + tl.L.hdr;
    const float *v = c.ws + tl.L.v + T * b;
    const float *rs_s = c.ws + tl.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *f2 = c.ws + tl.L.f2 + b * kH * T * kD;
    const float *lg = ls + (int64_t)T * kH * sq;
    float *gl = gout + (int64_t)T * kH * sq, *dir = c.ws + tl.dir_s + (int64_t)T * kH * sq;
    const float a0 = p.gcn[0].act[0], a3 = p.gcn[3].act[0];
    const int rows = T * kH * n;
    const int r0 = (int)chunk * kBwdRows, r1 = r0 + kBwdRows < rows ? r0 + kBwdRows : rows;
    float gw0[kD], ga0 = 0.f, ga3 = 0.f, gw3 = 0.f;
#pragma unroll
    for (int d = 0; d < kD; ++d) gw0[d] = 0.f;
    for (int rb = r0; rb < r1; rb += kSnThreads) {  // one row per thread, then the 256 rows' part of d gcn[3].w
        const int r = rb + tid;
        float dzo[kD], accn[kD];
#pragma unroll
        for (int d = 0; d < kD; ++d) dzo[d] = accn[d] = 0.f;
        if (r < r1) {
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
                const float e = zsm_num(dense(ti, xj, m, sum) * smask_of<GP>(lrow[j], ident_s(I, t, i, j, n), grp, i, j));
                ssum += e;
                sx = fmaf(e, xj, sx);
                const float *fr = f2 + (((int64_t)j * kH + h) * T + t) * kD;
#pragma unroll
                for (int d = 0; d < kD; ++d) acc[d] = fmaf(e, fr[d], acc[d]);
            }
            const float den = ssum + 1e-5f;
            const float ax = sx / den;
            const float *g1 = c.ws + tl.df1 + b * kH * T * kD + (int64_t)r * kD;
            float dax = 0.f;
#pragma unroll
            for (int d = 0; d < kD; ++d) {
                accn[d] = acc[d] / den;
                const float w = p.gcn[0].w[d], z = w * ax, g = g1[d];
                const float dz = z > 0.f ? g : a0 * g;
                ga0 += z > 0.f ? 0.f : g * z;
                gw0[d] = fmaf(dz, ax, gw0[d]);
                dax = fmaf(dz, w, dax);
            }
            const float *g3 = c.ws + tl.dts + (((b + i) * kH + h) * T + t) * kD;
            for (int d = 0; d < kD; ++d) {
                float o = 0.f;
#pragma unroll
                for (int q = 0; q < kD; ++q) o = fmaf(p.gcn[3].w[d * kD + q], accn[q], o);
                const float g = g3[d];
                dzo[d] = o > 0.f ? g : a3 * g;
                ga3 += o > 0.f ? 0.f : g * o;
            }
            float dacc[kD];
#pragma unroll
            for (int q = 0; q < kD; ++q) {
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < kD; ++d) s = fmaf(p.gcn[3].w[d * kD + q], dzo[d], s);
                dacc[q] = s;
            }
            float *rec = c.ws + tl.rrec + ((int64_t)T * kH * b + r) * 17;
            rec[0] = den;
#pragma unroll
            for (int q = 0; q < kD; ++q) rec[1 + q] = dacc[q];
            if constexpr (GP) c.ws[tl.dax + (int64_t)T * kH * b + r] = dax;
            // d A_s[j] = dax x_j + dacc . f2[j].  d e[j] = (d A_s[j] - sum_j' d A_s[j'] A_s[j']) / den, formed around c0 = d A_s[0]
            // (sum A_s = 1 - 1e-5 / den): the plain form cancels where one entry carries the row, exactly so in a scene of one
            float sdy = 0.f, c0 = 0.f;
            for (int j = 0; j < n; ++j) {
                const float xj = v[t * n + j];
                const float e = zsm_num(dense(ti, xj, m, sum) * smask_of<GP>(lrow[j], ident_s(I, t, i, j, n), grp, i, j));
                const float *fr = f2 + (((int64_t)j * kH + h) * T + t) * kD;
                float dy = dax * xj;
#pragma unroll
                for (int d = 0; d < kD; ++d) dy = fmaf(dacc[d], fr[d], dy);
                if (j == 0) c0 = dy;
                sdy = fmaf(dy - c0, e / den, sdy);
            }
            const float tail0 = c0 * (1e-5f / den);
            for (int j = 0; j < n; ++j) {
                const float xj = v[t * n + j];
                const float dn = dense(ti, xj, m, sum), mk = smask_of<GP>(lrow[j], ident_s(I, t, i, j, n), grp, i, j);
                const float *fr = f2 + (((int64_t)j * kH + h) * T + t) * kD;
                float dy = dax * xj;
#pragma unroll
                for (int d = 0; d < kD; ++d) dy = fmaf(dacc[d], fr[d], dy);
                float direct, dl;
                zsm_entry_bwd(dn, mk, lrow[j], ((dy - c0) - sdy + tail0) / den, direct, dl);
                dir[(int64_t)r * n + j] = direct;
                gl[(int64_t)r * n + j] = dl;
            }
        }
#pragma unroll
        for (int d = 0; d < kD; ++d) {
            s_dz[d * kSnThreads + tid] = dzo[d];
            s_ac[d * kSnThreads + tid] = accn[d];
        }
        __syncthreads();
        {
            const int d = tid / kD, q = tid % kD;
            for (int e = 0; e < kSnThreads; ++e) gw3 = fmaf(s_dz[d * kSnThreads + e], s_ac[q * kSnThreads + e], gw3);
        }
        __syncthreads();
    }
    part[kD + 1 + tid] = gw3;
    const int wv = tid / kWave;
#pragma unroll
    for (int d = 0; d < kD; ++d) {
        const float s = wave_sum(gw0[d]);
        if ((tid & (kWave - 1)) == 0) red[wv * (kD + 2) + d] = s;
    }
    {
        const float s0 = wave_sum(ga0), s3 = wave_sum(ga3);
        if ((tid & (kWave - 1)) == 0) {
            red[wv * (kD + 2) + kD] = s0;
            red[wv * (kD + 2) + kD + 1] = s3;
        }
    }
    __syncthreads();
    if (tid < kD + 2) {
        float s = 0.f;
        for (int w = 0; w < kSnThreads / kWave; ++w) s += red[w * (kD + 2) + tid];
        part[tid <= kD ? tid : kD + 1 + kD * kD] = s;
    }
}

// ---- d f2 (n,4,T,16): entry (j,h,t) gathers A_s[t,h,i,j] d (A_s f2)[t,h,i,:] over i ascending
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_sadj_f2(Ctx c, TLay tl, Ident I, const float *__restrict__ ls) {
    int64_t b, sq;
    int n;
    if (!scene_at<GP>(c, blockIdx.x, b, n, sq)) return;
    const int T = c.T;
    const int32_t *grp = group_index_of<GP>(c, blockIdx.x, b);
    const float *hdr = c.ws + tl.L.hdr;
    const float *v = c.ws + tl.L.v + T * b;
    const float *rs_s = c.ws + tl.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *lg = ls + (int64_t)T * kH * sq;
    const float *rrec = c.ws + tl.rrec + (int64_t)T * kH * b * 17;
    const float *daxr = c.ws + tl.dax + (int64_t)T * kH * b;  // GP: d (A_s x) per row, for the input gradient
    float *df2 = c.ws + tl.df2 + b * kH * T * kD;
    const int items = n * kH * T;
    for (int it = blockIdx.y * kSnThreads + threadIdx.x; it < items; it += gridDim.y * kSnThreads) {
        const int t = it % T, h = (it / T) % kH, j = it / (T * kH);
        const float xj = v[t * n + j];
        float acc[kD], ax = 0.f;
#pragma unroll
        for (int d = 0; d < kD; ++d) acc[d] = 0.f;
        for (int i = 0; i < n; ++i) {
            const int r = (t * kH + h) * n + i;
            const float ti = fmaf(v[t * n + i], hdr[h], hdr[4 + h]);
            const float e = zsm_num(dense(ti, xj, rs_s[2 * r], rs_s[2 * r + 1]) *
                                    smask_of<GP>(lg[(int64_t)r * n + j], ident_s(I, t, i, j, n), grp, i, j));
            const float *rec = rrec + (int64_t)r * 17;
            const float y = e / rec[0];
#pragma unroll
            for (int d = 0; d < kD; ++d) acc[d] = fmaf(y, rec[1 + d], acc[d]);
            if constexpr (GP) ax = fmaf(y, daxr[r], ax);
        }
#pragma unroll
        for (int d = 0; d < kD; ++d) df2[(int64_t)it * kD + d] = acc[d];
        if constexpr (GP) c.ws[tl.dx_as + b * kH * T + it] = ax;  // A_s^T d (A_s x) at (j,h,t)
    }
}

// ---- tadj backward: temporal rows (i,h,t)
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_tadj_bwd(Ctx c, TLay tl, et_sgcn_params p, Ident I,
                                                            const float *__restrict__ lt, float *__restrict__ gout) {
    __shared__ float red[(kSnThreads / kWave) * (kD + 1)];
    const int tid = threadIdx.x, T = c.T;
    constexpr int G = kD + 1;
    float *part = c.ws + tl.p_tadj + (int64_t)blockIdx.x * G;
    int64_t chunk, b, sq;
    int n;
    if (!find_slot<GP>(c, blockIdx.x, kBwdRows, [T](int m) { return (int64_t)T * kH * m; }, chunk, b, n, sq)) {
        if (tid < G) part[tid] = 0.f;
        return;
    }
    const float *hdr = c.ws + tl.L.hdr;
    const float *v = c.ws + tl.L.v + T * b;
    const float *vp = c.ws + tl.L.vp + T * b;  // (GP only)
    const float *rs_t = c.ws + tl.L.rs_t + 2 * (int64_t)T * kH * b;
    const float *lg = lt + b * kH * T * T;
    const float *dat = c.ws + tl.dat + b * kH * T * T;
    const float *df2 = c.ws + tl.df2 + b * kH * T * kD;
    float *gl = gout + b * kH * T * T, *dir = c.ws + tl.dir_t + b * kH * T * T;
    const float a2 = p.gcn[2].act[0];
    const int rows = n * kH * T;
    const int r0 = (int)chunk * kBwdRows, r1 = r0 + kBwdRows < rows ? r0 + kBwdRows : rows;
    float gw[kD], ga = 0.f;
#pragma unroll
    for (int d = 0; d < kD; ++d) gw[d] = 0.f;
    for (int r = r0 + tid; r < r1; r += kSnThreads) {
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
            const float e = zsm_num(expf(tscore<GP>(tr, v, vp, n, u, i) - m) / sum *
                                    mask_of(lg[(int64_t)r * T + u], ident_t(I, i, t, u, T)));
            acc = fmaf(e / den, v[u * n + i], acc);
        }
        float dacc = 0.f;
#pragma unroll
        for (int d = 0; d < kD; ++d) {
            const float w = p.gcn[2].w[d], z = w * acc, g = df2[(int64_t)r * kD + d];
            const float dz = z > 0.f ? g : a2 * g;
            ga += z > 0.f ? 0.f : g * z;
            gw[d] = fmaf(dz, acc, gw[d]);
            dacc = fmaf(dz, w, dacc);
        }
        if constexpr (GP) c.ws[tl.dacc_t + b * kH * T + r] = dacc;
        float sdy = 0.f, c0 = 0.f;  // around c0 = d A_t[0], as in sgcn_sadj_bwd
        for (int u = 0; u < T; ++u) {
            const float e = zsm_num(expf(tscore<GP>(tr, v, vp, n, u, i) - m) / sum *
                                    mask_of(lg[(int64_t)r * T + u], ident_t(I, i, t, u, T)));
            const float dy = fmaf(dacc, v[u * n + i], dat[(int64_t)r * T + u]);
            if (u == 0) c0 = dy;
            sdy = fmaf(dy - c0, e / den, sdy);
        }
        const float tail0 = c0 * (1e-5f / den);
        for (int u = 0; u < T; ++u) {
            const float dn = expf(tscore<GP>(tr, v, vp, n, u, i) - m) / sum;
            const float l = lg[(int64_t)r * T + u], mk = mask_of(l, ident_t(I, i, t, u, T));
            const float dy = fmaf(dacc, v[u * n + i], dat[(int64_t)r * T + u]);
            float direct, dl;
            zsm_entry_bwd(dn, mk, l, ((dy - c0) - sdy + tail0) / den, direct, dl);
            dir[(int64_t)r * T + u] = direct;
            gl[(int64_t)r * T + u] = dl;
        }
    }
    const int wv = tid / kWave;
#pragma unroll
    for (int d = 0; d < kD; ++d) {
        const float s = wave_sum(gw[d]);
        if ((tid & (kWave - 1)) == 0) red[wv * G + d] = s;
    }
    {
        const float s = wave_sum(ga);
        if ((tid & (kWave - 1)) == 0) red[wv * G + kD] = s;
    }
    __syncthreads();
    if (tid < G) {
        float s = 0.f;
        for (int w = 0; w < kSnThreads / kWave; ++w) s += red[w * G + tid];
        part[tid] = s;
    }
}

// ---- asym backward.  d pre-activation of position (pp, q) of block x / gradient block g, all four channels (zero outside)
__device__ __forceinline__ void asym_dz(const float *__restrict__ x, const float *__restrict__ g, int P, int Q, int pp, int q,
                                        const et_sgcn_asym &A, float a, float dz[4], float xc[4], float xl[4], float xr[4],
                                        float xu[4], float xd[4], float z[4], float gc[4]) {
    if (pp < 0 || pp >= P || q < 0 || q >= Q) {
#pragma unroll
        for (int o = 0; o < 4; ++o) dz[o] = 0.f;
        return;
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int64_t at = ((int64_t)ch * P + pp) * Q + q;
        xc[ch] = x[at];
        xl[ch] = q > 0 ? x[at - 1] : 0.f;
        xr[ch] = q + 1 < Q ? x[at + 1] : 0.f;
        xu[ch] = pp > 0 ? x[at - Q] : 0.f;
        xd[ch] = pp + 1 < P ? x[at + Q] : 0.f;
        gc[ch] = g[at];
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float acc2 = A.conv2_b[o], acc1 = 0.f;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const float *w2 = A.conv2_w + (o * 4 + ch) * 3;
            acc2 = fmaf(w2[0], xl[ch], acc2);
            acc2 = fmaf(w2[1], xc[ch], acc2);
            acc2 = fmaf(w2[2], xr[ch], acc2);
            const float *w1 = A.conv1_w + (o * 4 + ch) * 3;
            acc1 = fmaf(w1[0], xu[ch], acc1);
            acc1 = fmaf(w1[1], xc[ch], acc1);
            acc1 = fmaf(w1[2], xd[ch], acc1);
        }
        z[o] = acc2 + acc1;
        dz[o] = z[o] > 0.f ? gc[o] : a * gc[o];
    }
}

template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_asym_bwd(Ctx c, TLay tl, et_sgcn_asym As, et_sgcn_asym At, int layer,
                                                            const float *in_s, const float *g_s, float *o_s,
                                                            const float *in_t, const float *g_t, float *o_t) {
    __shared__ float red[(kSnThreads / kWave) * kAsymG];
    const int tid = threadIdx.x, T = c.T;
    const bool spatial = (int64_t)blockIdx.x < tl.n_as;
    const int64_t slot = spatial ? blockIdx.x : blockIdx.x - tl.n_as;
    float *part = c.ws + (spatial ? tl.p_asym_s + ((int64_t)layer * tl.n_as + slot) * kAsymG
                                  : tl.p_asym_t + ((int64_t)layer * tl.n_at + slot) * kAsymG);
    int64_t chunk, b, sq;
    int n;
    const bool found = spatial ? find_slot<GP>(c, slot, kBwdItems, [T](int m) { return (int64_t)T * m * m; }, chunk, b, n, sq)
                               : find_slot<GP>(c, slot, kBwdItems, [T](int m) { return (int64_t)m * T * T; }, chunk, b, n, sq);
    if (!found) {
        if (tid < kAsymG) part[tid] = 0.f;
        return;
    }
    const et_sgcn_asym &A = spatial ? As : At;
    const int P = spatial ? n : T, Q = P;
    const int64_t base = spatial ? (int64_t)T * kH * sq : b * kH * T * T;
    const float *in = (spatial ? in_s : in_t) + base, *gg = (spatial ? g_s : g_t) + base;
    float *out = (spatial ? o_s : o_t) + base;
    const int64_t items = spatial ? (int64_t)T * n * n : (int64_t)n * T * T;
    const int64_t i0 = chunk * kBwdItems, i1 = i0 + kBwdItems < items ? i0 + kBwdItems : items;
    const float a = A.act[0];
    float acc[kAsymG];
#pragma unroll
    for (int e = 0; e < kAsymG; ++e) acc[e] = 0.f;
    for (int64_t it = i0 + tid; it < i1; it += kSnThreads) {
        const int q = (int)(it % Q), pp = (int)((it / Q) % P);
        const int64_t bb = it / ((int64_t)P * Q);
        const float *x = in + bb * 4 * P * Q, *g = gg + bb * 4 * P * Q;
        float xc[4], xl[4], xr[4], xu[4], xd[4], z[4], gc[4], dzc[4];
        float t0[4], t1[4], t2[4], t3[4], t4[4], t5[4], t6[4];
        float dzl[4], dzr[4], dzu[4], dzd[4];
        asym_dz(x, g, P, Q, pp, q, A, a, dzc, xc, xl, xr, xu, xd, z, gc);
        asym_dz(x, g, P, Q, pp, q - 1, A, a, dzl, t0, t1, t2, t3, t4, t5, t6);
        asym_dz(x, g, P, Q, pp, q + 1, A, a, dzr, t0, t1, t2, t3, t4, t5, t6);
        asym_dz(x, g, P, Q, pp - 1, q, A, a, dzu, t0, t1, t2, t3, t4, t5, t6);
        asym_dz(x, g, P, Q, pp + 1, q, A, a, dzd, t0, t1, t2, t3, t4, t5, t6);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            float d = gc[ch];  // the shortcut
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const float *w2 = A.conv2_w + (o * 4 + ch) * 3, *w1 = A.conv1_w + (o * 4 + ch) * 3;
                d = fmaf(w2[0], dzr[o], d);
                d = fmaf(w2[1], dzc[o], d);
                d = fmaf(w2[2], dzl[o], d);
                d = fmaf(w1[0], dzd[o], d);
                d = fmaf(w1[1], dzc[o], d);
                d = fmaf(w1[2], dzu[o], d);
            }
            out[bb * 4 * P * Q + ((int64_t)ch * P + pp) * Q + q] = d;
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const int e = (o * 4 + ch) * 3;
                acc[e] = fmaf(dzc[o], xu[ch], acc[e]);
                acc[e + 1] = fmaf(dzc[o], xc[ch], acc[e + 1]);
                acc[e + 2] = fmaf(dzc[o], xd[ch], acc[e + 2]);
                acc[48 + e] = fmaf(dzc[o], xl[ch], acc[48 + e]);
                acc[48 + e + 1] = fmaf(dzc[o], xc[ch], acc[48 + e + 1]);
                acc[48 + e + 2] = fmaf(dzc[o], xr[ch], acc[48 + e + 2]);
            }
            acc[96 + o] += dzc[o];
            acc[100] += z[o] > 0.f ? 0.f : gc[o] * z[o];
        }
    }
    const int wv = tid / kWave;
#pragma unroll
    for (int e = 0; e < kAsymG; ++e) {
        const float s = wave_sum(acc[e]);
        if ((tid & (kWave - 1)) == 0) red[wv * kAsymG + e] = s;
    }
    __syncthreads();
    if (tid < kAsymG) {
        float s = 0.f;
        for (int w = 0; w < kSnThreads / kWave; ++w) s += red[w * kAsymG + tid];
        part[tid] = s;
    }
}

// ---- fuse backward: entries (h,i,j) in tiles of kFuseTile, one thread per entry; then a thread owns pairs (u,t) of d fus_w
template <bool GP>
__global__ __launch_bounds__(kFuseTile) void sgcn_fuse_bwd(Ctx c, TLay tl, et_sgcn_params p, const float *__restrict__ g0) {
    __shared__ float s_d[kSnMaxT * kFuseTile], s_da[kSnMaxT * kFuseTile];
    __shared__ float red[kFuseTile / kWave];
    constexpr int kPairs = (kSnMaxT * kSnMaxT + kFuseTile - 1) / kFuseTile;
    const int tid = threadIdx.x, T = c.T;
    const int G = T * T + T + 1;
    float *part = c.ws + tl.p_fuse + (int64_t)blockIdx.x * G;
    int64_t chunk, b, sq;
    int n;
    if (!find_slot<GP>(c, blockIdx.x, kBwdItems, [](int m) { return (int64_t)kH * m * m; }, chunk, b, n, sq)) {
        for (int q = tid; q < G; q += kFuseTile) part[q] = 0.f;
        return;
    }
    const float *hdr = c.ws + tl.L.hdr;
    const float *v = c.ws + tl.L.v + T * b;
    const float *rs_s = c.ws + tl.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *g = g0 + (int64_t)T * kH * sq;
    const float *dir = c.ws + tl.dir_s + (int64_t)T * kH * sq;
    float *dds = c.ws + tl.dd_s + (int64_t)T * kH * sq;
    const int64_t items = (int64_t)kH * n * n;
    const int64_t i0 = chunk * kBwdItems, i1 = i0 + kBwdItems < items ? i0 + kBwdItems : items;
    const float fa = p.fus_a[0];
    float wacc[kPairs], bacc = 0.f, la = 0.f;
#pragma unroll
    for (int q = 0; q < kPairs; ++q) wacc[q] = 0.f;
    for (int64_t ib = i0; ib < i1; ib += kFuseTile) {
        const int64_t it = ib + tid;
        if (it < i1) {
            const int j = (int)(it % n), i = (int)((it / n) % n), h = (int)(it / ((int64_t)n * n));
            const float al = hdr[h], be = hdr[4 + h];
            for (int t = 0; t < T; ++t) {
                const int r = (t * kH + h) * n + i;
                s_d[t * kFuseTile + tid] = dense(fmaf(v[t * n + i], al, be), v[t * n + j], rs_s[2 * r], rs_s[2 * r + 1]);
            }
            for (int u = 0; u < T; ++u) {
                float acc = p.fus_b[u];
                for (int t = 0; t < T; ++t) acc = fmaf(p.fus_w[u * T + t], s_d[t * kFuseTile + tid], acc);
                const float gu = g[(((int64_t)u * kH + h) * n + i) * n + j];
                s_da[u * kFuseTile + tid] = acc > 0.f ? gu : fa * gu;
                la += acc > 0.f ? 0.f : gu * acc;
            }
            for (int t = 0; t < T; ++t) {
                const int64_t at = (((int64_t)t * kH + h) * n + i) * n + j;
                float d = g[at];
                for (int u = 0; u < T; ++u) d = fmaf(p.fus_w[u * T + t], s_da[u * kFuseTile + tid], d);
                dds[at] = d + dir[at];
            }
        } else {
            for (int t = 0; t < T; ++t) s_d[t * kFuseTile + tid] = s_da[t * kFuseTile + tid] = 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPairs; ++q) {
            const int pair = tid + q * kFuseTile;
            if (pair < T * T) {
                const int u = pair / T, t = pair % T;
                float acc = wacc[q];
                for (int e = 0; e < kFuseTile; ++e) acc = fmaf(s_da[u * kFuseTile + e], s_d[t * kFuseTile + e], acc);
                wacc[q] = acc;
            }
        }
        if (tid < T)
            for (int e = 0; e < kFuseTile; ++e) bacc += s_da[tid * kFuseTile + e];
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kPairs; ++q) {
        const int pair = tid + q * kFuseTile;
        if (pair < T * T) part[pair] = wacc[q];
    }
    if (tid < T) part[T * T + tid] = bacc;
    const float sa = block_sum(la, red);
    if (tid == 0) part[T * T + T] = sa;
}

// ---- softmax rows: d score = dense (d dense - sum dense d dense); d alpha_h, d beta_h of both attentions
template <bool GP>
__global__ __launch_bounds__(kSnThreads) void sgcn_rows_bwd(Ctx c, TLay tl, const float *__restrict__ gt0) {
    constexpr int kG = GP ? 32 : 16;  // GP: the temporal score row carries six numbers per head, hdr[8 + 4 q + h]
    __shared__ float red[(kSnThreads / kWave) * kG];
    const int tid = threadIdx.x, T = c.T;
    float *part = c.ws + tl.p_rows + (int64_t)blockIdx.x * kG;
    int64_t chunk, b, sq;
    int n;
    if (!find_slot<GP>(c, blockIdx.x, kBwdRows, [T](int m) { return 2 * (int64_t)T * kH * m; }, chunk, b, n, sq)) {
        if (tid < kG) part[tid] = 0.f;
        return;
    }
    const float *hdr = c.ws + tl.L.hdr;
    const float *v = c.ws + tl.L.v + T * b;
    const float *vp = c.ws + tl.L.vp + T * b;  // (GP only)
    const float *rs_s = c.ws + tl.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *dd_s = c.ws + tl.dd_s + (int64_t)T * kH * sq;
    const float *dn_t = c.ws + tl.L.ta + b * kH * T * T;  // the kept temporal attention
    const float *dd_t = c.ws + tl.dir_t + b * kH * T * T, *g_t = gt0 + b * kH * T * T;
    const int rows = T * kH * n;
    const int r0 = (int)chunk * kBwdRows, r1 = r0 + kBwdRows < 2 * rows ? r0 + kBwdRows : 2 * rows;
    float acc[kG];
#pragma unroll
    for (int e = 0; e < kG; ++e) acc[e] = 0.f;
    for (int rr = r0 + tid; rr < r1; rr += kSnThreads) {
        const bool temporal = rr >= rows;
        int h;
        float xi, dti = 0.f;
        float pi = 0.f, dtb = 0.f;  // GP, a temporal row: its position, and d b next to d a (dti)
        if (!temporal) {
            const int r = rr, i = r % n, t = r / (n * kH);
            h = (r / n) % kH;
            xi = v[t * n + i];
            const float ti = fmaf(xi, hdr[h], hdr[4 + h]), m = rs_s[2 * r], sum = rs_s[2 * r + 1];
            float s = 0.f;
            for (int j = 0; j < n; ++j) s = fmaf(dense(ti, v[t * n + j], m, sum), dd_s[(int64_t)r * n + j], s);
            for (int j = 0; j < n; ++j) {
                const float xj = v[t * n + j];
                dti = fmaf(dense(ti, xj, m, sum) * (dd_s[(int64_t)r * n + j] - s), xj, dti);
            }
            if constexpr (GP) {
                float *rec = c.ws + tl.srec + 2 * ((int64_t)T * kH * b + r);
                rec[0] = s;
                rec[1] = dti;
            }
        } else {
            const int r = rr - rows, t = r % T, i = r / (T * kH);
            h = (r / T) % kH;
            xi = v[t * n + i];
            float s = 0.f;
            for (int u = 0; u < T; ++u) s = fmaf(dn_t[(int64_t)r * T + u], g_t[(int64_t)r * T + u] + dd_t[(int64_t)r * T + u], s);
            if constexpr (GP) {
                pi = vp[t * n + i];
                for (int u = 0; u < T; ++u) {
                    const float ds = dn_t[(int64_t)r * T + u] * (g_t[(int64_t)r * T + u] + dd_t[(int64_t)r * T + u] - s);
                    dti = fmaf(ds, vp[u * n + i], dti);
                    dtb = fmaf(ds, v[u * n + i], dtb);
                }
                float *rec = c.ws + tl.trec + 3 * (b * kH * T + r);
                rec[0] = s;
                rec[1] = dti;
                rec[2] = dtb;
            } else {
                for (int u = 0; u < T; ++u)
                    dti = fmaf(dn_t[(int64_t)r * T + u] * (g_t[(int64_t)r * T + u] + dd_t[(int64_t)r * T + u] - s), v[u * n + i], dti);
            }
        }
        if (GP && temporal) {  // a = p h0 + c h1 + h2, b = p h3 + c h4 + h5
#pragma unroll
            for (int e = 8; e < kG; ++e) {
                if (e == 8 + h) acc[e] = fmaf(dti, pi, acc[e]);
                if (e == 12 + h) acc[e] = fmaf(dti, xi, acc[e]);
                if (e == 16 + h) acc[e] += dti;
                if (e == 20 + h) acc[e] = fmaf(dtb, pi, acc[e]);
                if (e == 24 + h) acc[e] = fmaf(dtb, xi, acc[e]);
                if (e == 28 + h) acc[e] += dtb;
            }
        } else {
            const int base = (temporal ? 8 : 0) + h;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e == base) acc[e] = fmaf(dti, xi, acc[e]);
                if (e == base + 4) acc[e] += dti;
            }
        }
    }
    const int wv = tid / kWave;
#pragma unroll
    for (int e = 0; e < kG; ++e) {
        const float s = wave_sum(acc[e]);
        if ((tid & (kWave - 1)) == 0) red[wv * kG + e] = s;
    }
    __syncthreads();
    if (tid < kG) {
        float s = 0.f;
        for (int w = 0; w < kSnThreads / kWave; ++w) s += red[w * kG + tid];
        part[tid] = s;
    }
}

// ---- prep backward: d alpha / d beta (their partials summed here, slots ascending) -> the attention tensors, fp64
__global__ __launch_bounds__(kSnThreads) void sgcn_prep_bwd(et_sgcn_params p, TLay tl, const float *ws, float *grads, GLay G) {
    __shared__ double aq[2][kE], cq[2][kE], ak[2][kE], daq[2][kE], dcq[2][kE], dak[2][kE];
    __shared__ float dab[16];
    const int tid = threadIdx.x;
    if (tid < 16) {
        float s = 0.f;
        for (int64_t g = 0; g < tl.n_rows2; ++g) s += ws[tl.p_rows + g * 16 + tid];
        dab[tid] = s;
    }
    if (tid < 2 * kE) {
        const int a = tid / kE, cc = tid % kE;
        const et_sgcn_attention &A = p.att[a];
        double s_aq = 0, s_cq = (double)A.q_b[cc], s_ak = 0;
        for (int e = 0; e < kE; ++e) {
            const double we = A.emb_w[e], be = A.emb_b[e];
            s_aq = fma((double)A.q_w[cc * kE + e], we, s_aq);
            s_cq = fma((double)A.q_w[cc * kE + e], be, s_cq);
            s_ak = fma((double)A.k_w[cc * kE + e], we, s_ak);
        }
        aq[a][cc] = s_aq;
        cq[a][cc] = s_cq;
        ak[a][cc] = s_ak;
    }
    __syncthreads();
    if (tid < 2 * kE) {
        const int a = tid / kE, cc = tid % kE, h = cc / kD;
        const double da = dab[a * 8 + h], db = dab[a * 8 + 4 + h];
        daq[a][cc] = da * ak[a][cc] * 0.125;
        dcq[a][cc] = db * ak[a][cc] * 0.125;
        dak[a][cc] = (da * aq[a][cc] + db * cq[a][cc]) * 0.125;
    }
    __syncthreads();
    for (int a = 0; a < 2; ++a) {
        const et_sgcn_attention &A = p.att[a];
        float *g = grads + G.att[a];  // emb_w 64, emb_b 64, q_w 4096, q_b 64, k_w 4096, k_b 64
        float *g_qw = g + 2 * kE, *g_qb = g_qw + kE * kE, *g_kw = g_qb + kE, *g_kb = g_kw + kE * kE;
        for (int q = tid; q < kE * kE; q += kSnThreads) {
            const int cc = q / kE, e = q % kE;
            g_qw[q] = (float)(daq[a][cc] * (double)A.emb_w[e] + dcq[a][cc] * (double)A.emb_b[e]);
            g_kw[q] = (float)(dak[a][cc] * (double)A.emb_w[e]);
        }
        if (tid < kE) {
            g_qb[tid] = (float)dcq[a][tid];
            g_kb[tid] = 0.f;  // the key bias shifts a softmax row by a constant
            double sw = 0, sb = 0;
            for (int cc = 0; cc < kE; ++cc) {
                sw = fma((double)A.q_w[cc * kE + tid], daq[a][cc], sw);
                sw = fma((double)A.k_w[cc * kE + tid], dak[a][cc], sw);
                sb = fma((double)A.q_w[cc * kE + tid], dcq[a][cc], sb);
            }
            g[tid] = (float)sw;
            g[kE + tid] = (float)sb;
        }
    }
}

// GP: the spatial attention as above; the temporal one reads x = (p, c) through a (64, 2) embedding.  Slots as sgcn_prep<true>:
// 0 spatial, 1 the coefficient column, 2 the position column; d h_q (q = 0..5, per head) at dab[8 + 4 q + h] with
//   h0 = aq_p.ak_p, h1 = aq_c.ak_p, h2 = cq.ak_p, h3 = aq_p.ak_c, h4 = aq_c.ak_c, h5 = cq.ak_c  (each / 8)
__global__ __launch_bounds__(kSnThreads) void sgcn_prep_bwd_gp(et_sgcn_params p, TLay tl, const float *ws, float *grads,
                                                               GLay G) {
    __shared__ double aq[3][kE], cq[3][kE], ak[3][kE], daq[3][kE], dcq[3][kE], dak[3][kE];
    __shared__ float dab[32];
    const int tid = threadIdx.x;
    if (tid < 32) {
        float s = 0.f;
        for (int64_t g = 0; g < tl.n_rows2; ++g) s += ws[tl.p_rows + g * 32 + tid];
        dab[tid] = s;
    }
    if (tid < 3 * kE) {
        const int slot = tid / kE, a = slot ? 1 : 0, cc = tid % kE;
        const int stride = a ? 2 : 1, col = slot == 1 ? 1 : 0;
        const et_sgcn_attention &A = p.att[a];
        double s_aq = 0, s_cq = (double)A.q_b[cc], s_ak = 0;
        for (int e = 0; e < kE; ++e) {
            const double we = A.emb_w[e * stride + col], be = A.emb_b[e];
            s_aq = fma((double)A.q_w[cc * kE + e], we, s_aq);
            s_cq = fma((double)A.q_w[cc * kE + e], be, s_cq);
            s_ak = fma((double)A.k_w[cc * kE + e], we, s_ak);
        }
        aq[slot][cc] = s_aq;
        cq[slot][cc] = s_cq;
        ak[slot][cc] = s_ak;
    }
    __syncthreads();
    if (tid < 3 * kE) {
        const int slot = tid / kE, cc = tid % kE, h = cc / kD;
        if (slot == 0) {
            const double da = dab[h], db = dab[4 + h];
            daq[0][cc] = da * ak[0][cc] * 0.125;
            dcq[0][cc] = db * ak[0][cc] * 0.125;
            dak[0][cc] = (da * aq[0][cc] + db * cq[0][cc]) * 0.125;
        } else {
            const double h0 = dab[8 + h], h1 = dab[12 + h], h2 = dab[16 + h], h3 = dab[20 + h], h4 = dab[24 + h], h5 = dab[28 + h];
            if (slot == 2) {  // the position column
                daq[2][cc] = (h0 * ak[2][cc] + h3 * ak[1][cc]) * 0.125;
                dak[2][cc] = (h0 * aq[2][cc] + h1 * aq[1][cc] + h2 * cq[1][cc]) * 0.125;
                dcq[2][cc] = 0;
            } else {  // the coefficient column, and the bias path
                daq[1][cc] = (h1 * ak[2][cc] + h4 * ak[1][cc]) * 0.125;
                dak[1][cc] = (h3 * aq[2][cc] + h4 * aq[1][cc] + h5 * cq[1][cc]) * 0.125;
                dcq[1][cc] = (h2 * ak[2][cc] + h5 * ak[1][cc]) * 0.125;
            }
        }
    }
    __syncthreads();
    {  // the spatial attention: emb_w 64, emb_b 64, q_w 4096, q_b 64, k_w 4096, k_b 64
        const et_sgcn_attention &A = p.att[0];
        float *g = grads + G.att[0];
        float *g_qw = g + 2 * kE, *g_qb = g_qw + kE * kE, *g_kw = g_qb + kE, *g_kb = g_kw + kE * kE;
        for (int q = tid; q < kE * kE; q += kSnThreads) {
            const int cc = q / kE, e = q % kE;
            g_qw[q] = (float)(daq[0][cc] * (double)A.emb_w[e] + dcq[0][cc] * (double)A.emb_b[e]);
            g_kw[q] = (float)(dak[0][cc] * (double)A.emb_w[e]);
        }
        if (tid < kE) {
            g_qb[tid] = (float)dcq[0][tid];
            g_kb[tid] = 0.f;  // the key bias shifts a softmax row by a constant
            double sw = 0, sb = 0;
            for (int cc = 0; cc < kE; ++cc) {
                sw = fma((double)A.q_w[cc * kE + tid], daq[0][cc], sw);
                sw = fma((double)A.k_w[cc * kE + tid], dak[0][cc], sw);
                sb = fma((double)A.q_w[cc * kE + tid], dcq[0][cc], sb);
            }
            g[tid] = (float)sw;
            g[kE + tid] = (float)sb;
        }
    }
    {  // the temporal attention: emb_w (64, 2) 128, emb_b 64, q_w 4096, q_b 64, k_w 4096, k_b 64
        const et_sgcn_attention &A = p.att[1];
        float *g = grads + G.att[1];
        float *g_eb = g + 2 * kE, *g_qw = g_eb + kE, *g_qb = g_qw + kE * kE, *g_kw = g_qb + kE, *g_kb = g_kw + kE * kE;
        for (int q = tid; q < kE * kE; q += kSnThreads) {
            const int cc = q / kE, e = q % kE;
            const double wp = A.emb_w[2 * e], wc = A.emb_w[2 * e + 1];
            g_qw[q] = (float)(daq[2][cc] * wp + daq[1][cc] * wc + dcq[1][cc] * (double)A.emb_b[e]);
            g_kw[q] = (float)(dak[2][cc] * wp + dak[1][cc] * wc);
        }
        if (tid < kE) {
            g_qb[tid] = (float)dcq[1][tid];
            g_kb[tid] = 0.f;
            double swp = 0, swc = 0, sb = 0;
            for (int cc = 0; cc < kE; ++cc) {
                swp = fma((double)A.q_w[cc * kE + tid], daq[2][cc], swp);
                swp = fma((double)A.k_w[cc * kE + tid], dak[2][cc], swp);
                swc = fma((double)A.q_w[cc * kE + tid], daq[1][cc], swc);
                swc = fma((double)A.k_w[cc * kE + tid], dak[1][cc], swc);
                sb = fma((double)A.q_w[cc * kE + tid], dcq[1][cc], sb);
            }
            g[2 * tid] = (float)swp;
            g[2 * tid + 1] = (float)swc;
            g_eb[tid] = (float)sb;
        }
    }
}

// ---- reduce: grads[goff + e] = the sum over the slots of part[pbase + slot * pstride + poff + e]
struct Seg {
    int64_t goff, pbase, pstride, nslots;
    int len, poff;
};
struct Segs {
    int n;
    int64_t total;  // elements over all segments
    Seg s[2 * ET_SGCN_MAX_LAYERS + 8];  // the base's 2 layers + 6, and GP-Graph's two (et_gpgraph_train.inl)
};

__global__ __launch_bounds__(kSnThreads) void sgcn_grad_reduce(Segs sg, const float *__restrict__ ws, float *__restrict__ grads) {
    int64_t e = (int64_t)blockIdx.x * kSnThreads + threadIdx.x;
    if (e >= sg.total) return;
    int q = 0;
    while (e >= sg.s[q].len) {
        e -= sg.s[q].len;
        ++q;
    }
    const Seg &s = sg.s[q];
    const float *src = ws + s.pbase + s.poff + e;
    float acc = 0.f;
    for (int64_t g = 0; g < s.nslots; ++g) acc += src[g * s.pstride];
    grads[s.goff + e] = acc;
}

static Ctx train_ctx(const et_sgcn_params &p, const TLay &tl, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2,
                     void *workspace) {
    Ctx c;
    c.off = off;
    c.N = N;
    c.n2cap = sum_n2;
    c.S = n_scenes;
    c.T = p.obs_len;
    c.ws = (float *)workspace;
    c.L = tl.L;
    c.Nr = N;
    c.Sr = n_scenes;
    return c;
}

// the eval driver (run_layers) on the kept layout: layer j reads stack j and writes stack j + 1, the tail stores its activations
static int run_train(const et_sgcn_params &p, const float *gv, const Ident &I, const float *C_obs, const float *nrm, int64_t N,
                     const int32_t *off, int n_scenes, int64_t sum_n2, int64_t max_n, float *out, float *logit_s,
                     float *logit_t, void *workspace, size_t workspace_bytes, hipStream_t st) {
    const int T = p.obs_len;
    const TLay tl = tlay_of(p, N, sum_n2, n_scenes);
    if (!workspace || workspace_bytes < (size_t)tl.total * 4) return ET_ERR_WORKSPACE;
    const Ctx c = train_ctx(p, tl, N, off, n_scenes, sum_n2, workspace);
    hipLaunchKernelGGL(sgcn_prep<false>, dim3(1), dim3(kSnThreads), 0, st, p, c.ws);
    run_layers<false>(p, c, gv, I, C_obs, nrm, max_n, out, nullptr, nullptr, st, tl.xs_stride, tl.xt_stride, c.ws + tl.keep);
    ET_LAUNCH_CHECK();
    const float *ls = c.ws + tl.xs + p.n_asym * tl.xs_stride, *lt = c.ws + tl.xt + p.n_asym * tl.xt_stride;
    if (logit_s && hipMemcpyAsync(logit_s, ls, (size_t)T * kH * sum_n2 * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ET_ERR_HIP;
    if (logit_t && hipMemcpyAsync(logit_t, lt, (size_t)N * kH * T * T * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ET_ERR_HIP;
    return ET_OK;
}

// tail_bwd .. prep_bwd on the scenes of c (GP: the 3 Sr virtual scenes; d_out (k, c.N, S)): number_asymmetric_conv_layer + 7
// launches; and the segments of the base's gradients for the reduce launch, which the caller makes
template <bool GP>
static void run_backward_core(const et_sgcn_params &p, const Ident &I, const Ctx &c, const TLay &tl, const GLay &G, int64_t max_n,
                              const float *d_out, float *grads, hipStream_t st, Segs &sg) {
    const int T = p.obs_len, na = p.n_asym, n_scenes = c.S;
    const dim3 blk(kSnThreads);
    float *ws = c.ws;
    const float *ls = ws + tl.xs + na * tl.xs_stride, *lt = ws + tl.xt + na * tl.xt_stride;
    hipLaunchKernelGGL(sgcn_tail_bwd<GP>, dim3((unsigned)tl.n_tail), blk, 0, st, c, tl, p, d_out);
    hipLaunchKernelGGL(sgcn_sadj_bwd<GP>, dim3((unsigned)tl.n_rows), blk, 0, st, c, tl, p, I, ls, ws + tl.gs + na * tl.xs_stride);
    const unsigned by_r = chunks((int64_t)T * kH * max_n * 4, n_scenes);
    hipLaunchKernelGGL(sgcn_sadj_f2<GP>, dim3((unsigned)n_scenes, by_r), blk, 0, st, c, tl, I, ls);
    hipLaunchKernelGGL(sgcn_tadj_bwd<GP>, dim3((unsigned)tl.n_rows), blk, 0, st, c, tl, p, I, lt, ws + tl.gt + na * tl.xt_stride);
    for (int j = na - 1; j >= 0; --j)  // d stack j + 1 -> d stack j
        hipLaunchKernelGGL(sgcn_asym_bwd<GP>, dim3((unsigned)(tl.n_as + tl.n_at)), blk, 0, st, c, tl, p.asym_s[j], p.asym_t[j], j,
                           ws + tl.xs + j * tl.xs_stride, ws + tl.gs + (j + 1) * tl.xs_stride, ws + tl.gs + j * tl.xs_stride,
                           ws + tl.xt + j * tl.xt_stride, ws + tl.gt + (j + 1) * tl.xt_stride, ws + tl.gt + j * tl.xt_stride);
    hipLaunchKernelGGL(sgcn_fuse_bwd<GP>, dim3((unsigned)tl.n_fuse), dim3(kFuseTile), 0, st, c, tl, p, ws + tl.gs);
    hipLaunchKernelGGL(sgcn_rows_bwd<GP>, dim3((unsigned)tl.n_rows2), blk, 0, st, c, tl, ws + tl.gt);
    if constexpr (GP)
        hipLaunchKernelGGL(sgcn_prep_bwd_gp, dim3(1), blk, 0, st, p, tl, ws, grads, G);
    else
        hipLaunchKernelGGL(sgcn_prep_bwd, dim3(1), blk, 0, st, p, tl, ws, grads, G);
    sg.n = 0;
    sg.total = 0;
    auto seg = [&](int64_t goff, int len, int64_t pbase, int64_t pstride, int64_t nslots, int poff) {
        sg.s[sg.n++] = Seg{goff, pbase, pstride, nslots, len, poff};
        sg.total += len;
    };
    const int gt_rest = (int)(tl.g_tail - (kD * kD + 1));
    seg(G.fus, T * T + T + 1, tl.p_fuse, T * T + T + 1, tl.n_fuse, 0);
    for (int j = 0; j < na; ++j) seg(G.asym_s + j * kAsymG, kAsymG, tl.p_asym_s + j * tl.n_as * kAsymG, kAsymG, tl.n_as, 0);
    for (int j = 0; j < na; ++j) seg(G.asym_t + j * kAsymG, kAsymG, tl.p_asym_t + j * tl.n_at * kAsymG, kAsymG, tl.n_at, 0);
    constexpr int kSadjG = kD + 1 + kD * kD + 1;
    seg(G.gcn[0], kD + 1, tl.p_sadj, kSadjG, tl.n_rows, 0);
    seg(G.gcn[1], kD * kD + 1, tl.p_tail, tl.g_tail, tl.n_tail, 0);
    seg(G.gcn[2], kD + 1, tl.p_tadj, kD + 1, tl.n_rows, 0);
    seg(G.gcn[3], kD * kD + 1, tl.p_sadj, kSadjG, tl.n_rows, kD + 1);
    seg(G.fusion, gt_rest, tl.p_tail, tl.g_tail, tl.n_tail, kD * kD + 1);
}

static int run_backward(const et_sgcn_params &p, const Ident &I, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2,
                        int64_t max_n, const float *d_out, float *grads, void *workspace, size_t workspace_bytes,
                        hipStream_t st) {
    const TLay tl = tlay_of(p, N, sum_n2, n_scenes);
    if (!workspace || workspace_bytes < (size_t)tl.total * 4) return ET_ERR_WORKSPACE;
    const Ctx c = train_ctx(p, tl, N, off, n_scenes, sum_n2, workspace);
    Segs sg;
    run_backward_core<false>(p, I, c, tl, glay_of(p), max_n, d_out, grads, st, sg);
    hipLaunchKernelGGL(sgcn_grad_reduce, dim3((unsigned)ceil_div(sg.total, kSnThreads)), dim3(kSnThreads), 0, st, sg, c.ws, grads);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

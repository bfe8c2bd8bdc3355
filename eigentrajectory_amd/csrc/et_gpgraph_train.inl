// et_gpgraph_train.inl -- GP-Graph-SGCN training (include/eigentraj.h "GP-Graph-SGCN predictor, training"): the training
// forward (the eval kernels of et_gpgraph.hip on a layout that keeps what the backward reads) and the backward pass with
// respect to every parameter of the wrapper and of its base.  #included by et_gpgraph.hip after et_sgcn_train.inl, whose
// kernels (their GP = true instantiations) are the base's backward on the 3 Sr virtual scenes.
//
// Backward, number_asymmetric_conv_layer + 13 launches for any number of scenes, in the order the gradient flows:
//   mix_bwd    per pedestrian      d o_m = g / 3 + (W^T g)_m (z > 0 ? 1 : a) for its three passes' outputs; PReLU(z), g and its
//                                  part of d mix_a stay for the next launch
//   mixw_bwd   per element of (mix_a, mix_w, mix_b) and chunk of ET_GPGRAPH_BWD_ROWS pedestrians: the chunk's rows ascending
//              (one-dimensional grid, chunk-major: the number of chunks is not held to a grid's y limit)
//   unpool     per virtual row     the base's upstream gradient: passes 0 and 2 as they are, a group's row the sum of its
//                                  members' d o_1, members ascending
//   tail_bwd .. prep_bwd           et_sgcn_train.inl on the virtual scenes (weight gradients: chunks ascending, then virtual
//                                  scenes ascending, which is pass 0's scenes, pass 1's, pass 2's)
//   dx         per (t, i) of the virtual scenes of passes 1 and 2 (pass 0's input is detached): the input gradient, channel 1
//                                  (coefficients) from the spatial attention as query and as key, the temporal attention, A_s x
//                                  and A_t x of the two first gcn layers; channel 0 (position) from the temporal attention
//   group_bwd  per real scene      pool, straight-through, the soft assignment, the learned distance, group_cnn
//   reduce     per gradient element  the fixed-order sum of the per-workgroup partials (et_sgcn_train.inl)
// No atomics; every sum has a fixed order (a lane's items ascending, the lanes by a fixed butterfly, the wavefronts ascending,
// the partials ascending), so two runs agree bit for bit and a scene's kept values do not depend on its neighbours.
constexpr int kGpBwdRows = ET_GPGRAPH_BWD_ROWS;  // pedestrians per slot of the mix weights' partials
constexpr int kGrpG = 1 + 3 * kGpHid + kGpHid;   // group_gen.th, group_cnn.0.weight (8, 1, 3, 1), .bias (8)

struct GTLay {  // the training workspace, in floats
    TLay t;                          // the base's, for the 3 Nr virtual rows
    WLay W;                          // v_abs, group_cnn's features, dist, sig / colsum, the three passes' outputs
    int64_t sig, cs, cnt;            // kept by the group kernel: sig (sum n^2), its column sums (Nr), group sizes int32 (Nr)
    int64_t dmix, dpo;               // (k, 3 Nr, S) each: d o_m per pedestrian; the base's upstream gradient (pass 1 pooled)
    int64_t mact, mg, mda;           // per pedestrian: PReLU(z) (3 S k), g (S k), its part of d mix_a (1)
    int64_t dvp, dP, dsig, dd, df;   // d v' (2, T, n) at 2 T b; (n, n) blocks at the scene's packed offset; d f (8, T, n) at 8 T b
    int64_t p_mix, n_mix, g_mix, p_grp;
    int64_t total;
};

__host__ __device__ inline GTLay gtlay_of(const et_sgcn_params &p, int64_t N, int64_t n2, int64_t S) {
    GTLay g;
    const int T = p.obs_len, k = p.pred_len, So = p.out_dims;
    g.t = tlay_of(p, 3 * N, 3 * n2, 3 * S, true);
    g.W = wlay_of(g.t.L, T, k, So, N, n2);
    int64_t at = g.W.total;
    auto take = [&](int64_t n) {
        const int64_t o = at;
        at = up4(at + n);
        return o;
    };
    const int64_t Sk = (int64_t)So * k;
    g.sig = take(n2);
    g.cs = take(N);
    g.cnt = take(N);
    g.dmix = take(k * 3 * N * So);
    g.dpo = take(k * 3 * N * So);
    g.mact = take(N * 3 * Sk);
    g.mg = take(N * Sk);
    g.mda = take(N);
    g.dvp = take(2 * T * N);
    g.dP = take(n2);
    g.dsig = take(n2);
    g.dd = take(n2);
    g.df = take((int64_t)kGpHid * T * N);
    g.g_mix = 1 + Sk * 3 * Sk + Sk;
    g.n_mix = ceil_div(N, (int64_t)kGpBwdRows);
    g.p_mix = take(g.n_mix * g.g_mix);
    g.p_grp = take(S * kGrpG);
    g.total = at;
    return g;
}

// ---- mix backward: one workgroup per pedestrian, as gp_mix
__global__ __launch_bounds__(kMixThreads) void gp_mix_bwd(GpTab c, GpWeights p, GTLay gl, float *__restrict__ ws,
                                                          const float *__restrict__ g_out, int graph_layout) {
    extern __shared__ float mixb_lds[];  // z (3 S k), g (S k)
    __shared__ float red[kMixThreads / kWave];
    const int k = p.k, S = p.S, Sk = S * k, tid = threadIdx.x;
    float *raw = mixb_lds, *g = mixb_lds + 3 * Sk;
    const int64_t r = blockIdx.x, Nr = c.Nr;
    const int s = c.off ? scene_of_row(c.off, c.Sr, r) : 0;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    const bool ok = r >= b && r < e && c.sq[s] >= 0;
    int64_t row[3] = {r, r, 2 * Nr + r};
    if (ok) row[1] = Nr + b + c.gidx[r];
    const float *po = ws + gl.W.po;
    const float a = p.mix_a[0];
    for (int q = tid; q < 3 * Sk; q += kMixThreads) {
        const int m = q / Sk, ss = (q % Sk) / k, t = q % k;
        raw[q] = ok ? po[((int64_t)t * 3 * Nr + row[m]) * S + ss] : 0.f;
    }
    for (int o = tid; o < Sk; o += kMixThreads) {
        const int ss = o / k, t = o % k;
        const float x = !ok ? 0.f : graph_layout ? g_out[((int64_t)ss * k + t) * Nr + r] : g_out[((int64_t)t * Nr + r) * S + ss];
        g[o] = x;
        ws[gl.mg + r * Sk + o] = x;
    }
    __syncthreads();
    float la = 0.f;
    for (int q = tid; q < 3 * Sk; q += kMixThreads) {
        float acc = 0.f;
        for (int o = 0; o < Sk; ++o) acc = fmaf(p.mix_w[(int64_t)o * 3 * Sk + q], g[o], acc);
        const int m = q / Sk, ss = (q % Sk) / k, t = q % k;
        const float z = raw[q];
        const float dz = g[q % Sk] / 3.0f + (z > 0.f ? acc : a * acc);
        la += z > 0.f ? 0.f : acc * z;
        ws[gl.dmix + ((int64_t)t * 3 * Nr + m * Nr + r) * S + ss] = ok ? dz : 0.f;  // (pass 1: still per pedestrian)
        ws[gl.mact + r * 3 * Sk + q] = ok ? prelu(z, a) : 0.f;
    }
    const float sa = block_sum(la, red);
    if (tid == 0) ws[gl.mda + r] = sa;
}

// ---- d (mix_a, mix_w, mix_b): block b is part b % per of chunk b / per (per = the blocks an element range takes); element e
// of the chunk, the chunk's pedestrians ascending
__global__ __launch_bounds__(kSnThreads) void gp_mixw_bwd(GTLay gl, float *__restrict__ ws, int64_t Nr, int Sk, unsigned per) {
    const int64_t chunk = blockIdx.x / per;
    const int64_t e = (int64_t)(blockIdx.x % per) * kSnThreads + threadIdx.x;
    if (e >= gl.g_mix) return;
    const int64_t r0 = chunk * kGpBwdRows, r1 = r0 + kGpBwdRows < Nr ? r0 + kGpBwdRows : Nr;
    const float *mg = ws + gl.mg, *mact = ws + gl.mact;
    float acc = 0.f;
    if (e == 0) {
        for (int64_t r = r0; r < r1; ++r) acc += ws[gl.mda + r];
    } else if (e <= (int64_t)Sk * 3 * Sk) {
        const int64_t o = (e - 1) / (3 * Sk), q = (e - 1) % (3 * Sk);
        for (int64_t r = r0; r < r1; ++r) acc = fmaf(mg[r * Sk + o], mact[r * 3 * Sk + q], acc);
    } else {
        const int64_t o = e - 1 - (int64_t)Sk * 3 * Sk;
        for (int64_t r = r0; r < r1; ++r) acc += mg[r * Sk + o];
    }
    ws[gl.p_mix + chunk * gl.g_mix + e] = acc;
}

// ---- unpool: virtual row (pass m, row) of the base's upstream gradient
__global__ __launch_bounds__(kMixThreads) void gp_unpool_bwd(GpTab c, GTLay gl, float *__restrict__ ws, int k, int S) {
    const int64_t vr = blockIdx.x, Nr = c.Nr;
    const int m = (int)(vr / Nr);
    const int64_t r = vr - (int64_t)m * Nr;
    const int s = c.off ? scene_of_row(c.off, c.Sr, r) : 0;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    const bool ok = r >= b && r < e && c.sq[s] >= 0;
    const float *dmix = ws + gl.dmix;
    float *dpo = ws + gl.dpo;
    const int n = (int)(e - b), g = (int)(r - b);
    const bool group_row = ok && m == 1 && g < c.vn[c.Sr + s];
    for (int q = threadIdx.x; q < k * S; q += kMixThreads) {
        const int t = q / S, ss = q % S;
        float x = 0.f;
        if (m != 1) {
            if (ok) x = dmix[((int64_t)t * 3 * Nr + vr) * S + ss];
        } else if (group_row) {
            for (int i = 0; i < n; ++i)
                if (c.gidx[b + i] == g) x += dmix[((int64_t)t * 3 * Nr + Nr + b + i) * S + ss];
        }
        dpo[((int64_t)t * 3 * Nr + vr) * S + ss] = x;
    }
}

// ---- the base's input gradient of the virtual scenes of passes 1 and 2: item (t, i), both channels
__global__ __launch_bounds__(kSnThreads) void gp_dx(Ctx c, TLay tl) {
    int64_t b, sq;
    int n;
    const int s = c.Sr + blockIdx.x;
    if (!scene_at<true>(c, s, b, n, sq)) return;
    const int T = c.T;
    const float *hdr = c.ws + tl.L.hdr;
    const float *v = c.ws + tl.L.v + T * b;
    const float *vp = c.ws + tl.L.vp + T * b;
    const float *rs_s = c.ws + tl.L.rs_s + 2 * (int64_t)T * kH * b;
    const float *dd_s = c.ws + tl.dd_s + (int64_t)T * kH * sq;
    const float *srec = c.ws + tl.srec + 2 * (int64_t)T * kH * b;
    const float *trec = c.ws + tl.trec + 3 * (b * kH * T);
    const float *dx_as = c.ws + tl.dx_as + b * kH * T;
    const float *dacc_t = c.ws + tl.dacc_t + b * kH * T;
    const float *at = c.ws + tl.L.at + b * kH * T * T;
    const float *dn_t = c.ws + tl.L.ta + b * kH * T * T;  // the kept temporal attention
    const float *g_t = c.ws + tl.gt + b * kH * T * T, *dd_t = c.ws + tl.dir_t + b * kH * T * T;
    float *dxp = c.ws + tl.dxp + T * b, *dxv = c.ws + tl.dxv + T * b;
    for (int it = blockIdx.y * kSnThreads + threadIdx.x; it < T * n; it += gridDim.y * kSnThreads) {
        const int i = it % n, t = it / n;
        const float xi = v[t * n + i];
        float dc = 0.f, dp = 0.f;
        for (int h = 0; h < kH; ++h) {
            // the spatial attention: score (i, j) = t_i x_j, t_i = x_i alpha + beta; as the query, then as the key of every row
            dc = fmaf(srec[2 * ((t * kH + h) * n + i) + 1], hdr[h], dc);
            float key = 0.f;
            for (int i2 = 0; i2 < n; ++i2) {
                const int r2 = (t * kH + h) * n + i2;
                const float ti = fmaf(v[t * n + i2], hdr[h], hdr[4 + h]);
                const float ds = dense(ti, xi, rs_s[2 * r2], rs_s[2 * r2 + 1]) * (dd_s[(int64_t)r2 * n + i] - srec[2 * r2]);
                key = fmaf(ds, ti, key);
            }
            dc += key;
            dc += dx_as[(i * kH + h) * T + t];  // A_s x of spatial_temporal gcn 0
            // the temporal attention: score (t, u) = p_u a_t + c_u b_t; as the query
            const float *rec = trec + 3 * ((i * kH + h) * T + t);
            dp = fmaf(rec[1], hdr[8 + h], dp);
            dp = fmaf(rec[2], hdr[20 + h], dp);
            dc = fmaf(rec[1], hdr[12 + h], dc);
            dc = fmaf(rec[2], hdr[24 + h], dc);
            float kp = 0.f, kc = 0.f, ax = 0.f;  // as the key of every row t2; A_t x of temporal_spatial gcn 0
            for (int t2 = 0; t2 < T; ++t2) {
                const int r2 = (i * kH + h) * T + t2;
                const int64_t at2 = (int64_t)r2 * T + t;
                const float ds = dn_t[at2] * (g_t[at2] + dd_t[at2] - trec[3 * r2]);
                const TRow<true> tr = trow_of<true>(hdr, v, vp, n, t2, i, h);
                kp = fmaf(ds, tr.a, kp);
                kc = fmaf(ds, tr.b, kc);
                ax = fmaf(at[at2], dacc_t[r2], ax);
            }
            dp += kp;
            dc += kc;
            dc += ax;
        }
        dxp[it] = dp;
        dxv[it] = dc;
    }
}

// ---- pool, straight-through, soft assignment, learned distance and group_cnn of one real scene
__global__ __launch_bounds__(kSnThreads) void gp_group_bwd(Ctx c, GpTab tab, GpWeights p, GTLay gl) {
    __shared__ float cols[ET_SGCN_MAX_N];
    __shared__ float red[(kSnThreads / kWave) * kGrpG];
    const int s = blockIdx.x, tid = threadIdx.x, T = c.T, Sr = c.Sr;
    const int64_t Nr = c.Nr;
    float *ws = c.ws;
    float *part = ws + gl.p_grp + (int64_t)s * kGrpG;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    const int64_t sq = e > b ? tab.sq[s] : -1;
    if (sq < 0) {  // an empty scene, or one the forward did not compute
        if (tid < kGrpG) part[tid] = 0.f;
        return;
    }
    const int n = (int)(e - b), G = tab.vn[Sr + s];
    const int32_t *idx = tab.gidx + b;
    const int32_t *cnt = reinterpret_cast<const int32_t *>(ws + gl.cnt) + b;
    const float tau = p.tau;
    const float *x0[2] = {ws + gl.t.L.vp + T * b, ws + gl.t.L.v + T * b};                        // v_rel (pass 0's input)
    const float *d1[2] = {ws + gl.t.dxp + T * (Nr + b), ws + gl.t.dxv + T * (Nr + b)};          // d (pooled in) (T, G)
    const float *d2[2] = {ws + gl.t.dxp + T * (2 * Nr + b), ws + gl.t.dxv + T * (2 * Nr + b)};  // d v'_intra (T, n)
    float *dvp = ws + gl.dvp + 2 * T * b;
    float *dP = ws + gl.dP + sq, *dsig = ws + gl.dsig + sq, *dd = ws + gl.dd + sq;
    const float *sn = ws + gl.W.sn + sq, *sig = ws + gl.sig + sq, *cs = ws + gl.cs + b;
    const float *va = ws + gl.W.va + T * b, *feat = ws + gl.W.feat + (int64_t)kGpHid * T * b;
    float *df = ws + gl.df + (int64_t)kGpHid * T * b;
    // pool: d v' = d v'_intra + d (pooled in)[group] / |group|; the straight-through estimator hands it to v_soft as it is
    for (int q = tid; q < 2 * T * n; q += kSnThreads) {
        const int i = q % n, t = (q / n) % T, ch = q / (n * T);
        const int g = idx[i];
        dvp[q] = d2[ch][t * n + i] + d1[ch][t * G + g] / (float)cnt[g];
    }
    __syncthreads();
    // v_soft = v_rel @ P: d P[i][j] = sum over (channel, t) of v_rel[.., i] d v_soft[.., j]
    for (int q = tid; q < n * n; q += kSnThreads) {
        const int i = q / n, j = q % n;
        float acc = 0.f;
        for (int ch = 0; ch < 2; ++ch)
            for (int t = 0; t < T; ++t) acc = fmaf(x0[ch][t * n + i], dvp[(ch * T + t) * n + j], acc);
        dP[q] = acc;
    }
    __syncthreads();
    // P = sig / colsum: d sig[i][j] = (d P[i][j] - sum_i' P[i'][j] d P[i'][j]) / c_j
    for (int j = tid; j < n; j += kSnThreads) {
        float acc = 0.f;
        for (int i = 0; i < n; ++i) acc = fmaf(sn[i * n + j], dP[i * n + j], acc);
        cols[j] = acc;
    }
    __syncthreads();
    float gth = 0.f;
    for (int q = tid; q < n * n; q += kSnThreads) {
        const int j = q % n;
        const float sg = sig[q];
        const float ds = (dP[q] - cols[j]) / cs[j];
        const float du = ds * (sg * (1.0f - sg));  // sig = sigmoid(u), u = -(d - th) / tau
        dsig[q] = ds;
        dd[q] = -du / tau;
        gth += du / tau;
    }
    __syncthreads();
    // d[i][j] = mean over t of |f_i - f_j|: d f_i = sum_j (d d[i][j] + d d[j][i]) / T (f_i - f_j) / |f_i - f_j|, 0 where the norm is 0
    for (int q = tid; q < T * n; q += kSnThreads) {
        const int i = q % n, t = q / n;
        float fi[kGpHid], acc[kGpHid];
#pragma unroll
        for (int ch = 0; ch < kGpHid; ++ch) {
            fi[ch] = feat[(ch * T + t) * n + i];
            acc[ch] = 0.f;
        }
        for (int j = 0; j < n; ++j) {
            float dfc[kGpHid], ss = 0.f;
#pragma unroll
            for (int ch = 0; ch < kGpHid; ++ch) {
                dfc[ch] = fi[ch] - feat[(ch * T + t) * n + j];
                ss = fmaf(dfc[ch], dfc[ch], ss);
            }
            const float nr = sqrtf(ss);
            if (nr > 0.f) {
                const float w = ((dd[i * n + j] + dd[j * n + i]) / (float)T) / nr;
#pragma unroll
                for (int ch = 0; ch < kGpHid; ++ch) acc[ch] = fmaf(w, dfc[ch], acc[ch]);
            }
        }
#pragma unroll
        for (int ch = 0; ch < kGpHid; ++ch) df[(ch * T + t) * n + i] = acc[ch];
    }
    __syncthreads();
    // group_cnn: Conv2d(1, 8, (3, 1), padding (1, 0)) along t
    float gw[3 * kGpHid], gb[kGpHid];
#pragma unroll
    for (int q = 0; q < 3 * kGpHid; ++q) gw[q] = 0.f;
#pragma unroll
    for (int ch = 0; ch < kGpHid; ++ch) gb[ch] = 0.f;
    for (int q = tid; q < T * n; q += kSnThreads) {
        const int i = q % n, t = q / n;
        const float xm = t > 0 ? va[(t - 1) * n + i] : 0.f, xc = va[t * n + i], xn = t + 1 < T ? va[(t + 1) * n + i] : 0.f;
#pragma unroll
        for (int ch = 0; ch < kGpHid; ++ch) {
            const float g = df[(ch * T + t) * n + i];
            gw[ch * 3] = fmaf(g, xm, gw[ch * 3]);
            gw[ch * 3 + 1] = fmaf(g, xc, gw[ch * 3 + 1]);
            gw[ch * 3 + 2] = fmaf(g, xn, gw[ch * 3 + 2]);
            gb[ch] += g;
        }
    }
    const int wv = tid / kWave;
    {
        const float sv = wave_sum(gth);
        if ((tid & (kWave - 1)) == 0) red[wv * kGrpG] = sv;
    }
#pragma unroll
    for (int q = 0; q < 3 * kGpHid; ++q) {
        const float sv = wave_sum(gw[q]);
        if ((tid & (kWave - 1)) == 0) red[wv * kGrpG + 1 + q] = sv;
    }
#pragma unroll
    for (int ch = 0; ch < kGpHid; ++ch) {
        const float sv = wave_sum(gb[ch]);
        if ((tid & (kWave - 1)) == 0) red[wv * kGrpG + 1 + 3 * kGpHid + ch] = sv;
    }
    __syncthreads();
    if (tid < kGrpG) {
        float sv = 0.f;
        for (int w = 0; w < kSnThreads / kWave; ++w) sv += red[w * kGrpG + tid];
        part[tid] = sv;
    }
}

// the flat gradient buffer: the base's (glay_of, GP), then group_gen.th, group_cnn.0.weight, .bias, then
// group_mix.st_gcns_mix.0.weight, .1.weight, .1.bias
static int64_t gp_grad_floats(const et_sgcn_params &b) {
    const int64_t Sk = (int64_t)b.out_dims * b.pred_len;
    return glay_of(b, true).total + kGrpG + 1 + Sk * 3 * Sk + Sk;
}

static Ctx gp_train_ctx(const et_sgcn_params &bp, const GTLay &gl, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2,
                        void *workspace) {
    Ctx c;
    c.off = off;
    c.N = 3 * N;
    c.n2cap = 3 * sum_n2;
    c.S = 3 * n_scenes;
    c.T = bp.obs_len;
    c.ws = (float *)workspace;
    c.L = gl.t.L;
    c.Nr = N;
    c.Sr = n_scenes;
    return c;
}

// gp_run on the kept layout: the same kernels and launches
static int gp_run_train(const et_gpgraph_sgcn_params &p, const float *g_abs, const float *g_rel, const float *C_obs,
                        const float *nrm, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2, int64_t max_n, float *out,
                        int graph_layout, int32_t *group_index, float *dist, float *logit_s, float *logit_t, void *workspace,
                        size_t workspace_bytes, hipStream_t st) {
    const et_sgcn_params &bp = p.base;
    const int T = bp.obs_len;
    const GTLay gl = gtlay_of(bp, N, sum_n2, n_scenes);
    if (!workspace || workspace_bytes < (size_t)gl.total * 4) return ET_ERR_WORKSPACE;
    const Ctx c = gp_train_ctx(bp, gl, N, off, n_scenes, sum_n2, workspace);
    const Ident I{nullptr, nullptr, 1, -1};
    hipLaunchKernelGGL(sgcn_prep<true>, dim3(1), dim3(kSnThreads), 0, st, bp, c.ws);
    const GpTab tab = tab_of(c);
    const GpWeights w = weights_of(p);
    hipLaunchKernelGGL(gp_group, dim3((unsigned)n_scenes), dim3(kSnThreads), 0, st, c, tab, w, gl.W, GpKeep{gl.sig, gl.cs, gl.cnt},
                       sum_n2, g_abs, g_rel, C_obs, nrm, group_index, dist);
    float *po = c.ws + gl.W.po;
    run_layers<true>(bp, c, nullptr, I, nullptr, nullptr, max_n, po, nullptr, nullptr, st, gl.t.xs_stride, gl.t.xt_stride,
                     c.ws + gl.t.keep);
    hipLaunchKernelGGL(gp_mix, dim3((unsigned)N), dim3(kMixThreads), 6 * bp.out_dims * bp.pred_len * sizeof(float), st, tab, w,
                       po, out, graph_layout);
    ET_LAUNCH_CHECK();
    const float *ls = c.ws + gl.t.xs + bp.n_asym * gl.t.xs_stride, *lt = c.ws + gl.t.xt + bp.n_asym * gl.t.xt_stride;
    if (logit_s && hipMemcpyAsync(logit_s, ls, (size_t)T * kH * 3 * sum_n2 * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ET_ERR_HIP;
    if (logit_t && hipMemcpyAsync(logit_t, lt, (size_t)3 * N * kH * T * T * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return ET_ERR_HIP;
    return ET_OK;
}

static int gp_run_backward(const et_gpgraph_sgcn_params &p, int64_t N, const int32_t *off, int n_scenes, int64_t sum_n2,
                           int64_t max_n, const float *d_out, int graph_layout, float *grads, void *workspace,
                           size_t workspace_bytes, hipStream_t st) {
    const et_sgcn_params &bp = p.base;
    const int T = bp.obs_len, k = bp.pred_len, S = bp.out_dims, Sk = S * k;
    const GTLay gl = gtlay_of(bp, N, sum_n2, n_scenes);
    if (!workspace || workspace_bytes < (size_t)gl.total * 4) return ET_ERR_WORKSPACE;
    const Ctx c = gp_train_ctx(bp, gl, N, off, n_scenes, sum_n2, workspace);
    const Ident I{nullptr, nullptr, 1, -1};
    const GpTab tab = tab_of(c);
    const GpWeights w = weights_of(p);
    const GLay G = glay_of(bp, true);
    const dim3 blk(kSnThreads);
    const int64_t per = ceil_div(gl.g_mix, (int64_t)kSnThreads);  // blocks of mixw_bwd per chunk of pedestrians
    if (per * gl.n_mix > INT32_MAX) return ET_ERR_INVALID_ARG;    // (its grid; answered before any launch)
    hipLaunchKernelGGL(gp_mix_bwd, dim3((unsigned)N), dim3(kMixThreads), 4 * Sk * sizeof(float), st, tab, w, gl, c.ws, d_out,
                       graph_layout);
    hipLaunchKernelGGL(gp_mixw_bwd, dim3((unsigned)(per * gl.n_mix)), blk, 0, st, gl, c.ws, N, Sk, (unsigned)per);
    hipLaunchKernelGGL(gp_unpool_bwd, dim3((unsigned)(3 * N)), dim3(kMixThreads), 0, st, tab, gl, c.ws, k, S);
    Segs sg;
    run_backward_core<true>(bp, I, c, gl.t, G, max_n, c.ws + gl.dpo, grads, st, sg);
    const unsigned by = chunks((int64_t)T * max_n, n_scenes);
    hipLaunchKernelGGL(gp_dx, dim3((unsigned)(2 * n_scenes), by), blk, 0, st, c, gl.t);
    hipLaunchKernelGGL(gp_group_bwd, dim3((unsigned)n_scenes), blk, 0, st, c, tab, w, gl);
    sg.s[sg.n++] = Seg{G.total, gl.p_grp, kGrpG, n_scenes, kGrpG, 0};
    sg.s[sg.n++] = Seg{G.total + kGrpG, gl.p_mix, gl.g_mix, gl.n_mix, (int)gl.g_mix, 0};
    sg.total += kGrpG + gl.g_mix;
    hipLaunchKernelGGL(sgcn_grad_reduce, dim3((unsigned)ceil_div(sg.total, (int64_t)kSnThreads)), blk, 0, st, sg, c.ws, grads);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

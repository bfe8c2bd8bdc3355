// et_gpgraph_core.inl -- what GP-Graph does around its base network, whichever base that is: the grouping of one scene and the
// mix of the three passes.  One fragment #included (after et_sgcn_core.inl, whose scene helpers it uses) by et_gpgraph.hip
// (SGCN base: v_rel carries CH = 2 channels, position and coefficients) and et_gpgraph_stgcnn.hip (Social-STGCNN base: CH = 1)
// inside their anonymous namespaces.  The CH = 2 instantiation keeps the statements and the orders et_gpgraph.hip had.
constexpr int kGpHid = 8;  // group_cnn's output channels
constexpr int kMixThreads = 128;

__device__ __forceinline__ float sig_of(float d, float th, float tau) { return 1.0f / (1.0f + expf(-(-(d - th) / tau))); }

struct GpTab {  // the tables the group kernel leaves for the kernels behind it
    const int32_t *off;  // the real scenes' offsets, or NULL: one scene of Nr rows
    int64_t Nr;
    int Sr;
    int64_t *sq;    // [3 Sr] (pass m, scene s): the scene's offset in the packed n^2 stacks, -1: not computed
    int32_t *vn;    // [3 Sr] node counts: n, G, n
    int32_t *gidx;  // [Nr] scene-local group index
};

struct GpScene {  // where one real scene's grouping goes (floats in the workspace)
    float *va, *feat;   // v_abs (T, n), group_cnn's features (8, T, n)
    float *D, *sn;      // dist and sig_norm (n, n)
    float *in[3][2];    // pass m's input, channel ch: (T, n_m) blocks (CH = 1: [m][0] only)
    float *sig = nullptr, *cs = nullptr;   // the training forward keeps sig (n, n) and its column sums (n); else NULL
    int32_t *cnt = nullptr;                // ... and the group sizes (n)
};

struct GpWeights {
    const float *group_w, *group_b, *th;
    float tau;
    const float *mix_a, *mix_w, *mix_b;
    int k, S;
};

// ---- the grouping of real scene s (rows b .. b + n of Nr, packed offset sq): one workgroup of kSnThreads.  g_abs / g_rel:
// the graph form's inputs (T, n) / (CH, T, n), or NULL: the scenes form builds them from C_obs and nrm
template <int CH>
__device__ __forceinline__ void gp_group_scene(const GpTab &tab, const GpScene &gs, const GpWeights &p, int s, int64_t b, int n,
                                               int T, int64_t sq, const float *__restrict__ g_abs,
                                               const float *__restrict__ g_rel, const float *__restrict__ C_obs,
                                               const float *__restrict__ nrm, int32_t *__restrict__ group_index,
                                               float *__restrict__ dist_out) {
    __shared__ float red[2 * kSnThreads / kWave];
    __shared__ int lab[ET_SGCN_MAX_N], cmx[ET_SGCN_MAX_N], idx[ET_SGCN_MAX_N], cnt[ET_SGCN_MAX_N];
    __shared__ unsigned char hit[ET_SGCN_MAX_N];
    __shared__ float cs[ET_SGCN_MAX_N];
    __shared__ int n_groups;
    const int tid = threadIdx.x, Sr = tab.Sr;
    const int64_t Nr = tab.Nr;
    float *va = gs.va, *feat = gs.feat, *D = gs.D, *sn = gs.sn;
    float *p0 = gs.in[0][0], *v0 = gs.in[0][CH - 1], *p1 = gs.in[1][0], *v1 = gs.in[1][CH - 1], *p2 = gs.in[2][0],
          *v2 = gs.in[2][CH - 1];
    const float th = p.th[0], tau = p.tau;

    // v_abs, and the pedestrian graph v_rel (CH = 2: [position; coefficients])
    scene_v(va, g_abs, C_obs, nrm, Nr, b, n, T, red);
    if constexpr (CH == 2) {
        for (int q = tid; q < T * n; q += kSnThreads) {
            p0[q] = g_rel ? g_rel[q] : (float)(q / n + 1);
            if (g_rel) v0[q] = g_rel[T * n + q];
        }
    }
    __syncthreads();
    if (CH == 1 || !g_rel)
        for (int q = tid; q < T * n; q += kSnThreads) v0[q] = CH == 1 && g_rel ? g_rel[q] : va[q];
    // group_cnn: Conv2d(1, 8, (3, 1), padding (1, 0)) along t
    for (int q = tid; q < kGpHid * T * n; q += kSnThreads) {
        const int i = q % n, t = (q / n) % T, ch = q / (n * T);
        float acc = p.group_b[ch];
        for (int d = 0; d < 3; ++d) {
            const int tt = t + d - 1;
            if (tt >= 0 && tt < T) acc = fmaf(p.group_w[ch * 3 + d], va[tt * n + i], acc);
        }
        feat[q] = acc;
    }
    __syncthreads();
    // d[i][j]: the mean over t of the L2 norm over the channels (symmetric bit for bit: (a - b)^2 = (b - a)^2, one order)
    for (int q = tid; q < n * n; q += kSnThreads) {
        const int i = q / n, j = q % n;
        float tot = 0.f;
        for (int t = 0; t < T; ++t) {
            float ss = 0.f;
            for (int ch = 0; ch < kGpHid; ++ch) {
                const float df = feat[(ch * T + t) * n + i] - feat[(ch * T + t) * n + j];
                ss = fmaf(df, df, ss);
            }
            tot += sqrtf(ss);
        }
        const float d = tot / (float)T;
        D[q] = d;
        if (dist_out) dist_out[sq + q] = d;
    }
    __syncthreads();
    // the last close column of every row (-1: none), and the labels' start
    for (int r = tid; r < n; r += kSnThreads) {
        int cm = -1;
        for (int cc = 0; cc < r; ++cc)
            if (D[r * n + cc] <= th) cm = cc;
        cmx[r] = cm;
        lab[r] = r;
    }
    __syncthreads();
    for (int r = 1; r < n; ++r) {
        const int cm = cmx[r];
        if (cm < 0) continue;  // (uniform)
        const int lr = lab[r];
        for (int cc = tid; cc < n; cc += kSnThreads) hit[cc] = cc < r && D[r * n + cc] <= th;
        __syncthreads();
        for (int i = tid; i < n; i += kSnThreads) {
            const int l = lab[i];
            if (hit[l] || l == lr) lab[i] = cm;
        }
        __syncthreads();
    }
    // compact labels in the order of the surviving values; group sizes
    for (int i = tid; i < n; i += kSnThreads) {
        hit[i] = 0;
        cnt[i] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kSnThreads) hit[lab[i]] = 1;
    __syncthreads();
    for (int i = tid; i < n; i += kSnThreads) {
        int rank = 0;
        for (int l = 0; l < lab[i]; ++l) rank += hit[l];
        idx[i] = rank;
        atomicAdd(&cnt[rank], 1);
    }
    if (tid == 0) {
        int g = 0;
        for (int l = 0; l < n; ++l) g += hit[l];
        n_groups = g;
    }
    __syncthreads();
    const int ng = n_groups;
    if (tid == 0) {
        int32_t *vn = tab.vn;
        vn[s] = n;
        vn[Sr + s] = ng;
        vn[2 * Sr + s] = n;
    }
    int32_t *gi = tab.gidx + b;
    for (int i = tid; i < n; i += kSnThreads) {
        gi[i] = idx[i];
        if (group_index) group_index[b + i] = idx[i];
    }
    // sig / sig.sum(dim = 0)
    for (int j = tid; j < n; j += kSnThreads) {
        float sum = 0.f;
        for (int i = 0; i < n; ++i) sum += sig_of(D[i * n + j], th, tau);
        cs[j] = sum;
        if (gs.cs) gs.cs[j] = sum;
    }
    __syncthreads();
    for (int q = tid; q < n * n; q += kSnThreads) {
        const float sg = sig_of(D[q], th, tau);
        sn[q] = sg / cs[q % n];
        if (gs.sig) gs.sig[q] = sg;
    }
    __syncthreads();
    // v' = (v_rel - v_soft) + v_soft, v_soft = v_rel @ sig_norm: every channel
    for (int q = tid; q < CH * T * n; q += kSnThreads) {
        const int j = q % n, t = (q / n) % T, ch = q / (n * T);
        const float *x = (ch ? v0 : p0) + t * n;
        float soft = 0.f;
        for (int i = 0; i < n; ++i) soft = fmaf(x[i], sn[i * n + j], soft);
        (ch ? v2 : p2)[t * n + j] = (x[j] - soft) + soft;
    }
    __syncthreads();
    // the group means of v', pedestrians in ascending order
    for (int q = tid; q < CH * T * ng; q += kSnThreads) {
        const int g = q % ng, t = (q / ng) % T, ch = q / (ng * T);
        const float *x = (ch ? v2 : p2) + t * n;
        float sum = 0.f;
        for (int i = 0; i < n; ++i)
            if (idx[i] == g) sum += x[i];
        (ch ? v1 : p1)[t * ng + g] = sum / (float)cnt[g];
    }
    if (gs.cnt)
        for (int g = tid; g < ng; g += kSnThreads) gs.cnt[g] = cnt[g];
}

// ---- mix: one workgroup per pedestrian; po (k, 3 Nr, S): the three passes' outputs, pass 1's on the group rows
__global__ __launch_bounds__(kMixThreads) void gp_mix(GpTab c, GpWeights p, const float *__restrict__ po,
                                                      float *__restrict__ out, int graph_layout) {
    extern __shared__ float mix_lds[];  // the three passes' (S, k) as they are, and after the PReLU
    const int k = p.k, S = p.S, Sk = S * k, tid = threadIdx.x;
    float *raw = mix_lds, *act = mix_lds + 3 * Sk;
    const int64_t r = blockIdx.x, Nr = c.Nr;
    const int s = c.off ? scene_of_row(c.off, c.Sr, r) : 0;
    const int64_t b = c.off ? c.off[s] : 0;
    const int64_t e = c.off ? c.off[s + 1] : Nr;
    const bool ok = r >= b && r < e && c.sq[s] >= 0;
    int64_t row[3] = {r, r, 2 * Nr + r};
    if (ok) row[1] = Nr + b + c.gidx[r];  // unpool: the group's row
    const float a = p.mix_a[0];
    for (int q = tid; q < 3 * Sk; q += kMixThreads) {
        const int m = q / Sk, ss = (q % Sk) / k, t = q % k;
        const float x = ok ? po[((int64_t)t * 3 * Nr + row[m]) * S + ss] : __builtin_nanf("");
        raw[q] = x;
        act[q] = prelu(x, a);
    }
    __syncthreads();
    for (int o = tid; o < Sk; o += kMixThreads) {
        const float *w = p.mix_w + (int64_t)o * 3 * Sk;
        float acc = p.mix_b[o];
        for (int q = 0; q < 3 * Sk; ++q) acc = fmaf(w[q], act[q], acc);
        const float y = ((raw[o] + raw[Sk + o]) + raw[2 * Sk + o]) / 3.0f + acc;
        const int ss = o / k, t = o % k;
        if (graph_layout)
            out[((int64_t)ss * k + t) * Nr + r] = y;
        else
            out[((int64_t)t * Nr + r) * S + ss] = y;
    }
}

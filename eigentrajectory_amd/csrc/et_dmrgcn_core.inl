// et_dmrgcn_core.inl -- what the DMRGCN inference unit (et_dmrgcn.hip) and the training unit (et_dmrgcn_train.hip) share,
// #included inside their anonymous namespaces after et_scene_helpers.inl and et_stgcnn_core.inl: the dimensions and the arena
// size, the bin of a distance, the two sources of a scene (graph form, scenes form) and the parameter check.  The statements
// are et_dmrgcn.hip's, moved here unchanged (its header comment describes them).
static_assert(kSnThreads == kSgThreads, "scene_v strides by the workgroup size of the scene kernels");

constexpr int kDmBins = ET_DMRGCN_BINS;
constexpr int kDmRB = 2 * kDmBins;  // (relation, bin) graphs per time row
constexpr int kDmRows = 2;          // contracted rows per lane
constexpr float kDmLast = 1e10f;    // closes the last bin (dmrgcn.py:29)

struct DmDims {
    int K, k, S, n_st, n_tp;
    int qpp;  // floats per pedestrian of each of the three rotating buffers
};

__host__ __device__ inline DmDims dm_dims_of(const et_dmrgcn_params &p) {
    DmDims d{p.seq_len, p.pred_seq_len, p.output_feat, p.n_stgcn, p.n_tpcnn, 0};
    int q = d.S * d.K;                             // x, y; the tpcnn planes (k,S,n) are smaller
    if (q < kDmRB * 2) q = kDmRB * 2;              // first block: one time row of 10 (1 + 1) contracted rows at least
    if (d.n_st > 1 && kDmRB * (d.S + 1) > q) q = kDmRB * (d.S + 1);  // later blocks: C_in = S
    d.qpp = q;
    return d;
}

__host__ __device__ inline int64_t dm_arena_per_ped(const DmDims &d) { return (2 + kDmRB) * d.K + 3 * (int64_t)d.qpp; }

// the bin of a distance: b with s[b] < dist < s[b+1] (s[5] = 1e10), or -1; s[0] >= 0, so 0 is in no bin
__device__ __forceinline__ int bin_of(float dist, const float *s) {
    int bin = -1;
#pragma unroll
    for (int b = 0; b < kDmBins; ++b) {
        const float hi = b + 1 < kDmBins ? s[b + 1] : kDmLast;
        if (dist > s[b] && dist < hi) bin = b;
    }
    return bin;
}

// one scene as the bridge hands it over: v (1,1,K,N), a (1,2,K,N,N) read as given
struct GraphSrc {
    static constexpr bool kComputed = false;
    const float *v, *a;
    float *out;  // (1,S,k,N) raw network output
    __device__ void load(float *u, int64_t b, int n, int K, float *red) const { scene_v(u, v, nullptr, nullptr, 0, b, n, K, red); }
    // the two distances of row w and column vv of time row t: [0] displacement, [1] distance
    __device__ void pair(int t, int w, int vv, int n, int K, const float *, const float *, float, float, float *dist) const {
        const int64_t at = ((int64_t)t * n + w) * n + vv;
        dist[0] = a[at];
        dist[1] = a[(int64_t)K * n * n + at];
    }
    // the last tpcnn block's (t, s, w) -> permute (predictor.py:96) -> (1,S,k,N)
    __device__ void store(int t, int s, int w, int k, int, int n, int64_t, float val) const {
        out[((int64_t)s * k + t) * n + w] = val;
    }
};

// a split: C_obs (k,N), nrm (4,N), scenes by offsets; the distances formed from u and rel
struct ScenesSrc {
    static constexpr bool kComputed = true;
    const float *C_obs, *nrm;
    int64_t N;
    float *out;  // (k,N,S) C_pred_refine
    __device__ void load(float *u, int64_t b, int n, int K, float *red) const { scene_v(u, nullptr, C_obs, nrm, N, b, n, K, red); }
    __device__ void pair(int t, int, int vv, int n, int, const float *u, const float *rel, float uw, float rw, float *dist) const {
        dist[0] = fabsf(rw - rel[t * n + vv]);
        dist[1] = fabsf(uw - u[t * n + vv]);
    }
    // (t, s, w) -> (1,S,k,N) -> the post-hook's permute(0,2,3,1) (bridge.py:40): (k,N,S)
    __device__ void store(int t, int s, int w, int, int S, int, int64_t b, float val) const {
        out[((int64_t)t * N + b + w) * S + s] = val;
    }
};

static int dm_check_params(const et_dmrgcn_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->input_feat != 1 || p->kernel_size != 3 || p->pred_seq_len < 1 || p->pred_seq_len > ET_MAX_K ||
        p->seq_len != p->pred_seq_len + 2 || p->output_feat < 1 || p->output_feat > kSgMaxS || p->n_stgcn < 1 ||
        p->n_stgcn > ET_DMRGCN_MAX_STGCN || p->n_tpcnn < 1 || p->n_tpcnn > ET_DMRGCN_MAX_TPCNN)
        return ET_ERR_UNSUPPORTED;
    for (int r = 0; r < 2; ++r) {  // ascending, so that a distance is in at most one bin (NaN fails every comparison)
        if (!(p->split[r][0] >= 0.f) || !(p->split[r][kDmBins - 1] < kDmLast)) return ET_ERR_UNSUPPORTED;
        for (int b = 0; b + 1 < kDmBins; ++b)
            if (!(p->split[r][b] < p->split[r][b + 1])) return ET_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < p->n_stgcn; ++i) {
        const et_dmrgcn_layer &l = p->st_dmrgcns[i];
        if (!l.gcn_w[0] || !l.gcn_w[1] || !l.gcn_b[0] || !l.gcn_b[1] || !l.tcn_prelu || !l.tcn_w || !l.tcn_b || !l.prelu)
            return ET_ERR_INVALID_ARG;
        const bool res = (i == 0 ? p->input_feat : p->output_feat) != p->output_feat;  // dmrgcn.py:212-217
        if (res != (l.res_w != nullptr) || (res && !l.res_b)) return ET_ERR_INVALID_ARG;
    }
    for (int j = 0; j < p->n_tpcnn; ++j) {
        const et_dmrgcn_tpcnn &t = p->tpcnns[j];
        for (int m = 0; m < 2; ++m)
            if (!t.conv_w[m] || !t.conv_b[m] || !t.conv_a[m]) return ET_ERR_INVALID_ARG;
        if (!t.gta_w || !t.gta_b || !t.gta_a) return ET_ERR_INVALID_ARG;
        const bool res = j == 0;  // predictor.py:37-42: K != k in the first block only
        if (res != (t.res_w != nullptr) || (res && !t.res_b)) return ET_ERR_INVALID_ARG;
    }
    return ET_OK;
}

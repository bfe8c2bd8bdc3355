// et_graphtern_core.inl -- what the Graph-TERN inference unit (et_graphtern.hip) and the training unit
// (et_graphtern_train.hip) share, #included inside their anonymous namespaces after et_scene_helpers.inl and
// et_stgcnn_core.inl: the dimensions and the arena size, the two sources of a scene (graph form, scenes form), the
// replicate-padded 3x3 convolution, the four relations of a pair and the parameter check.  The statements are
// et_graphtern.hip's, moved here unchanged (its header comment describes them).
static_assert(kSnThreads == kSgThreads, "scene_v strides by the workgroup size of the scene kernels");

constexpr int kGtRel = 4;      // relations per time row
constexpr int kGtHidden = 16;  // model.py:229
constexpr int kGtRows = 2;     // contracted rows per lane

struct GtDims {
    int T, k, S, n_gcn, n_cnn;
    int qpp;  // floats per pedestrian of each of the three rotating buffers
};

__host__ __device__ inline GtDims gt_dims_of(const et_graphtern_params &p) {
    GtDims d{p.seq_len, p.pred_seq_len, p.n_smpl, p.n_epgcn, p.n_epcnn, 0};
    int q = kGtHidden * d.T;                                      // the st_mrgcn planes and the first epcnn input
    if (d.k * d.S > q) q = d.k * d.S;                             // the last epcnn block's (k,S,n) output
    if (d.n_gcn > 1 && kGtRel * (kGtHidden + 1) > q) q = kGtRel * (kGtHidden + 1);  // later blocks: C_in = 16, one time row
    d.qpp = q;
    return d;
}

__host__ __device__ inline int64_t gt_arena_per_ped(const GtDims &d) { return (2 + kGtRel) * d.T + 3 * (int64_t)d.qpp; }

// one scene as the bridge hands it over: S_obs (1,2,T,N,1) = [abs, rel], both read as given
struct GraphSrc {
    static constexpr bool kComputed = false;
    const float *s_obs;
    __device__ void load(float *u, float *rel, int64_t, int n, int T, float *) const {
        for (int i = threadIdx.x; i < T * n; i += kSgThreads) {
            u[i] = s_obs[i];
            rel[i] = s_obs[(int64_t)T * n + i];
        }
    }
};

// a split: C_obs (k,N), nrm (4,N), scenes by offsets; rel formed from u
struct ScenesSrc {
    static constexpr bool kComputed = true;
    const float *C_obs, *nrm;
    int64_t N;
    __device__ void load(float *u, float *, int64_t b, int n, int T, float *red) const {
        scene_v(u, nullptr, C_obs, nrm, N, b, n, T, red);
    }
};

// 3x3 convolution with REPLICATE padding over a (H, W = n) plane: entry (channel i, row h, column w) of `in` is at
// in[(i ci + h ch) n + w] -> output channel o at (h, w)
__device__ __forceinline__ float conv33_replicate(const float *in, int Cin, int ci, int H, int ch, int n, const float *W,
                                                  const float *bias, int o, int h, int w) {
    float acc = bias[o];
    int hh[3], ww[3];
#pragma unroll
    for (int dd = 0; dd < 3; ++dd) {
        hh[dd] = min(max(h + dd - 1, 0), H - 1) * ch;
        ww[dd] = min(max(w + dd - 1, 0), n - 1);
    }
    for (int i = 0; i < Cin; ++i) {
        const float *wi = W + ((int64_t)o * Cin + i) * 9;
        const float *pi = in + (int64_t)i * ci * n;
#pragma unroll
        for (int dh = 0; dh < 3; ++dh)
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) acc = fmaf(wi[dh * 3 + dw], pi[(int64_t)hh[dh] * n + ww[dw]], acc);
    }
    return acc;
}

// the four relations of a pair from its two fp32 distances: [A_abs, A_rel, 1/A_abs, 1/A_rel], 0 where the distance is 0
__device__ __forceinline__ void gt_relations(float a_abs, float a_rel, float *A) {
    A[0] = a_abs;
    A[1] = a_rel;
    A[2] = a_abs == 0.f ? 0.f : 1.0f / a_abs;
    A[3] = a_rel == 0.f ? 0.f : 1.0f / a_rel;
}

static int gt_check_params(const et_graphtern_params *p) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->input_feat != 1 || p->hidden_feat != kGtHidden || p->pred_seq_len < 1 || p->pred_seq_len > ET_MAX_K ||
        p->seq_len != p->pred_seq_len + 2 || p->n_smpl < 1 || p->n_smpl > kSgMaxS || p->n_epgcn < 1 ||
        p->n_epgcn > ET_GRAPHTERN_MAX_EPGCN || p->n_epcnn < 2 || p->n_epcnn > ET_GRAPHTERN_MAX_EPCNN)
        return ET_ERR_UNSUPPORTED;
    for (int i = 0; i < p->n_epgcn; ++i) {
        const et_graphtern_layer &l = p->tp_mrgcns[i];  // (l.prelu is carried for completeness: the network never applies it)
        if (!l.gcn_w || !l.gcn_b || !l.tcn_prelu || !l.tcn_w || !l.tcn_b) return ET_ERR_INVALID_ARG;
        const bool res = i == 0;  // stmrgcn.py:44-47: input_feat != 16 in the first block only
        if (res != (l.res_w != nullptr) || (res && !l.res_b)) return ET_ERR_INVALID_ARG;
    }
    for (int j = 0; j < p->n_epcnn; ++j) {
        const et_graphtern_epcnn &e = p->tpcnns[j];
        if (!e.tpcn_w || !e.tpcn_b || !e.tpcn_a || !e.cpcn_w || !e.cpcn_b || !e.cpcn_a) return ET_ERR_INVALID_ARG;
        const bool rest = j == 0;                                              // stmrgcn.py:91: T != k in the first block
        const bool resc = j + 1 == p->n_epcnn && p->n_smpl != kGtHidden;       // stmrgcn.py:88: 16 != S in the last block
        if (rest != (e.rest_w != nullptr) || (rest && !e.rest_b)) return ET_ERR_INVALID_ARG;
        if (resc != (e.resc_w != nullptr) || (resc && !e.resc_b)) return ET_ERR_INVALID_ARG;
    }
    return ET_OK;
}

// et_mlp_chain.inl -- what et_mlp.hip (inference) and et_mlp_train.hip (training) share: the launch structures, the bodies of
// the chain kernel and of the pooling kernel, and the parameter checks.  #included inside namespace et { namespace { ... } } after
// et_scene_helpers.inl.  mlp_chain_kernel<MlLaunch> is the inference kernel (et_mlp.hip's header describes it);
// mlp_chain_kernel<MlTrainLaunch> additionally stores every hidden layer's activations (a compile-time variant: the
// inference kernel's code has no switch for it).  nonlocal_pool_kernel<AtLaunch> / <AtTrainLaunch> likewise: the training form
// also stores the features it gathered.

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMlThreads = kSnThreads;
constexpr int kMlWaves = kMlThreads / kWave;
constexpr int kMlRows = 16;
constexpr int kMlStride = ET_MLP_MAX_WIDTH + 4;  // row r of an image starts at bank 4 r: the 64 lanes of an A read hit 64 banks
constexpr int kMlLdsBytes = 2 * kMlRows * kMlStride * 4;
constexpr int kMlMaxJobs = 3;

struct MlSrc {
    const float *p;
    int width;
    int64_t rs, cs;  // element (row, c) = p[row * rs + c * cs]
};

struct MlJob {
    int n_layers, n_src;
    int widths[ET_MLP_MAX_LAYERS + 1];
    const float *w[ET_MLP_MAX_LAYERS], *b[ET_MLP_MAX_LAYERS];
    MlSrc src[3];
    float *out;
    int out_s;  // element (row, col) of the last layer at out[(col / out_s) N out_s + row out_s + col % out_s]
};

// the scene form's first launch: the workgroups of job 1 (encoder_dest) centre their rows
struct MlScene {
    const float *C_obs, *nrm;
    const int32_t *off;
    int n_scenes, k;
    float *pos;  // (N, 2) obs_ori
    float *gin;  // (k + 2, N) or null
};

struct MlLaunch {
    static constexpr bool kSave = false;
    MlJob job[kMlMaxJobs];
    MlScene sc;
    int64_t N;
};

// the training forward's launch: save[j][l] receives the output of layer l of job j, (N, widths[l + 1]) row-major, for
// every layer but the last
struct MlTrainLaunch : MlLaunch {
    static constexpr bool kSave = true;
    float *save[kMlMaxJobs][ET_MLP_MAX_LAYERS];
};

// the range [b, e) of row r: its scene, or all rows; offsets outside [0, N] are clamped
__device__ __forceinline__ void range_of_row(const int32_t *off, int n_scenes, int64_t N, int64_t r, int &s, int64_t &b,
                                             int64_t &e) {
    if (!off) {
        s = 0, b = 0, e = N;
        return;
    }
    s = scene_of_row(off, n_scenes, r);
    b = min((int64_t)max(off[s], 0), N);
    e = min((int64_t)max(off[s + 1], 0), N);
    if (e < b) e = b;
}

__device__ __forceinline__ float gather(const MlSrc *src, int n_src, int64_t row, int c) {
    for (int s = 0; s < n_src; ++s) {
        if (c < src[s].width) return src[s].p[row * src[s].rs + c * src[s].cs];
        c -= src[s].width;
    }
    return 0.f;
}

template <class Launch>
__global__ __launch_bounds__(kMlThreads) void mlp_chain_kernel(Launch L) {
    extern __shared__ float lds[];
    __shared__ float red[2 * kMlWaves];
    const MlJob &J = L.job[blockIdx.y];
    const int64_t N = L.N, row0 = (int64_t)blockIdx.x * kMlRows;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float *cur = lds, *nxt = lds + kMlRows * kMlStride;

    if (L.sc.nrm && blockIdx.y == 1) {
        // obs_ori of the tile's rows: a scene's mean once per run of rows of that scene, in scene_v's order
        const MlScene &Sc = L.sc;
        int prev = -1;
        float mx = 0.f, my = 0.f;
        for (int i = 0; i < kMlRows; ++i) {
            const int64_t row = row0 + i;
            if (row >= N) {
                if (tid < 4) cur[i * kMlStride + tid] = 0.f;
                continue;
            }
            int s;
            int64_t b, e;
            range_of_row(Sc.off, Sc.n_scenes, N, row, s, b, e);
            if (s != prev) {
                prev = s;
                const int n = (int)(e - b);
                float sx = 0.f, sy = 0.f;
                for (int w = tid; w < n; w += kMlThreads) {
                    sx += Sc.nrm[b + w];
                    sy += Sc.nrm[N + b + w];
                }
                for (int o = 32; o > 0; o >>= 1) {
                    sx += __shfl_xor(sx, o);
                    sy += __shfl_xor(sy, o);
                }
                __syncthreads();  // the previous scene's partials have been read
                if (lane == 0) {
                    red[wave] = sx;
                    red[kMlWaves + wave] = sy;
                }
                __syncthreads();
                mx = 0.f, my = 0.f;
                for (int w = 0; w < kMlWaves; ++w) {
                    mx += red[w];
                    my += red[kMlWaves + w];
                }
                mx = mx / (float)n;
                my = my / (float)n;
            }
            if (tid == 0) {
                const float ox = Sc.nrm[row] - mx, oy = Sc.nrm[N + row] - my;
                float *c = cur + i * kMlStride;
                c[0] = ox, c[1] = oy, c[2] = 0.f, c[3] = 0.f;
                Sc.pos[row * 2] = ox, Sc.pos[row * 2 + 1] = oy;
                if (Sc.gin) Sc.gin[(int64_t)Sc.k * N + row] = ox, Sc.gin[(int64_t)(Sc.k + 1) * N + row] = oy;
            }
            if (Sc.gin)
                for (int c = tid; c < Sc.k; c += kMlThreads) Sc.gin[(int64_t)c * N + row] = Sc.C_obs[(int64_t)c * N + row];
        }
    } else {
        const int in = J.widths[0], inp = (int)up4(in);
        for (int idx = tid; idx < kMlRows * inp; idx += kMlThreads) {
            const int i = idx / inp, c = idx - i * inp;
            const int64_t row = row0 + i;
            cur[i * kMlStride + c] = (row < N && c < in) ? gather(J.src, J.n_src, row, c) : 0.f;
        }
    }
    __syncthreads();

    const int col = lane & 15, kq = lane >> 4;
    for (int l = 0; l < J.n_layers; ++l) {
        const int in = J.widths[l], out = J.widths[l + 1];
        const bool last = l + 1 == J.n_layers;
        const float *__restrict__ W = J.w[l], *__restrict__ B = J.b[l];
        const int nblk = (out + 15) / 16;
        const float *ar = cur + col * kMlStride + kq;  // A: row `col` of the tile, k = k0 + kq
        for (int blk = wave; blk < nblk; blk += 2 * kMlWaves) {
            const int j0 = blk * 16 + col, j1 = (blk + kMlWaves) * 16 + col;
            const bool ok0 = j0 < out, ok1 = j1 < out;
            const float *w0 = W + (int64_t)(ok0 ? j0 : 0) * in + kq, *w1 = W + (int64_t)(ok1 ? j1 : 0) * in + kq;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const int inm = in & ~3;  // whole k steps; the weights of a block past `out` are read from row 0 and dropped
            int k0 = 0;
            for (; k0 + 16 <= inm; k0 += 16) {  // four steps' operands in flight, then the products in k order
                float a[4], t0[4], t1[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = ar[k0 + 4 * u], t0[u] = w0[k0 + 4 * u], t1[u] = w1[k0 + 4 * u];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], ok0 ? t0[u] : 0.f, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], ok1 ? t1[u] : 0.f, acc1, 0, 0, 0);
                }
            }
            for (; k0 < inm; k0 += 4) {
                const float a = ar[k0], t0 = w0[k0], t1 = w1[k0];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok0 ? t0 : 0.f, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok1 ? t1 : 0.f, acc1, 0, 0, 0);
            }
            if (inm < in) {  // the last, partial step: the image holds zeros in columns in .. inp
                const bool kok = inm + kq < in;
                const float a = ar[inm];
                const float b0 = (ok0 && kok) ? w0[inm] : 0.f, b1 = (ok1 && kok) ? w1[inm] : 0.f;
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = h ? j1 : j0;
                const bool ok = h ? ok1 : ok0;
                if ((h ? blk + kMlWaves : blk) >= nblk) continue;
                const f32x4 acc = h ? acc1 : acc0;
                const float bias = ok ? B[j] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 4 * kq + r;
                    float v = acc[r] + bias;
                    if (!last) {
                        v = v < 0.f ? 0.f : v;  // ReLU; a NaN stays a NaN
                        nxt[i * kMlStride + j] = ok ? v : 0.f;  // j < 16 nblk <= ET_MLP_MAX_WIDTH: inside the row
                        if constexpr (Launch::kSave) {
                            if (ok && row0 + i < N) L.save[blockIdx.y][l][(row0 + i) * out + j] = v;
                        }
                    } else if (ok && row0 + i < N) {
                        J.out[(int64_t)(j / J.out_s) * N * J.out_s + (row0 + i) * J.out_s + j % J.out_s] = v;
                    }
                }
            }
        }
        __syncthreads();
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
}

constexpr int kAtRows = kMlWaves;  // rows per workgroup of the pooling kernel, one per wavefront
constexpr int kAtLdsBytes = kAtRows * ET_MLP_MAX_RANGE * 4;

struct AtLaunch {
    static constexpr bool kKeep = false;
    const float *theta, *phi, *g;  // (N, D), (N, D), (N, F)
    int D, F, n_src;
    MlSrc src[3];       // feat (N, F), gathered
    const float *mask;  // (N, N) or null
    const int32_t *off;
    int n_scenes;
    int64_t N;
    float *out;  // (N, F)
};

// the training forward's launch: feat_keep (N, F) or null receives the gathered feat (round 0's concatenation)
struct AtTrainLaunch : AtLaunch {
    static constexpr bool kKeep = true;
    float *feat_keep;
};

template <class Launch>
__global__ __launch_bounds__(kMlThreads) void nonlocal_pool_kernel(Launch A) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t N = A.N, row = (int64_t)blockIdx.x * kAtRows + wave;
    float *lg = lds + wave * ET_MLP_MAX_RANGE;
    int s = 0;
    int64_t b = 0, e = 0;
    if (row < N) range_of_row(A.off, A.n_scenes, N, row, s, b, e);
    const bool fits = e - b <= ET_MLP_MAX_RANGE;
    const int n = (row < N && fits) ? (int)(e - b) : 0;
    const int D = A.D, F = A.F;

    const float *th = A.theta + row * D;
    float m = -INFINITY;
    for (int j = lane; j < n; j += kWave) {
        const float *ph = A.phi + (b + j) * D;
        float acc = 0.f;
        for (int c = 0; c < D; ++c) acc = fmaf(th[c], ph[c], acc);
        lg[j] = acc;
        m = fmaxf(m, acc);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float z = 0.f;
    for (int j = lane; j < n; j += kWave) {
        const float ex = expf(lg[j] - m);
        lg[j] = ex;
        z += ex;
    }
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
    float l1 = 0.f;
    for (int j = lane; j < n; j += kWave) {
        float w = lg[j] / z;
        if (A.mask) w = w * A.mask[row * N + b + j];
        lg[j] = w;
        l1 += fabsf(w);
    }
    for (int o = 32; o > 0; o >>= 1) l1 += __shfl_xor(l1, o);
    const float den = fmaxf(l1, 1e-12f);
    for (int j = lane; j < n; j += kWave) lg[j] = lg[j] / den;
    __syncthreads();  // (every wavefront gets here: no early exit above) the row's weights are in LDS
    if (row < N) {
        for (int c = lane; c < F; c += kWave) {
            float acc = 0.f;
            for (int j = 0; j < n; ++j) acc = fmaf(lg[j], A.g[(b + j) * F + c], acc);
            if constexpr (Launch::kKeep) {  // (the training entries refuse a range that does not fit)
                const float fv = gather(A.src, A.n_src, row, c);
                A.out[row * F + c] = acc + fv;
                if (A.feat_keep) A.feat_keep[row * F + c] = fv;
            } else {
                A.out[row * F + c] = fits ? acc + gather(A.src, A.n_src, row, c) : __builtin_nanf("");
            }
        }
    }
}

static int chain_check(const et_mlp_chain &c, int in, int out) {
    if (c.n_layers < 2 || c.n_layers > ET_MLP_MAX_LAYERS) return ET_ERR_UNSUPPORTED;
    for (int i = 0; i <= c.n_layers; ++i)
        if (c.widths[i] < 1 || c.widths[i] > ET_MLP_MAX_WIDTH) return ET_ERR_UNSUPPORTED;
    if (c.widths[0] != in || c.widths[c.n_layers] != out) return ET_ERR_UNSUPPORTED;
    for (int i = 0; i < c.n_layers; ++i)
        if (!c.w[i] || !c.b[i]) return ET_ERR_INVALID_ARG;
    return ET_OK;
}

// the feature width: ftraj | dest features | initial_pos
static int feat_width(const et_mlp_params &p) { return 2 * p.fdim + p.pos_width; }

static int ml_check_params(const et_mlp_params *p, bool pecnet) {
    if (!p) return ET_ERR_INVALID_ARG;
    if (p->fdim < 1 || p->fdim > ET_MLP_MAX_WIDTH || p->out_width < 1 || p->pos_width != (pecnet ? 2 : 0) ||
        p->nonlocal_pools < 0 || p->nonlocal_pools > (pecnet ? ET_MLP_MAX_POOLS : 0))
        return ET_ERR_UNSUPPORTED;
    const int F = feat_width(*p);
    if (F > ET_MLP_MAX_WIDTH) return ET_ERR_UNSUPPORTED;
    int rc = chain_check(p->encoder_past, p->encoder_past.widths[0], p->fdim);
    if (rc == ET_OK) rc = chain_check(p->encoder_dest, p->encoder_dest.widths[0], p->fdim);
    if (rc == ET_OK) rc = chain_check(p->predictor, F, p->out_width);
    if (rc == ET_OK && p->nonlocal_pools > 0) {
        if (p->non_local_dim < 1) return ET_ERR_UNSUPPORTED;
        rc = chain_check(p->non_local_theta, F, p->non_local_dim);
        if (rc == ET_OK) rc = chain_check(p->non_local_phi, F, p->non_local_dim);
        if (rc == ET_OK) rc = chain_check(p->non_local_g, F, F);
    }
    return rc;
}

static void job_of(MlJob &j, const et_mlp_chain &c, float *out, int out_s) {
    j.n_layers = c.n_layers;
    for (int i = 0; i <= c.n_layers; ++i) j.widths[i] = c.widths[i];
    for (int i = 0; i < c.n_layers; ++i) j.w[i] = c.w[i], j.b[i] = c.b[i];
    j.out = out;
    j.out_s = out_s;
}

static MlSrc rows_of(const float *p, int width) { return MlSrc{p, width, width, 1}; }

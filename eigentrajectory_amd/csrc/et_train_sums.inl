// et_train_sums.inl -- the fixed-order sums, the small backward pieces and the tail (the scenes' gradient reduce, the
// backward entries' argument check) that the scene training units share (et_stgcnn_train.hip, et_dmrgcn_train.hip),
// #included inside their anonymous namespaces after et_stgcnn_core.inl (kSgThreads).  The statements are
// et_stgcnn_train.hip's, moved here unchanged; its header comment ("wave_sum") gives the order of every sum.
constexpr int kTrWaves = kSgThreads / kWave;

// header comment: "wave_sum".  Called by all 64 lanes of a wavefront with the same count; every lane gets the sum.
template <class F>
__device__ __forceinline__ float wave_sum(int count, F f) {
    float s = 0.f;
    for (int p = threadIdx.x & (kWave - 1); p < count; p += kWave) s += f(p);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// dst[e] = wave_sum(count, f(e, .)) for e < E: wavefront w takes e = w, w + 4, ...
template <class F>
__device__ __forceinline__ void wave_sums(float *dst, int E, int count, F f) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int e = threadIdx.x / kWave; e < E; e += kTrWaves) {
        const float s = wave_sum(count, [&](int p) { return f(e, p); });
        if (lane == 0) dst[e] = s;
    }
}

__device__ __forceinline__ float slope(float x, const float *a) { return x > 0.f ? 1.f : a[0]; }
__device__ __forceinline__ float neg_part(float x) { return x > 0.f ? 0.f : x; }

// d in[i,hh,ww] of a 3x3 convolution with padding 1: sum over o ascending, then the taps row-major
__device__ __forceinline__ float conv33_dx(const float *dY, int Cout, int Cin, int S, int n, const float *W, int i, int hh,
                                           int ww) {
    float acc = 0.f;
    for (int o = 0; o < Cout; ++o) {
        const float *wi = W + ((int64_t)o * Cin + i) * 9;
        const float *po = dY + (int64_t)o * S * n;
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
            const int h = hh - dh + 1;
            if (h < 0 || h >= S) continue;
#pragma unroll
            for (int dw = 0; dw < 3; ++dw) {
                const int w = ww - dw + 1;
                if (w < 0 || w >= n) continue;
                acc = fmaf(wi[dh * 3 + dw], po[h * n + w], acc);
            }
        }
    }
    return acc;
}

// T sums at once, one wavefront: sum t is wave_sum(count, f(., t)) term for term (the same lane chains, the same butterfly);
// f(p, t) of the T taps of one position share their loads, and T chains hide each other's latency
template <int T, class F>
__device__ __forceinline__ void wave_sum_taps(float *dst, int count, F f) {
    float s[T];
#pragma unroll
    for (int t = 0; t < T; ++t) s[t] = 0.f;
    for (int p = threadIdx.x & (kWave - 1); p < count; p += kWave) {
#pragma unroll
        for (int t = 0; t < T; ++t) s[t] += f(p, t);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float v = s[t];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & (kWave - 1)) == 0) dst[t] = v;
    }
}

// grads[e] = the scenes' partials (scene s's G floats at partials + s * G) in ascending order, the first live one copied
// (et_stgcnn_train.hip's header comment: "scenes"); a scene is live with 1 to max_n pedestrians; no live scene: +0
__global__ __launch_bounds__(kSgThreads) void scene_grad_reduce_kernel(const float *__restrict__ partials, int64_t G,
                                                                       int max_n, const int32_t *__restrict__ off,
                                                                       int n_scenes, int64_t N, float *grads) {
    const int64_t i = (int64_t)blockIdx.x * kSgThreads + threadIdx.x;
    if (i >= G) return;
    float acc = 0.f;
    bool first = true;
    for (int s = 0; s < n_scenes; ++s) {
        const int64_t n = off ? (int64_t)off[s + 1] - off[s] : N;
        if (n < 1 || n > max_n) continue;
        const float v = partials[s * G + i];
        acc = first ? v : acc + v;
        first = false;
    }
    grads[i] = acc;
}

// the last launch of a backward pass: ns scenes' partials -> grads (no scene when N = 0: every gradient +0)
static int scene_grad_reduce(const float *partials, int64_t G, int max_n, const int32_t *off, int ns, int64_t N, float *grads,
                             et_stream_t stream) {
    hipLaunchKernelGGL(scene_grad_reduce_kernel, dim3((unsigned)ceil_div(G, kSgThreads)), dim3(kSgThreads), 0,
                       (hipStream_t)stream, partials, G, max_n, off, N > 0 ? ns : 0, N, grads);
    ET_LAUNCH_CHECK();
    return ET_OK;
}

// a training workspace as its layout sizes it, in floats
static inline bool train_ws_fits(int64_t total_floats, const void *workspace, size_t workspace_bytes) {
    return workspace && workspace_bytes >= (size_t)total_floats * 4;
}

// The arguments of an et_*_backward_scenes / _graph entry point (the graph form: no offsets, n_scenes = 0), checked once
// its parameters have passed: N rows in range, max_n the most that may come as one scene, grads of at least need floats,
// d_out wherever there is a row.  -> ET_OK or ET_ERR_INVALID_ARG; the workspace is the caller's next check.
static inline int backward_args_status(int64_t N, const int32_t *scene_offsets, int n_scenes, int max_n, const float *d_out,
                                       const float *grads, int64_t grads_floats, int64_t need) {
    if (N < 0 || N > INT32_MAX || n_scenes < 0 || !grads || grads_floats < need) return ET_ERR_INVALID_ARG;
    if (scene_offsets ? (n_scenes == 0 && N != 0) : N > max_n) return ET_ERR_INVALID_ARG;
    return N > 0 && !d_out ? ET_ERR_INVALID_ARG : ET_OK;
}

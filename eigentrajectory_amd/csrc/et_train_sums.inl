// et_train_sums.inl -- what the three scene training units hold once (et_stgcnn_train.hip, et_dmrgcn_train.hip,
// et_graphtern_train.hip): the fixed-order sums and the small backward pieces, the skeleton of a training workspace (the
// layout array and its tail, a scene's fields, the et_*_train_layout copy-out), the preamble of a scene kernel (its row range,
// the NaN rows of a scene over the cap), the weight-gradient kernels' round robin (DMRGCN, Graph-TERN) and the tail of a
// backward pass (the scenes' gradient reduce, the backward entries' argument check).  #included inside the unit's anonymous
// namespace after et_stgcnn_core.inl (kSgThreads) and after the unit's own field enum, whose F_PER (= the number of
// per-pedestrian fields, which come first), F_PARTIALS, F_GRADS, F_TOTAL and F_COUNT this file reads.  The statements are
// the units', moved here unchanged; et_stgcnn_train.hip's header comment ("wave_sum") gives the order of every sum.
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

// dst[0] = wave_sum(count, f): one wavefront, lane 0 writes
template <class F>
__device__ __forceinline__ void sum_to(float *dst, int count, F f) {
    const float s = wave_sum(count, f);
    if ((threadIdx.x & (kWave - 1)) == 0) dst[0] = s;
}

// the items of one segment of the gradient buffer, round robin over a scene's Waves weight-gradient wavefronts: item g of
// the whole list (start = the items of the segments before) goes to wavefront g % Waves; f(it) for this wavefront's (wv)
template <int Waves, class F>
__device__ __forceinline__ void segment(int &start, int count, int wv, F f) {
    const int first = (wv - start % Waves + Waves) % Waves;
    for (int it = first; it < count; it += Waves) f(it);
    start += count;
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

// a training workspace's offsets in floats, as et_*_train_layout hands them out: the unit's field enum indexes them
struct TrainLayout {
    int64_t o[F_COUNT];
};

// the tail of every layout: `per` floats per pedestrian, the scenes' gradient partials (G floats each) from `partials` on
__host__ __device__ inline void layout_tail(TrainLayout &L, int64_t per, int64_t partials, int64_t G, int64_t n_scenes) {
    L.o[F_PER] = per;
    L.o[F_PARTIALS] = partials;
    L.o[F_GRADS] = G;
    L.o[F_TOTAL] = L.o[F_PARTIALS] + n_scenes * L.o[F_GRADS];
}

// the body of an et_*_train_layout entry point once its parameters have passed; make() -> the TrainLayout
template <class Make>
static inline int layout_out(int64_t N, int n_scenes, int64_t *offsets, int n_offsets, Make make) {
    if (N < 0 || n_scenes < 1 || !offsets || n_offsets != F_COUNT) return ET_ERR_INVALID_ARG;
    const TrainLayout L = make();
    for (int i = 0; i < F_COUNT; ++i) offsets[i] = L.o[i];
    return ET_OK;
}

// a scene's fields in the workspace (n pedestrians from row b on) and its gradient partial: DMRGCN's and Graph-TERN's
// scene structs start with these.  et_stgcnn_train.hip takes scene_fields alone: it places its statistics before the
// partial, and in the other order its kernels compile to other code
struct TrainScene {
    float *f[F_PER];
    float *part;
    int n;
};

__device__ __forceinline__ void scene_fields(float *(&f)[F_PER], float *ws, const TrainLayout &L, int64_t b, int n) {
    float *base = ws + b * L.o[F_PER];
    for (int i = 0; i < F_PER; ++i) f[i] = base + L.o[i] * n;
}

__device__ __forceinline__ TrainScene train_scene(float *ws, const TrainLayout &L, int64_t b, int n, int scene) {
    TrainScene w;
    scene_fields(w.f, ws, L, b, n);
    w.part = ws + L.o[F_PARTIALS] + scene * L.o[F_GRADS];
    w.n = n;
    return w;
}

// a scene kernel's preamble: workgroup blockIdx.x's scene is rows [b, e) (the graph form, off = NULL: all N rows).  A kernel
// returns on empty(), which it touches nothing of, and on n() over its cap (the forward after nan_scene); it spells the
// two tests in its own `if`: folded into one bool here they compile to other code
struct SceneRows {
    int64_t b, e;
    __device__ __forceinline__ int64_t n() const { return e - b; }
    __device__ __forceinline__ bool empty() const { return e <= b; }
};

__device__ __forceinline__ SceneRows scene_rows(const int32_t *off, int64_t N) {
    const int64_t b = off ? off[blockIdx.x] : 0;
    const int64_t e = off ? off[blockIdx.x + 1] : N;
    return {b, e};
}

// a scene over the cap is not computed: store(r, s, w, NaN) for every entry (r, s, w) of its (rows, S, n) output
template <class Store>
__device__ __forceinline__ void nan_scene(int rows, int S, int64_t n, Store store) {
    const float nan = __builtin_nanf("");
    for (int64_t i = threadIdx.x; i < (int64_t)rows * S * n; i += kSgThreads) {
        const int w = (int)(i % n), rs = (int)(i / n);
        store(rs / S, rs % S, w, nan);
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

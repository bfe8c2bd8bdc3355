// et_train_sums.inl -- the fixed-order sums and the small backward pieces that the scene training units share
// (et_stgcnn_train.hip, et_dmrgcn_train.hip), #included inside their anonymous namespaces after et_stgcnn_core.inl
// (kSgThreads).  The statements are et_stgcnn_train.hip's, moved here unchanged; its header comment ("wave_sum") gives the
// order of every sum.
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

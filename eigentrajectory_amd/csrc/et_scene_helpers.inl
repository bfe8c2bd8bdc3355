// et_scene_helpers.inl -- what the per-scene kernels of et_sgcn_core.inl, et_gpgraph_core.inl and et_gpgraph_stgcnn.hip share:
// the workgroup size, the scene of a row, the packed n^2 offset of a scene, a scene's input v = [C_obs; obs_ori].  #included
// inside the anonymous namespace (by et_sgcn_core.inl for the SGCN translation units).
constexpr int kSnThreads = 256;

__host__ __device__ inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// the scene of row r among `off` (S scenes): the first s with off[s + 1] > r
__device__ __forceinline__ int scene_of_row(const int32_t *off, int S, int64_t r) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the squared sizes of the scenes before s (those of more than `cap` pedestrians left out), summed in a fixed order (part:
// kSnThreads int64 of LDS); ends on a barrier
__device__ __forceinline__ int64_t scene_sq_before(const int32_t *off, int s, int64_t *part, int64_t cap) {
    const int tid = threadIdx.x;
    int64_t mine = 0;
    for (int q = tid; q < s; q += kSnThreads) {
        const int64_t m = (int64_t)off[q + 1] - off[q];
        if (m > 0 && m <= cap) mine += m * m;
    }
    part[tid] = mine;
    __syncthreads();
    int64_t sq = 0;
    for (int q = 0; q < kSnThreads; ++q) sq += part[q];
    return sq;
}

// v (T, n) of a scene: the given graph, or [C_obs; obs_ori] with obs_ori = last observed position - its mean over the scene,
// summed in et_scene_project's order (red: 2 kSnThreads / kWave floats of LDS).  The caller puts a barrier after it.
__device__ __forceinline__ void scene_v(float *v, const float *__restrict__ gv, const float *__restrict__ C_obs,
                                        const float *__restrict__ nrm, int64_t N, int64_t b, int n, int T, float *red) {
    const int tid = threadIdx.x;
    if (gv) {
        for (int i = tid; i < T * n; i += kSnThreads) v[i] = gv[i];
    } else {
        const int k = T - 2;
        for (int i = tid; i < k * n; i += kSnThreads) v[i] = C_obs[(int64_t)(i / n) * N + b + (i % n)];
        float sx = 0.f, sy = 0.f;
        for (int w = tid; w < n; w += kSnThreads) {
            sx += nrm[b + w];
            sy += nrm[N + b + w];
        }
        for (int o = 32; o > 0; o >>= 1) {
            sx += __shfl_xor(sx, o);
            sy += __shfl_xor(sy, o);
        }
        if ((tid & (kWave - 1)) == 0) {
            red[tid / kWave] = sx;
            red[kSnThreads / kWave + tid / kWave] = sy;
        }
        __syncthreads();
        float mx = 0.f, my = 0.f;
        for (int w = 0; w < kSnThreads / kWave; ++w) {
            mx += red[w];
            my += red[kSnThreads / kWave + w];
        }
        mx = mx / (float)n;
        my = my / (float)n;
        for (int w = tid; w < n; w += kSnThreads) {
            v[k * n + w] = nrm[b + w] - mx;
            v[(k + 1) * n + w] = nrm[N + b + w] - my;
        }
    }
}

__device__ __forceinline__ float prelu(float x, float a) { return x > 0.f ? x : a * x; }

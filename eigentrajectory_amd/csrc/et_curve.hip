// et_curve.hip -- the curve-fitting baselines of the paper's Table 1 (reference: CurveModel/curve_fitting.py,
// script/descriptor_evaluation.py:38-85): control points of a fixed basis fitted to every trajectory of a set by Adam on
// the mean L2 reconstruction error, the recon of the step with the lowest loss returned.
//
// One launch runs a batch of fits (basis, trajectory set), each with its own N, T <= 32 and ncp <= 8, for all n_steps:
//   lane = (fit, pedestrian); its control points, Adam moments and gradient sum (4 x ncp x 2 fp32), trajectory and the
//   fit's basis stay in registers for the whole loop.  A pedestrian's gradient depends on the others only through 1 / (N T), so the only
//   coupling is the choice of the best step by the summed loss.
// That choice is made deterministic by summing in fixed point: per step each lane rounds its fp64 sum of the T norms to
// an integer in units of 2^-28, the wave adds them, one integer atomic adds the wave's sum to the fit's slot of the step.
// Integer addition is associative, so the per-step loss does not depend on the launch geometry or on scheduling.
//   pass 1  all n_steps, per-step sums into the workspace
//   best    per fit: the first step of minimum loss (the reference keeps the recon of the first strict new minimum)
//   pass 2  every lane replays its pedestrian to its fit's best step, writes recon (and cp)
// The reference's loop calls loss.backward() and optimizer.step() but never zero_grad(), so the gradient Adam sees at
// step k is the fp32 running sum G += g of the step gradients; that is reproduced.
// Arithmetic (fp32, unfused, correctly rounded sqrt / division) follows torch.optim.Adam's single-tensor path on G:
//   m = m + (1-b1) (g - m)                      lerp_ (weight < 0.5 form)
//   v = v b2 + ((1-b2) g) g                     mul_ + addcmul_
//   d = sqrt(v) / sqrt(1 - b2^k) + eps          bias correction in fp64, rounded to fp32 where ATen rounds it
//   p = p + ((-lr / (1 - b1^k)) m) / d          addcdiv_
// b^k is a running fp64 product.  tests/_curve_fit_np.py restates all of it; the GPU tests compare bit for bit.
#include "et_common.h"

namespace {

constexpr int kMaxT = 32;
constexpr int kMaxC = 8;
constexpr double kFix = 268435456.0;       // 2^28: loss units
constexpr double kFixClamp = 67108864.0;   // 2^26: per-pedestrian sums are clamped here (NaN included)

struct Fit {
    int32_t n, T, ncp, pad;
    int64_t traj_off, basis_off, cp_off;
};
struct FitTable {
    Fit f[ET_CURVE_MAX_FITS];
};
struct Hyper {
    double lr, beta1, beta2, eps;
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, et::kWave);
    return q;
}

// One pedestrian of one fit: `steps` Adam steps, then (pass 2) the recon of the parameters reached.
// EXACT: T == MT and ncp == MC at compile time; otherwise every t / i loop is guarded by the runtime bounds.
template <int MT, int MC, bool EXACT>
__device__ __forceinline__ void run(const Fit &fit, const float *__restrict__ traj, const float *__restrict__ basis,
                                    const Hyper h, int64_t steps, unsigned long long *__restrict__ acc,
                                    float *__restrict__ recon, float *__restrict__ cp_out) {
    const int T = EXACT ? MT : fit.T;
    const int C = EXACT ? MC : fit.ncp;
    const int64_t n = fit.n;
    const int64_t ped = (int64_t)blockIdx.x * et::kWave + threadIdx.x;
    const bool live = ped < n;
    const int64_t p = live ? ped : n - 1;  // idle lanes shadow the last pedestrian: all lanes stay active

    float x[MT], y[MT], B[MT][MC], xl = 0.f, yl = 0.f;
    const float *tr = traj + fit.traj_off + p * T * 2;
    const float *bs = basis + fit.basis_off;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        if (t < T) {
            x[t] = tr[2 * t];
            y[t] = tr[2 * t + 1];
            if (t == T - 1) {  // traj[-1] without a dynamic register index
                xl = x[t];
                yl = y[t];
            }
#pragma unroll
            for (int i = 0; i < MC; ++i)
                if (i < C) B[t][i] = bs[t * C + i];
        }
    }
    // curve_fitting.py:13-15: cp[0] = traj[0], cp[i] = cp[i-1] + (traj[-1] - traj[0]) / (ncp - 1)
    float cx[MC], cy[MC], mx[MC], my[MC], vx[MC], vy[MC], ax[MC], ay[MC];
    const float dx = xl - x[0], dy = yl - y[0];
    const float den = (float)(C - 1);
    const float sx = dx / den, sy = dy / den;
    cx[0] = x[0];
    cy[0] = y[0];
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        if (i > 0 && i < C) {
            cx[i] = cx[i - 1] + sx;
            cy[i] = cy[i - 1] + sy;
        }
        mx[i] = my[i] = vx[i] = vy[i] = ax[i] = ay[i] = 0.f;
    }
    const float w1 = (float)(1.0 - h.beta1), b2f = (float)h.beta2, c2f = (float)(1.0 - h.beta2), epsf = (float)h.eps;
    const float scale = 1.0f / (float)(n * T);  // d mean / d norm
    double p1 = 1.0, p2 = 1.0;

    for (int64_t st = 0; st < steps; ++st) {
        float gx[MC], gy[MC];
        double a = 0.0;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (t < T) {
                float rx = B[t][0] * cx[0], ry = B[t][0] * cy[0];
#pragma unroll
                for (int i = 1; i < MC; ++i) {
                    if (i < C) {
                        rx = rx + B[t][i] * cx[i];
                        ry = ry + B[t][i] * cy[i];
                    }
                }
                rx = rx - x[t];
                ry = ry - y[t];
                const float nn = sqrtf(rx * rx + ry * ry);
                a = a + (double)nn;
                const float sc = nn == 0.f ? 0.f : scale / nn;  // the norm's gradient is 0 at a zero residual
                const float grx = rx * sc, gry = ry * sc;
#pragma unroll
                for (int i = 0; i < MC; ++i) {
                    if (i < C) {
                        if (t == 0) {
                            gx[i] = B[0][i] * grx;
                            gy[i] = B[0][i] * gry;
                        } else {
                            gx[i] = gx[i] + B[t][i] * grx;
                            gy[i] = gy[i] + B[t][i] * gry;
                        }
                    }
                }
            }
        }
        if (acc) {
            const unsigned long long q = live ? (unsigned long long)__double2ll_rn(fmin(a, kFixClamp) * kFix) : 0ull;
            const unsigned long long w = wave_sum(q);
            if (threadIdx.x == 0) atomicAdd(acc + st, w);
        }
        p1 = p1 * h.beta1;
        p2 = p2 * h.beta2;
        const float nss = (float)(-(h.lr / (1.0 - p1)));
        const float bc2s = (float)sqrt(1.0 - p2);
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            if (i < C) {
                ax[i] = ax[i] + gx[i];  // the reference never zeroes .grad: the gradient Adam sees is the running sum
                ay[i] = ay[i] + gy[i];
                gx[i] = ax[i];
                gy[i] = ay[i];
                mx[i] = mx[i] + w1 * (gx[i] - mx[i]);
                my[i] = my[i] + w1 * (gy[i] - my[i]);
                vx[i] = vx[i] * b2f + (c2f * gx[i]) * gx[i];
                vy[i] = vy[i] * b2f + (c2f * gy[i]) * gy[i];
                const float ex = sqrtf(vx[i]) / bc2s + epsf, ey = sqrtf(vy[i]) / bc2s + epsf;
                cx[i] = cx[i] + (nss * mx[i]) / ex;
                cy[i] = cy[i] + (nss * my[i]) / ey;
            }
        }
    }
    if (!recon || !live) return;
    float *ro = recon + fit.traj_off + p * T * 2;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        if (t < T) {
            float rx = B[t][0] * cx[0], ry = B[t][0] * cy[0];
#pragma unroll
            for (int i = 1; i < MC; ++i) {
                if (i < C) {
                    rx = rx + B[t][i] * cx[i];
                    ry = ry + B[t][i] * cy[i];
                }
            }
            ro[2 * t] = rx;
            ro[2 * t + 1] = ry;
        }
    }
    if (cp_out) {
        float *co = cp_out + fit.cp_off + p * C * 2;
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            if (i < C) {
                co[2 * i] = cx[i];
                co[2 * i + 1] = cy[i];
            }
        }
    }
}

__host__ __device__ inline bool exact_shape(int T, int ncp) { return (T == 8 || T == 12) && ncp >= 2 && ncp <= 6; }

// grid (max_n / 64, n_fits), one wavefront per block.  pass 1: acc != NULL, recon == NULL; pass 2: the reverse.
// The Table-1 shapes (T = 8 / 12, ncp = 2..6) are compiled exactly; GENERIC takes every other shape (runtime bounds) in a
// kernel of its own, so its larger register arrays do not cut the occupancy of the exact one.
template <bool GENERIC>
__global__ __launch_bounds__(64) void curve_fit_kernel(const FitTable tab, const float *__restrict__ traj,
                                                       const float *__restrict__ basis, const Hyper h, int64_t n_steps,
                                                       const int32_t *__restrict__ best, unsigned long long *acc,
                                                       float *recon, float *cp_out) {
    const int f = blockIdx.y;
    const Fit fit = tab.f[f];
    if ((int64_t)blockIdx.x * et::kWave >= fit.n || exact_shape(fit.T, fit.ncp) == GENERIC) return;
    const int64_t steps = best ? (int64_t)best[f] : n_steps;
    unsigned long long *a = acc ? acc + (int64_t)f * n_steps : nullptr;
    if (GENERIC) {
        if (fit.T <= 16)
            run<16, kMaxC, false>(fit, traj, basis, h, steps, a, recon, cp_out);
        else
            run<kMaxT, kMaxC, false>(fit, traj, basis, h, steps, a, recon, cp_out);
        return;
    }
    switch (fit.T * 16 + fit.ncp) {
#define ET_CURVE_CASE(TT, CC) \
    case TT * 16 + CC: run<TT, CC, true>(fit, traj, basis, h, steps, a, recon, cp_out); break;
        ET_CURVE_CASE(8, 2) ET_CURVE_CASE(8, 3) ET_CURVE_CASE(8, 4) ET_CURVE_CASE(8, 5) ET_CURVE_CASE(8, 6)
        ET_CURVE_CASE(12, 2) ET_CURVE_CASE(12, 3) ET_CURVE_CASE(12, 4) ET_CURVE_CASE(12, 5) ET_CURVE_CASE(12, 6)
#undef ET_CURVE_CASE
    }
}

// one block per fit: best[f] = first index of the minimum of acc[f][:]; loss[f][s] = acc * 2^-28 / (N T)
__global__ __launch_bounds__(256) void curve_best_kernel(const FitTable tab, const unsigned long long *__restrict__ acc,
                                                         int64_t n_steps, int32_t *__restrict__ best,
                                                         double *__restrict__ loss) {
    __shared__ unsigned long long sv[256];
    __shared__ int64_t si[256];
    const int f = blockIdx.x;
    const unsigned long long *a = acc + (int64_t)f * n_steps;
    const double nt = (double)((int64_t)tab.f[f].n * tab.f[f].T);
    unsigned long long bv = ~0ull;
    int64_t bi = n_steps;
    for (int64_t s = threadIdx.x; s < n_steps; s += 256) {
        const unsigned long long v = a[s];
        if (v < bv) {
            bv = v;
            bi = s;
        }
        if (loss) loss[(int64_t)f * n_steps + s] = ((double)(long long)v * (1.0 / kFix)) / nt;
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const unsigned long long v = sv[threadIdx.x + o];
            const int64_t i = si[threadIdx.x + o];
            if (v < sv[threadIdx.x] || (v == sv[threadIdx.x] && i < si[threadIdx.x])) {
                sv[threadIdx.x] = v;
                si[threadIdx.x] = i;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[f] = (int32_t)si[0];
}

size_t acc_bytes(int n_fits, int64_t n_steps) { return (size_t)n_fits * (size_t)n_steps * sizeof(unsigned long long); }
size_t best_off(int n_fits, int64_t n_steps) { return (acc_bytes(n_fits, n_steps) + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t et_curve_fit_batch_workspace_bytes(int n_fits, int64_t n_steps) {
    if (n_fits < 1 || n_fits > ET_CURVE_MAX_FITS || n_steps < 1 || n_steps > INT32_MAX) return 0;
    return best_off(n_fits, n_steps) + (size_t)ET_CURVE_MAX_FITS * sizeof(int32_t);
}

extern "C" int et_curve_fit_batch(const float *traj, const float *basis, const int64_t *fits_host, int n_fits,
                                  int64_t n_steps, double lr, double beta1, double beta2, double eps, float *recon,
                                  float *cp, double *loss, int32_t *best_step, void *workspace, size_t workspace_bytes,
                                  et_stream_t stream) {
    if (!traj || !basis || !fits_host || !recon || n_fits < 1 || n_fits > ET_CURVE_MAX_FITS || n_steps < 1 ||
        n_steps > INT32_MAX)
        return ET_ERR_INVALID_ARG;
    if (!(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return ET_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(basis) | reinterpret_cast<uintptr_t>(recon) |
         reinterpret_cast<uintptr_t>(cp)) & 3u)
        return ET_ERR_INVALID_ARG;
    FitTable tab{};
    int64_t max_n = 0;
    bool any_exact = false, any_generic = false;
    for (int f = 0; f < n_fits; ++f) {
        const int64_t *d = fits_host + 6 * f;
        if (d[0] < 1 || d[0] > INT32_MAX || d[1] < 2 || d[1] > kMaxT || d[2] < 2 || d[2] > kMaxC || d[3] < 0 ||
            d[4] < 0 || d[5] < 0)
            return ET_ERR_INVALID_ARG;
        tab.f[f] = Fit{(int32_t)d[0], (int32_t)d[1], (int32_t)d[2], 0, d[3], d[4], d[5]};
        max_n = d[0] > max_n ? d[0] : max_n;
        (exact_shape((int)d[1], (int)d[2]) ? any_exact : any_generic) = true;
    }
    if (!workspace || workspace_bytes < et_curve_fit_batch_workspace_bytes(n_fits, n_steps)) return ET_ERR_WORKSPACE;
    auto *acc = static_cast<unsigned long long *>(workspace);
    int32_t *best = best_step ? best_step
                              : reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + best_off(n_fits, n_steps));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Hyper h{lr, beta1, beta2, eps};
    const dim3 grid((unsigned)et::ceil_div(max_n, et::kWave), (unsigned)n_fits);
    ET_HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes(n_fits, n_steps), s));
    for (int g = 0; g < 2; ++g) {
        if (!(g ? any_generic : any_exact)) continue;
        (g ? curve_fit_kernel<true> : curve_fit_kernel<false>)<<<grid, et::kWave, 0, s>>>(tab, traj, basis, h, n_steps,
                                                                                           nullptr, acc, nullptr, nullptr);
        ET_LAUNCH_CHECK();
    }
    curve_best_kernel<<<n_fits, 256, 0, s>>>(tab, acc, n_steps, best, loss);
    ET_LAUNCH_CHECK();
    for (int g = 0; g < 2; ++g) {
        if (!(g ? any_generic : any_exact)) continue;
        (g ? curve_fit_kernel<true> : curve_fit_kernel<false>)<<<grid, et::kWave, 0, s>>>(tab, traj, basis, h, n_steps,
                                                                                           best, nullptr, recon, cp);
        ET_LAUNCH_CHECK();
    }
    return ET_OK;
}

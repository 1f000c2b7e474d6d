// The element-wise side of a universal perturbation (unidefense_amd/universal.py: UniversalRunner): ONE pattern delta [per]
// shared by every sample, fitted by sign-gradient (L-infinity) or normalised-gradient (L2) ascent on the batch's summed loss.
// What is new next to csrc/attack.hip is the reduction over the batch dimension inside the captured iteration:
//   ud_uap_control     : one thread per sample: who steers the pattern this iteration (the clamped-loss rule, a source label)
//   ud_uap_reduce      : gsum[e] = sum over the counted n of g[n][e], ascending n, one fp32 add per term
//   ud_uap_update_linf : delta <- clamp(delta + step sign(gsum), -eps, eps) and x_adv[n] <- clamp(x[n] + delta) in one pass
//   ud_uap_apply       : the optional L2 ball projection of delta (in place) and x_adv[n] <- clamp(x[n] + delta)
// The L2 step on delta itself is ud_sample_sumsq + ud_attack_step_l2 with N = 1 (csrc/attack.hip).
//
// All three streaming kernels give one thread one element of delta (a float4 group where per % 4 == 0 and every base is
// 16-byte aligned) and walk the samples in a loop: consecutive threads read consecutive addresses of every g[n] / x[n], the
// element's sum lives in a register, and nothing is shared between threads — no atomics, no workspace, a replay gives the
// same bits.  Per iteration: reduce reads 4 N per bytes and writes 4 per; update reads 4 (N + 2) per and writes 4 (N + 1) per.
#include <climits>

#include "attack_common.h"

namespace {

// ---- control: one thread per sample ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void uap_control(const float* __restrict__ f, const long long* __restrict__ y,
                                                  int* __restrict__ w, int* __restrict__ ist, float* __restrict__ history,
                                                  int* __restrict__ counted, int N, int steps, float beta, int source) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int k = ist[(long)UD_UAP_I_K * N + n];
    if (k < 0 || k >= steps) return;
    const float fn = f[n];
    const int c = (fn < beta) && (source < 0 || y[n] == (long long)source) ? 1 : 0;      // a NaN f compares false
    history[(long)k * N + n] = fn;
    w[n] = c;
    counted[(long)k * N + n] = c;
    ist[(long)UD_UAP_I_K * N + n] = k + 1;
}

// ---- reduce over the batch: T = f32x4 (E = 4) or float (E = 1); nelem = per / E ------------------------------------------------
template <typename T>
__device__ __forceinline__ T zero_of();
template <>
__device__ __forceinline__ float zero_of<float>() { return 0.f; }
template <>
__device__ __forceinline__ f32x4 zero_of<f32x4>() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// w[n] is the same for every thread: the branch is uniform, an excluded sample's row is never read.  (Issuing four samples'
// loads ahead of their adds was measured and lost: 9.1 against 7.0-7.6 us at N 32, per 196608.)
template <typename T>
__global__ __launch_bounds__(NT) void uap_reduce(const float* __restrict__ g, const int* __restrict__ w,
                                                 float* __restrict__ gsum, int N, long nelem) {
#pragma clang fp contract(off)
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < nelem; i += nthr) {
        T acc = zero_of<T>();
        for (int n = 0; n < N; ++n)
            if (w[n] != 0) acc = acc + reinterpret_cast<const T*>(g)[(long)n * nelem + i];
        reinterpret_cast<T*>(gsum)[i] = acc;
    }
}

// ---- delta's two updates, each followed by the broadcast apply -------------------------------------------------------------------
__device__ __forceinline__ float uap_linf_elem(float d, float gs, float step, float eps) {
#pragma clang fp contract(off)
    return clampf(d + sign_inc(gs, step), -eps, eps);
}

__device__ __forceinline__ float uap_add_elem(float x, float d, float lo, float hi) {
#pragma clang fp contract(off)
    return clampf(x + d, lo, hi);
}

// delta scaled onto the ball: a factor of exactly 1 leaves it untouched, as l2_ball_elem does
__device__ __forceinline__ float uap_ball_elem(float d, double f) { return f < 1.0 ? (float)((double)d * f) : d; }

constexpr int ROWS = 4;              // samples a thread loads before it stores the first (15.0 -> 11.2 us at N 32, per 196608)

// MODE 0: the L-infinity step on delta from gsum; MODE 1: delta scaled by l2_ball_factor(dss[0], eps); MODE 2: delta as it is.
// Then x_adv[n] = clamp(x[n] + delta) for every n.  x_adv may be x itself (no other overlap).
template <typename T, int E, int MODE>
__global__ __launch_bounds__(NT) void uap_apply(float* delta, const float* gsum, const double* dss, const float* x, float* x_adv,
                                                int N, long nelem, float step, float eps, float lo, float hi) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    const double f = MODE == 1 ? l2_ball_factor(dss[0], (double)eps) : 1.0;
    for (long i = tid; i < nelem; i += nthr) {
        T dv = reinterpret_cast<const T*>(delta)[i];
        float* d = reinterpret_cast<float*>(&dv);
        if (MODE == 0) {
            const T gv = reinterpret_cast<const T*>(gsum)[i];
            const float* gs = reinterpret_cast<const float*>(&gv);
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = uap_linf_elem(d[e], gs[e], step, eps);
        } else if (MODE == 1) {
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = uap_ball_elem(d[e], f);
        }
        if (MODE != 2) reinterpret_cast<T*>(delta)[i] = dv;
        // x_adv may be x, so the compiler keeps every load behind the store before it: ROWS samples are loaded, then stored
        for (int n0 = 0; n0 < N; n0 += ROWS) {
            T xv[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
                if (n0 + r < N) xv[r] = reinterpret_cast<const T*>(x)[(long)(n0 + r) * nelem + i];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                if (n0 + r >= N) break;
                float* xe = reinterpret_cast<float*>(&xv[r]);
#pragma unroll
                for (int e = 0; e < E; ++e) xe[e] = uap_add_elem(xe[e], d[e], lo, hi);
                reinterpret_cast<T*>(x_adv)[(long)(n0 + r) * nelem + i] = xv[r];
            }
        }
    }
}

template <int MODE>
int launch_apply(float* delta, const float* gsum, const double* dss, const float* x, float* x_adv, int N, long per, float step,
                 float eps, float lo, float hi, hipStream_t s) {
    const bool vec = per % 4 == 0 && aligned16(delta) && aligned16(x) && aligned16(x_adv) && (MODE != 0 || aligned16(gsum));
    if (vec)
        hipLaunchKernelGGL((uap_apply<f32x4, 4, MODE>), dim3(ew_blocks(per / 4)), dim3(NT), 0, s, delta, gsum, dss, x, x_adv, N,
                           per / 4, step, eps, lo, hi);
    else
        hipLaunchKernelGGL((uap_apply<float, 1, MODE>), dim3(ew_blocks(per)), dim3(NT), 0, s, delta, gsum, dss, x, x_adv, N, per,
                           step, eps, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int ud_uap_control(const float* f, const long long* y, int* w, int* ist, float* history, int* counted, int N, int steps,
                   float beta, int source, ud_stream_t stream) {
    if (!f || !y || !w || !ist || !history || !counted) return UD_EINVAL;
    if (N < 1 || steps < 1 || (long)steps * N > INT_MAX || beta != beta) return UD_EINVAL;
    hipLaunchKernelGGL(uap_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, y, w, ist, history,
                       counted, N, steps, beta, source);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_uap_reduce(const float* g, const int* w, float* gsum, int N, long per, ud_stream_t stream) {
    if (!g || !w || !gsum || !shape_ok(N, per)) return UD_EINVAL;
    if (per % 4 == 0 && aligned16(g) && aligned16(gsum))
        hipLaunchKernelGGL(uap_reduce<f32x4>, dim3(ew_blocks(per / 4)), dim3(NT), 0, (hipStream_t)stream, g, w, gsum, N, per / 4);
    else
        hipLaunchKernelGGL(uap_reduce<float>, dim3(ew_blocks(per)), dim3(NT), 0, (hipStream_t)stream, g, w, gsum, N, per);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_uap_update_linf(float* delta, const float* gsum, const float* x, float* x_adv, int N, long per, float step, float eps,
                       float lo, float hi, ud_stream_t stream) {
    if (!delta || !gsum || !x || !x_adv || !shape_ok(N, per) || !(eps >= 0.f) || !(lo <= hi) || step != step) return UD_EINVAL;
    return launch_apply<0>(delta, gsum, nullptr, x, x_adv, N, per, step, eps, lo, hi, (hipStream_t)stream);
}

int ud_uap_apply(float* delta, const double* dss, const float* x, float* x_adv, int N, long per, float eps, float lo, float hi,
                 ud_stream_t stream) {
    if (!delta || !x || !x_adv || !shape_ok(N, per) || !(eps >= 0.f) || !(lo <= hi)) return UD_EINVAL;
    if (dss) return launch_apply<1>(delta, nullptr, dss, x, x_adv, N, per, 0.f, eps, lo, hi, (hipStream_t)stream);
    return launch_apply<2>(delta, nullptr, nullptr, x, x_adv, N, per, 0.f, eps, lo, hi, (hipStream_t)stream);
}

}  // extern "C"

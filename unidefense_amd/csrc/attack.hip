// The element-wise side of an iterated input-gradient attack (unidefense_amd/attack.py: AttackRunner): the L-infinity
// sign step with its two projections, the per-sample squared L2 norm, and the L2 normalised-gradient step and ball
// projection.  All tensors are contiguous fp32 planes [N][3][H][W] (per = 3 H W elements per sample, total = N per).
//
// These launches are ~0.1 % of an attack iteration (16 B per element next to a whole forward + d/dx); they exist so that
// the iteration stays inside one captured graph with one launch where torch would issue six.  So: plain grid-stride
// kernels, a float4 body with a scalar tail (total and per need not be multiples of 4), no atomics, no data-dependent
// partition — a replay gives the same bits.
#include "attack_common.h"

namespace {

constexpr int CHUNK = 4096;          // elements of one sample that one workgroup of ud_sample_sumsq sums (16 per thread)

// One element of the L-infinity step, in the order torch evaluates
//   clamp(clamp(x + step * sign(g), x0 - eps, x0 + eps), lo, hi)
// with one fp32 rounding per operation
__device__ __forceinline__ float linf_elem(float x, float x0, float g, float step, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    return proj_linf(x + sign_inc(g, step), x0, eps, lo, hi);
}

// nvec float4 groups from the start, then the scalar elements [4 nvec, total)
__global__ __launch_bounds__(NT) void attack_step_linf(float* __restrict__ xa, const float* __restrict__ x0,
                                                        const float* __restrict__ g, long nvec, long total, float step,
                                                        float eps, float lo, float hi) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < nvec; i += nthr) {
        f32x4 v = reinterpret_cast<const f32x4*>(xa)[i];
        const f32x4 b = reinterpret_cast<const f32x4*>(x0)[i];
        const f32x4 d = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = linf_elem(v[e], b[e], d[e], step, eps, lo, hi);
        reinterpret_cast<f32x4*>(xa)[i] = v;
    }
    for (long i = 4 * nvec + tid; i < total; i += nthr) xa[i] = linf_elem(xa[i], x0[i], g[i], step, eps, lo, hi);
}

// number of CHUNK-element parts of one sample: a function of per alone
inline long sumsq_parts(long per) { return (per + CHUNK - 1) / CHUNK; }

// Part p of sample n: sum over i in [p CHUNK, min(per, (p + 1) CHUNK)) of (a - b)^2, formed in double.  Every thread adds
// its elements in index order, the wave folds by shuffles, the four waves are added in wave order: a fixed tree.
template <bool VEC>
__global__ __launch_bounds__(NT) void sample_sumsq_parts(const float* __restrict__ a, const float* __restrict__ b, long per,
                                                          double* __restrict__ dst) {
    const long n = blockIdx.y, p = blockIdx.x;
    const long lo = p * CHUNK, hi = lo + CHUNK < per ? lo + CHUNK : per;
    const float* pa = a + n * per;
    const float* pb = b ? b + n * per : nullptr;
    double acc = 0.0;
    if (VEC) {           // per % 4 == 0 and 16-byte aligned bases: lo and hi are multiples of 4
        for (long i = lo / 4 + threadIdx.x; i < hi / 4; i += NT) {
            const f32x4 va = reinterpret_cast<const f32x4*>(pa)[i];
            f32x4 vb = {0.f, 0.f, 0.f, 0.f};
            if (pb) vb = reinterpret_cast<const f32x4*>(pb)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)va[e] - (double)vb[e];
                acc += d * d;
            }
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += NT) {
            const double d = (double)pa[i] - (pb ? (double)pb[i] : 0.0);
            acc += d * d;
        }
    }
    acc = ud_wave_sum_d(acc);
    __shared__ double part[NT / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = part[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) s += part[w];
        dst[n * gridDim.x + p] = s;
    }
}

// out[n] = ws[n][0] + ws[n][1] + ... in index order (one thread per sample)
__global__ __launch_bounds__(64) void sample_sumsq_fold(const double* __restrict__ ws, int N, long parts,
                                                         double* __restrict__ out) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (long p = 0; p < parts; ++p) s += ws[(long)n * parts + p];
    out[n] = s;
}

__device__ __forceinline__ float l2_step_elem(float x, float g, double f) { return (float)((double)x + (double)g * f); }

// PROJ = false: x_adv[n] += step g[n] / max(|g[n]|, 1e-12), other = g, ss = gss, c = step
// PROJ = true : x_adv[n] <- clamp(x0[n] + d[n] min(1, eps / max(|d[n]|, 1e-12))), other = x0, ss = dss, c = eps
// A float4 group may straddle two samples when per is not a multiple of 4: the factor is looked up per element then.
template <bool PROJ>
__global__ __launch_bounds__(NT) void attack_l2(float* __restrict__ xa, const float* __restrict__ other,
                                                 const double* __restrict__ ss, long nvec, long total, long per, double c,
                                                 float lo, float hi) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < nvec; i += nthr) {
        f32x4 v = reinterpret_cast<const f32x4*>(xa)[i];
        const f32x4 o = reinterpret_cast<const f32x4*>(other)[i];
        const long n0 = (4 * i) / per, n3 = (4 * i + 3) / per;
        const double f0 = PROJ ? l2_ball_factor(ss[n0], c) : l2_dir_factor(ss[n0], c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double f = f0;
            if (n3 != n0) {
                const long n = (4 * i + e) / per;
                if (n != n0) f = PROJ ? l2_ball_factor(ss[n], c) : l2_dir_factor(ss[n], c);
            }
            v[e] = PROJ ? l2_ball_elem(v[e], o[e], f, lo, hi) : l2_step_elem(v[e], o[e], f);
        }
        reinterpret_cast<f32x4*>(xa)[i] = v;
    }
    for (long i = 4 * nvec + tid; i < total; i += nthr) {
        const long n = i / per;
        const double f = PROJ ? l2_ball_factor(ss[n], c) : l2_dir_factor(ss[n], c);
        xa[i] = PROJ ? l2_ball_elem(xa[i], other[i], f, lo, hi) : l2_step_elem(xa[i], other[i], f);
    }
}

}  // namespace

extern "C" {

int ud_attack_step_linf(float* x_adv, const float* x0, const float* g, long total, float step, float eps, float lo, float hi,
                        ud_stream_t stream) {
    if (!x_adv || !x0 || !g || total <= 0 || !(eps >= 0.f) || !(lo <= hi) || step != step) return UD_EINVAL;
    const long nvec = aligned16(x_adv) && aligned16(x0) && aligned16(g) ? total / 4 : 0;
    hipLaunchKernelGGL(attack_step_linf, dim3(ew_blocks(nvec + (total - 4 * nvec))), dim3(NT), 0, (hipStream_t)stream, x_adv, x0,
                       g, nvec, total, step, eps, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

long ud_sample_sumsq_ws_bytes(int N, long per) {
    if (!shape_ok(N, per)) return UD_EINVAL;
    const long parts = sumsq_parts(per);
    return parts > 1 ? (long)N * parts * (long)sizeof(double) : 0;
}

int ud_sample_sumsq(const float* a, const float* b, int N, long per, double* out, double* ws, long ws_bytes,
                    ud_stream_t stream) {
    if (!a || !out || !shape_ok(N, per)) return UD_EINVAL;
    const long parts = sumsq_parts(per);
    if (parts > 2147483647L) return UD_EINVAL;
    if (parts > 1 && (!ws || ws_bytes < ud_sample_sumsq_ws_bytes(N, per))) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* dst = parts > 1 ? ws : out;
    const dim3 grid((unsigned)parts, (unsigned)N);
    if (per % 4 == 0 && aligned16(a) && (!b || aligned16(b)))
        hipLaunchKernelGGL(sample_sumsq_parts<true>, grid, dim3(NT), 0, s, a, b, per, dst);
    else
        hipLaunchKernelGGL(sample_sumsq_parts<false>, grid, dim3(NT), 0, s, a, b, per, dst);
    UD_LAUNCH_CHECK();
    if (parts > 1) {
        hipLaunchKernelGGL(sample_sumsq_fold, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, s, ws, N, parts, out);
        UD_LAUNCH_CHECK();
    }
    return 0;
}

int ud_attack_step_l2(float* x_adv, const float* g, const double* gss, int N, long per, float step, ud_stream_t stream) {
    if (!x_adv || !g || !gss || !shape_ok(N, per) || step != step) return UD_EINVAL;
    const long total = (long)N * per;
    const long nvec = aligned16(x_adv) && aligned16(g) ? total / 4 : 0;
    hipLaunchKernelGGL(attack_l2<false>, dim3(ew_blocks(nvec + (total - 4 * nvec))), dim3(NT), 0, (hipStream_t)stream, x_adv, g,
                       gss, nvec, total, per, (double)step, 0.f, 0.f);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_attack_project_l2(float* x_adv, const float* x0, const double* dss, int N, long per, float eps, float lo, float hi,
                         ud_stream_t stream) {
    if (!x_adv || !x0 || !dss || !shape_ok(N, per) || !(eps >= 0.f) || !(lo <= hi)) return UD_EINVAL;
    const long total = (long)N * per;
    const long nvec = aligned16(x_adv) && aligned16(x0) ? total / 4 : 0;
    hipLaunchKernelGGL(attack_l2<true>, dim3(ew_blocks(nvec + (total - 4 * nvec))), dim3(NT), 0, (hipStream_t)stream, x_adv, x0,
                       dss, nvec, total, per, (double)eps, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

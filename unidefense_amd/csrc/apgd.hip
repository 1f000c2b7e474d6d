// Auto-PGD (unidefense_amd/attack.py: APGDRunner): the per-sample control of step size, momentum and restarts-from-best,
// and the element-wise update that obeys it.  Everything that depends on the data — which samples improved, whose step is
// halved, who jumps back to their best point — is device state read and written by these kernels, so one iteration is a
// static sequence of launches inside a captured graph with no host round trip.
//
// ud_apgd_control is one thread per sample: the iteration index is a per-sample counter that the thread itself increments,
// and no two threads store to the same address.  The element-wise kernels follow csrc/attack.hip: contiguous fp32 planes
// [N][3][H][W] (per = 3 H W), grid-stride, a float4 body with a scalar tail, a group that straddles two samples looks its
// sample up per element, no atomics, NaN-transparent clamps — a replay gives the same bits.
#include "ud_common.h"

namespace {

constexpr int NT = 256;
constexpr int MAXCK = UD_APGD_MAX_CHECKPOINTS;

// rows of the [5][N] state arrays (UD_APGD_I_* / UD_APGD_F_* of the header)
enum { I_K = 0, I_CNT = 1, I_HALVED = 2, I_IMPROVED = 3, I_RESET = 4 };
enum { F_PREV = 0, F_BEST = 1, F_CKPT = 2, F_ETA = 3, F_A = 4 };

struct Checkpoints {          // by value in the kernel arguments
    int w[MAXCK];             // iteration index of the checkpoint
    int thr[MAXCK];           // ceil(rho * window): condition 1 is cnt < thr, in integers
    int n;
};

inline int ew_blocks(long work) {
    long b = (work + NT - 1) / NT;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool shape_ok(int N, long per) { return N >= 1 && N <= 65535 && per >= 1 && per <= (1L << 40) / N; }

// clamp that keeps a NaN (both comparisons are false for it)
__device__ __forceinline__ float clampf(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// ---- control --------------------------------------------------------------------------------------------------------------
// closing == 0: iteration k = ist[I_K][n] of the state machine (k outside [0, steps) writes nothing), then k + 1 is stored.
// closing != 0: the keep-best decision on the loss of the last point, history row `steps`; the counter is left alone.
__global__ __launch_bounds__(64) void apgd_control(const float* __restrict__ f, int* __restrict__ ist,
                                                    float* __restrict__ fst, float* __restrict__ history, int N, int steps,
                                                    const Checkpoints ck, float eta0, float alpha, int closing) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const float fk = f[n];
    if (closing) {
        const float fb = fst[(long)F_BEST * N + n];
        const int imp = fk > fb;
        if (imp) fst[(long)F_BEST * N + n] = fk;
        ist[(long)I_IMPROVED * N + n] = imp;
        history[(long)steps * N + n] = fk;
        return;
    }
    const int k = ist[(long)I_K * N + n];
    if (k < 0 || k >= steps) return;
    float fbest, fckpt, eta, a;
    int cnt, halved, improved;
    if (k == 0) {
        fbest = fckpt = fk;
        eta = eta0;
        improved = 1, cnt = 0, halved = 0;
        a = 1.f;
    } else {
        fbest = fst[(long)F_BEST * N + n];
        fckpt = fst[(long)F_CKPT * N + n];
        eta = fst[(long)F_ETA * N + n];
        cnt = ist[(long)I_CNT * N + n] + (fk > fst[(long)F_PREV * N + n] ? 1 : 0);
        halved = ist[(long)I_HALVED * N + n];
        improved = fk > fbest;
        if (improved) fbest = fk;
        a = alpha;
    }
    int reset = 0;
    for (int j = 0; j < ck.n; ++j) {
        if (ck.w[j] != k) continue;
        const bool c1 = cnt < ck.thr[j];
        const bool c2 = !halved && fckpt == fbest;
        if (c1 || c2) {
            eta = eta * 0.5f;
            reset = 1, halved = 1;
            a = 1.f;
        } else {
            halved = 0;
        }
        fckpt = fbest;
        cnt = 0;
    }
    fst[(long)F_PREV * N + n] = fk;
    fst[(long)F_BEST * N + n] = fbest;
    fst[(long)F_CKPT * N + n] = fckpt;
    fst[(long)F_ETA * N + n] = eta;
    fst[(long)F_A * N + n] = a;
    ist[(long)I_K * N + n] = k + 1;
    ist[(long)I_CNT * N + n] = cnt;
    ist[(long)I_HALVED * N + n] = halved;
    ist[(long)I_IMPROVED * N + n] = improved;
    ist[(long)I_RESET * N + n] = reset;
    history[(long)k * N + n] = fk;
}

// ---- L-infinity update ----------------------------------------------------------------------------------------------------
struct Sample {               // what the control left for one sample
    int improved, reset;
    float eta, a;
};

__device__ __forceinline__ Sample load_sample(const int* __restrict__ ist, const float* __restrict__ fst, int N, long n) {
    Sample s;
    s.improved = ist[(long)I_IMPROVED * N + n];
    s.reset = ist[(long)I_RESET * N + n];
    s.eta = fst[(long)F_ETA * N + n];
    s.a = fst[(long)F_A * N + n];
    return s;
}

// projection onto the box around x0, then onto clip, as csrc/attack.hip forms it
__device__ __forceinline__ float proj_linf(float v, float x0, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    const float bl = x0 - eps, bh = x0 + eps;
    return clampf(clampf(v, bl, bh), lo, hi);
}

// One element, one fp32 rounding per operation, in the order of the torch expression
//   z = P(src + eta sign(gs));   x' = z  if a == 1  else  P((src + a (z - src)) + (1 - a) (src - x_prev))
// eta sign(gs) is +-eta or 0 exactly; a NaN gs gives a NaN.  x_best / g_best are read only for a sample that resets
// without having improved, and written only for a sample that improved.
__device__ __forceinline__ void linf_elem(float* __restrict__ x, float* __restrict__ xprev, float* __restrict__ xbest,
                                          float* __restrict__ gbest, const float* __restrict__ x0,
                                          const float* __restrict__ g, long i, const Sample s, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    float src = x[i], gs = g[i];
    if (s.improved) {
        xbest[i] = src;
        gbest[i] = gs;
    } else if (s.reset) {
        src = xbest[i];
        gs = gbest[i];
    }
    const float b = x0[i];
    const float inc = gs > 0.f ? s.eta : (gs < 0.f ? -s.eta : (gs == gs ? 0.f : gs));
    const float z = proj_linf(src + inc, b, eps, lo, hi);
    float xn = z;
    if (s.a != 1.f) {
        const float t1 = s.a * (z - src);
        const float t2 = (1.f - s.a) * (src - xprev[i]);
        xn = proj_linf((src + t1) + t2, b, eps, lo, hi);
    }
    xprev[i] = src;
    x[i] = xn;
}

// the same on a float4 group that lies inside one sample
__device__ __forceinline__ void linf_group(float* __restrict__ x, float* __restrict__ xprev, float* __restrict__ xbest,
                                           float* __restrict__ gbest, const float* __restrict__ x0,
                                           const float* __restrict__ g, long i4, const Sample s, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    f32x4 src = reinterpret_cast<const f32x4*>(x)[i4];
    f32x4 gs = reinterpret_cast<const f32x4*>(g)[i4];
    if (s.improved) {
        reinterpret_cast<f32x4*>(xbest)[i4] = src;
        reinterpret_cast<f32x4*>(gbest)[i4] = gs;
    } else if (s.reset) {
        src = reinterpret_cast<const f32x4*>(xbest)[i4];
        gs = reinterpret_cast<const f32x4*>(gbest)[i4];
    }
    const f32x4 b = reinterpret_cast<const f32x4*>(x0)[i4];
    f32x4 xn;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float inc = gs[e] > 0.f ? s.eta : (gs[e] < 0.f ? -s.eta : (gs[e] == gs[e] ? 0.f : gs[e]));
        xn[e] = proj_linf(src[e] + inc, b[e], eps, lo, hi);
    }
    if (s.a != 1.f) {
        const f32x4 p = reinterpret_cast<const f32x4*>(xprev)[i4];
        const float oma = 1.f - s.a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t1 = s.a * (xn[e] - src[e]);
            const float t2 = oma * (src[e] - p[e]);
            xn[e] = proj_linf((src[e] + t1) + t2, b[e], eps, lo, hi);
        }
    }
    reinterpret_cast<f32x4*>(xprev)[i4] = src;
    reinterpret_cast<f32x4*>(x)[i4] = xn;
}

__global__ __launch_bounds__(NT) void apgd_update_linf(float* __restrict__ x, float* __restrict__ xprev,
                                                        float* __restrict__ xbest, float* __restrict__ gbest,
                                                        const float* __restrict__ x0, const float* __restrict__ g,
                                                        const int* __restrict__ ist, const float* __restrict__ fst, int N,
                                                        long per, long nvec, long total, float eps, float lo, float hi) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < nvec; i += nthr) {
        const long n0 = (4 * i) / per, n3 = (4 * i + 3) / per;
        if (n3 == n0) {
            linf_group(x, xprev, xbest, gbest, x0, g, i, load_sample(ist, fst, N, n0), eps, lo, hi);
        } else {
            for (int e = 0; e < 4; ++e)
                linf_elem(x, xprev, xbest, gbest, x0, g, 4 * i + e, load_sample(ist, fst, N, (4 * i + e) / per), eps, lo, hi);
        }
    }
    for (long i = 4 * nvec + tid; i < total; i += nthr)
        linf_elem(x, xprev, xbest, gbest, x0, g, i, load_sample(ist, fst, N, i / per), eps, lo, hi);
}

// ---- keep-best copy: dst[n] <- src[n] where flag[n] != 0 ------------------------------------------------------------------
__global__ __launch_bounds__(NT) void apgd_keep(float* __restrict__ dst, const float* __restrict__ src,
                                                 const int* __restrict__ flag, long per, long nvec, long total) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < nvec; i += nthr) {
        const long n0 = (4 * i) / per, n3 = (4 * i + 3) / per;
        if (n3 == n0) {
            if (flag[n0]) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
        } else {
            for (int e = 0; e < 4; ++e)
                if (flag[(4 * i + e) / per]) dst[4 * i + e] = src[4 * i + e];
        }
    }
    for (long i = 4 * nvec + tid; i < total; i += nthr)
        if (flag[i / per]) dst[i] = src[i];
}

// ---- L2: step and combination (the two projections are ud_sample_sumsq + apgd_project_l2 / ud_attack_project_l2) ----------
__device__ __forceinline__ double l2_dir_factor(double ss, float eta) { return (double)eta / fmax(sqrt(ss), 1e-12); }

// One element of the L2 step: keep-best copy, source selection, x <- src, z <- src + eta gs / max(|gs|, 1e-12) formed in
// double and rounded once.  gss[n] = |g[n]|^2; gss_best[n] is kept beside g_best (written by the thread of the sample's
// first element when the sample improved, read only when it resets without having improved: never both in one launch).
__device__ __forceinline__ void l2_step_elem(float* __restrict__ x, float* __restrict__ z, float* __restrict__ xbest,
                                             float* __restrict__ gbest, double* __restrict__ gss_best,
                                             const float* __restrict__ g, const double* __restrict__ gss, long i, long n,
                                             long per, const Sample s) {
    float src = x[i], gs = g[i];
    double ss = gss[n];
    if (s.improved) {
        xbest[i] = src;
        gbest[i] = gs;
        if (i == n * per) gss_best[n] = ss;
    } else if (s.reset) {
        src = xbest[i];
        gs = gbest[i];
        ss = gss_best[n];
        x[i] = src;
    }
    z[i] = (float)((double)src + (double)gs * l2_dir_factor(ss, s.eta));
}

__global__ __launch_bounds__(NT) void apgd_step_l2(float* __restrict__ x, float* __restrict__ z, float* __restrict__ xbest,
                                                    float* __restrict__ gbest, double* __restrict__ gss_best,
                                                    const float* __restrict__ g, const double* __restrict__ gss,
                                                    const int* __restrict__ ist, const float* __restrict__ fst, int N,
                                                    long per, long total) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < total; i += nthr) {
        const long n = i / per;
        l2_step_elem(x, z, xbest, gbest, gss_best, g, gss, i, n, per, load_sample(ist, fst, N, n));
    }
}

// x holds src, z the projected step: x <- z if a == 1 else src + a (z - src) + (1 - a) (src - x_prev) (double, one
// rounding); x_prev <- src
__global__ __launch_bounds__(NT) void apgd_combine_l2(float* __restrict__ x, float* __restrict__ xprev,
                                                       const float* __restrict__ z, const float* __restrict__ fst, int N,
                                                       long per, long total) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < total; i += nthr) {
        const float a = fst[(long)F_A * N + i / per];
        const float src = x[i], zz = z[i];
        float xn = zz;
        if (a != 1.f) {
            const double s = (double)src, da = (double)a;
            xn = (float)(s + da * ((double)zz - s) + (1.0 - da) * (s - (double)xprev[i]));
        }
        xprev[i] = src;
        x[i] = xn;
    }
}

// ud_attack_project_l2 on the samples whose a != 1 (the momentum point); a sample with a == 1 holds z, which is projected
// already, and is left exactly as it is
__global__ __launch_bounds__(NT) void apgd_project_l2(float* __restrict__ x, const float* __restrict__ x0,
                                                       const double* __restrict__ dss, const float* __restrict__ fst, int N,
                                                       long per, long total, double eps, float lo, float hi) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < total; i += nthr) {
        const long n = i / per;
        if (fst[(long)F_A * N + n] == 1.f) continue;
        const double f = fmin(1.0, eps / fmax(sqrt(dss[n]), 1e-12));
        const float xi = x[i], b = x0[i];
        const float v = f < 1.0 ? (float)((double)b + ((double)xi - (double)b) * f) : xi;
        x[i] = clampf(v, lo, hi);
    }
}

}  // namespace

extern "C" {

int ud_apgd_control(const float* f, int* ist, float* fst, float* history, int N, int steps, const int* ck_w,
                    const int* ck_thr, int n_ck, float eta0, float alpha, int closing, ud_stream_t stream) {
    if (!f || !ist || !fst || !history || N < 1 || steps < 1 || n_ck < 0 || n_ck > MAXCK) return UD_EINVAL;
    if (n_ck > 0 && (!ck_w || !ck_thr)) return UD_EINVAL;
    if (!(eta0 >= 0.f) || !(alpha > 0.f && alpha <= 1.f)) return UD_EINVAL;
    Checkpoints ck{};
    for (int j = 0; j < n_ck; ++j) {
        if (ck_w[j] < 1 || ck_w[j] >= steps || ck_thr[j] < 0 || (j > 0 && ck_w[j] <= ck_w[j - 1])) return UD_EINVAL;
        ck.w[j] = ck_w[j];
        ck.thr[j] = ck_thr[j];
    }
    ck.n = n_ck;
    hipLaunchKernelGGL(apgd_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ist, fst, history, N,
                       steps, ck, eta0, alpha, closing);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_apgd_update_linf(float* x, float* x_prev, float* x_best, float* g_best, const float* x0, const float* g, const int* ist,
                        const float* fst, int N, long per, float eps, float lo, float hi, ud_stream_t stream) {
    if (!x || !x_prev || !x_best || !g_best || !x0 || !g || !ist || !fst || !shape_ok(N, per) || !(eps >= 0.f) || !(lo <= hi))
        return UD_EINVAL;
    const long total = (long)N * per;
    const bool al = aligned16(x) && aligned16(x_prev) && aligned16(x_best) && aligned16(g_best) && aligned16(x0) && aligned16(g);
    const long nvec = al ? total / 4 : 0;
    hipLaunchKernelGGL(apgd_update_linf, dim3(ew_blocks(nvec + (total - 4 * nvec))), dim3(NT), 0, (hipStream_t)stream, x, x_prev,
                       x_best, g_best, x0, g, ist, fst, N, per, nvec, total, eps, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_apgd_keep(float* dst, const float* src, const int* flag, int N, long per, ud_stream_t stream) {
    if (!dst || !src || !flag || !shape_ok(N, per)) return UD_EINVAL;
    const long total = (long)N * per;
    const long nvec = aligned16(dst) && aligned16(src) ? total / 4 : 0;
    hipLaunchKernelGGL(apgd_keep, dim3(ew_blocks(nvec + (total - 4 * nvec))), dim3(NT), 0, (hipStream_t)stream, dst, src, flag,
                       per, nvec, total);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_apgd_step_l2(float* x, float* z, float* x_best, float* g_best, double* gss_best, const float* g, const double* gss,
                    const int* ist, const float* fst, int N, long per, ud_stream_t stream) {
    if (!x || !z || !x_best || !g_best || !gss_best || !g || !gss || !ist || !fst || !shape_ok(N, per)) return UD_EINVAL;
    const long total = (long)N * per;
    hipLaunchKernelGGL(apgd_step_l2, dim3(ew_blocks(total)), dim3(NT), 0, (hipStream_t)stream, x, z, x_best, g_best, gss_best, g,
                       gss, ist, fst, N, per, total);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_apgd_combine_l2(float* x, float* x_prev, const float* z, const float* fst, int N, long per, ud_stream_t stream) {
    if (!x || !x_prev || !z || !fst || !shape_ok(N, per)) return UD_EINVAL;
    const long total = (long)N * per;
    hipLaunchKernelGGL(apgd_combine_l2, dim3(ew_blocks(total)), dim3(NT), 0, (hipStream_t)stream, x, x_prev, z, fst, N, per,
                       total);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_apgd_project_l2(float* x, const float* x0, const double* dss, const float* fst, int N, long per, float eps, float lo,
                       float hi, ud_stream_t stream) {
    if (!x || !x0 || !dss || !fst || !shape_ok(N, per) || !(eps >= 0.f) || !(lo <= hi)) return UD_EINVAL;
    const long total = (long)N * per;
    hipLaunchKernelGGL(apgd_project_l2, dim3(ew_blocks(total)), dim3(NT), 0, (hipStream_t)stream, x, x0, dss, fst, N, per, total,
                       (double)eps, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

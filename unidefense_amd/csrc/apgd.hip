// Auto-PGD (unidefense_amd/attack.py: APGDRunner): the per-sample control of step size, momentum and restarts-from-best,
// and the element-wise update that obeys it.  Everything that depends on the data — which samples improved, whose step is
// halved, who jumps back to their best point — is device state read and written by these kernels, so one iteration is a
// static sequence of launches inside a captured graph with no host round trip.
//
// ud_apgd_control is one thread per sample: the iteration index is a per-sample counter that the thread itself increments,
// and no two threads store to the same address.  The element-wise kernels follow csrc/attack.hip: contiguous fp32 planes
// [N][3][H][W] (per = 3 H W), grid-stride, a float4 body with a scalar tail, a group that straddles two samples looks its
// sample up per element, no atomics, NaN-transparent clamps — a replay gives the same bits.
#include "attack_common.h"

namespace {

constexpr int MAXCK = UD_APGD_MAX_CHECKPOINTS;

struct Checkpoints {          // by value in the kernel arguments
    int w[MAXCK];             // iteration index of the checkpoint
    int thr[MAXCK];           // ceil(rho * window): condition 1 is cnt < thr, in integers
    int n;
};

// ---- control --------------------------------------------------------------------------------------------------------------
// closing == 0: iteration k = ist[UD_APGD_I_K][n] of the state machine (k outside [0, steps) writes nothing), then k + 1 is
// stored.
// closing != 0: the keep-best decision on the loss of the last point, history row `steps`; the counter is left alone.
__global__ __launch_bounds__(64) void apgd_control(const float* __restrict__ f, int* __restrict__ ist,
                                                    float* __restrict__ fst, float* __restrict__ history, int N, int steps,
                                                    const Checkpoints ck, float eta0, float alpha, int closing) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const float fk = f[n];
    if (closing) {
        const float fb = fst[(long)UD_APGD_F_BEST * N + n];
        const int imp = fk > fb;
        if (imp) fst[(long)UD_APGD_F_BEST * N + n] = fk;
        ist[(long)UD_APGD_I_IMPROVED * N + n] = imp;
        history[(long)steps * N + n] = fk;
        return;
    }
    const int k = ist[(long)UD_APGD_I_K * N + n];
    if (k < 0 || k >= steps) return;
    float fbest, fckpt, eta, a;
    int cnt, halved, improved;
    if (k == 0) {
        fbest = fckpt = fk;
        eta = eta0;
        improved = 1, cnt = 0, halved = 0;
        a = 1.f;
    } else {
        fbest = fst[(long)UD_APGD_F_BEST * N + n];
        fckpt = fst[(long)UD_APGD_F_CKPT * N + n];
        eta = fst[(long)UD_APGD_F_ETA * N + n];
        cnt = ist[(long)UD_APGD_I_CNT * N + n] + (fk > fst[(long)UD_APGD_F_PREV * N + n] ? 1 : 0);
        halved = ist[(long)UD_APGD_I_HALVED * N + n];
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
    fst[(long)UD_APGD_F_PREV * N + n] = fk;
    fst[(long)UD_APGD_F_BEST * N + n] = fbest;
    fst[(long)UD_APGD_F_CKPT * N + n] = fckpt;
    fst[(long)UD_APGD_F_ETA * N + n] = eta;
    fst[(long)UD_APGD_F_A * N + n] = a;
    ist[(long)UD_APGD_I_K * N + n] = k + 1;
    ist[(long)UD_APGD_I_CNT * N + n] = cnt;
    ist[(long)UD_APGD_I_HALVED * N + n] = halved;
    ist[(long)UD_APGD_I_IMPROVED * N + n] = improved;
    ist[(long)UD_APGD_I_RESET * N + n] = reset;
    history[(long)k * N + n] = fk;
}

// ---- L-infinity update ----------------------------------------------------------------------------------------------------
struct Sample {               // what the control left for one sample
    int improved, reset;
    float eta, a;
};

__device__ __forceinline__ Sample load_sample(const int* __restrict__ ist, const float* __restrict__ fst, int N, long n) {
    Sample s;
    s.improved = ist[(long)UD_APGD_I_IMPROVED * N + n];
    s.reset = ist[(long)UD_APGD_I_RESET * N + n];
    s.eta = fst[(long)UD_APGD_F_ETA * N + n];
    s.a = fst[(long)UD_APGD_F_A * N + n];
    return s;
}

// One element, one fp32 rounding per operation, in the order of the torch expression
//   z = P(src + eta sign(gs));   x' = z  if a == 1  else  P((src + a (z - src)) + (1 - a) (src - x_prev))
// with P = proj_linf.  prev is looked at only for a sample with a != 1.
__device__ __forceinline__ float linf_new(float src, float gs, float prev, float x0, const Sample s, float eps, float lo,
                                          float hi) {
#pragma clang fp contract(off)
    const float z = proj_linf(src + sign_inc(gs, s.eta), x0, eps, lo, hi);
    if (s.a == 1.f) return z;
    const float t1 = s.a * (z - src);
    const float t2 = (1.f - s.a) * (src - prev);
    return proj_linf((src + t1) + t2, x0, eps, lo, hi);
}

// The update of one element (V = float) or of a float4 group that lies inside one sample (V = f32x4), i counting in units
// of V.  x_best / g_best are read only for a sample that resets without having improved and written only for a sample that
// improved; x_prev is read only for a sample with a != 1.
template <typename V>
__device__ __forceinline__ void linf_update(float* __restrict__ x, float* __restrict__ xprev, float* __restrict__ xbest,
                                            float* __restrict__ gbest, const float* __restrict__ x0,
                                            const float* __restrict__ g, long i, const Sample s, float eps, float lo, float hi) {
    V src = reinterpret_cast<const V*>(x)[i], gs = reinterpret_cast<const V*>(g)[i];
    if (s.improved) {
        reinterpret_cast<V*>(xbest)[i] = src;
        reinterpret_cast<V*>(gbest)[i] = gs;
    } else if (s.reset) {
        src = reinterpret_cast<const V*>(xbest)[i];
        gs = reinterpret_cast<const V*>(gbest)[i];
    }
    const V b = reinterpret_cast<const V*>(x0)[i];
    V prev = src, xn;
    if (s.a != 1.f) prev = reinterpret_cast<const V*>(xprev)[i];
    if constexpr (sizeof(V) == sizeof(float)) {
        xn = linf_new(src, gs, prev, b, s, eps, lo, hi);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xn[e] = linf_new(src[e], gs[e], prev[e], b[e], s, eps, lo, hi);
    }
    reinterpret_cast<V*>(xprev)[i] = src;
    reinterpret_cast<V*>(x)[i] = xn;
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
            linf_update<f32x4>(x, xprev, xbest, gbest, x0, g, i, load_sample(ist, fst, N, n0), eps, lo, hi);
        } else {
            for (long j = 4 * i; j < 4 * i + 4; ++j)
                linf_update<float>(x, xprev, xbest, gbest, x0, g, j, load_sample(ist, fst, N, j / per), eps, lo, hi);
        }
    }
    for (long i = 4 * nvec + tid; i < total; i += nthr)
        linf_update<float>(x, xprev, xbest, gbest, x0, g, i, load_sample(ist, fst, N, i / per), eps, lo, hi);
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
        const float a = fst[(long)UD_APGD_F_A * N + i / per];
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

// csrc/attack.hip's ball projection on the samples whose a != 1 (the momentum point); a sample with a == 1 holds z, which is
// projected already, and is left exactly as it is
__global__ __launch_bounds__(NT) void apgd_project_l2(float* __restrict__ x, const float* __restrict__ x0,
                                                       const double* __restrict__ dss, const float* __restrict__ fst, int N,
                                                       long per, long total, double eps, float lo, float hi) {
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < total; i += nthr) {
        const long n = i / per;
        if (fst[(long)UD_APGD_F_A * N + n] == 1.f) continue;
        const double f = l2_ball_factor(dss[n], eps);
        x[i] = l2_ball_elem(x[i], x0[i], f, lo, hi);
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

// Fast Minimum-Norm attack (unidefense_amd/attack.py: FMNRunner): the smallest perturbation that flips each sample.  The
// per-sample budget eps adapts on the device: ud_fmn_norm_parts makes the four norms an iteration needs in ONE streaming pass
// over x, x0 and g, ud_fmn_control (one thread per sample) folds them, decides and writes the new eps, ud_fmn_update steps
// and projects.  As in csrc/apgd.hip one iteration is a static sequence of launches inside a captured graph with no host
// round trip; no atomics, fixed reduction trees, NaN-transparent clamps: a replay gives the same bits.
#include "attack_common.h"

namespace {

constexpr int CHUNK = UD_FMN_CHUNK;      // elements of one sample that one workgroup of the norm pass covers (16 per thread)
constexpr int NPART = UD_FMN_PARTS;      // doubles per part

inline long fmn_parts(long per) { return (per + CHUNK - 1) / CHUNK; }

// max that keeps a NaN, whichever side it is on
__device__ __forceinline__ double nanmax(double m, double v) { return (v != v || v > m) ? v : m; }

__device__ __forceinline__ double wave_nanmax_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

struct Acc {
    double gss, gabs, dss, dmax;
};

template <bool HAS_G>
__device__ __forceinline__ void acc_elem(Acc& a, float x, float x0, float g) {
    const double d = (double)x - (double)x0;
    a.dss += d * d;
    a.dmax = nanmax(a.dmax, fabs(d));
    if (HAS_G) {
        const double gd = (double)g;
        a.gss += gd * gd;
        a.gabs += fabs(gd);
    }
}

// Part p of sample n: over i in [p CHUNK, min(per, (p + 1) CHUNK)) the sums of g^2, |g|, (x - x0)^2 and the maximum of
// |x - x0|, formed in double.  Every thread takes its elements in index order, the wave folds by shuffles, the four waves are
// combined in wave order: a fixed tree.  HAS_G == false leaves the two g entries of dst untouched.
template <bool VEC, bool HAS_G>
__global__ __launch_bounds__(NT) void fmn_norm_parts(const float* __restrict__ x, const float* __restrict__ x0,
                                                      const float* __restrict__ g, long per, double* __restrict__ dst) {
    const long n = blockIdx.y, p = blockIdx.x;
    const long lo = p * CHUNK, hi = lo + CHUNK < per ? lo + CHUNK : per;
    const float* px = x + n * per;
    const float* pb = x0 + n * per;
    const float* pg = HAS_G ? g + n * per : nullptr;
    Acc a{0.0, 0.0, 0.0, 0.0};
    if (VEC) {           // per % 4 == 0 and 16-byte aligned bases: lo and hi are multiples of 4
        for (long i = lo / 4 + threadIdx.x; i < hi / 4; i += NT) {
            const f32x4 vx = reinterpret_cast<const f32x4*>(px)[i];
            const f32x4 vb = reinterpret_cast<const f32x4*>(pb)[i];
            f32x4 vg = {0.f, 0.f, 0.f, 0.f};
            if (HAS_G) vg = reinterpret_cast<const f32x4*>(pg)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc_elem<HAS_G>(a, vx[e], vb[e], vg[e]);
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += NT) acc_elem<HAS_G>(a, px[i], pb[i], HAS_G ? pg[i] : 0.f);
    }
    a.dss = ud_wave_sum_d(a.dss);
    a.dmax = wave_nanmax_d(a.dmax);
    if (HAS_G) {
        a.gss = ud_wave_sum_d(a.gss);
        a.gabs = ud_wave_sum_d(a.gabs);
    }
    __shared__ double part[NT / 64][NPART];
    if ((threadIdx.x & 63) == 0) {
        double* w = part[threadIdx.x >> 6];
        w[UD_FMN_P_GSS] = a.gss, w[UD_FMN_P_GABS] = a.gabs, w[UD_FMN_P_DSS] = a.dss, w[UD_FMN_P_DMAX] = a.dmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc s{part[0][UD_FMN_P_GSS], part[0][UD_FMN_P_GABS], part[0][UD_FMN_P_DSS], part[0][UD_FMN_P_DMAX]};
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            s.gss += part[w][UD_FMN_P_GSS];
            s.gabs += part[w][UD_FMN_P_GABS];
            s.dss += part[w][UD_FMN_P_DSS];
            s.dmax = nanmax(s.dmax, part[w][UD_FMN_P_DMAX]);
        }
        double* o = dst + (n * gridDim.x + p) * NPART;
        if (HAS_G) o[UD_FMN_P_GSS] = s.gss, o[UD_FMN_P_GABS] = s.gabs;
        o[UD_FMN_P_DSS] = s.dss, o[UD_FMN_P_DMAX] = s.dmax;
    }
}

// ---- control --------------------------------------------------------------------------------------------------------------
// One thread per sample: the rules are stated operation by operation in include/unidefense_hip.h (tests/test_fmn_cpu.py:
// ref_fmn_control restates them in numpy).  No contraction: every double operation rounds once, as numpy's does.
__global__ __launch_bounds__(64) void fmn_control(const float* __restrict__ f, const double* __restrict__ parts_ws,
                                                   int* __restrict__ ist, float* __restrict__ fst, double* __restrict__ fac,
                                                   float* __restrict__ history, float* __restrict__ eps_history,
                                                   const float* __restrict__ alpha, const float* __restrict__ gamma,
                                                   const float* __restrict__ worst, int N, long parts, int steps, int l2,
                                                   int closing) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int k = ist[(long)UD_FMN_I_K * N + n];
    if (!closing && (k < 0 || k >= steps)) return;
    const float fk = f[n];
    const double* pw = parts_ws + (long)n * parts * NPART;
    double gss = 0.0, gabs = 0.0, dss = 0.0, dmax = 0.0;
    for (long p = 0; p < parts; ++p) {
        dss += pw[p * NPART + UD_FMN_P_DSS];
        dmax = nanmax(dmax, pw[p * NPART + UD_FMN_P_DMAX]);
        if (!closing) {
            gss += pw[p * NPART + UD_FMN_P_GSS];
            gabs += pw[p * NPART + UD_FMN_P_GABS];
        }
    }
    const float dn = (float)(l2 ? sqrt(dss) : dmax);
    float eps, best;
    int found;
    if (!closing && k == 0) {
        eps = best = __builtin_inff();
        found = 0;
    } else {
        eps = fst[(long)UD_FMN_F_EPS * N + n];
        best = fst[(long)UD_FMN_F_BEST * N + n];
        found = ist[(long)UD_FMN_I_FOUND * N + n];
    }
    const int adv = fk < 0.f;
    const int improved = adv && dn < best;
    if (improved) best = dn;
    if (closing) {
        fst[(long)UD_FMN_F_BEST * N + n] = best;
        ist[(long)UD_FMN_I_FOUND * N + n] = found | adv;
        ist[(long)UD_FMN_I_IMPROVED * N + n] = improved;
        history[(long)steps * N + n] = fk;
        return;
    }
    const double gm = (double)gamma[k], ed = (double)eps;
    double e;
    if (adv) {
        const double t = ed * (1.0 - gm), b = (double)best;
        e = t < b ? t : b;
    } else if (found) {
        e = ed * (1.0 + gm);
    } else {
        const double gq = l2 ? sqrt(gss) : gabs;
        e = (double)dn + fabs((double)fk) / (gq < 1e-12 ? 1e-12 : gq);
    }
    const double w = (double)worst[n];
    e = w < e ? w : e;
    if (e == e) eps = (float)e;
    const double g2 = sqrt(gss);
    fst[(long)UD_FMN_F_EPS * N + n] = eps;
    fst[(long)UD_FMN_F_BEST * N + n] = best;
    fac[n] = (double)alpha[k] / (g2 < 1e-12 ? 1e-12 : g2);
    ist[(long)UD_FMN_I_K * N + n] = k + 1;
    ist[(long)UD_FMN_I_FOUND * N + n] = found | adv;
    ist[(long)UD_FMN_I_IMPROVED * N + n] = improved;
    history[(long)k * N + n] = fk;
    eps_history[(long)k * N + n] = eps;
}

// ---- update ---------------------------------------------------------------------------------------------------------------
struct Sample {               // what the control left for one sample
    int improved;
    float eps;
    double fac;
};

__device__ __forceinline__ Sample load_sample(const int* __restrict__ ist, const float* __restrict__ fst,
                                              const double* __restrict__ fac, int N, long n) {
    Sample s;
    s.improved = ist[(long)UD_FMN_I_IMPROVED * N + n];
    s.eps = fst[(long)UD_FMN_F_EPS * N + n];
    s.fac = fac[n];
    return s;
}

// z = x - g fac: product and difference in double, one rounding each, then one to fp32; L-infinity: the box of the sample's
// own eps (an infinite eps gives the box (-inf, inf)), then clip
template <bool L2>
__device__ __forceinline__ float fmn_new(float x, float g, float x0, const Sample s, float lo, float hi) {
#pragma clang fp contract(off)
    const double t = (double)g * s.fac;
    const float z = (float)((double)x - t);
    return L2 ? z : proj_linf(z, x0, s.eps, lo, hi);
}

// One element (V = float) or a float4 group inside one sample (V = f32x4), i counting in units of V
template <bool L2, typename V>
__device__ __forceinline__ void fmn_update_at(float* __restrict__ x, float* __restrict__ xbest, const float* __restrict__ x0,
                                              const float* __restrict__ g, long i, const Sample s, float lo, float hi) {
    const V src = reinterpret_cast<const V*>(x)[i], gs = reinterpret_cast<const V*>(g)[i];
    if (s.improved) reinterpret_cast<V*>(xbest)[i] = src;
    V b = src, xn;
    if (!L2) b = reinterpret_cast<const V*>(x0)[i];
    if constexpr (sizeof(V) == sizeof(float)) {
        xn = fmn_new<L2>(src, gs, b, s, lo, hi);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xn[e] = fmn_new<L2>(src[e], gs[e], b[e], s, lo, hi);
    }
    reinterpret_cast<V*>(x)[i] = xn;
}

// Sample n = blockIdx.y, so no thread divides by per; VEC (per % 4 == 0 and 16-byte aligned bases): float4 groups, else scalars
template <bool L2, bool VEC>
__global__ __launch_bounds__(NT) void fmn_update(float* __restrict__ x, float* __restrict__ xbest,
                                                  const float* __restrict__ x0, const float* __restrict__ g,
                                                  const int* __restrict__ ist, const float* __restrict__ fst,
                                                  const double* __restrict__ fac, int N, long per, float lo, float hi) {
    const long n = blockIdx.y, base = n * per;
    const Sample s = load_sample(ist, fst, fac, N, n);
    const long count = VEC ? per / 4 : per, nthr = (long)gridDim.x * NT;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < count; i += nthr) {
        if (VEC)
            fmn_update_at<L2, f32x4>(x + base, xbest + base, x0 + base, g + base, i, s, lo, hi);
        else
            fmn_update_at<L2, float>(x + base, xbest + base, x0 + base, g + base, i, s, lo, hi);
    }
}

// csrc/attack.hip's ball projection with the budget read per sample; the same grid
template <bool VEC>
__global__ __launch_bounds__(NT) void fmn_project_l2(float* __restrict__ x, const float* __restrict__ x0,
                                                      const double* __restrict__ dss, const float* __restrict__ fst, int N,
                                                      long per, float lo, float hi) {
    const long n = blockIdx.y, base = n * per;
    const double f = l2_ball_factor(dss[n], (double)fst[(long)UD_FMN_F_EPS * N + n]);
    const long count = VEC ? per / 4 : per, nthr = (long)gridDim.x * NT;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < count; i += nthr) {
        if (VEC) {
            f32x4 v = reinterpret_cast<const f32x4*>(x + base)[i];
            const f32x4 b = reinterpret_cast<const f32x4*>(x0 + base)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = l2_ball_elem(v[e], b[e], f, lo, hi);
            reinterpret_cast<f32x4*>(x + base)[i] = v;
        } else {
            x[base + i] = l2_ball_elem(x[base + i], x0[base + i], f, lo, hi);
        }
    }
}

// blocks along one sample: 8 elements (two float4 or eight scalars) per thread, at most 1024
static inline unsigned sample_blocks(long count) {
    long b = (count + 2L * NT - 1) / (2L * NT);
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

inline bool norm_ok(int norm) { return norm == UD_FMN_LINF || norm == UD_FMN_L2; }

}  // namespace

extern "C" {

long ud_fmn_norms_ws_bytes(int N, long per) {
    if (!shape_ok(N, per)) return UD_EINVAL;
    return (long)N * fmn_parts(per) * NPART * (long)sizeof(double);
}

int ud_fmn_norm_parts(const float* x, const float* x0, const float* g, int N, long per, double* ws, long ws_bytes,
                      ud_stream_t stream) {
    if (!x || !x0 || !ws || !shape_ok(N, per)) return UD_EINVAL;
    const long parts = fmn_parts(per);
    if (parts > 2147483647L || ws_bytes < ud_fmn_norms_ws_bytes(N, per)) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)parts, (unsigned)N);
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x0) && (!g || aligned16(g));
    if (g) {
        if (vec)
            hipLaunchKernelGGL((fmn_norm_parts<true, true>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
        else
            hipLaunchKernelGGL((fmn_norm_parts<false, true>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
    } else {
        if (vec)
            hipLaunchKernelGGL((fmn_norm_parts<true, false>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
        else
            hipLaunchKernelGGL((fmn_norm_parts<false, false>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
    }
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_fmn_control(const float* f, const double* ws, long ws_bytes, int* ist, float* fst, double* fac, float* history,
                   float* eps_history, const float* alpha, const float* gamma, const float* worst, int N, long per, int steps,
                   int norm, int closing, ud_stream_t stream) {
    if (!f || !ws || !ist || !fst || !fac || !history || !eps_history || !alpha || !gamma || !worst) return UD_EINVAL;
    if (!shape_ok(N, per) || steps < 1 || !norm_ok(norm) || ws_bytes < ud_fmn_norms_ws_bytes(N, per)) return UD_EINVAL;
    hipLaunchKernelGGL(fmn_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ws, ist, fst, fac,
                       history, eps_history, alpha, gamma, worst, N, fmn_parts(per), steps, norm == UD_FMN_L2 ? 1 : 0,
                       closing);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_fmn_update(float* x, float* x_best, const float* x0, const float* g, const int* ist, const float* fst, const double* fac,
                  int N, long per, int norm, float lo, float hi, ud_stream_t stream) {
    if (!x || !x_best || !x0 || !g || !ist || !fst || !fac || !shape_ok(N, per) || !norm_ok(norm) || !(lo <= hi))
        return UD_EINVAL;
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x_best) && aligned16(x0) && aligned16(g);
    const dim3 grid(sample_blocks(vec ? per / 4 : per), (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
    if (norm == UD_FMN_L2) {
        if (vec)
            hipLaunchKernelGGL((fmn_update<true, true>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fst, fac, N, per, lo, hi);
        else
            hipLaunchKernelGGL((fmn_update<true, false>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fst, fac, N, per, lo, hi);
    } else {
        if (vec)
            hipLaunchKernelGGL((fmn_update<false, true>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fst, fac, N, per, lo, hi);
        else
            hipLaunchKernelGGL((fmn_update<false, false>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fst, fac, N, per, lo, hi);
    }
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_fmn_project_l2(float* x, const float* x0, const double* dss, const float* fst, int N, long per, float lo, float hi,
                      ud_stream_t stream) {
    if (!x || !x0 || !dss || !fst || !shape_ok(N, per) || !(lo <= hi)) return UD_EINVAL;
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x0);
    const dim3 grid(sample_blocks(vec ? per / 4 : per), (unsigned)N);
    if (vec)
        hipLaunchKernelGGL(fmn_project_l2<true>, grid, dim3(NT), 0, (hipStream_t)stream, x, x0, dss, fst, N, per, lo, hi);
    else
        hipLaunchKernelGGL(fmn_project_l2<false>, grid, dim3(NT), 0, (hipStream_t)stream, x, x0, dss, fst, N, per, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

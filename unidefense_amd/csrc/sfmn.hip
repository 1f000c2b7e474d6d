// Sparse minimum-norm attack (unidefense_amd/attack.py: SparseFMNRunner): csrc/fmn.hip's state machine with an L1 or an L0
// budget per sample.  What is new is the projection: the L1 ball needs the soft threshold tau with sum max(a - tau, 0) = eps
// and the L0 "ball" needs the (kk + 1)-th largest |z - x0|, both per sample over all `per` elements and inside the captured
// iteration.  ud_sfmn_select finds that one number per sample with ONE workgroup per sample that re-reads the sample (from L2 /
// the Infinity Cache: 768 KB at 3 x 256 x 256 does not fit the LDS) a fixed number of times; ud_sfmn_apply is the one pass that
// writes x_best and x.  z is formed by ONE device function (sfmn_z) from x, g and fac in both, so it never needs a buffer.
// No floating-point atomics, fixed reduction trees, every loop has a compile-time trip count or runs over the sample once:
// a replay gives the same bits and a NaN cannot keep anything alive.
#include "attack_common.h"

namespace {

constexpr int CHUNK = UD_SFMN_CHUNK;     // elements of one sample that one workgroup of the norm pass covers (16 per thread)
constexpr int NPART = UD_SFMN_PARTS;     // doubles per part
constexpr int ST = 1024;                 // threads of the select workgroup: 16 waves on one CU
constexpr int SW = ST / 64;

inline long sfmn_parts(long per) { return (per + CHUNK - 1) / CHUNK; }

// max that keeps a NaN, whichever side it is on
__device__ __forceinline__ double nanmax(double m, double v) { return (v != v || v > m) ? v : m; }

__device__ __forceinline__ double wave_nanmax_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- norm parts ------------------------------------------------------------------------------------------------------------
struct Acc {
    double gss, gmax, dabs, dcnt;
};

template <bool HAS_G>
__device__ __forceinline__ void acc_elem(Acc& a, float x, float x0, float g) {
    const double d = (double)x - (double)x0;
    a.dabs += fabs(d);
    a.dcnt += x != x0 ? 1.0 : 0.0;
    if (HAS_G) {
        const double gd = (double)g;
        a.gss += gd * gd;
        a.gmax = nanmax(a.gmax, fabs(gd));
    }
}

// Part p of sample n: over i in [p CHUNK, min(per, (p + 1) CHUNK)) the sum of g^2, the maximum of |g|, the sum of |x - x0| and
// the number of x != x0 (a double: an exact integer), formed in double.  csrc/fmn.hip's tree: every thread takes its elements in
// index order, the wave folds by shuffles, the four waves are combined in wave order.  HAS_G == false leaves the two g entries.
template <bool VEC, bool HAS_G>
__global__ __launch_bounds__(NT) void sfmn_norm_parts(const float* __restrict__ x, const float* __restrict__ x0,
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
    a.dabs = ud_wave_sum_d(a.dabs);
    a.dcnt = ud_wave_sum_d(a.dcnt);
    if (HAS_G) {
        a.gss = ud_wave_sum_d(a.gss);
        a.gmax = wave_nanmax_d(a.gmax);
    }
    __shared__ double part[NT / 64][NPART];
    if ((threadIdx.x & 63) == 0) {
        double* w = part[threadIdx.x >> 6];
        w[UD_SFMN_P_GSS] = a.gss, w[UD_SFMN_P_GMAX] = a.gmax, w[UD_SFMN_P_DABS] = a.dabs, w[UD_SFMN_P_DCNT] = a.dcnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc s{part[0][UD_SFMN_P_GSS], part[0][UD_SFMN_P_GMAX], part[0][UD_SFMN_P_DABS], part[0][UD_SFMN_P_DCNT]};
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            s.gss += part[w][UD_SFMN_P_GSS];
            s.gmax = nanmax(s.gmax, part[w][UD_SFMN_P_GMAX]);
            s.dabs += part[w][UD_SFMN_P_DABS];
            s.dcnt += part[w][UD_SFMN_P_DCNT];
        }
        double* o = dst + (n * gridDim.x + p) * NPART;
        if (HAS_G) o[UD_SFMN_P_GSS] = s.gss, o[UD_SFMN_P_GMAX] = s.gmax;
        o[UD_SFMN_P_DABS] = s.dabs, o[UD_SFMN_P_DCNT] = s.dcnt;
    }
}

// ---- control --------------------------------------------------------------------------------------------------------------
// One thread per sample: the rules are stated operation by operation in include/unidefense_hip.h (tests/test_sparse_fmn_cpu.py:
// ref_sfmn_control restates them in Python floats).  No contraction: every double operation rounds once.
__global__ __launch_bounds__(64) void sfmn_control(const float* __restrict__ f, const double* __restrict__ parts_ws,
                                                    int* __restrict__ ist, float* __restrict__ fst, double* __restrict__ fac,
                                                    float* __restrict__ history, float* __restrict__ eps_history,
                                                    const float* __restrict__ alpha, const float* __restrict__ gamma,
                                                    const float* __restrict__ worst, int N, long parts, int steps, int l0,
                                                    float lo, float hi, int closing) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int k = ist[(long)UD_SFMN_I_K * N + n];
    if (!closing && (k < 0 || k >= steps)) return;
    const float fk = f[n];
    const double* pw = parts_ws + (long)n * parts * NPART;
    double gss = 0.0, gmax = 0.0, dabs = 0.0, dcnt = 0.0;
    for (long p = 0; p < parts; ++p) {
        dabs += pw[p * NPART + UD_SFMN_P_DABS];
        dcnt += pw[p * NPART + UD_SFMN_P_DCNT];
        if (!closing) {
            gss += pw[p * NPART + UD_SFMN_P_GSS];
            gmax = nanmax(gmax, pw[p * NPART + UD_SFMN_P_GMAX]);
        }
    }
    const float dn = (float)(l0 ? dcnt : dabs);
    float eps, best;
    int found;
    if (!closing && k == 0) {
        eps = best = __builtin_inff();
        found = 0;
    } else {
        eps = fst[(long)UD_SFMN_F_EPS * N + n];
        best = fst[(long)UD_SFMN_F_BEST * N + n];
        found = ist[(long)UD_SFMN_I_FOUND * N + n];
    }
    const int adv = fk < 0.f;
    const int improved = adv && dn < best;
    if (improved) best = dn;
    if (closing) {
        fst[(long)UD_SFMN_F_BEST * N + n] = best;
        ist[(long)UD_SFMN_I_FOUND * N + n] = found | adv;
        ist[(long)UD_SFMN_I_IMPROVED * N + n] = improved;
        history[(long)steps * N + n] = fk;
        return;
    }
    const double gm = (double)gamma[k], ed = (double)eps;
    double e;
    if (adv) {
        const double b = (double)best;
        double t = ed * (1.0 - gm);
        if (l0) {
            t = floor(t);
            const double u = ed - 1.0;
            t = u < t ? u : t;
        }
        e = t < b ? t : b;
    } else if (found) {
        e = ed * (1.0 + gm);
        if (l0) {
            e = floor(e);
            const double u = ed + 1.0;
            e = u > e ? u : e;
        }
    } else {
        const double gq = gmax < 1e-12 ? 1e-12 : gmax;
        if (l0) {
            const double w = (double)hi - (double)lo;
            double c = ceil(fabs((double)fk) / (w * gq));
            c = c < 1.0 ? 1.0 : c;
            e = (double)dn + c;
        } else {
            e = (double)dn + fabs((double)fk) / gq;
        }
    }
    if (l0) e = e < 0.0 ? 0.0 : e;
    const double w = (double)worst[n];
    e = w < e ? w : e;
    if (e == e) eps = (float)e;
    const double g2 = sqrt(gss);
    fst[(long)UD_SFMN_F_EPS * N + n] = eps;
    fst[(long)UD_SFMN_F_BEST * N + n] = best;
    fac[n] = (double)alpha[k] / (g2 < 1e-12 ? 1e-12 : g2);
    ist[(long)UD_SFMN_I_K * N + n] = k + 1;
    ist[(long)UD_SFMN_I_FOUND * N + n] = found | adv;
    ist[(long)UD_SFMN_I_IMPROVED * N + n] = improved;
    history[(long)k * N + n] = fk;
    eps_history[(long)k * N + n] = eps;
}

// ---- the step, written once --------------------------------------------------------------------------------------------------
// z = x - g fac: product and difference in double, one rounding each, then one to fp32 (csrc/fmn.hip's fmn_new)
__device__ __forceinline__ float sfmn_z(float x, float g, double fac) {
#pragma clang fp contract(off)
    const double t = (double)g * fac;
    return (float)((double)x - t);
}

// Every thread of the select workgroup visits its elements of one sample in index order: fn(a), a = |(double)z - (double)x0|
template <bool VEC, typename F>
__device__ __forceinline__ void for_each_a(const float* __restrict__ px, const float* __restrict__ pg,
                                           const float* __restrict__ pb, long per, double fac, F&& fn) {
    if (VEC) {
        for (long i = threadIdx.x; i < per / 4; i += ST) {
            const f32x4 vx = reinterpret_cast<const f32x4*>(px)[i];
            const f32x4 vg = reinterpret_cast<const f32x4*>(pg)[i];
            const f32x4 vb = reinterpret_cast<const f32x4*>(pb)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) fn(fabs((double)sfmn_z(vx[e], vg[e], fac) - (double)vb[e]));
        }
    } else {
        for (long i = threadIdx.x; i < per; i += ST) fn(fabs((double)sfmn_z(px[i], pg[i], fac) - (double)pb[i]));
    }
}

// ---- select, L1 --------------------------------------------------------------------------------------------------------------
constexpr int L1_BITS = 44;              // of a's bit pattern, from the top: sign, exponent and 32 bits of the significand
constexpr int L1_LEVELS = L1_BITS / 2;   // two bits per pass

// One pass over the sample: for the three thresholds t the number C and the sum S of the a > t (a NaN a is above nothing).
// Threads in index order, wave shuffles, waves in order; every thread ends up with the same six numbers.
template <bool VEC>
__device__ __forceinline__ void above3(const float* px, const float* pg, const float* pb, long per, double fac, const double t[3],
                                       double (*sh)[6], double C[3], double S[3]) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const double t0 = t[0], t1 = t[1], t2 = t[2];
    for_each_a<VEC>(px, pg, pb, per, fac, [&](double a) {
        const bool b0 = a > t0, b1 = a > t1, b2 = a > t2;
        c0 += b0 ? 1.0 : 0.0, s0 += b0 ? a : 0.0;
        c1 += b1 ? 1.0 : 0.0, s1 += b1 ? a : 0.0;
        c2 += b2 ? 1.0 : 0.0, s2 += b2 ? a : 0.0;
    });
    c0 = ud_wave_sum_d(c0), c1 = ud_wave_sum_d(c1), c2 = ud_wave_sum_d(c2);
    s0 = ud_wave_sum_d(s0), s1 = ud_wave_sum_d(s1), s2 = ud_wave_sum_d(s2);
    __syncthreads();                     // the previous pass's readers are done with sh
    if ((threadIdx.x & 63) == 0) {
        double* w = sh[threadIdx.x >> 6];
        w[0] = c0, w[1] = c1, w[2] = c2, w[3] = s0, w[4] = s1, w[5] = s2;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        double c = sh[0][b], s = sh[0][3 + b];
#pragma unroll 2
        for (int w = 1; w < SW; ++w) c += sh[w][b], s += sh[w][3 + b];
        C[b] = c, S[b] = s;
    }
}

// Sample n = blockIdx.x.  G(t) = sum max(a - t, 0) falls as t rises; the kernel looks for the smallest threshold pattern v (the
// top L1_BITS bits of a double, the bits below them all ones) with G(v) <= eps, two bits per pass, and keeps (C, S) of the
// largest threshold it saw with G > eps: that one is v's predecessor, whose a > t are the support, and
// tau = (S - eps) / C.  At most L1_LEVELS + 1 passes, whatever the data; fewer once no a lies between the largest threshold
// with G > eps and the smallest with G <= eps any more (the counts above the two are equal): the support, its sum in the same
// tree and so tau are then what the remaining passes would give, bit for bit.  thr[n] = -1: nothing to project (sum a <= eps).
template <bool VEC>
__global__ __launch_bounds__(ST) void sfmn_select_l1(const float* __restrict__ x, const float* __restrict__ x0,
                                                      const float* __restrict__ g, const float* __restrict__ fst,
                                                      const double* __restrict__ facs, int N, long per,
                                                      double* __restrict__ thr) {
#pragma clang fp contract(off)
    __shared__ double sh[SW][6];
    const long n = blockIdx.x;
    const float* px = x + n * per;
    const float* pg = g + n * per;
    const float* pb = x0 + n * per;
    const double eps = (double)fst[(long)UD_SFMN_F_EPS * N + n], fac = facs[n];
    double C[3], S[3];
    double t[3] = {-1.0, -1.0, -1.0};
    above3<VEC>(px, pg, pb, per, fac, t, sh, C, S);          // every a that is a number
    if (S[0] <= eps) {                                       // inside the ball, or an infinite eps (uniform over the workgroup)
        if (threadIdx.x == 0) thr[n] = -1.0;
        return;
    }
    if (!(eps > 0.0)) {                                      // a ball of radius 0 (a sample that is adversarial as it is): x0
        if (threadIdx.x == 0) thr[n] = (double)__builtin_inff();
        return;
    }
    double rc = C[0], rs = S[0], uc = 0.0;                   // counts above the largest threshold with G > eps, the smallest with G <= eps
    unsigned long long prefix = 0;
#pragma unroll 1
    for (int L = 0; L < L1_LEVELS && rc != uc; ++L) {        // rc == uc: no a is left between the two, the support is known
        const int shift = L1_BITS - 2 * (L + 1);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const unsigned long long key = (((prefix << 2) | (unsigned long long)b) << shift) | ((1ULL << shift) - 1ULL);
            t[b] = __longlong_as_double((long long)((key << (64 - L1_BITS)) | ((1ULL << (64 - L1_BITS)) - 1ULL)));
        }
        above3<VEC>(px, pg, pb, per, fac, t, sh, C, S);
        int pick = 3;
#pragma unroll
        for (int b = 2; b >= 0; --b)
            if (C[b] == 0.0 || S[b] - C[b] * t[b] <= eps) pick = b;
        if (pick > 0) rc = C[pick - 1], rs = S[pick - 1];
        if (pick < 3) uc = C[pick];
        prefix = (prefix << 2) | (unsigned long long)pick;
    }
    if (threadIdx.x == 0) {
        double tau = rc > 0.0 ? (rs - eps) / rc : (double)__builtin_inff();
        tau = tau < 0.0 ? 0.0 : tau;
        thr[n] = tau;
    }
}

// ---- select, L0 --------------------------------------------------------------------------------------------------------------
constexpr int L0_DIGIT = 11, L0_BINS = 1 << L0_DIGIT, L0_LEVELS = 6;       // 6 x 11 bits cover the 64 of a double

// Sample n = blockIdx.x: the (kk + 1)-th largest a, counting multiplicity, kk = eps read as an integer: a radix select on a's
// bit pattern (non-negative doubles order as unsigned integers; a NaN a counts as 0), 11 bits per pass, counts only (integer LDS
// atomics: order-free).  thr[n] = -1: everything is kept (eps infinite or kk >= per).
template <bool VEC>
__global__ __launch_bounds__(ST) void sfmn_select_l0(const float* __restrict__ x, const float* __restrict__ x0,
                                                      const float* __restrict__ g, const float* __restrict__ fst,
                                                      const double* __restrict__ facs, int N, long per,
                                                      double* __restrict__ thr) {
    __shared__ unsigned hist[L0_BINS];
    __shared__ unsigned wtot[SW];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_need;
    const long n = blockIdx.x;
    const float eps = fst[(long)UD_SFMN_F_EPS * N + n];
    if (!(eps < (float)per)) {                               // infinite (or NaN) eps, kk >= per: uniform over the workgroup
        if (threadIdx.x == 0) thr[n] = -1.0;
        return;
    }
    if (!(eps >= 1.f)) {                                     // kk = 0 (a sample that is adversarial as it is): nothing is kept
        if (threadIdx.x == 0) thr[n] = (double)__builtin_inff();
        return;
    }
    const float* px = x + n * per;
    const float* pg = g + n * per;
    const float* pb = x0 + n * per;
    const double fac = facs[n];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long prefix = 0;
    unsigned need = (unsigned)eps + 1u;                      // 2 .. per: the histogram of level 0 holds per entries
    if (threadIdx.x == 0) s_prefix = 0, s_need = need;
#pragma unroll
    for (int L = 0; L < L0_LEVELS; ++L) {
        const int shift = L0_DIGIT * (L0_LEVELS - 1 - L);
        hist[2 * threadIdx.x] = 0, hist[2 * threadIdx.x + 1] = 0;
        __syncthreads();
        for_each_a<VEC>(px, pg, pb, per, fac, [&](double a) {
            const unsigned long long key = a == a ? (unsigned long long)__double_as_longlong(a) : 0ULL;
            if (L == 0 || (key >> (L == 0 ? 0 : shift + L0_DIGIT)) == prefix)
                atomicAdd(&hist[(unsigned)(key >> shift) & (L0_BINS - 1)], 1u);
        });
        __syncthreads();
        // bins from the top: thread c holds bins 2c and 2c + 1; v = the entries of the wave's bins from this thread's on
        const unsigned h0 = hist[2 * threadIdx.x], h1 = hist[2 * threadIdx.x + 1], s = h0 + h1;
        unsigned v = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_down(v, o, 64);
            if (lane + o < 64) v += u;
        }
        if (lane == 0) wtot[wave] = v;
        __syncthreads();
        unsigned above = v - s;                              // entries in bins above 2c + 1
        for (int w = wave + 1; w < SW; ++w) above += wtot[w];
        if (above < need && need <= above + s) {             // exactly one thread: the need-th largest lies in its bins
            const bool top = above + h1 >= need;
            s_prefix = (prefix << L0_DIGIT) | (unsigned long long)(2 * threadIdx.x + (top ? 1 : 0));
            s_need = need - above - (top ? 0u : h1);
        }
        __syncthreads();
        prefix = s_prefix, need = s_need;
    }
    if (threadIdx.x == 0) thr[n] = __longlong_as_double((long long)prefix);
}

// ---- apply -----------------------------------------------------------------------------------------------------------------
// One element: what x becomes.  A NaN a (a NaN gradient element) stays a NaN in x.
template <bool L0>
__device__ __forceinline__ float sfmn_new(float x, float g, float x0, double fac, double thr, float lo, float hi) {
#pragma clang fp contract(off)
    const float z = sfmn_z(x, g, fac);
    const double d = (double)z - (double)x0, a = fabs(d);
    if (a != a) return z;
    if (thr < 0.0) return clampf(z, lo, hi);                 // nothing to project: z untouched before the clamp
    if (L0) return clampf(a > thr ? z : x0, lo, hi);
    double m = a - thr;
    m = m > 0.0 ? m : 0.0;
    return clampf((float)((double)x0 + (d < 0.0 ? -m : m)), lo, hi);
}

template <bool L0, typename V>
__device__ __forceinline__ void sfmn_apply_at(float* __restrict__ x, float* __restrict__ xbest, const float* __restrict__ x0,
                                              const float* __restrict__ g, long i, int improved, double fac, double thr,
                                              float lo, float hi) {
    const V src = reinterpret_cast<const V*>(x)[i], gs = reinterpret_cast<const V*>(g)[i];
    const V b = reinterpret_cast<const V*>(x0)[i];
    if (improved) reinterpret_cast<V*>(xbest)[i] = src;
    V xn;
    if constexpr (sizeof(V) == sizeof(float)) {
        xn = sfmn_new<L0>(src, gs, b, fac, thr, lo, hi);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xn[e] = sfmn_new<L0>(src[e], gs[e], b[e], fac, thr, lo, hi);
    }
    reinterpret_cast<V*>(x)[i] = xn;
}

// Sample n = blockIdx.y, csrc/fmn.hip's grid; VEC (per % 4 == 0 and 16-byte aligned bases): float4 groups, else scalars
template <bool L0, bool VEC>
__global__ __launch_bounds__(NT) void sfmn_apply(float* __restrict__ x, float* __restrict__ xbest, const float* __restrict__ x0,
                                                  const float* __restrict__ g, const int* __restrict__ ist,
                                                  const double* __restrict__ facs, const double* __restrict__ thrs, int N,
                                                  long per, float lo, float hi) {
    const long n = blockIdx.y, base = n * per;
    const int improved = ist[(long)UD_SFMN_I_IMPROVED * N + n];
    const double fac = facs[n], thr = thrs[n];
    const long count = VEC ? per / 4 : per, nthr = (long)gridDim.x * NT;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < count; i += nthr) {
        if (VEC)
            sfmn_apply_at<L0, f32x4>(x + base, xbest + base, x0 + base, g + base, i, improved, fac, thr, lo, hi);
        else
            sfmn_apply_at<L0, float>(x + base, xbest + base, x0 + base, g + base, i, improved, fac, thr, lo, hi);
    }
}

// blocks along one sample: 8 elements (two float4 or eight scalars) per thread, at most 1024
static inline unsigned sample_blocks(long count) {
    long b = (count + 2L * NT - 1) / (2L * NT);
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

inline bool norm_ok(int norm) { return norm == UD_SFMN_L1 || norm == UD_SFMN_L0; }

// the count of an L0 run lives in an fp32 state row: exact below 2^24
inline bool per_ok(int norm, long per) { return norm != UD_SFMN_L0 || per < UD_SFMN_L0_MAX_PER; }

}  // namespace

extern "C" {

long ud_sfmn_norms_ws_bytes(int N, long per) {
    if (!shape_ok(N, per)) return UD_EINVAL;
    return (long)N * sfmn_parts(per) * NPART * (long)sizeof(double);
}

int ud_sfmn_norm_parts(const float* x, const float* x0, const float* g, int N, long per, double* ws, long ws_bytes,
                       ud_stream_t stream) {
    if (!x || !x0 || !ws || !shape_ok(N, per)) return UD_EINVAL;
    const long parts = sfmn_parts(per);
    if (parts > 2147483647L || ws_bytes < ud_sfmn_norms_ws_bytes(N, per)) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)parts, (unsigned)N);
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x0) && (!g || aligned16(g));
    if (g) {
        if (vec)
            hipLaunchKernelGGL((sfmn_norm_parts<true, true>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
        else
            hipLaunchKernelGGL((sfmn_norm_parts<false, true>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
    } else {
        if (vec)
            hipLaunchKernelGGL((sfmn_norm_parts<true, false>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
        else
            hipLaunchKernelGGL((sfmn_norm_parts<false, false>), grid, dim3(NT), 0, s, x, x0, g, per, ws);
    }
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_sfmn_control(const float* f, const double* ws, long ws_bytes, int* ist, float* fst, double* fac, float* history,
                    float* eps_history, const float* alpha, const float* gamma, const float* worst, int N, long per, int steps,
                    int norm, float lo, float hi, int closing, ud_stream_t stream) {
    if (!f || !ws || !ist || !fst || !fac || !history || !eps_history || !alpha || !gamma || !worst) return UD_EINVAL;
    if (!shape_ok(N, per) || steps < 1 || !norm_ok(norm) || !per_ok(norm, per) || !(lo < hi)) return UD_EINVAL;
    if (ws_bytes < ud_sfmn_norms_ws_bytes(N, per)) return UD_EINVAL;
    hipLaunchKernelGGL(sfmn_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ws, ist, fst, fac,
                       history, eps_history, alpha, gamma, worst, N, sfmn_parts(per), steps, norm == UD_SFMN_L0 ? 1 : 0, lo, hi,
                       closing);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_sfmn_select(const float* x, const float* x0, const float* g, const float* fst, const double* fac, double* thr, int N,
                   long per, int norm, ud_stream_t stream) {
    if (!x || !x0 || !g || !fst || !fac || !thr || !shape_ok(N, per) || !norm_ok(norm) || !per_ok(norm, per)) return UD_EINVAL;
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)N);
    if (norm == UD_SFMN_L0) {
        if (vec)
            hipLaunchKernelGGL(sfmn_select_l0<true>, grid, dim3(ST), 0, s, x, x0, g, fst, fac, N, per, thr);
        else
            hipLaunchKernelGGL(sfmn_select_l0<false>, grid, dim3(ST), 0, s, x, x0, g, fst, fac, N, per, thr);
    } else {
        if (vec)
            hipLaunchKernelGGL(sfmn_select_l1<true>, grid, dim3(ST), 0, s, x, x0, g, fst, fac, N, per, thr);
        else
            hipLaunchKernelGGL(sfmn_select_l1<false>, grid, dim3(ST), 0, s, x, x0, g, fst, fac, N, per, thr);
    }
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_sfmn_apply(float* x, float* x_best, const float* x0, const float* g, const int* ist, const double* fac, const double* thr,
                  int N, long per, int norm, float lo, float hi, ud_stream_t stream) {
    if (!x || !x_best || !x0 || !g || !ist || !fac || !thr || !shape_ok(N, per) || !norm_ok(norm) || !(lo <= hi))
        return UD_EINVAL;
    const bool vec = per % 4 == 0 && aligned16(x) && aligned16(x_best) && aligned16(x0) && aligned16(g);
    const dim3 grid(sample_blocks(vec ? per / 4 : per), (unsigned)N);
    hipStream_t s = (hipStream_t)stream;
    if (norm == UD_SFMN_L0) {
        if (vec)
            hipLaunchKernelGGL((sfmn_apply<true, true>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fac, thr, N, per, lo, hi);
        else
            hipLaunchKernelGGL((sfmn_apply<true, false>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fac, thr, N, per, lo, hi);
    } else {
        if (vec)
            hipLaunchKernelGGL((sfmn_apply<false, true>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fac, thr, N, per, lo, hi);
        else
            hipLaunchKernelGGL((sfmn_apply<false, false>), grid, dim3(NT), 0, s, x, x_best, x0, g, ist, fac, thr, N, per, lo, hi);
    }
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// The kernel work of the decision-based minimum-norm attack (HopSkipJump; unidefense_amd/hsj.py: HSJRunner).  A query is
// propose -> forward -> control; the per-sample scalars of the search live in device state (ist, fst: the header's rows), so a
// query kind is a static launch sequence inside a captured graph and all samples walk one schedule that the host knows.
//   ud_hsj_propose  : one streaming pass that writes the next point to be judged (or settles the boundary point)
//   ud_hsj_control  : one thread per sample: the logits row becomes ONE bit, the bit advances the sample's state
//   ud_hsj_dist     : per sample |a - b|^2 and max |a - b| in double, one workgroup per sample, a fixed reduction order
//   ud_hsj_estimate : v = sum_b (phi_b - mean phi) u_b with all B directions re-made in registers, ascending b
//
// The directions are made from csrc/philox.h's Philox words (the uniform rule is philox.h's, the Gaussian one is gaussian_pair64
// below, not smooth.hip's fp32 one): a pure function of (seed, sample id, draw, element), element 4 q + j = word j of the
// quad q.  Nothing depends on the sample's row, on N, on the launch geometry or on the float4 / scalar path.  Every fp32
// expression is rounded once per operation in the order written (no contraction): hsj.ref_hsj_propose restates them in numpy.
#include <climits>

#include "attack_common.h"
#include "philox.h"

namespace {

// Box-Muller on philox.h's exact uniforms with DOUBLE library functions, rounded to fp32 once: the decisions of a whole attack
// are compared row for row with a numpy restatement, which an fp32 logf / sincospif (a few ulp off, so another fp32 value in
// a good part of the elements) would not allow.  The double functions are right to ~1e-16: the fp32 value is the restatement's
// but for about one element in 10^8.
__device__ __forceinline__ void gaussian_pair64(uint32_t wa, uint32_t wb, float& za, float& zb) {
    const double u1 = (double)((wa >> 8) + 1u) * (1.0 / 16777216.0);
    const double h = (double)(wb >> 8) * (2.0 / 16777216.0);
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(h, &s, &c);
    za = (float)(r * c);
    zb = (float)(r * s);
}

// UD_SMOOTH_UNIFORM: philox.h's; UD_SMOOTH_GAUSSIAN: the double Box-Muller above
template <int MODE>
__device__ __forceinline__ void hsj_noise_quad(const Words& p, float t[4]) {
    if (MODE == UD_SMOOTH_UNIFORM) {
        noise_quad<UD_SMOOTH_UNIFORM>(p, t);
    } else {
        gaussian_pair64(p.w[0], p.w[1], t[0], t[1]);
        gaussian_pair64(p.w[2], p.w[3], t[2], t[3]);
    }
}

__device__ __forceinline__ bool live_of(const int* __restrict__ ist, int N, int n) {
    return ist[(long)UD_HSJ_I_ACTIVE * N + n] != 0 && ist[(long)UD_HSJ_I_HAS * N + n] != 0;
}

// who takes part in a pass of `mode`, and the pass's per-sample scalar
template <int MODE, int NORM>
__device__ __forceinline__ bool propose_scalar(const int* __restrict__ ist, const float* __restrict__ fst, int N, int n, float aux,
                                               float& s, bool& plain) {
#pragma clang fp contract(off)
    s = 0.f;
    plain = false;
    if (MODE == UD_HSJ_P_COPY) return true;
    const bool active = ist[(long)UD_HSJ_I_ACTIVE * N + n] != 0, has = ist[(long)UD_HSJ_I_HAS * N + n] != 0;
    if (MODE == UD_HSJ_P_COPY_SEEK || MODE == UD_HSJ_P_NOISE) return active && !has;
    if (!(active && has)) return false;
    if (MODE == UD_HSJ_P_BISECT) {
        s = 0.5f * (fst[(long)UD_HSJ_F_LO * N + n] + fst[(long)UD_HSJ_F_HI * N + n]);
    } else if (MODE == UD_HSJ_P_SETTLE) {
        s = fst[(long)UD_HSJ_F_HI * N + n];
        plain = ist[(long)UD_HSJ_I_MOVED * N + n] == 0;      // the upper end never moved: x_cur itself is the verified point
    } else if (MODE == UD_HSJ_P_PROBE) {
        const float d = fst[(long)UD_HSJ_F_DELTA * N + n];
        s = NORM == UD_HSJ_L2 ? d * aux : d;
    } else {                                                 // UD_HSJ_P_STEP
        if (ist[(long)UD_HSJ_I_STEPDONE * N + n] != 0) return false;
        const float xi = fst[(long)UD_HSJ_F_XI * N + n];
        s = NORM == UD_HSJ_L2 ? xi * fst[(long)UD_HSJ_F_INVN * N + n] : xi;
    }
    return true;
}

// one element: a = the pass's source (src, x_cur or x_bd), b = x0 (bisect, settle) or v (step), t = the element's noise
template <int MODE, int NORM>
__device__ __forceinline__ float propose_elem(float a, float b, float t, float s, bool plain, float lo, float hi, float mid,
                                              float half) {
#pragma clang fp contract(off)
    if (MODE == UD_HSJ_P_COPY || MODE == UD_HSJ_P_COPY_SEEK) return a;
    if (MODE == UD_HSJ_P_NOISE) {
        const float p = half * t;
        return clampf(mid + p, lo, hi);
    }
    if (MODE == UD_HSJ_P_BISECT || MODE == UD_HSJ_P_SETTLE) {
        if (plain) return a;
        if (NORM == UD_HSJ_LINF) return proj_linf(a, b, s, lo, hi);
        const float d = a - b;
        const float p = s * d;
        return clampf(b + p, lo, hi);
    }
    const float p = s * (MODE == UD_HSJ_P_PROBE ? t : b);
    return clampf(a + p, lo, hi);
}

template <int MODE, int NORM, bool VEC>
__global__ __launch_bounds__(NT) void hsj_propose(float* dst, const float* a, const float* b, const long long* __restrict__ ids,
                                                  const int* __restrict__ ist, const float* __restrict__ fst, int N, long per,
                                                  long quads, float lo, float hi, float aux, uint32_t seed_lo, uint32_t seed_hi) {
    const int n = blockIdx.y;
    float s;
    bool plain;
    if (!propose_scalar<MODE, NORM>(ist, fst, N, n, aux, s, plain)) return;      // an idle sample costs nothing beyond this
    constexpr bool NOISY = MODE == UD_HSJ_P_NOISE || MODE == UD_HSJ_P_PROBE;
    constexpr bool READS_A = MODE != UD_HSJ_P_NOISE;
    constexpr bool READS_B = MODE == UD_HSJ_P_BISECT || MODE == UD_HSJ_P_SETTLE || MODE == UD_HSJ_P_STEP;
    constexpr int NOISE = (MODE == UD_HSJ_P_PROBE && NORM == UD_HSJ_L2) ? UD_SMOOTH_GAUSSIAN : UD_SMOOTH_UNIFORM;
    const unsigned long long id = NOISY ? (unsigned long long)ids[n] : 0ull;
    const uint32_t draw = NOISY ? (uint32_t)ist[(long)UD_HSJ_I_DRAW * N + n] : 0u;
    const float mid = 0.5f * (lo + hi), half = 0.5f * (hi - lo);
    const float* as = READS_A ? a + (long)n * per : nullptr;
    const float* bs = READS_B ? b + (long)n * per : nullptr;
    float* ds = dst + (long)n * per;
    const long nthr = (long)gridDim.x * NT;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISY) {
            const Words p = philox4x32_10((uint32_t)q, draw, (uint32_t)id, (uint32_t)(id >> 32), seed_lo, seed_hi);
            hsj_noise_quad<NOISE>(p, t);
        }
        if (VEC) {
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f}, o;
            if (READS_A) va = reinterpret_cast<const f32x4*>(as)[q];
            if (READS_B) vb = reinterpret_cast<const f32x4*>(bs)[q];
            o.x = propose_elem<MODE, NORM>(va.x, vb.x, t[0], s, plain, lo, hi, mid, half);
            o.y = propose_elem<MODE, NORM>(va.y, vb.y, t[1], s, plain, lo, hi, mid, half);
            o.z = propose_elem<MODE, NORM>(va.z, vb.z, t[2], s, plain, lo, hi, mid, half);
            o.w = propose_elem<MODE, NORM>(va.w, vb.w, t[3], s, plain, lo, hi, mid, half);
            reinterpret_cast<f32x4*>(ds)[q] = o;
        } else {
            const long e0 = 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < per)
                    ds[e0 + j] = propose_elem<MODE, NORM>(READS_A ? as[e0 + j] : 0.f, READS_B ? bs[e0 + j] : 0.f, t[j], s, plain, lo,
                                                          hi, mid, half);
        }
    }
}

template <int MODE, int NORM>
int launch_propose(float* dst, const float* a, const float* b, const long long* ids, const int* ist, const float* fst, int N,
                   long per, float lo, float hi, float aux, unsigned long long seed, hipStream_t s) {
    const long quads = (per + 3) / 4;
    const dim3 grid((unsigned)ew_blocks(quads), (unsigned)N);
    const uint32_t slo = (uint32_t)seed, shi = (uint32_t)(seed >> 32);
    if (per % 4 == 0 && aligned16(dst) && aligned16(a) && aligned16(b))
        hipLaunchKernelGGL((hsj_propose<MODE, NORM, true>), grid, dim3(NT), 0, s, dst, a, b, ids, ist, fst, N, per, quads, lo, hi, aux,
                           slo, shi);
    else
        hipLaunchKernelGGL((hsj_propose<MODE, NORM, false>), grid, dim3(NT), 0, s, dst, a, b, ids, ist, fst, N, per, quads, lo, hi,
                           aux, slo, shi);
    UD_LAUNCH_CHECK();
    return 0;
}

// ---- control: one thread per sample; only its own column of every table is touched ----------------------------------------------
struct ControlArgs {
    const float* logits;
    const long long* y;
    const double* nrm;
    int* ist;
    float* fst;
    signed char* phi;
    signed char* decisions;
    float* history;
    const float* xis;
    int N, C, Q, max_probes, steps;
    float delta0, inv_d, dfloor;
};

template <int NORM>
__global__ __launch_bounds__(64) void hsj_control(int mode, ControlArgs c) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * 64 + threadIdx.x;
    const int N = c.N;
    if (n >= N) return;
    int* ist = c.ist;
    float* fst = c.fst;
#define I_(row) ist[(long)(row) * N + n]
#define F_(row) fst[(long)(row) * N + n]
    const bool live = I_(UD_HSJ_I_ACTIVE) != 0 && I_(UD_HSJ_I_HAS) != 0;
    if (mode == UD_HSJ_C_BEGIN) {
        if (I_(UD_HSJ_I_ACTIVE) != 0 && I_(UD_HSJ_I_HAS) == 0) I_(UD_HSJ_I_ACTIVE) = 0;      // no adversarial start: idle from here on
        if (live) {
            F_(UD_HSJ_F_LO) = 0.f;
            F_(UD_HSJ_F_HI) = NORM == UD_HSJ_L2 ? 1.f : (float)c.nrm[(long)N + n];
            I_(UD_HSJ_I_MOVED) = 0;
        }
        return;
    }
    if (mode == UD_HSJ_C_DIST) {
        const int t = I_(UD_HSJ_I_T);
        float r;
        if (live) {
            const float dist = NORM == UD_HSJ_L2 ? (float)sqrt(c.nrm[n]) : (float)c.nrm[(long)N + n];
            const bool keep = dist < F_(UD_HSJ_F_BEST);
            if (keep) F_(UD_HSJ_F_BEST) = dist;
            r = F_(UD_HSJ_F_BEST);
            F_(UD_HSJ_F_DIST) = dist;
            I_(UD_HSJ_I_KEEP) = keep ? 1 : 0;
            I_(UD_HSJ_I_ACCEPT) = 1;
            const float d = t == 0 ? c.delta0 : dist * c.inv_d;
            F_(UD_HSJ_F_DELTA) = d > c.dfloor ? d : c.dfloor;
            if (t >= 0 && t < c.steps) F_(UD_HSJ_F_XI) = dist * c.xis[t];
            I_(UD_HSJ_I_STEPDONE) = 0;
        } else {
            r = I_(UD_HSJ_I_DONE0) != 0 ? 0.f : INFINITY;
            I_(UD_HSJ_I_KEEP) = 0;
            I_(UD_HSJ_I_ACCEPT) = 0;
        }
        I_(UD_HSJ_I_PB) = 0;
        F_(UD_HSJ_F_RADIUS) = r;
        if (t >= 0 && t <= c.steps) c.history[(long)t * N + n] = r;
        I_(UD_HSJ_I_T) = t + 1;
        return;
    }
    if (mode == UD_HSJ_C_VNORM) {
        if (live) {
            const double ss = c.nrm[n];
            F_(UD_HSJ_F_INVN) = NORM == UD_HSJ_L2 ? (ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f) : 1.f;
        }
        return;
    }
    // ---- the modes that judge a forward: the logits row becomes one bit, and nothing else of it is used ----
    const float* row = c.logits + (long)n * c.C;
    bool valid = true;
    int cls = 0;
    if (c.C == 1) {
        const float v = row[0];
        valid = v == v;
        cls = v > 0.f ? 1 : 0;
    } else {
        float best = row[0];
        valid = best == best;
        for (int k = 1; k < c.C; ++k) {
            const float v = row[k];
            valid = valid && v == v;
            if (v > best) {                      // strict: the first maximum is the class
                best = v;
                cls = k;
            }
        }
    }
    const int bit = valid && (long long)cls != c.y[n] ? 1 : 0;      // a row with a NaN counts as not adversarial
    bool part;
    I_(UD_HSJ_I_ACCEPT) = 0;
    if (mode == UD_HSJ_C_CLEAN) {
        part = true;
        I_(UD_HSJ_I_QUERIES) = 1;
        I_(UD_HSJ_I_DONE0) = bit;
        I_(UD_HSJ_I_ACTIVE) = 1 - bit;
        I_(UD_HSJ_I_HAS) = 0;
        F_(UD_HSJ_F_BEST) = INFINITY;
        F_(UD_HSJ_F_RADIUS) = bit ? 0.f : INFINITY;
    } else if (mode == UD_HSJ_C_START || mode == UD_HSJ_C_START_NOISE) {
        part = I_(UD_HSJ_I_ACTIVE) != 0 && I_(UD_HSJ_I_HAS) == 0;
        if (part) {
            I_(UD_HSJ_I_QUERIES) += 1;
            if (bit) {
                I_(UD_HSJ_I_HAS) = 1;
                I_(UD_HSJ_I_ACCEPT) = 1;
            }
        }
        if (mode == UD_HSJ_C_START_NOISE) I_(UD_HSJ_I_DRAW) += 1;
    } else if (mode == UD_HSJ_C_BISECT) {
        part = live;
        if (part) {
            I_(UD_HSJ_I_QUERIES) += 1;
            const float mid = 0.5f * (F_(UD_HSJ_F_LO) + F_(UD_HSJ_F_HI));
            if (bit) {
                F_(UD_HSJ_F_HI) = mid;
                I_(UD_HSJ_I_MOVED) = 1;
            } else {
                F_(UD_HSJ_F_LO) = mid;
            }
        }
    } else if (mode == UD_HSJ_C_PROBE) {
        part = live;
        const int pb = I_(UD_HSJ_I_PB);
        if (part) {
            I_(UD_HSJ_I_QUERIES) += 1;
            if (pb >= 0 && pb < c.max_probes) c.phi[(long)pb * N + n] = (signed char)bit;
        }
        I_(UD_HSJ_I_PB) = pb + 1;
        I_(UD_HSJ_I_DRAW) += 1;
    } else {                                     // UD_HSJ_C_STEP
        part = live && I_(UD_HSJ_I_STEPDONE) == 0;
        if (part) {
            I_(UD_HSJ_I_QUERIES) += 1;
            if (bit) {
                I_(UD_HSJ_I_STEPDONE) = 1;
                I_(UD_HSJ_I_ACCEPT) = 1;
            } else {
                F_(UD_HSJ_F_XI) = 0.5f * F_(UD_HSJ_F_XI);
            }
        }
    }
    if (part && !valid) I_(UD_HSJ_I_FLAGS) |= 1;
    const int k = I_(UD_HSJ_I_K);
    if (k >= 0 && k < c.Q) c.decisions[(long)k * N + n] = (signed char)(part ? bit : -1);
    I_(UD_HSJ_I_K) = k + 1;
#undef I_
#undef F_
}

// ---- dist: one workgroup per sample, differences and sums in double, a fixed order -----------------------------------------------
__global__ __launch_bounds__(NT) void hsj_dist(const float* __restrict__ a, const float* __restrict__ b,
                                               const int* __restrict__ ist, int N, long per, double* __restrict__ out) {
    const int n = blockIdx.x;
    if (ist && ist[(long)UD_HSJ_I_ACTIVE * N + n] == 0) return;
    __shared__ double sh_s[NT], sh_m[NT];
    const float* as = a + (long)n * per;
    const float* bs = b ? b + (long)n * per : nullptr;
    double ss = 0.0, mx = 0.0;
    for (long e = threadIdx.x; e < per; e += NT) {
        const double d = (double)as[e] - (bs ? (double)bs[e] : 0.0);
        const double ad = fabs(d);
        ss += d * d;
        mx = ad > mx || ad != ad ? ad : mx;      // a NaN difference shows in the maximum
    }
    sh_s[threadIdx.x] = ss;
    sh_m[threadIdx.x] = mx;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh_s[threadIdx.x] += sh_s[threadIdx.x + w];
            const double o = sh_m[threadIdx.x + w], m = sh_m[threadIdx.x];
            sh_m[threadIdx.x] = o > m || o != o ? o : m;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[n] = sh_s[0];
        out[(long)N + n] = sh_m[0];
    }
}

// ---- estimate: every direction re-made in registers; the weights once per workgroup in LDS ------------------------------------
template <int NORM, bool VEC>
__global__ __launch_bounds__(NT) void hsj_estimate(float* v, const signed char* __restrict__ phi,
                                                   const long long* __restrict__ ids, const int* __restrict__ ist, int N, long per,
                                                   long quads, int B, uint32_t draw0, float inv_b, uint32_t seed_lo,
                                                   uint32_t seed_hi) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    if (ist && !live_of(ist, N, n)) return;      // uniform for the workgroup: no barrier has been reached
    __shared__ float w[UD_HSJ_MAX_PROBES];
    __shared__ int cnt[NT];
    int mine = 0;
    for (int b = threadIdx.x; b < B; b += NT) mine += phi[(long)b * N + n] != 0 ? 1 : 0;
    cnt[threadIdx.x] = mine;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) cnt[threadIdx.x] += cnt[threadIdx.x + h];
        __syncthreads();
    }
    const int ones = cnt[0];
    // all equal: +-1 (every probe adversarial: +, none: -), as the authors' code does; otherwise phi_b - mean phi
    const float mean = (float)ones * inv_b;
    for (int b = threadIdx.x; b < B; b += NT) {
        const float p = phi[(long)b * N + n] != 0 ? 1.f : 0.f;
        w[b] = ones == B ? 1.f : (ones == 0 ? -1.f : p - mean);
    }
    __syncthreads();
    const unsigned long long id = (unsigned long long)ids[n];
    const uint32_t id_lo = (uint32_t)id, id_hi = (uint32_t)(id >> 32);
    float* vs = v + (long)n * per;
    const long nthr = (long)gridDim.x * NT;
    constexpr int NOISE = NORM == UD_HSJ_L2 ? UD_SMOOTH_GAUSSIAN : UD_SMOOTH_UNIFORM;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int b = 0; b < B; ++b) {            // the sums run in ascending b whatever the unroll: acc is one chain per element
            const Words p = philox4x32_10((uint32_t)q, draw0 + (uint32_t)b, id_lo, id_hi, seed_lo, seed_hi);
            float t[4];
            hsj_noise_quad<NOISE>(p, t);
            const float wb = w[b];               // one address for the whole wave: an LDS broadcast
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float pr = wb * t[j];
                acc[j] = acc[j] + pr;
            }
        }
        if (NORM == UD_HSJ_LINF) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = sign_inc(acc[j], 1.f);
        }
        if (VEC) {
            f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
            reinterpret_cast<f32x4*>(vs)[q] = o;
        } else {
            const long e0 = 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < per) vs[e0 + j] = acc[j];
        }
    }
}

}  // namespace

extern "C" {

int ud_hsj_propose(int mode, int norm, float* dst, const float* a, const float* b, const long long* ids, const int* ist,
                   const float* fst, int N, long per, float lo, float hi, float aux, long seed, ud_stream_t stream) {
    if (!dst || !ist || !fst) return UD_EINVAL;
    if (!shape_ok(N, per) || per > (1L << 34)) return UD_EINVAL;
    if (norm != UD_HSJ_LINF && norm != UD_HSJ_L2) return UD_EINVAL;
    if (!(lo < hi)) return UD_EINVAL;
    const bool noisy = mode == UD_HSJ_P_NOISE || mode == UD_HSJ_P_PROBE;
    const bool reads_b = mode == UD_HSJ_P_BISECT || mode == UD_HSJ_P_SETTLE || mode == UD_HSJ_P_STEP;
    if (mode < UD_HSJ_P_COPY || mode > UD_HSJ_P_STEP) return UD_EINVAL;
    if ((mode != UD_HSJ_P_NOISE && !a) || (reads_b && !b) || (noisy && !ids)) return UD_EINVAL;
    if (dst == a || dst == b) return UD_EINVAL;
    const unsigned long long sd = (unsigned long long)seed;
    hipStream_t s = (hipStream_t)stream;
#define UD_HSJ_PROPOSE(M)                                                                                              \
    case M:                                                                                                            \
        return norm == UD_HSJ_L2 ? launch_propose<M, UD_HSJ_L2>(dst, a, b, ids, ist, fst, N, per, lo, hi, aux, sd, s)  \
                                 : launch_propose<M, UD_HSJ_LINF>(dst, a, b, ids, ist, fst, N, per, lo, hi, aux, sd, s);
    switch (mode) {
        UD_HSJ_PROPOSE(UD_HSJ_P_COPY)
        UD_HSJ_PROPOSE(UD_HSJ_P_COPY_SEEK)
        UD_HSJ_PROPOSE(UD_HSJ_P_NOISE)
        UD_HSJ_PROPOSE(UD_HSJ_P_BISECT)
        UD_HSJ_PROPOSE(UD_HSJ_P_SETTLE)
        UD_HSJ_PROPOSE(UD_HSJ_P_PROBE)
        UD_HSJ_PROPOSE(UD_HSJ_P_STEP)
    }
#undef UD_HSJ_PROPOSE
    return UD_EINVAL;
}

int ud_hsj_control(int mode, int norm, const float* logits, int C, const long long* y, const double* nrm, int* ist, float* fst,
                   char* phi, char* decisions, float* history, const float* xis, int N, int Q, int max_probes, int steps,
                   float delta0, float inv_d, float dfloor, ud_stream_t stream) {
    if (!ist || !fst) return UD_EINVAL;
    if (N < 1 || N > 65535) return UD_EINVAL;
    if (norm != UD_HSJ_LINF && norm != UD_HSJ_L2) return UD_EINVAL;
    if (mode < UD_HSJ_C_CLEAN || mode > UD_HSJ_C_VNORM) return UD_EINVAL;
    if (mode <= UD_HSJ_C_STEP) {
        if (!logits || !y || !decisions || C < 1 || Q < 1 || (long)Q * N > INT_MAX) return UD_EINVAL;
        if (mode == UD_HSJ_C_PROBE && (!phi || max_probes < 1 || max_probes > UD_HSJ_MAX_PROBES)) return UD_EINVAL;
    } else {
        if (!nrm) return UD_EINVAL;
        if (mode == UD_HSJ_C_DIST && (!history || !xis || steps < 1 || ((long)steps + 1) * N > INT_MAX)) return UD_EINVAL;
        if (mode == UD_HSJ_C_DIST && !(delta0 > 0.f && inv_d > 0.f && dfloor > 0.f)) return UD_EINVAL;
    }
    ControlArgs c{logits, y, nrm, ist, fst, (signed char*)phi, (signed char*)decisions, history, xis, N, C, Q, max_probes, steps,
                  delta0, inv_d, dfloor};
    const dim3 grid((unsigned)ud_cdiv(N, 64));
    if (norm == UD_HSJ_L2)
        hipLaunchKernelGGL(hsj_control<UD_HSJ_L2>, grid, dim3(64), 0, (hipStream_t)stream, mode, c);
    else
        hipLaunchKernelGGL(hsj_control<UD_HSJ_LINF>, grid, dim3(64), 0, (hipStream_t)stream, mode, c);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_hsj_dist(const float* a, const float* b, const int* ist, int N, long per, double* out, ud_stream_t stream) {
    if (!a || !out) return UD_EINVAL;
    if (!shape_ok(N, per) || per > (1L << 34)) return UD_EINVAL;
    hipLaunchKernelGGL(hsj_dist, dim3((unsigned)N), dim3(NT), 0, (hipStream_t)stream, a, b, ist, N, per, out);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_hsj_estimate(float* v, const char* phi, const long long* ids, const int* ist, int N, long per, int B, int draw0, int norm,
                    float inv_b, long seed, ud_stream_t stream) {
    if (!v || !phi || !ids) return UD_EINVAL;
    if (!shape_ok(N, per) || per > (1L << 34)) return UD_EINVAL;
    if (B < 1 || B > UD_HSJ_MAX_PROBES || draw0 < 0 || (long)draw0 + B > INT_MAX) return UD_EINVAL;
    if (norm != UD_HSJ_LINF && norm != UD_HSJ_L2) return UD_EINVAL;
    const long quads = (per + 3) / 4;
    const dim3 grid((unsigned)ew_blocks(quads), (unsigned)N);
    const unsigned long long sd = (unsigned long long)seed;
    const uint32_t slo = (uint32_t)sd, shi = (uint32_t)(sd >> 32);
    const signed char* ph = (const signed char*)phi;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = per % 4 == 0 && aligned16(v);
#define UD_HSJ_ESTIMATE(NORM, VEC)                                                                                             \
    hipLaunchKernelGGL((hsj_estimate<NORM, VEC>), grid, dim3(NT), 0, s, v, ph, ids, ist, N, per, quads, B, (uint32_t)draw0, inv_b, \
                       slo, shi)
    if (norm == UD_HSJ_L2) {
        if (vec) UD_HSJ_ESTIMATE(UD_HSJ_L2, true);
        else UD_HSJ_ESTIMATE(UD_HSJ_L2, false);
    } else {
        if (vec) UD_HSJ_ESTIMATE(UD_HSJ_LINF, true);
        else UD_HSJ_ESTIMATE(UD_HSJ_LINF, false);
    }
#undef UD_HSJ_ESTIMATE
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// Deferred-BatchNorm helpers shared by csrc/fused.hip and csrc/dwtile.hip: coefficients of a channel quad from the fp64
// sums (ud_bn_ref), act(bn(x)) on a loaded quad, the SF gate factor, the fold of fp64 partials into an accumulator.
#pragma once
#include "colgeom.h"

namespace {

constexpr int NT = UD_COL_NT;

// rows in flight per thread of the streaming loops (for_rows), both storage types: the element-wise geometry (geom_ew) hands a
// thread 4 rows, and 8 rows x 2 tensors of converted half quads do not fit 128 VGPRs without spilling
constexpr int kRowGroup = 4;

__device__ __forceinline__ void atomic_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }

struct Bn4 { f32x4 mu, is, ga, be; };

// the row bodies handed to for_rows must vanish into its unrolled groups
#define UD_LAMBDA_INLINE __attribute__((always_inline))

// a * b rounded on its own, never contracted into a neighbouring add: where the one-row loops had a branch between a product
// and the sum that follows it, the grouped loops have straight-line code, and results are to stay bit for bit what they were
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ f32x4 mul_rn(const f32x4& a, const f32x4& b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ f32x4 mul_rn(const f32x4& a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// bn_load in two parts, so that a consumer has the coefficient loads AND its first rows in flight together: bn_issue decides the
// form once (kernel-uniform) and issues the quad's loads back to back — no wait, no branch between them (the fp64 accumulators
// are caller-owned: 8-byte accesses); bn_finish turns them into coefficients, the first use of the loaded values.
struct BnRaw {
    double s[4], ss[4];          // training form: the fp64 sums
    float rm[4], rv[4];          // eval form: the running statistics
    f32x4 ga, be;
};

__device__ __forceinline__ BnRaw bn_issue(const ud_bn_ref& b, int g, int C4, int c4) {
    BnRaw r;
    if (b.sum) {
        const long i0 = ((long)(b.G == 1 ? 0 : g) * C4 + c4) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) r.s[e] = b.sum[i0 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) r.ss[e] = b.sumsq[i0 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) r.rm[e] = r.rv[e] = 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r.rm[e] = b.running_mean[c4 * 4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) r.rv[e] = b.running_var[c4 * 4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) r.s[e] = r.ss[e] = 0.0;
    }
    r.ga = reinterpret_cast<const f32x4*>(b.gamma)[c4];
    r.be = reinterpret_cast<const f32x4*>(b.beta)[c4];
    return r;
}

// (mean, biased variance) of the quad: ud_bn_moments' two forms
__device__ __forceinline__ void bn_moments4(const ud_bn_ref& b, const BnRaw& r, double (&m)[4], double (&v)[4]) {
    const bool train = b.sum != nullptr;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double mt = r.s[e] * b.inv_count;
        double vt = r.ss[e] * b.inv_count - mt * mt;
        if (vt < 0.0) vt = 0.0;
        m[e] = train ? mt : (double)r.rm[e];
        v[e] = train ? vt : (double)r.rv[e];
    }
}

__device__ __forceinline__ Bn4 bn_finish(const ud_bn_ref& b, const BnRaw& r) {
    Bn4 o;
    double m[4], v[4];
    bn_moments4(b, r, m, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.mu[e] = (float)m[e];
        o.is[e] = rsqrtf((float)(v[e] + (double)b.eps));
    }
    o.ga = r.ga;
    o.be = r.be;
    return o;
}

// The designated thread of a kernel (exactly one per channel quad per launch) moves the running statistics (nn.BatchNorm2d
// training forward) — behind its row loop, off the path in front of it: the sums again (one thread per quad, L2 hits) and the
// eight running values in one trip, then the eight stores.  The eval form (sum == NULL) takes the running statistics as the
// moments and never writes them.
__device__ __forceinline__ void bn_update_running(const ud_bn_ref& b, int g, int C4, int c4) {
    if (!(b.sum && b.running_mean)) return;
    const BnRaw r = bn_issue(b, g, C4, c4);
    float rm[4], rv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) rm[e] = b.running_mean[c4 * 4 + e];
#pragma unroll
    for (int e = 0; e < 4; ++e) rv[e] = b.running_var[c4 * 4 + e];
    double m[4], v[4];
    bn_moments4(b, r, m, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        rm[e] = mul_rn(1.f - b.momentum, rm[e]) + mul_rn(b.momentum, (float)m[e]);
        rv[e] = mul_rn(1.f - b.momentum, rv[e]) + mul_rn(b.momentum, (float)(v[e] * b.unbias));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) b.running_mean[c4 * 4 + e] = rm[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) b.running_var[c4 * 4 + e] = rv[e];
}

// Coefficients of channel quad c4 in one call, for consumers that stage tiles rather than stream rows (csrc/dwtile.hip);
// update == true for exactly one thread per channel quad per launch.
__device__ __forceinline__ Bn4 bn_load(const ud_bn_ref& b, int g, int C4, int c4, bool update) {
    const Bn4 o = bn_finish(b, bn_issue(b, g, C4, c4));
    if (update) bn_update_running(b, g, C4, c4);
    return o;
}

// ACT is a template parameter in the streaming loops: a test of the run-time `act` per element makes every element its own basic
// block, and the next row's load is then not hoisted across it (one row in flight per thread)
template <int ACT>
__device__ __forceinline__ f32x4 bn_apply(const f32x4& a, const Bn4& b) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ud_act_fast(b.ga[e] * ((a[e] - b.mu[e]) * b.is[e]) + b.be[e], ACT);
    return o;
}
__device__ __forceinline__ f32x4 bn_apply(const f32x4& a, const Bn4& b, int act) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ud_act_fast(b.ga[e] * ((a[e] - b.mu[e]) * b.is[e]) + b.be[e], act);
    return o;
}

// f(ActC<A>{}) with A = act as a compile-time constant (ud_act_fast's reading of act: 1 swish, 2 ReLU, anything else identity):
// the loop versioning of the streaming kernels
template <int A> struct ActC { static constexpr int value = A; };
template <typename F>
__device__ __forceinline__ void act_switch(int act, F&& f) {
    if (act == 1) f(ActC<1>{});
    else if (act == 2) f(ActC<2>{});
    else f(ActC<0>{});
}

// This thread's rows r, r + rs, ... < r_end, quad index idx (+ step per row), NIN tensors read per row: groups of kRowGroup
// rows are LOADED back to back, then computed in ascending row order (body(idx, r, v[NIN])); the tail runs row by row.  `fin`
// runs once, behind the first group's loads — the place to wait for the prologue's loads (bn_finish, the gate's sigmoid), so that
// coefficients and first rows share one round trip.
template <typename T, int NIN, typename Fin, typename Body>
__device__ __forceinline__ void for_rows(int r, int r_end, int rs, long idx, long step, const In4<T> (&in)[NIN], Fin&& fin,
                                         Body&& body) {
    constexpr int U = kRowGroup;
    f32x4 v[U][NIN];
    auto load = [&]() UD_LAMBDA_INLINE {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < NIN; ++t) v[u][t] = in[t][idx + u * step];
    };
    auto compute = [&]() UD_LAMBDA_INLINE {
#pragma unroll
        for (int u = 0; u < U; ++u) body(idx + u * step, r + u * rs, v[u]);
        r += U * rs;
        idx += U * step;
    };
    const bool full = r + (U - 1) * rs < r_end;
    if (full) load();
    fin();
    if (full) compute();
    while (r + (U - 1) * rs < r_end) {
        load();
        compute();
    }
    for (; r < r_end; r += rs, idx += step) {
        f32x4 t[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) t[k] = in[k][idx];
        body(idx, r, t);
    }
}

__device__ __forceinline__ float gate_factor(const float* alpha, int mode) {
    if (mode == 0 || !alpha) return 1.f;
    const float a = ud_sigmoid(alpha[0]);          // accurate: a is 4.5e-5 at the initial sf_coef = -10
    return mode == 1 ? a : 1.f - a;
}

// acc[q][o] += sum_p part[q][(o / C) * P + p][o % C]   (8 outputs x 32 chunk-lanes per block, four partials in flight
// per lane: 512 partials per output are four rounds of loads)
__global__ __launch_bounds__(NT) void partials_to_acc(int nq, int G, int C, int P, const double* __restrict__ part,
                                                      double* __restrict__ a1, double* __restrict__ a2) {
    __shared__ double sm[2][NT];
    const int cl = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int idx = blockIdx.x * 8 + cl;
    const bool ok = idx < G * C;
    const long plane = (long)G * P * C;
    double a = 0.0, b = 0.0;
    if (ok) {
        const int g = idx / C, c = idx % C;
        const long base = (long)g * P * C + c, step = 32L * C;
        int p = pl;
        for (; p + 96 < P; p += 128) {
            const long o = base + (long)p * C;
            a += (part[o] + part[o + step]) + (part[o + 2 * step] + part[o + 3 * step]);
            if (nq == 2) b += (part[plane + o] + part[plane + o + step]) + (part[plane + o + 2 * step] + part[plane + o + 3 * step]);
        }
        for (; p < P; p += 32) {
            const long o = base + (long)p * C;
            a += part[o];
            if (nq == 2) b += part[plane + o];
        }
    }
    sm[0][threadIdx.x] = a;
    sm[1][threadIdx.x] = b;
    __syncthreads();
    if (ok && pl == 0) {
        for (int k = 1; k < 32; ++k) {
            a += sm[0][k * 8 + cl];
            b += sm[1][k * 8 + cl];
        }
        a1[idx] += a;
        if (nq == 2) a2[idx] += b;
    }
}

}  // namespace

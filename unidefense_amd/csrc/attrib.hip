// The kernel work of an attribution (unidefense_amd/attrib.py: AttributionRunner, DeletionRunner): the path integral of
// integrated gradients around the frozen forward + d/dx, and the deletion / insertion curve that scores a heat map.
//   ud_attr_point       : xp[n] = b[n] + alpha[k_n % steps] (x[n] - b[n]), the sample's point on the straight path
//   ud_attr_accumulate  : acc[n] += w[k_n % steps] g[n] in double
//   ud_attr_control     : one thread per sample: path[k][n] = f[n], the counter
//   ud_attr_finish      : attr, the per-pixel heat map, and total[n] = the sum of the attribution in double (completeness)
//   ud_attr_rank_select : per (sample, j) the kcount[j]-th largest pixel key of the heat map: a radix select on integer counts
//   ud_attr_mask        : xq = the image with its top pixels replaced by the baseline (deletion) or the reverse (insertion)
//
// The element-wise kernels own one quad of four consecutive elements (pixels) per thread: a float4 per thread where the length is
// a multiple of 4 and every base is 16-byte aligned, scalar accesses otherwise, the same bits either way.  Every expression is
// rounded once per operation in the order written (no contraction).  Nothing is accumulated with a floating-point atomic: total
// is a fixed tree per workgroup over a grid that depends on S alone, folded in index order by a second kernel, so a replay, another
// batch size and another row give the same bits.
#include <climits>

#include "attack_common.h"

namespace {

constexpr int NW = NT / 64;

// the sample's counter in [0, iters), or -1
__device__ __forceinline__ int counter_of(const int* __restrict__ k, int n, int iters) {
    const int v = k[n];
    return v >= 0 && v < iters ? v : -1;
}

// ---- point --------------------------------------------------------------------------------------------------------------------
// a == 1 is x and a == 0 is b by rule, not by arithmetic: b + 1 (x - b) is not x in fp32
__device__ __forceinline__ float point(float x, float b, float a) {
#pragma clang fp contract(off)
    if (a == 1.f) return x;
    if (a == 0.f) return b;
    const float d = x - b;
    const float m = a * d;
    return b + m;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void attr_point(const float* __restrict__ x, const float* __restrict__ b, float* __restrict__ xp,
                                                 const int* __restrict__ k, const float* __restrict__ alpha, int steps, int iters,
                                                 long per, long quads) {
    const int n = blockIdx.y;
    const int kn = counter_of(k, n, iters);
    if (kn < 0) return;
    const float a = alpha[kn % steps];
    const float* xs = x + (long)n * per;
    const float* bs = b + (long)n * per;
    float* os = xp + (long)n * per;
    const long nthr = (long)gridDim.x * NT;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        if (VEC) {
            const f32x4 u = reinterpret_cast<const f32x4*>(xs)[q], v = reinterpret_cast<const f32x4*>(bs)[q];
            f32x4 o;
            o.x = point(u.x, v.x, a);
            o.y = point(u.y, v.y, a);
            o.z = point(u.z, v.z, a);
            o.w = point(u.w, v.w, a);
            reinterpret_cast<f32x4*>(os)[q] = o;
        } else {
            const long e0 = 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < per) os[e0 + j] = point(xs[e0 + j], bs[e0 + j], a);
        }
    }
}

// ---- accumulate ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double accumulated(double acc, double w, float g) {
#pragma clang fp contract(off)
    const double t = w * (double)g;
    return acc + t;
}

typedef double f64x2 __attribute__((ext_vector_type(2)));

template <bool VEC>
__global__ __launch_bounds__(NT) void attr_accumulate(const float* __restrict__ g, double* __restrict__ acc,
                                                      const int* __restrict__ k, const double* __restrict__ w, int steps, int iters,
                                                      long per, long quads) {
    const int n = blockIdx.y;
    const int kn = counter_of(k, n, iters);
    if (kn < 0) return;
    const double wk = w[kn % steps];
    const float* gs = g + (long)n * per;
    double* as = acc + (long)n * per;
    const long nthr = (long)gridDim.x * NT;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        if (VEC) {
            const f32x4 v = reinterpret_cast<const f32x4*>(gs)[q];
            f64x2 lo = reinterpret_cast<const f64x2*>(as)[2 * q], hi = reinterpret_cast<const f64x2*>(as)[2 * q + 1];
            lo.x = accumulated(lo.x, wk, v.x);
            lo.y = accumulated(lo.y, wk, v.y);
            hi.x = accumulated(hi.x, wk, v.z);
            hi.y = accumulated(hi.y, wk, v.w);
            reinterpret_cast<f64x2*>(as)[2 * q] = lo;
            reinterpret_cast<f64x2*>(as)[2 * q + 1] = hi;
        } else {
            const long e0 = 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < per) as[e0 + j] = accumulated(as[e0 + j], wk, gs[e0 + j]);
        }
    }
}

// ---- control: one thread per sample; only its own column of path and its own counter are touched -----------------------------
__global__ __launch_bounds__(64) void attr_control(const float* __restrict__ f, int* __restrict__ ist, float* __restrict__ path,
                                                   int N, int iters) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int k = ist[(long)UD_ATTR_I_K * N + n];
    if (k < 0 || k >= iters) return;
    path[(long)k * N + n] = f[n];
    ist[(long)UD_ATTR_I_K * N + n] = k + 1;
}

// ---- finish -------------------------------------------------------------------------------------------------------------------
// workgroups of a sample: a function of the pixel count alone, so a sample's partials do not depend on N or on its row
static inline int finish_parts(long hw) { return ew_blocks((hw + 3) / 4); }

template <int MODE>
__device__ __forceinline__ double attr_value(float x, float b, double acc, double scale) {
#pragma clang fp contract(off)
    if (MODE == UD_ATTR_GRAD) return acc * scale;
    const double d = (double)x - (double)b;
    const double t = d * acc;
    return t * scale;
}

// channels 0, 1, 2 of one pixel: the three fp32 attributions, the heat value, and the pixel's three terms added to `sum`
template <int MODE, int REDUCE>
__device__ __forceinline__ void finish_pixel(const float* x3, const float* b3, const double* a3, double scale, float* attr3,
                                             float& heat, double& sum) {
#pragma clang fp contract(off)
    double h = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = attr_value<MODE>(x3[c], b3[c], a3[c], scale);
        attr3[c] = (float)v;
        const double t = REDUCE == UD_ATTR_ABS ? fabs(v) : v;
        h = c == 0 ? t : h + t;
        sum = sum + v;
    }
    heat = (float)h;
}

template <int MODE, int REDUCE, bool VEC>
__global__ __launch_bounds__(NT) void attr_finish(const float* __restrict__ x, const float* __restrict__ b,
                                                  const double* __restrict__ acc, float* __restrict__ attr,
                                                  float* __restrict__ heat, double* __restrict__ ws, double scale, long hw,
                                                  long quads) {
    __shared__ double part[NW];
    const long n = blockIdx.y;
    const long per = 3 * hw;
    const float* xs = x + n * per;
    const float* bs = b + n * per;
    const double* as = acc + n * per;
    float* os = attr + n * per;
    float* hs = heat + n * hw;
    double sum = 0.0;
    const long nthr = (long)gridDim.x * NT;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        float xv[4][3], bv[4][3], ov[4][3], hv[4];
        double av[4][3];
        const long p0 = 4 * q;
        if (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 u = reinterpret_cast<const f32x4*>(xs + c * hw)[q], v = reinterpret_cast<const f32x4*>(bs + c * hw)[q];
                const f64x2 lo = reinterpret_cast<const f64x2*>(as + c * hw)[2 * q], hi = reinterpret_cast<const f64x2*>(as + c * hw)[2 * q + 1];
                xv[0][c] = u.x, xv[1][c] = u.y, xv[2][c] = u.z, xv[3][c] = u.w;
                bv[0][c] = v.x, bv[1][c] = v.y, bv[2][c] = v.z, bv[3][c] = v.w;
                av[0][c] = lo.x, av[1][c] = lo.y, av[2][c] = hi.x, av[3][c] = hi.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const bool in = p0 + j < hw;
                    xv[j][c] = in ? xs[c * hw + p0 + j] : 0.f;
                    bv[j][c] = in ? bs[c * hw + p0 + j] : 0.f;
                    av[j][c] = in ? as[c * hw + p0 + j] : 0.0;
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (VEC || p0 + j < hw) finish_pixel<MODE, REDUCE>(xv[j], bv[j], av[j], scale, ov[j], hv[j], sum);
        if (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 o;
                o.x = ov[0][c], o.y = ov[1][c], o.z = ov[2][c], o.w = ov[3][c];
                reinterpret_cast<f32x4*>(os + c * hw)[q] = o;
            }
            f32x4 h;
            h.x = hv[0], h.y = hv[1], h.z = hv[2], h.w = hv[3];
            reinterpret_cast<f32x4*>(hs)[q] = h;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j < hw) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) os[c * hw + p0 + j] = ov[j][c];
                    hs[p0 + j] = hv[j];
                }
        }
    }
    // the workgroup's partial: a butterfly inside each wave, then the waves in order
    sum = ud_wave_sum_d(sum);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) t = t + part[w];
        ws[n * gridDim.x + blockIdx.x] = t;
    }
}

// one thread per sample: the partials in index order
__global__ __launch_bounds__(64) void attr_total(const double* __restrict__ ws, double* __restrict__ total, int N, int parts) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const double* p = ws + (long)n * parts;
    double t = p[0];
    for (int i = 1; i < parts; ++i) t = t + p[i];
    total[n] = t;
}

template <int MODE, int REDUCE>
int launch_finish(const float* x, const float* b, const double* acc, float* attr, float* heat, double* total, double* ws,
                  double scale, int N, long hw, hipStream_t s) {
    const long quads = (hw + 3) / 4;
    const int parts = finish_parts(hw);
    const dim3 grid((unsigned)parts, (unsigned)N);
    if (hw % 4 == 0 && aligned16(x) && aligned16(b) && aligned16(acc) && aligned16(attr) && aligned16(heat))
        hipLaunchKernelGGL((attr_finish<MODE, REDUCE, true>), grid, dim3(NT), 0, s, x, b, acc, attr, heat, ws, scale, hw, quads);
    else
        hipLaunchKernelGGL((attr_finish<MODE, REDUCE, false>), grid, dim3(NT), 0, s, x, b, acc, attr, heat, ws, scale, hw, quads);
    UD_LAUNCH_CHECK();
    hipLaunchKernelGGL(attr_total, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, s, ws, total, N, parts);
    UD_LAUNCH_CHECK();
    return 0;
}

// ---- rank: the key of a pixel ---------------------------------------------------------------------------------------------------
// high word: the order-preserving image of the heat value (a NaN: 0, below every number; -0 as +0); low word ~p: among equal
// heats the lower pixel index is the larger key, and no two pixels share a key
__device__ __forceinline__ unsigned long long rank_key(float h, uint32_t p) {
    uint32_t u = __float_as_uint(h);
    if (h != h) {
        u = 0u;
    } else {
        if (u == 0x80000000u) u = 0u;
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | (unsigned long long)(~p);
}

// Workgroup (j, n): the kcount[j]-th largest key of sample n, 8 bits per pass from the top: per pass a histogram of the keys that
// share the prefix found so far (integer LDS atomics: counts, order-free), then the bin in which the need-th largest lies.
__global__ __launch_bounds__(NT) void attr_rank_select(const float* __restrict__ heat, const int* __restrict__ kcount,
                                                       unsigned long long* __restrict__ thr, int N, long hw) {
    __shared__ unsigned hist[NT];
    __shared__ unsigned wtot[NW];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned s_need;
    const int j = blockIdx.x, n = blockIdx.y;
    long kc = kcount[j];
    kc = kc > hw ? hw : kc;
    if (kc <= 0) {                                             // uniform over the workgroup
        if (threadIdx.x == 0) thr[(long)j * N + n] = ~0ULL;
        return;
    }
    const float* hs = heat + (long)n * hw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long prefix = 0;
    unsigned need = (unsigned)kc;
    for (int L = 0; L < 8; ++L) {
        const int shift = 56 - 8 * L;
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (long p = threadIdx.x; p < hw; p += NT) {
            const unsigned long long key = rank_key(hs[p], (uint32_t)p);
            if (L == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        // thread t holds bin t; v = the entries of the wave's bins from this thread's on
        const unsigned h = hist[threadIdx.x];
        unsigned v = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_down(v, o, 64);
            if (lane + o < 64) v += u;
        }
        if (lane == 0) wtot[wave] = v;
        __syncthreads();
        unsigned above = v - h;                                // entries in the bins above this thread's
        for (int w = wave + 1; w < NW; ++w) above += wtot[w];
        if (above < need && need <= above + h) {               // exactly one thread
            s_prefix = (prefix << 8) | (unsigned long long)threadIdx.x;
            s_need = need - above;
        }
        __syncthreads();
        prefix = s_prefix, need = s_need;
    }
    if (threadIdx.x == 0) thr[(long)j * N + n] = prefix;
}

// ---- mask -----------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(NT) void attr_mask(const float* __restrict__ x, const float* __restrict__ b,
                                                const float* __restrict__ heat, const unsigned long long* __restrict__ thr,
                                                const int* __restrict__ ist, float* __restrict__ xq, int insert, int N, long hw,
                                                long quads, int K) {
    const long n = blockIdx.y;
    const int j = ist[(long)UD_ATTR_I_K * N + n];
    if (j < 0 || j >= K) return;
    const unsigned long long t = thr[(long)j * N + n];
    const long per = 3 * hw;
    const float* xs = x + n * per;
    const float* bs = b + n * per;
    const float* hs = heat + n * hw;
    float* os = xq + n * per;
    const long nthr = (long)gridDim.x * NT;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        const long p0 = 4 * q;
        if (VEC) {
            const f32x4 h = reinterpret_cast<const f32x4*>(hs)[q];
            const bool t0 = (rank_key(h.x, (uint32_t)p0) >= t) != (insert != 0), t1 = (rank_key(h.y, (uint32_t)(p0 + 1)) >= t) != (insert != 0);
            const bool t2 = (rank_key(h.z, (uint32_t)(p0 + 2)) >= t) != (insert != 0), t3 = (rank_key(h.w, (uint32_t)(p0 + 3)) >= t) != (insert != 0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 u = reinterpret_cast<const f32x4*>(xs + c * hw)[q], v = reinterpret_cast<const f32x4*>(bs + c * hw)[q];
                f32x4 o;
                o.x = t0 ? v.x : u.x;
                o.y = t1 ? v.y : u.y;
                o.z = t2 ? v.z : u.z;
                o.w = t3 ? v.w : u.w;
                reinterpret_cast<f32x4*>(os + c * hw)[q] = o;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (p0 + i < hw) {
                    const bool base = (rank_key(hs[p0 + i], (uint32_t)(p0 + i)) >= t) != (insert != 0);
#pragma unroll
                    for (int c = 0; c < 3; ++c) os[c * hw + p0 + i] = base ? bs[c * hw + p0 + i] : xs[c * hw + p0 + i];
                }
        }
    }
}

// S in [1, 32768] and N in [1, 65535]: 3 S^2 N stays inside a long, a pixel index inside 32 bits
static inline bool image_ok(int N, int S) { return N >= 1 && N <= 65535 && S >= 1 && S <= 32768; }

}  // namespace

extern "C" {

int ud_attr_point(const float* x, const float* b, float* xp, const int* k, const float* alpha, int steps, int iters, int N,
                  long per, ud_stream_t stream) {
    if (!x || !b || !xp || !k || !alpha) return UD_EINVAL;
    if (!shape_ok(N, per) || steps < 1 || iters < 1 || (long)iters * N > INT_MAX) return UD_EINVAL;
    const long quads = (per + 3) / 4;
    const dim3 grid((unsigned)ew_blocks(quads), (unsigned)N);
    if (per % 4 == 0 && aligned16(x) && aligned16(b) && aligned16(xp))
        hipLaunchKernelGGL(attr_point<true>, grid, dim3(NT), 0, (hipStream_t)stream, x, b, xp, k, alpha, steps, iters, per, quads);
    else
        hipLaunchKernelGGL(attr_point<false>, grid, dim3(NT), 0, (hipStream_t)stream, x, b, xp, k, alpha, steps, iters, per, quads);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_attr_accumulate(const float* g, double* acc, const int* k, const double* w, int steps, int iters, int N, long per,
                       ud_stream_t stream) {
    if (!g || !acc || !k || !w) return UD_EINVAL;
    if (!shape_ok(N, per) || steps < 1 || iters < 1 || (long)iters * N > INT_MAX) return UD_EINVAL;
    const long quads = (per + 3) / 4;
    const dim3 grid((unsigned)ew_blocks(quads), (unsigned)N);
    if (per % 4 == 0 && aligned16(g) && aligned16(acc))
        hipLaunchKernelGGL(attr_accumulate<true>, grid, dim3(NT), 0, (hipStream_t)stream, g, acc, k, w, steps, iters, per, quads);
    else
        hipLaunchKernelGGL(attr_accumulate<false>, grid, dim3(NT), 0, (hipStream_t)stream, g, acc, k, w, steps, iters, per, quads);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_attr_control(const float* f, int* ist, float* path, int N, int iters, ud_stream_t stream) {
    if (!f || !ist || !path) return UD_EINVAL;
    if (N < 1 || N > 65535 || iters < 1 || (long)iters * N > INT_MAX) return UD_EINVAL;
    hipLaunchKernelGGL(attr_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ist, path, N, iters);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_attr_finish_ws_bytes(int N, long per) {
    if (!shape_ok(N, per) || per % 3 != 0) return UD_EINVAL;
    const long bytes = (long)N * finish_parts(per / 3) * (long)sizeof(double);
    return bytes > INT_MAX ? UD_EINVAL : (int)bytes;
}

int ud_attr_finish(const float* x, const float* b, const double* acc, float* attr, float* heat, double* total, double* ws,
                   long ws_bytes, int mode, int reduce, double scale, int N, int S, ud_stream_t stream) {
    if (!x || !b || !acc || !attr || !heat || !total || !ws) return UD_EINVAL;
    if (!image_ok(N, S)) return UD_EINVAL;
    if (mode != UD_ATTR_IG && mode != UD_ATTR_GRAD) return UD_EINVAL;
    if (reduce != UD_ATTR_SUM && reduce != UD_ATTR_ABS) return UD_EINVAL;
    if (!(scale == scale)) return UD_EINVAL;
    const long hw = (long)S * S;
    const int need = ud_attr_finish_ws_bytes(N, 3 * hw);
    if (need < 0 || ws_bytes < need) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (mode == UD_ATTR_IG)
        return reduce == UD_ATTR_SUM ? launch_finish<UD_ATTR_IG, UD_ATTR_SUM>(x, b, acc, attr, heat, total, ws, scale, N, hw, s)
                                     : launch_finish<UD_ATTR_IG, UD_ATTR_ABS>(x, b, acc, attr, heat, total, ws, scale, N, hw, s);
    return reduce == UD_ATTR_SUM ? launch_finish<UD_ATTR_GRAD, UD_ATTR_SUM>(x, b, acc, attr, heat, total, ws, scale, N, hw, s)
                                 : launch_finish<UD_ATTR_GRAD, UD_ATTR_ABS>(x, b, acc, attr, heat, total, ws, scale, N, hw, s);
}

int ud_attr_rank_select(const float* heat, const int* kcount, unsigned long long* thr, int N, long HW, int K,
                        ud_stream_t stream) {
    if (!heat || !kcount || !thr) return UD_EINVAL;
    if (N < 1 || N > 65535 || HW < 1 || HW > (1L << 30) || K < 1 || (long)K * N > INT_MAX) return UD_EINVAL;
    hipLaunchKernelGGL(attr_rank_select, dim3((unsigned)K, (unsigned)N), dim3(NT), 0, (hipStream_t)stream, heat, kcount, thr, N, HW);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_attr_mask(const float* x, const float* b, const float* heat, const unsigned long long* thr, const int* ist, float* xq,
                 int mode, int N, int S, int K, ud_stream_t stream) {
    if (!x || !b || !heat || !thr || !ist || !xq) return UD_EINVAL;
    if (!image_ok(N, S) || K < 1 || (long)K * N > INT_MAX) return UD_EINVAL;
    if (mode != UD_ATTR_DELETE && mode != UD_ATTR_INSERT) return UD_EINVAL;
    const long hw = (long)S * S, quads = (hw + 3) / 4;
    const dim3 grid((unsigned)ew_blocks(quads), (unsigned)N);
    if (hw % 4 == 0 && aligned16(x) && aligned16(b) && aligned16(heat) && aligned16(xq))
        hipLaunchKernelGGL(attr_mask<true>, grid, dim3(NT), 0, (hipStream_t)stream, x, b, heat, thr, ist, xq,
                           mode == UD_ATTR_INSERT, N, hw, quads, K);
    else
        hipLaunchKernelGGL(attr_mask<false>, grid, dim3(NT), 0, (hipStream_t)stream, x, b, heat, thr, ist, xq,
                           mode == UD_ATTR_INSERT, N, hw, quads, K);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

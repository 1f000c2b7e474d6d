// The flow-field (stAdv) attack's kernels (unidefense_amd/flow.py: flow_warp, FlowRunner): a per-pixel displacement field w
// [N][2][S][S] in pixels resamples the image bilinearly, and the attack ascends the loss in w.
//   ud_flow_warp    : out(p) = the bilinear sample of x at p + w(p), coordinates clamped to the image
//   ud_flow_grad    : gw(p) = sign d out(p) / d w(p) . g(p) - tau t(p), t the gradient of the smoothness term: a gather over the
//                     four taps of p's own cell and over w's four neighbours
//   ud_flow_control : one thread per sample: the history and the keep-best decision
//   ud_flow_update  : w_best <- w where kept, the signed step on w inside the L-infinity bound, and the new x_adv: one pass
// The output pixel p depends on w(p) alone, so the adjoint with respect to w needs no scatter: every kernel is a pixel-local
// gather with ordinary vector loads and stores, no atomics, no workspace, and a replay gives the same bits.  The rules, the order
// of the fp32 operations and the rounding counts are the header's (include/unidefense_hip.h); nothing here is contracted.
//
// A workgroup owns a TX x TY tile of one sample: 64 consecutive columns per wave, so every access to g, w, gw and out is
// coalesced; a thread handles the three channels of its pixel, so the cell, the fractions and the twelve taps are computed
// once.  The flow is a few pixels, so a wave's taps fall on the rows next to its own and hit L1 / L2: they are plain global
// gathers.  One pixel per thread was measured against 2, 4 and 8 rows per thread (tiles of 8, 16 and 32 rows) at bs 32: the update
// with every sample kept takes 27.7 / 31.1 / 31.8 / 31.9 us at 256^2 and 65.0 / 69.6 / 74.3 / 81.9 us at 380^2, the gradient
// 28.5 / - / 30.0 / 35.1 us at 256^2 (profiles/r25/flow.txt).
#include <climits>

#include "attack_common.h"

namespace {

constexpr int TX = 64;                    // the tile's width: one wave per row
constexpr int TY = NT / TX;               // the tile's height: one pixel per thread

// the cell and the fraction of the source coordinate q (the header's rule): every index in [0, S - 2] for any q
struct Axis {
    int i0;
    float f;
    bool inside;                          // 0 < q < S - 1, strictly: the coordinate moves with w
};

__device__ __forceinline__ Axis axis_of(float q, int S) {
#pragma clang fp contract(off)
    const float hi = (float)(S - 1);
    const bool nan = !(q == q);
    float p = nan ? 0.f : q;              // before any conversion to an integer
    p = p < 0.f ? 0.f : (p > hi ? hi : p);
    float c = floorf(p);
    c = c > hi - 1.f ? hi - 1.f : c;
    int i = (int)c;
    i = i < 0 ? 0 : (i > S - 2 ? S - 2 : i);
    Axis a;
    a.i0 = i;
    a.f = nan ? q : p - c;
    a.inside = q > 0.f && q < hi;
    return a;
}

struct Cell {
    Axis X, Y;
    long o00;                             // y0 S + x0
};

__device__ __forceinline__ Cell cell_of(int r, int c, float w0, float w1, int S) {
#pragma clang fp contract(off)
    Cell k;
    k.X = axis_of((float)c + w0, S);
    k.Y = axis_of((float)r + w1, S);
    k.o00 = (long)k.Y.i0 * S + k.X.i0;
    return k;
}

__device__ __forceinline__ float bilinear(float u00, float u01, float u10, float u11, float fx, float fy) {
#pragma clang fp contract(off)
    const float ax = 1.f - fx, ay = 1.f - fy;
    const float top = ax * u00 + fx * u01;
    const float bot = ax * u10 + fx * u11;
    return ay * top + fy * bot;
}

// the three channels of the pixel (r, c) of one sample (xs, os: the sample's planes) for the displacement (w0, w1)
__device__ __forceinline__ void warp_pixel(const float* __restrict__ xs, float* __restrict__ os, long plane, int S, int r, int c,
                                           float w0, float w1) {
    const Cell k = cell_of(r, c, w0, w1, S);
    const long p = (long)r * S + c;
    float u[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* t = xs + ch * plane + k.o00;
        u[ch][0] = t[0], u[ch][1] = t[1], u[ch][2] = t[S], u[ch][3] = t[S + 1];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) os[ch * plane + p] = bilinear(u[ch][0], u[ch][1], u[ch][2], u[ch][3], k.X.f, k.Y.f);
}

__global__ __launch_bounds__(NT) void flow_warp(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ out,
                                                int S) {
    const int n = blockIdx.z, c = blockIdx.x * TX + threadIdx.x % TX;
    const long plane = (long)S * S;
    const float* xs = x + (long)n * 3 * plane;
    const float* ws = w + (long)n * 2 * plane;
    float* os = out + (long)n * 3 * plane;
    const int r = blockIdx.y * TY + threadIdx.x / TX;
    if (c >= S || r >= S) return;
    const long p = (long)r * S + c;
    warp_pixel(xs, os, plane, S, r, c, ws[p], ws[plane + p]);
}

// one neighbour's term of t: d / sqrt(d0 d0 + d1 d1 + tv_eps), d = w(p) - w(q)
__device__ __forceinline__ void tv_term(float w0, float w1, float q0, float q1, float tv_eps, float& t0, float& t1) {
#pragma clang fp contract(off)
    const float d0 = w0 - q0, d1 = w1 - q1;
    const float s = sqrtf(d0 * d0 + d1 * d1 + tv_eps);
    t0 = t0 + d0 / s;
    t1 = t1 + d1 / s;
}

__global__ __launch_bounds__(NT) void flow_grad(const float* __restrict__ g, const float* __restrict__ x,
                                                const float* __restrict__ w, float* __restrict__ gw, int S, float sign, float tau,
                                                float tv_eps) {
#pragma clang fp contract(off)
    const int n = blockIdx.z, c = blockIdx.x * TX + threadIdx.x % TX;
    const long plane = (long)S * S;
    const float* gs = g + (long)n * 3 * plane;
    const float* xs = x + (long)n * 3 * plane;
    const float* ws = w + (long)n * 2 * plane;
    float* os = gw + (long)n * 2 * plane;
    const int r = blockIdx.y * TY + threadIdx.x / TX;
    if (c >= S || r >= S) return;
    const long p = (long)r * S + c;
    const float w0 = ws[p], w1 = ws[plane + p];
    const Cell k = cell_of(r, c, w0, w1, S);
    const float fx = k.X.f, fy = k.Y.f, ax = 1.f - fx, ay = 1.f - fy;
    float gx = 0.f, gy = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* t = xs + ch * plane + k.o00;
        const float u00 = t[0], u01 = t[1], u10 = t[S], u11 = t[S + 1];
        const float gc = gs[ch * plane + p];
        const float dx = ay * (u01 - u00) + fy * (u11 - u10);
        const float dy = ax * (u10 - u00) + fx * (u11 - u01);
        gx = ch == 0 ? gc * dx : gx + gc * dx;
        gy = ch == 0 ? gc * dy : gy + gc * dy;
    }
    gx = k.X.inside ? gx : 0.f;
    gy = k.Y.inside ? gy : 0.f;
    float t0 = 0.f, t1 = 0.f;
    if (c > 0) tv_term(w0, w1, ws[p - 1], ws[plane + p - 1], tv_eps, t0, t1);
    if (c < S - 1) tv_term(w0, w1, ws[p + 1], ws[plane + p + 1], tv_eps, t0, t1);
    if (r > 0) tv_term(w0, w1, ws[p - S], ws[plane + p - S], tv_eps, t0, t1);
    if (r < S - 1) tv_term(w0, w1, ws[p + S], ws[plane + p + S], tv_eps, t0, t1);
    os[p] = sign * gx - tau * t0;
    os[plane + p] = sign * gy - tau * t1;
}

// ---- control: one thread per sample ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void flow_control(const float* __restrict__ f, int* __restrict__ ist, float* __restrict__ fst,
                                                   float* __restrict__ history, int steps, int N, int maximise) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int k = ist[(long)UD_FLOW_I_K * N + n];
    if (k < 0 || k > steps) {
        ist[(long)UD_FLOW_I_KEEP * N + n] = 0;
        return;
    }
    const float fk = f[n], best = fst[(long)UD_FLOW_F_BEST * N + n];
    history[(long)k * N + n] = fk;
    const bool better = maximise ? fk > best : fk < best;             // strict: a tie keeps the earliest k
    const bool keep = k == 0 || better || (best != best && fk == fk);
    if (keep) fst[(long)UD_FLOW_F_BEST * N + n] = fk;
    ist[(long)UD_FLOW_I_KEEP * N + n] = keep ? 1 : 0;
    ist[(long)UD_FLOW_I_K * N + n] = k + 1;
}

// ---- update: keep-best, the signed step inside the bound, the new image ---------------------------------------------------------
__device__ __forceinline__ float flow_step_elem(float w, float gw, float step, float bound) {
#pragma clang fp contract(off)
    return clampf(w + sign_inc(gw, step), -bound, bound);
}

template <bool CLOSING>
__global__ __launch_bounds__(NT) void flow_update(float* __restrict__ w, float* __restrict__ w_best, const float* __restrict__ gw,
                                                  const int* __restrict__ keep, const float* __restrict__ x,
                                                  float* __restrict__ x_adv, int S, float step, float bound) {
    const int n = blockIdx.z, c = blockIdx.x * TX + threadIdx.x % TX;
    const long plane = (long)S * S;
    const float* xs = x + (long)n * 3 * plane;
    float* os = x_adv + (long)n * 3 * plane;
    float* ws = w + (long)n * 2 * plane;
    float* bs = w_best + (long)n * 2 * plane;
    const int r = blockIdx.y * TY + threadIdx.x / TX;
    const bool kept = keep[n] != 0;                               // uniform over the workgroup
    if (c >= S || r >= S) return;
    const long p = (long)r * S + c;
    float w0, w1;
    if (CLOSING) {                                                // the winner's image; w is read only where it is the winner
        w0 = kept ? ws[p] : bs[p];
        w1 = kept ? ws[plane + p] : bs[plane + p];
        if (kept) bs[p] = w0, bs[plane + p] = w1;
    } else {
        w0 = ws[p], w1 = ws[plane + p];
        if (kept) bs[p] = w0, bs[plane + p] = w1;
        const float* gs = gw + (long)n * 2 * plane;
        w0 = flow_step_elem(w0, gs[p], step, bound);
        w1 = flow_step_elem(w1, gs[plane + p], step, bound);
        ws[p] = w0, ws[plane + p] = w1;
    }
    warp_pixel(xs, os, plane, S, r, c, w0, w1);
}

inline bool image_ok(int N, int S) { return N >= 1 && N <= 65535 && S >= 2 && S <= 32768; }
inline dim3 image_grid(int N, int S) { return dim3((unsigned)ud_cdiv(S, TX), (unsigned)ud_cdiv(S, TY), (unsigned)N); }
inline bool finite(float v) { return v - v == 0.f; }

}  // namespace

extern "C" {

int ud_flow_warp(const float* x, const float* w, float* out, int N, int S, ud_stream_t stream) {
    if (!x || !w || !out || x == out || !image_ok(N, S)) return UD_EINVAL;
    hipLaunchKernelGGL(flow_warp, image_grid(N, S), dim3(NT), 0, (hipStream_t)stream, x, w, out, S);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_flow_grad(const float* g, const float* x, const float* w, float* gw, int N, int S, int sign, float tau, float tv_eps,
                 ud_stream_t stream) {
    if (!g || !x || !w || !gw || gw == w || !image_ok(N, S)) return UD_EINVAL;
    if ((sign != 1 && sign != -1) || !(tau >= 0.f) || !finite(tau) || !(tv_eps > 0.f) || !finite(tv_eps)) return UD_EINVAL;
    hipLaunchKernelGGL(flow_grad, image_grid(N, S), dim3(NT), 0, (hipStream_t)stream, g, x, w, gw, S, (float)sign, tau, tv_eps);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_flow_control(const float* f, int* ist, float* fst, float* history, int steps, int N, int maximise, ud_stream_t stream) {
    if (!f || !ist || !fst || !history || steps < 1 || N < 1 || ((long)steps + 1) * N > INT_MAX) return UD_EINVAL;
    hipLaunchKernelGGL(flow_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ist, fst, history, steps,
                       N, maximise);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_flow_update(float* w, float* w_best, const float* gw, const int* keep, const float* x, float* x_adv, int N, int S,
                   float step, float bound, int closing, ud_stream_t stream) {
    if (!w || !w_best || !keep || !x || !x_adv || (!closing && !gw) || x_adv == x || w_best == w || gw == w || gw == w_best ||
        !image_ok(N, S))
        return UD_EINVAL;
    if (step != step || !(bound >= 0.f)) return UD_EINVAL;
    if (closing)
        hipLaunchKernelGGL(flow_update<true>, image_grid(N, S), dim3(NT), 0, (hipStream_t)stream, w, w_best, gw, keep, x, x_adv, S,
                           step, bound);
    else
        hipLaunchKernelGGL(flow_update<false>, image_grid(N, S), dim3(NT), 0, (hipStream_t)stream, w, w_best, gw, keep, x, x_adv,
                           S, step, bound);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

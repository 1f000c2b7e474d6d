// What csrc/attack.hip, csrc/apgd.hip and csrc/square.hip share: the launch geometry and argument tests of their
// element-wise kernels and the per-element pieces of the two projections and the two directions.  One definition each, so
// that the PGD, Auto-PGD and Square runners step and project with the same bits.
#pragma once
#include "ud_common.h"

constexpr int NT = 256;

// workgroups of NT threads for `work` items of a grid-stride kernel
static inline int ew_blocks(long work) {
    long b = (work + NT - 1) / NT;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// N samples of `per` elements: N fits gridDim.y and N per stays far inside a long
static inline bool shape_ok(int N, long per) { return N >= 1 && N <= 65535 && per >= 1 && per <= (1L << 40) / N; }

// clamp that keeps a NaN (both comparisons are false for it)
__device__ __forceinline__ float clampf(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// projection onto the box |v - x0| <= eps, then onto clip, in the order torch evaluates
//   clamp(clamp(v, x0 - eps, x0 + eps), lo, hi)
// with one fp32 rounding per operation
__device__ __forceinline__ float proj_linf(float v, float x0, float eps, float lo, float hi) {
#pragma clang fp contract(off)
    const float bl = x0 - eps, bh = x0 + eps;
    return clampf(clampf(v, bl, bh), lo, hi);
}

// s * sign(g): +-s or 0 exactly; a NaN g gives a NaN increment
__device__ __forceinline__ float sign_inc(float g, float s) { return g > 0.f ? s : (g < 0.f ? -s : (g == g ? 0.f : g)); }

// per-sample L2 factors, in double, from the sample's sum of squares ss
//   direction: x + g f is a step of length `step` along g
//   ball     : x0 + d f is d = x - x0 scaled back onto |d| <= eps; exactly 1 for a d inside the ball
__device__ __forceinline__ double l2_dir_factor(double ss, double step) { return step / fmax(sqrt(ss), 1e-12); }
__device__ __forceinline__ double l2_ball_factor(double ss, double eps) { return fmin(1.0, eps / fmax(sqrt(ss), 1e-12)); }

// x0 + d f with d = x - x0, then the clip; a factor of exactly 1 leaves x as it is before the clamp
__device__ __forceinline__ float l2_ball_elem(float x, float x0, double f, float lo, float hi) {
    const float v = f < 1.0 ? (float)((double)x0 + ((double)x - (double)x0) * f) : x;
    return clampf(v, lo, hi);
}

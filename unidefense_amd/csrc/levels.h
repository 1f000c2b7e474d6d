// What csrc/corrupt.hip and csrc/warp.hip share: the 8-bit grey level of a model input.  One definition, so that a corruption
// and a warp of the same batch read the same levels.
#pragma once
#include "ud_common.h"

// model units x in [-1, 1] (Normalize(0.5, 0.5)) -> u = clamp(floor((x + 1) 127.5 + 0.5), 0, 255) in fp32 with contraction off
__device__ __forceinline__ int level_of(float x) {
#pragma clang fp contract(off)
    const float t = (x + 1.0f) * 127.5f;
    if (!(t == t)) return 0;                       // NaN: level 0, on purpose
    float v = floorf(t + 0.5f);
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);   // +-inf clamp like any other value
    return (int)v;
}

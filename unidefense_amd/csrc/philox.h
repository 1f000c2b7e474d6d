// The counter-based noise that csrc/smooth.hip and csrc/hsj.hip share: Philox4x32-10, the symmetric 24-bit uniform and Box-Muller
// on a pair of words.  One definition each, so that a draw of the smoothing certificate and a direction of the decision-based
// attack are the same pure function of (seed, sample id, draw, element), with the same bits.
#pragma once
#include "attack_common.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr float TWO_M24 = 1.0f / 16777216.0f;

struct Words {
    uint32_t w[4];
};

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Words{{c0, c1, c2, c3}};
}

// the odd integer 2 m + 1 - 2^24 (|.| < 2^24, exact in fp32) times 2^-24: symmetric, never 0, inside (-1, 1)
__device__ __forceinline__ float uniform_of(uint32_t w) { return (float)(2 * (int)(w >> 8) + 1 - (1 << 24)) * TWO_M24; }

// Box-Muller on a pair of words: u1 in (0, 1], the angle 2 u2 in [0, 2) half turns, both exact
__device__ __forceinline__ void gaussian_pair(uint32_t wa, uint32_t wb, float& za, float& zb) {
    const float u1 = (float)((wa >> 8) + 1u) * TWO_M24;
    const float h = (float)(wb >> 8) * (2.0f * TWO_M24);
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(h, &s, &c);
    za = r * c;
    zb = r * s;
}

template <int MODE>
__device__ __forceinline__ void noise_quad(const Words& p, float t[4]) {
    if (MODE == UD_SMOOTH_UNIFORM) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = uniform_of(p.w[j]);
    } else {
        gaussian_pair(p.w[0], p.w[1], t[0], t[1]);
        gaussian_pair(p.w[2], p.w[3], t[2], t[3]);
    }
}

}  // namespace

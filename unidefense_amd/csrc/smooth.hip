// The kernel work on both sides of a randomized-smoothing draw (unidefense_amd/smooth.py: CertifyRunner): noise in, votes out.
//   ud_smooth_noise : out[n][e] = x[n][e] + scale noise(seed, ids[n], draw_n, e), one streaming pass, the noise made in registers
//   ud_smooth_vote  : one thread per sample: the draw's class, its logit margin, the phase's vote count, the draw counter
//
// The noise is a pure function of (seed, sample id, draw, element): Philox4x32-10 with the key (seed low, seed high) and the
// counter (q, draw, id low, id high), q the index of the quad of four consecutive elements of the flattened sample; element
// 4 q + j takes output word j.  Nothing depends on the sample's row, on N, on the launch geometry or on which of the two paths
// (float4 or scalar) stores the element, so one image's certificate can be re-created alone.  No table of draws exists in memory:
// the pass reads x and writes out, 8 bytes per element.
//
// One thread owns one quad in both paths.  Per quad: 10 rounds of 2 x (v_mul_lo + v_mul_hi) and 4 xors, then per element one
// product and one add (uniform) or per pair a logf, a sqrtf and a sincospif (Gaussian: Box-Muller with the accurate library
// functions; the angle 2 u2 is an exact fp32 number, so sincospif sees no rounded multiple of pi).
#include <climits>

#include "attack_common.h"
#include "philox.h"   // Philox4x32-10, uniform_of, gaussian_pair, noise_quad: shared with csrc/hsj.hip

namespace {

__device__ __forceinline__ float noisy(float x, float scale, float t) {
#pragma clang fp contract(off)
    const float d = scale * t;
    return x + d;
}

// VEC: per % 4 == 0 and both bases 16-byte aligned: one float4 load and store per quad; otherwise up to four scalar ones (the
// tail quad of a per that is no multiple of 4 uses its first words only).  out may be x: a thread reads its quad, then writes it.
template <int MODE, bool VEC>
__global__ __launch_bounds__(NT) void smooth_noise(const float* x, float* out, const long long* __restrict__ ids,
                                                   const int* __restrict__ k, uint32_t draw0, long per, long quads, float scale,
                                                   uint32_t seed_lo, uint32_t seed_hi) {
    const int n = blockIdx.y;
    const unsigned long long id = (unsigned long long)ids[n];
    const uint32_t draw = draw0 + (k ? (uint32_t)k[n] : 0u);
    const float* xs = x + (long)n * per;
    float* os = out + (long)n * per;
    const long nthr = (long)gridDim.x * NT;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < quads; q += nthr) {
        const Words p = philox4x32_10((uint32_t)q, draw, (uint32_t)id, (uint32_t)(id >> 32), seed_lo, seed_hi);
        float t[4];
        noise_quad<MODE>(p, t);
        if (VEC) {
            f32x4 v = reinterpret_cast<const f32x4*>(xs)[q];
            v.x = noisy(v.x, scale, t[0]);
            v.y = noisy(v.y, scale, t[1]);
            v.z = noisy(v.z, scale, t[2]);
            v.w = noisy(v.w, scale, t[3]);
            reinterpret_cast<f32x4*>(os)[q] = v;
        } else {
            const long e0 = 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < per) os[e0 + j] = noisy(xs[e0 + j], scale, t[j]);
        }
    }
}

template <int MODE>
int launch_noise(const float* x, float* out, const long long* ids, const int* k, uint32_t draw0, int N, long per, float scale,
                 unsigned long long seed, hipStream_t s) {
    const long quads = (per + 3) / 4;
    const dim3 grid((unsigned)ew_blocks(quads), (unsigned)N);
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    if (per % 4 == 0 && aligned16(x) && aligned16(out))
        hipLaunchKernelGGL((smooth_noise<MODE, true>), grid, dim3(NT), 0, s, x, out, ids, k, draw0, per, quads, scale, lo, hi);
    else
        hipLaunchKernelGGL((smooth_noise<MODE, false>), grid, dim3(NT), 0, s, x, out, ids, k, draw0, per, quads, scale, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

// ---- vote: one thread per sample; only its own rows of votes, margins, counts and ist are touched -------------------------------
__global__ __launch_bounds__(64) void smooth_vote(const float* __restrict__ logits, int N, int C, int* __restrict__ ist,
                                                  int* __restrict__ counts, int* __restrict__ votes,
                                                  float* __restrict__ margins, int draws, int n0) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int d = ist[(long)UD_SMOOTH_I_K * N + n];
    if (d < 0 || d >= draws) return;
    const float* row = logits + (long)n * C;
    const int Ce = C < 2 ? 2 : C;
    int cls;
    float margin;
    bool valid = true;
    if (C == 1) {
        const float v = row[0];
        valid = v == v;
        cls = v > 0.f ? 1 : 0;
        margin = fabsf(v);
    } else {
        float best = row[0], second = -INFINITY;
        valid = best == best;
        cls = 0;
        for (int c = 1; c < C; ++c) {
            const float v = row[c];
            valid = valid && v == v;
            if (v > best) {                      // strict: the first maximum keeps the vote
                second = best;
                best = v;
                cls = c;
            } else if (v > second) {
                second = v;
            }
        }
        margin = best - second;
    }
    if (!valid) {
        cls = -1;
        margin = __uint_as_float(0x7fc00000u);
    }
    votes[(long)d * N + n] = cls;
    margins[(long)d * N + n] = margin;
    if (valid) counts[((long)(d < n0 ? 0 : 1) * N + n) * Ce + cls] += 1;
    ist[(long)UD_SMOOTH_I_K * N + n] = d + 1;
}

}  // namespace

extern "C" {

int ud_smooth_noise(const float* x, float* out, const long long* ids, const int* k, int draw0, int N, long per, int mode,
                    float scale, long seed, ud_stream_t stream) {
    if (!x || !out || !ids) return UD_EINVAL;
    if (!shape_ok(N, per) || per > (1L << 34)) return UD_EINVAL;
    if (mode != UD_SMOOTH_GAUSSIAN && mode != UD_SMOOTH_UNIFORM) return UD_EINVAL;
    if (!(scale >= 0.f)) return UD_EINVAL;
    if (mode == UD_SMOOTH_GAUSSIAN)
        return launch_noise<UD_SMOOTH_GAUSSIAN>(x, out, ids, k, (uint32_t)draw0, N, per, scale, (unsigned long long)seed,
                                                (hipStream_t)stream);
    return launch_noise<UD_SMOOTH_UNIFORM>(x, out, ids, k, (uint32_t)draw0, N, per, scale, (unsigned long long)seed,
                                           (hipStream_t)stream);
}

int ud_smooth_vote(const float* logits, int N, int C, int* ist, int* counts, int* votes, float* margins, int draws, int n0,
                   ud_stream_t stream) {
    if (!logits || !ist || !counts || !votes || !margins) return UD_EINVAL;
    if (N < 1 || C < 1 || draws < 1 || n0 < 0 || n0 > draws) return UD_EINVAL;
    if ((long)draws * N > INT_MAX || 2L * N * (C < 2 ? 2 : C) > INT_MAX) return UD_EINVAL;
    hipLaunchKernelGGL(smooth_vote, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, logits, N, C, ist, counts,
                       votes, margins, draws, n0);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

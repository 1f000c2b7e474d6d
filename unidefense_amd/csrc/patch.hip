// The adversarial patch's kernels (unidefense_amd/patch.py: paste, PatchRunner): ONE small texture patch [3][P][P] with a fixed
// coverage mask alpha [P][P] is pasted into every sample under that sample's own affine placement (a centre, a roll, a size),
// and the attack ascends the summed loss in the texture.
//   ud_patch_paste  : out(p) = clamp((1 - cov(p)) x(p) + sum over p's four taps of omega patch(tap)), x's own bits outside
//   ud_patch_grad   : gp[n](t) = sum over the pixels p that name the texel t as a tap of omega(p, t) g[n](p): the adjoint of the
//                     paste with respect to the texture, per sample (ud_uap_reduce then sums the counted samples)
//   ud_patch_update : patch <- clamp(patch + step sign(gsum), lo, hi)
// The natural adjoint scatters with atomics; here it is a GATHER, so that a replay gives the same bits: a thread owns one texel
// (its three channels), maps it forward to the nearest pixel, walks the (2 reach + 1)^2 window around that pixel in row-major
// order and evaluates for each candidate the SAME integer inverse map the paste evaluates, keeping the tap that names its own
// texel.  The weights are exact integers (Q16 coordinates, 8-bit fractions) times alpha, rounded once: both directions use the
// one omega.  Sums over a window are in double and rounded once.  No atomics, no workspace, no LDS; plain vector loads and
// stores.  The placement rows are device data the host cannot see at launch: the row index is clamped into the table, reach
// into [0, 8], the window is cut to the image and every tap is tested against [0, P - 1]^2, so the kernels stay in bounds for
// any content of the table.  The rules are the header's (include/unidefense_hip.h); nothing here is contracted.
//
// The paste follows csrc/flow.hip's tile: a workgroup owns 64 columns x 4 rows of one sample, one wave per row, a thread its
// pixel's three channels, so x and out are coalesced and the taps are computed once; the texture is small and stays in L1 / L2.
// Measured on the MI355X at UDEB4's 256^2 bs 96 with P = 64 (profiles/r31/patch.txt), operands rotated out of the Infinity Cache:
// the paste 34.0 us for 151 MB (81 % of 5.5 TB/s), the gather 20.2 us, the update 9.3 us; the captured iteration 52.97 ms next
// to UniversalRunner's 53.25 ms.
#include <climits>

#include "attack_common.h"

namespace {

constexpr int TX = 64;                    // the paste's tile: one wave per row
constexpr int TY = NT / TX;
constexpr int ROW = UD_PATCH_ROW;         // int32 words per placement
constexpr int MAX_REACH = UD_PATCH_MAX_REACH;

// the placement of sample n: row clamp(k[0], 0, rows - 1) of table [rows][N][ROW]
__device__ __forceinline__ const int* place_of(const int* __restrict__ table, const int* __restrict__ k, int rows, int N, int n) {
    int kk = k[0];
    kk = kk < 0 ? 0 : (kk > rows - 1 ? rows - 1 : kk);
    return table + ((long)kk * N + n) * ROW;
}

// the integer weight (in 1 / 65536) of the tap (i0 + di, j0 + dj) of a pixel with the fractions (fy, fx), di, dj in {0, 1}
__device__ __forceinline__ int tap_weight(int fx, int fy, int dj, int di) { return (dj ? fx : 256 - fx) * (di ? fy : 256 - fy); }

// omega = fl32(w alpha): w = wi / 65536 is exact
__device__ __forceinline__ float omega_of(int wi, float a) {
#pragma clang fp contract(off)
    return ((float)wi * (1.f / 65536.f)) * a;
}

__global__ __launch_bounds__(NT) void patch_paste(const float* __restrict__ x, const float* __restrict__ patch,
                                                  const float* __restrict__ alpha, const int* __restrict__ table,
                                                  const int* __restrict__ k, int rows, float* __restrict__ out, int N, int S, int P,
                                                  float lo, float hi) {
#pragma clang fp contract(off)
    const int n = blockIdx.z, c = blockIdx.x * TX + threadIdx.x % TX, r = blockIdx.y * TY + threadIdx.x / TX;
    if (c >= S || r >= S) return;
    const int* m = place_of(table, k, rows, N, n);
    const long U = (long)m[0] * c + (long)m[1] * r + m[2], V = (long)m[3] * c + (long)m[4] * r + m[5];
    const long j0 = U >> 16, i0 = V >> 16;
    const int fx = (int)(U >> 8) & 255, fy = (int)(V >> 8) & 255;
    const long plane = (long)S * S, p = (long)r * S + c, pp = (long)P * P;
    const float* xs = x + (long)n * 3 * plane + p;
    float* os = out + (long)n * 3 * plane + p;
    float x0 = xs[0], x1 = xs[plane], x2 = xs[2 * plane];
    if (i0 >= -1 && i0 <= P - 1 && j0 >= -1 && j0 <= P - 1) {          // some tap inside the texture
        float cov = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int di = t >> 1, dj = t & 1;
            const long i = i0 + di, j = j0 + dj;
            if (i < 0 || i > P - 1 || j < 0 || j > P - 1) continue;
            const int wi = tap_weight(fx, fy, dj, di);
            if (wi == 0) continue;
            const long q = i * P + j;
            const float om = omega_of(wi, alpha[q]);
            if (om == 0.f) continue;
            any = true;
            cov = cov + om;
            a0 = a0 + om * patch[q];
            a1 = a1 + om * patch[pp + q];
            a2 = a2 + om * patch[2 * pp + q];
        }
        if (any && cov != 0.f) {
            const float keep = 1.f - cov;
            x0 = clampf(keep * x0 + a0, lo, hi);
            x1 = clampf(keep * x1 + a1, lo, hi);
            x2 = clampf(keep * x2 + a2, lo, hi);
        }
    }
    os[0] = x0, os[plane] = x1, os[2 * plane] = x2;
}

__global__ __launch_bounds__(NT) void patch_grad(const float* __restrict__ g, const float* __restrict__ alpha,
                                                 const int* __restrict__ table, const int* __restrict__ k, int rows,
                                                 float* __restrict__ gp, int N, int S, int P) {
    const int n = blockIdx.y, t = blockIdx.x * NT + threadIdx.x;
    const int pp = P * P;
    if (t >= pp) return;
    const int i = t / P, j = t - i * P;
    const int* m = place_of(table, k, rows, N, n);
    const long m00 = m[0], m01 = m[1], o0 = m[2], m10 = m[3], m11 = m[4], o1 = m[5];
    // the pixel nearest the texel's image under the forward map
    const long pc = ((long)m[6] * j + (long)m[7] * i + m[8] + 32768) >> 16, pr = ((long)m[9] * j + (long)m[10] * i + m[11] + 32768) >> 16;
    int reach = m[12];
    reach = reach < 0 ? 0 : (reach > MAX_REACH ? MAX_REACH : reach);
    const long r0 = pr - reach < 0 ? 0 : pr - reach, r1 = pr + reach > S - 1 ? S - 1 : pr + reach;
    const long c0 = pc - reach < 0 ? 0 : pc - reach, c1 = pc + reach > S - 1 ? S - 1 : pc + reach;
    const float a = alpha[t];
    const long plane = (long)S * S;
    const float* gs = g + (long)n * 3 * plane;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (a != 0.f) {
        for (long r = r0; r <= r1; ++r) {
            long U = m00 * c0 + m01 * r + o0, V = m10 * c0 + m11 * r + o1;
            for (long c = c0; c <= c1; ++c, U += m00, V += m10) {
                const long dj = j - (U >> 16), di = i - (V >> 16);
                if ((dj | di) & ~1L) continue;                        // the texel is none of this pixel's four taps
                const int wi = tap_weight((int)(U >> 8) & 255, (int)(V >> 8) & 255, (int)dj, (int)di);
                if (wi == 0) continue;
                const float om = omega_of(wi, a);
                if (om == 0.f) continue;
                const long p = r * S + c;
                s0 += (double)om * (double)gs[p];
                s1 += (double)om * (double)gs[plane + p];
                s2 += (double)om * (double)gs[2 * plane + p];
            }
        }
    }
    float* os = gp + (long)n * 3 * pp + t;
    os[0] = (float)s0, os[pp] = (float)s1, os[2 * pp] = (float)s2;
}

__global__ __launch_bounds__(NT) void patch_update(float* __restrict__ patch, const float* __restrict__ gsum, long per, float step,
                                                   float lo, float hi) {
#pragma clang fp contract(off)
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long e = tid; e < per; e += nthr) patch[e] = clampf(patch[e] + sign_inc(gsum[e], step), lo, hi);
}

inline bool image_ok(int N, int S, int P) { return N >= 1 && N <= 65535 && S >= 2 && S <= 32768 && P >= 1 && P <= 256; }

}  // namespace

extern "C" {

int ud_patch_paste(const float* x, const float* patch, const float* alpha, const int* table, const int* k, int rows, float* out,
                   int N, int S, int P, float lo, float hi, ud_stream_t stream) {
    if (!x || !patch || !alpha || !table || !k || !out || out == x || !image_ok(N, S, P) || rows < 1 || !(lo <= hi)) return UD_EINVAL;
    hipLaunchKernelGGL(patch_paste, dim3((unsigned)ud_cdiv(S, TX), (unsigned)ud_cdiv(S, TY), (unsigned)N), dim3(NT), 0,
                       (hipStream_t)stream, x, patch, alpha, table, k, rows, out, N, S, P, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_patch_grad(const float* g, const float* alpha, const int* table, const int* k, int rows, float* gp, int N, int S, int P,
                  ud_stream_t stream) {
    if (!g || !alpha || !table || !k || !gp || gp == g || !image_ok(N, S, P) || rows < 1) return UD_EINVAL;
    hipLaunchKernelGGL(patch_grad, dim3((unsigned)ud_cdiv((long)P * P, NT), (unsigned)N), dim3(NT), 0, (hipStream_t)stream, g, alpha,
                       table, k, rows, gp, N, S, P);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_patch_update(float* patch, const float* gsum, long per, float step, float lo, float hi, ud_stream_t stream) {
    if (!patch || !gsum || patch == gsum || per < 1 || per > 3L * 256 * 256 || step != step || !(lo <= hi)) return UD_EINVAL;
    hipLaunchKernelGGL(patch_update, dim3(ew_blocks(per)), dim3(NT), 0, (hipStream_t)stream, patch, gsum, per, step, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

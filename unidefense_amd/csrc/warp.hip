// Affine warps on the device and the per-sample state of the worst-case spatial search (unidefense_amd/spatial.py: warp,
// SpatialRunner).  Like the corruptions (csrc/corrupt.hip) a warp is defined on 8-bit levels in integers and is ONE launch:
//   (a) level_of (levels.h): model units -> 0..255;
//   (b) for the output pixel (r, c): X = 2c + 1 - S, Y = 2r + 1 - S (centred half pixels); with the sample's six int32
//       (m00, m01, o0, m10, m11, o1):  px = (m00 X + m01 Y + o0 + ((S - 1) << 16)) >> 1,  py likewise: int64, arithmetic shift,
//       the source column and row in Q16 pixels;  x0 = px >> 16, fx = (px >> 8) & 255, y0, fy likewise;  the four taps
//       (y0 | y0 + 1, x0 | x0 + 1), each index through the border rule on its own;
//       v = ((256 - fx)(256 - fy) u00 + fx (256 - fy) u01 + (256 - fx) fy u10 + fx fy u11 + 32768) >> 16: the four weights sum to
//       2^16, so the sum is at most 255 * 2^16 + 2^15 < 2^31 and v is a level without a clamp;
//   (c) out = lut[v].
// No floating-point operation decides an output bit after (a): tests/test_spatial_cpu.py restates the kernel in numpy and the GPU
// tests compare bit for bit.  Ordinary vector loads and stores only, no atomics, nothing shared between workgroups.
//
// A workgroup owns a TW x TW tile of one sample's output, all three channels.  px and py are floors of functions that are linear
// in r and in c, so over the tile's rectangle x0 and y0 take their extremes at the four corner pixels: the taps lie in the box
// [min x0, max x0 + 1] x [min y0, max y0 + 1], exactly.  A box of at most BOX_MAX cells is staged in LDS once, as levels, the
// border rule applied while staging and the three channels of a cell packed into one dword (r | g << 8 | b << 16): a tap is
// one ds_read_b32 for all channels, four LDS reads per output pixel, and the interpolation loop has no branch.  A larger box
// (strong minification, or a garbage table) reads its taps from global memory with the same border rule: a workgroup-uniform
// branch with identical results.  mat and row are device data that the host cannot see at launch: the row index is clamped and
// every coordinate is int64, so any content of either keeps every access in bounds.
#include <climits>

#include "attack_common.h"
#include "levels.h"

namespace {

constexpr int TW = 32;                    // the tile's side: NT threads, four output pixels each
constexpr int BOX_MAX = 4608;             // staged cells: 18 KiB of LDS + the level table's 1 KiB, eight workgroups per CU

// position of `i` in the period 2 (S - 1) of reflect-101 (mathematical mod: any distance, either sign); 0 for S == 1
__device__ __forceinline__ unsigned reflect_phase(long i, int S) {
    if (S == 1) return 0u;
    const long p = 2L * (S - 1);
    const long j = i % p;
    return (unsigned)(j < 0 ? j + p : j);
}

// the source index of coordinate base + l (0 <= l <= BOX_MAX) under the border rule; phase = reflect_phase(base, S);
// -1: outside, under UD_WARP_FILL
__device__ __forceinline__ int border_index(long base, unsigned phase, int l, int S, int border) {
    if (border == UD_WARP_REFLECT) {
        if (S == 1) return 0;
        const unsigned p = 2u * (unsigned)(S - 1);
        const unsigned j = (phase + (unsigned)l) % p;                 // phase < p <= 65534, l <= BOX_MAX
        return (int)(j >= (unsigned)S ? p - j : j);
    }
    const long g = base + l;
    if (border == UD_WARP_EDGE) return g < 0 ? 0 : (g > S - 1 ? S - 1 : (int)g);
    return g < 0 || g > S - 1 ? -1 : (int)g;
}

// the packed levels of the source pixel (sy, sx); an index of -1 is the fill level in every channel
__device__ __forceinline__ unsigned packed_levels(const float* __restrict__ xs, long plane, int S, int sy, int sx) {
    if (sy < 0 || sx < 0) return 128u | 128u << 8 | 128u << 16;
    const long p = (long)sy * S + sx;
    return (unsigned)level_of(xs[p]) | (unsigned)level_of(xs[p + plane]) << 8 | (unsigned)level_of(xs[p + 2 * plane]) << 16;
}

struct Affine {
    long m00, m01, c0, m10, m11, c1;      // c* = o* + ((S - 1) << 16)
    int S;
    __device__ __forceinline__ long px(int r, int c) const { return (m00 * (2L * c + 1 - S) + m01 * (2L * r + 1 - S) + c0) >> 1; }
    __device__ __forceinline__ long py(int r, int c) const { return (m10 * (2L * c + 1 - S) + m11 * (2L * r + 1 - S) + c1) >> 1; }
};

__device__ __forceinline__ long min2(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long max2(long a, long b) { return a > b ? a : b; }
__device__ __forceinline__ long min4(long a, long b, long c, long d) { return min2(min2(a, b), min2(c, d)); }
__device__ __forceinline__ long max4(long a, long b, long c, long d) { return max2(max2(a, b), max2(c, d)); }

__global__ __launch_bounds__(NT) void warp_affine(const float* __restrict__ x, float* __restrict__ out,
                                                  const float* __restrict__ lut, const int* __restrict__ mat,
                                                  const int* __restrict__ row, int size, int rows, int border) {
    __shared__ unsigned box[BOX_MAX];
    __shared__ float slut[256];
    const int tid = threadIdx.x, S = size;
    const int n = blockIdx.z;
    int rw = row[n];
    rw = rw < 0 ? 0 : (rw > rows - 1 ? rows - 1 : rw);                // the contract: any content of row stays inside mat
    const int* m = mat + (long)rw * 6;
    const long centre = (long)(S - 1) << 16;
    const Affine A{m[0], m[1], (long)m[2] + centre, m[3], m[4], (long)m[5] + centre, S};
    const long plane = (long)S * S;
    const float* xs = x + (long)n * 3 * plane;
    float* os = out + (long)n * 3 * plane;
    slut[tid] = lut[tid];

    // the tile's rectangle inside the image and the box of its taps: uniform over the workgroup
    const int r0 = blockIdx.y * TW, c0 = blockIdx.x * TW;
    const int r1 = (r0 + TW < S ? r0 + TW : S) - 1, c1 = (c0 + TW < S ? c0 + TW : S) - 1;
    const long xa = A.px(r0, c0) >> 16, xb = A.px(r0, c1) >> 16, xc = A.px(r1, c0) >> 16, xd = A.px(r1, c1) >> 16;
    const long ya = A.py(r0, c0) >> 16, yb = A.py(r0, c1) >> 16, yc = A.py(r1, c0) >> 16, yd = A.py(r1, c1) >> 16;
    const long bx = min4(xa, xb, xc, xd), by = min4(ya, yb, yc, yd);
    const long bw = max4(xa, xb, xc, xd) - bx + 2, bh = max4(ya, yb, yc, yd) - by + 2;
    const bool staged = bw <= BOX_MAX && bh <= BOX_MAX && bw * bh <= BOX_MAX;
    const int w = staged ? (int)bw : 0;

    if (staged) {
        const unsigned phx = reflect_phase(bx, S), phy = reflect_phase(by, S);
        const int cells = w * (int)bh;
        for (int i = tid; i < cells; i += NT) {
            const int ly = i / w, lx = i - ly * w;
            box[i] = packed_levels(xs, plane, S, border_index(by, phy, ly, S, border), border_index(bx, phx, lx, S, border));
        }
    }
    __syncthreads();

    for (int i = tid; i < TW * TW; i += NT) {
        const int r = r0 + i / TW, c = c0 + i % TW;
        if (r >= S || c >= S) continue;                               // the image's edge inside the last tiles
        const long px = A.px(r, c), py = A.py(r, c);
        const long x0 = px >> 16, y0 = py >> 16;
        const int fx = (int)(px >> 8) & 255, fy = (int)(py >> 8) & 255;
        unsigned t00, t01, t10, t11;
        if (staged) {
            const unsigned* b = box + (int)(y0 - by) * w + (int)(x0 - bx);
            t00 = b[0], t01 = b[1], t10 = b[w], t11 = b[w + 1];
        } else {
            const unsigned phx = reflect_phase(x0, S), phy = reflect_phase(y0, S);
            const int sx0 = border_index(x0, phx, 0, S, border), sx1 = border_index(x0, phx, 1, S, border);
            const int sy0 = border_index(y0, phy, 0, S, border), sy1 = border_index(y0, phy, 1, S, border);
            t00 = packed_levels(xs, plane, S, sy0, sx0), t01 = packed_levels(xs, plane, S, sy0, sx1);
            t10 = packed_levels(xs, plane, S, sy1, sx0), t11 = packed_levels(xs, plane, S, sy1, sx1);
        }
        const int w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
        const long p = (long)r * S + c;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int sh = 8 * ch;
            const int v = (w00 * (int)(t00 >> sh & 255u) + w01 * (int)(t01 >> sh & 255u) + w10 * (int)(t10 >> sh & 255u) +
                           w11 * (int)(t11 >> sh & 255u) + 32768) >> 16;
            os[p + ch * plane] = slut[v];
        }
    }
}

// ---- control: one thread per sample ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void spatial_control(const float* __restrict__ f, int* __restrict__ ist,
                                                      float* __restrict__ fst, float* __restrict__ history, int K, int N,
                                                      int closing) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    if (closing) {                                                    // the winner's row for the last warp
        int b = ist[(long)UD_SPATIAL_I_BEST_K * N + n];
        b = b < 0 ? 0 : (b > K - 1 ? K - 1 : b);
        ist[(long)UD_SPATIAL_I_ROW * N + n] = b * N + n;
        return;
    }
    const int k = ist[(long)UD_SPATIAL_I_K * N + n];
    if (k < 0 || k >= K) return;
    const float fk = f[n];
    history[(long)k * N + n] = fk;
    if (k == 0 || fk < fst[(long)UD_SPATIAL_F_BEST * N + n]) {        // strict: a tie keeps the lowest k, a NaN never wins
        fst[(long)UD_SPATIAL_F_BEST * N + n] = fk;
        ist[(long)UD_SPATIAL_I_BEST_K * N + n] = k;
    }
    ist[(long)UD_SPATIAL_I_ROW * N + n] = (k + 1 < K - 1 ? k + 1 : K - 1) * N + n;
    ist[(long)UD_SPATIAL_I_K * N + n] = k + 1;
}

}  // namespace

extern "C" {

int ud_warp_affine(const float* x, float* out, const float* lut, const int* mat, const int* row, int N, int size, int rows,
                   int border, ud_stream_t stream) {
    if (!x || !out || !lut || !mat || !row || x == out) return UD_EINVAL;
    if (N < 1 || N > 65535 || size < 1 || size > 32768 || rows < 1) return UD_EINVAL;
    if (border != UD_WARP_REFLECT && border != UD_WARP_EDGE && border != UD_WARP_FILL) return UD_EINVAL;
    const dim3 grid((unsigned)ud_cdiv(size, TW), (unsigned)ud_cdiv(size, TW), (unsigned)N);
    hipLaunchKernelGGL(warp_affine, grid, dim3(NT), 0, (hipStream_t)stream, x, out, lut, mat, row, size, rows, border);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_spatial_control(const float* f, int* ist, float* fst, float* history, int K, int N, int closing, ud_stream_t stream) {
    if (!ist || K < 1 || N < 1 || (long)K * N > INT_MAX) return UD_EINVAL;
    if (!closing && (!f || !fst || !history)) return UD_EINVAL;
    hipLaunchKernelGGL(spatial_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ist, fst, history, K,
                       N, closing);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

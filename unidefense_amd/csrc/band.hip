// The device side of the frequency-band attack (unidefense_amd/band.py: dct2, idct2, BandRunner): a per-plane 2-D DCT on the
// fp32-input MFMA and the two streaming kernels of the band-limited L2 step.
//   ud_plane_dct2  : forward  y_p = mask (.) (D x_p D^T),  inverse  y_p = D^T (mask (.) x_p) D  [+ base, clamped], any side S
//   ud_band_dots   : per sample |w|^2, <w, G>, |G|^2 in one pass, double partials folded in a fixed order
//   ud_band_update : w <- s (w + a G), a and s formed per sample from the three dots: step and ball projection in one pass
//
// The transform.  Both directions are  Y = L (A R)  with A the (masked) input plane and L, R one of D, D^T: the host hands over
// D and its transpose, both row-major, so the kernel has ONE form: forward (L, R) = (D, D^T), inverse (D^T, D).  A 256^2 fp32
// plane (256 KB) does not fit the LDS, a 32-column strip of the intermediate does: one workgroup per (plane, 32-column strip)
//   stage 1: U = A R[:, strip]   (S x 32) into LDS, the four waves take the 32-row tiles in turn
//   stage 2: Y[:, strip] = L U   the four waves take the 32-row tiles of Y in turn, U is the MFMA's B operand out of LDS
// with A, L and R read through L2 (each strip re-reads the plane; at S = 256 that is 8 reads of 256 KB per plane, all but the
// first from L2).  Products are exact fp32 on v_mfma_f32_32x32x2_f32 with fp32 accumulation.  The k index is walked in a fixed
// permuted order (lane half h of MFMA q of a group of four takes k = k0 + 4 h + q) so that a lane's four A values are one
// 16-byte load; the order depends on S alone, so a replay gives the same bits.  Rows, columns and k past S are loaded as
// zeros in BOTH operands (never 0 * NaN from outside the plane) and never stored.
#include "attack_common.h"

namespace {

constexpr int TS = 32;               // strip width and MFMA tile side
constexpr int ULD = TS + 1;          // row stride of U in LDS (floats)
constexpr int DCT_MAX_S = 480;       // ceil32(S) * ULD * 4 bytes of LDS: 63360 at 480, within 64 KB (512 rows would be 67584)

// four consecutive elements row[k .. k + 3] of a row of length S; VEC: one 16-byte load (S % 4 == 0, aligned base, k % 4 == 0)
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ row, int k, int S, bool row_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if (VEC) {
        if (k < S) v = *reinterpret_cast<const f32x4*>(row + k);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < S) v[e] = row[k + e];
    }
    return v;
}

// Y = L (A R) for strip blockIdx.x % strips of plane blockIdx.x / strips.  in_mask multiplies A on load (inverse), out_mask
// multiplies Y on store (forward); base != nullptr: Y <- clamp(base + Y, lo, hi).
template <bool VEC>
__global__ __launch_bounds__(NT) void plane_dct2(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ L,
                                                 const float* __restrict__ R, const float* __restrict__ in_mask,
                                                 const float* __restrict__ out_mask, const float* __restrict__ base, int S,
                                                 int strips, float lo, float hi) {
    extern __shared__ float U[];                                   // [ceil32(S)][ULD]
    const long plane = blockIdx.x / strips;
    const int v0 = (int)(blockIdx.x % strips) * TS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const int tiles = (S + TS - 1) / TS;
    const float* xp = x + plane * (long)S * S;
    const int col = v0 + l31;
    const bool col_ok = col < S;

    // ---- stage 1: U[i][v] = sum_j A[i][j] R[j][v0 + v] ----
    for (int t = wave; t < tiles; t += NT / 64) {
        const int i = t * TS + l31;
        const bool row_ok = i < S;
        const float* arow = xp + (long)i * S;
        const float* mrow = in_mask ? in_mask + (long)i * S : nullptr;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < S; k0 += 8) {
            const int k = k0 + 4 * half;
            f32x4 a = load4<VEC>(arow, k, S, row_ok);
            if (mrow) {
                const f32x4 m = load4<VEC>(mrow, k, S, row_ok);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = a[e] * m[e];
            }
            float b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = (col_ok && k + q < S) ? R[(long)(k + q) * S + col] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
        }
        // D[i][j]: j = lane & 31, i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
        for (int r = 0; r < 16; ++r) U[(t * TS + (r & 3) + 8 * (r >> 2) + 4 * half) * ULD + l31] = acc[r];
    }
    __syncthreads();

    // ---- stage 2: Y[u][v0 + v] = sum_i L[u][i] U[i][v] ----
    float* yp = y + plane * (long)S * S;
    const float* bp = base ? base + plane * (long)S * S : nullptr;
    for (int t = wave; t < tiles; t += NT / 64) {
        const int u = t * TS + l31;
        const bool row_ok = u < S;
        const float* lrow = L + (long)u * S;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < S; k0 += 8) {
            const int k = k0 + 4 * half;
            const f32x4 a = load4<VEC>(lrow, k, S, row_ok);
            float b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = k + q < tiles * TS ? U[(k + q) * ULD + l31] : 0.f;   // rows [S, ceil32(S)) hold zeros
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
        }
        if (!col_ok) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
            const int row = t * TS + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (row >= S) continue;
            const long o = (long)row * S + col;
            float v = acc[r];
            if (out_mask) v = v * out_mask[o];
            if (bp) v = clampf(bp[o] + v, lo, hi);
            yp[o] = v;
        }
    }
}

// ---- the three dots ------------------------------------------------------------------------------------------------------------
constexpr int CHUNK = 4096;          // elements of one sample that one workgroup sums: ud_sample_sumsq's partition

inline long dots_parts(long per) { return (per + CHUNK - 1) / CHUNK; }

// Part p of sample n: the three sums over i in [p CHUNK, min(per, (p + 1) CHUNK)), products and sums formed in double.  Every
// thread adds its elements in index order, the wave folds by shuffles, the four waves are added in wave order: a fixed tree.
template <bool VEC>
__global__ __launch_bounds__(NT) void band_dots_parts(const float* __restrict__ w, const float* __restrict__ g, long per,
                                                      double* __restrict__ dst) {
#pragma clang fp contract(off)
    const long n = blockIdx.y, p = blockIdx.x;
    const long lo = p * CHUNK, hi = lo + CHUNK < per ? lo + CHUNK : per;
    const float* pw = w + n * per;
    const float* pg = g + n * per;
    double ww = 0.0, wg = 0.0, gg = 0.0;
    if (VEC) {           // per % 4 == 0 and 16-byte aligned bases: lo and hi are multiples of 4
        for (long i = lo / 4 + threadIdx.x; i < hi / 4; i += NT) {
            const f32x4 a = reinterpret_cast<const f32x4*>(pw)[i];
            const f32x4 b = reinterpret_cast<const f32x4*>(pg)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double da = (double)a[e], db = (double)b[e];
                ww += da * da;
                wg += da * db;
                gg += db * db;
            }
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += NT) {
            const double da = (double)pw[i], db = (double)pg[i];
            ww += da * da;
            wg += da * db;
            gg += db * db;
        }
    }
    ww = ud_wave_sum_d(ww);
    wg = ud_wave_sum_d(wg);
    gg = ud_wave_sum_d(gg);
    __shared__ double part[3][NT / 64];
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = ww;
        part[1][threadIdx.x >> 6] = wg;
        part[2][threadIdx.x >> 6] = gg;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = part[threadIdx.x][0];
#pragma unroll
        for (int k = 1; k < NT / 64; ++k) s += part[threadIdx.x][k];
        dst[(n * gridDim.x + p) * 3 + threadIdx.x] = s;
    }
}

// out[n][c] = ws[n][0][c] + ws[n][1][c] + ... in index order (one thread per sample and dot)
__global__ __launch_bounds__(64) void band_dots_fold(const double* __restrict__ ws, int N, long parts, double* __restrict__ out) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 64 + threadIdx.x;
    if (t >= 3L * N) return;
    const long n = t / 3, c = t % 3;
    double s = 0.0;
    for (long p = 0; p < parts; ++p) s += ws[(n * parts + p) * 3 + c];
    out[t] = s;
}

// ---- the update ----------------------------------------------------------------------------------------------------------------
// a = step / max(|G|, 1e-12); n2 = |w|^2 + 2 a <w, G> + a^2 |G|^2; s = min(1, eps / max(sqrt(max(n2, 0)), 1e-12))
__device__ __forceinline__ void band_factors(const double* __restrict__ dots, long n, double step, double eps, double& a,
                                             double& s) {
#pragma clang fp contract(off)
    const double ww = dots[3 * n], wg = dots[3 * n + 1], gg = dots[3 * n + 2];
    a = step / fmax(sqrt(gg), 1e-12);
    const double n2 = ww + 2.0 * a * wg + a * a * gg;
    s = fmin(1.0, eps / fmax(sqrt(fmax(n2, 0.0)), 1e-12));
}

__device__ __forceinline__ float band_elem(float w, float g, double a, double s) {
#pragma clang fp contract(off)
    return (float)(s * ((double)w + a * (double)g));
}

// one sample per blockIdx.y; nvec float4 groups of the sample, then its scalar tail
__global__ __launch_bounds__(NT) void band_update(float* __restrict__ w, const float* __restrict__ g,
                                                  const double* __restrict__ dots, long per, long nvec, double step, double eps) {
    const long n = blockIdx.y;
    double a, s;
    band_factors(dots, n, step, eps, a, s);
    float* pw = w + n * per;
    const float* pg = g + n * per;
    const long tid = (long)blockIdx.x * NT + threadIdx.x, nthr = (long)gridDim.x * NT;
    for (long i = tid; i < nvec; i += nthr) {
        f32x4 v = reinterpret_cast<const f32x4*>(pw)[i];
        const f32x4 d = reinterpret_cast<const f32x4*>(pg)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = band_elem(v[e], d[e], a, s);
        reinterpret_cast<f32x4*>(pw)[i] = v;
    }
    for (long i = 4 * nvec + tid; i < per; i += nthr) pw[i] = band_elem(pw[i], pg[i], a, s);
}

}  // namespace

extern "C" {

int ud_plane_dct2(const float* x, float* y, const float* d, const float* dt, const float* mask, const float* base, long P, int S,
                  int inverse, int clip, float lo, float hi, ud_stream_t stream) {
    if (!x || !y || !d || !dt || x == y || d == dt) return UD_EINVAL;
    if (S < 2 || S > DCT_MAX_S || P < 1) return UD_EINVAL;
    if (base && (!inverse || !clip)) return UD_EINVAL;             // the apply epilogue is the inverse's, and it clamps
    if (clip && (!base || !(lo <= hi))) return UD_EINVAL;
    if (base == y) return UD_EINVAL;
    const int strips = (S + TS - 1) / TS;
    if (P > 0x7fffffffL / strips) return UD_EINVAL;
    const float* L = inverse ? dt : d;
    const float* R = inverse ? d : dt;
    const float* in_mask = inverse ? mask : nullptr;
    const float* out_mask = inverse ? nullptr : mask;
    const size_t lds = (size_t)strips * TS * ULD * sizeof(float);
    const dim3 grid((unsigned)(P * strips));
    // the 16-byte loads are those of x, L and the inverse's mask; R, the forward's mask, base and y are accessed by element
    if (S % 4 == 0 && aligned16(x) && aligned16(L) && (!in_mask || aligned16(in_mask)))
        hipLaunchKernelGGL(plane_dct2<true>, grid, dim3(NT), lds, (hipStream_t)stream, x, y, L, R, in_mask, out_mask, base, S, strips,
                           lo, hi);
    else
        hipLaunchKernelGGL(plane_dct2<false>, grid, dim3(NT), lds, (hipStream_t)stream, x, y, L, R, in_mask, out_mask, base, S,
                           strips, lo, hi);
    UD_LAUNCH_CHECK();
    return 0;
}

// ws: three times ud_sample_sumsq_ws_bytes(N, per), the same partition with three sums per part
int ud_band_dots(const float* w, const float* g, int N, long per, double* out, double* ws, long ws_bytes, ud_stream_t stream) {
    if (!w || !g || !out || !shape_ok(N, per)) return UD_EINVAL;
    const long parts = dots_parts(per);
    if (parts > 2147483647L) return UD_EINVAL;
    if (parts > 1 && (!ws || ws_bytes < 3L * N * parts * (long)sizeof(double))) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* dst = parts > 1 ? ws : out;
    const dim3 grid((unsigned)parts, (unsigned)N);
    if (per % 4 == 0 && aligned16(w) && aligned16(g))
        hipLaunchKernelGGL(band_dots_parts<true>, grid, dim3(NT), 0, s, w, g, per, dst);
    else
        hipLaunchKernelGGL(band_dots_parts<false>, grid, dim3(NT), 0, s, w, g, per, dst);
    UD_LAUNCH_CHECK();
    if (parts > 1) {
        hipLaunchKernelGGL(band_dots_fold, dim3((unsigned)ud_cdiv(3L * N, 64)), dim3(64), 0, s, ws, N, parts, out);
        UD_LAUNCH_CHECK();
    }
    return 0;
}

int ud_band_update(float* w, const float* g, const double* dots, int N, long per, float step, float eps, ud_stream_t stream) {
    if (!w || !g || !dots || w == g || !shape_ok(N, per) || step != step || !(eps >= 0.f)) return UD_EINVAL;
    const long nvec = per % 4 == 0 && aligned16(w) && aligned16(g) ? per / 4 : 0;
    long bx = ew_blocks(nvec + (per - 4 * nvec));
    if (bx > 256) bx = 256;                                        // N rows of them: the grid-stride loop takes the rest
    hipLaunchKernelGGL(band_update, dim3((unsigned)bx, (unsigned)N), dim3(NT), 0, (hipStream_t)stream, w, g, dots, per, nvec,
                       (double)step, (double)eps);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

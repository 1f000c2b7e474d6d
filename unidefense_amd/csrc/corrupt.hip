// Common image corruptions on the device (unidefense_amd/corrupt.py): JPEG recompression, Gaussian blur, Gaussian noise,
// pixelation, contrast, saturation and masked 8x8 blocks, each ONE launch that reads the fp32 batch once and writes it once.
//
// Every corruption is defined on 8-bit grey levels, so every kernel has the same three stages:
//   (a) level_of: model units x in [-1, 1] (Normalize(0.5, 0.5)) -> u = clamp(floor((x + 1) 127.5 + 0.5), 0, 255) in fp32 with
//       contraction off; a NaN gives level 0;
//   (b) the corruption, on integers (int32; the bounds that keep it there are written at each product);
//   (c) out = lut[level]: a 256-entry fp32 table made by the host in float64 (level / 127.5 - 1).
// No floating-point operation decides an output bit after (a) — Gaussian noise's u + s z is the one exception and is two
// fp32 operations with contraction off — so tests/test_corrupt_cpu.py restates every kernel in numpy and the GPU tests compare
// bit for bit.  Ordinary vector loads and stores only, no atomics, nothing shared between workgroups: a replay gives the same bits.
#include "attack_common.h"
#include "levels.h"

namespace {

// ---- (a): level_of (levels.h), and the colour transforms ----------------------------------------------------------------------
// a value already in level units (noise): round half up, clamp, NaN -> 0
__device__ __forceinline__ int level_round(float v) {
#pragma clang fp contract(off)
    if (!(v == v)) return 0;
    float r = floorf(v + 0.5f);
    r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
    return (int)r;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// JFIF RGB -> YCbCr in Q16.  Every sum lies in [0, 255 * 65536 + 65535]: the results are levels without a clamp.
__device__ __forceinline__ int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }
// and back; >> of a negative sum is the arithmetic shift (floor)
__device__ __forceinline__ void ycc_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
    cb -= 128, cr -= 128;
    r = clamp255(y + ((91881 * cr + 32768) >> 16));
    g = clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    b = clamp255(y + ((116130 * cb + 32768) >> 16));
}

// ---- JPEG -------------------------------------------------------------------------------------------------------------------------
// T[k][n] = round(c_k cos((2n + 1) k pi / 16) 2^13), c_0 = sqrt(1/8), c_k = 1/2: the orthonormal 8-point DCT-II in Q13
__device__ constexpr int DCT_T[8][8] = {
    {2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
    {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
    {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
    {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// A workgroup owns a TILE x TILE pixel tile (4 x 4 MCUs of 16 x 16 in 4:2:0, 8 x 8 MCUs of 8 x 8 in 4:4:4).  Every 8 x 8 block
// lives in LDS as 8 rows of stride 9 (72 ints): with 8 threads per block (one per row or column) and consecutive blocks 72
// ints apart, the 32 lanes of a half wave fall on 32 different banks in the row passes and in the column passes alike.
// 4:2:0 keeps one ring of chroma blocks around the tile (6 x 6 instead of 4 x 4): the triangle up-sampling reads one chroma
// sample across each tile edge, and a chroma sample after the codec depends on its whole block, so the ring is recomputed here
// rather than exchanged with the neighbouring workgroup.
constexpr int TILE = 64, BLK = 72, YB = 64;

template <int SUB>
struct Geo {                                              // SUB = 2: 4:2:0, SUB = 1: 4:4:4
    static constexpr int RING = SUB == 2 ? 1 : 0;                     // chroma blocks recomputed around the tile
    static constexpr int CB = TILE / SUB / 8 + 2 * RING;              // chroma blocks per side: 6 or 8
    static constexpr int CS = CB * 8;                                 // chroma samples per side: 48 or 64
    static constexpr int NBLK = YB + 2 * CB * CB;                     // 136 or 192 blocks
};

// in-place 1-D transforms of one row (stride 1) or column (stride 9) of a block
// forward: o[k] = (sum_n T[k][n] v[n] + half) >> sh;  inverse: o[n] = (sum_k T[k][n] v[k] + half) >> sh
// __mul24 is exact: |T| <= 4017 < 2^12 and every |v| below is < 2^23
template <bool INV>
__device__ __forceinline__ void dct8(const int* v, int* o, int sh) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int s = 1 << (sh - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += __mul24(INV ? DCT_T[j][i] : DCT_T[i][j], v[j]);
        o[i] = s >> sh;
    }
}

template <int SUB>
__global__ __launch_bounds__(NT) void corrupt_jpeg(const float* __restrict__ x, float* __restrict__ out,
                                                   const float* __restrict__ lut, const int* __restrict__ qtab, int size,
                                                   int padded) {
    using G = Geo<SUB>;
    __shared__ int blk[G::NBLK * BLK];
    __shared__ int q[128];
    __shared__ float slut[256];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;         // the tile's origin, pixels
    const long plane = (long)size * size;
    const float* xs = x + (long)blockIdx.z * 3 * plane;
    float* os = out + (long)blockIdx.z * 3 * plane;
    if (tid < 128) q[tid] = qtab[tid];
    slut[tid] = lut[tid];
    const int pc = padded / SUB;                                      // the padded chroma plane's side

    // ---- load: one thread per chroma sample of the region; levels, colour transform, down-sampling, level shift -----------------
    for (int i = tid; i < G::CS * G::CS; i += NT) {
        const int ly = i / G::CS, lx = i % G::CS;                     // region-relative chroma sample
        const int cy = r0 / SUB + ly - 8 * G::RING, cx = c0 / SUB + lx - 8 * G::RING;     // in the padded chroma plane
        const bool in_plane = cy >= 0 && cy < pc && cx >= 0 && cx < pc;
        int scb = 0, scr = 0;
#pragma unroll
        for (int dy = 0; dy < SUB; ++dy) {
#pragma unroll
            for (int dx = 0; dx < SUB; ++dx) {
                const int py = cy * SUB + dy, px = cx * SUB + dx;     // padded pixel; the padding replicates the last row / column
                int r = 0, g = 0, b = 0;
                if (in_plane) {
                    const long p = (long)(py < size ? py : size - 1) * size + (px < size ? px : size - 1);
                    r = level_of(xs[p]), g = level_of(xs[p + plane]), b = level_of(xs[p + 2 * plane]);
                }
                scb += rgb_cb(r, g, b), scr += rgb_cr(r, g, b);
                const int ty = py - r0, tx = px - c0;                 // tile-relative: luma is kept for the tile only
                if (ty >= 0 && ty < TILE && tx >= 0 && tx < TILE)
                    blk[((ty >> 3) * 8 + (tx >> 3)) * BLK + (ty & 7) * 9 + (tx & 7)] = in_plane ? rgb_y(r, g, b) - 128 : 0;
            }
        }
        if (SUB == 2) scb = (scb + 2) >> 2, scr = (scr + 2) >> 2;
        const int o = ((ly >> 3) * G::CB + (lx >> 3)) * BLK + (ly & 7) * 9 + (lx & 7);
        blk[YB * BLK + o] = in_plane ? scb - 128 : 0;
        blk[(YB + G::CB * G::CB) * BLK + o] = in_plane ? scr - 128 : 0;
    }
    __syncthreads();

    // ---- the codec on every block: 8 threads per block, four in-place passes ---------------------------------------------------
    // bounds for any 8-bit input (|v| <= 128), with sum_n |T[k][n]| <= 8 * 4017 = 32136:
    //   forward columns  |sum| <= 32136 * 128   = 4.2e6,  >> 10 -> |tmp|  <= 4017   (Q3)
    //   forward rows     |sum| <= 32136 * 4017  = 1.3e8,  >> 13 -> |coef| <= 15759  (Q3: eight times the DCT coefficient)
    //   quantise q = sign(coef) (|coef| + 4 Q) / (8 Q)  (round half away), de-quantise r = q Q: |r| <= (15759 + 1020) / 8 = 2097
    //   inverse columns  |sum| <= 32136 * 2097  = 6.8e7,  >> 11 -> |tmp|  <= 32905  (Q2)
    //   inverse rows     |sum| <= 32136 * 32905 = 1.06e9 < 2^31, >> 15 -> the sample (Q0)
    constexpr int NVEC = G::NBLK * 8;
    for (int i = tid; i < NVEC; i += NT) {                            // forward, columns
        int* p = blk + (i >> 3) * BLK + (i & 7);
        int v[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[j * 9];
        dct8<false>(v, o, 10);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j * 9] = o[j];
    }
    __syncthreads();
    for (int i = tid; i < NVEC; i += NT) {                            // forward, rows; quantise and de-quantise row k
        const int b = i >> 3, k = i & 7;
        int* p = blk + b * BLK + k * 9;
        const int* qt = q + (b < YB ? 0 : 64) + k * 8;
        int v[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[j];
        dct8<false>(v, o, 13);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int Q = qt[j], a = o[j] < 0 ? -o[j] : o[j];
            const int m = (a + 4 * Q) / (8 * Q) * Q;
            p[j] = o[j] < 0 ? -m : m;
        }
    }
    __syncthreads();
    for (int i = tid; i < NVEC; i += NT) {                            // inverse, columns
        int* p = blk + (i >> 3) * BLK + (i & 7);
        int v[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[j * 9];
        dct8<true>(v, o, 11);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j * 9] = o[j];
    }
    __syncthreads();
    for (int i = tid; i < NVEC; i += NT) {                            // inverse, rows; level shift back, clamp
        int* p = blk + (i >> 3) * BLK + (i & 7) * 9;
        int v[8], o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[j];
        dct8<true>(v, o, 15);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = clamp255(o[j] + 128);
    }
    __syncthreads();

    // ---- store: one thread per pixel, rows coalesced; chroma up-sampling, colour transform back, table ------------------------
    const int* pcb = blk + YB * BLK;
    const int* pcr = blk + (YB + G::CB * G::CB) * BLK;
    // chroma sample (cy, cx) of the padded chroma plane, edges replicated, from the region's blocks
    auto chroma = [&](const int* pl, int cy, int cx) {
        cy = cy < 0 ? 0 : (cy > pc - 1 ? pc - 1 : cy);
        cx = cx < 0 ? 0 : (cx > pc - 1 ? pc - 1 : cx);
        const int ly = cy - r0 / SUB + 8 * G::RING, lx = cx - c0 / SUB + 8 * G::RING;
        return pl[((ly >> 3) * G::CB + (lx >> 3)) * BLK + (ly & 7) * 9 + (lx & 7)];
    };
    for (int i = tid; i < TILE * TILE; i += NT) {
        const int ty = i / TILE, tx = i % TILE, py = r0 + ty, px = c0 + tx;
        if (py >= size || px >= size) continue;                       // the crop
        const int yv = blk[((ty >> 3) * 8 + (tx >> 3)) * BLK + (ty & 7) * 9 + (tx & 7)];
        int cb, cr;
        if (SUB == 2) {
            // triangle filter: 3/4 of the nearer and 1/4 of the farther chroma sample in both directions; bias 8 on even
            // output columns and 7 on odd ones
            const int cy = py >> 1, cx = px >> 1;
            const int ny = (py & 1) ? cy + 1 : cy - 1, nx = (px & 1) ? cx + 1 : cx - 1;
            const int bias = (px & 1) ? 7 : 8;
            cb = (3 * (3 * chroma(pcb, cy, cx) + chroma(pcb, ny, cx)) + 3 * chroma(pcb, cy, nx) + chroma(pcb, ny, nx) + bias) >> 4;
            cr = (3 * (3 * chroma(pcr, cy, cx) + chroma(pcr, ny, cx)) + 3 * chroma(pcr, cy, nx) + chroma(pcr, ny, nx) + bias) >> 4;
        } else {
            cb = chroma(pcb, py, px), cr = chroma(pcr, py, px);
        }
        int r, g, b;
        ycc_rgb(yv, cb, cr, r, g, b);
        const long p = (long)py * size + px;
        os[p] = slut[r], os[p + plane] = slut[g], os[p + 2 * plane] = slut[b];
    }
}

// ---- Gaussian blur: separable, reflect-101, integer weights that sum to 2^14 -----------------------------------------------------
// A workgroup owns a BH x BW tile of one plane: the levels of the tile and its halo go to LDS, the horizontal pass stays in LDS,
// the vertical pass stores.  (sum w u + 2^13) >> 14 per pass: sum <= 255 * 2^14 + 2^13 < 2^23.
constexpr int BH = 32, BW = 64, BLUR_MAX_K = 31, BR = BLUR_MAX_K / 2;

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(NT) void corrupt_blur(const float* __restrict__ x, float* __restrict__ out,
                                                   const float* __restrict__ lut, const int* __restrict__ w, int size, int k,
                                                   int tiles_y) {
    __shared__ unsigned char raw[(BH + 2 * BR) * (BW + 2 * BR)];
    __shared__ unsigned char hor[(BH + 2 * BR) * BW];
    __shared__ int sw[BLUR_MAX_K];
    __shared__ float slut[256];
    const int tid = threadIdx.x, rad = k / 2;
    const int ch = blockIdx.y / tiles_y;                              // gridDim.y = 3 tiles_y, gridDim.z = N
    const int r0 = (blockIdx.y % tiles_y) * BH, c0 = blockIdx.x * BW;
    const long plane = (long)size * size;
    const float* xs = x + ((long)blockIdx.z * 3 + ch) * plane;
    float* os = out + ((long)blockIdx.z * 3 + ch) * plane;
    if (tid < k) sw[tid] = w[tid];
    slut[tid] = lut[tid];
    const int rows = BH + 2 * rad, cols = BW + 2 * rad;
    // rows and columns past the image's end are reflections of rows the tile never needs, but reflect101 keeps every index
    // inside [0, size) only for positions within rad of the image: clamp the position first
    for (int i = tid; i < rows * cols; i += NT) {
        const int ly = i / cols, lx = i % cols;
        int gy = r0 + ly - rad, gx = c0 + lx - rad;
        gy = gy > size - 1 + rad ? size - 1 + rad : gy;
        gx = gx > size - 1 + rad ? size - 1 + rad : gx;
        gy = reflect101(gy, size), gx = reflect101(gx, size);          // rad <= size - 1: one reflection lands inside
        raw[ly * cols + lx] = (unsigned char)level_of(xs[(long)gy * size + gx]);
    }
    __syncthreads();
    for (int i = tid; i < rows * BW; i += NT) {
        const int ly = i / BW, lx = i % BW;
        int s = 1 << 13;
        for (int j = 0; j < k; ++j) s += sw[j] * raw[ly * cols + lx + j];
        hor[ly * BW + lx] = (unsigned char)(s >> 14);
    }
    __syncthreads();
    for (int i = tid; i < BH * BW; i += NT) {
        const int ly = i / BW, lx = i % BW, py = r0 + ly, px = c0 + lx;
        if (py >= size || px >= size) continue;
        int s = 1 << 13;
        for (int j = 0; j < k; ++j) s += sw[j] * hor[(ly + j) * BW + lx];
        os[(long)py * size + px] = slut[s >> 14];
    }
}

// ---- point operations: contrast, saturation, Gaussian noise; one thread per pixel, all three channels --------------------------
__device__ __forceinline__ int scale_about_128(int u, int f8) { return clamp255(128 + (((u - 128) * f8 + 128) >> 8)); }

__global__ __launch_bounds__(NT) void corrupt_point(const float* __restrict__ x, float* __restrict__ out,
                                                    const float* __restrict__ lut, const float* __restrict__ z, int N, long plane,
                                                    int mode, int f8, float s) {
#pragma clang fp contract(off)
    const long total = (long)N * plane;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long p = (i / plane) * 3 * plane + i % plane;
        int r = level_of(x[p]), g = level_of(x[p + plane]), b = level_of(x[p + 2 * plane]);
        if (mode == UD_CORRUPT_CONTRAST) {
            r = scale_about_128(r, f8), g = scale_about_128(g, f8), b = scale_about_128(b, f8);
        } else if (mode == UD_CORRUPT_SATURATION) {
            const int y = rgb_y(r, g, b), cb = scale_about_128(rgb_cb(r, g, b), f8), cr = scale_about_128(rgb_cr(r, g, b), f8);
            ycc_rgb(y, cb, cr, r, g, b);
        } else {                                                      // noise: u + s z, one product and one sum in fp32
            r = level_round((float)r + s * z[p]);
            g = level_round((float)g + s * z[p + plane]);
            b = level_round((float)b + s * z[p + 2 * plane]);
        }
        out[p] = lut[r], out[p + plane] = lut[g], out[p + 2 * plane] = lut[b];
    }
}

// ---- pixelate: every f x f cell becomes its integer mean ---------------------------------------------------------------------
// A workgroup owns `cells` cells of one row of cells (cells f <= NT columns, one thread per column) and walks `bands` rows of
// cells: column sums over the cell's rows go to LDS, every thread adds its cell's column sums and stores the cell's rows.
constexpr int PIX_MAX_F = NT;                 // a cell's sum <= 255 * 256^2 < 2^24

__global__ __launch_bounds__(NT) void corrupt_pixelate(const float* __restrict__ x, float* __restrict__ out,
                                                       const float* __restrict__ lut, int size, int f, int cells, int bands,
                                                       int tiles_y) {
    __shared__ int colsum[NT];
    const int tid = threadIdx.x, width = cells * f;
    const int c = blockIdx.x * width + tid;                           // this thread's column
    const bool live = tid < width && c < size;
    const long plane = (long)size * size;
    const int ch = blockIdx.y / tiles_y;                              // gridDim.y = 3 tiles_y, gridDim.z = N
    const float* xs = x + ((long)blockIdx.z * 3 + ch) * plane;
    float* os = out + ((long)blockIdx.z * 3 + ch) * plane;
    for (int band = 0; band < bands; ++band) {
        const int y0 = ((blockIdx.y % tiles_y) * bands + band) * f;               // uniform over the workgroup
        if (y0 >= size) break;
        const int y1 = y0 + f < size ? y0 + f : size;
        int s = 0;
        if (live)
            for (int yy = y0; yy < y1; ++yy) s += level_of(xs[(long)yy * size + c]);
        colsum[tid] = s;
        __syncthreads();
        if (live) {
            const int t0 = tid / f * f;                               // the cell's first column, workgroup-relative
            int t1 = t0 + f;
            if (blockIdx.x * width + t1 > size) t1 = size - blockIdx.x * width;
            int sum = 0;
            for (int t = t0; t < t1; ++t) sum += colsum[t];
            const int cnt = (t1 - t0) * (y1 - y0);
            const float v = lut[(sum + cnt / 2) / cnt];
            for (int yy = y0; yy < y1; ++yy) os[(long)yy * size + c] = v;
        }
        __syncthreads();
    }
}

// ---- blocks: `count` 8 x 8 blocks per sample at level 128, clipped by the image ----------------------------------------------
constexpr int BLOCKS_MAX = 1024;

__global__ __launch_bounds__(NT) void corrupt_blocks(const float* __restrict__ x, float* __restrict__ out,
                                                     const float* __restrict__ lut, const int* __restrict__ pos, int size,
                                                     int count) {
    __shared__ int sy[BLOCKS_MAX], sx[BLOCKS_MAX];
    const int n = blockIdx.y;
    for (int j = threadIdx.x; j < count; j += NT) sy[j] = pos[((long)n * count + j) * 2], sx[j] = pos[((long)n * count + j) * 2 + 1];
    __syncthreads();
    const long plane = (long)size * size;
    const float grey = lut[128];
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < plane; i += (long)gridDim.x * NT) {
        const int py = (int)(i / size), px = (int)(i % size);
        bool hit = false;
        for (int j = 0; j < count; ++j) hit |= (unsigned)(py - sy[j]) < 8u && (unsigned)(px - sx[j]) < 8u;
        const long p = (long)n * 3 * plane + i;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[p + ch * plane] = hit ? grey : lut[level_of(x[p + ch * plane])];
    }
}

bool images_ok(const void* x, const void* out, const void* lut, int N, int size) {
    return x && out && lut && x != out && N >= 1 && N <= 65535 && size >= 1 && size <= 32768;
}

}  // namespace

extern "C" {

int ud_corrupt_jpeg(const float* x, float* out, const float* lut, const int* qtab, int N, int size, int quality, int subsampling,
                    ud_stream_t stream) {
    if (!images_ok(x, out, lut, N, size) || !qtab || quality < 1 || quality > 100) return UD_EINVAL;
    if (subsampling != UD_CORRUPT_JPEG_420 && subsampling != UD_CORRUPT_JPEG_444) return UD_EINVAL;
    const int mcu = subsampling == UD_CORRUPT_JPEG_420 ? 16 : 8;
    const int padded = (size + mcu - 1) / mcu * mcu;
    const dim3 grid((unsigned)ud_cdiv(padded, TILE), (unsigned)ud_cdiv(padded, TILE), (unsigned)N);
    if (subsampling == UD_CORRUPT_JPEG_420)
        hipLaunchKernelGGL(corrupt_jpeg<2>, grid, dim3(NT), 0, (hipStream_t)stream, x, out, lut, qtab, size, padded);
    else
        hipLaunchKernelGGL(corrupt_jpeg<1>, grid, dim3(NT), 0, (hipStream_t)stream, x, out, lut, qtab, size, padded);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_corrupt_blur(const float* x, float* out, const float* lut, const int* w, int N, int size, int k, ud_stream_t stream) {
    if (!images_ok(x, out, lut, N, size) || !w) return UD_EINVAL;
    if (k < 1 || k > BLUR_MAX_K || k % 2 == 0 || size < (k + 1) / 2) return UD_EINVAL;
    const int tiles_y = ud_cdiv(size, BH);
    const dim3 grid((unsigned)ud_cdiv(size, BW), (unsigned)(3 * tiles_y), (unsigned)N);
    hipLaunchKernelGGL(corrupt_blur, grid, dim3(NT), 0, (hipStream_t)stream, x, out, lut, w, size, k, tiles_y);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_corrupt_point(const float* x, float* out, const float* lut, const float* z, int N, int size, int mode, int f8, float s,
                     ud_stream_t stream) {
    if (!images_ok(x, out, lut, N, size)) return UD_EINVAL;
    if (mode == UD_CORRUPT_NOISE) {
        if (!z || !(s >= 0.f) || !(s <= 65536.f)) return UD_EINVAL;                 // !(s >= 0): a NaN too
    } else if (mode == UD_CORRUPT_CONTRAST || mode == UD_CORRUPT_SATURATION) {
        if (f8 < 0 || f8 > 65536) return UD_EINVAL;                                 // |(u - 128) f8| <= 2^23
    } else {
        return UD_EINVAL;
    }
    const long plane = (long)size * size;
    hipLaunchKernelGGL(corrupt_point, dim3((unsigned)ew_blocks((long)N * plane)), dim3(NT), 0, (hipStream_t)stream, x, out, lut, z,
                       N, plane, mode, f8, s);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_corrupt_pixelate(const float* x, float* out, const float* lut, int N, int size, int factor, ud_stream_t stream) {
    if (!images_ok(x, out, lut, N, size) || factor < 1 || factor > PIX_MAX_F) return UD_EINVAL;
    const int cells = NT / factor, bands = factor >= 16 ? 1 : 16 / factor;
    const int tiles_y = ud_cdiv(ud_cdiv(size, factor), bands);
    const dim3 grid((unsigned)ud_cdiv(size, cells * factor), (unsigned)(3 * tiles_y), (unsigned)N);
    hipLaunchKernelGGL(corrupt_pixelate, grid, dim3(NT), 0, (hipStream_t)stream, x, out, lut, size, factor, cells, bands, tiles_y);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_corrupt_blocks(const float* x, float* out, const float* lut, const int* pos, int N, int size, int count,
                      ud_stream_t stream) {
    if (!images_ok(x, out, lut, N, size) || count < 0 || count > BLOCKS_MAX || (count > 0 && !pos)) return UD_EINVAL;
    long bx = ((long)size * size + NT - 1) / NT;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(corrupt_blocks, dim3((unsigned)bx, (unsigned)N), dim3(NT), 0, (hipStream_t)stream, x, out, lut, pos, size,
                       count);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// Eval-mode MBConv: the expand conv computed inside the depthwise conv's staging (include/unidefense_hip.h, ud_mb_eval_dw).
//
// With BatchNorm on running statistics (the eval form of ud_bn_ref) BN0 is a fixed per-channel affine map, so the expanded
// tensor e = swish(bn0(x We^T)) of a block can be made tile by tile from the THIN block input and never written: a
// workgroup stages an 8 x TW output tile's input halo of x (all Ci channels, in chunks of KC) in LDS, forms e for its
// CC expanded channels over the halo, zero outside the image (the depthwise conv's SAME padding pads e), replaces the
// staged x by e, and runs the 3 x 3 depthwise conv with stride from LDS.  The result z = swish(bn1(dw)) is summed per
// (image, tile, channel) for the SE squeeze; `d` receives z (out_act = 1) or the raw depthwise output (out_act = 0: the
// form ud_pj_fwd_fused applies BN1 to on load).
//
// Precision: plain fp32 FMA.  e[p][c] = sum over ci = 0 .. Ci-1 in ascending order of x[p][ci] We[c][ci] (one fp32
// accumulator), then BN0 and swish in fp32 (accurate expf); dw[o][c] = sum over taps ky-major, kx ascending of
// e * w in fp32; each tile's pool partial is the sum of its outputs in row-major order, then of the 16 pixel groups
// in order.  No atomics: the result does not depend on scheduling.
#include "ud_common.h"

namespace {

constexpr int NT = 256;
constexpr int CC = 16;           // expanded channels per workgroup
constexpr int PG = NT / CC;      // pixel groups: thread t owns channel t % CC and pixels t / CC + k PG
constexpr int KC = 32;           // input channels staged per round
constexpr int KS = 3;            // depthwise kernel size
constexpr int TH = 8;            // output tile rows

struct EvalDwArgs {
    const float* x;       // [N][H][W][Ci]
    const float* we;      // [CE][Ci]
    const float* wt;      // [KS*KS][CE] tap-major
    float* d;             // [N][Ho][Wo][CE]
    float* part;          // [N][tiles][CE]
    ud_bn_ref bn0, bn1;
    int H, W, Ci, CE, Ho, Wo, pad_t, pad_l, tiles_x, tiles, out_act;
};

struct Affine { float mu, is, ga, be; };

__device__ __forceinline__ Affine affine_of(const ud_bn_ref& b, int c) {
    double m, v;
    ud_bn_moments(b, c, c, m, v);
    return Affine{(float)m, rsqrtf((float)(v + (double)b.eps)), b.gamma[c], b.beta[c]};
}

__device__ __forceinline__ float bn_swish(float a, const Affine& f) { return ud_swish(f.ga * ((a - f.mu) * f.is) + f.be); }

template <int S, int TW>
__global__ __launch_bounds__(NT) void mb_eval_dw_kernel(EvalDwArgs a) {
    constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS, P = IH * IW;
    constexpr int NA = (P + PG - 1) / PG;          // halo pixels per thread
    constexpr int NO = TH * TW / PG;               // output pixels per thread
    static_assert(KC >= CC, "the staged x chunk is reused for e");
    __shared__ __attribute__((aligned(16))) float xs[P * KC];
    __shared__ float red[PG][CC];

    const int tid = threadIdx.x, cl = tid % CC, pg = tid / CC;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int c = blockIdx.y * CC + cl;
    const int n = blockIdx.z;
    const int iy0 = ty * TH * S - a.pad_t, ix0 = tx * TW * S - a.pad_l;
    const float* xn = a.x + (long)n * a.H * a.W * a.Ci;

    // ---- expand conv over the halo: acc[k] = e (pre-BN0) of pixel pg + k PG, channel c
    float acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.f;
    for (int k0 = 0; k0 < a.Ci; k0 += KC) {
        const int kq = min(KC, a.Ci - k0) / 4;
        __syncthreads();                                   // the previous chunk's reads are done
        for (int i = tid; i < P * (KC / 4); i += NT) {
            const int p = i / (KC / 4), q = i % (KC / 4);
            const int iy = iy0 + p / IW, ix = ix0 + p % IW;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < kq && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v = *reinterpret_cast<const f32x4*>(xn + ((long)iy * a.W + ix) * a.Ci + k0 + 4 * q);
            reinterpret_cast<f32x4*>(xs)[i] = v;
        }
        f32x4 w[KC / 4];
        const f32x4* wr = reinterpret_cast<const f32x4*>(a.we + (long)c * a.Ci + k0);
#pragma unroll
        for (int q = 0; q < KC / 4; ++q) w[q] = q < kq ? wr[q] : f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int p = pg + k * PG;
            if (p < P) {
                const f32x4* xp = reinterpret_cast<const f32x4*>(xs + p * KC);
                float s = acc[k];
#pragma unroll
                for (int q = 0; q < KC / 4; ++q) {
                    const f32x4 v = xp[q];
                    s = fmaf(v[0], w[q][0], s);
                    s = fmaf(v[1], w[q][1], s);
                    s = fmaf(v[2], w[q][2], s);
                    s = fmaf(v[3], w[q][3], s);
                }
                acc[k] = s;
            }
        }
    }

    // ---- e = swish(bn0(.)) inside the image, 0 in the padding; replaces x in LDS as [P][CC]
    const Affine f0 = affine_of(a.bn0, c);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int p = pg + k * PG;
        if (p < P) {
            const int iy = iy0 + p / IW, ix = ix0 + p % IW;
            const bool in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            xs[p * CC + cl] = in ? bn_swish(acc[k], f0) : 0.f;
        }
    }
    __syncthreads();

    // ---- depthwise conv + swish(bn1(.)), the tile's pool partial
    float wk[KS * KS];
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) wk[t] = a.wt[(long)t * a.CE + c];
    const Affine f1 = affine_of(a.bn1, c);
    float ps = 0.f;
#pragma unroll
    for (int k = 0; k < NO; ++k) {
        const int o = pg + k * PG;
        const int oy = o / TW, ox = o % TW;
        float s = 0.f;
#pragma unroll
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) s = fmaf(xs[((oy * S + ky) * IW + ox * S + kx) * CC + cl], wk[ky * KS + kx], s);
        const int gy = ty * TH + oy, gx = tx * TW + ox;
        if (gy < a.Ho && gx < a.Wo) {
            const float z = bn_swish(s, f1);
            a.d[(((long)n * a.Ho + gy) * a.Wo + gx) * a.CE + c] = a.out_act ? z : s;
            ps += z;
        }
    }
    red[pg][cl] = ps;
    __syncthreads();
    if (tid < CC) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < PG; ++g) t += red[g][tid];
        a.part[((long)n * a.tiles + blockIdx.x) * a.CE + c] = t;
    }
}

int tile_w(int Wo, int stride) { return (stride == 1 && Wo >= 16) ? 16 : 8; }

template <int S, int TW>
int launch(const EvalDwArgs& a, int N, hipStream_t st) {
    hipLaunchKernelGGL((mb_eval_dw_kernel<S, TW>), dim3(a.tiles, a.CE / CC, N), dim3(NT), 0, st, a);
    return 0;
}

}  // namespace

extern "C" {

int ud_mb_eval_dw_ok(int Ci, int CE, int K, int stride) {
    return (Ci >= 4 && Ci % 4 == 0 && CE >= CC && CE % CC == 0 && K == KS && (stride == 1 || stride == 2)) ? 1 : 0;
}

long ud_mb_eval_dw_tiles(int Ho, int Wo, int stride) {
    if (Ho < 1 || Wo < 1 || (stride != 1 && stride != 2)) return UD_EINVAL;
    const int tw = tile_w(Wo, stride);
    return (long)ud_cdiv(Ho, TH) * ud_cdiv(Wo, tw);
}

int ud_mb_eval_dw(const float* x, const float* we, const ud_bn_ref* bn0, const float* wt, const ud_bn_ref* bn1, float* d, float* part,
                  int N, int H, int W, int Ci, int CE, int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int out_act,
                  ud_stream_t stream) {
    if (!x || !we || !wt || !d || !part || N < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || !ud_mb_eval_dw_ok(Ci, CE, K, stride))
        return UD_EINVAL;
    if (!ud_bn_eval_form(bn0) || !ud_bn_eval_form(bn1) || !bn0->gamma || !bn0->beta || !bn1->gamma || !bn1->beta) return UD_EINVAL;
    if (pad_t < 0 || pad_l < 0 || pad_t >= K || pad_l >= K) return UD_EINVAL;
    // every output reads inside the padded input: (Ho - 1) stride + K <= H + pad_t + (K - 1) and the same for W
    if ((long)(Ho - 1) * stride - pad_t > H - 1 || (long)(Wo - 1) * stride - pad_l > W - 1) return UD_EINVAL;
    if (((uintptr_t)x | (uintptr_t)we) & 15) return UD_EINVAL;
    EvalDwArgs a;
    a.x = x; a.we = we; a.wt = wt; a.d = d; a.part = part; a.bn0 = *bn0; a.bn1 = *bn1;
    a.H = H; a.W = W; a.Ci = Ci; a.CE = CE; a.Ho = Ho; a.Wo = Wo; a.pad_t = pad_t; a.pad_l = pad_l; a.out_act = out_act ? 1 : 0;
    const int tw = tile_w(Wo, stride);
    a.tiles_x = ud_cdiv(Wo, tw);
    a.tiles = (int)ud_mb_eval_dw_tiles(Ho, Wo, stride);
    hipStream_t st = (hipStream_t)stream;
    if (stride == 2) launch<2, 8>(a, N, st);
    else if (tw == 16) launch<1, 16>(a, N, st);
    else launch<1, 8>(a, N, st);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// ---- half storage: ud_mb_eval_dw_h ----------------------------------------------------------------------------------------
// The same node for the fp16 inference forward (include/unidefense_hip.h, ud_mb_eval_dw_h): x and d are _Float16 in memory,
// the expand conv runs on the matrix pipe.  Per workgroup (4 waves, CC = 16 expanded channels, the 8 x TW output tile of the
// fp32 kernel): the halo of x is staged in LDS as fp16 [pixel][KC] in chunks of KC = 32 input channels (zero beyond Ci and
// outside the image), the chunk of We [CC][KC] is rounded to fp16 as it is staged, and the halo pixels x CC channels product is
// v_mfma_f32_16x16x32_f16 with fp32 accumulation: A = 16 halo pixels x 32 input channels (lane l: pixel l & 15, channels
// 8 (l >> 4) .. + 7, one 16-byte LDS read), B = the same 32 channels x 16 expanded channels (lane l: channel l & 15), C: channel
// l & 15, pixels 4 (l >> 4) + r.  A wave owns pixel blocks w, w + 4, ...  Then swish(bn0(.)) in fp32 (0 in the SAME padding)
// into an fp32 LDS image [pixel][CC], the 3 x 3 depthwise conv and swish(bn1(.)) in fp32 as in the fp32 kernel, d stored as
// fp16 (activated, or raw for a consumer that applies BN1 + swish on load), and per (image, tile, channel) the sum of the
// values that consumer reads back — swish(bn1(.)) of the stored half value — for the SE squeeze.  No atomics.
namespace {

constexpr int HKC = 32;               // input channels per MFMA chunk (the k of one 16x16x32 product)
constexpr int HXS = HKC + 8;          // LDS row stride of the staged x (halves): 80 bytes, 16-byte aligned rows
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct EvalDwHArgs {
    const _Float16* x;    // [N][H][W][Ci]
    const float* we;      // [CE][Ci]
    const float* wt;      // [KS*KS][CE] tap-major
    _Float16* d;          // [N][Ho][Wo][CE]
    float* part;          // [N][tiles][CE]
    ud_bn_ref bn0, bn1;
    int H, W, Ci, CE, Ho, Wo, pad_t, pad_l, tiles_x, tiles, out_act;
};

template <int S, int TW>
__global__ __launch_bounds__(NT) void mb_eval_dw_h_kernel(EvalDwHArgs a) {
    constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS, P = IH * IW;
    constexpr int PB = (P + 15) / 16;              // 16-pixel blocks of the halo (the last one partly past P)
    constexpr int NW = NT / 64;
    constexpr int NB = (PB + NW - 1) / NW;         // blocks per wave
    constexpr int NO = TH * TW / PG;
    __shared__ __attribute__((aligned(16))) _Float16 xs[PB * 16 * HXS];
    __shared__ __attribute__((aligned(16))) _Float16 ws[CC * HXS];
    __shared__ float es[P * CC];
    __shared__ float red[PG][CC];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int c0 = blockIdx.y * CC;
    const int n = blockIdx.z;
    const int iy0 = ty * TH * S - a.pad_t, ix0 = tx * TW * S - a.pad_l;
    const _Float16* xn = a.x + (long)n * a.H * a.W * a.Ci;

    f32x4 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kq = lane >> 4, row = lane & 15;
    for (int k0 = 0; k0 < a.Ci; k0 += HKC) {
        __syncthreads();                                   // the previous chunk's reads are done
        for (int i = tid; i < PB * 16 * (HKC / 8); i += NT) {
            const int p = i / (HKC / 8), q = i % (HKC / 8);
            const int iy = iy0 + p / IW, ix = ix0 + p % IW;
            f16x8 v = {};
            if (p < P && k0 + 8 * q < a.Ci && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v = *reinterpret_cast<const f16x8*>(xn + ((long)iy * a.W + ix) * a.Ci + k0 + 8 * q);
            *reinterpret_cast<f16x8*>(xs + p * HXS + 8 * q) = v;
        }
        for (int i = tid; i < CC * HKC; i += NT) {
            const int cc = i / HKC, k = i % HKC;
            ws[cc * HXS + k] = (k0 + k < a.Ci) ? (_Float16)a.we[(long)(c0 + cc) * a.Ci + k0 + k] : (_Float16)0.f;
        }
        __syncthreads();
        const f16x8 b = *reinterpret_cast<const f16x8*>(ws + row * HXS + 8 * kq);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int blk = wave + j * NW;
            if (blk < PB) {
                const f16x8 av = *reinterpret_cast<const f16x8*>(xs + (blk * 16 + row) * HXS + 8 * kq);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, b, acc[j], 0, 0, 0);
            }
        }
    }

    // ---- e = swish(bn0(.)) inside the image, 0 in the padding: es [P][CC] fp32
    {
        const int cl = lane & 15;
        const Affine f0 = affine_of(a.bn0, c0 + cl);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int blk = wave + j * NW;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = blk * 16 + 4 * kq + r;
                if (blk < PB && p < P) {
                    const int iy = iy0 + p / IW, ix = ix0 + p % IW;
                    const bool in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                    es[p * CC + cl] = in ? bn_swish(acc[j][r], f0) : 0.f;
                }
            }
        }
    }
    __syncthreads();

    // ---- depthwise conv + swish(bn1(.)) from LDS, d in fp16, the tile's pool partial of what the consumer reads
    const int cl = tid % CC, pg = tid / CC, c = c0 + cl;
    float wk[KS * KS];
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) wk[t] = a.wt[(long)t * a.CE + c];
    const Affine f1 = affine_of(a.bn1, c);
    float ps = 0.f;
#pragma unroll
    for (int k = 0; k < NO; ++k) {
        const int o = pg + k * PG;
        const int oy = o / TW, ox = o % TW;
        float s = 0.f;
#pragma unroll
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) s = fmaf(es[((oy * S + ky) * IW + ox * S + kx) * CC + cl], wk[ky * KS + kx], s);
        const int gy = ty * TH + oy, gx = tx * TW + ox;
        if (gy < a.Ho && gx < a.Wo) {
            const _Float16 v = a.out_act ? (_Float16)bn_swish(s, f1) : (_Float16)s;
            a.d[(((long)n * a.Ho + gy) * a.Wo + gx) * a.CE + c] = v;
            ps += a.out_act ? (float)v : bn_swish((float)v, f1);
        }
    }
    red[pg][cl] = ps;
    __syncthreads();
    if (tid < CC) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < PG; ++g) t += red[g][tid];
        a.part[((long)n * a.tiles + blockIdx.x) * a.CE + c0 + tid] = t;
    }
}

template <int S, int TW>
int launch_h(const EvalDwHArgs& a, int N, hipStream_t st) {
    hipLaunchKernelGGL((mb_eval_dw_h_kernel<S, TW>), dim3(a.tiles, a.CE / CC, N), dim3(NT), 0, st, a);
    return 0;
}

}  // namespace

extern "C" {

int ud_mb_eval_dw_h_ok(int Ci, int CE, int K, int stride) {
    return (Ci >= 8 && Ci % 8 == 0 && CE >= CC && CE % CC == 0 && K == KS && (stride == 1 || stride == 2)) ? 1 : 0;
}

long ud_mb_eval_dw_h_tiles(int Ho, int Wo, int stride) { return ud_mb_eval_dw_tiles(Ho, Wo, stride); }

int ud_mb_eval_dw_h(const void* x, const float* we, const ud_bn_ref* bn0, const float* wt, const ud_bn_ref* bn1, void* d, float* part,
                    int N, int H, int W, int Ci, int CE, int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int out_act,
                    ud_stream_t stream) {
    if (!x || !we || !wt || !d || !part || N < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || !ud_mb_eval_dw_h_ok(Ci, CE, K, stride))
        return UD_EINVAL;
    if (!ud_bn_eval_form(bn0) || !ud_bn_eval_form(bn1) || !bn0->gamma || !bn0->beta || !bn1->gamma || !bn1->beta) return UD_EINVAL;
    if (pad_t < 0 || pad_l < 0 || pad_t >= K || pad_l >= K) return UD_EINVAL;
    if ((long)(Ho - 1) * stride - pad_t > H - 1 || (long)(Wo - 1) * stride - pad_l > W - 1) return UD_EINVAL;
    if ((uintptr_t)x & 15) return UD_EINVAL;
    EvalDwHArgs a;
    a.x = (const _Float16*)x; a.we = we; a.wt = wt; a.d = (_Float16*)d; a.part = part; a.bn0 = *bn0; a.bn1 = *bn1;
    a.H = H; a.W = W; a.Ci = Ci; a.CE = CE; a.Ho = Ho; a.Wo = Wo; a.pad_t = pad_t; a.pad_l = pad_l; a.out_act = out_act ? 1 : 0;
    const int tw = tile_w(Wo, stride);
    a.tiles_x = ud_cdiv(Wo, tw);
    a.tiles = (int)ud_mb_eval_dw_tiles(Ho, Wo, stride);
    hipStream_t st = (hipStream_t)stream;
    if (stride == 2) launch_h<2, 8>(a, N, st);
    else if (tw == 16) launch_h<1, 16>(a, N, st);
    else launch_h<1, 8>(a, N, st);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

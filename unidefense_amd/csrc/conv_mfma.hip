// Direct 3x3 convolution on the matrix pipe for the reconstruction decoder's 20/40/80/160-channel layers (model/unidefense.py:
// 59-102): forward, data gradient, the ConvTranspose2d(k3, s2) forward and its stride-2 data gradient.  Same operation and
// gather rule as ud_conv_small / ud_gemm a_mode 2:
//   y[m][co] = sum_{tap,ci} x[src(m, tap)][ci] * wmat[co][tap*CIN + ci]        m = (n, oh, ow), pixel-major fp32 tensors
//
// One workgroup (NW waves: 4, or 2 / 1 for the 16 x 16 layers so that their grid still has >= 256 workgroups) owns TH x TW
// output pixels of one image and all COUT.
//  * The input patch the tile needs is read from global memory ONCE (16-byte runs, predicated: out-of-image pixels and the
//    channel padding become zero rows in LDS), split ONCE into two fp16 pieces under a power-of-two scale taken from the patch's
//    own |x|max (a per-tile scale is a per-row scale of the GEMM), and stays in LDS for all nine taps.
//  * The weights stream through LDS in stages of TS taps x CK input channels, split the same way while they are staged; the
//    stage's scale follows the stage's |w|max, and when it has to move the accumulators are multiplied by the ratio, a power of
//    two, so one accumulator set serves all stages exactly.  Limits of a shared scale: inside a stage a weight keeps both
//    pieces down to 2^-17 of the stage's |w|max and is gone 2^-39 below it; across stages the scale rises at most 2^80 above
//    the smallest one used.  Only an output pixel that sees none of the larger weights (zero padding) could tell.
//  * Arithmetic: three v_mfma_f32_16x16x32_f16 per k-step (lo.hi, hi.lo, hi.hi) into fp32 accumulators — gemm_p3's PREC-2 idea
//    with the residual piece kept unscaled: with |max| scaled into [2^14, 2^15) an element's two pieces carry it to
//    max(2^-23 |v|, 2^-25), the dropped lo.lo product is 2^-22 relative.
//  * The reduction index is a list of 8-channel chunks (tap, c8); a k-step takes four of them, one per 16-lane group, so CIN only
//    pads to 8 and a stage pads to 32 with zero weight columns.
//  * Weights are the MFMA's A operand (rows = output channels), pixels its B operand: a lane ends up with 4 consecutive output
//    channels of one pixel and stores them as one 16-byte run.
//  * Transposed stride 2: the tile's pixels are ordered by output parity, every 16-pixel MFMA block has one parity, and a block
//    runs only the taps valid for it (1, 2, 2 or 4 of the 9): the zero taps are never multiplied.
// No atomics, no inter-workgroup waits, barriers only in uniform control flow, LDS <= 64 KiB (two workgroups per CU).
#include "pw_common.h"

namespace {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));


// a row of `bytes` (a multiple of 16) padded to an odd number of 16-byte slots: 16 consecutive rows then start in 16 different
// slots of the 64 banks
constexpr int odd_slots(int bytes) { return (bytes / 16) % 2 == 0 ? bytes + 16 : bytes; }
constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// MODE 0: stride 1 pad 1 ("same"); 1: transposed stride 2 pad 1 (Hout = 2 Hin); 2: stride 2 pad 1 (Hin = 2 Hout)
template <int CIN_, int COUT_, int MODE_, int TH_, int TW_, int CK_, int TS_, int NW_ = 4>
struct Cfg {
    static constexpr int CIN = CIN_, COUT = COUT_, MODE = MODE_, TH = TH_, TW = TW_, CK = CK_, TS = TS_, NW = NW_, NT = 64 * NW_;
    static constexpr int CINP = round_up(CIN, 8), COUTP = round_up(COUT, 16), NTL = COUTP / 16;
    static constexpr int PIX = TH * TW, MW = PIX / 16 / NW;                 // 16-pixel blocks per wave
    static constexpr int PH = MODE == 0 ? TH + 2 : MODE == 1 ? TH / 2 + 1 : 2 * TH + 1;
    static constexpr int PW = MODE == 0 ? TW + 2 : MODE == 1 ? TW / 2 + 1 : 2 * TW + 1;
    static constexpr int PROW = odd_slots(CINP * 2), PPLANE = PH * PW * PROW;          // bytes: one patch pixel, one piece plane
    static constexpr int NCC = CIN / CK, NSTAGE = (9 / TS) * NCC;
    static constexpr int CPT = round_up(CK, 8) / 8, NCH = TS * CPT;                     // 8-channel chunks per tap, per stage
    static constexpr int KSTEPS = (NCH + 3) / 4, KSP = KSTEPS * 32;
    static constexpr int WROW = odd_slots(KSP * 2), WPLANE = COUTP * WROW;
    static constexpr int LDS = 2 * PPLANE + 2 * WPLANE;
    static_assert(PIX % (16 * NW) == 0, "whole 16-pixel blocks for every wave");
    static_assert(CIN % 4 == 0 && COUT % 4 == 0 && CK % 4 == 0, "16-byte runs");
    static_assert(CIN % CK == 0 && (NCC == 1 || CK % 8 == 0) && 9 % TS == 0, "stages tile the reduction");
    static_assert(MODE != 1 || (TS == 1 && TH % 2 == 0 && TW % 2 == 0 && (PIX / 4) % 16 == 0), "one parity per 16-pixel block");
    static_assert(LDS + 64 <= 65536, "two workgroups per CU");
};

__device__ __forceinline__ float absmax4(float m, const f32x4& v) {
    return fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
}
// a quad of floats times s -> its two fp16 pieces, 8 bytes each, at dst and dst + plane
__device__ __forceinline__ void store_split4h(char* dst, int plane, const f32x4& v, float s) {
    uint32_t hi[2], lo[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float a = v[2 * h] * s, b = v[2 * h + 1] * s;
        const f16x2 p = {(_Float16)a, (_Float16)b};
        const f16x2 q = {(_Float16)(a - (float)p[0]), (_Float16)(b - (float)p[1])};
        hi[h] = __builtin_bit_cast(uint32_t, p);
        lo[h] = __builtin_bit_cast(uint32_t, q);
    }
    *reinterpret_cast<u32x2*>(dst) = u32x2{hi[0], hi[1]};
    *reinterpret_cast<u32x2*>(dst + plane) = u32x2{lo[0], lo[1]};
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }          // -126 <= e <= 127

template <class C>
__global__ __launch_bounds__(C::NT) void conv_mfma(ud_conv_geom g, const float* __restrict__ x, const float* __restrict__ wmat,
                                                float* __restrict__ y, int tiles_x, int tiles_y) {
    constexpr int CIN = C::CIN, COUT = C::COUT, MODE = C::MODE, TH = C::TH, TW = C::TW, CK = C::CK, TS = C::TS;
    constexpr int PW = C::PW, PROW = C::PROW, PPLANE = C::PPLANE, WROW = C::WROW, WPLANE = C::WPLANE;
    constexpr int NT = C::NT, NW = C::NW;
    constexpr int NTL = C::NTL, MW = C::MW, NCH = C::NCH, CPT = C::CPT, KSTEPS = C::KSTEPS, K = 9 * CIN;
    __shared__ __attribute__((aligned(16))) char sm[C::LDS];
    __shared__ float sred[2][4];
    char* const patch = sm;
    char* const ws = sm + 2 * PPLANE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, pl = lane & 15, grp = lane >> 4;
    int b = blockIdx.x;
    const int tile_x = b % tiles_x;
    b /= tiles_x;
    const int tile_y = b % tiles_y, n = b / tiles_y;
    const int oh0 = tile_y * TH, ow0 = tile_x * TW;
    const int ih0 = MODE == 0 ? oh0 - 1 : MODE == 1 ? oh0 / 2 : 2 * oh0 - 1;
    const int iw0 = MODE == 0 ? ow0 - 1 : MODE == 1 ? ow0 / 2 : 2 * ow0 - 1;

    // ---- the stage's weights, global -> registers: rows COUTP x (KSP / 4) quads; padding rows / chunks / channels are zeros
    constexpr int WQ = C::KSP / 4, WITEMS = C::COUTP * WQ, NWI = (WITEMS + NT - 1) / NT;
    f32x4 wr[NWI];
    auto wload = [&](int stage) {
        const int tap0 = (stage / C::NCC) * TS, c0 = (stage % C::NCC) * CK;
#pragma unroll
        for (int j = 0; j < NWI; ++j) {
            const int i = t + j * NT;
            const int co = i / WQ, c4 = i - co * WQ;
            const int q = c4 >> 1, tl = q / CPT, cl = (q - tl * CPT) * 8 + (c4 & 1) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (i < WITEMS && co < COUT && q < NCH && cl < CK)
                v = *reinterpret_cast<const f32x4*>(wmat + (long)co * K + (tap0 + tl) * CIN + c0 + cl);
            wr[j] = v;
        }
    };
    wload(0);

    // ---- the input patch: global -> registers -> |x|max -> scale -> two fp16 pieces in LDS
    float sx, inv_sx;
    {
        constexpr int CQ = C::CINP / 4, PITEMS = C::PH * PW * CQ, NPI = (PITEMS + NT - 1) / NT;
        f32x4 pv[NPI];
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < NPI; ++j) {
            const int i = t + j * NT;
            const int pix = i / CQ, c4 = i - pix * CQ;
            const int py = pix / PW, px = pix - py * PW;
            const int ih = ih0 + py, iw = iw0 + px;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (i < PITEMS && c4 * 4 < CIN && ih >= 0 && ih < g.Hin && iw >= 0 && iw < g.Win)
                v = *reinterpret_cast<const f32x4*>(x + (((long)n * g.Hin + ih) * g.Win + iw) * CIN + c4 * 4);
            pv[j] = v;
            mx = absmax4(mx, v);
        }
        mx = ud_wave_max(mx);
        if (lane == 0) sred[1][wave] = mx;
        __syncthreads();
        mx = sred[1][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) mx = fmaxf(mx, sred[1][w]);
        ud_h2_scale(__float_as_uint(mx), sx, inv_sx);
#pragma unroll
        for (int j = 0; j < NPI; ++j) {
            const int i = t + j * NT;
            const int pix = i / CQ, c4 = i - pix * CQ;
            if (i < PITEMS) store_split4h(patch + pix * PROW + c4 * 8, PPLANE, pv[j], sx);
        }
    }

    // ---- this lane's pixel in each of the wave's 16-pixel blocks
    int ty[MW], tx[MW];
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) {
        const int p = (wave + NW * mi) * 16 + pl;
        if (MODE == 1) {
            constexpr int PC = C::PIX / 4, HW = TW / 2;          // pixels per parity class, class row length
            const int cls = p / PC, r = p - cls * PC;
            ty[mi] = 2 * (r / HW) + (cls >> 1);
            tx[mi] = 2 * (r % HW) + (cls & 1);
        } else {
            ty[mi] = p / TW;
            tx[mi] = p % TW;
        }
    }

    f32x4 acc[MW][NTL];
#pragma unroll
    for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) acc[mi][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // weight scale 2^swe; smin: the smallest exponent used so far.  A later stage may scale up to 2^80 above it: what was
    // accumulated under smin is below 2^15 2^15 K < 2^42 and stays below 2^122.
    int swe = 0, smin = 0;
    bool have = false;
#pragma unroll 1
    for (int stage = 0; stage < C::NSTAGE; ++stage) {
        const int tap0 = (stage / C::NCC) * TS, c0 = (stage % C::NCC) * CK;
        float mw = 0.f;
#pragma unroll
        for (int j = 0; j < NWI; ++j) mw = absmax4(mw, wr[j]);
        mw = ud_wave_max(mw);
        if (lane == 0) sred[stage & 1][wave] = mw;
        __syncthreads();          // the stage's |w|max is complete, and every wave is done reading the previous stage's weights
        mw = sred[stage & 1][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) mw = fmaxf(mw, sred[stage & 1][w]);
        int ratio_e = 0;
        {
            const uint32_t bits = __float_as_uint(mw);
            const int ef = (int)(bits >> 23) & 0xff;
            if (ef != 0) {          // (all-zero or subnormal-only stage: keep the scale)
                int want = 14 - (ef - 127);          // takes |w|max into [2^14, 2^15)
                want = want < -100 ? -100 : want > 100 ? 100 : want;
                if (!have) {
                    swe = smin = want;
                    have = true;
                } else {
                    const int top = ef - 127 + swe;          // exponent of the scaled |w|max under the current scale
                    if (top > 14 || top < 4) {
                        const int ne = want < smin + 80 ? want : smin + 80;
                        ratio_e = ne - swe;
                        swe = ne;
                        smin = ne < smin ? ne : smin;
                    }
                }
            }
        }
        const float sw = pow2f(swe);
#pragma unroll
        for (int j = 0; j < NWI; ++j) {
            const int i = t + j * NT;
            const int co = i / WQ, c4 = i - co * WQ;
            if (i < WITEMS) store_split4h(ws + co * WROW + c4 * 8, WPLANE, wr[j], sw);
        }
        if (stage + 1 < C::NSTAGE) wload(stage + 1);          // in flight during this stage's MFMAs
        __syncthreads();
        if (ratio_e != 0) {
            const float ratio = pow2f(ratio_e < -126 ? -126 : ratio_e);
#pragma unroll
            for (int mi = 0; mi < MW; ++mi)
#pragma unroll
                for (int nt = 0; nt < NTL; ++nt) acc[mi][nt] *= ratio;
        }
        // transposed: a block of output parity (a, b) takes tap (kh, kw) only if kh = a + 1 and kw = b + 1 (mod 2)
        bool act[MW];
        bool any = false;
#pragma unroll
        for (int mi = 0; mi < MW; ++mi) {
            act[mi] = true;
            if (MODE == 1) {
                const int cls = (wave + NW * mi) / (C::PIX / 64);          // 16-pixel blocks per parity class: PIX / 4 / 16
                const int kh = tap0 / 3, kw = tap0 - 3 * kh;
                act[mi] = ((kh & 1) != (cls >> 1)) && ((kw & 1) != (cls & 1));
            }
            any = any || act[mi];
        }
        if (!any) continue;          // wave-uniform; the barriers are above
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int q = ks * 4 + grp;
            f16x8 wf[NTL][2];
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) {
                const char* s = ws + (nt * 16 + pl) * WROW + q * 16;
                wf[nt][0] = *reinterpret_cast<const f16x8*>(s);
                wf[nt][1] = *reinterpret_cast<const f16x8*>(s + WPLANE);
            }
            const int qc = q < NCH ? q : NCH - 1;          // a padding chunk multiplies zero weights: read any real chunk
            const int tl = qc / CPT, c8 = qc - tl * CPT;
            const int tap = tap0 + tl, kh = tap / 3, kw = tap - 3 * kh;
            const int coff = (c0 + c8 * 8) * 2;
#pragma unroll
            for (int mi = 0; mi < MW; ++mi) {
                if (!act[mi]) continue;
                int py, px;
                if (MODE == 0) {
                    py = ty[mi] + kh;
                    px = tx[mi] + kw;
                } else if (MODE == 1) {
                    py = (ty[mi] + 1 - kh) >> 1;
                    px = (tx[mi] + 1 - kw) >> 1;
                } else {
                    py = 2 * ty[mi] + kh;
                    px = 2 * tx[mi] + kw;
                }
                const char* s = patch + (py * PW + px) * PROW + coff;
                const f16x8 xh = *reinterpret_cast<const f16x8*>(s);
                const f16x8 xl = *reinterpret_cast<const f16x8*>(s + PPLANE);
#pragma unroll
                for (int nt = 0; nt < NTL; ++nt) {
                    f32x4 c = acc[mi][nt];
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt][1], xh, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt][0], xl, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[nt][0], xh, c, 0, 0, 0);
                    acc[mi][nt] = c;
                }
            }
        }
    }

    // ---- results: lane (pl, grp) holds output channels nt*16 + 4 grp .. + 3 of its pixel
    const float inv_sw = pow2f(-swe);
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) {
        const int oh = oh0 + ty[mi], ow = ow0 + tx[mi];
        if (oh >= g.Hout || ow >= g.Wout) continue;
        float* dst = y + (((long)n * g.Hout + oh) * g.Wout + ow) * COUT;
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            const int co = nt * 16 + grp * 4;
            if (co < COUT) *reinterpret_cast<f32x4*>(dst + co) = acc[mi][nt] * inv_sw * inv_sx;
        }
    }
}

template <class C>
int launch(const ud_conv_geom& g, const float* x, const float* wmat, float* y, hipStream_t s) {
    const int tiles_x = ud_cdiv(g.Wout, C::TW), tiles_y = ud_cdiv(g.Hout, C::TH);
    const long blocks = (long)g.N * tiles_x * tiles_y;
    if (blocks > 0x7fffffffL) return UD_EINVAL;
    hipLaunchKernelGGL((conv_mfma<C>), dim3((unsigned)blocks), dim3(C::NT), 0, s, g, x, wmat, y, tiles_x, tiles_y);
    UD_LAUNCH_CHECK();
    return 0;
}


// ---- weight gradient of the same convs ---------------------------------------------------------------------------------------
//   out[ma][tap*CIN + ci] = sum_m a[m][ma] * x[src(m, tap)][ci],   m = (n, oh, ow) over g's output grid    (ud_gemm's b_mode 2)
// The reduction index is pixels: both MFMA operands want 8 consecutive pixels of one channel per lane, so the tile of `a` and
// the gathered patch are staged TRANSPOSED (channel-major rows of 8 pixels), the patch once per kw so that every tap's run of 8
// pixels (px = S tx + kw) is one aligned 16-byte row.  Tile = 4 x 8 output pixels = one 32-deep k-step; lane group g reads tile
// row g.  Arithmetic: pw_common.h's exact bf16 x 3 split and six v_mfma_f32_16x16x32_bf16 products — tiles of any magnitude add
// into one accumulator set with no scale to carry.  A workgroup walks tiles blockIdx.x, + gridDim.x, ..., keeps its MA x 9 CC
// block of the result in registers (grid.y splits the gathered channels into chunks of CC) and writes one partial; pw::fold_launch
// sums the partials in a fixed order: deterministic, no atomics, no zero fill.
template <int CIN_, int MA_, int MODE_, int CC_>
struct WCfg {
    static constexpr int CIN = CIN_, MA = MA_, MODE = MODE_, CC = CC_, S = MODE == 0 ? 1 : 2;
    static constexpr int PH = 3 * S + 3, PWP = 7 * S + 3;          // patch rows / columns of a 4 x 8 tile
    static constexpr int MAP = round_up(MA, 16), MT = MAP / 16, NY = CIN / CC;
    static constexpr int NC = 9 * CC, NTILES = round_up(NC, 16) / 16, NTW = (NTILES + 3) / 4;          // result columns, 16-wide, per wave
    static constexpr int AROW = 80, APLANE = MAP * AROW;          // 32 pixels x 2 bytes, padded to an odd number of 16-byte slots
    static constexpr int XPLANE = 3 * CC * PH * 16;               // [kw][ci][patch row][8 pixels]
    static constexpr int LDS = 3 * APLANE + 3 * XPLANE;
    static_assert(MODE == 0 || MODE == 2, "gathers of a plain conv: stride 1 or 2, pad 1");
    static_assert(CIN % CC == 0 && CC % 4 == 0 && MA % 4 == 0, "16-byte runs");
    static_assert(LDS <= 65536, "two workgroups per CU");
};

__device__ __forceinline__ void store_split4t(char* dst, int plane, int stride, const f32x4& v) {
    // four channels of one pixel -> their three bf16 pieces, one 2-byte store per (channel, piece) at dst + c stride + piece plane
    uint32_t p[2][3];
    pw::split2(v[0], v[1], p[0][0], p[0][1], p[0][2]);
    pw::split2(v[2], v[3], p[1][0], p[1][1], p[1][2]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t w = p[c >> 1][k];
            *reinterpret_cast<uint16_t*>(dst + c * stride + k * plane) = (uint16_t)((c & 1) ? (w >> 16) : (w & 0xffffu));
        }
}

template <class C>
__global__ __launch_bounds__(256) void conv_mfma_wgrad(ud_conv_geom g, const float* __restrict__ a, const float* __restrict__ x,
                                                       float* __restrict__ part, int tiles_x, int tiles_y, int ntiles) {
    constexpr int CIN = C::CIN, MA = C::MA, CC = C::CC, S = C::S, PH = C::PH, PWP = C::PWP, MT = C::MT, NTW = C::NTW;
    constexpr int AROW = C::AROW, APLANE = C::APLANE, XPLANE = C::XPLANE, NC = C::NC, K = 9 * CIN;
    __shared__ __attribute__((aligned(16))) char sm[C::LDS];
    char* const at = sm;
    char* const xs = sm + 3 * APLANE;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, pl = lane & 15, grp = lane >> 4;
    const int c0 = blockIdx.y * CC;
    f32x4 acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this lane's column of each of the wave's 16-wide result blocks: (tap, channel) -> the patch rows it reads
    int xoff[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        int c = (wave + 4 * j) * 16 + pl;
        c = c < NC ? c : NC - 1;          // padding columns compute a copy of the last one and are not stored
        const int tap = c / CC, ci = c - tap * CC, kh = tap / 3, kw = tap - 3 * kh;
        xoff[j] = ((kw * CC + ci) * PH + S * grp + kh) * 16;
    }
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int b = tile;
        const int tile_x = b % tiles_x;
        b /= tiles_x;
        const int tile_y = b % tiles_y, n = b / tiles_y;
        const int oh0 = tile_y * 4, ow0 = tile_x * 8, ih0 = S * oh0 - 1, iw0 = S * ow0 - 1;
        __syncthreads();          // the previous tile's fragments are read
        {
            constexpr int Q = C::MAP / 4, ITEMS = 32 * Q;
            for (int i = t; i < ITEMS; i += 256) {
                const int p = i / Q, c4 = i - p * Q;
                const int oh = oh0 + (p >> 3), ow = ow0 + (p & 7);
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (c4 * 4 < MA && oh < g.Hout && ow < g.Wout)
                    v = *reinterpret_cast<const f32x4*>(a + (((long)n * g.Hout + oh) * g.Wout + ow) * MA + c4 * 4);
                store_split4t(at + c4 * 4 * AROW + p * 2, APLANE, AROW, v);
            }
        }
        {
            constexpr int Q = CC / 4, ITEMS = PH * PWP * Q;
            for (int i = t; i < ITEMS; i += 256) {
                const int pix = i / Q, c4 = i - pix * Q;
                const int py = pix / PWP, px = pix - py * PWP;
                const int ih = ih0 + py, iw = iw0 + px;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ih >= 0 && ih < g.Hin && iw >= 0 && iw < g.Win)
                    v = *reinterpret_cast<const f32x4*>(x + (((long)n * g.Hin + ih) * g.Win + iw) * CIN + c0 + c4 * 4);
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int d = px - kw;
                    if (d >= 0 && d % S == 0 && d / S < 8)
                        store_split4t(xs + ((kw * CC + c4 * 4) * PH + py) * 16 + (d / S) * 2, XPLANE, PH * 16, v);
                }
            }
        }
        __syncthreads();
        pw::Frag3 af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const char* sp = at + (mt * 16 + pl) * AROW + grp * 16;
#pragma unroll
            for (int k = 0; k < 3; ++k) af[mt].p[k] = *reinterpret_cast<const pw::bf16x8*>(sp + k * APLANE);
        }
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            if ((wave + 4 * j) * 16 >= NC) continue;          // wave-uniform
            pw::Frag3 bf;
#pragma unroll
            for (int k = 0; k < 3; ++k) bf.p[k] = *reinterpret_cast<const pw::bf16x8*>(xs + xoff[j] + k * XPLANE);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt][j] = pw::mma6(af[mt], bf, acc[mt][j]);
        }
    }
    // lane (pl, grp) holds rows ma = 16 mt + 4 grp .. + 3 of column c = 16 (wave + 4 j) + pl
    float* dst = part + (long)blockIdx.x * MA * K;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int c = (wave + 4 * j) * 16 + pl;
        if (c >= NC) continue;
        const int tap = c / CC, ci = c - tap * CC;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ma = mt * 16 + grp * 4 + r;
                if (ma < MA) dst[(long)ma * K + tap * CIN + c0 + ci] = acc[mt][j][r];
            }
    }
}

// partials per launch: at least four tiles per workgroup, at most 512 workgroups, at most 6 M floats of partials
int wgrad_parts(long ntiles, int Cin, int Ma, int ny) {
    long cap = 6L * 1024 * 1024 / ((long)Ma * 9 * Cin);
    if (cap > 512 / ny) cap = 512 / ny;
    long p = ntiles / 4;
    if (p > cap) p = cap;
    return p < 1 ? 1 : (int)p;
}

template <class C>
int launch_wgrad(const ud_conv_geom& g, const float* a, const float* x, float* part, float* out, hipStream_t s) {
    const int tiles_x = ud_cdiv(g.Wout, 8), tiles_y = ud_cdiv(g.Hout, 4);
    const long ntiles = (long)g.N * tiles_x * tiles_y;
    if (ntiles > 0x7fffffffL) return UD_EINVAL;
    const int parts = wgrad_parts(ntiles, C::CIN, C::MA, C::NY);
    hipLaunchKernelGGL((conv_mfma_wgrad<C>), dim3((unsigned)parts, (unsigned)C::NY), dim3(256), 0, s, g, a, x, part, tiles_x, tiles_y,
                       (int)ntiles);
    UD_LAUNCH_CHECK();
    if (!out) return parts;          // the caller folds the partials later (ud_param_fold_multi)
    return pw::fold_launch(part, parts, C::MA * 9 * C::CIN, out, nullptr, nullptr, 0, nullptr, nullptr, s);
}

// geometry class of g: 0 same, 1 transposed stride 2, 2 stride 2; -1 none of them
int mode_of(const ud_conv_geom& g) {
    if (g.KH != 3 || g.KW != 3 || g.pad_t != 1 || g.pad_l != 1) return -1;
    if (!g.transposed && g.stride == 1 && g.Hout == g.Hin && g.Wout == g.Win) return 0;
    if (g.transposed && g.stride == 2 && g.Hout == 2 * g.Hin && g.Wout == 2 * g.Win) return 1;
    if (!g.transposed && g.stride == 2 && g.Hin == 2 * g.Hout && g.Win == 2 * g.Wout) return 2;
    return -1;
}

}  // namespace

// (Cin, Cout, mode) -> tile and stage shape.  LDS per workgroup in the comments.
#define UD_CONV_MFMA_CASES(X)                                                                   \
    X(20, 20, 0, 16, 16, 20, 9, 4)  /* 59 KiB */                                                \
    X(40, 20, 0, 8, 16, 40, 3, 4)   /* 45 KiB */                                                \
    X(40, 40, 0, 8, 16, 40, 3, 4)   /* 54 KiB */                                                \
    X(20, 40, 0, 8, 16, 20, 9, 4)   /* 60 KiB */                                                \
    X(80, 40, 0, 8, 8, 80, 1, 4)    /* 54 KiB */                                                \
    X(80, 80, 0, 8, 8, 40, 1, 4)    /* 57 KiB */                                                \
    X(40, 80, 0, 8, 8, 40, 3, 4)    /* 58 KiB */                                                \
    X(160, 80, 0, 4, 8, 40, 1, 2)   /* 62 KiB; 16 x 16 layer: 32-pixel tiles, 256 workgroups at batch 32 */ \
    X(80, 160, 0, 4, 8, 16, 1, 2)   /* 46 KiB; 16 x 16 layer */                                 \
    X(20, 20, 1, 16, 16, 20, 1, 4)  /* 13 KiB */                                                \
    X(40, 40, 1, 16, 16, 40, 1, 4)  /* 26 KiB */                                                \
    X(80, 80, 1, 8, 16, 80, 1, 4)   /* 48 KiB */                                                \
    X(20, 20, 2, 8, 8, 20, 9, 4)    /* 56 KiB */                                                \
    X(40, 40, 2, 8, 8, 40, 1, 4)    /* 59 KiB */                                                \
    X(80, 80, 2, 4, 4, 40, 1, 1)    /* 50 KiB; 16 x 16 layer: 16-pixel tiles, 512 workgroups at batch 32 */

extern "C" {

// geometry class of g for ud_conv_mfma: 0 stride 1 pad 1 "same", 1 transposed stride 2 pad 1 with Hout = 2 Hin, 2 stride 2 pad 1
// with Hin = 2 Hout (3x3 windows); -1: none of them (or g == NULL)
int ud_conv_mfma_mode(const ud_conv_geom* g) { return g ? mode_of(*g) : -1; }

// 1 when ud_conv_mfma has a kernel for (Cin, Cout) under geometry class `mode` (0 stride 1 pad 1 "same", 1 transposed stride 2
// pad 1 with Hout = 2 Hin, 2 stride 2 pad 1 with Hin = 2 Hout), else 0
int ud_conv_mfma_supported(int Cin, int Cout, int mode) {
#define X(ci, co, m, th, tw, ck, ts, nw) \
    if (Cin == ci && Cout == co && mode == m) return 1;
    UD_CONV_MFMA_CASES(X)
#undef X
    return 0;
}

// y[N][Hout][Wout][Cout] = gather-conv(x[N][Hin][Win][Cin], wmat[Cout][9*Cin]) under geometry g; x, wmat, y 16-byte aligned
int ud_conv_mfma(const ud_conv_geom* g, const float* x, const float* wmat, float* y, int Cout, ud_stream_t stream) {
    if (!g || !x || !wmat || !y) return UD_EINVAL;
    const int mode = mode_of(*g);
    if (mode < 0 || !ud_conv_mfma_supported(g->Cin, Cout, mode)) return UD_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)wmat | (uintptr_t)y) & 15) != 0) return UD_EINVAL;
    if (g->N < 1 || g->Hout < 1 || g->Wout < 1) return 0;
    hipStream_t s = (hipStream_t)stream;
#define X(ci, co, m, th, tw, ck, ts, nw) \
    if (g->Cin == ci && Cout == co && mode == m) return launch<Cfg<ci, co, m, th, tw, ck, ts, nw>>(*g, x, wmat, y, s);
    UD_CONV_MFMA_CASES(X)
#undef X
    return UD_EINVAL;
}

// (gathered channels Cin, columns Ma of `a`, mode, channels per grid.y block): the decoder's conv weight gradients (mode 0: a = dy,
// x gathered) and its transposed convs' (mode 2: a = x, dy gathered at stride 2)
#define UD_CONV_MFMA_WGRAD_CASES(X) \
    X(160, 80, 0, 40) X(80, 80, 0, 40) X(80, 40, 0, 40) X(40, 40, 0, 40) X(40, 20, 0, 40) X(20, 20, 0, 20) \
    X(80, 80, 2, 20) X(40, 40, 2, 20) X(20, 20, 2, 20)

// 1 when ud_conv_mfma_wgrad has a kernel for gathering Cin channels against Ma columns of `a` under geometry class `mode` (0 or 2)
int ud_conv_mfma_wgrad_supported(int Cin, int Ma, int mode) {
#define X(ci, ma, m, cc) \
    if (Cin == ci && Ma == ma && mode == m) return 1;
    UD_CONV_MFMA_WGRAD_CASES(X)
#undef X
    return 0;
}

// floats of scratch `part` must hold (per-workgroup partial results), for any geometry
long ud_conv_mfma_wgrad_ws_floats(int Cin, int Ma) {
    if (Cin < 1 || Ma < 1) return UD_EINVAL;
    return (long)wgrad_parts(1L << 40, Cin, Ma, 1) * Ma * 9 * Cin;
}

// out[Ma][9*Cin] = sum over rows m = (n,oh,ow) of g's output grid of a[m][Ma] (x) patch(x)[m][9*Cin]; pointers 16-byte aligned
int ud_conv_mfma_wgrad(const ud_conv_geom* g, const float* a, const float* x, float* part, float* out, int Ma, ud_stream_t stream) {
    if (!g || !a || !x || !part) return UD_EINVAL;
    const int mode = mode_of(*g);
    if (mode < 0 || !ud_conv_mfma_wgrad_supported(g->Cin, Ma, mode)) return UD_EINVAL;
    if ((((uintptr_t)a | (uintptr_t)x) & 15) != 0) return UD_EINVAL;
    if (g->N < 1 || g->Hout < 1 || g->Wout < 1) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
#define X(ci, ma, m, cc) \
    if (g->Cin == ci && Ma == ma && mode == m) return launch_wgrad<WCfg<ci, ma, m, cc>>(*g, a, x, part, out, s);
    UD_CONV_MFMA_WGRAD_CASES(X)
#undef X
    return UD_EINVAL;
}

}  // extern "C"

// Gradient with respect to the input image (x.grad of model(x)): the data gradient of the stem convs, and the two small
// elementwise pieces of the attention's clean-input path (model/unidefense.py:130-157: |pred - x| in the spatial and the
// frequency domain, fed to the dynamic filters).
//
// Stem data gradient.  The stem convs read 3 input channels with a k x k window at stride 2 (EfficientNet-B4: 3x3, 48
// outputs, static SAME pads 0 / 1; ResNet-18 / 50: 7x7, 64 outputs, pad 3).  As a transposed conv over dy the gather GEMM
// has 3 output columns (a 32-wide MFMA tile is 90 % padding) and a zero-stuffed reduction.  Here one thread owns one input
// pixel and its 3 channels.  The input grid is split by phase, ((ih + pad_t) mod 2, (iw + pad_l) mod 2): only the taps
// kh = rh + 2 jh, kw = rw + 2 jw meet an output pixel, at (oh, ow) = (qh - jh, qw - jw) with ih + pad_t = 2 qh + rh.  Each
// workgroup takes one phase of one image, so its tap set (1 / 2 / 4 taps for 3x3, 9 / 12 / 16 for 7x7) is wave-uniform and
// the weights are wave-uniform scalar loads feeding the FMAs, as in conv_small.hip.  dy is read as float4 runs of Co
// channels; neighbouring lanes read neighbouring dy pixels, and the pixels one lane's taps share with its neighbours' come
// from L1 / L2.  The result is written straight into x's planes [N][3][H][W], optionally added to what is there (the
// attention's and the reconstruction losses' parts of dx).
#include "ud_common.h"

namespace {

constexpr int NT = 256;
constexpr int STRIDE = 2;

// first input row / column of phase r (ih + pad = 2 q + r) and how many the phase holds in [0, n)
__device__ __forceinline__ void phase_range(int n, int pad, int r, int& first, int& count) {
    first = ((r - pad) % STRIDE + STRIDE) % STRIDE;
    count = first < n ? (n - 1 - first) / STRIDE + 1 : 0;
}

template <int KS, int CO>
__global__ __launch_bounds__(NT) void stem_dgrad(ud_conv_geom g, const float* __restrict__ dy, const float* __restrict__ w,
                                                  float* __restrict__ dx, int accumulate) {
    static_assert(CO % 4 == 0, "dy is read in channel quads");
    constexpr int KK = KS * KS;
    const int ph = blockIdx.y & 3;
    const int n = blockIdx.y >> 2;
    const int rh = ph >> 1, rw = ph & 1;
    int ih0, nqh, iw0, nqw;
    phase_range(g.Hin, g.pad_t, rh, ih0, nqh);
    phase_range(g.Win, g.pad_l, rw, iw0, nqw);
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= (long)nqh * nqw) return;
    const int ih = ih0 + STRIDE * (int)(i / nqw);
    const int iw = iw0 + STRIDE * (int)(i % nqw);
    const int qh = (ih + g.pad_t - rh) / STRIDE, qw = (iw + g.pad_l - rw) / STRIDE;
    const int nth = (KS - rh + 1) / STRIDE, ntw = (KS - rw + 1) / STRIDE;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 1
    for (int jh = 0; jh < nth; ++jh) {
        const int oh = qh - jh;
        if (oh < 0 || oh >= g.Hout) continue;
        const int kh = rh + STRIDE * jh;
#pragma unroll 1
        for (int jw = 0; jw < ntw; ++jw) {
            const int ow = qw - jw;
            if (ow < 0 || ow >= g.Wout) continue;
            const int kw = rw + STRIDE * jw;
            const f32x4* src = reinterpret_cast<const f32x4*>(dy + (((long)n * g.Hout + oh) * g.Wout + ow) * CO);
            const float* wt = w + kh * KS + kw;            // w[co][ci][kh][kw] = wt[(3 co + ci) KK]: wave-uniform
#pragma unroll
            for (int c = 0; c < CO / 4; ++c) {
                const f32x4 v = src[c];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int co = 4 * c + e;
                    a0 = fmaf(v[e], wt[(3 * co + 0) * KK], a0);
                    a1 = fmaf(v[e], wt[(3 * co + 1) * KK], a1);
                    a2 = fmaf(v[e], wt[(3 * co + 2) * KK], a2);
                }
            }
        }
    }
    const long plane = (long)g.Hin * g.Win;
    float* dst = dx + (long)n * 3 * plane + (long)ih * g.Win + iw;
    if (accumulate) {
        a0 += dst[0];
        a1 += dst[plane];
        a2 += dst[2 * plane];
    }
    dst[0] = a0;
    dst[plane] = a1;
    dst[2 * plane] = a2;
}

template <int KS, int CO>
int launch_stem(const ud_conv_geom& g, const float* dy, const float* w, float* dx, int accumulate, hipStream_t s) {
    const long per_phase = (long)((g.Hin + 1) / STRIDE) * ((g.Win + 1) / STRIDE);     // the largest phase
    hipLaunchKernelGGL((stem_dgrad<KS, CO>), dim3((unsigned)ud_cdiv(per_phase, NT), (unsigned)(4 * g.N)), dim3(NT), 0, s, g, dy,
                       w, dx, accumulate);
    UD_LAUNCH_CHECK();
    return 0;
}

inline int ew_blocks(long total) {
    long b = (total + NT - 1) / NT;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

// da = sign(a - b) g, db = -sign(a - b) g (sign(0) = 0, as torch.abs's gradient); either output may be NULL
__global__ __launch_bounds__(NT) void absdiff_bwd(long total, const float* __restrict__ a, const float* __restrict__ b,
                                                   const float* __restrict__ g, float* __restrict__ da,
                                                   float* __restrict__ db) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const float d = a[i] - b[i];
        const float s = d > 0.f ? g[i] : (d < 0.f ? -g[i] : 0.f);
        if (da) da[i] = s;
        if (db) db[i] = -s;
    }
}

// out[m][j] = u[m] v[j]
__global__ __launch_bounds__(NT) void outer(long total, int D, const float* __restrict__ u, const float* __restrict__ v,
                                             float* __restrict__ out) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long m = i / D;
        out[i] = u[m] * v[i - m * D];
    }
}

}  // namespace

extern "C" {

// 1 when ud_stem_dgrad has a kernel for this conv, else 0
int ud_stem_dgrad_supported(int Cin, int Cout, int KH, int KW, int stride) {
    if (Cin != 3 || stride != STRIDE || KH != KW) return 0;
    return (KH == 3 && Cout == 48) || (KH == 7 && Cout == 64) ? 1 : 0;
}

// dx[N][3][Hin][Win] (+)= data gradient of the conv g (F.conv2d geometry) given dy[N][Hout][Wout][Cout] and the module
// weight w[Cout][3][KH][KW]
int ud_stem_dgrad(const ud_conv_geom* g, const float* dy, const float* w, float* dx, int Cout, int accumulate,
                  ud_stream_t stream) {
    if (!g || !ud_stem_dgrad_supported(g->Cin, Cout, g->KH, g->KW, g->stride) || g->transposed) return UD_EINVAL;
    if (g->pad_t < 0 || g->pad_l < 0 || g->pad_t >= g->KH || g->pad_l >= g->KW) return UD_EINVAL;
    if (g->N < 1 || g->N > 16383 || g->Hin < 1 || g->Win < 1 || g->Hout < 1 || g->Wout < 1) return UD_EINVAL;
    if (!dy || !w || !dx) return UD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (g->KH == 3) return launch_stem<3, 48>(*g, dy, w, dx, accumulate, s);
    return launch_stem<7, 64>(*g, dy, w, dx, accumulate, s);
}

int ud_absdiff_bwd(const float* a, const float* b, const float* g, float* da, float* db, long total, ud_stream_t stream) {
    if (total < 0 || !a || !b || !g || (!da && !db)) return UD_EINVAL;
    if (total == 0) return 0;
    hipLaunchKernelGGL(absdiff_bwd, dim3(ew_blocks(total)), dim3(NT), 0, (hipStream_t)stream, total, a, b, g, da, db);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_outer(const float* u, const float* v, float* out, long M, int D, ud_stream_t stream) {
    if (M < 0 || D < 1 || !u || !v || !out) return UD_EINVAL;
    if (M == 0) return 0;
    hipLaunchKernelGGL(outer, dim3(ew_blocks(M * D)), dim3(NT), 0, (hipStream_t)stream, M * D, D, u, v, out);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

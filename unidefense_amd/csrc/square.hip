// Square attack, L-infinity (unidefense_amd/attack.py: SquareRunner): a score-based black-box search that needs the forward
// only.  As in csrc/apgd.hip everything that depends on the data — which samples are still searched, whether the last proposal
// is kept or undone, where the next square goes — is device state and device tables read by these two kernels, so one
// iteration is a static sequence of launches inside a captured graph with no host round trip.
//
// ud_square_control is one thread per sample: the iteration index is a per-sample counter that the thread itself increments.
// ud_square_propose settles the previous proposal's window and writes the next one in one launch: every element of the union
// of the two windows is owned by exactly one thread, which forms the settled value and then stores x_best and x_try, so
// identical, overlapping and disjoint consecutive windows need no ordering between threads.  Ordinary vector stores only, no
// atomics, nothing shared between threads, NaN-transparent clamps — a replay gives the same bits.  Only the windows' bytes
// are touched: at most 2 (s'^2 + s^2) 3 N 4 bytes of reads and as many of writes.
#include "attack_common.h"

namespace {

constexpr int MAX_BLOCKS_X = 64;      // per sample; the threads stride over the windows' elements

struct Window {               // rows [h, h + s) x columns [w, w + s); s == 0: none
    int s, h, w;
    __device__ __forceinline__ bool has(int r, int c) const { return s && r >= h && r < h + s && c >= w && c < w + s; }
};

// row `row` of the draw tables for sample n; a row that would leave the image is no window at all
__device__ __forceinline__ Window load_window(const int* __restrict__ side, const int* __restrict__ dh,
                                              const int* __restrict__ dw, long row, int N, int n, int size) {
    Window q;
    q.s = side[row];
    q.h = dh[row * N + n];
    q.w = dw[row * N + n];
    if (q.s < 1 || q.s > size || q.h < 0 || q.h > size - q.s || q.w < 0 || q.w > size - q.s) q.s = 0;
    return q;
}

// ---- propose: resolve proposal k - 1, write proposal k -------------------------------------------------------------------
__global__ __launch_bounds__(NT) void square_propose(float* __restrict__ x_try, float* __restrict__ x_best,
                                                     const float* __restrict__ x0, const int* __restrict__ ist,
                                                     const int* __restrict__ side, const int* __restrict__ dh,
                                                     const int* __restrict__ dw, const float* __restrict__ dsign, int N,
                                                     int size, int steps, float eps, float lo, float hi, int closing) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const int k = ist[(long)UD_SQUARE_I_K * N + n];
    Window prev{0, 0, 0}, next{0, 0, 0};
    int accepted = 0;
    float inc[3] = {0.f, 0.f, 0.f};
    if (k >= 2 && k <= steps + 1) {
        prev = load_window(side, dh, dw, k - 2, N, n, size);
        accepted = ist[(long)UD_SQUARE_I_ACCEPTED * N + n];
    }
    if (!closing && k >= 1 && k <= steps) {
        next = load_window(side, dh, dw, k - 1, N, n, size);
        const float* sg = dsign + ((long)(k - 1) * N + n) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) inc[c] = sg[c] * eps;             // +-eps exactly
    }
    const long a_prev = (long)prev.s * prev.s, total = a_prev + (long)next.s * next.s;
    const long plane = (long)size * size;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        int r, c;
        bool in_prev, in_next;
        if (i < a_prev) {                                             // an element of W': this thread owns it
            r = prev.h + (int)(i / prev.s), c = prev.w + (int)(i % prev.s);
            in_prev = true, in_next = next.has(r, c);
        } else {                                                      // an element of W: owned here unless W' holds it too
            const long j = i - a_prev;
            r = next.h + (int)(j / next.s), c = next.w + (int)(j % next.s);
            if (prev.has(r, c)) continue;
            in_prev = false, in_next = true;
        }
        const long p0 = (long)n * 3 * plane + (long)r * size + c;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long p = p0 + ch * plane;
            if (in_prev) {
                if (accepted) {
                    x_best[p] = x_try[p];                             // kept: x_try holds the settled value already
                } else if (!in_next) {
                    x_try[p] = x_best[p];                             // undone
                }
            }
            if (in_next) x_try[p] = clampf(x0[p] + inc[ch], lo, hi);
        }
    }
}

// ---- control ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void square_control(const float* __restrict__ f, int* __restrict__ ist,
                                                     float* __restrict__ fst, float* __restrict__ history,
                                                     int* __restrict__ decisions, int N, int steps, int early_stop) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int k = ist[(long)UD_SQUARE_I_K * N + n];
    if (k < 0 || k > steps) return;
    const float fk = f[n];
    float fbest;
    int accepted = 0, queries;
    if (k == 0) {
        fbest = fk;
        queries = 1;
    } else {
        fbest = fst[(long)UD_SQUARE_F_BEST * N + n];
        const int active = ist[(long)UD_SQUARE_I_ACTIVE * N + n];
        queries = ist[(long)UD_SQUARE_I_QUERIES * N + n] + (active ? 1 : 0);
        accepted = active && fk < fbest;
        if (accepted) fbest = fk;
    }
    fst[(long)UD_SQUARE_F_BEST * N + n] = fbest;
    ist[(long)UD_SQUARE_I_K * N + n] = k + 1;
    ist[(long)UD_SQUARE_I_ACCEPTED * N + n] = accepted;
    ist[(long)UD_SQUARE_I_ACTIVE * N + n] = early_stop ? (fbest > 0.f ? 1 : 0) : 1;
    ist[(long)UD_SQUARE_I_QUERIES * N + n] = queries;
    history[(long)k * N + n] = fk;
    decisions[(long)k * N + n] = accepted;
}

}  // namespace

extern "C" {

int ud_square_propose(float* x_try, float* x_best, const float* x0, const int* ist, const int* side, const int* dh,
                      const int* dw, const float* dsign, int N, int size, int steps, float eps, float lo, float hi, int closing,
                      ud_stream_t stream) {
    if (!x_try || !x_best || !x0 || !ist || !side || !dh || !dw || !dsign) return UD_EINVAL;
    if (N < 1 || N > 65535 || size < 1 || size > 32768 || steps < 1 || !(eps >= 0.f) || !(lo <= hi)) return UD_EINVAL;
    long bx = (2L * size * size + NT - 1) / NT;
    if (bx > MAX_BLOCKS_X) bx = MAX_BLOCKS_X;
    hipLaunchKernelGGL(square_propose, dim3((unsigned)bx, (unsigned)N), dim3(NT), 0, (hipStream_t)stream, x_try, x_best, x0, ist,
                       side, dh, dw, dsign, N, size, steps, eps, lo, hi, closing);
    UD_LAUNCH_CHECK();
    return 0;
}

int ud_square_control(const float* f, int* ist, float* fst, float* history, int* decisions, int N, int steps, int early_stop,
                      ud_stream_t stream) {
    if (!f || !ist || !fst || !history || !decisions || N < 1 || steps < 1) return UD_EINVAL;
    hipLaunchKernelGGL(square_control, dim3((unsigned)ud_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, f, ist, fst, history,
                       decisions, N, steps, early_stop);
    UD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

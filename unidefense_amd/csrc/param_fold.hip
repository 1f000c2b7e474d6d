// ud_param_fold_multi: every launch of a backward that only FINISHES a parameter's gradient — the fold of per-workgroup partials
// into a weight gradient, InstanceNorm's sum over samples into dgamma / dbeta, the copy of a conv weight gradient into the
// parameter's layout — as an item of ONE launch.  Nothing else in the step reads these results, yet on the replayed graph's single
// queue each such launch costs its ~4.5 us floor; here they run side by side.  The items travel by value in the kernel
// arguments (no device table: the launch sits inside a captured graph), a workgroup finds its item by a scan of the (uniform) block
// prefix.  The producers' immediate forms fold through the same kernel with one item, so each kind has ONE summation order.
#include "ud_common.h"
#include "bnref.h"

namespace {

static_assert(NT == 256, "16 elements x 16 lanes of partials per workgroup");
constexpr int FOLD_MAX = 44;          // 44 x 80 bytes of items + the prefix table: within the 4 KiB of kernel arguments
struct FoldArgs {
    ud_wgrad_fold it[FOLD_MAX];
    int block0[FOLD_MAX + 1];
    int n;
};

// element i of a conv weight gradient [A][KK][B] -> its place in the parameter's [A][B][KK]; KK <= 1: i itself
__device__ __forceinline__ long out_index(int i, int KK, int B) {
    if (KK <= 1) return i;
    const int a = i / (KK * B), r = i - a * (KK * B), tap = r / B, b = r - tap * B;
    return ((long)a * B + b) * KK + tap;
}

// dw[c][tap] = gate * sum_p part[p][tap][c]   (fp64 accumulation; the parameter's own layout [C][K*K])
__device__ __forceinline__ void fold_dw(const ud_wgrad_fold& f, int blk, double* smem) {
    double(*sm)[16][4] = reinterpret_cast<double(*)[16][4]>(smem);
    const int KK = f.p0 * f.p0, C = f.p1, KKC = KK * C, nparts = f.nparts;
    const int lane = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int i = (blk * 16 + lane) * 4;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < KKC) {
        const f32x4* p4 = reinterpret_cast<const f32x4*>(f.part + i);
        const long step = (long)KKC / 4;
        for (int p = sl; p < nparts; p += 16) {
            const f32x4 w = p4[(long)p * step];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += (double)w[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[sl][lane][e] = v[e];
    __syncthreads();
    if (sl < 4 && i < KKC) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sm[k][lane][sl];
        const int o = i + sl, tap = o / C, c = o % C;
        f.dst[(long)c * KK + tap] = (float)(t * (double)gate_factor(f.aux, f.p2));
    }
}

// Workgroup = 16 consecutive elements x 16 lanes of partials: lane group j adds partials j, j + 16, ... (independent loads, 64-byte
// segments, two chains), the 16 group sums are added in order through LDS.  `src` + p * `st`: partial p of this thread's element.
__device__ __forceinline__ void fold_f32_lanes(const float* src, long st, int nparts, bool live, float* dst, float* smem) {
    float(*red)[17] = reinterpret_cast<float(*)[17]>(smem);
    const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
    float s0 = 0.f, s1 = 0.f;
    if (live) {
        int p = grp;
        for (; p + 16 < nparts; p += 32) {
            s0 += src[p * st];
            s1 += src[(p + 16) * st];
        }
        if (p < nparts) s0 += src[p * st];
    }
    red[grp][el] = s0 + s1;
    __syncthreads();
    if (grp == 0 && live) {
        float t = red[0][el];
#pragma unroll
        for (int j = 1; j < 16; ++j) t += red[j][el];
        *dst = t;
    }
}

__device__ __forceinline__ void fold_f32(const ud_wgrad_fold& f, int blk, double* smem) {
    const int i = blk * 16 + (threadIdx.x & 15);
    const bool live = i < f.n;
    fold_f32_lanes(f.part + i, f.n, f.nparts, live, live ? f.dst + out_index(i, f.p0, f.p1) : nullptr, reinterpret_cast<float*>(smem));
    const int c = blk * NT + threadIdx.x;          // dgamma / dbeta from this rank's fp64 sums (ud_normbwd_apply's side outputs)
    if (c < f.p2) {
        if (f.dbeta) f.dbeta[c] = (float)f.s1l[c];
        if (f.dgamma) f.dgamma[c] = (float)f.s2l[c];
    }
}

// dw[co][c0 + cc] = the nparts partials of chunk c0 / CC summed in workgroup order
__device__ __forceinline__ void fold_pj(const ud_wgrad_fold& f, int blk, double* smem) {
    const int CO = f.p0, CE = f.p1, CC = f.p2;
    const int i = blk * 16 + (threadIdx.x & 15);
    const bool live = i < f.n;
    const float* src = f.part;
    if (live) {
        const int co = i / CE, c = i - co * CE, chunk = c / CC, cc = c - chunk * CC;
        src += (long)chunk * f.nparts * (CO * CC) + co * CC + cc;
    }
    fold_f32_lanes(src, (long)CO * CC, f.nparts, live, f.dst + i, reinterpret_cast<float*>(smem));
}

// out[i] = sum_b part[b][i]; 16 entries x 16 partial-lanes per workgroup, fp64 accumulation
__device__ __forceinline__ void fold_f64(const ud_wgrad_fold& f, int blk, double* sm) {
    const int el = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int i = blk * 16 + el, n = f.n;
    double acc = 0.0;
    if (i < n)
        for (int b = pl; b < f.nparts; b += 16) acc += (double)f.part[(long)b * n + i];
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (pl == 0 && i < n) {
        for (int k = 1; k < 16; ++k) acc += sm[k * 16 + el];
        f.dst[out_index(i, f.p0, f.p1)] = (float)acc;
    }
}

// dgamma[c] = sum_g s2[g][c], dbeta[c] = sum_g s1[g][c]   (G > 1: InstanceNorm)
__device__ __forceinline__ void fold_group(const ud_wgrad_fold& f, int blk) {
    const int c = blk * NT + threadIdx.x, C = f.n;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int g = 0; g < f.nparts; ++g) {
        a += (double)f.part[(long)g * C + c];
        b += (double)f.aux[(long)g * C + c];
    }
    if (f.dbeta) f.dbeta[c] = (float)a;
    if (f.dgamma) f.dgamma[c] = (float)b;
}

__device__ __forceinline__ void fold_layout(const ud_wgrad_fold& f, int blk) {
    const int i = blk * NT + threadIdx.x;
    if (i < f.n) f.dst[out_index(i, f.p0, f.p1)] = f.part[i];
}

__global__ __launch_bounds__(NT) void param_fold_multi(const FoldArgs a) {
    __shared__ double sm[16 * 16 * 4];
    int j = 0;
    while (j + 1 < a.n && (int)blockIdx.x >= a.block0[j + 1]) ++j;
    const ud_wgrad_fold& f = a.it[j];
    const int blk = (int)blockIdx.x - a.block0[j];
    switch (f.kind) {          // uniform over the workgroup
        case UD_FOLD_DW: fold_dw(f, blk, sm); break;
        case UD_FOLD_F32: fold_f32(f, blk, sm); break;
        case UD_FOLD_PJ: fold_pj(f, blk, sm); break;
        case UD_FOLD_F64: fold_f64(f, blk, sm); break;
        case UD_FOLD_GROUP: fold_group(f, blk); break;
        default: fold_layout(f, blk); break;
    }
}

// an item's workgroups; 0: not a valid item
int item_blocks(const ud_wgrad_fold& f) {
    if (!f.part || f.nparts < 1) return 0;
    const bool conv = f.kind == UD_FOLD_F32 || f.kind == UD_FOLD_F64 || f.kind == UD_FOLD_LAYOUT;
    if (conv && f.p0 > 1 && (f.p1 < 1 || f.n < 1 || f.n % (f.p0 * f.p1))) return 0;          // [A][KK][B] -> [A][B][KK]
    switch (f.kind) {
        case UD_FOLD_DW:
            if (!f.dst || (f.p0 != 3 && f.p0 != 5) || f.p1 < 4 || f.p1 % 4 || f.p2 < 0 || f.p2 > 2 || (f.p2 != 0 && !f.aux)) return 0;
            return ud_cdiv(f.p0 * f.p0 * f.p1, 64);
        case UD_FOLD_F32:
            if (!f.dst || f.n < 1 || f.p2 < 0 || f.p2 > 16L * f.n) return 0;
            if (f.p2 > 0 && ((f.dgamma && !f.s2l) || (f.dbeta && !f.s1l))) return 0;
            return ud_cdiv(f.n, 16);
        case UD_FOLD_PJ:
            if (!f.dst || f.p0 < 1 || f.p1 < 1 || f.p2 < 1 || f.p1 % f.p2 || f.n != f.p0 * f.p1) return 0;
            return ud_cdiv(f.n, 16);
        case UD_FOLD_F64:
            if (!f.dst || f.n < 1) return 0;
            return ud_cdiv(f.n, 16);
        case UD_FOLD_GROUP:
            if (!f.aux || f.n < 1 || (!f.dgamma && !f.dbeta)) return 0;
            return ud_cdiv(f.n, NT);
        case UD_FOLD_LAYOUT:
            if (!f.dst || f.n < 1 || f.dst == f.part) return 0;
            return ud_cdiv(f.n, NT);
        default: return 0;
    }
}

}  // namespace

extern "C" {

int ud_param_fold_multi(const ud_wgrad_fold* items, int n, ud_stream_t stream) {
    if (!items || n < 1) return UD_EINVAL;
    for (int i = 0; i < n; ++i)
        if (item_blocks(items[i]) < 1) return UD_EINVAL;
    for (int i0 = 0; i0 < n; i0 += FOLD_MAX) {
        FoldArgs a;
        a.n = n - i0 < FOLD_MAX ? n - i0 : FOLD_MAX;
        int b = 0;
        for (int j = 0; j < a.n; ++j) {
            a.it[j] = items[i0 + j];
            a.block0[j] = b;
            b += item_blocks(a.it[j]);
        }
        a.block0[a.n] = b;
        hipLaunchKernelGGL(param_fold_multi, dim3((unsigned)b), dim3(NT), 0, (hipStream_t)stream, a);
        UD_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"

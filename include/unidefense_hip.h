/*
 * unidefense_hip.h — C ABI of libunidefense_hip.so (gfx950 / MI355X).
 *
 * The reference (VISION-SJTU/UniDefense) has no native code and no FFI: its hot path reaches the
 * GPU through torch.nn / torch.fft (ATen -> vendor libraries).  Each entry point below replaces
 * one of those implicit kernels; the comment on each names the reference call site it serves
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every tensor is fp32, contiguous, "pixel-major" (NHWC): [N][H][W][C], i.e. a row-major
 *     matrix [M = N*H*W][C]; image-domain tensors with C = 3 are planes [N*C][H][W] (NCHW).
 *     "[G][R][C]" below means G groups of R rows (G = 1: batch norm; G = N, R = H*W: per sample).
 *   - plain pointers + sizes; the caller owns every buffer, including the scratch buffers
 *     ("part*") whose sizes the *_chunks / *_parts / *_blocks helpers return.  No allocation, no
 *     host synchronisation inside: every function only enqueues kernels on `stream` (a hipStream_t
 *     passed as void*) and is safe to capture into a hipGraph.
 *   - return 0 on success, a negative hipError_t on launch failure, UD_EINVAL on invalid arguments
 *     (the helpers return a non-negative count).
 *   - act / act_in: 0 = identity, 1 = swish x*sigmoid(x) (model/efficientnet/utils.py:66-82).
 */
#ifndef UNIDEFENSE_HIP_H
#define UNIDEFENSE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UD_EINVAL (-1000)

typedef void* ud_stream_t;

/* ---- conv geometry used by the gather modes of ud_gemm ------------------------------------
 * rows r = (n, oh, ow) over [N][Hout][Wout]; taps (kh, kw); source pixel of (r, tap):
 *   transposed == 0 :  ih = oh*stride - pad_t + kh                       (F.conv2d)
 *   transposed == 1 :  t = oh + pad_t - kh; valid iff t % stride == 0;  ih = t / stride
 *                                                                          (F.conv_transpose2d)
 * out-of-range sources read as 0. */
typedef struct {
    int N, Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad_t, pad_l, transposed;
} ud_conv_geom;

/* ---- ud_gemm: C[M][N] (+)= A . B on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) ---------
 * a_mode 0: A[m][k] at A + m*lda + k          (activations [pixels][Cin])
 *        1: A[k][m] at A + k*lda + m          (dY as the A operand of a weight gradient)
 *        2: conv gather: m = (n,oh,ow), k = (kh*KW+kw)*Cin + ci -> In[n][ih][iw][ci]  (geom g)
 * b_mode 0: B[n][k] at B + n*ldb + k          (weights [Cout][K])
 *        1: B[k][n] at B + k*ldb + n          (weights for the data gradient, X for the weight gradient)
 *        2: conv gather with k = (n,oh,ow) and n = (kh*KW+kw)*Cin + ci        (weight gradient of a conv)
 * supported (a_mode, b_mode): (0,0) (0,1) (1,1) (2,0) (1,2).
 * out_mode 0: store, 1: C += result, 2: atomicAdd (split_k > 1; C pre-zeroed or holding a term to add to),
 *          3: split s STORES its partial product into its own slice C + s * slice_stride (split_k >= 1; fp32, batch 1):
 *             the deterministic form of split-K — ud_sum_slices then adds the slices in ascending order
 * Serves: F.conv2d 1x1 in model/efficientnet/model.py:108,125 and exp.py:57 (freq_conv),
 *         nn.Conv2d 3x3 / nn.ConvTranspose2d in model/unidefense.py:59-102, model/modules.py:82,111,
 *         the stem conv model/efficientnet/model.py:185, torch.fft.rfft2 at 256x256 (as DFT-matrix
 *         GEMMs, model/unidefense.py:246-249), and their autograd backward (convolution_backward). */
typedef struct {
    const float* A; const float* B; float* C;
    int M, N, K;
    long lda, ldb, ldc;
    int a_mode, b_mode, out_mode, split_k;
    int batch; long strideA, strideB, strideC;   /* batch >= 1; element strides between batches */
    ud_conv_geom g;
    /* Optional epilogue statistics of the RESULT (training-mode BatchNorm behind a 1x1 conv, model.py:108-109,125-126):
     * stat_sum[n] += sum_m C[m][n], stat_sumsq[n] += sum_m C[m][n]^2, fp64 atomic adds — the BatchNorm's statistics pass
     * disappears.  Honoured only where ud_gemm_stats_slots() returns > 0 (split-bf16 kernel, out_mode 0, split_k 1,
     * batch 1); with more than 64 row tiles the adds go to slot (row tile % 64) of [64][N] arrays instead (the caller
     * passes zeroed slot arrays as stat_sum / stat_sumsq and folds them, e.g. with ud_stat_slots_fold). */
    double* stat_sum; double* stat_sumsq;
    /* Half storage (BASELINE configs[4]): bit 0 / 1 / 2 set = A / B / C point to _Float16 instead of float (element
     * strides unchanged).  Such descriptors always run on the fp16 MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulation):
     * plain modes only — (0,0) and (0,1) with A half (activations x fp32 weights), (1,1) with A and B half (the weight
     * gradient), any of them with fp32 operands; batch 1; a half C takes out_mode 0 / 1 (no atomics: split_k 1). */
    int half_mask;
    /* Tile of the BF16-pipe kernel: 0 = chosen by the library's cost model; 1..4 = 128x128, 128x64, 64x128, 64x64 —
     * for callers that tune per shape by measurement (unidefense_amd/kernels.py does, on the thin expand / project
     * GEMMs whose few tiles leave the k-loop latency exposed).
     * bit 8: reserved, ignored. */
    int tile_cfg;
    long slice_stride;       /* out_mode 3: elements between the splits' slices (>= M * ldc) */
} ud_gemm_desc;
int ud_gemm(const ud_gemm_desc* d, ud_stream_t stream);
/* out[i] (+)= sum_s ws[s * slice_stride + i], s = 0 .. slices-1 in this order (total, slice_stride multiples of 4) */
int ud_sum_slices(const float* ws, float* out, int slices, long total, long slice_stride, int accumulate,
                  ud_stream_t stream);
/* 0: ud_gemm would ignore stat_sum / stat_sumsq for this descriptor (the caller runs ud_colstats on the result);
 * 1: the epilogue adds straight into [N] accumulators; 64: it adds into 64 slots of [64][N] (see ud_gemm_desc). */
int ud_gemm_stats_slots(const ud_gemm_desc* d);
/* acc_sum[n] += sum_s slot_sum[s][n], likewise sumsq   (slots: the 64 above) */
int ud_stat_slots_fold(const double* slot_sum, const double* slot_sumsq, int slots, int N, double* acc_sum,
                       double* acc_sumsq, ud_stream_t stream);
/* Arithmetic path of ud_gemm (process-wide; initial value from env UD_GEMM_PATH):
 *   0 auto (default): plain GEMMs (a_mode, b_mode in {0,1}, 16-byte aligned, M,N,K >= 16) run on the BF16
 *     matrix pipe with every fp32 operand split exactly into three bf16 pieces and six piece products
 *     accumulated in fp32 (csrc/gemm_x3.hip: fp32-GEMM accuracy, error terms < 2^-26 |a||b|); all other shapes
 *     and the gather modes run on v_mfma_f32_32x32x2_f32;
 *   1 fp32 MFMA only;   2 split-bf16 wherever eligible;
 *   3 mixed precision (BASELINE configs[4]): wherever the split-bf16 kernel would run, the operands are rounded to fp16
 *     and multiplied by ONE v_mfma_f32_32x32x16_f16 per product tile with fp32 accumulation (fp32 storage stays). */
int ud_gemm_set_path(int path);
int ud_gemm_get_path(void);
/* 2 if ud_gemm would run this descriptor on the BF16 matrix pipe (split-bf16 kernel), 3 for its fp16 mixed-precision
 * mode (path 3), 1 for the fp32 pipe */
int ud_gemm_query_path(const ud_gemm_desc* d);

/* ---- ud_gemm_p3: the same fp32-accurate product from PRE-SPLIT operands (round 4) ----------------------------------
 * Serves the spectral 1x1 conv of the SF blocks, F.conv2d(x_freq, freq_conv.weight) in model/efficientnet/exp.py:57 (and
 * model/resnet/exp.py's copy), its data gradient and its weight gradient — the large GEMMs of the step.
 * An operand is a matrix X[R][Cx] stored as 16-bit planes in the "P32" panel layout:
 *     piece p of X[r][c]   at   X + p * plane + (c / 32) * panel + r * 32 + (c % 32)        (16-bit elements)
 * Each panel must be backed by rows up to the next multiple of 128 (panel >= 32 * roundup(R, 128); slack rows are read,
 * their products discarded).
 *   prec 3: three bf16 planes x = x0 + x1 + x2 (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1): the exact split
 *           ud_gemm performs inside its k-loop), six piece products — bitwise ud_gemm's result.  Written by ud_split_planes.
 *   prec 2: two fp16 planes s * x = h0 + 2^-11 h1 with a power-of-two scale s that takes the largest |x| it covers into
 *           [2^14, 2^15) — ONE scale for the tensor (ud_absmax + ud_split_planes_h2t; any mode) or one per row of X
 *           (ud_split_planes_h2; mode 0 only: the scale must be constant along k).  Three piece products on the fp16 matrix
 *           pipe into two fp32 accumulators (a0b0, and a1b0 + a0b1), the result (hi + 2^-11 lo) * a_inv_scale[m * a_scale_stride]
 *           * b_inv_scale[n * b_scale_stride] (= 1 / s; stride 0: a scalar, 1: a vector [M] / [N]).  22 significand bits of every
 *           element within 2^-18 of the scale's maximum (smaller elements: an absolute error of 2^-40 of that maximum — so with ONE
 *           scale per tensor a GEMM row lying 2^-24 below the largest keeps ~16 bits; with a scale per row every row keeps 22), the
 *           dropped a1b1 < 2^-24 |ab|, fp32 accumulation: the accuracy of an
 *           fp32 GEMM (measured at or below ud_gemm's error on every operand distribution tried) at half the matrix work.
 *   prec 1: ONE fp16 plane per operand — the first plane of prec-2 operands (or planes written by ud_planes_from_half, scale 1):
 *           one product per tile on the fp16 matrix pipe, fp32 accumulation, the result times the two inverse scales — the
 *           mixed-precision mode (BASELINE configs[4]: fp16 MFMA operands), 530-770 TFLOP/s on the spectral convs' shapes against
 *           290-530 of ud_gemm's path 3 (tools/bench_p3_prec1.py).  (a_mode, b_mode) as prec 2; c_half: a half-stored result.
 *   mode 0: GEMM row = row of X, k = column of X     (activations [pixels][C] as A; weights [Cout][Cin] as B)
 *   mode 1: GEMM row = column of X, k = row of X     (dY / X of a weight gradient; weights of a data gradient)
 * (a_mode, b_mode): prec 3 any; prec 2 (0,0) (0,1) (1,1).  K % 32 == 0.  *_npanel: panels reachable from the pointer (mode 1 clamps
 * its tile to them).  out_mode / split_k / slice_stride / stat_sum / stat_sumsq as in ud_gemm_desc (statistics: out_mode 0,
 * split_k 1; one slot array [N] while M <= 64 * 128, else 64 slots).
 * tile_cfg bit 8: reserved, ignored; bit 9 (0x200): XCD-aware grouped raster — XCD x takes a
 * contiguous range of an order that walks groups of GM = bits 12-15 (0: 4) tile rows column by column, so the workgroups of one L2
 * share GM A panels and 32 / GM B panels; bit 11 (0x800): stream-K — one workgroup per CU, the
 * (tile, K-tile) units dealt evenly; out_mode 0 (C zeroed by the caller: whole-tile segments store, partial ones add
 * atomically) or 1 (C holds a term to add to); split_k 1, no statistics. */
typedef struct {
    const uint16_t* A; const uint16_t* B; float* C;
    int M, N, K;
    long a_panel, a_plane, b_panel, b_plane;   /* 16-bit elements between panels / between the planes */
    int a_npanel, b_npanel;
    long ldc;
    int a_mode, b_mode, out_mode, split_k;
    double* stat_sum; double* stat_sumsq;
    int tile_cfg;
    long slice_stride;
    int prec;                                   /* 3, 2 or 1 */
    const float* a_inv_scale; const float* b_inv_scale;   /* prec 2 / 1 */
    int a_scale_stride, b_scale_stride;         /* 0: one scale for the operand; 1: one per GEMM row */
    int c_half;                                 /* prec 1: C is _Float16 (out_mode 0 / 1, split_k 1, no stream-K) */
} ud_gemm_p3_desc;
int ud_gemm_p3(const ud_gemm_p3_desc* d, ud_stream_t stream);
/* TWO products in one launch: the data gradient (nn: a_mode 0, b_mode 1) and the weight gradient (tn: a_mode 1, b_mode 1) of one
 * 1x1 conv — prec 2, out_mode 0 / 1 / 2, split_k >= 1, no stream-K form, no epilogue statistics.  The weight gradient's workgroups
 * follow the data gradient's in the same grid, so they start on the CUs the data gradient's last round of tiles leaves idle
 * (540 + 225 tiles on 256 CUs: 3 rounds instead of 3 + 1); tn->tile_cfg bit 16 (0x10000): the weight gradient's workgroups lead
 * the grid instead (few long tiles: the pair's critical path).  Results are those of two ud_gemm_p3 calls.
 * Round 6, the TAIL PAIR of one forward product (both descriptors a_mode 0, b_mode 0, prec 2): `nn` = the leading row tiles of
 * y = x w^T that fill whole rounds of the CUs (plain), `tn` = the remaining row tiles (A / C advanced to their first row) split
 * over K with atomics onto zeroed rows — their short workgroups fill what the plain part's last round leaves idle. */
int ud_gemm_p3_pair(const ud_gemm_p3_desc* nn, const ud_gemm_p3_desc* tn, ud_stream_t stream);
/* A half-stored matrix X[R][C] (row stride ld elements, C % 8 == 0, 16-byte aligned) as ONE fp16 plane in the P32 layout, values
 * unchanged (*inv_scale = 1): the operand of ud_gemm_p3 prec 1 for the activations of the mixed-precision mode (BASELINE
 * configs[4]); pad columns of the last panel zero. */
int ud_planes_from_half(const void* x, long R, int C, long ld, uint16_t* planes, long panel_stride, float* inv_scale,
                        ud_stream_t stream);
/* x fp32 [R][C] (row stride ld; C, ld multiples of 4) -> three bf16 planes in the P32 layout above; columns C .. 32*ceil(C/32)-1
 * are written as zeros, slack rows are left untouched. */
int ud_split_planes(const float* x, long R, int C, long ld, uint16_t* planes, long panel_stride, long plane_stride,
                    ud_stream_t stream);
/* the prec-2 form with one scale per row: two fp16 planes of s_r * x[r][:] and inv_scale[r] = 1 / s_r (C <= 4096) */
int ud_split_planes_h2(const float* x, long R, int C, long ld, uint16_t* planes, long panel_stride, long plane_stride,
                       float* inv_scale, ud_stream_t stream);
/* the prec-2 form with one scale for the tensor: absmax[256] = partial maxima of |x| over the matrix, as the bit patterns of
 * non-negative floats (ud_absmax writes all 256; a producer kernel may fill them instead), then the split folds them and writes
 * the planes and *inv_scale = 1 / s */
int ud_absmax(const float* x, long R, int C, long ld, uint32_t* absmax, ud_stream_t stream);
int ud_split_planes_h2t(const float* x, long R, int C, long ld, uint16_t* planes, long panel_stride, long plane_stride,
                        const uint32_t* absmax, float* inv_scale, ud_stream_t stream);
/* Every weight matrix of a step in TWO launches (an absmax pass and a split pass over all of them) instead of two per matrix:
 * `items` is a DEVICE array of n descriptors sorted by their block prefixes — item i owns absmax blocks [amax_block0,
 * amax_block0 + amax_blocks) (amax_blocks <= 256: block b writes slot b of the item's 256 slots; the caller zeroes the
 * n * 256 slots ONCE, the unused ones stay zero) and split blocks [split_block0, split_block0 + split_bx * ceil(C / 32)),
 * split_bx = ceil(R / 64).  Same planes and scales as ud_absmax + ud_split_planes_h2t per matrix (tested bitwise). */
typedef struct {
    const float* x; uint16_t* out; float* inv_scale;
    long R, ld, panel, plane;
    int C, amax_block0, amax_blocks, split_block0, split_bx, pad_;
} ud_split_item;
int ud_split_planes_h2t_multi(const ud_split_item* items_dev, int n, uint32_t* slots, int amax_blocks_total,
                              int split_blocks_total, ud_stream_t stream);

/* A k x k conv (F.conv2d, any stride; model/resnet/exp.py:95-111, model/modules.py:111, the decoders) as a 1x1 conv on ud_gemm_p3:
 * ud_im2col_planes writes its im2col matrix [N Hout Wout] x [KH KW Cin] (g->transposed == 0, Cin % 32 == 0) DIRECTLY as prec-2
 * planes (P32 layout, one scale from `absmax`: 256 slots holding |x|max of the conv's input) — forward = planes . W^T, weight
 * gradient = dY^T . planes, data gradient = ud_col2im(dY . W): dx[n][ih][iw][ci] = sum over the taps of the [N Hout Wout] x
 * [KH KW Cin] fp32 matrix dcol (the gather adjoint to the im2col; dx written). */
int ud_im2col_planes(const float* x, const ud_conv_geom* g, uint16_t* planes, long panel_stride, long plane_stride,
                     const uint32_t* absmax, float* inv_scale, ud_stream_t stream);
int ud_col2im(const float* dcol, const ud_conv_geom* g, float* dx, ud_stream_t stream);

/* All k x k conv weights of a step into the [rows][tap][reduced channel] matrices the implicit-GEMM convs read, in ONE launch
 * (F.conv2d / ConvTranspose2d weights of model/unidefense.py:59-102, model/modules.py:111, the stem, model/resnet/exp.py:95-111):
 * src W[A][B][KH][KW] -> mode 0: dst[a][kh][kw][b]; mode 1: dst[b][KH-1-kh][KW-1-kw][a]; mode 2: dst[b][kh][kw][a].
 * items_dev: device table; item i owns blocks [block0, block0 + ceil(A B KH KW / 256)), blocks_total their sum. */
typedef struct {
    const float* src;
    float* dst;
    int A, B, KH, KW, mode, block0;
} ud_layout_item;
int ud_weight_layouts_multi(const ud_layout_item* items_dev, int n, int blocks_total, ud_stream_t stream);

/* ---- column reductions / normalisation on [G][R][C]  (C % 4 == 0) -----------------------------
 * Every reduction is a partial pass (fp64 per-workgroup totals stored into the scratch `ws`) plus a small
 * finalize launch; deterministic, no atomics.  ws: ud_reduce_ws_doubles(G, R, C) doubles of scratch, no
 * initialisation needed, contents undefined afterwards (one buffer can serve all calls issued in order on a stream).
 * Serves nn.BatchNorm2d/1d in training mode (model/efficientnet/model.py:67,77,91,186,222;
 * model/unidefense.py:104; model/modules.py:83,112), nn.InstanceNorm2d (model/unidefense.py:54),
 * MemoryEfficientSwish (utils.py:66-82), adaptive_avg_pool2d(x,1) / mean([-2,-1]). */
int ud_reduce_ws_doubles(int G, int R, int C);
/* mean[G][C], invstd[G][C] = 1/sqrt(biased var + eps); var_out optional; when running_mean != NULL and
 * G == 1 the running statistics are updated in place (momentum, unbiased variance) like nn.BatchNorm. */
int ud_norm_stats(const float* x, int G, int R, int C, float eps, double* ws, float* mean, float* invstd,
                  float* var_out, float momentum, float* running_mean, float* running_var, ud_stream_t stream);
/* torch.nn.SyncBatchNorm forward exchange (engine/forgery_engine.py:142), after an all_gather of every rank's
 * (mean, biased var) over `rows_per_rank` rows each: gathered[world][2][C] -> global mean / invstd, running
 * statistics updated with the unbiased variance over world*rows_per_rank rows (running_* may be NULL). */
int ud_syncbn_combine(const float* gathered, int world, int C, long rows_per_rank, float eps, float momentum,
                      float* running_mean, float* running_var, float* mean, float* invstd, ud_stream_t stream);
/* y = act(gamma * (x - mean[g]) * invstd[g] + beta) */
int ud_norm_apply_fwd(const float* x, int G, int R, int C, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, int act, float* y, ud_stream_t stream);
/* dz = dy * act'(z); s1 = sum dz, s2 = sum dz*xhat per (g,c); dgamma = sum_g s2, dbeta = sum_g s1;
 * dx = gamma*invstd*(dz - s1/R - xhat*s2/R)   (dx may be NULL: reductions only) */
int ud_norm_bwd(const float* x, const float* dy, int G, int R, int C, const float* mean, const float* invstd,
                const float* gamma, const float* beta, int act, double* ws, float* s1, float* s2, float* dgamma,
                float* dbeta, float* dx, ud_stream_t stream);
/* the elementwise half of ud_norm_bwd with caller-provided sums (already all-reduced over the ranks) and
 * inv_count = 1 / (rows of all ranks): SyncBatchNorm backward (engine/forgery_engine.py:142) */
int ud_norm_bwd_apply(const float* x, const float* dy, int G, int R, int C, const float* mean,
                      const float* invstd, const float* gamma, const float* beta, const float* s1,
                      const float* s2, float inv_count, int act, float* dx, ud_stream_t stream);
/* out[g][c] = scale * sum_r x[g][r][c] ;  out[g][c] = scale * sum_r a*b */
int ud_group_colsum(const float* x, int G, int R, int C, float scale, double* ws, float* out, ud_stream_t stream);
int ud_group_coldot(const float* a, const float* b, int G, int R, int C, float scale, double* ws, float* out,
                    ud_stream_t stream);
/* out[n][p][c] = g[n][c] * scale   (gradient of the mean over the HW rows) */
int ud_bcast_rows(const float* g, float scale, float* out, int N, int HW, int C, ud_stream_t stream);

/* ---- depthwise k x k conv, k in {3,5}, stride in {1,2}; weights tap-major wt[k*k][C] ------------
 * Serves the depthwise Conv2dStaticSamePadding / the spatial branch of SFConv2dStaticSamePadding
 * (model/efficientnet/utils.py:277-280, exp.py:49-51); pad_t/pad_l = top/left of the static ZeroPad2d. */
int ud_dwconv_fwd(const void* x, const float* wt, void* y, int N, int H, int W, int C, int Ho, int Wo, int K,
    int stride, int pad_t, int pad_l, int f16, ud_stream_t stream);
/* add (may be NULL): another contribution to the same gradient, [N][H][W][C]; dx = conv-transpose(dy) + add
 * (the input of SFConv's spatial branch also feeds its frequency branch, exp.py:49-55) */
int ud_dwconv_bwd_data(const void* dy, const float* wt, const void* add, void* dx, int N, int H, int W, int C,
    int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int f16, ud_stream_t stream);
int ud_dwconv_bwd_weight_parts(int C, int chunks);   /* rows of K*K*C floats that `part` must hold */
/* every depthwise weight of the network to the tap-major layout in one launch.  table: layers x 4 int64 in DEVICE
 * memory (source pointer [C][K*K], C, K*K, destination offset in floats); dst[off + tap*C + c] = src[c*K*K + tap];
 * max_elems = the largest C*K*K */
int ud_dw_weights_tapmajor(const void* table, int layers, long max_elems, float* dst, ud_stream_t stream);
/* dwt: the gradient in the PARAMETER's layout [C][K*K] (nn.Conv2d weight [C,1,K,K]), not tap-major */
int ud_dwconv_bwd_weight(const float* x, const float* dy, float* dwt, float* part, int chunks, int N,
                         int H, int W, int C, int Ho, int Wo, int K, int stride, int pad_t, int pad_l,
                         ud_stream_t stream);

/* ---- batched real 2-D FFT, S x S planes, S in {8,16,32,64}, channel = lane --------------------
 * ud_rfft2 : x[N][S][S][C] -> Y[N][S][S/2+1][2C]  (Re in channels [0,C), Im in [C,2C)),
 *            Y = f(kx) * DFT2(x), f = scale for kx in {0,S/2}, scale*w_interior otherwise
 * ud_irfft2: Y -> x = scale * C2R(f(kx) * Y), f = 1 / w_interior likewise
 * torch.fft.rfft2/irfft2 (model/efficientnet/exp.py:55,60; model/unidefense.py:130-145):
 *   forward rfft2 = (scale,1), its adjoint = ud_irfft2(scale, 0.5);
 *   forward irfft2 = (scale,1), its adjoint = ud_rfft2(scale, 2). */
int ud_rfft2(const void* x, void* Y, int N, int S, int C, float scale, float w_interior, int f16, ud_stream_t
    stream);
int ud_irfft2(const void* Y, void* x, int N, int S, int C, float scale, float w_interior, int f16, ud_stream_t
    stream);
/* S = 32: the transform may be shared by a LANE PAIR (lanes l and l ^ 32 hold the even / odd decimated samples, the last
 * radix-2 stage crosses the halves with wavefront shuffles; a wave owns 32 channels = whole 128-byte lines).  0 auto (where the
 * 32-channel groups are full and fit one round of workgroups), 1 never, 2 always (env UD_FFT32_WAVE = 0 / 1: never / always).
 * Returns the previous mode. */
int ud_fft32_set_wave(int mode);

/* ---- small FC: y[n][o] = sum_i act_in(x[n][i]) W[o][i] + b[o]  (SE 1x1 convs, classifier) ------
 * model/efficientnet/model.py:119-121; model/modules.py:27.  Any of dx / dW / db may be NULL. */
int ud_fc_fwd(const float* x, const float* W, const float* b, float* y, int N, int I, int O, int act_in,
              ud_stream_t stream);
int ud_fc_bwd(const float* dy, const float* W, const float* x, float* dx, float* dW, float* db, int N,
              int I, int O, int act_in, ud_stream_t stream);

/* ---- SE gating (model/efficientnet/model.py:122): y = x * sigmoid(s[n][c]);
 *      dx = dy * sigmoid(s) + dpool[n][c] / HW;   v *= sigmoid'(s) */
int ud_se_scale_fwd(const float* x, const float* s, float* y, int N, int HW, int C, ud_stream_t stream);
int ud_se_scale_bwd(const float* dy, const float* s, const float* dpool, float* dx, int N, int HW, int C,
                    ud_stream_t stream);
int ud_sigmoid_grad_mul(const float* s, float* v, long n, ud_stream_t stream);

/* ---- SFConv mixing (model/efficientnet/exp.py:61-65): y = (1-a) spat + a P(freq), a = sigmoid(*alpha),
 *      P = identity or the 2x2 average pool (pool = 1: freq is [N][2Ho][2Wo][C]).
 *      bwd: part holds ud_sfmix_blocks() DOUBLES; dalpha[0] = sigmoid'(alpha) * sum dy (P(freq) - spat) */
int ud_sfmix_blocks(int N, int Ho, int Wo, int C);
int ud_sfmix_fwd(const void* spat, const void* freq, const float* alpha, void* y, int N, int Ho, int Wo, int C,
    int pool, int f16, ud_stream_t stream);
int ud_sfmix_bwd(const void* spat, const void* freq, const float* alpha, const void* dy, void* dspat, void*
    dfreq, double* part, float* dalpha, int N, int Ho, int Wo, int C, int pool, int f16, ud_stream_t stream);
/* dfreq [N][2 Ho][2 Wo][C] = U(dy) / 4 for dy [N][Ho][Wo][C]: the data gradient of the 2 x 2 mean of the pooled frequency branch
 * alone — ud_sfmix_bwd's dfreq (pool = 1) without the gate factor, dspat and dalpha, for a frozen backward that keeps neither
 * branch (the gate factor is applied by the ud_rfft2_ex that follows; the spatial branch by the dgrad kernel's gate mode 2) */
int ud_sfmix_pool_bwd(const void* dy, void* dfreq, int N, int Ho, int Wo, int C, int f16, ud_stream_t stream);
/* same for two equal-shape tensors (fuse_coef, model/unidefense.py:153-154) */
int ud_gate_mix_blocks(long total);
int ud_gate_mix_fwd(const float* p, const float* q, const float* alpha, float* y, long total,
                    ud_stream_t stream);
int ud_gate_mix_bwd(const float* p, const float* q, const float* alpha, const float* dy, float* dp, float* dq,
                    double* part, float* dalpha, long total, ud_stream_t stream);

/* ---- elementwise --------------------------------------------------------------------------------
 * ud_residual_fwd: out = x * (keep[n] * inv_keep) + skip   (drop_connect + skip, model.py:130-134;
 *                  skip / keep may be NULL)
 * ud_axpby: out = alpha*a + beta*b (b may be NULL); ud_mask_scale: out = x*mask*scale (dropout by mask);
 * ud_absdiff: out = |a - b| (b may be NULL) */
int ud_residual_fwd(const float* x, const float* skip, const float* keep, float inv_keep, float* out,
                    long total, long per_sample, ud_stream_t stream);
int ud_axpby(const void* a, float alpha, const void* b, float beta, void* out, long total, int f16, ud_stream_t
    stream);
int ud_mask_scale(const float* x, const float* mask, float scale, float* out, long total,
                  ud_stream_t stream);
int ud_absdiff(const float* a, const float* b, float* out, long total, ud_stream_t stream);

/* ---- layout + image-domain tail --------------------------------------------------------------------
 * ud_pix_to_planes: [N][HW][C] -> [N][C][HW], mode 1 applies tanh (nn.Tanh, model/unidefense.py:101)
 * ud_planes_to_pix: reverse; mode 2 multiplies by (1 - aux^2), aux = saved tanh output (planes)
 * ud_bilinear_*   : F.interpolate(mode='bilinear', align_corners=True) on P planes (unidefense.py:16)
 * ud_l1_*         : out[n] = scale * sum |a - b| per sample and its gradient g[n]*scale*sign(a-b)
 *                   (torch.abs(...).mean(dim=[-3,-2,-1]), unidefense.py:245,251-253); b may be NULL */
int ud_pix_to_planes(const float* in, float* out, int N, int C, int HW, int mode, ud_stream_t stream);
int ud_planes_to_pix(const float* in, const float* aux, float* out, int N, int C, int HW, int mode,
                     ud_stream_t stream);
int ud_bilinear_fwd(const float* x, float* y, int P, int Hi, int Wi, int Ho, int Wo, ud_stream_t stream);
int ud_bilinear_bwd(const float* dy, float* dx, int P, int Hi, int Wi, int Ho, int Wo, ud_stream_t stream);
int ud_l1_chunks(long per_sample);
int ud_l1_fwd(const float* a, const float* b, float* part, float* out, int N, long per_sample, float scale,
              ud_stream_t stream);
int ud_l1_bwd(const float* a, const float* b, const float* g, float scale, int accumulate, float* da, int N,
              long per_sample, ud_stream_t stream);

/* ---- dynamic-filter mask (model/modules.py:94-104, 123-133), rows m over pixels:
 *      pre[m] = [mean_c proj, max_c proj, diff[m][0..D)], mask = sigmoid(w2 . pre), out = mask * x
 *      bwd: dx = mask*dout; dlogit[m]; dproj[m][c] = dlogit*(w2[0]/C + w2[1]*[c == argmax]) */
int ud_dynfilter_fwd(const float* proj, const float* diff, const float* w2, const float* x, float* pre,
                     int* argmax, float* mask, float* out, int M, int C, int D, int Cx, ud_stream_t stream);
int ud_dynfilter_bwd(const float* dout, const float* dmask_ext, const float* x, const float* mask,
                     const int* argmax, const float* w2, float* dx, float* dlogit, float* dproj, int M,
                     int C, int Cx, ud_stream_t stream);

/* ---- ResNet-variant helpers (model/resnet/module_exp.py, model/resnet/exp.py) ------------------------
 * ud_avgpool_*    : k x k average pool to [N][Ho][Wo][C] (F.adaptive_avg_pool2d to size/k, module_exp.py:30-31)
 * ud_maxpool3s2_* : nn.MaxPool2d(3, 2, 1) with the winning tap per output in arg (module_exp.py:73-75)
 * ud_add_act_fwd  : y = act(a + b) (act 0 / 2 = ReLU) — `x += shortcut; act(x)` (resnet/exp.py:146-147)
 * ud_relu_bwd     : g = dy * [y > 0]
 * ud_copy_cols    : dir 0: wide[m][off..off+Cn) = narrow[m][:] (torch.cat(dim=1), module_exp.py:32);
 *                   dir 1: the reverse (slice = gradient of the concat) */
int ud_avgpool_fwd(const float* x, float* y, int N, int Ho, int Wo, int C, int k, ud_stream_t stream);
int ud_avgpool_bwd(const float* dy, float* dx, int N, int Ho, int Wo, int C, int k, ud_stream_t stream);
/* F.adaptive_avg_pool2d to an output size that does not divide the input (model/efficientnet/exp.py:61-62 on the 95 x 95 map of
 * the 380 x 380 trunk: 95 -> 48), pixel-major [N][H][W][C] -> [N][Ho][Wo][C], Ho <= H, Wo <= W; windows [floor(o H / Ho),
 * ceil((o + 1) H / Ho)) as in ATen; _bwd is its adjoint (dx written, not accumulated). */
int ud_adaptive_avgpool_fwd(const float* x, float* y, int N, int H, int W, int Ho, int Wo, int C, ud_stream_t stream);
int ud_adaptive_avgpool_bwd(const float* dy, float* dx, int N, int H, int W, int Ho, int Wo, int C, ud_stream_t stream);
int ud_maxpool3s2_fwd(const float* x, float* y, unsigned char* arg, int N, int H, int W, int C,
                      ud_stream_t stream);
int ud_maxpool3s2_bwd(const float* dy, const unsigned char* arg, float* dx, int N, int H, int W, int C,
                      ud_stream_t stream);
int ud_add_act_fwd(const float* a, const float* b, int act, float* y, long total, ud_stream_t stream);
int ud_relu_bwd(const float* dy, const float* y, float* g, long total, ud_stream_t stream);
int ud_copy_cols(float* narrow, float* wide, long M, int Cn, int Cw, int off, int dir, ud_stream_t stream);

/* ---- asymmetrical weighted triplet loss (loss/triplet_loss.py:16-82) on feat[N][D]; anchors = the first n_real
 * rows (the batch is ordered [real...; fake...], triplet_loss.py:46-53).  Writes the scalar loss and
 * dfeat[N][D] = d loss / d feat in two launches (as torch ops: ~90 tiny kernels per feature).
 * ws: n_real * (N + 1) floats of scratch. */
int ud_aw_triplet(const float* feat, int N, int D, int n_real, float* loss, float* dfeat, float* ws,
                  ud_stream_t stream);

/* ---- the scalar tail of one pass's loss in two launches (engine/abstract_engine.py:241-281 of the reference: `softmax`
 * criterion on cls_out :250-254, the mask means :256-263, the triplet terms :232-240, the real / fake means of the per-sample
 * reconstruction and frequency terms :241-249, their weighted sum :264-270 — ~45 torch launches of 4-5 us per pass):
 *   vals[0] = w_cls CE(cls, tgt) + w_fm mean(fm) + w_sm mean(sm) + w_trip sum_f awtriplet(feat_f) + w_rec mean(spatial[:R])
 *             + w_freq mean(freq[:R]);  vals[1..8] = CE, sum of triplet terms, real / fake mean of spatial, real / fake mean
 *   of freq, mean(fm), mean(sm);  d* = d vals[0] / d (that input).  The first R rows are the real samples, the next F the fake
 * ones (triplet_loss.py:46-53).  NULL fm / sm / spatial / freq: the term is absent.  ws: ud_loss_tail_ws_floats floats. */
typedef struct {
    const float* feat[3]; float* dfeat[3]; int D[3]; int nfeat;          /* triplet features [N][D_f] */
    const float* cls; const long long* tgt; float* dcls; int N, C, R, F;   /* logits [N][C], int64 labels */
    const float* fm; float* dfm; int nfm; const float* sm; float* dsm; int nsm;
    const float* spatial; float* dspatial; const float* freq; float* dfreq; /* [N] */
    float w_cls, w_fm, w_sm, w_trip, w_rec, w_freq;
    float* vals;                                                            /* 9 floats */
    float* ws;
} ud_loss_tail;
int ud_loss_tail_ws_floats(int N, int n_real, int nfeat);
int ud_loss_tail_run(const ud_loss_tail* t, ud_stream_t stream);

/* ---- direct 3x3 conv for small channel counts (csrc/conv_small.hip): the image-resolution end of the decoder
 * (model/unidefense.py:59-102: 40 -> 20 -> 3 channels at 64x64 / 128x128), its data gradients / transposed conv, and
 * the stem conv (model/efficientnet/model.py:185).  Same operation and geometry as ud_gemm with a_mode 2:
 * y[N][Hout][Wout][Cout] = gather-conv(x[N][Hin][Win][Cin], wmat[Cout][9*Cin]); one thread per output pixel.
 * ud_conv_small_supported: 1 if a kernel exists for (Cin, Cout, KH, KW), else 0 (use ud_gemm). */
int ud_conv_small_supported(int Cin, int Cout, int KH, int KW);
int ud_conv_small(const ud_conv_geom* g, const float* x, const float* wmat, float* y, int Cout, ud_stream_t stream);
/* weight gradient of the same convs (ud_gemm's b_mode 2): out[Ma][9*Cin] = sum over the rows m = (n,oh,ow) of g's
 * output grid of a[m][Ma] (x) patch(x)[m][9*Cin].  part: ud_conv_small_wgrad_ws_floats(Cin, Ma) floats of scratch
 * (per-workgroup partial results, summed by a second launch; deterministic, no atomics). */
int ud_conv_small_wgrad_supported(int Cin, int Ma, int KH, int KW);
long ud_conv_small_wgrad_ws_floats(int Cin, int Ma);
int ud_conv_small_wgrad(const ud_conv_geom* g, const float* a, const float* x, float* part, float* out, int Ma,
                        ud_stream_t stream);

/* ---- direct 3x3 conv on the matrix pipe (csrc/conv_mfma.hip): the decoder's 20/40/80/160-channel convs, their data gradients,
 * the ConvTranspose2d(k3, s2) forward and its stride-2 data gradient.  Same operation as ud_conv_small; one workgroup owns a
 * tile of output pixels and all Cout, the input patch is staged and split into two fp16 pieces once, three fp16 MFMAs per
 * k-step give fp32-GEMM accuracy.  ud_conv_mfma_mode: the geometry class of g — 0 stride 1 pad 1 with Hout = Hin, 1 transposed
 * stride 2 pad 1 with Hout = 2 Hin, 2 stride 2 pad 1 with Hin = 2 Hout (3x3 windows only), -1 none of them.
 * ud_conv_mfma_supported: 1 if a kernel exists for (Cin, Cout, mode), else 0; ud_conv_mfma classifies g the same way and returns
 * UD_EINVAL for any other geometry or pair, and for pointers that are not 16-byte aligned. */
int ud_conv_mfma_mode(const ud_conv_geom* g);
int ud_conv_mfma_supported(int Cin, int Cout, int mode);
int ud_conv_mfma(const ud_conv_geom* g, const float* x, const float* wmat, float* y, int Cout, ud_stream_t stream);
/* weight gradient of the same convs (ud_gemm's b_mode 2; geometry classes 0 and 2): out[Ma][9*Cin] = sum over the rows
 * m = (n,oh,ow) of g's output grid of a[m][Ma] (x) patch(x)[m][9*Cin] — a = dy and x gathered for a conv, a = x and dy gathered at
 * stride 2 for a transposed conv.  Pixels are the MFMA's reduction index; exact bf16 x 3 split, six products.  part:
 * ud_conv_mfma_wgrad_ws_floats(Cin, Ma) floats of scratch (per-workgroup partials, summed in a fixed order by a second launch:
 * deterministic, no atomics, no zero fill). */
int ud_conv_mfma_wgrad_supported(int Cin, int Ma, int mode);
long ud_conv_mfma_wgrad_ws_floats(int Cin, int Ma);
int ud_conv_mfma_wgrad(const ud_conv_geom* g, const float* a, const float* x, float* part, float* out, int Ma,
                       ud_stream_t stream);

/* ---- gradient with respect to the input image (csrc/inputgrad.hip): x.grad of model(x) ----------------------------
 * ud_stem_dgrad   : dx[N][3][Hin][Win] (+= when accumulate) the data gradient of the stem conv g (F.conv2d geometry, Cin 3,
 *                   stride 2) from dy[N][Hout][Wout][Cout] (pixel-major) and the module weight w[Cout][3][KH][KW]
 *                   (model/efficientnet/model.py:185, 3x3 -> 48 with static SAME pads; model/resnet/exp.py:395, 7x7 -> 64,
 *                   pad 3).  dx is x's planes layout; accumulate adds onto the gradient already there.  dy 16-byte aligned.
 *                   ud_stem_dgrad_supported: 1 for (Cin, Cout, KH, KW, stride) = (3, 48, 3, 3, 2) or (3, 64, 7, 7, 2), else 0;
 *                   any other geometry (or a pad outside [0, KH)) is UD_EINVAL.
 * ud_absdiff_bwd  : gradients of out = |a - b|: da = sign(a - b) g, db = -sign(a - b) g, sign(0) = 0 as in torch.abs
 *                   (model/unidefense.py:138,148: the attention's difference inputs); da or db may be NULL.
 * ud_outer        : out[M][D] = u[M] v[D] (the difference inputs' gradient of a dynamic filter, model/modules.py:94-104:
 *                   dlogit times the filter weights of those channels). */
int ud_stem_dgrad_supported(int Cin, int Cout, int KH, int KW, int stride);
int ud_stem_dgrad(const ud_conv_geom* g, const float* dy, const float* w, float* dx, int Cout, int accumulate,
                  ud_stream_t stream);
int ud_absdiff_bwd(const float* a, const float* b, const float* g, float* da, float* db, long total, ud_stream_t stream);
int ud_outer(const float* u, const float* v, float* out, long M, int D, ud_stream_t stream);

/* ---- iterated input-gradient attacks (csrc/attack.hip; unidefense_amd/attack.py: AttackRunner) ---------------------
 * All fp32 tensors are contiguous planes [N][3][H][W]: per = 3 H W elements per sample, total = N per; neither needs to be
 * a multiple of 4.  No atomics and no data-dependent partition: the results are a function of shapes and inputs only.
 * UD_EINVAL: a NULL tensor, total <= 0 / N < 1 / per < 1, eps < 0, lo > hi, a scratch buffer that is too small.
 * ud_attack_step_linf  : in place  x_adv <- clamp(clamp(x_adv + step sign(g), x0 - eps, x0 + eps), lo, hi), evaluated in
 *                        that order with one fp32 rounding per operation (bitwise what the same torch fp32 expression
 *                        gives); sign(0) = 0; a NaN in g becomes a NaN in x_adv at that element; step may be negative.
 * ud_sample_sumsq      : out[n] = sum_i (a[n][i] - b[n][i])^2 as double, difference, square and sum formed in double
 *                        (b NULL: the plain sum of squares).  per is cut into fixed 4096-element parts; with more than one
 *                        part the partial sums go to ws (ud_sample_sumsq_ws_bytes(N, per) bytes, 0 for one part; ws_bytes
 *                        is what the caller holds) and a second launch adds them in index order.
 * ud_attack_step_l2    : in place  x_adv[n] += step g[n] / max(sqrt(gss[n]), 1e-12)   (gss[n] = |g[n]|^2, double)
 * ud_attack_project_l2 : in place, with d = x_adv - x0 and dss[n] = |d[n]|^2 (double):
 *                        x_adv[n] <- clamp(x0[n] + d[n] min(1, eps / max(sqrt(dss[n]), 1e-12)), lo, hi); a factor of
 *                        exactly 1 leaves x_adv[n] as it is before the clamp.  Both L2 kernels form the factor and the
 *                        new value in double and round once to fp32. */
int ud_attack_step_linf(float* x_adv, const float* x0, const float* g, long total, float step, float eps, float lo, float hi,
                        ud_stream_t stream);
long ud_sample_sumsq_ws_bytes(int N, long per);
int ud_sample_sumsq(const float* a, const float* b, int N, long per, double* out, double* ws, long ws_bytes,
                    ud_stream_t stream);
int ud_attack_step_l2(float* x_adv, const float* g, const double* gss, int N, long per, float step, ud_stream_t stream);
int ud_attack_project_l2(float* x_adv, const float* x0, const double* dss, int N, long per, float eps, float lo, float hi,
                         ud_stream_t stream);

/* ---- Auto-PGD (csrc/apgd.hip; unidefense_amd/attack.py: APGDRunner) -------------------------------------------------
 * Per-sample control state on the device, so that one iteration is a static launch sequence inside a captured graph:
 *   ist [5][N] int32 : rows UD_APGD_I_K (iteration index), _CNT (rises of f since the last checkpoint), _HALVED (eta was
 *                      halved at the previous checkpoint), _IMPROVED, _RESET (what the update of this iteration obeys)
 *   fst [5][N] fp32  : rows UD_APGD_F_PREV (f of the previous iteration), _BEST, _CKPT (f_best at the last checkpoint), _ETA, _A
 *   history [steps + 1][N] fp32 : row k = f_k, row steps = f of the closing evaluation
 * ud_apgd_control: f [N] fp32 = the per-sample objective at the current point.  One thread per sample; with k = ist[K][n]:
 *   k == 0: f_best = f_ckpt = f, eta = eta0, improved = 1, cnt = 0, halved = 0, a = 1
 *   k  > 0: cnt += (f > f_prev); improved = f > f_best (f_best updated); a = alpha
 *   k == ck_w[j]: c1 = cnt < ck_thr[j]; c2 = !halved && f_ckpt == f_best; c1 || c2: eta /= 2, reset = 1, a = 1, halved = 1,
 *                 else halved = 0; then f_ckpt = f_best, cnt = 0          (reset = 0 where no checkpoint fired)
 *   then f_prev = f, history[k][n] = f, ist[K][n] = k + 1.  k outside [0, steps) writes nothing.  The caller zeroes row
 *   UD_APGD_I_K to start a run.  A NaN f compares false everywhere.  ck_w (strictly rising, in [1, steps - 1]) and ck_thr
 *   (ceil(rho * window), so that c1 is an integer comparison) are HOST arrays of n_ck <= UD_APGD_MAX_CHECKPOINTS entries,
 *   passed by value to the kernel.  closing != 0: only improved = f > f_best (f_best updated) and history[steps][n] = f.
 * ud_apgd_update_linf: one pass over contiguous fp32 [N][per] tensors obeying (improved, reset, eta, a) of each sample:
 *   improved: (x_best, g_best) <- (x, g);  (src, gs) = (x_best, g_best) if reset else (x, g);
 *   z = P(src + eta sign(gs));  x <- z if a == 1 else P((src + a (z - src)) + (1 - a) (src - x_prev));  x_prev <- src
 *   with P(v) = clamp(clamp(v, x0 - eps, x0 + eps), lo, hi), one fp32 rounding per operation in exactly this order (bitwise
 *   the torch fp32 expression), sign(0) = 0, a NaN gradient element gives a NaN there.
 * ud_apgd_keep: dst[n] <- src[n] for the samples with flag[n] != 0 (flag [N] int32).
 * L2 (per-sample factors, sums and new values formed in double, one rounding to fp32, as ud_attack_step_l2):
 *   ud_apgd_step_l2   : gss[n] = |g[n]|^2.  improved: (x_best, g_best, gss_best) <- (x, g, gss); source selection as above
 *                       with x <- src; z <- src + eta gs / max(|gs|, 1e-12)   (z is projected by ud_sample_sumsq +
 *                       ud_attack_project_l2 next)
 *   ud_apgd_combine_l2: x holds src, z the projected step: x <- z if a == 1 else src + a (z - src) + (1 - a)(src - x_prev);
 *                       x_prev <- src
 *   ud_apgd_project_l2: ud_attack_project_l2 on the samples with a != 1 only; a sample with a == 1 is left as it is.
 * UD_EINVAL before any HIP call: a NULL pointer, N < 1, per < 1, steps < 1, eps < 0 or NaN, lo > hi or NaN, eta0 < 0 or NaN,
 * alpha outside (0, 1], a checkpoint table that is too long, not rising or outside [1, steps - 1]. */
#define UD_APGD_MAX_CHECKPOINTS 16
#define UD_APGD_I_K 0
#define UD_APGD_I_CNT 1
#define UD_APGD_I_HALVED 2
#define UD_APGD_I_IMPROVED 3
#define UD_APGD_I_RESET 4
#define UD_APGD_F_PREV 0
#define UD_APGD_F_BEST 1
#define UD_APGD_F_CKPT 2
#define UD_APGD_F_ETA 3
#define UD_APGD_F_A 4
int ud_apgd_control(const float* f, int* ist, float* fst, float* history, int N, int steps, const int* ck_w,
                    const int* ck_thr, int n_ck, float eta0, float alpha, int closing, ud_stream_t stream);
int ud_apgd_update_linf(float* x, float* x_prev, float* x_best, float* g_best, const float* x0, const float* g, const int* ist,
                        const float* fst, int N, long per, float eps, float lo, float hi, ud_stream_t stream);
int ud_apgd_keep(float* dst, const float* src, const int* flag, int N, long per, ud_stream_t stream);
int ud_apgd_step_l2(float* x, float* z, float* x_best, float* g_best, double* gss_best, const float* g, const double* gss,
                    const int* ist, const float* fst, int N, long per, ud_stream_t stream);
int ud_apgd_combine_l2(float* x, float* x_prev, const float* z, const float* fst, int N, long per, ud_stream_t stream);
int ud_apgd_project_l2(float* x, const float* x0, const double* dss, const float* fst, int N, long per, float eps, float lo,
                       float hi, ud_stream_t stream);

/* ---- Fast Minimum-Norm attack (csrc/fmn.hip; unidefense_amd/attack.py: FMNRunner) ------------------------------------
 * The smallest perturbation that makes each sample adversarial (objective f < 0), norm UD_FMN_LINF or UD_FMN_L2.  The budget
 * eps is per-sample device state, so that one iteration is a static launch sequence inside a captured graph:
 *   ist [3][N] int32 : rows UD_FMN_I_K (iteration index), _FOUND (some iterate was adversarial), _IMPROVED (this iterate is
 *                      the sample's best: what ud_fmn_update and ud_apgd_keep obey)
 *   fst [2][N] fp32  : rows UD_FMN_F_EPS (the budget of this iteration's projection), _BEST (the smallest adversarial norm)
 *   fac [N] double   : alpha_k / max(|g|_2, 1e-12), the factor of this iteration's step
 *   history [steps + 1][N] fp32 : row k = f_k, row steps = f of the closing evaluation;  eps_history [steps][N] fp32: eps_k
 *   alpha, gamma [steps] fp32 (device tables, indexed with the sample's own counter), worst [N] fp32 (the cap on eps)
 * ud_fmn_norm_parts: x, x0, g fp32 [N][per].  For part p (UD_FMN_CHUNK elements) of sample n, ws[(n parts + p) UD_FMN_PARTS +
 *   j], parts = ceil(per / UD_FMN_CHUNK), holds as doubles j = UD_FMN_P_GSS: sum g^2, _GABS: sum |g|, _DSS: sum (x - x0)^2,
 *   _DMAX: max |x - x0|.  Differences, squares and sums in double; the maximum keeps a NaN; a fixed tree (thread order, wave
 *   shuffles, waves in order), no atomics.  g == NULL writes the two d entries only.  float4 loads where per % 4 == 0 and all
 *   bases are 16-byte aligned, scalar loads otherwise.  ws holds ud_fmn_norms_ws_bytes(N, per) bytes (ws_bytes: what the
 *   caller holds); there is no fold launch: ud_fmn_control adds a sample's parts itself.
 * ud_fmn_control: f [N] fp32 at the current point, ws as ud_fmn_norm_parts left it.  One thread per sample, every operation
 *   below in double with one rounding (no contraction) unless it says fp32; (float) is round-to-nearest-even:
 *     GSS, GABS, DSS = 0.0 + part 0 + part 1 + ... in index order;  DMAX = m(... m(m(0.0, part 0), part 1) ...) with
 *     m(a, v) = v if v is NaN or v > a, else a;       dn = (float)(l2 ? sqrt(DSS) : DMAX)      (sqrt correctly rounded)
 *     k = ist[K][n]; k outside [0, steps) writes nothing.  k == 0: eps = best = +inf (fp32), found = 0; else as stored.
 *     adv = f < 0 (fp32);  improved = adv && dn < best (fp32);  improved: best = dn
 *     g = (double)gamma[k], E = (double)eps, q = l2 ? sqrt(GSS) : GABS
 *     adv: t = E (1 - g); e = t < (double)best ? t : (double)best       else found: e = E (1 + g)
 *     else: e = (double)dn + |(double)f| / (q < 1e-12 ? 1e-12 : q)
 *     w = (double)worst[n]; e = w < e ? w : e;   e == e (not NaN): eps = (float)e;   found |= adv
 *     fac[n] = (double)alpha[k] / (s < 1e-12 ? 1e-12 : s), s = sqrt(GSS)          (a NaN norm gives a NaN factor)
 *     stored: fst[EPS] = eps, fst[BEST] = best, ist[K] = k + 1, ist[FOUND], ist[IMPROVED], history[k][n] = f, eps_history[k][n] = eps
 *   A NaN f is never adversarial.  The caller zeroes row UD_FMN_I_K to start a run.  closing != 0 (any k): the GSS / GABS
 *   entries are not read; adv, improved and best as above from the stored state; stored: fst[BEST], ist[FOUND] |= adv,
 *   ist[IMPROVED], history[steps][n] = f — nothing else.
 * ud_fmn_update: one pass over [N][per].  improved: x_best <- x.  Then t = (double)g fac[n], z = (float)((double)x - t) (product
 *   and difference rounded once each), UD_FMN_LINF: x <- clamp(clamp(z, x0 - eps[n], x0 + eps[n]), lo, hi) as
 *   ud_attack_step_linf evaluates it (an infinite eps[n] projects nothing); UD_FMN_L2: x <- z (projected by ud_sample_sumsq(x, x0)
 *   + ud_fmn_project_l2 next).  A NaN gradient element stays a NaN in x at that element.
 * ud_fmn_project_l2: ud_attack_project_l2 with the budget read per sample from fst[UD_FMN_F_EPS] (the same per-element
 *   functions: a finite equal eps gives its bits; an infinite eps leaves the clip only).
 * UD_EINVAL before any HIP call: a NULL pointer (g of ud_fmn_norm_parts excepted), N < 1, per < 1, steps < 1, a norm that is
 * neither, lo > hi or NaN, ws_bytes < ud_fmn_norms_ws_bytes(N, per). */
#define UD_FMN_CHUNK 4096
#define UD_FMN_PARTS 4
#define UD_FMN_P_GSS 0
#define UD_FMN_P_GABS 1
#define UD_FMN_P_DSS 2
#define UD_FMN_P_DMAX 3
#define UD_FMN_LINF 0
#define UD_FMN_L2 1
#define UD_FMN_I_K 0
#define UD_FMN_I_FOUND 1
#define UD_FMN_I_IMPROVED 2
#define UD_FMN_F_EPS 0
#define UD_FMN_F_BEST 1
long ud_fmn_norms_ws_bytes(int N, long per);
int ud_fmn_norm_parts(const float* x, const float* x0, const float* g, int N, long per, double* ws, long ws_bytes,
                      ud_stream_t stream);
int ud_fmn_control(const float* f, const double* ws, long ws_bytes, int* ist, float* fst, double* fac, float* history,
                   float* eps_history, const float* alpha, const float* gamma, const float* worst, int N, long per, int steps,
                   int norm, int closing, ud_stream_t stream);
int ud_fmn_update(float* x, float* x_best, const float* x0, const float* g, const int* ist, const float* fst, const double* fac,
                  int N, long per, int norm, float lo, float hi, ud_stream_t stream);
int ud_fmn_project_l2(float* x, const float* x0, const double* dss, const float* fst, int N, long per, float lo, float hi,
                      ud_stream_t stream);

/* ---- Sparse minimum-norm attack (csrc/sfmn.hip; unidefense_amd/attack.py: SparseFMNRunner) ----------------------------
 * The FMN state machine above with norm UD_SFMN_L1 (the budget bounds sum |x - x0|) or UD_SFMN_L0 (it bounds the NUMBER of
 * elements with x != x0, an integer kept in fp32: per < UD_SFMN_L0_MAX_PER = 2^24).  ist [3][N], fst [2][N], fac [N], history,
 * eps_history, alpha, gamma, worst as there (rows UD_SFMN_I_*, UD_SFMN_F_*);  thr [N] double: what ud_sfmn_select leaves.
 * ud_sfmn_norm_parts: ud_fmn_norm_parts's pass, layout and tree with the four entries j = UD_SFMN_P_GSS: sum g^2, _GMAX:
 *   max |g| (keeps a NaN), _DABS: sum |x - x0|, _DCNT: the number of x != x0 as a double (a NaN differs).  g == NULL writes
 *   the two d entries only.  ws holds ud_sfmn_norms_ws_bytes(N, per) bytes.
 * ud_sfmn_control: one thread per sample, every operation in double with one rounding (no contraction) unless it says fp32:
 *     GSS, DABS, DCNT = 0.0 + part 0 + part 1 + ... in index order;  GMAX = m(... m(m(0.0, part 0), part 1) ...), m as above
 *     dn = (float)(l0 ? DCNT : DABS)
 *     k = ist[K][n]; k outside [0, steps) writes nothing.  k == 0: eps = best = +inf (fp32), found = 0; else as stored.
 *     adv = f < 0 (fp32);  improved = adv && dn < best (fp32);  improved: best = dn
 *     g = (double)gamma[k], E = (double)eps, b = (double)best, q = GMAX < 1e-12 ? 1e-12 : GMAX
 *     adv  : t = E (1 - g);  l0: t = floor(t), u = E - 1, t = u < t ? u : t;          e = t < b ? t : b
 *     else found: e = E (1 + g);  l0: e = floor(e), u = E + 1, e = u > e ? u : e
 *     else : l1: e = (double)dn + |(double)f| / q
 *            l0: c = ceil(|(double)f| / (((double)hi - (double)lo) q)), c = c < 1 ? 1 : c, e = (double)dn + c
 *                (every coordinate moves f by at most (hi - lo) max |g|: the linearised lower bound on their number)
 *     l0: e = e < 0 ? 0 : e;   w = (double)worst[n]; e = w < e ? w : e;   e == e (not NaN): eps = (float)e;   found |= adv
 *     fac[n] = (double)alpha[k] / (s < 1e-12 ? 1e-12 : s), s = sqrt(GSS)
 *     stored: as ud_fmn_control.  floor(inf) = inf.  An l0 eps is an integer or +inf at every step.
 *   closing != 0: as ud_fmn_control's (the GSS / GMAX entries are not read).
 * The step, for ud_sfmn_select and ud_sfmn_apply alike: z = (float)((double)x - (double)g fac[n]) (product and difference
 *   rounded once each), d = (double)z - (double)x0, a = |d|.
 * ud_sfmn_select: ONE workgroup (1024 threads) per sample reads the sample a bounded number of times and writes thr[n]:
 *   UD_SFMN_L1: sum a <= eps[n] (an infinite eps included): thr = -1, nothing to project.  Else eps[n] <= 0 (or NaN): thr =
 *     +inf, everything returns to x0, in one pass.  Else thr = tau with
 *     sum max(a - tau, 0) = eps: G(t) = sum_{a > t} a - |{a > t}| t is evaluated for thresholds t whose bit pattern is fixed
 *     in its top 44 bits (sign, exponent, 32 bits of the significand; the bits below all ones), two bits per pass (three
 *     thresholds each), at most 22 passes after one that sums every a: v = the smallest such t with G(t) <= eps, (C, S) =
 *     count and sum of the a above v's predecessor, tau = max((S - eps) / C, 0); C == 0: tau = +inf.  The passes stop early
 *     once no a lies between the largest t seen with G > eps and the smallest with G <= eps (equal counts above the two): C, S
 *     and tau are then the bits the remaining passes would give.  tau is within 2^-32 relative of the exact one.  Counts and
 *     sums in double: thread order, wave shuffles, waves in order.
 *   UD_SFMN_L0: kk = (integer) eps[n]; eps infinite or kk >= per: thr = -1, everything is kept; kk < 1: thr = +inf, nothing is
 *     kept (neither reads the sample).  Else thr = the
 *     (kk + 1)-th largest a counting multiplicity, exactly: a radix select on a's 64-bit pattern, 11 bits per pass, 6 passes,
 *     integer counts in LDS (integer atomics only).
 *   A NaN a counts as no element (L1) or as 0 (L0).  Every loop has a compile-time bound on its trip count: any input ends.
 * ud_sfmn_apply: one pass over [N][per].  improved: x_best <- x.  Then with z, d, a as above: a NaN a: x <- z (the NaN).
 *   thr < 0: x <- clamp(z, lo, hi).  UD_SFMN_L1: m = a - tau, m = m > 0 ? m : 0, x <- clamp((float)((double)x0 + (d < 0 ? -m :
 *   m)), lo, hi).  UD_SFMN_L0: x <- clamp(a > thr ? z : x0, lo, hi): ties at the threshold are all dropped, at most kk
 *   elements survive and no index order enters.
 * UD_EINVAL before any HIP call: a NULL pointer (g of ud_sfmn_norm_parts excepted), N < 1, per < 1, steps < 1, a norm that is
 * neither, UD_SFMN_L0 with per >= UD_SFMN_L0_MAX_PER (control, select), lo >= hi or NaN (control; apply: lo > hi),
 * ws_bytes < ud_sfmn_norms_ws_bytes(N, per). */
#define UD_SFMN_CHUNK 4096
#define UD_SFMN_PARTS 4
#define UD_SFMN_P_GSS 0
#define UD_SFMN_P_GMAX 1
#define UD_SFMN_P_DABS 2
#define UD_SFMN_P_DCNT 3
#define UD_SFMN_L1 0
#define UD_SFMN_L0 1
#define UD_SFMN_I_K 0
#define UD_SFMN_I_FOUND 1
#define UD_SFMN_I_IMPROVED 2
#define UD_SFMN_F_EPS 0
#define UD_SFMN_F_BEST 1
#define UD_SFMN_L0_MAX_PER 16777216
long ud_sfmn_norms_ws_bytes(int N, long per);
int ud_sfmn_norm_parts(const float* x, const float* x0, const float* g, int N, long per, double* ws, long ws_bytes,
                       ud_stream_t stream);
int ud_sfmn_control(const float* f, const double* ws, long ws_bytes, int* ist, float* fst, double* fac, float* history,
                    float* eps_history, const float* alpha, const float* gamma, const float* worst, int N, long per, int steps,
                    int norm, float lo, float hi, int closing, ud_stream_t stream);
int ud_sfmn_select(const float* x, const float* x0, const float* g, const float* fst, const double* fac, double* thr, int N,
                   long per, int norm, ud_stream_t stream);
int ud_sfmn_apply(float* x, float* x_best, const float* x0, const float* g, const int* ist, const double* fac, const double* thr,
                  int N, long per, int norm, float lo, float hi, ud_stream_t stream);

/* ---- Square attack, L-infinity (csrc/square.hip; unidefense_amd/attack.py: SquareRunner) ------------------------------
 * Score-based black-box search: proposal j (j = 1..steps) overwrites one side[j-1] x side[j-1] window of the trial image
 * with x0 +- eps per channel; the control keeps it where the objective f fell.  Device state, so that one iteration
 * (propose, forward, f, control) is a static launch sequence inside a captured graph:
 *   ist [4][N] int32 : rows UD_SQUARE_I_K (iteration index), _ACCEPTED (the last proposal was kept), _ACTIVE (the sample is
 *                      still searched), _QUERIES (forwards that counted for the sample)
 *   fst [1][N] fp32  : row UD_SQUARE_F_BEST (the lowest f so far)
 *   history [steps + 1][N] fp32 : row k = f_k;  decisions [steps + 1][N] int32 : row k = accepted_k (row 0 is 0)
 *   draw tables      : side [steps] int32 (1 <= side <= size), dh, dw [steps][N] int32 (0 <= dh, dw <= size - side),
 *                      dsign [steps][N][3] fp32 (+-1); row j - 1 belongs to proposal j.  A row that breaks these bounds is
 *                      skipped by the kernel, never followed out of the image.
 * ud_square_propose: x_try, x_best, x0 fp32 [N][3][size][size]; with k = ist[K][n], ONE launch does
 *   resolve (2 <= k <= steps + 1): on the window W' of proposal k - 1: accepted ? x_best[W'] = x_try[W'] : x_try[W'] = x_best[W']
 *   write   (1 <= k <= steps, closing == 0): on the window W of proposal k: x_try[c][W] = min(max(x0[c][W] + dsign[c] eps, lo), hi)
 *   (one fp32 add, NaN-transparent clamps: bitwise the torch fp32 expression).  Every element of W' u W is owned by exactly one
 *   thread, which forms the settled value and then stores x_best and x_try: identical, overlapping and disjoint consecutive
 *   windows need no ordering between threads.  Only the windows' bytes are touched.  closing != 0: resolve only.
 * ud_square_control: f [N] fp32 = the objective at x_try.  One thread per sample; with k = ist[K][n]:
 *   k == 0          : f_best = f, accepted = 0, queries = 1, active = early_stop ? f_best > 0 : 1
 *   1 <= k <= steps : queries += active; accepted = active && f < f_best (f_best follows); active as above
 *   then history[k][n] = f, decisions[k][n] = accepted, ist[K][n] = k + 1.  k outside [0, steps] writes nothing.  The caller
 *   zeroes row UD_SQUARE_I_K to start a run.  A NaN f compares false everywhere and stays in history.
 * UD_EINVAL before any HIP call: a NULL pointer, N < 1 or > 65535, size < 1 or > 32768, steps < 1, eps < 0 or NaN, lo > hi or
 * NaN. */
#define UD_SQUARE_I_K 0
#define UD_SQUARE_I_ACCEPTED 1
#define UD_SQUARE_I_ACTIVE 2
#define UD_SQUARE_I_QUERIES 3
#define UD_SQUARE_F_BEST 0
int ud_square_propose(float* x_try, float* x_best, const float* x0, const int* ist, const int* side, const int* dh,
                      const int* dw, const float* dsign, int N, int size, int steps, float eps, float lo, float hi, int closing,
                      ud_stream_t stream);
int ud_square_control(const float* f, int* ist, float* fst, float* history, int* decisions, int N, int steps, int early_stop,
                      ud_stream_t stream);

/* ---- common image corruptions (csrc/corrupt.hip; unidefense_amd/corrupt.py: corrupt, CorruptionRunner) -------------------
 * x, out fp32 [N][3][size][size], out != x.  Every corruption works on 8-bit levels and is ONE launch that reads x once and
 * writes out once:
 *   level  u = clamp(floor((x + 1) 127.5 + 0.5), 0, 255), fp32 without contraction; a NaN is level 0
 *   out    = lut[level]: lut [256] fp32 made by the host in float64 (level / 127.5 - 1)
 * and everything in between is int32 arithmetic that tests/test_corrupt_cpu.py restates in numpy bit for bit.
 * ud_corrupt_jpeg: baseline JPEG without the (lossless) entropy coding.  Pad to a multiple of 16 (4:4:4: 8) by replicating the
 *   last column and row; JFIF RGB -> YCbCr in Q16; 4:2:0: (a + b + c + d + 2) >> 2; level shift by 128; 8 x 8 DCT as two
 *   integer products with T[k][n] = round(c_k cos((2n + 1) k pi / 16) 2^13): columns (s + 2^9) >> 10, rows (s + 2^12) >> 13
 *   (eight times the coefficient); round-half-away division by 8 Q and multiplication by Q with qtab [128] int32 (luma
 *   then chroma, row-major natural order, each 1..255); inverse columns (s + 2^10) >> 11, rows (s + 2^14) >> 15; + 128, clamp;
 *   4:2:0 chroma back by the triangle filter (3/4, 1/4 in both directions, bias 8 on even and 7 on odd output columns, edges of
 *   the padded plane replicated); YCbCr -> RGB in Q16, clamp; crop.  quality (1..100) is what qtab was made for; the kernel
 *   reads qtab only.  subsampling: UD_CORRUPT_JPEG_420 or _444.
 * ud_corrupt_blur: separable k-tap blur (k odd, <= 31, size >= (k + 1) / 2), reflect-101 borders, w [k] int32 summing to
 *   2^14; per pass (sum w u + 2^13) >> 14.
 * ud_corrupt_point: mode UD_CORRUPT_CONTRAST: 128 + (((u - 128) f8 + 128) >> 8) clamped; _SATURATION: the same on Cb and Cr
 *   between the Q16 colour transforms; _NOISE: clamp(floor((u + s z) + 0.5)) with z fp32 [N][3][size][size] (one fp32 product,
 *   two fp32 sums, no contraction; a NaN gives level 0).  f8 in 0..65536 (256 = factor 1), s in [0, 65536].
 * ud_corrupt_pixelate: every factor x factor cell (1 <= factor <= 256) becomes (sum + cnt / 2) / cnt over the cnt pixels the
 *   cell has inside the image.
 * ud_corrupt_blocks: pos [N][count][2] int32 (row, column of a block's first pixel; any value): every pixel inside one of the
 *   sample's 8 x 8 blocks becomes level 128, the rest lut[u].  0 <= count <= 1024; pos may be NULL when count == 0.
 * UD_EINVAL before any HIP call: a NULL pointer, out == x, N < 1 or > 65535, size < 1 or > 32768, quality outside 1..100, an
 * unknown subsampling or mode, k even, < 1, > 31 or > 2 size - 1, factor < 1 or > 256, f8 or count out of range, s < 0 or NaN. */
#define UD_CORRUPT_JPEG_420 0
#define UD_CORRUPT_JPEG_444 1
#define UD_CORRUPT_CONTRAST 0
#define UD_CORRUPT_SATURATION 1
#define UD_CORRUPT_NOISE 2
int ud_corrupt_jpeg(const float* x, float* out, const float* lut, const int* qtab, int N, int size, int quality, int subsampling,
                    ud_stream_t stream);
int ud_corrupt_blur(const float* x, float* out, const float* lut, const int* w, int N, int size, int k, ud_stream_t stream);
int ud_corrupt_point(const float* x, float* out, const float* lut, const float* z, int N, int size, int mode, int f8, float s,
                     ud_stream_t stream);
int ud_corrupt_pixelate(const float* x, float* out, const float* lut, int N, int size, int factor, ud_stream_t stream);
int ud_corrupt_blocks(const float* x, float* out, const float* lut, const int* pos, int N, int size, int count,
                      ud_stream_t stream);

/* ---- affine warps and the worst-case spatial search (csrc/warp.hip; unidefense_amd/spatial.py: warp, SpatialRunner) --------
 * ud_warp_affine: x, out fp32 [N][3][size][size], out != x; lut [256] fp32, the corruptions' level table; mat [rows][6] int32
 *   and row [N] int32 on the device: sample n uses mat[clamp(row[n], 0, rows - 1)].  The clamp is part of the contract: both
 *   tables are device data that the host cannot see at launch, and the kernel stays in bounds for any content of either.
 *   ONE launch, defined in exact integers (int64 where written), restated in numpy by tests/test_spatial_cpu.py bit for bit:
 *     levels       u = clamp(floor((x + 1) 127.5 + 0.5), 0, 255), fp32 without contraction; a NaN is level 0
 *     coordinates  for the output pixel at row r, column c: X = 2c + 1 - size, Y = 2r + 1 - size (centred half pixels); with
 *                  (m00, m01, o0, m10, m11, o1) the sample's row of mat:
 *                    px = (m00 X + m01 Y + o0 + ((size - 1) << 16)) >> 1,  py = (m10 X + m11 Y + o1 + ((size - 1) << 16)) >> 1
 *                  in int64 with arithmetic shift: the source column and row in Q16 pixels
 *     taps         x0 = px >> 16, fx = (px >> 8) & 255, y0 and fy likewise; the four taps (y0 | y0 + 1, x0 | x0 + 1), each index
 *                  through the border rule on its own:
 *                    UD_WARP_REFLECT  reflect-101: j = i mod 2 (size - 1) (mathematical mod, any distance), j = 2 (size - 1) - j
 *                                     where j >= size; size == 1: index 0
 *                    UD_WARP_EDGE     clamp to 0 .. size - 1
 *                    UD_WARP_FILL     a tap whose row or column lies outside has level 128
 *     interpolation v = ((256 - fx)(256 - fy) u00 + fx (256 - fy) u01 + (256 - fx) fy u10 + fx fy u11 + 32768) >> 16: fits int32,
 *                  needs no clamp
 *     output       out = lut[v]
 *   The host makes a row of mat from the inverse of p_out = scale R(angle) diag(flip ? -1 : 1, 1) p_src + shift in float64:
 *   m = floor(A^-1 65536 + 0.5), o = floor(2 (-A^-1 shift) 65536 + 0.5) (spatial.affine_q16).
 * ud_spatial_control: the per-sample state of a search over K candidates, one thread per sample, so that one query (warp,
 *   forward, f, control) is a static launch sequence inside a captured graph:
 *     ist [3][N] int32 : rows UD_SPATIAL_I_K (the sample's counter), _BEST_K (the candidate with the lowest f), _ROW (the row of
 *                        mat [K N][6] the next warp reads for the sample: ud_warp_affine's `row` is this row of ist)
 *     fst [1][N] fp32  : row UD_SPATIAL_F_BEST (the lowest f so far)
 *     history [K][N] fp32 : row k = f of candidate k
 *   closing == 0, with k = ist[K][n] in [0, K): history[k][n] = f[n]; where k == 0 or f[n] < f_best[n] (strict: a tie keeps the
 *   lowest k, a NaN never wins) f_best[n] = f[n], best_k[n] = k; row[n] = min(k + 1, K - 1) N + n; ist[K][n] = k + 1.  k outside
 *   [0, K) writes nothing.  The caller zeroes the state and sets row[n] = n to start a run.
 *   closing != 0: only row[n] = clamp(best_k[n], 0, K - 1) N + n (f, fst, history may be NULL).
 * UD_EINVAL before any HIP call: a NULL pointer, out == x, N < 1 or > 65535, size < 1 or > 32768, rows < 1, an unknown border;
 * K < 1, N < 1, K N > 2^31 - 1. */
#define UD_WARP_REFLECT 0
#define UD_WARP_EDGE 1
#define UD_WARP_FILL 2
#define UD_SPATIAL_I_K 0
#define UD_SPATIAL_I_BEST_K 1
#define UD_SPATIAL_I_ROW 2
#define UD_SPATIAL_F_BEST 0
int ud_warp_affine(const float* x, float* out, const float* lut, const int* mat, const int* row, int N, int size, int rows,
                   int border, ud_stream_t stream);
int ud_spatial_control(const float* f, int* ist, float* fst, float* history, int K, int N, int closing, ud_stream_t stream);

/* ---- universal perturbation (csrc/universal.hip; unidefense_amd/universal.py: UniversalRunner) -----------------------------
 * ONE pattern delta [per] fp32 shared by all N samples of contiguous fp32 [N][per] batches; an iteration is a static launch
 * sequence inside a captured graph: forward + d/dx, control, reduce, update.
 * ud_uap_control: one thread per sample.  ist [1][N] int32, row UD_UAP_I_K: the sample's iteration counter (the caller zeroes it
 *   to start a run).  With k = ist[K][n] in [0, steps): history[k][n] = f[n] (fp32 [steps][N]);
 *   w[n] = (f[n] < beta) && (source < 0 || y[n] == source) as 0 / 1 (int32 [N]; y int64 [N]; a NaN f gives 0; beta = +inf counts
 *   everyone); counted[k][n] = w[n] (int32 [steps][N]); ist[K][n] = k + 1.  k outside [0, steps) writes nothing.
 * ud_uap_reduce: gsum[e] = sum over n with w[n] != 0 of g[n][e], added in ascending n from 0.f, one fp32 add per term and no
 *   fused multiply-add: a float32 loop on the host reproduces it to the bit.  An excluded sample's row is not read (its NaN
 *   does not leak); a counted sample's NaN stays.  No sample counted: gsum = 0.  One thread per element, float4 per thread where
 *   per % 4 == 0 and g, gsum are 16-byte aligned; no workspace.
 * ud_uap_update_linf: one pass: delta[e] <- clamp(delta[e] + step sign(gsum[e]), -eps, eps), then for every n
 *   x_adv[n][e] = clamp(x[n][e] + delta[e], lo, hi); one fp32 rounding per operation in this order (bitwise the torch fp32
 *   expression), sign(0) = 0, a NaN in gsum becomes a NaN in delta at that element.
 * ud_uap_apply: dss != NULL (one double, |delta|^2 from ud_sample_sumsq(delta, NULL, 1, per)): delta is first scaled in place
 *   by min(1, eps / max(sqrt(dss[0]), 1e-12)), product formed in double and rounded once; a factor of exactly 1 leaves it
 *   untouched.  Then x_adv[n][e] = clamp(x[n][e] + delta[e], lo, hi) for every n; dss == NULL: only that, delta is not written.
 *   x_adv may be x itself (no other overlap).  The L2 step on delta itself is ud_sample_sumsq(gsum) + ud_attack_step_l2(delta, gsum, gss, 1, per, step).
 * UD_EINVAL before any HIP call: a NULL pointer (but dss), N < 1 or > 65535, per < 1, steps < 1, steps N > 2^31 - 1, a NaN beta
 * or step, eps < 0 or NaN, lo > hi or NaN. */
#define UD_UAP_I_K 0
int ud_uap_control(const float* f, const long long* y, int* w, int* ist, float* history, int* counted, int N, int steps,
                   float beta, int source, ud_stream_t stream);
int ud_uap_reduce(const float* g, const int* w, float* gsum, int N, long per, ud_stream_t stream);
int ud_uap_update_linf(float* delta, const float* gsum, const float* x, float* x_adv, int N, long per, float step, float eps,
                       float lo, float hi, ud_stream_t stream);
int ud_uap_apply(float* delta, const double* dss, const float* x, float* x_adv, int N, long per, float eps, float lo, float hi,
                 ud_stream_t stream);

/* ---- adversarial patch (csrc/patch.hip; unidefense_amd/patch.py: paste, PatchRunner) ------------------------------------------
 * ONE texture patch fp32 [3][P][P] with a fixed coverage mask alpha fp32 [P][P] in [0, 1], pasted into every sample of x fp32
 * [N][3][S][S] under the sample's own placement.  table [rows][N][UD_PATCH_ROW] int32 and k (one int32) are DEVICE data: sample n
 * uses the row table[clamp(k[0], 0, rows - 1)][n].  The clamp is part of the contract, as are reach clamped into
 * [0, UD_PATCH_MAX_REACH], the window cut to the image and every tap tested against the texture: the host cannot see the table
 * at launch, and the kernels stay in bounds for any content of it.  (The host side that MAKES a table, patch.placement_q16 and
 * patch.check_table, refuses a row with reach > UD_PATCH_MAX_REACH or a non-zero reserved word before it is uploaded.)
 * A row (patch.placement_q16), pixel and texel centres on the integers, x to the right, y down, t0 = (P - 1) / 2, the forward
 * map p = s R(angle) (t - t0) + centre, made in float64 and quantised as floor(v 65536 + 0.5):
 *     words 0..5   m00 m01 o0 m10 m11 o1: the INVERSE map, texel column = m00 c + m01 r + o0, texel row = m10 c + m11 r + o1
 *     words 6..11  the FORWARD map likewise: pixel column from (texel column j, texel row i), then the pixel row
 *     word  12     reach = floor(s sqrt(2) (1 + 2^-7)) + 2;   words 13..15 zero
 * Weights.  For the output pixel (r, c): U = m00 c + m01 r + o0, V = m10 c + m11 r + o1 in int64; j0 = U >> 16, fx = (U >> 8) & 255,
 *   i0 = V >> 16, fy = (V >> 8) & 255 (arithmetic shifts).  The four taps, in this order: (i0, j0), (i0, j0 + 1), (i0 + 1, j0),
 *   (i0 + 1, j0 + 1), with the integer weights w = wx wy / 65536, wx = 256 - fx | fx, wy = 256 - fy | fy: exact dyadics.  The tap
 *   weight is omega = fl32(w alpha[i][j]), ONE rounding, the only weight either direction uses.  A tap outside [0, P - 1]^2 is
 *   absent, and so is a tap whose omega is zero (so a NaN texel shows exactly where it has weight).
 * ud_patch_paste: cov = sum omega, acc_ch = sum omega patch[ch][i][j], both fp32 from 0.f over the present taps in tap order,
 *   the product rounded, then the sum, no fused multiply-add; out = clamp((1 - cov) x + acc, lo, hi) (difference, product, sum:
 *   one rounding each; the clamp keeps a NaN).  A pixel with no present tap, or cov == 0, gets x's own bits, unclamped.  One
 *   launch, one thread per pixel for the three channels; x is only read; out != x.
 * ud_patch_grad: the adjoint with respect to the texture, per sample, as a GATHER.  For sample n and the texel (i, j): the pixel
 *   nearest its forward image, pc = (f00 j + f01 i + fo0 + 32768) >> 16, pr likewise (int64); the window [pr - reach, pr + reach] x
 *   [pc - reach, pc + reach] cut to the image, walked in row-major order; every candidate pixel evaluates the weights above and
 *   keeps the tap that names (i, j), if any; gp[n][ch][i][j] = fl32(sum of (double) omega (double) g[n][ch][r][c]), the sum in
 *   double in the walk's order, rounded ONCE.  Every element of gp fp32 [N][3][P][P] is written, zeros included.  No atomics, no
 *   workspace: a replay gives the same bits.  gp != g.
 * ud_patch_update: patch[e] <- clamp(patch[e] + step sign(gsum[e]), lo, hi) for e < per, sign(0) = 0, a NaN in gsum becomes a NaN
 *   in patch: bitwise the torch fp32 expression.  gsum != patch.
 * UD_EINVAL before any HIP call: a NULL pointer, out == x, gp == g, gsum == patch, N < 1 or > 65535, S < 2 or > 32768, P < 1 or
 * > 256, rows < 1, per < 1 or > 3 256^2, lo > hi or NaN, a NaN step. */
#define UD_PATCH_ROW 16
#define UD_PATCH_MAX_REACH 8
int ud_patch_paste(const float* x, const float* patch, const float* alpha, const int* table, const int* k, int rows, float* out,
                   int N, int S, int P, float lo, float hi, ud_stream_t stream);
int ud_patch_grad(const float* g, const float* alpha, const int* table, const int* k, int rows, float* gp, int N, int S, int P,
                  ud_stream_t stream);
int ud_patch_update(float* patch, const float* gsum, long per, float step, float lo, float hi, ud_stream_t stream);

/* ---- frequency-band attack (csrc/band.hip; unidefense_amd/band.py: dct2, idct2, BandRunner) -----------------------------------
 * ud_plane_dct2: the orthonormal 2-D DCT-II of P contiguous fp32 planes [P][S][S], 2 <= S <= 480, any S in between (odd, no
 *   multiple of 32).  d is D [S][S] row-major (D[u][i] = c_u cos(pi (2 i + 1) u / (2 S)), made in float64 and rounded once), dt
 *   its transpose, also row-major.  inverse == 0: y_p = mask (.) (D x_p D^T); inverse != 0: y_p = D^T (mask (.) x_p) D.  mask
 *   [S][S] fp32 may be NULL (bitwise a mask of ones); it multiplies, so a 0 entry gives +-0.  The inverse takes base [P][S][S]
 *   with clip != 0: y_p = clamp(base_p + D^T (mask (.) x_p) D, lo, hi), one fp32 rounding for the sum, a NaN kept.  Products are
 *   exact fp32 on the fp32-input MFMA, fp32 accumulation, in an order that depends on S alone: a second launch gives the same
 *   bits.  One workgroup per (plane, 32-column strip), the strip of the intermediate in LDS; no workspace.  x is only read.
 *   16-byte loads where S % 4 == 0 and the bases are 16-byte aligned, element loads otherwise.
 * ud_band_dots: out[n][0..2] = |w[n]|^2, <w[n], g[n]>, |g[n]|^2 for contiguous fp32 [N][per], products and sums in double, one
 *   pass.  per is cut into fixed 4096-element parts as ud_sample_sumsq cuts it; with more than one part the partial sums go to
 *   ws (3 ud_sample_sumsq_ws_bytes(N, per) bytes, 0 for one part) and are folded in part order: deterministic.
 * ud_band_update: in place, with the sample's dots (ww, wg, gg) = dots[n][0..2], all in double and unfused:
 *   a = step / max(sqrt(gg), 1e-12); n2 = ww + 2 a wg + a a gg; s = min(1, eps / max(sqrt(max(n2, 0)), 1e-12));
 *   w[n][e] <- (float)(s ((double)w[n][e] + a (double)g[n][e])): the normalised step and the projection onto |w|_2 <= eps in
 *   one pass, because the stepped point's norm follows from the dots of the old one.  step may be negative.
 * UD_EINVAL before any HIP call: a NULL pointer (but mask, base, ws for one part), x == y, d == dt, base == y, w == g, S < 2 or
 *   > 480, P < 1, N < 1 or > 65535, per < 1, base without clip or without inverse, clip without base, lo > hi or NaN, a NaN step,
 *   eps < 0 or NaN, a ws smaller than 3 ud_sample_sumsq_ws_bytes(N, per). */
int ud_plane_dct2(const float* x, float* y, const float* d, const float* dt, const float* mask, const float* base, long P, int S,
                  int inverse, int clip, float lo, float hi, ud_stream_t stream);
int ud_band_dots(const float* w, const float* g, int N, long per, double* out, double* ws, long ws_bytes, ud_stream_t stream);
int ud_band_update(float* w, const float* g, const double* dots, int N, long per, float step, float eps, ud_stream_t stream);

/* ---- randomized smoothing (csrc/smooth.hip; unidefense_amd/smooth.py: CertifyRunner) ----------------------------------------
 * One draw of a certificate is a static launch sequence inside a captured graph: noise, forward, vote.
 * ud_smooth_noise: out[n][e] = x[n][e] + scale noise(n, e) for contiguous fp32 [N][per]; out may be x itself (no other overlap).
 *   The noise is a pure function of (seed, ids[n], draw_n, e), draw_n = (uint32)(draw0 + (k ? k[n] : 0)); ids int64 [N] (the
 *   sample's stream id), k int32 [N] or NULL (the sample's own draw counter), seed: 64 bits.  Philox4x32-10 (multipliers
 *   0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with the key (seed low word, seed high word) and the counter
 *   (q, draw_n, id low word, id high word), q = e / 4; element 4 q + j takes output word j.  From a word w, m = w >> 8.
 *   UD_SMOOTH_UNIFORM : t = (2 m + 1 - 2^24) 2^-24, exact in fp32, symmetric, never 0, inside (-1, 1).
 *   UD_SMOOTH_GAUSSIAN: Box-Muller on the word pairs (w0, w1) -> elements (4 q, 4 q + 1) and (w2, w3) -> (4 q + 2, 4 q + 3):
 *     u1 = (m_a + 1) 2^-24 in (0, 1], u2 = m_b 2^-24, r = sqrt(-2 ln u1), t = (r cos(2 pi u2), r sin(2 pi u2)), |t| <= 5.77;
 *     logf, sqrtf and sincospif(2 u2), not the fast intrinsics.
 *   out = x + scale t with one fp32 product and one fp32 add, not contracted (uniform: bitwise a float32 host expression).  A
 *   NaN in x stays a NaN at its own element.  One thread per quad; a float4 per thread where per % 4 == 0 and both bases are
 *   16-byte aligned, scalar accesses otherwise (the tail quad of another per uses its first words): the same bits either way.
 * ud_smooth_vote: one thread per sample.  ist [1][N] int32, row UD_SMOOTH_I_K: the sample's draw counter (the caller zeroes it).
 *   With d = ist[K][n] in [0, draws): the class is the first maximum of logits[n][0..C) (C == 1: logit > 0), Ce = max(C, 2);
 *   votes[d][n] = the class, or -1 if any logit of the row is NaN (int32 [draws][N]); margins[d][n] = the top logit minus the
 *   runner-up (C == 1: |logit|; an invalid row: NaN; fp32 [draws][N]); counts[d < n0 ? 0 : 1][n][class] += 1 for a valid row
 *   (int32 [2][N][Ce]); ist[K][n] = d + 1.  d outside [0, draws) writes nothing.  No atomics: a thread touches its sample only.
 * UD_EINVAL before any HIP call: a NULL pointer (but k), N < 1 or > 65535, per < 1 or > 2^34, an unknown mode, scale < 0 or NaN;
 * C < 1, draws < 1, n0 outside [0, draws], draws N or 2 N Ce > 2^31 - 1. */
#define UD_SMOOTH_I_K 0
#define UD_SMOOTH_GAUSSIAN 0
#define UD_SMOOTH_UNIFORM 1
int ud_smooth_noise(const float* x, float* out, const long long* ids, const int* k, int draw0, int N, long per, int mode,
                    float scale, long seed, ud_stream_t stream);
int ud_smooth_vote(const float* logits, int N, int C, int* ist, int* counts, int* votes, float* margins, int draws, int n0,
                   ud_stream_t stream);

/* ---- flow-field (stAdv) attack on a differentiable warp (csrc/flow.hip; unidefense_amd/flow.py: flow_warp, FlowRunner) --------
 * x, out, g, x_adv fp32 [N][3][S][S]; w, w_best, gw fp32 [N][2][S][S], a displacement per output pixel in pixels: channel 0 the
 * column displacement, channel 1 the row displacement.  Every kernel is one launch, one thread per pixel for the three channels,
 * pixel-local gathers with ordinary vector loads and stores: no atomics, no workspace, a replay gives the same bits.  Every fp32
 * operation below is rounded once, in the order written, without contraction.
 * The cell of the output pixel (r, c):  qx = (float)c + w0 (one rounding; everything below starts from this fp32 value),
 *   px = min(max(qx, 0), S - 1), x0 = min(floor(px), S - 2), fx = px - x0 in [0, 1] (floor and the difference are exact);
 *   qy, py, y0, fy likewise from r and w1.  A NaN qx (qy) takes the cell 0 and fx (fy) = NaN: it is replaced BEFORE the
 *   conversion to an integer, and the integer is clamped to [0, S - 2] once more, so every tap index lies in [0, S - 1] for ANY
 *   content of w (NaN, +-inf, huge values).  The taps u_ab = x[ch][y0 + a][x0 + b].
 * ud_flow_warp: out[ch] = (1 - fy) ((1 - fx) u00 + fx u01) + fy ((1 - fx) u10 + fx u11), out != x: at most FIVE roundings on a
 *   path (1 - fx, the product, the sum, the product with 1 - fy, the sum).  A zero flow returns a finite x (a -0.0 as +0.0); a
 *   NaN component of w gives NaN at that pixel only.
 * ud_flow_grad: gw = sign (gx, gy) - tau t, sign = +1 (ascend) or -1 (targeted), with g = dL/dout:
 *     gx = 0 < qx < S - 1 ? sum_ch g[ch] ((1 - fy) (u01 - u00) + fy (u11 - u10)) : 0      (strict, as torch's grid_sample)
 *     gy = 0 < qy < S - 1 ? sum_ch g[ch] ((1 - fx) (u10 - u00) + fx (u11 - u01)) : 0
 *   the channel sum from ch = 0 upwards (six roundings on a path), and t the gradient at p of the smoothness term
 *   L_flow = sum over the unordered horizontal and vertical neighbour pairs (p, q) of sqrt(|w(p) - w(q)|^2 + tv_eps):
 *     t = sum over q in (left, right, up, down) inside the image of d / sqrt(d0 d0 + d1 d1 + tv_eps), d = w(p) - w(q),
 *   added in that order from 0 (ten roundings on a path), then tau t and the difference: TWELVE roundings on the longest path.
 *   It reads w's neighbours: gw must not be w.
 * ud_flow_control: one thread per sample, so that an iteration is a static launch sequence inside a captured graph.
 *     ist [2][N] int32 : rows UD_FLOW_I_K (the sample's counter; the caller zeroes it to start a run), UD_FLOW_I_KEEP
 *     fst [1][N] fp32  : row UD_FLOW_F_BEST (the best f so far);  history [steps + 1][N] fp32: row k = f of candidate k
 *   With k = ist[K][n] in [0, steps]: history[k][n] = f[n]; keep = k == 0 || better(f, best) || (isnan(best) && !isnan(f)),
 *   better strict > (maximise != 0) or < (maximise == 0): a tie keeps the earliest k, a NaN wins only at k == 0; where keep,
 *   best = f; ist[KEEP][n] = keep; ist[K][n] = k + 1.  A k outside [0, steps] writes nothing but KEEP = 0.
 * ud_flow_update: one pass.  Where keep[n] != 0 (ud_flow_control's KEEP row): w_best(p) = w(p), the flow that produced the f just
 *   judged.  closing == 0: w(p) <- min(max(w(p) + step sign(gw(p)), -bound), bound) per component, sign(0) = 0, a NaN stays
 *   (bitwise torch's fp32 clamp(w + step sign(gw), -bound, bound)), then x_adv(p) = ud_flow_warp's value at p for the new w.
 *   closing != 0: w and gw are not touched (gw may be NULL) and x_adv(p) = ud_flow_warp's value at p for w_best.
 *   x_adv != x, w_best != w, gw neither of them.
 * UD_EINVAL before any HIP call: a NULL pointer, out == x, gw == w or w_best, x_adv == x, w_best == w, N < 1 or > 65535, S < 2 or > 32768,
 * sign not +-1, tau < 0 or not finite, tv_eps <= 0 or not finite, a NaN step, bound < 0 or NaN; steps < 1, (steps + 1) N > 2^31 - 1. */
#define UD_FLOW_I_K 0
#define UD_FLOW_I_KEEP 1
#define UD_FLOW_F_BEST 0
int ud_flow_warp(const float* x, const float* w, float* out, int N, int S, ud_stream_t stream);
int ud_flow_grad(const float* g, const float* x, const float* w, float* gw, int N, int S, int sign, float tau, float tv_eps,
                 ud_stream_t stream);
int ud_flow_control(const float* f, int* ist, float* fst, float* history, int steps, int N, int maximise, ud_stream_t stream);
int ud_flow_update(float* w, float* w_best, const float* gw, const int* keep, const float* x, float* x_adv, int N, int S,
                   float step, float bound, int closing, ud_stream_t stream);

/* ---- decision-based minimum-norm attack, HopSkipJump (csrc/hsj.hip; unidefense_amd/hsj.py: HSJRunner) ----------------------
 * A query is a static launch sequence inside a captured graph: propose(mode), forward, control(mode).  All samples walk ONE
 * schedule that the host knows; what differs per sample is device state, one column per sample:
 *   ist [13][N] int32: UD_HSJ_I_ACTIVE (still attacked), _HAS (an adversarial start is known; live = ACTIVE and HAS), _MOVED (the
 *     bisection's upper end has moved), _STEPDONE (the step search has succeeded), _ACCEPT (the point just judged becomes x_cur:
 *     the flag of the ud_apgd_keep that follows), _KEEP (the settled point is the best so far: likewise for x_adv), _K (the next
 *     row of decisions), _DRAW (the next noise draw: ONE counter for the whole call, so no direction is used twice), _PB (the
 *     next row of phi), _T (the iteration), _QUERIES (forwards that counted), _FLAGS (bit 0: a counted row held a NaN), _DONE0
 *     (the clean input is already misclassified)
 *   fst [8][N] fp32: UD_HSJ_F_LO, _HI (the bisection's interval of alpha: HI is the adversarial end), _DELTA (probe size), _XI
 *     (step size), _INVN (1 / |v|, L2), _DIST (the settled point's distance), _BEST (the least so far), _RADIUS (what the call
 *     returns: BEST, 0 for DONE0, +inf without a start)
 *   The caller zeroes ist and fst to start a call; UD_HSJ_C_CLEAN initialises the rest.
 * Every fp32 expression below is rounded once per operation, in the order written, without contraction; clamp is NaN-transparent.
 * ud_hsj_propose(mode): contiguous fp32 [N][per]; dst is never a or b.  One thread per quad of four elements, a float4 where
 *   per % 4 == 0 and the bases are 16-byte aligned, scalar accesses otherwise: the same bits.  A sample that does not take part
 *   is left after reading its state.  With m = 0.5 (lo + hi), h = 0.5 (hi - lo):
 *   UD_HSJ_P_COPY      every sample            dst = a
 *   UD_HSJ_P_COPY_SEEK ACTIVE and not HAS      dst = a
 *   UD_HSJ_P_NOISE     ACTIVE and not HAS      dst = clamp(m + h t, lo, hi), t the uniform noise of (seed, ids[n], DRAW, e)
 *   UD_HSJ_P_BISECT    live                    dst = point(0.5 (LO + HI)), with a = x_cur, b = x0 and
 *                        UD_HSJ_L2:   point(s) = clamp(b + s (a - b), lo, hi)
 *                        UD_HSJ_LINF: point(s) = clamp(clamp(a, b - s, b + s), lo, hi)
 *   UD_HSJ_P_SETTLE    live                    dst = MOVED ? point(HI) : a    (x_cur itself has been verified, point(1) has not)
 *   UD_HSJ_P_PROBE     live                    dst = clamp(a + s t, lo, hi); LINF: s = DELTA, t uniform; L2: s = DELTA aux
 *                                              (aux = 1 / sqrt(per) as fp32), t Gaussian; the draw is DRAW
 *   UD_HSJ_P_STEP      live and not STEPDONE   dst = clamp(a + s b, lo, hi), b = v; LINF: s = XI; L2: s = XI INVN
 *   The noise: ud_smooth_noise's Philox4x32-10 words, key (seed low, seed high), counter (e / 4, draw, id low, id high), and its
 *   uniform rule, bit for bit.  The Gaussian rule is NOT ud_smooth_noise's: the same Box-Muller on the same exact uniforms, but
 *   with log, sqrt and sincospi in DOUBLE and ONE rounding of r cos / r sin to fp32 (ud_smooth_noise: logf, sqrtf, sincospif).
 *   The fp32 value is then float32(float64 Box-Muller) but for about one element in 10^8, which lets a host restatement
 *   reproduce a whole attack's decisions; the two kernels' Gaussian fields for one counter differ in the last bits.
 * ud_hsj_control(mode): one thread per sample.  UD_HSJ_C_CLEAN .. _STEP judge logits [N][C]: the class is the first maximum
 *   (C == 1: logit > 0), bit = class != y[n] (y int64), a row with a NaN gives bit 0 and, where the sample takes part, FLAGS |= 1.
 *   From there on only the bit is used.  ACCEPT = 0 first; a sample that takes part counts the query; then
 *   _CLEAN       every sample: QUERIES = 1, DONE0 = bit, ACTIVE = !bit, HAS = 0, BEST = +inf
 *   _START       ACTIVE and not HAS: bit -> HAS = ACCEPT = 1;  _START_NOISE: the same, and DRAW += 1 for every sample
 *   _BISECT      live: mid = 0.5 (LO + HI); bit ? (HI = mid, MOVED = 1) : LO = mid
 *   _PROBE       live: phi[PB][n] = bit (int8 [max_probes][N]); PB += 1 and DRAW += 1 for every sample
 *   _STEP        live and not STEPDONE: bit ? STEPDONE = ACCEPT = 1 : XI = 0.5 XI
 *   and decisions[K][n] = bit, or -1 for a sample that took no part (int8 [Q][N]); K += 1 for every sample.
 *   The other modes read nrm [2][N] double (ud_hsj_dist) and no logits:
 *   _BEGIN       ACTIVE and not HAS -> ACTIVE = 0; live: LO = 0, HI = L2 ? 1 : (float)max, MOVED = 0
 *   _DIST        live: dist = (float)(L2 ? sqrt(sumsq) : max); KEEP = dist < BEST (BEST follows); ACCEPT = 1; DELTA = max(T == 0 ?
 *                delta0 : dist inv_d, dfloor); XI = dist xis[T] (xis fp32 [steps]); STEPDONE = 0.  Every sample: PB = 0, RADIUS =
 *                history[T][n] = live ? BEST : (DONE0 ? 0 : +inf) (fp32 [steps + 1][N]), T += 1
 *   _VNORM       live: INVN = L2 ? (sumsq > 0 ? (float)(1 / sqrt(sumsq)) : 0) : 1
 *   A counter outside its table writes no row.
 * ud_hsj_dist: out[n] = sum_e (a - b)^2, out[N + n] = max_e |a - b|, differences, squares and sums in double (b NULL: of a), one
 *   workgroup per sample and a fixed order; ist given: a sample with ACTIVE == 0 is skipped.
 * ud_hsj_estimate: live samples (ist NULL: all): v[n][e] = sum over b = 0 .. B - 1, ascending, of w_b u_b[e], one fp32 product and
 *   one fp32 add per term; u_b the noise of draw draw0 + b as ud_hsj_propose makes it (LINF uniform, L2 the double Box-Muller); w_b = phi[b][n] - mean, mean = (float)ones
 *   inv_b; all phi equal: w_b = +1 (all ones) or -1 (all zeros).  LINF: the sign of the sum (+-1, 0) is written.  The B
 *   directions are re-made in registers, the weights held in LDS: the pass reads phi and writes v, nothing else; B <= 4096.
 * UD_EINVAL before any HIP call: a NULL pointer that the mode reads, N < 1 or > 65535, per < 1 or > 2^34, an unknown mode or
 * norm, lo >= hi or NaN, dst == a or b, C < 1, Q < 1, Q N or (steps + 1) N > 2^31 - 1, max_probes or B outside [1, 4096],
 * delta0, inv_d or dfloor <= 0 or NaN, draw0 < 0. */
#define UD_HSJ_MAX_PROBES 4096
#define UD_HSJ_LINF 0
#define UD_HSJ_L2 1
#define UD_HSJ_I_ACTIVE 0
#define UD_HSJ_I_HAS 1
#define UD_HSJ_I_MOVED 2
#define UD_HSJ_I_STEPDONE 3
#define UD_HSJ_I_ACCEPT 4
#define UD_HSJ_I_KEEP 5
#define UD_HSJ_I_K 6
#define UD_HSJ_I_DRAW 7
#define UD_HSJ_I_PB 8
#define UD_HSJ_I_T 9
#define UD_HSJ_I_QUERIES 10
#define UD_HSJ_I_FLAGS 11
#define UD_HSJ_I_DONE0 12
#define UD_HSJ_F_LO 0
#define UD_HSJ_F_HI 1
#define UD_HSJ_F_DELTA 2
#define UD_HSJ_F_XI 3
#define UD_HSJ_F_INVN 4
#define UD_HSJ_F_DIST 5
#define UD_HSJ_F_BEST 6
#define UD_HSJ_F_RADIUS 7
#define UD_HSJ_P_COPY 0
#define UD_HSJ_P_COPY_SEEK 1
#define UD_HSJ_P_NOISE 2
#define UD_HSJ_P_BISECT 3
#define UD_HSJ_P_SETTLE 4
#define UD_HSJ_P_PROBE 5
#define UD_HSJ_P_STEP 6
#define UD_HSJ_C_CLEAN 0
#define UD_HSJ_C_START 1
#define UD_HSJ_C_START_NOISE 2
#define UD_HSJ_C_BISECT 3
#define UD_HSJ_C_PROBE 4
#define UD_HSJ_C_STEP 5
#define UD_HSJ_C_BEGIN 6
#define UD_HSJ_C_DIST 7
#define UD_HSJ_C_VNORM 8
int ud_hsj_propose(int mode, int norm, float* dst, const float* a, const float* b, const long long* ids, const int* ist,
                   const float* fst, int N, long per, float lo, float hi, float aux, long seed, ud_stream_t stream);
int ud_hsj_control(int mode, int norm, const float* logits, int C, const long long* y, const double* nrm, int* ist, float* fst,
                   char* phi, char* decisions, float* history, const float* xis, int N, int Q, int max_probes, int steps,
                   float delta0, float inv_d, float dfloor, ud_stream_t stream);
int ud_hsj_dist(const float* a, const float* b, const int* ist, int N, long per, double* out, ud_stream_t stream);
int ud_hsj_estimate(float* v, const char* phi, const long long* ids, const int* ist, int N, long per, int B, int draw0, int norm,
                    float inv_b, long seed, ud_stream_t stream);

/* ---- attribution: integrated gradients and the deletion / insertion score (csrc/attrib.hip; unidefense_amd/attrib.py) ---------
 * x, b, xp, g, attr, xq contiguous fp32 [N][per], per = 3 S^2 (b: the baseline, one per sample: the host expands a shared one);
 * acc float64 [N][per]; heat fp32 [N][S^2].  One iteration of the path integral is a static launch sequence inside a captured
 * graph: point, (noise,) forward + d/dx, accumulate, control; k int32 [N] is the sample's iteration counter (row UD_ATTR_I_K of
 * ist [1][N], which the caller zeroes to start a run) and `iters` the length of the run: iteration k takes node k % steps.
 * The element-wise kernels give one thread a quad of four consecutive elements (finish, mask: pixels): a float4 per thread where
 * the length is a multiple of 4 and every base is 16-byte aligned, scalar accesses otherwise, the same bits either way.  Every
 * expression is rounded once per operation, in the order written, without contraction.  No floating-point atomics: a replay
 * gives the same bits.
 * ud_attr_point: a = alpha[k[n] % steps] (alpha: an fp32 table [steps]); xp = b + a (x - b): d = x - b, m = a d, xp = b + m, three
 *   fp32 operations.  By rule, not arithmetic: a == 1 writes x bit for bit, a == 0 writes b.  A NaN in x shows at its own element
 *   only (not at a == 0).  k[n] outside [0, iters) leaves xp[n] untouched.  xp is a buffer of its own.
 * ud_attr_accumulate: acc[n][e] = acc[n][e] + (double)w[k[n] % steps] (double)g[n][e] (w: a float64 table [steps]): one double
 *   product and one double add.  A NaN in g stays at its element.  k[n] outside [0, iters) leaves acc[n] untouched.
 * ud_attr_control: one thread per sample.  With k = ist[K][n] in [0, iters): path[k][n] = f[n] (fp32 [iters][N]), ist[K][n] =
 *   k + 1.  k outside [0, iters) writes nothing.  The deletion runner records its curve with it.
 * ud_attr_finish: per element the double value v = ((double)x - (double)b) acc scale (UD_ATTR_IG: the difference, the product
 *   with acc, the product with scale) or v = acc scale (UD_ATTR_GRAD; x and b do not enter); attr = (float)v;
 *   heat[n][p] = (float)(t0 + t1 + t2), t_c = v (UD_ATTR_SUM) or |v| (UD_ATTR_ABS) at channel c of pixel p, added in double in the
 *   order 0, 1, 2; total[n] (double) = the sum over all elements of v, before the fp32 rounding.  total: a thread adds the values
 *   of its pixels (pixel by pixel, channels 0, 1, 2; its pixels in ascending order) from 0.0, a workgroup adds its threads in a
 *   fixed tree (a butterfly in each wave, then the waves in order) into ws[n][part]; the number of workgroups per sample depends
 *   on S alone; a second kernel (one thread per sample) folds the sample's partials in index order.  total[n] therefore does not
 *   depend on arrival order, on N or on the sample's row.  ws: ud_attr_finish_ws_bytes(N, 3 S^2) bytes (per must be 3 S^2).
 * ud_attr_rank_select: one workgroup per (sample n, j < K).  The key of pixel p is 64 bits: the high word is the order-preserving
 *   uint32 image of heat[n][p] (u = the bit pattern; a NaN: 0, so it ranks last; -0 as +0; otherwise u < 2^31 ? u | 2^31 : ~u), the
 *   low word is ~p: among equal heats the LOWER pixel index has the larger key, and all keys of a sample differ.  thr[j][n]
 *   (uint64 [K][N]) = the kcount[j]-th largest key (kcount int32 [K] in device memory; a value above HW counts as HW), found by a
 *   radix select of 8 passes of 8 bits on integer counts in LDS; 2^64 - 1 for kcount[j] <= 0.  Exactly kcount[j] pixels have
 *   key >= thr[j][n].
 * ud_attr_mask: j = ist[K][n]; top = key(p) >= thr[j][n].  UD_ATTR_DELETE: xq = top ? b : x at the three channels of pixel p;
 *   UD_ATTR_INSERT: xq = top ? x : b.  Copies only.  j outside [0, K) leaves xq[n] untouched.  xq is a buffer of its own.
 * UD_EINVAL before any HIP call: a NULL pointer, N < 1 or > 65535, per < 1, steps < 1, iters < 1, iters N > 2^31 - 1; S < 1 or
 * > 32768, an unknown mode or reduce, a NaN scale, ws_bytes below ud_attr_finish_ws_bytes (itself UD_EINVAL for a per that is no
 * multiple of 3 or a workspace beyond 2^31 - 1 bytes: 8 bytes per 1024 pixels, at most 8192 parts per sample); HW < 1 or > 2^30, K < 1, K N > 2^31 - 1. */
#define UD_ATTR_I_K 0
#define UD_ATTR_IG 0
#define UD_ATTR_GRAD 1
#define UD_ATTR_SUM 0
#define UD_ATTR_ABS 1
#define UD_ATTR_DELETE 0
#define UD_ATTR_INSERT 1
int ud_attr_point(const float* x, const float* b, float* xp, const int* k, const float* alpha, int steps, int iters, int N,
                  long per, ud_stream_t stream);
int ud_attr_accumulate(const float* g, double* acc, const int* k, const double* w, int steps, int iters, int N, long per,
                       ud_stream_t stream);
int ud_attr_control(const float* f, int* ist, float* path, int N, int iters, ud_stream_t stream);
int ud_attr_finish_ws_bytes(int N, long per);
int ud_attr_finish(const float* x, const float* b, const double* acc, float* attr, float* heat, double* total, double* ws,
                   long ws_bytes, int mode, int reduce, double scale, int N, int S, ud_stream_t stream);
int ud_attr_rank_select(const float* heat, const int* kcount, unsigned long long* thr, int N, long HW, int K, ud_stream_t stream);
int ud_attr_mask(const float* x, const float* b, const float* heat, const unsigned long long* thr, const int* ist, float* xq,
                 int mode, int N, int S, int K, ud_stream_t stream);

/* ---- pass-2 input perturbations (model/unidefense.py:177-198), NCHW planes x[planes][H][W], no gradients --------
 * ud_gather2d      : out[p][y][x] = in[p][iy[y]][ix[x]] — downscale (model/modules.py:19-21): the two nearest
 *                    F.interpolate calls composed into one gather (index vectors from ATen's float32 rule)
 * ud_blur5_reflect : torchvision gaussian_blur(k=5), model/modules.py:15-16: reflect pad 2, taps (k0,k1,k2,k1,k0)^2
 * ud_amp_mix       : FrequencyStyleTransfer's spectrum step (model/modules.py:44-52) on spectra laid out
 *                    [planes][2S][Whp] (rows [0,S) Re, [S,2S) Im; columns [0,S/2] valid):
 *                    out = w(kx) * (l|A| + (1-l)|B|) * exp(i angle(A)), l = lmda[plane / planes_per_sample],
 *                    w = 2 on the interior columns so the forward transform's adjoint yields irfft2
 * ud_efdm          : SpatialStyleTransfer (model/modules.py:58-76) on rows of L values:
 *                    out = (c + (1-l) * style_sorted[rank(c)]) - (1-l) * c ; ws from ud_efdm_ws_bytes (bytes, <0: bad
 *                    sizes); equal content values take the equal-rank style values in index order
 * ud_coral_moments : CORAL statistics (utils/operation.py:7-13,24-34) of x[N][3][HW]: per (sample, chunk) partial
 *                    sums part[N][chunks][9] = (sum x_c (3), sum x_c x_d for 00 01 02 11 12 22), fp64
 * ud_affine3       : out[n][c][i] = sum_k M[n][c][k] x[n][k][i] + M[n][c][3]   (M[N][3][4]; CORAL's transfer,
 *                    utils/operation.py:36-45, folded into one affine colour map per sample) */
int ud_gather2d(const float* in, float* out, const int* iy, const int* ix, long planes, int H, int W,
                ud_stream_t stream);
int ud_blur5_reflect(const float* in, float* out, long planes, int H, int W, float k0, float k1, float k2,
                     ud_stream_t stream);
int ud_amp_mix(const float* A, const float* B, const float* lmda, float* out, long planes, int S, int Whp,
               int planes_per_sample, ud_stream_t stream);
long ud_efdm_ws_bytes(int rows, int L);
int ud_efdm(const float* content, const float* style, const float* lmda, float* out, int rows, int L,
            int rows_per_sample, void* ws, long ws_bytes, ud_stream_t stream);
int ud_coral_moments(const float* x, double* part, int N, int HW, int chunks, ud_stream_t stream);
int ud_affine3(const float* x, const float* M, float* out, int N, int HW, ud_stream_t stream);

/* ---- deferred normalisation: the fused MBConv path (csrc/fused.hip) ------------------------------------------------
 * MBConvBlock.forward (model/efficientnet/model.py:94-135) alternates 1x1 convs / depthwise or SF convs with
 * BatchNorm + swish, squeeze-excite and the residual.  Here a BatchNorm is never applied as a pass of its own: its
 * batch statistics live as fp64 sums (sum x, sum x^2 per channel) in a zero-initialised accumulator that the
 * PRODUCING side fills with atomic adds (ud_colstats, ud_irfft2_mix), and every CONSUMER applies
 * act(gamma (x - mean) invstd + beta) while it loads x (ud_bn_ref).  The same holds for the backward sums
 * (sum dz, sum dz xhat).  No finalize launches, no normalised copy of the activation in HBM.
 * The accumulators are caller-owned fp64 buffers that must be zero before the producing kernel runs.
 * Data shape arguments (G, R, C): G samples x R pixels x C channels (C % 4 == 0).
 * gate_alpha / gate_mode: an optional scalar factor read on the device: 0 none, 1 sigmoid(alpha[0]),
 * 2 1 - sigmoid(alpha[0])  (the sf_coef mix of exp.py:61-65 carried into the backward kernels).
 * EVAL FORM: sum == NULL with running_mean and running_var both set is an eval-mode BatchNorm: mean = running_mean and
 * var = running_var (the fixed affine map of nn.BatchNorm2d.eval()); the running buffers are only read, never written,
 * and sumsq / inv_count / unbias / momentum are ignored.  Every forward consumer takes it; every TRAINING-FORM BACKWARD entry
 * point (ud_coldot_bn, ud_normbwd_*, ud_se_scale_bwd_bn, ud_dwconv_bwd_data_bn, ud_dwtile_wgrad, ud_dwtile_bwd, ud_irfft2_dwbwd,
 * ud_pw_bwd_fused, ud_pj_bwd_fused_a / _b) returns UD_EINVAL for it: their statistics terms do not exist for a fixed affine map.
 * FROZEN BACKWARD: the backward THROUGH an eval-form BatchNorm is dx = gamma invstd dz per channel — no sums, no apply pass, no
 * statistics exchange.  The entry points that take it (ud_coldot_bn_eval, ud_se_scale_bwd_bn_eval, ud_bn_eval_bwd,
 * ud_dwtile_dgrad_eval: the data-gradient-only backward of a frozen MBConv block, tape.mbconv_frozen_half) REQUIRE the eval form
 * and return UD_EINVAL for a training-form ud_bn_ref; they write no parameter gradient.
 * STATISTICS OFF IN EVAL: a forward whose BatchNorms are all in the eval form needs no batch statistics, so producers
 * whose statistics epilogue is optional skip it when handed no accumulator, and ud_colstats is not launched at all.
 * ud_dwtile (stats 0), ud_gemm (stat_sum NULL) and ud_pj_fwd_fused (sum == sumsq == NULL) always took this; ud_irfft2_mix and
 * ud_irfft2_two_pass take sum == sumsq == NULL since the fp16 inference forward. */
typedef struct {
    const double* sum;       /* [G][C] sum of x over the rows (and ranks) the statistics cover */
    const double* sumsq;     /* [G][C] sum of x^2 */
    const float* gamma;      /* [C] */
    const float* beta;       /* [C] */
    double inv_count;        /* 1 / (number of values behind each sum) */
    double unbias;           /* count / (count - 1): running_var takes the unbiased variance (nn.BatchNorm) */
    float eps;
    float momentum;
    int act;                 /* activation applied after the affine map: 0 none, 1 swish */
    int G;                   /* groups of the STATISTICS: 1 = batch norm (one set for all samples) */
    float* running_mean;     /* optional [C]: updated once by the consuming kernel that is handed them (eval form: read) */
    float* running_var;
} ud_bn_ref;

/* Storage type: entry points with an `int f16` parameter take their ACTIVATION tensors (declared const void* / void*) as
 * float (f16 = 0) or _Float16 (f16 = 1, "half storage", BASELINE configs[4]); per-channel / per-sample vectors,
 * weights, weight gradients and the fp64 accumulators keep their types.  Arithmetic is fp32 in registers either way;
 * half results are rounded to nearest even on store, and statistics are taken of the rounded values.
 *
 * Reducing entry points take `ws`: fp64 scratch of ud_fused_reduce_ws_doubles(G, R, C, per_group, min_rows) doubles
 * (per_group = 1 for [G][C] outputs, 0 for one [C] set; min_rows = 8) — they run as ONE launch with fp64 atomic adds
 * while at most 64 workgroups would add to the same addresses (ws unused, the helper returns 0) and as partials +
 * finalize otherwise.  ws may be NULL (always atomics). */
long ud_fused_reduce_ws_doubles(int G, int R, int C, int per_group, int min_rows);
/* sum[g][c] += sum_r x, sumsq[g][c] += sum_r x^2   (training-mode BatchNorm statistics, model.py:109,114,126) */
int ud_colstats(const void* x, int G, int R, int C, double* sum, double* sumsq, double* ws, int f16, ud_stream_t
    stream);
/* out[g][c] += sum_r act(bn(x))            (SE squeeze: adaptive_avg_pool2d of the activated tensor, model.py:118;
 *                                           head pooling unidefense.py:226)  — bn->running_* are updated here */
int ud_colsum_bn(const void* x, const ud_bn_ref* bn, int G, int R, int C, double* out, double* ws, int f16,
    ud_stream_t stream);
/* out[g][c] += sum_r dy * act(bn(x))       (gradient of the SE gate) */
int ud_coldot_bn(const void* dy, const void* x, const ud_bn_ref* bn, int G, int R, int C, double* out, double*
    ws, int f16, ud_stream_t stream);
/* y[n][o] = sum_i (xsum[n][i] * xscale) W[o][i] + b[o]      (SE reduce conv on the pooled sums) */
int ud_fc_fwd_d(const double* xsum, float xscale, const float* W, const float* b, float* y, int N, int I, int O,
                ud_stream_t stream);
/* y = act(bn(x)) * sigmoid(s[g][c])        (BN1 + swish + SE gate in one pass, model.py:114-122)
 * absmax (here and below; may be NULL): 256 caller-zeroed slots that receive |result|max as a side output — the scale of
 * ud_split_planes_h2t without a pass of its own, for results that feed a 1x1 conv on ud_gemm_p3 */
int ud_se_scale_bn(const void* x, const ud_bn_ref* bn, const float* s, void* y, int G, int R, int C, int f16,
    uint32_t* absmax, ud_stream_t stream);
/* ud_colsum_bn (fp32 storage) that also leaves max |act(bn(x))| in the 256 caller-zeroed slots `absmax`, and ud_se_scale_bn
 * writing its result y = act(bn(x)) * sigmoid(s) DIRECTLY as the fp16 x 2 planes of the project conv's operand (ud_gemm_p3 prec 2,
 * P32 layout over [G R] x C, C % 32 == 0) with the scale that maximum gives (|y| <= it: the gate is a sigmoid) — the SE squeeze
 * pass has just read the whole tensor, so the split pass (ud_split_planes_h2t) and the fp32 tensor between them are not needed. */
int ud_colsum_bn_amax(const void* x, const ud_bn_ref* bn, int G, int R, int C, double* out, double* ws, uint32_t* absmax,
                      ud_stream_t stream);
int ud_se_scale_bn_planes(const void* x, const ud_bn_ref* bn, const float* s, uint16_t* planes, long panel_stride,
                          long plane_stride, float* inv_scale, const uint32_t* amax_in, int G, int R, int C,
                          ud_stream_t stream);
/* half storage (the mixed-precision mode): ud_se_scale_bn whose half result is laid into the ONE fp16 plane of ud_gemm_p3 prec 1 */
int ud_se_scale_bn_plane_half(const void* x, const ud_bn_ref* bn, const float* s, uint16_t* plane, long panel_stride,
                              float* inv_scale, int G, int R, int C, ud_stream_t stream);
/* out = bn(x) * (keep[g] * inv_keep) + skip   (BN2 + drop_connect + residual, model.py:126-134; keep / skip may be
 * NULL; bn->running_* are updated here) */
int ud_residual_bn(const void* x, const ud_bn_ref* bn, const float* keep, float inv_keep, const void* skip,
    void* out, int G, int R, int C, int f16, uint32_t* absmax, ud_stream_t stream);
/* ud_residual_bn (fp32 storage) that ALSO writes its result as the fp16 x 2 planes of the next block's expand conv (ud_gemm_p3 prec 2,
 * P32 layout over [G R] x C) — no split pass over the block output.  Scale from an a-priori bound: |bn(x)_c| <= |gamma_c| sqrt(count)
 * + |beta_c| (times inv_keep under drop-connect) + max |skip| (skip_absmax: the 256 absmax slots its producer left; required with skip). */
int ud_residual_bn_planes(const float* x, const ud_bn_ref* bn, const float* keep, float inv_keep, const float* skip,
                          const uint32_t* skip_absmax, float* out, uint16_t* planes, long panel_stride, long plane_stride,
                          float* inv_scale, int G, int R, int C, uint32_t* absmax, ud_stream_t stream);
/* BatchNorm backward, reductions: dz = dy * (keep[g] * inv_keep) * act'(z)  (dy_is_dz: dz = dy);
 * s1[c] += sum dz, s2[c] += sum dz * xhat;  s3 (optional) [c] += sum dz^2, rounded up (ud_normbwd_apply_planes' energy) */
int ud_normbwd_sums(const void* x, const void* dy, const float* keep, float inv_keep, const ud_bn_ref* bn, int
    dy_is_dz, int G, int R, int C, double* s1, double* s2, double* s3, double* ws, int f16, ud_stream_t stream);
/* dx = gamma invstd (dz - s1 inv_count - xhat s2 inv_count); s1/s2: sums over ALL ranks, s1_local/s2_local: this
 * rank's sums -> dbeta / dgamma (NULL: not written) */
int ud_normbwd_apply(const void* x, const void* dy, const float* keep, float inv_keep, const ud_bn_ref* bn, int
    dy_is_dz, const double* s1, const double* s2, const double* s1_local, const double* s2_local, int G, int R,
    int C, void* dx, float* dgamma, float* dbeta, int f16, uint32_t* absmax, ud_stream_t stream);
/* ud_normbwd_apply (fp32) writing dx DIRECTLY as the fp16 x 2 planes of the GEMMs that read it (the 1x1 conv's weight and data
 * gradient on ud_gemm_p3 prec 2; P32 layout over [G R] x C, pad columns of the last panel zero) — no fp32 dx, no split pass.  One
 * power-of-two scale for the tensor from an a-priori bound: dx_c = gamma_c invstd_c P(dz_c) with P a contraction, so
 * |dx| <= max_c |gamma_c invstd_c| sqrt(energy[c]), energy[c] >= sum_rows dz_c^2 over the whole batch (ud_normbwd_sums' s3 or
 * ud_irfft2_dwbwd's s3, reduced over the ranks like s1 / s2); *inv_scale receives 1 / scale.  A bound above the true maximum
 * costs log2(bound / max) of the 18 binades in which an element keeps its 22 bits, nothing of the large elements' precision. */
int ud_normbwd_apply_planes(const float* x, const float* dy, const float* keep, float inv_keep, const ud_bn_ref* bn,
                            int dy_is_dz, const double* s1, const double* s2, const double* s1_local,
                            const double* s2_local, const double* energy, int G, int R, int C, uint16_t* planes,
                            long panel_stride, long plane_stride, float* inv_scale, float* dgamma, float* dbeta,
                            ud_stream_t stream);
/* Backward of a THIN expand 1x1 conv (model/efficientnet/model.py:101-109: _expand_conv + _bn0 of the 128 x 128 / 64 x 64 blocks) in
 * ONE pass over its two big tensors: ud_normbwd_apply (dy_is_dz = 1) + the conv's weight gradient + its data gradient —
 *     de = gamma invstd (dz - s1 / count - xhat s2 / count)   formed in registers from (dz, e), never written
 *     dw[CE][CIN] = de^T x        dx[M][CIN] = de w (+ add; add may alias dx)
 * with gemm_x3's arithmetic (exact three-way bf16 split, six piece products, fp32 accumulation).  (CE, CIN) must be a pair
 * ud_pw_bwd_fused_ok accepts; part: ud_pw_bwd_fused_grid(M) * CE * CIN floats of scratch (one weight-gradient partial per workgroup,
 * folded in workgroup order: bit-reproducible).  dgamma / dbeta (optional) from this rank's sums, as ud_normbwd_apply. */
int ud_pw_bwd_fused_ok(int CE, int CIN);
/* launch form of ud_pw_bwd_fused (kernel bench, tools/bench_pwbwd.py): 0 the shipped form per shape; 1..4 = (tiles of loads in flight
 * per thread, workgroups per CU) in (1, 2), (2, 2), (3, 1), (4, 1) */
int ud_pw_bwd_set_form(int form);
long ud_pw_bwd_fused_grid(long M);
int ud_pw_bwd_fused(const float* e, const float* dz, const ud_bn_ref* bn, const double* s1, const double* s2,
                    const double* s1_local, const double* s2_local, const float* x, const float* w, const float* add, long M,
                    int CE, int CIN, float* dx, float* dw, float* part, float* dgamma, float* dbeta, ud_stream_t stream);
/* Backward of a THIN project 1x1 conv and the squeeze-excite gate in front of it (model/efficientnet/model.py:113-126 of the 64 x 64
 * blocks: c = swish(bn1(d)) sigmoid(s), p = c Wp^T) WITHOUT the conv's data gradient dc = dp Wp ever written: a 32-row tile of dc is
 * re-made from the thin dp [N HW][CO] inside each of the two passes over d that need it —
 *   ud_pj_bwd_fused_a:  dw[CO][CE] = dp^T c  (c re-made from d on load, as ud_se_scale_bn makes it)   and
 *                       dgate[n][ch] += sum_hw dc act(bn1(d))   (ud_coldot_bn's result; dgate zeroed by the caller);
 *                       part: ud_pj_bwd_fused_grid(N, HW, CE, CO) * CO * CE floats of scratch (partials folded in a fixed order);
 *   ud_pj_bwd_fused_b:  dz = (dc sigmoid(s) + dpool inv_hw) act'(bn1(d)),  s1[ch] += sum dz, s2[ch] += sum dz xhat
 *                       (ud_se_scale_bwd_bn's results).
 * gemm_x3's arithmetic for the products.  (CE, CO, HW) must be a triple ud_pj_bwd_fused_ok accepts (HW % 32 == 0: a tile of rows
 * belongs to one sample). */
int ud_pj_bwd_fused_ok(int CE, int CO, int HW);
int ud_pj_fwd_fused_ok(int CE, int CO, int HW);
/* ... and the forward of the same pair of layers in ONE pass over d: p[N HW][CO] = (act(bn1(d)) sigmoid(s)) w^T with the gated tensor
 * made on load (ud_se_scale_bn's values) and never written; sum / sumsq (optional, together): p's BatchNorm-2 statistics
 * (sum[co] += sum_rows p, sumsq[co] += sum_rows p^2).  (CE, CO, HW): a triple ud_pj_fwd_fused_ok accepts. */
int ud_pj_fwd_fused(const float* d, const ud_bn_ref* bn, const float* s, const float* w, int N, int HW, int CE, int CO, float* p,
                    double* sum, double* sumsq, ud_stream_t stream);
long ud_pj_bwd_fused_grid(int N, int HW, int CE, int CO);
/* Eval-mode MBConv, expand conv + BN0 + swish + depthwise conv + BN1 + swish in ONE pass over the thin block input
 * (csrc/evalblk.hip): x [N][H][W][Ci], we [CE][Ci] (the expand conv), wt [K*K][CE] (tap-major depthwise weights), bn0 / bn1
 * in the EVAL FORM of ud_bn_ref (anything else is UD_EINVAL).  e = swish(bn0(x we^T)) is formed per output tile from its input
 * halo in LDS and never written; the depthwise conv has stride `stride` and SAME padding (pad_t, pad_l; e is zero outside the
 * image).  d [N][Ho][Wo][CE] receives z = swish(bn1(dw)) (out_act = 1) or the raw depthwise output dw (out_act = 0, the input
 * ud_pj_fwd_fused applies BN1 to); part [N][tiles][CE] (tiles = ud_mb_eval_dw_tiles) receives per output tile the sum of z,
 * the SE squeeze (ud_group_colsum over the tiles gives the mean).  fp32 FMA throughout, no atomics: results are
 * deterministic.  x and we 16-byte aligned.  ud_mb_eval_dw_ok: the (Ci, CE, K, stride) it takes (Ci % 4 == 0,
 * CE % 16 == 0, K == 3, stride 1 or 2). */
int ud_mb_eval_dw_ok(int Ci, int CE, int K, int stride);
long ud_mb_eval_dw_tiles(int Ho, int Wo, int stride);
int ud_mb_eval_dw(const float* x, const float* we, const ud_bn_ref* bn0, const float* wt, const ud_bn_ref* bn1, float* d, float* part,
                  int N, int H, int W, int Ci, int CE, int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int out_act,
                  ud_stream_t stream);
/* The same node in half storage (the fp16 inference forward): x and d are _Float16, we / wt / part fp32.  The expand conv runs
 * on v_mfma_f32_16x16x32_f16 (halo pixels x input channels from LDS, We rounded to fp16 as it is staged, fp32 accumulation);
 * BN0 + swish, the zero padding, the depthwise conv and BN1 + swish in fp32.  d receives z rounded to fp16 (out_act = 1) or the
 * raw dw rounded to fp16 (out_act = 0); part receives per tile the sum of what a consumer reads back: the stored z, or
 * swish(bn1(.)) of the stored raw value.  No atomics.  x 16-byte aligned.  ud_mb_eval_dw_h_ok: Ci % 8 == 0, CE % 16 == 0,
 * K == 3, stride 1 or 2; ud_mb_eval_dw_h_tiles == ud_mb_eval_dw_tiles. */
int ud_mb_eval_dw_h_ok(int Ci, int CE, int K, int stride);
long ud_mb_eval_dw_h_tiles(int Ho, int Wo, int stride);
int ud_mb_eval_dw_h(const void* x, const float* we, const ud_bn_ref* bn0, const float* wt, const ud_bn_ref* bn1, void* d, float* part,
                    int N, int H, int W, int Ci, int CE, int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int out_act,
                    ud_stream_t stream);
int ud_pj_bwd_fused_a(const float* d, const float* dp, const ud_bn_ref* bn, const float* s, const float* w, int N, int HW, int CE,
                      int CO, float* dw, double* dgate, float* part, ud_stream_t stream);
int ud_pj_bwd_fused_b(const float* d, const float* dp, const ud_bn_ref* bn, const float* s, const float* dpool, float inv_hw,
                      const float* w, int N, int HW, int CE, int CO, float* dz, double* s1, double* s2, ud_stream_t stream);
/* ---- the same two passes with the BatchNorm-1 backward folded in: dz is never written ----
 * ud_pj_bwd_fused_a_se : ud_pj_bwd_fused_a that also sums the four per-sample dots of ud_coldot_bn_se: dots [5][N][CE] fp64, zeroed
 *                        by the caller, receives (dgate, A1, A2, B1, B2); dgate's products are ud_pj_bwd_fused_a's.  ud_se_bwd_b_bn
 *                        turns the dots into the sums s1 / s2.
 * ud_pj_bwd_fused_c    : one pass over d in place of ud_pj_bwd_fused_b + ud_normbwd_apply: dz formed as there, kept in registers,
 *                        dd = gamma invstd (dz - s1 / count - xhat s2 / count) written (ud_normbwd_apply's rounding); dgamma / dbeta
 *                        (optional) from this rank's sums s2_local / s1_local, which they require.
 * ud_pj_bwd_fused_c_mix: ... in place of ud_normbwd_apply_mix: diff, dalpha_acc (64 slots) and energy (optional) as there.
 * Training-form BatchNorm only (the eval form is UD_EINVAL); (CE, CO, HW): a triple ud_pj_bwd_fused_se_ok accepts (the pairs of
 * ud_pj_bwd_fused_ok but the 24-column ones). */
int ud_pj_bwd_fused_se_ok(int CE, int CO, int HW);
int ud_pj_bwd_fused_a_se(const float* d, const float* dp, const ud_bn_ref* bn, const float* s, const float* w, int N, int HW, int CE,
                         int CO, float* dw, double* dots, float* part, ud_stream_t stream);
int ud_pj_bwd_fused_c(const float* d, const float* dp, const ud_bn_ref* bn, const float* s, const float* dpool, float inv_hw,
                      const float* w, const double* s1, const double* s2, const double* s1_local, const double* s2_local, int N,
                      int HW, int CE, int CO, float* dd, float* dgamma, float* dbeta, ud_stream_t stream);
int ud_pj_bwd_fused_c_mix(const float* d, const float* dp, const ud_bn_ref* bn, const float* s, const float* dpool, float inv_hw,
                          const float* w, const double* s1, const double* s2, const double* s1_local, const double* s2_local,
                          const float* diff, int N, int HW, int CE, int CO, float* dd, double* dalpha_acc, float* dgamma,
                          float* dbeta, double* energy, ud_stream_t stream);
/* Half storage (the mixed-precision mode): ud_normbwd_apply whose half result is laid straight into the ONE fp16 plane (P32 layout,
 * scale 1) that ud_gemm_p3 prec 1 reads — the row-major tensor and the ud_planes_from_half pass over it are not needed. */
int ud_normbwd_apply_plane_half(const void* x, const void* dy, const float* keep, float inv_keep, const ud_bn_ref* bn,
                                int dy_is_dz, const double* s1, const double* s2, const double* s1_local,
                                const double* s2_local, int G, int R, int C, uint16_t* plane, long panel_stride,
                                float* inv_scale, float* dgamma, float* dbeta, ud_stream_t stream);
/* SE backward, the two small FC layers (model.py:119-121) in two launches:
 *   a: dpre = dgate[n][c] * sigmoid'(s2);  ds1[n][i] = swish'(s1) sum_c dpre W_e[c][i];
 *      dW_e[c][i] = sum_n dpre swish(s1[n][i]);  db_e[c] = sum_n dpre
 *   b: dpool[n][c] = sum_i ds1 W_r[i][c];  dW_r[i][c] = sum_n ds1[n][i] pool[n][c] * pool_scale;  db_r[i] = sum_n ds1 */
/* dWe == dbe == NULL (a: both or neither) / dWr == dbr == NULL (b; pool may then be NULL too): the workgroups that form the
 * weight and bias gradients are not launched — the data-gradient-only backward of a frozen model */
int ud_se_bwd_a(const double* dgate, const float* s2, const float* s1, const float* We, double* ds1_acc, float* dWe,
                float* dbe, int N, int C, int Cs, ud_stream_t stream);
int ud_se_bwd_b(const double* ds1_acc, const float* s1, const float* Wr, const double* pool, float pool_scale,
                float* dpool, float* dWr, float* dbr, int N, int C, int Cs, ud_stream_t stream);
/* db = dc * sigmoid(s[g][c]) + dpool[g][c] * inv_hw;  dz = db * act'(bn(x));  s1 += sum dz, s2 += sum dz xhat
 * (gradient through the SE gate and the swish of BN1, with BN1's backward sums) */
int ud_se_scale_bwd_bn(const void* dc, const void* x, const ud_bn_ref* bn, const float* s, const float* dpool,
    float inv_hw, void* dz, double* s1, double* s2, double* ws, int G, int R, int C, int f16, ud_stream_t
    stream);
/* ---- the same SE / BatchNorm-1 backward WITHOUT dz ever written: the BatchNorm sums from per-sample dots ----
 * s1 = sum dz and s2 = sum dz xhat of dz = (dc g + p) act'(bn(x)), g = sigmoid(s[n][c]), p = dpool[n][c] inv_hw, are linear in
 * the per-sample quantities (g, p):  s1[c] = sum_n (g A1[n][c] + p B1[n][c]),  s2[c] = sum_n (g A2[n][c] + p B2[n][c])  with
 *   A1 = sum_hw dc act'(y)   A2 = sum_hw dc act'(y) xhat   B1 = sum_hw act'(y)   B2 = sum_hw act'(y) xhat   (y = bn(x)).
 * fp32 storage only (f16 != 0: UD_EINVAL); training-form entry points: the eval form of ud_bn_ref is UD_EINVAL.
 * ud_coldot_bn_se        : ud_coldot_bn that also sums the four dots: out [5][G][C] fp64, zeroed by the caller, receives
 *                          (dgate, A1, A2, B1, B2).  One launch, fp64 atomics with at most 64 adds per address; no scratch.
 * ud_se_bwd_b_bn         : ud_se_bwd_b whose (n, c) thread also adds g A + p B of its sample into bs1[c] / bs2[c] (fp64, zeroed by
 *                          the caller; N adds per address).  s2: the gate's pre-activation [N][C]; dots: ud_coldot_bn_se's out.
 *                          Same dpool / dWr / dbr as ud_se_bwd_b.
 * ud_normbwd_apply_se    : ud_normbwd_apply whose second input is dc: dz is formed on load from (dc, x, s, dpool); s / dpool
 *                          [G][C], one sample per group.  dx, dgamma, dbeta, absmax as ud_normbwd_apply.
 * ud_normbwd_apply_mix_se: ud_normbwd_apply_mix likewise (dalpha_acc, energy as there). */
int ud_coldot_bn_se(const void* dy, const void* x, const ud_bn_ref* bn, int G, int R, int C, double* out, int f16,
                    ud_stream_t stream);
int ud_se_bwd_b_bn(const double* ds1_acc, const float* s1, const float* Wr, const double* pool, float pool_scale,
                   float* dpool, float* dWr, float* dbr, const float* s2, const double* dots, float inv_hw, double* bs1,
                   double* bs2, int N, int C, int Cs, ud_stream_t stream);
int ud_normbwd_apply_se(const void* x, const void* dc, const ud_bn_ref* bn, const float* s, const float* dpool, float inv_hw,
                        const double* s1, const double* s2, const double* s1_local, const double* s2_local, int G, int R,
                        int C, void* dx, float* dgamma, float* dbeta, int f16, uint32_t* absmax, ud_stream_t stream);
int ud_normbwd_apply_mix_se(const void* x, const void* dc, const ud_bn_ref* bn, const float* s, const float* dpool,
                            float inv_hw, const double* s1, const double* s2, const double* s1_local,
                            const double* s2_local, const void* diff, int G, int R, int C, void* dd, double* dalpha_acc,
                            float* dgamma, float* dbeta, double* energy, int f16, ud_stream_t stream);
/* ---- frozen backward: the same steps through EVAL-FORM BatchNorms (required; UD_EINVAL for the training form) ----
 * ud_coldot_bn_eval      : out[g][c] += sum_r dy * act(bn(x)) (the SE gate's gradient; out zeroed by the caller).  Deterministic:
 *                          no atomic add is shared by two workgroups — one row-chunk per sample adds once into the zeroed slot,
 *                          more go through ws (ud_coldot_bn_eval_ws_doubles(G, R, C) doubles; 0: not needed) and a fold.
 * ud_se_scale_bwd_bn_eval: dd = (dc * sigmoid(s[g][c]) + dpool[g][c] * inv_hw) * act'(bn(x)) * gamma invstd: the gradient through
 *                          the SE gate, the swish and BN1 itself in ONE pass over (dc, x); no s1 / s2 / ws.
 * ud_bn_eval_bwd         : dx = dy * gamma invstd [* act'(bn(x)) when bn->act != 0; x may be NULL otherwise] */
long ud_coldot_bn_eval_ws_doubles(int G, int R, int C);
int ud_coldot_bn_eval(const void* dy, const void* x, const ud_bn_ref* bn, int G, int R, int C, double* out, double* ws,
                      int f16, ud_stream_t stream);
int ud_se_scale_bwd_bn_eval(const void* dc, const void* x, const ud_bn_ref* bn, const float* s, const float* dpool,
                            float inv_hw, void* dd, int G, int R, int C, int f16, ud_stream_t stream);
int ud_bn_eval_bwd(const void* dy, const void* x, const ud_bn_ref* bn, void* dx, int G, int R, int C, int f16,
                   ud_stream_t stream);
/* ud_normbwd_apply (dy_is_dz) fused with the gradient of the SF mix y = (1-a) spat + a freq (exp.py:61-65):
 * writes dd = dL/dy and accumulates sum dd * diff, diff = freq - spat as stored by ud_irfft2_mix, into the 64 slots
 * dalpha_acc[0..64) (zeroed by the caller); energy (optional, C doubles zeroed by the caller): += sum_rows dd_c^2, rounded up —
 * the per-channel energy bound ud_rfft2_ex_planes takes for the transform of dd that follows */
int ud_normbwd_apply_mix(const void* x, const void* dz, const ud_bn_ref* bn, const double* s1, const double* s2,
    const double* s1_local, const double* s2_local, const void* diff, int G, int R, int C, void* dd,
    double* dalpha_acc, float* dgamma, float* dbeta, double* energy, int f16, ud_stream_t stream);
/* out[0] = sigmoid'(alpha[0]) * sum(acc[0..64))      (sf_coef gradient from the accumulator above) */
int ud_gate_grad_from_acc(const double* acc, const float* alpha, float* out, ud_stream_t stream);
/* y = act(bn(x)): the materialised form for consumers that re-read their input per tap (a plain depthwise conv and its
 * weight gradient: re-evaluating the swish per window load costs more than this pass); bn->running_* are updated here */
int ud_bn_apply(const void* x, const ud_bn_ref* bn, void* y, int G, int R, int C, int f16, ud_stream_t stream);
/* data gradient of the depthwise conv, scaled by the gate, plus `add`, pushed through the swish of the deferred
 * BatchNorm of its INPUT x:  da = gate * dwconv_bwd_data(dy) + add;  dz = da * act'(bn(x));  s1/s2 as above */
int ud_dwconv_bwd_data_bn(const void* dy, const float* gate_alpha, int gate_mode, const float* wt, const void*
    add, const void* x, const ud_bn_ref* bn, void* dz, double* s1, double* s2, double* ws, int N, int H, int W,
    int C, int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int f16, ud_stream_t stream);
long ud_dwconv_bwd_data_bn_ws_doubles(int N, int H, int W, int C, int stride);
/* ud_dwconv_bwd_data with the gate factor on dy */
int ud_dwconv_bwd_data_ex(const void* dy, const float* gate_alpha, int gate_mode, const float* wt, const void*
    add, void* dx, int N, int H, int W, int C, int Ho, int Wo, int K, int stride, int pad_t, int pad_l, int f16,
    ud_stream_t stream);
/* ud_dwconv_bwd_weight with the gate factor on dy */
int ud_dwconv_bwd_weight_ex(const void* x, const void* dy, const float* gate_alpha, int gate_mode, float* dwt,
    float* part, int chunks, int N, int H, int W, int C, int Ho, int Wo, int K, int stride, int pad_t, int
    pad_l, int f16, ud_stream_t stream);
/* ud_rfft2 of act(bn(x)) (bn may be NULL), optionally also writing the activated input (act_out) and scaling the
 * result by the gate:  SFConv's spectral branch reading the expand conv's raw output (exp.py:55) and, as the
 * adjoint of irfft2, its backward (gate = sigmoid(sf_coef)).  gate_grad (optional): also finishes the gate's gradient,
 * gate_grad[0] = sigmoid'(alpha) * sum(gate_acc[0..64)), from the slots ud_normbwd_apply_mix filled just before. */
int ud_rfft2_ex(const void* x, void* Y, int N, int S, int C, float scale, float w_interior, const ud_bn_ref* bn,
    void* act_out, const float* gate_alpha, int gate_mode, const double* gate_acc, float* gate_grad, int f16,
    uint32_t* absmax, ud_stream_t stream);
/* ud_rfft2_ex whose result goes DIRECTLY into the fp16 x 2 planes ud_gemm_p3 (prec 2) reads — P32 panel layout over the matrix
 * [N S (S/2+1)] x [Re 0..C | Im 0..C], one power-of-two scale for the tensor — instead of fp32 + ud_split_planes_h2t (the
 * spectral 1x1 conv's operand, model/efficientnet/exp.py:55-57, and its output gradient in the backward).  The scale is taken
 * from an a-priori UPPER BOUND of |Y|: bound_pre * sqrt(max_c e_c) with e_c = gamma_c^2 + beta_c^2 (bn given: the input is
 * act(bn(x)), |act(z)| <= |z|; bound_pre = f_max S sqrt(count)) or e_c = energy[c] >= sum_{n,h,w} x_c^2 (bound_pre = f_max S);
 * a bound 2^b above the true maximum moves the 2^-18 window of full 22-bit precision up by b binades and changes nothing for
 * the large elements.  S in {8, 16, 32, 12, 24, 48}, (2 C) % 32 == 0, fp32 storage; *inv_scale receives 1 / scale.
 * dw_k = 3 / 5 (S in {8, 16, 32}; 0: off): the kernel ALSO writes dw_out[N][S][S][C] = the stride-1 depthwise dw_k x dw_k conv
 * (pads (dw_k - 1) / 2, taps dw_wt tap-major [dw_k^2][C]) of the same activated plane act(bn(x)) — SFConv's spatial branch
 * (exp.py:49-51) without a kernel of its own. */
int ud_rfft2_ex_planes(const void* x, uint16_t* planes, long panel_stride, long plane_stride, float* inv_scale, float bound_pre,
                       const double* energy, int N, int S, int C, float scale, float w_interior, const ud_bn_ref* bn,
                       void* act_out, const float* gate_alpha, int gate_mode, const double* gate_acc, float* gate_grad,
                       const float* dw_wt, void* dw_out, int dw_k, ud_stream_t stream);
/* irfft2 + SF mix + BN1 statistics (exp.py:60-65, stride 1):  freq = irfft2(Y) * scale;
 * y = (1 - a) spat + a freq, a = sigmoid(alpha[0]);  diff_out = freq - spat (what the backward needs of the two
 * branches: neither has to be kept);  sum[c] += sum y, sumsq[c] += sum y^2 (both NULL: no statistics) */
int ud_irfft2_mix(const void* Y, void* y, int N, int S, int C, float scale, float w_interior, const void* spat,
    const float* alpha, void* diff_out, double* sum, double* sumsq, int f16, ud_stream_t stream);

/* Two-pass forms of the 32 x 32 / 64 x 64 transforms (torch.fft.rfft2 / irfft2 of exp.py:55,60 and their adjoints): a
 * row kernel and a column kernel with the half-spectrum between them in ws (ud_fft2_two_pass_ws_floats floats, fp32,
 * [N][S][S/2+1][Re 0..C | Im 0..C]); a wave owns 64 consecutive channels of one image row / one kx column, so every access
 * is a run of whole lines where the one-kernel forms above read 16 ... 64-byte pieces.  Same results to the last bit or
 * two.  bn / act_out / gate_*: as ud_rfft2_ex (all NULL / 0: plain
 * ud_rfft2); spat / alpha / freq_out / sum / sumsq: as ud_irfft2_mix (spat NULL: plain ud_irfft2). */
long ud_fft2_two_pass_ws_floats(int N, int S, int C);
int ud_rfft2_two_pass(const void* x, void* Y, float* ws, int N, int S, int C, float scale, float w_interior,
    const ud_bn_ref* bn, void* act_out, const float* gate_alpha, int gate_mode, const double* gate_acc,
    float* gate_grad, int f16, uint32_t* absmax, ud_stream_t stream);
int ud_irfft2_two_pass(const void* Y, void* y, float* ws, int N, int S, int C, float scale, float w_interior,
    const void* spat, const float* alpha, void* freq_out, double* sum, double* sumsq, int f16, ud_stream_t stream);

/* ---- multi-tensor AdamW (csrc/optim.hip) ------------------------------------------------------------------------
 * torch.optim.AdamW(amsgrad) over timm's weight-decay groups (engine/forgery_engine.py:149-156) with GradScaler's
 * unscale and found_inf skip (engine/abstract_engine.py:281-283) folded in: ONE launch for all parameter tensors.
 * table: device array of entries of 8 x int64 {p, g, m, v, vmax (0: no amsgrad) pointers, numel, group, 0}; chunk_map: device array of int32 pairs (tensor, chunk of ud_adamw_chunk_elems() elements),
 * one workgroup each; lr / wd: host arrays per group (<= 8); grad_scale, found_inf: device scalars or NULL;
 * step_in / step_out: device int32 counters (out = in + 1, or in when found_inf != 0 and nothing is updated). */
int ud_adamw_chunk_elems(void);
int ud_adamw_multi(const void* table, const void* chunk_map, int n_chunks, const float* lr, const float* wd, int n_groups,
                   double beta1, double beta2, double eps, int amsgrad, int maximize, const float* grad_scale,
                   const float* found_inf, const int* step_in, int* step_out, ud_stream_t stream);

/* ---- gradient accumulation of a second backward (csrc/optim.hip) --------------------------------------------------
 * The train step calls backward() twice per zero_grad() (engine/abstract_engine.py:281 and :374 under the one
 * optimizer.zero_grad() of engine/forgery_engine.py:241): torch's AccumulateGrad adds the second backward's gradients with one
 * launch per parameter tensor.  ud_multi_add: dst[i][0..numel[i]) += src[i][0..numel[i]) for n fp32 tensors in ceil(n / 120)
 * launches; dst / src / numel are HOST arrays (device pointers inside), read at call time — nothing staged on the device, so the
 * call can sit inside a captured step.  numel[i] < 2^31. */
int ud_multi_add(void* const* dst, const void* const* src, const long* numel, int n, ud_stream_t stream);

/* ---- LDS-tiled depthwise conv, stride 1 (csrc/dwtile.hip) -----------------------------------------------------------
 * The depthwise k x k conv of MBConvBlock.forward (model/efficientnet/model.py:112-115; SFConv's spatial branch
 * exp.py:49-51) with a halo tile of 32 channels staged in LDS once per workgroup, act(bn_in(src)) applied while staging
 * (the activated tensor never exists in HBM).  out(oh, ow) = sum_{i,j} src'(oh + i - P_t, ow + j - P_l) * w[tap(i, j)],
 * src' = act(bn_in(src)) (bn_in NULL: src), zero outside the image; flip = 0: tap = i*K + j (forward, P = the conv's
 * pads); flip = 1: tap = K*K-1 - (i*K + j) with P = K-1 - pad: the data gradient over dy.  wt: tap-major [K*K][C].
 * epi 0: store.  epi 1: also s1 += sum out, s2 += sum out^2 per channel (BN1 statistics of a plain depthwise block).
 * epi 2: out = gate(gate_alpha, gate_mode) * conv [+ add]; with bn_out: out *= act'(bn_out(xbn)) and s1 += sum out,
 * s2 += sum out * xhat (the BatchNorm backward sums).  ws: ud_dwtile_ws_doubles doubles when sums are taken.
 * stride 2 (the four down-sampling blocks): flip = 0 — the forward reads src(2 oh + i - P_t, ..) (epi 0 / 1); flip = 1 with
 * epi 2 — the data gradient: src = dy of the strided conv is read through a zero-stuffed grid (position v holds dy(v / 2)
 * for even v), P = K-1 - pad as for stride 1. */
long ud_dwtile_ws_doubles(int N, int Ho, int Wo, int C);
int ud_dwtile(const void* src, const ud_bn_ref* bn_in, const float* wt, void* out, int N, int Hs, int Ws, int C, int Ho,
              int Wo, int K, int P_t, int P_l, int flip, const float* gate_alpha, int gate_mode, const void* add,
              const void* xbn, const ud_bn_ref* bn_out, int epi, double* s1, double* s2, double* ws, int stride,
              int f16, ud_stream_t stream);
/* weight gradient dwt[C][K*K] = gate * sum_pixels act(bn_in(src))(oh + i - P_t, ow + j - P_l) * dy(oh, ow);
 * part: ud_dwtile_wgrad_part_rows(N, Ho, Wo) rows of K*K*C floats */
long ud_dwtile_wgrad_part_rows(int N, int Ho, int Wo);
int ud_dwtile_wgrad(const void* src, const ud_bn_ref* bn_in, const void* dy, const float* gate_alpha, int gate_mode,
                    float* dwt, float* part, long part_rows, int N, int Hs, int Ws, int C, int Ho, int Wo, int K, int P_t,
                    int P_l, int stride, int f16, ud_stream_t stream);
/* Backward of the stride-1 depthwise conv (autograd of model/efficientnet/model.py:112-115 / exp.py:49-51) in ONE pass over its
 * operands: both halo tiles (dy, act(bn(x))) staged once per image and workgroup;
 *   dz = (gate * conv_flipped(dy) [+ add]) * act'(bn(x))   (bn NULL: no activation factor, x is the conv's input itself),
 *   s1 += sum dz, s2 += sum dz * xhat (bn given; ws: ud_dwtile_ws_doubles(N, H, W, C) doubles),
 *   dwt[C][K*K] = gate * sum_pixels act(bn(x))(oh + i - P_t, ow + j - P_l) * dy(oh, ow)
 * (ud_dwtile epi 2 + ud_dwtile_wgrad, which read each operand twice).  wpart: ud_dwtile_wgrad_part_rows(N, H, W) rows.
 * dwt == NULL: the partial rows are left for ud_param_fold_multi and their number is returned. */
int ud_dwtile_bwd(const void* dy, const void* x, const ud_bn_ref* bn, const float* wt, const float* gate_alpha, int gate_mode,
                  const void* add, void* dz, float* dwt, float* wpart, long part_rows, double* s1, double* s2, double* ws,
                  int N, int H, int W, int C, int K, int P_t, int P_l, int f16, ud_stream_t stream);
/* Frozen backward: ud_dwtile's data gradient (flipped taps, stride 2 through the zero-stuffed grid of dy, gate modes 0 / 1 / 2,
 * optional add) pushed through the EVAL-FORM BatchNorm + activation of the conv's input xbn in the epilogue:
 *   dx = (gate * dwconv^T(dy) + add) * act'(bn(xbn)) * gamma invstd
 * dy [N][Ho][Wo][C]; add (may be NULL) / xbn / dx [N][H][W][C]; pad_t / pad_l: the FORWARD conv's pads; K 3 / 5, stride 1 / 2.
 * Requires the eval form (UD_EINVAL for a training-form bn); writes no sums and needs no scratch. */
int ud_dwtile_dgrad_eval(const void* dy, const float* wt, const float* gate_alpha, int gate_mode, const void* add,
                         const void* xbn, const ud_bn_ref* bn, void* dx, int N, int H, int W, int C, int Ho, int Wo, int K,
                         int pad_t, int pad_l, int stride, int f16, ud_stream_t stream);
/* dwt[C][K*K] = gate * sum_p part[p][K*K][C] (fp64 accumulation): the fold of per-workgroup weight-gradient partials, for kernels
 * outside csrc/dwtile.hip that produce them (ud_irfft2_dwbwd) */
int ud_dwtile_wgrad_finalize(const float* part, int nparts, int K, int C, const float* gate_alpha, int gate_mode, float* dwt,
                             ud_stream_t stream);
/* The folds that only FINISH a parameter's gradient — nothing else in a backward reads their result — as items of ONE launch per
 * 44 items (csrc/param_fold.hip; the items travel by value in the kernel arguments: capturable, no device table).  Every producer
 * that leaves per-workgroup partials also folds through this entry point when called in its immediate form, so one kernel body
 * (one summation order per kind) serves both.  Producers called with a NULL result pointer (ud_dwtile_wgrad / ud_dwtile_bwd dwt,
 * ud_pw_bwd_fused / ud_pj_bwd_fused_a / _a_se dw, ud_conv_small_wgrad / ud_conv_mfma_wgrad out) leave their partials in `part` and
 * RETURN their number (> 0) instead of folding; ud_irfft2_dwbwd's wpart holds N rows; ud_norm_bwd with dgamma == dbeta == NULL
 * leaves the group sum to an item.  The partial buffers must stay untouched until this call.  Item kinds (p0, p1, p2 per kind):
 *   UD_FOLD_DW      dst[C][K*K] = gate * sum_p part[p][K*K][C], fp64 (16 strided lanes, then lanes 0..15); p0 K, p1 C, p2 gate_mode,
 *                   aux = gate_alpha
 *   UD_FOLD_F32     dst[i] = sum_p part[p][i] (i < n), fp32: lane j of 16 adds partials j, j + 32, .. and j + 16, j + 48, .. in two chains, the 16
 *                   lane sums then in order (the thin expand convs, the direct MFMA weight gradients); p2 = CE > 0: also
 *                   dgamma[c] = (float)s2l[c], dbeta[c] = (float)s1l[c] for c < CE (CE <= 16 n)
 *   UD_FOLD_PJ      UD_FOLD_F32's order over the column-chunked partials of ud_pj_bwd_fused_a: dst[co][c] = sum_p
 *                   part[c / CC][p][co][c % CC]; nparts per chunk, n = CO CE, p0 CO, p1 CE, p2 CC
 *   UD_FOLD_F64     dst[i] = sum_p part[p][i] (i < n), fp64: 16 strided lanes, then lanes 0..15 (ud_conv_small_wgrad)
 *   UD_FOLD_GROUP   dgamma[c] = sum_g aux[g][c], dbeta[c] = sum_g part[g][c], fp64, ascending g (InstanceNorm: part = s1, aux = s2 of
 *                   ud_norm_bwd); nparts = G, n = C; either result may be NULL
 *   UD_FOLD_LAYOUT  dst = part in the parameter's layout (a permuting copy), n elements
 * UD_FOLD_F32 / _F64 / _LAYOUT with p0 = KH KW > 1 and p1 = B write a conv weight gradient [A][KH KW][B] (n = A p0 p1) straight
 * into the parameter's [A][B][KH][KW] (F.conv2d: A = Cout, B = Cin; ConvTranspose2d: A = Cin, B = Cout); p0 <= 1: as it is. */
#define UD_FOLD_DW 0
#define UD_FOLD_F32 1
#define UD_FOLD_PJ 2
#define UD_FOLD_F64 3
#define UD_FOLD_GROUP 4
#define UD_FOLD_LAYOUT 5
typedef struct {
    const float* part;          /* the partials [nparts][..] (UD_FOLD_LAYOUT: the source matrix) */
    float* dst;                 /* the gradient (unused by UD_FOLD_GROUP) */
    const float* aux;           /* UD_FOLD_DW: gate_alpha (gate_mode != 0); UD_FOLD_GROUP: s2 */
    const double* s1l;          /* UD_FOLD_F32 with p2 > 0 */
    const double* s2l;
    float* dgamma;              /* UD_FOLD_F32 with p2 > 0, UD_FOLD_GROUP */
    float* dbeta;
    int kind, nparts, n, p0, p1, p2;
} ud_wgrad_fold;
int ud_param_fold_multi(const ud_wgrad_fold* items, int n, ud_stream_t stream);
/* Half storage (the mixed-precision mode): ud_rfft2_ex of a half-stored x whose half result is laid straight into the ONE fp16
 * plane (P32 layout over [N S (S/2+1)] x 2C, scale 1) that ud_gemm_p3 prec 1 reads — no row-major spectrum, no layout pass.  The
 * one-kernel transform sizes (8, 16, 32, 12, 24, 48).  dw_wt / dw_out / dw_k as in ud_rfft2_ex_planes (the stride-1 depthwise conv
 * of the activated plane, half-stored result; S in {8, 16, 32}). */
int ud_rfft2_ex_plane_half(const void* x, uint16_t* plane, long panel_stride, float* inv_scale, int N, int S, int C, float scale,
                           float w_interior, const ud_bn_ref* bn, void* act_out, const float* gate_alpha, int gate_mode,
                           const double* gate_acc, float* gate_grad, const float* dw_wt, void* dw_out, int dw_k,
                           ud_stream_t stream);
/* Backward of an SF block's spatial branch inside the adjoint transform (csrc/fft.hip: irfft2_dwbwd_kernel; S in {8, 16}, K in
 * {3, 5}; f16: Y, dd, x, dz half-stored): da_f = scale * C2R(f(kx) Y) as ud_irfft2 (the adjoint of rfft2: w_interior = 1/2), then with dd = dL/d(conv output)
 * [N][S][S][C], x the conv's raw input and bn the BatchNorm in front of it:
 *   dz = (gate * conv_flipped(dd) + da_f) * act'(bn(x));  s1 += sum dz, s2 += sum dz * xhat;  s3 (optional) += sum dz^2, rounded
 *   up (the energy bound ud_normbwd_apply_planes takes);
 *   wpart[n][K*K][C] = sum_pixels act(bn(x))(window) * dd   of image n  (ud_dwtile_wgrad_finalize sums the N rows).
 * Replaces ud_irfft2 + the depthwise weight-gradient kernel + its finalize + the depthwise data-gradient kernel. */
int ud_irfft2_dwbwd(const void* Y, int N, int S, int C, float scale, float w_interior, const void* dd, const void* x,
                    const ud_bn_ref* bn, const float* wt, int K, const float* gate_alpha, int gate_mode, void* dz, double* s1,
                    double* s2, double* s3, float* wpart, int f16, ud_stream_t stream);

/* ---- large real 2-D FFT of image planes (csrc/fft_large.hip), S in {128, 256, 320} ------------------------------------
 * torch.fft.rfft2 on [N,3,S,S] images: the frequency reconstruction loss (model/unidefense.py:246-253; ResNet variants
 * :421-431, :615-625) and FrequencyStyleTransfer (model/modules.py:35-55), with their autograd adjoint.
 * Y[P][2S][Whp]: rows [0,S) = Re(ky), rows [S,2S) = Im(ky); columns [0, S/2] valid, the rest (Whp = ceil4(S/2+1)) zero.
 * ws: ud_rfft2_planes_ws_floats(P, S) floats of scratch.  The adjoint maps dY back to dx[P][S][S] (transpose of the
 * real-linear map x -> (Re Y, Im Y), same scale): with dY weighted 2 on the interior columns it is irfft2. */
long ud_rfft2_planes_ws_floats(long P, int S);
int ud_rfft2_planes(const float* x, float* Y, float* ws, long P, int S, float scale, ud_stream_t stream);
int ud_rfft2_planes_adjoint(const float* dY, float* dx, float* ws, long P, int S, float scale, ud_stream_t stream);

/* ---- one-shot SyncBatchNorm exchange (csrc/xchg.hip) ---------------------------------------------------------------
 * Replaces the per-BatchNorm library collectives of nn.SyncBatchNorm (engine/forgery_engine.py:142) on one node: every
 * rank owns a mailbox in fine-grained device memory mapped into its peers through HIP IPC; ud_xchg_allreduce is ONE
 * small kernel (a thread per double) that writes the rank's doubles, tagged with the exchange's sequence number, into
 * every mailbox (peer writes over xGMI), polls the own mailbox until all ranks' words carry the tag and sums the rows
 * in rank order (bit-identical on all ranks) — no fences, no separate flags.  seq_counter: two zero-initialised device
 * words advanced by the kernel (hipGraph replays keep counting); a peer that does not arrive within timeout_ms of
 * wall-clock time sets *err (1 + its rank) and turns the affected sums into NaN (never a partial sum) instead of hanging.  world <= 16.  Setup: ud_xchg_create on every rank, handles exchanged by the
 * host (64 bytes each), ud_xchg_open on every peer's handle, the `world` pointers (own base at [rank]) copied to a
 * device array.  max_doubles bounds n; slots >= 2 (a rank is never more than one exchange ahead of the slowest).
 * local_out (may be NULL): receives this rank's OWN n doubles as they were before the sum (the local dgamma / dbeta of a
 * BatchNorm backward) — the copy a separate launch made before round 6. */
long ud_xchg_bytes(int world, int max_doubles, int slots);
int ud_xchg_create(int world, int max_doubles, int slots, void** base, char* handle);
int ud_xchg_open(const char* handle, void** ptr);
int ud_xchg_close(void* ptr);
int ud_xchg_destroy(void* base);
int ud_xchg_allreduce(double* acc, int n, void* const* peers, int rank, int world, int max_doubles, int slots,
                      unsigned long long* seq_counter, int* err, long timeout_ms, double* local_out, ud_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

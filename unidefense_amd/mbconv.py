"""The MBConv block nodes of the EfficientNet trunk (tape.py holds the operators): one block = one call and, with a tape, ONE
tape node.  mbconv_fused: training mode, deferred BatchNorms, in named stages over one _Block state; mbconv_eval_half /
mbconv_frozen_half: the fp16 runners' forward (one _half_forward) without / with the frozen half backward; mbconv_eval: the fp32
runner's node; stem_fused: the stem in front of block 0.  All read sizes, pads and weight views from block_geom(blk, x); the
model's trunk loop picks the form by a TrunkMode (model.unidefense._run / _blocks).  DESIGN.md 3a.
"""
import collections
from types import SimpleNamespace

import torch

from . import kernels as K
from . import tape as T
from .config import cfg


# How the model's trunk loop runs its blocks (_run decides once, _blocks dispatches).  kind: FUSED (training: mbconv_fused; dp = the
# DataParallelCtx), HALF (the fp16 runners: mbconv_eval_half, with a tape mbconv_frozen_half), EVAL_NODE (the fp32 runner: mbconv_eval
# where eval_block_ok) or OPERATORS (tape.py's operators); wt: {id(depthwise weight): its tap-major copy} (kernels.dw_weights_tapmajor)
FUSED, HALF, EVAL_NODE, OPERATORS = "fused", "half", "eval_node", "operators"
TrunkMode = collections.namedtuple("TrunkMode", "kind wt dp", defaults=(None,))


# Stride-1 depthwise convs of the fused MBConv node on the LDS-tiled kernels of csrc/dwtile.hip (the deferred BatchNorm is
# applied while the halo tile is staged: swish(bn0(e)) is never materialised) WHERE THEY WIN — measured per shape against
# the strip kernels with tools/bench_dwtile.py on an MI355X (profiles/r03/dwtile_f32_bs32.txt, dwtile_f16_bs64.txt):
#   half storage  : everywhere, by 1.3 - 3x (forward 109 -> 53, data gradient 260 -> 86, weight gradient 284 -> 106 us ...:
#                   the strip kernels' per-tap 8-byte window loads and conversions);
#   fp32 forward  : every block (one launch replaces bn_apply + conv + colstats of the plain blocks: 118 -> 74, 63 -> 43,
#                   121 -> 52, 37 -> 23 us; SF blocks 43 -> 33, 31 -> 23 us) but the 5x5 / 8x8 maps (16 vs 14 us);
#   fp32 data grad: 5x5 at 16x16 and 32x32 (70 -> 49, 45 -> 36 us) and 3x3 at 32x32 ... 64x64 (101 -> 94 us); the strip kernel
#                   keeps the 8x8 and 128x128 maps;
#   fp32 weight grad: the plain blocks (63 -> 54, 66 -> 55 us at 128^2 / 64^2; they have no materialised activation any
#                   more); the SF blocks keep the strip kernel (36 vs 45, 23 vs 29 us) on the activation rfft2_ex writes.
_DW_TILED = True


# per-shape overrides of the two depthwise policies below, {(sf, k, stride, H, half): value}: measured IN the replayed step by
# tools/tune_in_step.py --knobs (the rules come from per-kernel timings); empty = the rules
_DW_TILE_OVERRIDE = {}
_DW_BWD_FUSED_OVERRIDE = {}


def _dw_tile_policy(sf, k, stride, H, half):
    """(forward, weight gradient, data gradient) on the tiled kernels?"""
    ov = _DW_TILE_OVERRIDE.get((bool(sf), k, stride, H, bool(half)))
    if ov is not None and _DW_TILED:
        return ov
    return _dw_tile_rule(sf, k, stride, H, half)


def _dw_tile_rule(sf, k, stride, H, half):
    if not _DW_TILED:
        return False, False, False
    if stride == 2:
        # the four down-sampling blocks (profiles/r03/dwtile_stride2.txt).  Data gradient through the zero-stuffed tile, with
        # the BatchNorm sums in its epilogue instead of a pass of their own: 189 -> 88, 59 -> 40, 57 -> 32 us (fp32), but not
        # on the 128 x 128 map in half storage (630 -> 699); forward 271 -> 130 us on the plain 128 x 128 block (incl. the
        # BatchNorm apply + statistics passes it absorbs), otherwise only on the large maps; weight gradient: half storage
        # (515 -> 177, 208 -> 100 us) and the plain block, the strip kernel elsewhere (49 vs 63 us)
        if half:
            return True, True, H < 128
        return (not sf) or H >= 64, not sf, True
    if half:
        return True, True, True
    fwd = not (k == 5 and H <= 8)
    bwd = (k == 5 and H >= 16) or (k == 3 and 32 <= H <= 64)
    return (fwd or not sf), not sf, bwd


# Round 5: the stride-1 blocks' depthwise data gradient and weight gradient as ONE kernel (kernels.dwtile_bwd: both halo tiles
# staged once; the separate kernels read dy and the conv's input twice each).  Where it is used: _dw_bwd_fused_policy.
def _dw_bwd_fused_policy(sf, k, stride, H, half):
    """data + weight gradient of this depthwise conv in one launch (csrc/dwtile.hip: dw_tile_bwd_kernel)?  Measured per shape
    against the pair of kernels _dw_tile_policy picks (tools/bench_dwbwd.py on an MI355X, profiles/r05/dwbwd_*.txt; us, pair ->
    fused): fp32 bs 32: 128^2 187 -> 151 and 74 -> 61, 32^2 k5 100 -> 81, 16^2 k5 70 -> 63, 16^2 k3 47 -> 45, 8^2 k3 47 -> 45;
    NOT the 64^2 k3 blocks (132 vs 134: two halo tiles of a 16 x 8 tile are 1.4x its pixels, twice) and NOT the 8^2 k5 blocks
    (48 vs 60: one workgroup per CU next to the strip kernels' eight).  Half storage bs 64: 328 -> 260, 90 -> 80, 224 -> 211,
    163 -> 156, 73 -> 71; a tie at 16^2 k5 and 8^2 k3, 72 vs 96 at 8^2 k5."""
    if stride != 1:
        return False
    ov = _DW_BWD_FUSED_OVERRIDE.get((bool(sf), k, stride, H, bool(half)))
    if ov is not None:
        return ov
    if H <= 8:
        return k == 3 and not half
    if half:
        return True
    return not (k == 3 and H == 64)


# The SE / BatchNorm-1 backward without dz1: the BatchNorm sums are linear in the per-sample gate and dpool, so the
# dot pass sums four more per-sample dots (K.coldot_bn_se), the second SE FC launch folds them into the sums (K.se_bwd(fold=...))
# and the apply pass forms dz1 on load from dc (K.normbwd_apply_se / _mix_se): se_scale_bwd_bn is not launched, dz1 never written.
_SE_BN1_FOLD_OVERRIDE = {}


def _se_bn1_fold_policy(sf, stride, Ho, Ce, half):
    """BatchNorm-1 backward sums from per-sample dots, dz1 formed on load?  For the blocks whose project conv's data gradient dc
    is a tensor (not pj_fused), fp32 storage.  Measured per block shape, old chain against new (tools/bench_se_bn1_fold.py on an
    MI355X, profiles/r23/se_bn1_fold.txt; us, bs 32): plain 128^2 x 48 155 -> 93 and x 24 90 -> 56, SF stride 2 16^2 x 336 41 -> 30,
    SF 16^2 x 672 55 -> 42 and x 960 67 -> 50, SF stride 2 8^2 x 960 32 -> 25, SF 8^2 x 1632 49 -> 43, plain 8^2 x 1632 44 -> 38 and
    x 2688 62 -> 51: every shape of the step wins, so the rule is "on"; the override keeps the old chain reachable per shape."""
    if half:
        return False
    ov = _SE_BN1_FOLD_OVERRIDE.get((bool(sf), stride, Ho, Ce))
    if ov is not None:
        return ov
    return True


# The same fold on the blocks whose project conv is thin (pj_fused: no dc tensor): K.project_bwd_fused_a_se sums the dots
# inside the weight-gradient pass, K.se_bwd(fold=...) folds them, and K.project_bwd_fused_c / _c_mix is project_bwd_fused_b and the
# BN1 apply in one pass — dz1 stays in registers.
_PJ_BN1_FOLD_OVERRIDE = {}
# (sf, stride, Ho, Ce) -> routed?  One entry per block shape MEASURED; a shape that is not in the table keeps passes A and B.
_PJ_BN1_FOLD_RULE = {(False, 2, 64, 144): True, (False, 1, 64, 192): True, (True, 2, 32, 192): True, (True, 1, 32, 336): True}


def _pj_bn1_fold_policy(sf, stride, Ho, Ce):
    """BatchNorm-1 backward folded into the thin-project passes (A with the five dots, C instead of B + the apply)?  For the blocks
    on ud_pj_bwd_fused_a / _b (pj_fused: fp32 storage by construction) whose (Ce, Co) pair K.project_bwd_fold_ok takes.  Measured per
    block shape, old chain against new (tools/bench_se_bn1_fold.py on an MI355X, profiles/r28/pj_bn1_fold.txt; us, bs 32): plain
    stride 2 64^2 x 144 129 -> 103, plain 64^2 x 192 155 -> 114, SF stride 2 32^2 x 192 79 -> 63, SF 32^2 x 336 120 -> 98 (pass A
    costs 7-15 us more for its second BatchNorm + swish evaluation; pass C is FASTER than pass B, and the apply launch is gone):
    every shape of the UDEB4 step at 256 x 256 wins and is on.  Shapes nobody measured stay off; the override reaches any shape."""
    key = (bool(sf), stride, Ho, Ce)
    ov = _PJ_BN1_FOLD_OVERRIDE.get(key)
    if ov is not None:
        return ov
    return _PJ_BN1_FOLD_RULE.get(key, False)


# ONE geometry per (block, input shape), read by all five nodes.
# sizes: x [N,H,W,Cin] (M pixels) -> expanded [N,H,W,Ce] -> depthwise [N,Ho,Wo,Ce] (HWo per sample, Mo pixels) -> [N,Ho,Wo,Co];
# pt / pl: the depthwise conv's top / left zero pad.  2-D weight views: We expand [Ce,Cin] (None: no expand conv), Wsr / Wse the
# squeeze-excite FCs [Cs,Ce] / [Ce,Cs], Wp project [Co,Ce], Wf the spectral conv [2Ce,2Ce] (None: not an SF block).
# sf: an SF block; then alpha its gate parameter and s_f / s_i the forward / inverse transform scales.
# Built per call: a parameter replaced by load_state_dict or .to() must not leave a stale view behind.
BlockGeom = collections.namedtuple(
    "BlockGeom", "N H W Cin M k stride pt pl Ho Wo HWo Mo Ce Co Cs We Wsr Wse Wp Wf sf alpha s_f s_i")


def block_geom(blk, x):
    """The BlockGeom of parameter container `blk` (model.unidefense._MBConvParams) applied to x [N,H,W,Cin]."""
    sp = blk.spec
    N, H, W, Cin = x.shape
    Ho, Wo = T.conv_out_hw(H, W, sp.k, sp.stride, sp.pad)
    Ce, Co, Cs = sp.cexp, sp.cout, sp.cse
    sf = sp.sf_norm is not None
    dwm = blk._depthwise_conv
    s_f, s_i = T._fft_scales(H, sp.sf_norm) if sf else (None, None)
    return BlockGeom(N, H, W, Cin, N * H * W, sp.k, sp.stride, sp.pad[2], sp.pad[0], Ho, Wo, Ho * Wo, N * Ho * Wo, Ce, Co, Cs,
                     blk._expand_conv.weight.view(Ce, Cin) if sp.expand != 1 else None,
                     blk._se_reduce.weight.view(Cs, Ce), blk._se_expand.weight.view(Ce, Cs), blk._project_conv.weight.view(Co, Ce),
                     dwm.freq_conv.weight.view(2 * Ce, 2 * Ce) if sf else None, sf, dwm.sf_coef if sf else None, s_f, s_i)


# ---- idioms the nodes share ----
def _grad_like(dout, out):
    """the incoming gradient, contiguous and in the output's shape"""
    return dout if (dout.is_contiguous() and dout.shape == out.shape) else dout.reshape(out.shape).contiguous()


def _skip_into_add(skip, add, dout):
    """Where a skip block's identity gradient goes when the block ends in a depthwise data-gradient kernel: into that kernel's
    `add` operand where it is free (no spectral branch claims it), else a pass afterwards.  Returns (add, skip_done)."""
    if skip and add is None:
        return dout, True
    return add, not skip


def _expand_dgrad(tape, skip, dout, x, product):
    """The expand conv's data gradient (+ the skip gradient).  product(acc) runs it and returns a tuple that starts with dx
    [M, Cin]: accumulated onto acc — dout itself, in place: the skip gradient for free — where the tape owns dout and no test
    watches it; else acc is None and the skip gradient is a pass afterwards.  Returns that tuple with dx finished, shaped like x."""
    acc = dout.view(-1, x.shape[-1]) if (skip and tape.watch is None and getattr(dout, "_ud_owned", False)) else None
    dx, *rest = product(acc)
    dx = dx.view(x.shape)
    if skip and acc is None:
        dx = K.axpby(dx, 1.0, dout, 1.0, out=dx)
    return (dx, *rest)


def _gemm_dy(ctx, dy, like):
    """The dy operand of a 1x1 conv's backward products (K.spectral_bwd(ctx, dy2, dy_absmax=amax)) from what its producer wrote:
    Planes are parked in ctx.dy — the launch wrappers then only want a tensor of the right device and, half storage (one plane),
    of the results' dtype: `like`; a row-major tensor goes as [rows, C] with its absmax side output.  Returns (dy2, amax)."""
    if isinstance(dy, K.Planes):
        ctx.dy = dy
        return (like if dy.prec == 1 else ctx.w.buf), None
    return dy.view(-1, dy.shape[-1]), getattr(dy, "_ud_absmax", None)


def _normbwd_to_gemm(ctx, pl, x, dy, keep, inv_keep, bn, is_dz, G, R, sacc, loc):
    """BatchNorm backward apply in front of a 1x1 conv's backward: pl (K.normbwd_planes_ok) — the apply pass writes the conv's dy
    operand as planes itself — else a row-major tensor + absmax.  Returns (dy2, amax, dgamma, dbeta): _gemm_dy."""
    if pl:
        t, dg, db = K.normbwd_apply_planes(x, dy, keep, inv_keep, bn, is_dz, G, R, sacc, loc)
    else:
        t, dg, db = K.normbwd_apply(x, dy, keep, inv_keep, bn, is_dz, G, R, sacc, loc, want_absmax=True)
    return _gemm_dy(ctx, t, dy) + (dg, db)


# the form in which a transform hands its result to the spectral GEMM
_ROWS, _PLANE_HALF, _PLANES = 0, 1, 2


def _rfft2_as(form, x, scale, w_interior, **kw):
    """rfft2_ex in the form the spectral GEMM takes its operand in.  _PLANES: the transform writes the GEMM's fp16 x 2 planes itself
    (scale from an a-priori bound): no split pass; _PLANE_HALF: the mixed-precision mode, the half result laid into the prec-1 plane
    by the transform (no layout pass); _ROWS: a row-major tensor + its absmax."""
    if form == _PLANES:
        return K.rfft2_ex_planes(x, scale, w_interior, **kw)
    if form == _PLANE_HALF:
        return K.rfft2_ex_plane_half(x, scale, w_interior, **kw)
    return K.rfft2_ex(x, scale, w_interior, want_absmax=True, **kw)


# ---- stem of the fused path ----
class LazyInput:
    """A block input that is still a raw conv output + deferred BatchNorm (the stem in front of block 0):
    backward(dz, sacc) receives the gradient already pushed through the activation and the BatchNorm sums."""

    def __init__(self, bn, backward):
        self.bn, self.backward = bn, backward


def _bn_of(mod, acc, count, act):
    return K.DeferredBN(acc, mod.num_features, count, mod.weight, mod.bias, mod.eps, act,
                        mod.momentum if mod.momentum is not None else 0.1, mod.running_mean, mod.running_var)


def stem_fused(tape, x_pix, w, bn_mod, stride, pad_t, pad_l, Ho, Wo, dp, storage=torch.float32, x_planes=None):
    """Stem conv (model/efficientnet/model.py:185-186) whose BatchNorm + swish is left to block 0's depthwise conv.
    storage: dtype the trunk keeps its activations in (torch.float16: the raw conv output is handed on rounded).
    x_planes: the input image as planes (its gradient is formed when it is the tape's tracked input; conv_dense)."""
    h32 = T.conv_dense(tape, x_pix, w, stride, pad_t, pad_l, Ho, Wo, need_dx=False, x_planes=x_planes)
    h = h32 if storage == torch.float32 else h32.to(storage)
    Cc = h.shape[-1]
    M = h.numel() // Cc
    acc = K.zeros64(2 * Cc, h)
    K.colstats(h.view(M, Cc), acc)
    dp.reduce(acc)
    bn = _bn_of(bn_mod, acc, M * dp.world, 1)

    def backward(dz, sacc, is_dz):
        loc = dp.reduce(sacc, keep_local=True)
        dh, dg, db = K.normbwd_apply(h, dz, None, 1.0, bn, is_dz, 1, M, sacc, loc)
        tape.add_param_grad(bn_mod.weight, dg)
        tape.add_param_grad(bn_mod.bias, db)
        tape.add_grad(h32, dh if dh.dtype == h32.dtype else dh.to(h32.dtype))
    return h, LazyInput(bn, backward)


# ---------------------------------------------------------------------------------------------
# Fused MBConv block: deferred BatchNorm, one tape node per block (csrc/fused.hip)
# ---------------------------------------------------------------------------------------------
class _Block:
    """State of one mbconv_fused call: arguments, geometry, the route flags a later stage reads (t_*, irdw, c_pl) and what the
    backward needs — nothing else: an intermediate no later stage reads stays a local of its stage.
    src / src_bn: the depthwise conv's raw input and the deferred BatchNorm + swish in front of it (e / bn0; without an expand conv
    x and lazy_in's BatchNorm or None); a: swish(src_bn(src)) where a strip kernel needed it materialised, else None; spat: the
    spatial branch, kept by the stride-2 SF blocks only; fr: freq - spat (stride 1) or freq (stride 2)."""
    __slots__ = ("blk", "geo", "x", "keep", "inv_keep", "wt", "dp", "lazy_in", "e", "ectx", "bn0", "src", "src_bn", "a",
                 "t_wg", "t_bwd", "t_fused", "irdw", "spat", "fr", "sctx", "xf_shape", "d", "bn1", "pool", "s1", "s2", "c_pl",
                 "p4", "pctx", "bn2", "out")


def mbconv_fused(tape, x, blk, keep, keep_prob, wt, dp, lazy_in=None, next_blk=None):
    """MBConvBlock.forward (model/efficientnet/model.py:94-135) in training mode as ONE tape node.
    x [N,H,W,Cin]: the block input (for block 0: the raw stem output, lazy_in its deferred BatchNorm);
    wt: the depthwise weight in tap-major layout [k*k][C]; keep: drop-connect keep vector [N] or None.

    Forward (SF block, stride 1):  expand GEMM -> colstats -> rfft2 of swish(bn0(e)) (also writes the activated
    tensor) -> depthwise conv | spectral GEMM -> irfft2 + SF mix + BN1 statistics -> SE pooling of swish(bn1(d)) ->
    2 small FCs -> BN1 + swish + gate -> project GEMM -> colstats -> BN2 + drop-connect + skip.
    Backward mirrors it with the BatchNorm backward sums accumulated by the kernel that produces the gradient."""
    assert not (blk.spec.skip and lazy_in is not None)
    b = _Block()
    b.blk, b.geo, b.x, b.keep, b.inv_keep, b.wt, b.dp, b.lazy_in = blk, block_geom(blk, x), x, keep, 1.0 / keep_prob, wt, dp, lazy_in
    _fwd_expand(b)
    _fwd_depthwise(b)
    c_amax = _fwd_se(b)
    _fwd_project(b, c_amax, next_blk)
    if T._needs(tape):
        tape.record(lambda: _fused_backward(b, tape))
    return b.out


def _fwd_expand(b):
    """expand conv + BN0 statistics (BN0 + swish are deferred: the depthwise stage's kernels apply them on load)"""
    g, x, blk = b.geo, b.x, b.blk
    if g.We is None:
        b.e = b.bn0 = b.ectx = None
        b.src, b.src_bn = x, (b.lazy_in.bn if b.lazy_in is not None else None)
        return
    acc0 = K.zeros64(2 * g.Ce, x)
    xp = getattr(x, "_ud_planes", None)          # the previous block's residual pass wrote this conv's operand planes itself
    if xp is not None and not (xp.R == g.M and xp.C == g.Cin and K.spectral_takes_planes(g.M, g.Ce, g.Cin, g.We, want_stats=True)):
        xp = None
    # BN0 statistics in the GEMM epilogue where the launch is plain
    (e, done), b.ectx = K.spectral_fwd(x.view(g.M, g.Cin) if xp is None else xp, g.We, stats=acc0, x_absmax=getattr(x, "_ud_absmax", None))
    if not done:
        K.colstats(e, acc0)
    b.e = e.view(g.N, g.H, g.W, g.Ce)
    b.dp.reduce(acc0)
    b.bn0 = _bn_of(blk._bn0, acc0, g.M * b.dp.world, 1)
    b.src, b.src_bn = b.e, b.bn0


def _fwd_depthwise(b):
    """depthwise / SF conv -> d (pre-BN1) + BN1 statistics.  Sets the depthwise route flags: t_wg / t_bwd (weight / data gradient
    on the tiled kernels), t_fused (both in one launch), irdw (SF, 8 x 8 maps: both inside the adjoint transform's kernel)."""
    g, x = b.geo, b.x
    acc1 = K.zeros64(2 * g.Ce, x)
    half = x.dtype == torch.float16
    t_fwd, b.t_wg, b.t_bwd = _dw_tile_policy(g.sf, g.k, g.stride, g.H, half)
    b.t_fused = _dw_bwd_fused_policy(g.sf, g.k, g.stride, g.H, half)
    b.irdw, b.spat, b.fr, b.sctx, b.xf_shape = False, None, None, None, None
    if g.sf:
        _fwd_sf(b, t_fwd, acc1)
    elif t_fwd:
        # halo tile staged in LDS with swish(bn0(e)) applied on the way in; BN1 statistics out of the epilogue
        b.a = None
        b.d = K.dwtile_fwd(b.src, b.wt, g.k, g.pt, g.pl, g.Ho, g.Wo, bn=b.src_bn, stats=acc1, update=True, stride=g.stride)
    else:
        # the strip kernel (and its weight gradient) re-reads its input per tap: materialise the activation
        b.a = K.bn_apply(b.src, b.src_bn, 1, g.M, update=True) if b.src_bn is not None else b.src
        b.d = K.dwconv_fwd(b.a, b.wt, g.k, g.stride, g.pt, g.pl, g.Ho, g.Wo)
        K.colstats(b.d.view(g.Mo, g.Ce), acc1)
    b.dp.reduce(acc1)
    b.bn1 = _bn_of(b.blk._bn1, acc1, g.Mo * b.dp.world, 1)


def _fwd_sf(b, t_fwd, acc1):
    """the SF block's conv: the depthwise conv of a = swish(bn0(e)) | rfft2(a) -> spectral 1x1 conv -> irfft2, mixed by the gate"""
    g, x, src, src_bn, wt, pad = b.geo, b.x, b.src, b.src_bn, b.wt, b.blk.spec.pad
    S, k, stride, Ce = g.H, g.k, g.stride, g.Ce
    spat = None
    if src_bn is not None:
        # 8 x 8 maps: the adjoint transform's kernel also does the depthwise conv's backward over the planes it holds
        b.irdw = K.irfft2_dwbwd_ok(S, k, stride, pad, x.dtype)
        # a strip kernel needs a = swish(bn0(e)) materialised (rfft2_ex writes it); the tiled ones apply it on load
        bwd_on_load = b.t_wg or b.t_fused or b.irdw          # (the backward then needs no materialised a)
        if K.rfft2_planes_ok(src, src_bn) and K.spectral_takes_planes(g.N * S * (S // 2 + 1), 2 * Ce, 2 * Ce, g.Wf):
            form = _PLANES
        elif K.rfft2_plane_half_ok(src) and K.spectral_takes_plane_half(g.N * S * (S // 2 + 1), 2 * Ce, 2 * Ce):
            form = _PLANE_HALF
        else:
            form = _ROWS
        if form != _ROWS and K.rfft2_dw_ok(S, k, stride, pad):
            # ... and, stride 1, the depthwise conv of the plane it holds anyway: no conv kernel either
            xf, a, spat = _rfft2_as(form, src, g.s_f, 1.0, bn=src_bn, want_act=not bwd_on_load, update=True, dw_wt=wt, dw_k=k)
        else:
            xf, a = _rfft2_as(form, src, g.s_f, 1.0, bn=src_bn, want_act=not (t_fwd and bwd_on_load), update=True)
    else:
        xf, a = K.rfft2(src, g.s_f, 1.0, want_absmax=True), src
    if spat is None and t_fwd:
        spat = K.dwtile_fwd(src, wt, k, g.pt, g.pl, g.Ho, g.Wo, bn=src_bn, stride=stride)
    elif spat is None:
        spat = K.dwconv_fwd(a, wt, k, stride, g.pt, g.pl, g.Ho, g.Wo)
    b.a = a
    b.xf_shape = (g.N, S, S // 2 + 1, 2 * Ce)
    if isinstance(xf, K.Planes):
        yf, b.sctx = K.spectral_fwd(xf, g.Wf)
    else:
        yf, b.sctx = K.spectral_fwd(xf.view(-1, 2 * Ce), g.Wf, x_absmax=getattr(xf, "_ud_absmax", None))
    yf = yf.view(b.xf_shape)
    xf = None          # the context holds what the backward needs of it
    if stride == 1:
        b.d, b.fr = K.irfft2_mix(yf, g.s_i, spat, g.alpha, acc1)          # fr: freq - spat (neither branch is kept)
        spat = None
    else:
        b.fr = K.irfft2(yf, g.s_i, 1.0)
        b.d = K.sfmix_fwd(spat, b.fr, g.alpha, True)
        K.colstats(b.d.view(g.Mo, Ce), acc1)
        b.spat = spat
    del yf


def _fwd_se(b):
    """squeeze-excite on swish(bn1(d)): the pooled sums and the two FCs (the gate is applied by the project stage).  Sets c_pl:
    the project conv takes the gated tensor as planes; returns their scale's source, max |swish(bn1(d))| (else None)."""
    g, x, blk, d = b.geo, b.x, b.blk, b.d
    b.pool = K.zeros64(g.N * g.Ce, x)
    # project conv on the planes GEMM: the gated tensor c is written as its planes by se_scale_bn itself, scaled by
    # max |swish(bn1(d))| — which the SE squeeze pass leaves behind (kernels.colsum_bn_amax)
    b.c_pl = (d.dtype == torch.float32 and g.Ce % 32 == 0 and cfg.spectral_p2 != "off"
              and K.spectral_takes_planes(g.Mo, g.Co, g.Ce, g.Wp, want_stats=True))
    c_amax = None
    if b.c_pl:
        c_amax = K.colsum_bn_amax(d, b.bn1, g.N, g.HWo, b.pool, update=True)
    else:
        K.colsum_bn(d, b.bn1, g.N, g.HWo, b.pool, update=True)
    b.s1 = K.fc_fwd_d(b.pool, 1.0 / g.HWo, g.Wsr, blk._se_reduce.bias, g.N)
    b.s2 = K.fc_fwd(b.s1, g.Wse, blk._se_expand.bias, 1)
    return c_amax


def _fwd_project(b, c_amax, next_blk):
    """BN1 + swish + gate -> c, project conv + BN2 statistics, BN2 + drop-connect + skip -> out"""
    g, x, blk, d, bn1, s2 = b.geo, b.x, b.blk, b.d, b.bn1, b.s2
    acc2 = K.zeros64(2 * g.Co, x)
    if not b.c_pl and K.project_fwd_fused_ok(d, g.Wp, g.HWo):
        # thin project conv (the 64 x 64 blocks): gate applied on load, BatchNorm-2 statistics out of the epilogue, c never written
        # (its backward re-makes c as well: csrc/pjbwd.hip)
        p, b.pctx = K.project_fwd_fused(d, bn1, s2, g.Wp, g.N, g.HWo, stats=acc2)
        done = True
    elif b.c_pl:
        c = K.se_scale_bn_planes(d, bn1, s2, g.N, g.HWo, c_amax)
        (p, done), b.pctx = K.spectral_fwd(c, g.Wp, stats=acc2)
    elif (d.dtype == torch.float16 and g.Ce % 8 == 0 and K.spectral_takes_plane_half(g.Mo, g.Co, g.Ce)):
        c = K.se_scale_bn_plane_half(d, bn1, s2, g.N, g.HWo)          # the mixed-precision mode: no row-major c, no layout pass
        (p, done), b.pctx = K.spectral_fwd(c, g.Wp, stats=acc2)
    else:
        c = K.se_scale_bn(d, bn1, s2, g.N, g.HWo, want_absmax=True)
        (p, done), b.pctx = K.spectral_fwd(c.view(g.Mo, g.Ce), g.Wp, stats=acc2, x_absmax=getattr(c, "_ud_absmax", None))
    if not done:
        K.colstats(p, acc2)
    b.dp.reduce(acc2)
    b.bn2 = _bn_of(blk._bn2, acc2, g.Mo * b.dp.world, 0)
    b.p4 = p.view(g.N, g.Ho, g.Wo, g.Co)
    # the block output is the next block's expand-conv operand: written as that GEMM's planes in the same pass where it takes them
    nxt = None
    if next_blk is not None and next_blk.spec.expand != 1:
        nxt = (g.Mo, next_blk.spec.cexp, next_blk._expand_conv.weight.view(next_blk.spec.cexp, g.Co))
    b.out = K.residual_bn(b.p4, b.bn2, b.keep, b.inv_keep, x if blk.spec.skip else None, g.N, g.HWo, update=True, want_absmax=True, planes_for=nxt)


def _fused_backward(b, tape):
    """The node's backward: the stages below in order.  gr holds the gradients in flight and the routes chosen on the way, for
    this replay only (each stage's docstring names what it leaves there)."""
    dout = tape.pop_grad(b.out)
    if dout is None:
        return
    gr = SimpleNamespace(dout=_grad_like(dout, b.out))
    _bwd_project(b, tape, gr)
    _bwd_se(b, tape, gr)
    _bwd_bn1(b, tape, gr)
    _bwd_depthwise(b, tape, gr)
    dx = gr.dx if b.src_bn is None else _bwd_expand(b, tape, gr)
    if dx is not None:
        dx._ud_owned = True
        tape.add_grad(b.x, dx)


def _bwd_project(b, tape, gr):
    """BN2 (+ drop-connect scale) and the project conv -> gr.dp2 (the gradient of the project output, [Mo, Co] or the planes'
    placeholder), gr.dc (the gated tensor's gradient; None where pj_fused), gr.dgate (the SE gate's, fp64 sums), gr.pj_fused,
    gr.se_dots (None, or [5 N Ce] fp64: dgate and the four dots of the BN1 sums — the route of _se_bn1_fold_policy)."""
    g, x, blk, dout = b.geo, b.x, b.blk, gr.dout
    # the project conv's backward on the planes GEMM: the apply pass writes its operand's planes itself, scaled by the bound
    # the sums pass leaves behind (the energy of the incoming gradient: a third sum)
    dp_pl = K.normbwd_planes_ok(b.p4, b.pctx)          # (1: fp32, the energy bound as a third sum; 2: half storage, one plane)
    sb2 = K.zeros64((3 if dp_pl == 1 else 2) * g.Co, x)
    K.normbwd_sums(b.p4, dout, b.keep, b.inv_keep, b.bn2, False, g.N, g.HWo, sb2)
    loc2 = b.dp.reduce(sb2, keep_local=True)
    gr.dp2, dp_amax, dg2, db2 = _normbwd_to_gemm(b.pctx, dp_pl, b.p4, dout, b.keep, b.inv_keep, b.bn2, False, g.N, g.HWo, sb2, loc2)
    tape.add_param_grad(blk._bn2.weight, dg2)
    tape.add_param_grad(blk._bn2.bias, db2)
    # thin project conv (the 64 x 64 blocks): its data gradient dc is never written — each of the two passes over d that need it
    # re-makes its tile from the thin dp (csrc/pjbwd.hip)
    gr.pj_fused = not dp_pl and b.pctx.plans is None and K.project_bwd_fused_ok(b.d, g.Wp, g.HWo)
    assert gr.pj_fused or b.pctx.x is not None, "the fused project forward kept no gated tensor: its backward must be the fused one"
    gr.se_dots = None
    if gr.pj_fused:
        gr.dc = None
        if K.project_bwd_fold_ok(g.Wp, g.HWo) and _pj_bn1_fold_policy(g.sf, g.stride, g.Ho, g.Ce):
            gr.se_dots = K.zeros64(5 * g.N * g.Ce, x)
            gr.dgate = gr.se_dots[:g.N * g.Ce]
            dWp = K.project_bwd_fused_a_se(b.d, b.bn1, b.s2, gr.dp2, g.Wp, g.N, g.HWo, gr.se_dots)
        else:
            gr.dgate = K.zeros64(g.N * g.Ce, x)
            dWp = K.project_bwd_fused_a(b.d, b.bn1, b.s2, gr.dp2, g.Wp, g.N, g.HWo, gr.dgate)
    else:
        dc, dWp = K.spectral_bwd(b.pctx, gr.dp2, dy_absmax=dp_amax)          # (one launch for both where that fills the chip better)
        gr.dc = dc.view(g.N, g.Ho, g.Wo, g.Ce)
        if _se_bn1_fold_policy(g.sf, g.stride, g.Ho, g.Ce, b.d.dtype != torch.float32 or dc.dtype != torch.float32):
            gr.se_dots = K.zeros64(5 * g.N * g.Ce, x)
            gr.dgate = gr.se_dots[:g.N * g.Ce]
            K.coldot_bn_se(gr.dc, b.d, b.bn1, g.N, g.HWo, gr.se_dots)
        else:
            gr.dgate = K.zeros64(g.N * g.Ce, x)
            K.coldot_bn(gr.dc, b.d, b.bn1, g.N, g.HWo, gr.dgate)
    tape.add_param_grad(blk._project_conv.weight, dWp)


def _bwd_se(b, tape, gr):
    """the two SE FCs, then gate + swish + the BN1 backward sums in one pass -> gr.dz1, gr.sb1 (summed over the ranks), gr.loc1;
    gr.se_dots given: the sums come out of the second FC launch, gr.dz1 is None and gr.dpool is kept for the apply pass"""
    g, blk = b.geo, b.blk
    gr.sb1 = K.zeros64(2 * g.Ce, b.x)
    fold = (gr.se_dots, 1.0 / g.HWo, gr.sb1) if gr.se_dots is not None else None
    dpool, dWe2, dbe2, dWr, dbr = K.se_bwd(gr.dgate, b.s2, b.s1, g.Wse, g.Wsr, b.pool, 1.0 / g.HWo, fold=fold)
    tape.add_param_grad(blk._se_expand.weight, dWe2)
    tape.add_param_grad(blk._se_expand.bias, dbe2)
    tape.add_param_grad(blk._se_reduce.weight, dWr)
    tape.add_param_grad(blk._se_reduce.bias, dbr)
    gr.dpool = dpool
    if fold is not None:
        gr.dz1 = None
    elif gr.pj_fused:
        gr.dz1 = K.project_bwd_fused_b(b.d, b.bn1, b.s2, dpool, 1.0 / g.HWo, gr.dp2, g.Wp, g.N, g.HWo, gr.sb1)
    else:
        gr.dz1 = K.se_scale_bwd_bn(gr.dc, b.d, b.bn1, b.s2, dpool, 1.0 / g.HWo, g.N, g.HWo, gr.sb1)
    gr.loc1 = b.dp.reduce(gr.sb1, keep_local=True)


def _bn1_apply(b, gr):
    """the BN1 backward apply from dz1 or, where dz1 was never written (gr.se_dots), from dc through the SE gate — a tensor, or
    (pj_fused: gr.dc is None) re-made per tile from the thin dp2 inside the pass"""
    g = b.geo
    if gr.dz1 is None and gr.dc is None:
        return K.project_bwd_fused_c(b.d, b.bn1, b.s2, gr.dpool, 1.0 / g.HWo, gr.dp2, g.Wp, g.N, g.HWo, gr.sb1, gr.loc1)
    if gr.dz1 is None:
        return K.normbwd_apply_se(b.d, gr.dc, b.bn1, b.s2, gr.dpool, 1.0 / g.HWo, g.N, g.HWo, gr.sb1, gr.loc1)
    return K.normbwd_apply(b.d, gr.dz1, None, 1.0, b.bn1, True, g.N, g.HWo, gr.sb1, gr.loc1)


def _bwd_bn1(b, tape, gr):
    """BN1 apply; SF blocks: the mix's adjoint, the adjoint of irfft2 and the spectral GEMM's backward.  Leaves gr.g_sp (the
    depthwise conv's output gradient, to be scaled by the gate: gr.g_alpha / gr.g_mode) and, SF: gr.dxf (the gradient of the
    spectrum of a) or, already through the adjoint of rfft2, gr.da_f — where not irdw, whose kernel does that itself."""
    g, x, blk, d = b.geo, b.x, b.blk, b.d
    gr.g_alpha, gr.g_mode, gr.da_f, gr.dxf = None, 0, None, None
    if not g.sf:
        gr.g_sp, dg1, db1 = _bn1_apply(b, gr)
    else:
        alpha, sctx = g.alpha, b.sctx
        if g.stride == 1:
            dacc = K.zeros64(64, x)
            dyf_pl = sctx.plans is not None and K.rfft2_planes_ok(d, None)
            en = K.zeros64(g.Ce, x) if dyf_pl else None
            if gr.dz1 is None and gr.dc is None:
                dd, dg1, db1 = K.project_bwd_fused_c_mix(d, b.bn1, b.s2, gr.dpool, 1.0 / g.HWo, gr.dp2, g.Wp, g.N, g.HWo, gr.sb1,
                                                         b.fr, dacc, gr.loc1, energy=en)
            elif gr.dz1 is None:
                dd, dg1, db1 = K.normbwd_apply_mix_se(d, gr.dc, b.bn1, b.s2, gr.dpool, 1.0 / g.HWo, g.N, g.HWo, gr.sb1, b.fr, dacc,
                                                      gr.loc1, energy=en)
            else:
                dd, dg1, db1 = K.normbwd_apply_mix(d, gr.dz1, b.bn1, g.N, g.HWo, gr.sb1, b.fr, dacc, gr.loc1, energy=en)
            # adjoint of irfft2, x sigmoid(a); the same launch turns the accumulator slots into the gate's gradient
            # (_PLANES: ... and writes the GEMMs' planes itself: scale from the energy of dd the apply pass just summed)
            form = _PLANES if dyf_pl else _PLANE_HALF if (sctx.plans is not None and K.rfft2_plane_half_ok(dd)) else _ROWS
            bound = {"energy": en} if dyf_pl else {}
            dyf, _, dalpha = _rfft2_as(form, dd, g.s_i, 2.0, gate_alpha=alpha, gate_mode=1, gate_acc=dacc, **bound)
            tape.add_param_grad(alpha, dalpha)
            gr.g_sp, gr.g_alpha, gr.g_mode = dd, alpha, 2                                   # spatial branch: x (1 - sigmoid(a))
        else:
            dd, dg1, db1 = _bn1_apply(b, gr)
            gr.g_sp, dfr, dalpha = K.sfmix_bwd(b.spat, b.fr, alpha, dd, True)
            tape.add_param_grad(alpha, dalpha)
            dyf = K.rfft2(dfr, g.s_i, 2.0, want_absmax=True)
        dyf2, dyf_amax = _gemm_dy(sctx, dyf, dd)
        dxf, dWf = K.spectral_bwd(sctx, dyf2, dy_absmax=dyf_amax)
        tape.add_param_grad(blk._depthwise_conv.freq_conv.weight, dWf)
        gr.dxf = dxf.view(b.xf_shape)
        if not b.irdw:
            gr.da_f = K.irfft2(gr.dxf, g.s_f, 0.5)                                         # adjoint of rfft2
    tape.add_param_grad(blk._bn1.weight, dg1)
    tape.add_param_grad(blk._bn1.bias, db1)


def _expand_planes_route(b):
    """de_pl: does the BN0 backward apply write the expand conv's dy operand as planes (K.normbwd_planes_ok: 1 fp32, 2 half)?
    fp32 planes want the energy of dz0 as a third BatchNorm sum, which only the irdw kernel accumulates; the half plane needs no
    bound, whichever kernel produced dz0."""
    if b.e is None or b.lazy_in is not None:
        return 0
    pl = K.normbwd_planes_ok(b.e, b.ectx)
    return pl if (b.irdw or (pl == 2 and b.x.dtype == torch.float16)) else 0


def _bwd_depthwise(b, tape, gr):
    """The depthwise conv's weight gradient and its data gradient (+ the spectral branch), through swish(bn0(.)) when the input is
    deferred.  src_bn given: leaves gr.dz0, gr.sb0 (the BN0 backward sums; 3C where gr.de_pl == 1) and gr.is_dz (dz0 is already
    through swish'(bn0(.))); else gr.dx: the block's input gradient, the skip gradient in it."""
    g, x, blk, src, src_bn, wt = b.geo, b.x, b.blk, b.src, b.src_bn, b.wt
    k, stride, pt, pl, C0 = g.k, g.stride, g.pt, g.pl, src.shape[-1]
    g_sp, g_alpha, g_mode, da_f, dout = gr.g_sp, gr.g_alpha, gr.g_mode, gr.da_f, gr.dout
    skip, dwm = blk.spec.skip, blk._depthwise_conv
    gr.de_pl = _expand_planes_route(b)
    gr.is_dz = True          # every kernel below hands dz0 on through swish'(bn0(.)) — but the stride-2 gather
    gr.dz0 = gr.dx = dw_f = None
    if b.irdw:
        # (+ the energy of dz0 where the expand conv's backward takes its operand as planes: _normbwd_to_gemm in _bwd_expand)
        gr.sb0 = K.zeros64((3 if gr.de_pl == 1 else 2) * C0, x)
        gr.dz0, dw_f = K.irfft2_dwbwd(gr.dxf, g.s_f, 0.5, g_sp, src, src_bn, wt, k, g_alpha, g_mode, gr.sb0)
        tape.add_param_grad(dwm.weight, dw_f)
    elif b.t_fused:
        # ---- depthwise data + weight gradient in one pass over (dd, src)
        if src_bn is not None:
            gr.sb0 = K.zeros64(2 * C0, x)
            gr.dz0, dw_f = K.dwtile_bwd(g_sp, src, wt, k, pt, pl, bn=src_bn, gate_alpha=g_alpha, gate_mode=g_mode, add=da_f, sacc=gr.sb0)
        else:
            add, skip_done = _skip_into_add(skip, da_f, dout)
            gr.dx, dw_f = K.dwtile_bwd(g_sp, src, wt, k, pt, pl, gate_alpha=g_alpha, gate_mode=g_mode, add=add)
        tape.add_param_grad(dwm.weight, dw_f)
    elif b.t_wg:
        tape.add_param_grad(dwm.weight, K.dwtile_bwd_weight(src, g_sp, k, pt, pl, bn=src_bn, gate_alpha=g_alpha, gate_mode=g_mode, stride=stride))
    else:
        tape.add_param_grad(dwm.weight, K.dwconv_bwd_weight_ex(b.a, g_sp, g_alpha, g_mode, k, stride, pt, pl))
    if src_bn is not None:
        if gr.dz0 is not None:
            return                                     # the fused kernel above made dz0 and the BatchNorm sums
        gr.sb0 = K.zeros64(2 * C0, x)
        if b.t_bwd:
            gr.dz0 = K.dwtile_bwd_data(g_sp, wt, k, pt, pl, g.H, g.W, g_alpha, g_mode, da_f, src, src_bn, gr.sb0, stride=stride)
        elif stride == 1:
            gr.dz0 = K.dwconv_bwd_data_bn(g_sp, g_alpha, g_mode, wt, da_f, src, src_bn, k, stride, pt, pl, gr.sb0)
        else:       # stride 2 (4 of 32 blocks): gather kernel, then the sums as a pass of their own
            gr.dz0 = K.dwconv_bwd_data(g_sp, wt, k, stride, pt, pl, g.H, g.W, add=da_f)
            K.normbwd_sums(src, gr.dz0, None, 1.0, src_bn, False, 1, g.M, gr.sb0)
            gr.is_dz = False
        return
    if dw_f is None:
        add, skip_done = _skip_into_add(skip, da_f, dout)
        if b.t_bwd:
            gr.dx = K.dwtile_bwd_data(g_sp, wt, k, pt, pl, g.H, g.W, g_alpha, g_mode, add, stride=stride)
        else:
            gr.dx = K.dwconv_bwd_data_ex(g_sp, g_alpha, g_mode, wt, add, k, stride, pt, pl, g.H, g.W)
    if not skip_done:
        gr.dx = K.axpby(gr.dx, 1.0, dout, 1.0, out=gr.dx)


def _bwd_expand(b, tape, gr):
    """BN0 and the expand conv (a deferred input: src_bn given).  Returns the block's input gradient — None where the input was
    lazy (block 0: the stem's own backward takes dz0 and the sums from here)."""
    g, x, blk, e, ectx, dz0, sb0, dout = b.geo, b.x, b.blk, b.e, b.ectx, gr.dz0, gr.sb0, gr.dout
    skip = blk.spec.skip
    if b.lazy_in is not None:
        b.lazy_in.backward(dz0, sb0, gr.is_dz)
        return None
    loc0 = b.dp.reduce(sb0, keep_local=True)
    # thin expand conv (the 128 x 128 / 64 x 64 blocks): BatchNorm backward + both gradients in ONE pass over (dz0, e)
    thin = not gr.de_pl and e is not None and ectx.plans is None and K.expand_bwd_fused_ok(e, ectx.w, gr.is_dz)
    if thin:
        dx, dWe, dg0, db0 = _expand_dgrad(tape, skip, dout, x, lambda acc: K.expand_bwd_fused(e, dz0, b.bn0, sb0, loc0, ectx.x, ectx.w, add=acc))
    else:
        de2, de_amax, dg0, db0 = _normbwd_to_gemm(ectx, gr.de_pl, e, dz0, None, 1.0, b.bn0, gr.is_dz, 1, g.M, sb0, loc0)
    tape.add_param_grad(blk._bn0.weight, dg0)
    tape.add_param_grad(blk._bn0.bias, db0)
    if not thin:
        dx, dWe = _expand_dgrad(tape, skip, dout, x, lambda acc: K.spectral_bwd(ectx, de2, out=acc, dy_absmax=de_amax))
    tape.add_param_grad(blk._expand_conv.weight, dWe)
    return dx


# ---- half storage, eval mode: the fp16 runners' block (forward only, and as a tape node with the frozen backward) ----
def _half_forward(x, blk, g, wt, src_bn):
    """The eval-mode half-storage forward of a block, the ONE copy both nodes below run: every BatchNorm in the eval form
    (kernels.EvalBN: the running buffers, read in place), no batch statistics anywhere — no accumulator is handed to a producer
    and ud_colstats is never launched.  src_bn: the BatchNorm + swish in front of the depthwise conv of a block WITHOUT an expand
    conv (block 0: the stem's EvalBN, applied on load), else None.
    Returns (out, kept): kept holds what a backward needs — src (the depthwise conv's raw input: the expand output e, or x) and
    its src_bn, d (the raw depthwise / SF output), s1, s2, the EvalBNs bn1 / bn2 and xf_shape — and not the gated tensor, the
    spectra, the two SF branches, the pooled sums or any activated tensor: those are gone when this returns."""
    bn1 = K.EvalBN(blk._bn1, 1)
    if g.We is not None:
        src, src_bn = K.gemm_nt(x.view(g.M, g.Cin), g.We).view(g.N, g.H, g.W, g.Ce), K.EvalBN(blk._bn0, 1)
    else:
        src = x
    # depthwise conv of act(bn0(e)) from LDS halo tiles (the activation applied on load); SF blocks: the transform of the
    # same activated tensor, the spectral 1x1 conv, and the inverse transform mixed with the spatial branch
    spat = K.dwtile_fwd(src, wt, g.k, g.pt, g.pl, g.Ho, g.Wo, bn=src_bn, stride=g.stride)
    xf_shape = None
    if g.sf:
        xf, _ = K.rfft2_ex(src, g.s_f, 1.0, bn=src_bn)
        xf_shape = xf.shape
        yf = K.gemm_nt(xf.view(-1, 2 * g.Ce), g.Wf).view(xf_shape)
        if g.stride == 1:
            d, _ = K.irfft2_mix(yf, g.s_i, spat, g.alpha, None)
        else:
            d = K.sfmix_fwd(spat, K.irfft2(yf, g.s_i, 1.0), g.alpha, True)
        del xf, yf, spat
    else:
        d = spat
    # squeeze-excite on swish(bn1(d)), then the gated tensor -> project conv -> BN2 (+ skip)
    pool = K.zeros64(g.N * g.Ce, x)
    K.colsum_bn(d, bn1, g.N, g.HWo, pool)
    s1 = K.fc_fwd_d(pool, 1.0 / g.HWo, g.Wsr, blk._se_reduce.bias, g.N)
    out, s2, bn2 = _eval_half_tail(x, blk, g, d, bn1, s1)
    return out, SimpleNamespace(src=src, src_bn=src_bn, d=d, s1=s1, s2=s2, bn1=bn1, bn2=bn2, xf_shape=xf_shape)


def _eval_half_tail(x, blk, g, d, bn1, s1):
    """the rest of the half forward after the SE squeeze's first FC: gate, project conv, BN2 (+ skip).  Returns (out, s2, bn2)."""
    s2 = K.fc_fwd(s1, g.Wse, blk._se_expand.bias, 1)
    p = K.gemm_nt(K.se_scale_bn(d, bn1, s2, g.N, g.HWo).view(g.Mo, g.Ce), g.Wp)
    bn2 = K.EvalBN(blk._bn2, 0)
    return K.residual_bn(p.view(g.N, g.Ho, g.Wo, g.Co), bn2, None, 1.0, x if blk.spec.skip else None, g.N, g.HWo), s2, bn2


def mbconv_eval_half(x, blk, wt, lazy_bn=None, node_max_cin=0):
    """MBConvBlock.forward in eval mode, half storage (the fp16 InferenceRunner, unidefense_amd/infer.py): the forward of
    mbconv_fused with every BatchNorm in the eval form and no batch statistics (_half_forward).  No tape, nothing kept.
    x [N,H,W,Cin] fp16 (for block 0: the raw stem output, lazy_bn its eval BatchNorm + swish, applied on load);
    wt: the depthwise weight tap-major [k*k][C].  Activations are stored as fp16, computed in fp32 registers; the 1x1 convs
    are fp16 MFMA products with fp32 accumulation, selected per GEMM descriptor by the half operands (ud_gemm_desc.half_mask),
    the fp32 weights converted as the kernel loads them.
    node_max_cin: an expanding non-SF block with at most this many input channels takes the half-storage eval node instead
    (ud_mb_eval_dw_h: expand conv on fp16 MFMA + BN0 + swish + depthwise + SE squeeze in one pass; e is never written)."""
    sp = blk.spec
    g = block_geom(blk, x)
    assert x.dtype == torch.float16 and not (sp.skip and lazy_bn is not None)
    if (sp.expand != 1 and sp.sf_norm is None and g.Cin <= node_max_cin and K.mb_eval_dw_h_ok(g.Cin, g.Ce, g.k, g.stride)):
        # d raw (BN1 + swish applied on load by se_scale_bn); pool: the mean of swish(bn1(.)) of the stored values
        bn1 = K.EvalBN(blk._bn1, 1)
        d, pmean = K.mb_eval_dw_h(x, g.We, K.EvalBN(blk._bn0, 1), wt, bn1, g.k, g.stride, g.pt, g.pl, g.Ho, g.Wo, out_act=False)
        s1 = K.fc_fwd(pmean, g.Wsr, blk._se_reduce.bias, 0)
        return _eval_half_tail(x, blk, g, d, bn1, s1)[0]
    return _half_forward(x, blk, g, wt, lazy_bn)[0]


# measurement hook of the frozen half backward: a callable (block's parameter container, name, half tensor) called for every half
# gradient tensor the node stores (tests and DESIGN 3l record the largest scaled magnitude against fp16's 65504 with it); None: off
HALF_GRAD_PROBE = None


def mbconv_frozen_half(tape, x, blk, wt, lazy_in=None):
    """MBConvBlock.forward in eval mode, half storage, as ONE tape node whose backward is the FROZEN one (the fp16 InputGradRunner /
    AttackRunner, unidefense_amd/attack.py): data gradients only, through eval-form BatchNorms.

    Forward: _half_forward, the very function mbconv_eval_half runs (the outputs are bitwise the fp16 InferenceRunner's).  Kept for
    the backward: e (raw expand output), d (raw depthwise / SF output), s1, s2 — not the gated tensor, the spectra, the two SF
    branches or any activated tensor.
    Backward: _frozen_backward.
    x [N,H,W,Cin] fp16; for block 0: the raw half stem output, lazy_in = LazyInput(the stem's EvalBN, backward(dh))."""
    if tape.wgrad_on:
        raise RuntimeError("mbconv_frozen_half is the backward of a FROZEN model (no parameter requires a gradient): it forms no "
                           "weight gradient; a half-storage backward with trainable parameters is the training step's")
    assert x.dtype == torch.float16 and not (blk.spec.skip and lazy_in is not None)
    g = block_geom(blk, x)
    out, f = _half_forward(x, blk, g, wt, lazy_in.bn if lazy_in is not None else None)
    tape.record(lambda: _frozen_backward(tape, x, blk, g, wt, lazy_in, out, f))
    return out


def _frozen_backward(tape, x, blk, g, wt, lazy_in, out, f):
    """The frozen backward of mbconv_frozen_half; f: what _half_forward kept.  Half storage, fp32 registers; an eval BatchNorm's
    backward is the per-channel constant gamma invstd, folded into the kernel that makes the gradient — no sums, no apply pass, no
    fp64 accumulators but the SE gate's:
      dp = gamma2 invstd2 dout (ud_bn_eval_bwd, the thin tensor) -> dc = dp @ Wp (half GEMM) -> dgate = sum_hw dc swish(bn1(d))
      (ud_coldot_bn_eval) -> the SE FCs' data gradient (ud_se_bwd_a / _b without their weight-gradient workgroups) ->
      dd = (dc sigmoid(s2) + dpool / HW) swish'(bn1(d)) gamma1 invstd1 (ud_se_scale_bwd_bn_eval) -> SF: the adjoint transforms
      around the spectral data-gradient GEMM, the gate applied by ud_rfft2_ex (frequency) and the dgrad kernel (spatial) ->
      de = (gate dwconv^T(dd) + da_f) swish'(bn0(e)) gamma0 invstd0 (ud_dwtile_dgrad_eval) -> dx = de @ We (+ the skip gradient)."""
    dout = tape.pop_grad(out)
    if dout is None:
        return
    dout = _grad_like(dout, out)
    assert dout.dtype == torch.float16
    skip, d, N, HWo = blk.spec.skip, f.d, g.N, g.HWo
    # ---- BN2: the constant applied in a pass over the thin tensor; project conv's data gradient on the half GEMM
    probe = HALF_GRAD_PROBE
    dp = K.bn_eval_bwd(dout, None, f.bn2, 1, g.Mo)
    dc = K.gemm_nn(dp.view(g.Mo, g.Co), g.Wp).view(N, g.Ho, g.Wo, g.Ce)
    if probe is not None:
        for nm, t in (("dout", dout), ("dp", dp), ("dc", dc)):
            probe(blk, nm, t)
    # ---- SE gate, the two FCs (data gradient only), then gate + swish + BN1 in one pass over (dc, d)
    dgate = K.zeros64(N * g.Ce, x)
    K.coldot_bn_eval(dc, d, f.bn1, N, HWo, dgate)
    dpool = K.se_bwd(dgate, f.s2, f.s1, g.Wse, g.Wsr, None, 1.0 / HWo, need_w=False)[0]
    dd = K.se_scale_bwd_bn_eval(dc, d, f.bn1, f.s2, dpool, 1.0 / HWo, N, HWo)
    del dc
    if probe is not None:
        probe(blk, "dd", dd)
    # ---- SF: frequency branch sigmoid(a) dd through the adjoint transforms and the spectral data-gradient GEMM (stride 2:
    # through the 2 x 2 mean first); spatial branch (1 - sigmoid(a)) dd by the dgrad kernel's gate mode 2; the gate is frozen
    g_alpha, g_mode, da_f = None, 0, None
    if g.sf:
        dfr = dd if g.stride == 1 else K.sfmix_pool_bwd(dd)
        dyf, _ = K.rfft2_ex(dfr, g.s_i, 2.0, gate_alpha=g.alpha, gate_mode=1)
        dxf = K.gemm_nn(dyf.view(-1, 2 * g.Ce), g.Wf).view(f.xf_shape)
        da_f = K.irfft2(dxf, g.s_f, 0.5)
        if probe is not None:
            for nm, t in (("dyf", dyf), ("dxf", dxf), ("da_f", da_f)):
                probe(blk, nm, t)
        del dfr, dyf, dxf
        g_alpha, g_mode = g.alpha, 2
    # ---- depthwise data gradient through BN0 (block 0: the stem's BatchNorm) + swish in one tiled pass, then the expand conv
    if f.src_bn is not None:
        de = K.dwtile_dgrad_eval(dd, wt, g.k, g.pt, g.pl, f.src, f.src_bn, g_alpha, g_mode, da_f, g.stride)
        if probe is not None:
            probe(blk, "de", de)
        if lazy_in is not None:
            lazy_in.backward(de)
            return
        dx, = _expand_dgrad(tape, skip, dout, x, lambda acc: (K.gemm_nn(de.view(g.M, g.Ce), g.We, out=acc, accumulate=acc is not None),))
    else:
        add, skip_done = _skip_into_add(skip, da_f, dout)
        dx = K.dwtile_bwd_data(dd, wt, g.k, g.pt, g.pl, g.H, g.W, g_alpha, g_mode, add, stride=g.stride)
        if not skip_done:
            dx = K.axpby(dx, 1.0, dout, 1.0, out=dx)
    if probe is not None:
        probe(blk, "dx", dx)
    dx._ud_owned = True
    tape.add_grad(x, dx)


# ---- fp32, eval mode: the InferenceRunner's node (csrc/evalblk.hip) ----
def eval_block_ok(blk, max_cin):
    """does mbconv_eval take this block?  max_cin: the widest block input it pays at (UniDefenseModelEb4.EVAL_NODE_MAX_CIN)"""
    sp = blk.spec
    return (sp.expand != 1 and sp.sf_norm is None and sp.cin <= max_cin and K.mb_eval_dw_ok(sp.cin, sp.cexp, sp.k, sp.stride))


def mbconv_eval(x, blk, wt):
    """MBConvBlock.forward in eval mode on the eval-form BatchNorms (kernels.EvalBN): ud_mb_eval_dw makes d and the SE
    squeeze from the thin input (the expanded tensor is never written), then the SE gate, the project conv and BN2 +
    the residual — ud_pj_fwd_fused (gate and BN1 applied on load) + ud_residual_bn where the project pair is built for it,
    ud_se_scale_fwd + the GEMM + ud_residual_bn elsewhere.  wt: the depthwise weight tap-major [k*k][C]."""
    g = block_geom(blk, x)
    bn1 = K.EvalBN(blk._bn1, 1)
    pj = K.project_fwd_fused_ok(x, g.Wp, g.HWo)
    d, pool = K.mb_eval_dw(x, g.We, K.EvalBN(blk._bn0, 1), wt, bn1, g.k, g.stride, g.pt, g.pl, g.Ho, g.Wo, out_act=not pj)
    s1 = K.fc_fwd(pool, g.Wsr, blk._se_reduce.bias, 0)
    s2 = K.fc_fwd(s1, g.Wse, blk._se_expand.bias, 1)
    if pj:
        p, _ = K.project_fwd_fused(d, bn1, s2, g.Wp, g.N, g.HWo)
    else:
        p = K.gemm_nt(K.se_scale_fwd(d, s2).view(g.Mo, g.Ce), g.Wp)
    return K.residual_bn(p.view(g.N, g.Ho, g.Wo, g.Co), K.EvalBN(blk._bn2, 0), None, 1.0, x if blk.spec.skip else None, g.N, g.HWo)

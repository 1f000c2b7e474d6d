"""Reverse-mode tape + differentiable operators of the UniDefense hot path, built on the HIP kernels.

The whole network is ONE node in torch's autograd graph (``model.unidefense._NetFunction``): its forward
runs these operators while recording backward closures on a ``Tape``; its backward replays the tape in
reverse.  Compared with ~2000 ``torch.autograd.Function`` nodes per step this keeps the host path short
and gives the executor full control over buffer lifetime and gradient accumulation.

Every operator takes pixel-major fp32 CUDA tensors (see kernels.py) and cites the reference op it replaces.
"""
import math
from typing import Optional

import torch

from . import kernels as K
from .config import cfg


class Tape:
    """Records backward closures; gradients are keyed by tensor identity."""

    def __init__(self):
        self.nodes = []
        self.grads = {}
        self.param_grads = {}
        self._keep = []          # keep keyed tensors alive so ids stay unique
        self.watch = None        # debug: {id(tensor): name} -> gradients captured into self.captured
        self.captured = {}
        self.kinks = None        # parity tests: {site: ReLU output} (site = id(norm weight) or an explicit name)
        self.gate_cond = {}      # parity tests (watch set): {id(sf_coef): sigmoid'(a) * sum |dy| |freq - spat|}, the
        #                          conditioning of that scalar gradient (a global sum that cancels heavily)
        # data parallel (engine/parallel.py): param_ready(id(p), g) is called the moment p's gradient is final, i.e.
        # after its param_uses[id(p)]-th contribution (counts learned from the first backward: param_seen)
        self.param_ready = None
        self.param_uses = None
        self.param_seen = {}
        self._deferred = set()   # id(param) whose stored gradient still waits for the flush's launch (kernels.flush_wgrad_folds)
        self.weight_snapshot = None      # kernels.weight_batch_snapshot() of the forward (checked before the replay)
        # gradient with respect to the input image: `input` is the tracked x planes [N,3,H,W] (model(x) with x.requires_grad
        # and no perturbation), its gradient is left in `input_grad` by backward().  wgrad_on = False: no parameter takes a
        # gradient (a frozen eval-mode model), so the operators launch no weight-gradient work
        self.input = None
        self.input_grad = None
        self.wgrad_on = True

    def tracks(self, t) -> bool:
        """is t the tracked input image?"""
        return self.input is not None and t is self.input

    # -- recording -------------------------------------------------------------------------
    def record(self, fn):
        self.nodes.append(fn)

    def add_grad(self, t: torch.Tensor, g: torch.Tensor):
        """Accumulate g into the gradient slot of activation t (functional: never mutates g)."""
        k = id(t)
        cur = self.grads.get(k)
        if cur is None:
            self.grads[k] = g
            self._keep.append(t)
        else:
            s = K.axpby(cur, 1.0, g.reshape(cur.shape), 1.0)
            s._ud_owned = True          # a fresh tensor only the tape holds: its consumer may accumulate onto it in place
            self.grads[k] = s

    def pop_grad(self, t: torch.Tensor) -> Optional[torch.Tensor]:
        g = self.grads.pop(id(t), None)
        if self.watch is not None and id(t) in self.watch:
            self.captured[self.watch[id(t)]] = g
        return g

    def add_param_grad(self, p, g: torch.Tensor):
        if not self.wgrad_on:
            return
        cur = self.param_grads.get(p)
        deferred = getattr(g, "_ud_deferred", False)
        if (deferred or id(p) in self._deferred) and (cur is not None or self.param_ready is not None):
            K.flush_wgrad_folds()          # read right away (summed with an earlier use / handed to the gradient reducer): fold now
            self._deferred.clear()         # (the flush folds every pending gradient, the stored ones included)
            deferred = False
        g = g.reshape(p.shape)
        g = g if cur is None else K.axpby(cur, 1.0, g, 1.0)
        self.param_grads[p] = g
        if deferred:
            self._deferred.add(id(p))      # stored unfolded: a later contribution to p must flush before it reads `cur`
        n = self.param_seen[id(p)] = self.param_seen.get(id(p), 0) + 1
        if self.param_ready is not None and n == self.param_uses.get(id(p)):
            self.param_ready(id(p), g)

    # -- weight gradients -------------------------------------------------------------------
    def wgrad(self, p, fn, *inputs):
        """Run `fn()` (the weight-gradient kernels of parameter p) and record the result.  One queue: a second stream for
        these launches was measured slower in rounds 1, 2 and 4 (46.3 vs 43.6, 36.15 vs 34.70, 29.1 vs 27.2 ms per step: the
        GEMMs own the CU's registers and LDS, nothing co-schedules) and is gone — with it the ordering hazard of operand
        planes made lazily on whichever stream touched them first.  A second stream for the reconstruction decoder (round 6)
        was measured slower as well (24.07 vs 24.44 ms, profiles/r06/side_branch_ab.txt) and is gone too."""
        self.add_param_grad(p, fn())

    # -- replay ----------------------------------------------------------------------------
    def backward(self):
        if self.weight_snapshot is not None:
            K.weight_batch_check(self.weight_snapshot)
        K.begin_wgrad_folds()          # the launches that only finish a parameter's gradient: one at the end instead of one each
        try:
            for fn in reversed(self.nodes):
                fn()
        finally:
            K.flush_wgrad_folds(end=True)
        if self.input is not None:
            self.input_grad = self.grads.get(id(self.input))
        self.nodes = []
        self.grads = {}
        self._keep = []


def _needs(tape):
    return tape is not None


def _tracks(tape, t):
    return tape is not None and tape.tracks(t)


def _wgrad(tape):
    return tape.wgrad_on


# ---------------------------------------------------------------------------------------------
# GEMM-shaped ops
# ---------------------------------------------------------------------------------------------
_CONST_AFFINE = {}


def _const_affine(Cc, like):
    """gamma = 1, beta = 0 for a norm built with affine=False (model/unidefense.py:38,61,116): constants, no gradients"""
    key = (Cc, like.device)
    v = _CONST_AFFINE.get(key)
    if v is None:
        v = _CONST_AFFINE[key] = (torch.ones(Cc, device=like.device), torch.zeros(Cc, device=like.device))
    return v


def bias_add(tape, y, b):
    """+ the bias of a conv built with bias=True (model/unidefense.py:36,60-100; modules.py:82,87,111,116) on channel-last y.
    No shipped config of the reference uses the variant, so these are plain device ops: a broadcast add, and a column sum for
    the bias gradient."""
    if b is None:
        return y
    out = y + b
    if _needs(tape):
        def bwd():
            d = tape.pop_grad(out)
            if d is None:
                return
            tape.add_grad(y, d)
            if _wgrad(tape):
                tape.add_param_grad(b, d.reshape(-1, d.shape[-1]).sum(0))
        tape.record(bwd)
    return out


def conv1x1(tape, x, w, need_dx=True):
    """F.conv2d with a [Cout,Cin,1,1] weight on pixel-major x[...,Cin] (model/efficientnet/model.py:108,125;
    exp.py:57; model/modules.py:82).  Backward = convolution_backward: dX = dY W, dW = dY^T X."""
    Co, Ci = w.shape[0], w.shape[1]
    w2 = w.view(Co, Ci)
    x2 = x.view(-1, Ci)
    if not _needs(tape):
        return K.gemm_nt(x2, w2).view(*x.shape[:-1], Co)
    # the three products share their operands: large shapes split them once into fp16 x 2 planes (kernels.spectral_*)
    y2, ctx = K.spectral_fwd(x2, w2)
    y = y2.view(*x.shape[:-1], Co)

    def bwd():
        dy = tape.pop_grad(y)
        if dy is None:
            return
        dy2 = dy.reshape(-1, Co)
        if not _wgrad(tape):
            if need_dx:
                tape.add_grad(x, K.spectral_dgrad(ctx, dy2).view(x.shape))
        elif need_dx:
            dx, dw = K.spectral_bwd(ctx, dy2)          # (one launch on the planes GEMM where both plans allow)
            tape.add_param_grad(w, dw)
            tape.add_grad(x, dx.view(x.shape))
        else:
            tape.wgrad(w, lambda: K.spectral_wgrad(ctx, dy2), dy2)
    tape.record(bwd)
    return y


def _conv_im2col(tape, x, w, wmat, g, need_dx):
    """A k x k conv as a 1x1 conv over its im2col matrix on the planes GEMM (kernels.im2col_planes): forward, weight gradient and
    data gradient (a GEMM + col2im) share the three operands' planes like tape.conv1x1's."""
    Co, Ci, KH, KW = w.shape
    xcol = K.im2col_planes(x, g)
    y2, ctx = K.spectral_fwd(xcol, wmat, force=True)
    y = y2.view(g.N, g.Hout, g.Wout, Co)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            dy2 = dy.reshape(-1, Co)
            if not dy2.is_contiguous():
                dy2 = dy2.contiguous()
            if not _wgrad(tape):
                dcol, dw = (K.spectral_dgrad(ctx, dy2) if need_dx else None), None
            elif need_dx:
                dcol, dw = K.spectral_bwd(ctx, dy2)                    # dw [Co, KH*KW*Ci]
            else:
                dcol, dw = None, K.spectral_wgrad(ctx, dy2)
            if dw is not None:
                tape.add_param_grad(w, dw.view(Co, KH, KW, Ci).permute(0, 3, 1, 2).contiguous())
            if need_dx:
                tape.add_grad(x, K.col2im(dcol, g))
        tape.record(bwd)
    return y


def _stem_dgrad(tape, dy, w, g, x_planes):
    """the stem conv's data gradient (kernels.stem_dgrad) added onto the tracked input image's gradient: the stem's backward
    runs last, so the attention's and the reconstruction losses' parts are already there and one pass completes dx"""
    cur = tape.grads.pop(id(x_planes), None)
    if cur is not None and not (cur.is_contiguous() and cur.dtype == torch.float32 and cur.shape == x_planes.shape):
        tape.grads[id(x_planes)], cur = cur, None
    tape.add_grad(x_planes, K.stem_dgrad(dy, w, g, out=cur))


def conv_dense(tape, x, w, stride, pad_t, pad_l, Hout, Wout, need_dx=True, x_planes=None):
    """Dense k x k F.conv2d (weight [Cout,Cin,kh,kw]) as an implicit GEMM (model/unidefense.py:60,67,...;
    model/modules.py:111; stem conv model/efficientnet/model.py:185 with its static asymmetric pad).
    x_planes: the stem's input image as planes — when it is the tape's tracked input, its data gradient is formed
    (kernels.stem_dgrad) instead of the need_dx gather."""
    N, Hin, Win, Ci = x.shape
    Co, _, KH, KW = w.shape
    g = K.conv_geom(N, Hin, Win, Ci, Hout, Wout, KH, KW, stride, pad_t, pad_l, 0)
    wmat = K.weight_layout(w, 0)
    stem_dx = _tracks(tape, x_planes)
    if K.conv_im2col_ok(g, Co, x):
        assert not stem_dx
        return _conv_im2col(tape, x, w, wmat, g, need_dx)
    y = K.conv_gather_nt(x, wmat, g)
    if _needs(tape):
        # dX = conv(dY, W flipped & transposed), pad = k-1-pad: its weight matrix comes out of the forward's one-launch batch
        wd = K.weight_layout(w, 1) if need_dx else None

        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            if need_dx:
                assert stride == 1 and Hout == Hin and Wout == Win, "data gradient implemented for stride 1 'same'"
                gd = K.conv_geom(N, Hout, Wout, Co, Hin, Win, KH, KW, 1, KH - 1 - pad_t, KW - 1 - pad_l, 0)
                tape.add_grad(x, K.conv_gather_nt(dy, wd, gd))
            elif stem_dx:
                _stem_dgrad(tape, dy, w, g, x_planes)
            if _wgrad(tape):
                tape.add_param_grad(w, K.conv_wgrad_param(dy.view(-1, Co), x, g))        # [Co, Ci, KH, KW]
        tape.record(bwd)
    return y


def conv_transpose_s2(tape, x, w):
    """nn.ConvTranspose2d(k=3, stride=2, padding=1, output_padding=1), weight [Cin,Cout,3,3]
    (model/unidefense.py:63-64,77-78,91-92)."""
    N, H, W, Ci = x.shape
    _, Co, KH, KW = w.shape
    Ho, Wo = 2 * H, 2 * W
    g = K.conv_geom(N, H, W, Ci, Ho, Wo, KH, KW, 2, 1, 1, 1)
    wmat = K.weight_layout(w, 2)
    y = K.conv_gather_nt(x, wmat, g)
    if _needs(tape):
        wd = K.weight_layout(w, 0)

        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            # dX[n,ih,iw,ci] = sum dY[n,2ih-1+kh,2iw-1+kw,co] W[ci,co,kh,kw]: a stride-2 conv over dY
            gd = K.conv_geom(N, Ho, Wo, Co, H, W, KH, KW, 2, 1, 1, 0)
            tape.add_grad(x, K.conv_gather_nt(dy, wd, gd))
            if _wgrad(tape):
                tape.add_param_grad(w, K.conv_wgrad_param(x.view(-1, Ci), dy, gd))       # [Ci, Co, KH, KW]
        tape.record(bwd)
    return y


def linear(tape, x, w, b):
    """nn.Linear (model/modules.py:27,31)."""
    y = K.fc_fwd(x, w, b, 0)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            wg = _wgrad(tape)
            dx, dW, db = K.fc_bwd(dy, w, x, 0, need_dw=wg)
            tape.add_grad(x, dx)
            if wg:
                tape.add_param_grad(w, dW)
                tape.add_param_grad(b, db)
        tape.record(bwd)
    return y


# ---------------------------------------------------------------------------------------------
# depthwise conv, FFT, SFConv
# ---------------------------------------------------------------------------------------------
DW_WT = {}            # {id(w): (w, w._version, tap-major wt)} for the forward in flight (kernels.dw_weights_tapmajor)


def conv_out_hw(H, W, k, stride, pad):
    """(Ho, Wo) of a k x k conv over an H x W map zero-padded by pad = (left, right, top, bottom) as in nn.ZeroPad2d"""
    pl, pr, pt, pb = pad
    return (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1


def dwconv(tape, x, w, stride, pad):
    """Depthwise Conv2dStaticSamePadding (model/efficientnet/utils.py:277-280; exp.py:49-51).
    pad = (left, right, top, bottom) as in nn.ZeroPad2d."""
    N, H, W, Cc = x.shape
    k = w.shape[-1]
    pl, pt = pad[0], pad[2]
    Ho, Wo = conv_out_hw(H, W, k, stride, pad)
    ent = DW_WT.get(id(w))                      # tap-major copy made for all layers at once (model._run), if any
    if ent is not None and ent[0] is w and ent[1] == w._version:
        wt = ent[2]
    else:
        wt = w.view(Cc, k * k).t().contiguous()
    y = K.dwconv_fwd(x, wt, k, stride, pt, pl, Ho, Wo)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            # x usually has a second consumer whose gradient is already there (SFConv's frequency branch, exp.py:55;
            # the SE pool): the data-gradient kernel adds it in its store instead of a separate axpby pass
            cur = tape.grads.pop(id(x), None)
            if cur is not None and not (cur.is_contiguous() and cur.shape == x.shape and cur.dtype == torch.float32):
                tape.grads[id(x)], cur = cur, None
            tape.add_grad(x, K.dwconv_bwd_data(dy, wt, k, stride, pt, pl, H, W, add=cur))
            if _wgrad(tape):
                tape.add_param_grad(w, K.dwconv_bwd_weight(x, dy, k, stride, pt, pl))     # already [C, k*k]
        tape.record(bwd)
    return y


def _fft_scales(S, norm):
    if norm == "ortho":
        return 1.0 / S, 1.0 / S
    if norm is None or norm == "backward":
        return 1.0, 1.0 / (S * S)
    raise ValueError(f"unsupported fft norm {norm!r}")


def rfft2_cat(tape, x, norm):
    """torch.fft.rfft2 + cat([re, im], channel)  (exp.py:55-56; unidefense.py:130-136)."""
    S = x.shape[1]
    sf, _ = _fft_scales(S, norm)
    y = K.rfft2(x, sf, 1.0)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.irfft2(dy, sf, 0.5))
        tape.record(bwd)
    return y


def irfft2_split(tape, y, norm):
    """tensor_split + torch.complex + torch.fft.irfft2(s=(S,S))  (exp.py:59-60; unidefense.py:142-145)."""
    S = y.shape[1]
    _, si = _fft_scales(S, norm)
    x = K.irfft2(y, si, 1.0)
    if _needs(tape):
        def bwd():
            dx = tape.pop_grad(x)
            if dx is None:
                return
            tape.add_grad(y, K.rfft2(dx, si, 2.0))
        tape.record(bwd)
    return x


def adaptive_avgpool(tape, x, Ho, Wo):
    """F.adaptive_avg_pool2d to a size that does not divide the input (exp.py:61-62 on the 95 x 95 map of the 380 x 380 trunk's
    stride-2 SF block: 95 -> 48, windows of 2 and 3 that overlap): csrc/pool.hip's adaptive_avgpool kernels (rounds 3-4: ATen's);
    the 2 x 2 case of the 256 x 256 trunk is fused into ud_sfmix."""
    H, W = x.shape[1], x.shape[2]
    y = K.adaptive_avgpool_fwd(x, Ho, Wo)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.adaptive_avgpool_bwd(dy.contiguous(), H, W))
        tape.record(bwd)
    return y


def sfmix(tape, spat, freq, alpha):
    """(1 - sigmoid(a)) * spat + sigmoid(a) * [avg-pooled] freq  (exp.py:61-65)."""
    if freq.shape[1] != spat.shape[1] and (freq.shape[1] != 2 * spat.shape[1] or freq.shape[2] != 2 * spat.shape[2]):
        freq = adaptive_avgpool(tape, freq, spat.shape[1], spat.shape[2])
    pool = freq.shape[1] != spat.shape[1]
    if pool:
        assert freq.shape[1] == 2 * spat.shape[1] and freq.shape[2] == 2 * spat.shape[2]
    y = K.sfmix_fwd(spat, freq, alpha, pool)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            ds, df, da = K.sfmix_bwd(spat, freq, alpha, dy, pool)
            if tape.watch is not None:
                with torch.no_grad():
                    f = freq.float()
                    if pool:
                        n_, h_, w_, c_ = spat.shape
                        f = f.view(n_, h_, 2, w_, 2, c_).mean((2, 4))
                    sg = torch.sigmoid(alpha.double())
                    tape.gate_cond[id(alpha)] = float(sg * (1 - sg) * (dy.double().abs() * (f.double() - spat.double()).abs()).sum())
            tape.add_grad(spat, ds)
            tape.add_grad(freq, df)
            tape.add_param_grad(alpha, da)
        tape.record(bwd)
    return y


def sfconv_dw(tape, x, w, w_freq, alpha, stride, pad, norm):
    """SFConv2dStaticSamePadding.forward (model/efficientnet/exp.py:46-65)."""
    spat = dwconv(tape, x, w, stride, pad)
    xf = rfft2_cat(tape, x, norm)
    yf = conv1x1(tape, xf, w_freq)
    fr = irfft2_split(tape, yf, norm)
    return sfmix(tape, spat, fr, alpha)


# ---------------------------------------------------------------------------------------------
# normalisation + activation
# ---------------------------------------------------------------------------------------------
# cfg.force_collectives: issue the data-parallel collectives (SyncBN statistics, gradient all-reduce) even in a
# world of one process, so that a single-GPU box exercises the RCCL calls and their hipGraph capture


def sync_batch_stats(mean_l, var_l, eps, group):
    """Combine per-rank (mean, biased var) over equally sized shards into the global statistics:
    mean = avg_r mean_r ;  var = avg_r (var_r + (mean_r - mean)^2).  One all_gather of 2C floats
    (torch.nn.SyncBatchNorm's forward exchange; RCCL on GPU, gloo in the CPU tests)."""
    import torch.distributed as dist
    ws = dist.get_world_size(group)
    mine = torch.cat([mean_l.reshape(-1), var_l.reshape(-1)])
    flat = torch.empty(ws * mine.numel(), dtype=mine.dtype, device=mine.device)
    dist.all_gather_into_tensor(flat, mine, group=group)
    allst = flat.view(ws, mine.numel())
    Cc = mean_l.numel()
    means, vars_ = allst[:, :Cc], allst[:, Cc:]
    mean = means.mean(0)
    var = (vars_ + (means - mean) ** 2).mean(0)
    return mean.view(1, Cc).contiguous(), var.view(1, Cc), torch.rsqrt(var + eps).view(1, Cc).contiguous()


def batchnorm_act(tape, x, weight, bias, running_mean, running_var, eps, momentum, training, act, sync_group=None,
                  exchange=None):
    """nn.BatchNorm2d/1d (+ MemoryEfficientSwish when act=1) on pixel-major x[..., C]
    (model/efficientnet/model.py:109-114,126; utils.py:66-82).  With sync_group: SyncBatchNorm semantics
    (statistics over the batches of all ranks; engine/forgery_engine.py:142, ocim_engine.py:130-133) — the fp64 sums
    (sum x, sum x^2; sum dz, sum dz xhat in the backward) travel through `exchange` (engine.parallel.BnExchange: one
    small kernel over peer-mapped mailboxes) when given, else through one dist.all_reduce each way."""
    Cc = x.shape[-1]
    x2 = x.view(-1, Cc)
    R = x2.shape[0]
    affine = weight is not None
    if not affine:
        weight, bias = _const_affine(Cc, x)
    synced = False
    if training and sync_group is not None:
        import torch.distributed as dist
        synced = dist.get_world_size(sync_group) > 1 or cfg.force_collectives
    if synced and Cc % 4 == 0:
        return _syncbn_act(tape, x, x2, R, Cc, weight, bias, running_mean, running_var, eps, momentum, act, sync_group,
                           exchange, affine)
    if synced:
        # channel counts the column kernels do not take (never in the reference's models): (mean, var) all_gather form
        world = dist.get_world_size(sync_group)
        mv = K.norm_stats_local(x2, 1, R, eps)                               # [2, 1, C]
        gathered = torch.empty((world, 2, Cc), dtype=mv.dtype, device=mv.device)
        dist.all_gather_into_tensor(gathered.view(-1), mv.view(-1), group=sync_group)
        mean, invstd = K.syncbn_combine(gathered, world, Cc, R, eps, momentum, running_mean, running_var)
    elif training:
        world = 1
        mean, invstd = K.norm_stats(x2, 1, R, eps, momentum, running_mean, running_var)
    else:
        world = 1
        mean = running_mean.view(1, Cc)
        invstd = torch.rsqrt(running_var + eps).view(1, Cc)
    y = K.norm_apply(x2, 1, R, mean, invstd, weight, bias, act).view(x.shape)
    if act == 2 and tape is not None and tape.kinks is not None:
        tape.kinks[id(weight)] = y
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            if not training:
                # eval mode: the statistics are constants (running_mean / running_var), so dx = gamma * invstd * dz with
                # dz = dy * act'(z) — the training formula with its two mean terms dropped (sums passed as zeros) — and
                # dgamma = sum dz * xhat, dbeta = sum dz as in training
                if _wgrad(tape):
                    s, dg, db = K.norm_bwd_sums(x2, dy.view(-1, Cc), 1, R, mean, invstd, weight, bias, act)
                    zs = torch.zeros_like(s)
                else:                      # a frozen model: no dgamma / dbeta, and dx needs no sums
                    zs, dg = K.zeros((2, 1, Cc), x2), None     # (carved from the zero pool: no launch)
                dx = K.norm_bwd_apply(x2, dy.view(-1, Cc), 1, R, mean, invstd, weight, bias, zs, 0.0, act)
            elif synced:
                import torch.distributed as dist
                s, dg, db = K.norm_bwd_sums(x2, dy.view(-1, Cc), 1, R, mean, invstd, weight, bias, act)
                dist.all_reduce(s, group=sync_group)           # sum_dz, sum_dz_xhat over all ranks
                dx = K.norm_bwd_apply(x2, dy.view(-1, Cc), 1, R, mean, invstd, weight, bias, s,
                                      1.0 / float(R * world), act)
            else:
                dx, dg, db = K.norm_bwd(x2, dy.view(-1, Cc), 1, R, mean, invstd, weight, bias, act)
            tape.add_grad(x, dx.view(x.shape))
            if affine and dg is not None:
                tape.add_param_grad(weight, dg)
                if bias.requires_grad:
                    tape.add_param_grad(bias, db)
        tape.record(bwd)
    return y


def _syncbn_act(tape, x, x2, R, Cc, weight, bias, running_mean, running_var, eps, momentum, act, sync_group, exchange,
                affine=True):
    """SyncBatchNorm of the operator path (attention, head, the ResNet models) on the deferred-BatchNorm kernels of the
    fused path: fp64 column sums -> summed over the ranks in place (DataParallelCtx.reduce: BnExchange's mailbox kernel or
    one all_reduce) -> one apply pass that also moves the running statistics; the backward sums the same way.  Every rank
    must hold the same number of rows (the count is R * world; engine/data.py pads the shards like DistributedSampler)."""
    dp = DataParallelCtx(sync_group, exchange)
    acc = K.zeros64(2 * Cc, x)
    K.colstats(x2, acc)
    dp.reduce(acc)
    bn = K.DeferredBN(acc, Cc, R * dp.world, weight, bias, eps, act, momentum, running_mean, running_var)
    y = K.bn_apply(x2, bn, 1, R, update=True).view(x.shape)
    if act == 2 and tape is not None and tape.kinks is not None:
        tape.kinks[id(weight)] = y
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            dy2 = dy.reshape(-1, Cc)
            if not dy2.is_contiguous():
                dy2 = dy2.contiguous()
            sb = K.zeros64(2 * Cc, x)
            K.normbwd_sums(x2, dy2, None, 1.0, bn, False, 1, R, sb)
            loc = dp.reduce(sb, keep_local=True)
            dx, dg, db = K.normbwd_apply(x2, dy2, None, 1.0, bn, False, 1, R, sb, loc, want_dbeta=bias.requires_grad)
            tape.add_grad(x, dx.view(x.shape))
            if affine:
                tape.add_param_grad(weight, dg)
                if bias.requires_grad:
                    tape.add_param_grad(bias, db)
        tape.record(bwd)
    return y


def instancenorm_act(tape, x, weight, bias, eps, act):
    """nn.InstanceNorm2d(affine=affine) (+swish) on x[N,H,W,C]  (model/unidefense.py:61-70); weight = bias = None: affine=False."""
    N, H, W, Cc = x.shape
    x2 = x.view(-1, Cc)
    affine = weight is not None
    if not affine:
        weight, bias = _const_affine(Cc, x)
    mean, invstd = K.norm_stats(x2, N, H * W, eps)
    y = K.norm_apply(x2, N, H * W, mean, invstd, weight, bias, act).view(x.shape)
    if act == 2 and tape is not None and tape.kinks is not None:
        tape.kinks[id(weight)] = y
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            dx, dg, db = K.norm_bwd(x2, dy.view(-1, Cc), N, H * W, mean, invstd, weight, bias, act)
            tape.add_grad(x, dx.view(x.shape))
            if affine:
                tape.add_param_grad(weight, dg)
                tape.add_param_grad(bias, db)
        tape.record(bwd)
    return y


# ---------------------------------------------------------------------------------------------
# pooling, SE, residual, dropout
# ---------------------------------------------------------------------------------------------
def mean_hw(tape, x):
    """x.mean([-2,-1]) / adaptive_avg_pool2d(x, 1) -> [N, C]  (unidefense.py:226,232-236)."""
    N, H, W, Cc = x.shape
    y = K.group_colsum(x.view(-1, Cc), N, H * W, 1.0 / (H * W))
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.bcast_rows(dy, H * W, 1.0 / (H * W)).view(x.shape))
        tape.record(bwd)
    return y


def squeeze_excite(tape, x, w_r, b_r, w_e, b_e):
    """model/efficientnet/model.py:117-122."""
    N, H, W, Cc = x.shape
    Cs = w_r.shape[0]
    wr2, we2 = w_r.view(Cs, Cc), w_e.view(Cc, Cs)
    pool = K.group_colsum(x.view(-1, Cc), N, H * W, 1.0 / (H * W))
    s1 = K.fc_fwd(pool, wr2, b_r, 0)
    s2 = K.fc_fwd(s1, we2, b_e, 1)          # swish on the input side
    y = K.se_scale_fwd(x, s2)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            ds2 = K.group_coldot(dy.view(-1, Cc), x.view(-1, Cc), N, H * W)
            K.sigmoid_grad_mul_(s2, ds2)
            wg = _wgrad(tape)
            ds1, dWe, dbe = K.fc_bwd(ds2, we2, s1, 1, need_dw=wg)
            dpool, dWr, dbr = K.fc_bwd(ds1, wr2, pool, 0, need_dw=wg)
            tape.add_grad(x, K.se_scale_bwd(dy, s2, dpool))
            if not wg:
                return
            tape.add_param_grad(w_e, dWe)
            tape.add_param_grad(b_e, dbe)
            tape.add_param_grad(w_r, dWr)
            tape.add_param_grad(b_r, dbr)
        tape.record(bwd)
    return y


def residual(tape, x, skip, keep=None, keep_prob=1.0):
    """drop_connect + skip: x / keep_prob * keep[n] + skip  (model.py:130-134; utils.py:131-156)."""
    inv = 1.0 / keep_prob
    y = K.residual(x, skip, keep, inv)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(skip, dy)
            tape.add_grad(x, dy if keep is None else K.residual(dy, None, keep, inv))
        tape.record(bwd)
    return y


def add(tape, a, b):
    y = K.axpby(a, 1.0, b, 1.0)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(a, dy)
            tape.add_grad(b, dy)
        tape.record(bwd)
    return y


def dropout_mask(tape, x, keep, p):
    """F.dropout with an explicit keep-mask: x * keep / (1 - p)."""
    sc = 1.0 / (1.0 - p)
    y = K.mask_scale(x, keep, sc)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.mask_scale(dy, keep, sc))
        tape.record(bwd)
    return y


def gate_mix(tape, p, q, alpha):
    """(1 - sigmoid(a)) p + sigmoid(a) q   (fuse_coef, model/unidefense.py:153-154)."""
    y = K.gate_mix_fwd(p, q, alpha)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            dp, dq, da = K.gate_mix_bwd(p, q, alpha, dy)
            if tape.watch is not None:
                with torch.no_grad():
                    sg = torch.sigmoid(alpha.double())
                    tape.gate_cond[id(alpha)] = float(sg * (1 - sg) * (dy.double().abs() * (q.double() - p.double()).abs()).sum())
            tape.add_grad(p, dp)
            tape.add_grad(q, dq)
            tape.add_param_grad(alpha, da)
        tape.record(bwd)
    return y


# ---------------------------------------------------------------------------------------------
# image-domain tail
# ---------------------------------------------------------------------------------------------
def tanh_to_planes(tape, x):
    """nn.Tanh on [N,H,W,3] and move to planes [N,3,H,W]  (model/unidefense.py:101)."""
    y = K.pix_to_planes(x, tanh=True)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.planes_to_pix(dy, tanh_out=y))
        tape.record(bwd)
    return y


def bilinear(tape, x, Ho, Wo):
    """F.interpolate(mode='bilinear', align_corners=True) on planes (model/unidefense.py:16,244)."""
    Hi, Wi = x.shape[-2:]
    y = K.bilinear_fwd(x, Ho, Wo)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.bilinear_bwd(dy, Hi, Wi))
        tape.record(bwd)
    return y


def planes_to_pix(tape, x):
    """[N,C,H,W] planes -> pixel-major [N,H,W,C] (the attention's resized input image, model/unidefense.py:130-131)."""
    y = K.planes_to_pix(x)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is not None:
                tape.add_grad(x, K.pix_to_planes(dy.contiguous()))
        tape.record(bwd)
    return y


def absdiff(tape, a, b):
    """|a - b| with a gradient to b only (a carries none): -sign(a - b) g, sign(0) = 0 as in torch.abs."""
    y = K.absdiff(a, b)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is not None:
                tape.add_grad(b, K.absdiff_bwd(a, b, dy.contiguous()))
        tape.record(bwd)
    return y


def attention_diffs(tape, pred_planes, x, h, w, norm):
    """The dynamic filters' difference inputs (model/unidefense.py:130-150; :326-361, :521-554 for the ResNet models):
    pred and x bilinearly resized to the h x w attention map, freq_diff = |rfft2(pred) - rfft2(x)| [N,h,w/2+1,6] and
    spat_diff = |pred - x| [N,h,w,3].  pred (the reconstruction) is read detached, as in the reference.  When x is the tape's
    tracked input the x side is recorded (bilinear, layout, rfft2, |.| nodes) and the third value is True: the dynamic filters
    then hand back d(diff).  Otherwise the same kernels run untaped."""
    pred = K.planes_to_pix(K.bilinear_fwd(pred_planes, h, w))       # [N,h,w,3]
    sf, _ = _fft_scales(h, norm)
    if not _tracks(tape, x):
        xs = K.planes_to_pix(K.bilinear_fwd(x, h, w))
        return K.absdiff(K.rfft2(pred, sf), K.rfft2(xs, sf)), K.absdiff(pred, xs), False
    xs = planes_to_pix(tape, bilinear(tape, x, h, w))
    freq_diff = absdiff(tape, K.rfft2(pred, sf), rfft2_cat(tape, xs, norm))
    return freq_diff, absdiff(tape, pred, xs), True


def rec_losses(tape, rec, x, norm):
    """spatial = mean|rec - x| ; freq = mean(|Re D| + |Im D|), D = rfft2(rec) - rfft2(x) = rfft2(rec - x)
    (model/unidefense.py:245-253), per sample.  rec, x: planes [N,3,S,S].
    `rec` itself is also a model output, so its external gradient is added in the same backward.  x takes the negative
    of the losses' gradient to rec when it is the tape's tracked input."""
    N, Cc, S, _ = rec.shape
    assert norm == "ortho", "frequency reconstruction loss implemented for freq_norm='ortho'"
    cnt_s = Cc * S * S
    Wh = S // 2 + 1
    cnt_f = Cc * S * Wh
    spatial = K.l1_fwd(rec, x, 1.0 / cnt_s)
    d = K.axpby(rec, 1.0, x, -1.0)
    Y = K.dft_rfft2_planes(d.view(N * Cc, S, S))            # zero padding columns contribute |0| = 0
    freq = K.l1_fwd(Y.view(N, -1), None, 1.0 / cnt_f)
    if _needs(tape):
        def bwd():
            gs = tape.pop_grad(spatial)
            gf = tape.pop_grad(freq)
            grec = tape.pop_grad(rec)
            if gs is None and gf is None and grec is None:
                return
            total = None
            if gf is not None:
                dY = K.l1_bwd(Y.view(N, -1), None, gf, 1.0 / cnt_f).view(Y.shape)
                total = K.dft_rfft2_planes_adjoint(dY, S).view(rec.shape)
            if gs is not None:
                total = K.l1_bwd(rec, x, gs, 1.0 / cnt_s, out=total)
            if total is not None and _tracks(tape, x):
                tape.add_grad(x, K.axpby(total, -1.0))        # d/dx of |rec - x| and of rfft2(rec - x): the negative
            if grec is not None:
                total = grec if total is None else K.axpby(total, 1.0, grec, 1.0)
            tape.grads[id(rec)] = total      # hand the summed gradient to rec's producer
            tape._keep.append(rec)
        tape.record(bwd)
    return spatial, freq


def dynamic_filter(tape, x, proj, diff, w2, b2=None, diff_grad=False):
    """mask = sigmoid(conv1x1([mean_c proj, max_c proj, diff]) (+ b2)), out = mask * x
    (model/modules.py:94-104, 123-133).  x, proj: [N,h,w,*]; diff: [N,h,w,D]; w2: [1,2+D,1,1]; b2: [1] — the bias of
    the bias=True variant rides as the weight of one more, constant-1 difference channel (the kernels take any D).
    diff_grad: diff depends on the tracked input image and takes d(diff) = dlogit (x) w2[2:2+D]; otherwise no gradient."""
    Cx, Cp, D = x.shape[-1], proj.shape[-1], diff.shape[-1]
    x2, p2, d2 = x.view(-1, Cx), proj.view(-1, Cp), diff.view(-1, D)
    w2f = w2.view(-1)
    if b2 is not None:
        d2 = torch.cat([d2, torch.ones_like(d2[:, :1])], 1)
        w2f = torch.cat([w2f.detach(), b2.detach().view(-1)])
    out2, mask, pre, argmax = K.dynfilter_fwd(p2, d2, w2f, x2)
    out = out2.view(x.shape)
    mask4 = mask.view(*x.shape[:-1], 1)
    if _needs(tape):
        def bwd():
            dout = tape.pop_grad(out)
            dmask = tape.pop_grad(mask4)
            if dout is None and dmask is None:
                return
            if dout is None:
                dout = torch.zeros_like(out)
            dx, dlogit, dproj = K.dynfilter_bwd(dout.view(-1, Cx), None if dmask is None else dmask.view(-1),
                                                x2, mask, argmax, w2f, Cp)
            tape.add_grad(x, dx.view(x.shape))
            tape.add_grad(proj, dproj.view(proj.shape))
            if diff_grad:
                tape.add_grad(diff, K.outer(dlogit, w2f[2:2 + D]).view(diff.shape))
            if not _wgrad(tape):
                return
            # dw2[j] = sum_m dlogit[m] * pre[m][j]   (8 or 5 numbers)
            g = K.gemm_tn(dlogit.view(-1, 1), pre)                 # [1, 2 + D (+ 1)]
            if b2 is None:
                tape.add_param_grad(w2, g.view(w2.shape))
            else:
                tape.add_param_grad(w2, g[:, :-1].reshape(w2.shape))
                tape.add_param_grad(b2, g[:, -1].reshape(b2.shape))
        tape.record(bwd)
    return out, mask4


# ---------------------------------------------------------------------------------------------
# ResNet-variant operators
# ---------------------------------------------------------------------------------------------
def conv_dense_any(tape, x, w, stride, pad, need_dx=True, x_planes=None):
    """Dense k x k F.conv2d with symmetric padding and any stride (ResNet convs, model/resnet/exp.py:95-111;
    7x7/2 stem :395; 1x1/2 downsample :235-246).  The data gradient is the transposed-conv gather
    (t = ih + pad - kh, oh = t / stride) with the un-flipped weights.  x_planes: as in conv_dense (the stem)."""
    N, Hin, Win, Ci = x.shape
    Co, _, KH, KW = w.shape
    Hout = (Hin + 2 * pad - KH) // stride + 1
    Wout = (Win + 2 * pad - KW) // stride + 1
    g = K.conv_geom(N, Hin, Win, Ci, Hout, Wout, KH, KW, stride, pad, pad, 0)
    wmat = K.weight_layout(w, 0)
    stem_dx = _tracks(tape, x_planes)
    if K.conv_im2col_ok(g, Co, x):
        assert not stem_dx
        return _conv_im2col(tape, x, w, wmat, g, need_dx)
    y = K.conv_gather_nt(x, wmat, g)
    if _needs(tape):
        wd = K.weight_layout(w, 2) if need_dx else None

        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            if need_dx:
                gd = K.conv_geom(N, Hout, Wout, Co, Hin, Win, KH, KW, stride, pad, pad, 1)
                tape.add_grad(x, K.conv_gather_nt(dy, wd, gd))
            elif stem_dx:
                _stem_dgrad(tape, dy, w, g, x_planes)
            if _wgrad(tape):
                tape.add_param_grad(w, K.conv_wgrad_param(dy.view(-1, Co), x, g))
        tape.record(bwd)
    return y


def sfconv_dense(tape, x, w, w_freq, alpha, stride, norm, bias=None):
    """SFConv2d.forward (model/resnet/exp.py:36-54): dense 3x3 conv (padding 1; + its bias, :39) + spectral 1x1 branch."""
    spat = bias_add(tape, conv_dense_any(tape, x, w, stride, 1), bias)
    xf = rfft2_cat(tape, x, norm)
    yf = conv1x1(tape, xf, w_freq)
    fr = irfft2_split(tape, yf, norm)
    return sfmix(tape, spat, fr, alpha)


def add_relu(tape, a, b, site=None):
    """`x += shortcut; x = relu(x)` (model/resnet/exp.py:146-147).  site: name under which the parity tests find
    this ReLU's on/off pattern (tape.kinks)."""
    y = K.add_act(a, b, 2)
    if tape is not None and tape.kinks is not None and site is not None:
        tape.kinks[site] = y
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            g = K.relu_bwd(dy, y)
            tape.add_grad(a, g)
            tape.add_grad(b, g)
        tape.record(bwd)
    return y


def avgpool(tape, x, k):
    """F.adaptive_avg_pool2d to (H/k, W/k) (model/resnet/module_exp.py:30-31)."""
    if k == 1:
        return x
    y = K.avgpool_fwd(x, k)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.avgpool_bwd(dy, k))
        tape.record(bwd)
    return y


def maxpool3s2(tape, x, return_arg=False):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (model/resnet/module_exp.py:73-75).
    return_arg: also hand back the uint8 winner map (kh*3+kw per window) for the parity tests."""
    H, W = x.shape[1], x.shape[2]
    y, arg = K.maxpool3s2_fwd(x)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            tape.add_grad(x, K.maxpool3s2_bwd(dy, arg, H, W))
        tape.record(bwd)
    return (y, arg) if return_arg else y


def concat_channels(tape, parts):
    """torch.cat(dim=1) in NCHW = channel concat in pixel-major (model/resnet/module_exp.py:32)."""
    y = K.concat_channels(parts)
    if _needs(tape):
        def bwd():
            dy = tape.pop_grad(y)
            if dy is None:
                return
            off = 0
            for p in parts:
                tape.add_grad(p, K.slice_channels(dy, off, p.shape[-1]))
                off += p.shape[-1]
        tape.record(bwd)
    return y


# ---------------------------------------------------------------------------------------------
# What the block nodes of mbconv.py (one tape node per MBConv block) share with the model: the SyncBatchNorm context
# of the fused path and the storage-type boundary of the half-storage trunk
# ---------------------------------------------------------------------------------------------
# bench.py's data-parallel diagnostics: when set to {"bn": [], "ar": []}, every SyncBN sum is bracketed by HIP events on its launch
# stream — (start, end, doubles) — and GradReducer.finish() appends (backward end, last collective waited for, bytes, collectives)
DP_PROFILE = None


class DataParallelCtx:
    """SyncBatchNorm context of the fused path: the fp64 accumulators are summed over the ranks in place (one
    all_reduce between the producing and the consuming kernels), counts are multiplied by the world size."""

    def __init__(self, group=None, exchange=None):
        self.group, self.world, self.synced = group, 1, False
        self.exchange = exchange            # engine.parallel.BnExchange (one kernel per sum) or None (dist.all_reduce)
        if group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(group)
            self.synced = self.world > 1 or cfg.force_collectives

    def reduce(self, acc, keep_local=False):
        """Sum `acc` over the ranks in place; returns this rank's own sums (a copy) when keep_local, else None."""
        if not self.synced:
            return None
        via_exchange = self.exchange is not None and acc.numel() <= self.exchange.MAX_DOUBLES
        # the rank's own sums: written by the exchange kernel itself (round 6; a clone launch per BatchNorm backward before)
        loc = (torch.empty_like(acc) if via_exchange else acc.clone()) if keep_local else None
        prof = DP_PROFILE
        if prof is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if via_exchange:
            self.exchange.allreduce(acc, loc)
        else:
            import torch.distributed as dist
            dist.all_reduce(acc, group=self.group)
        if prof is not None:
            e1.record()
            prof["bn"].append((e0, e1, acc.numel()))
        return loc


def cast(tape, x, dtype):
    """Storage-type boundary of the half-storage trunk (fp16 activations between the fp32 stem / decoder / attention /
    head): y = x.to(dtype), the gradient converted back."""
    if x.dtype == dtype:
        return x
    y = x.to(dtype)
    if _needs(tape):
        def bwd():
            g = tape.pop_grad(y)
            if g is not None:
                tape.add_grad(x, g.reshape(x.shape).to(x.dtype))
        tape.record(bwd)
    return y

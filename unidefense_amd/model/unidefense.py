"""UniDefenseModelEb4 on the MI355X HIP kernels.

Mirror of the reference's ``model/unidefense.py:28-256`` (class surface, constructor kwargs, forward
signature and return dict, state-dict key names).  The torch.nn modules below are only PARAMETER
CONTAINERS (they give the reference's key names, shapes and default initialisers); their ``forward`` is
never called — all compute goes through ``unidefense_amd.tape`` operators, i.e. the hand-written HIP kernels.
Internally every activation is pixel-major [N,H,W,C]; the public tensors keep the reference's NCHW shapes.
"""
from typing import List, Optional

import torch
import torch.nn as nn

from .. import kernels as K
from ..config import cfg
from .. import mbconv as MB
from .. import tape as T
from .arch import DELIMITER_DICT, build_arch


# ---------------------------------------------------------------------------------------------
# parameter containers (same attribute names as the reference => same state-dict keys)
# ---------------------------------------------------------------------------------------------
class _SFConvParams(nn.Conv2d):
    """model/efficientnet/exp.py:7-44 (SFConv2dStaticSamePadding: weight + freq_conv + sf_coef)."""

    def __init__(self, channels, k):
        super().__init__(channels, channels, k, groups=channels, bias=False)
        self.freq_conv = nn.Conv2d(channels * 2, channels * 2, kernel_size=1, bias=False)
        self.sf_coef = nn.Parameter(torch.tensor(-10.0))


class _MBConvParams(nn.Module):
    """model/efficientnet/model.py:52-92."""

    def __init__(self, spec, eps, momentum):
        super().__init__()
        self.spec = spec
        if spec.expand != 1:
            self._expand_conv = nn.Conv2d(spec.cin, spec.cexp, 1, bias=False)
            self._bn0 = nn.BatchNorm2d(spec.cexp, momentum=momentum, eps=eps)
        if spec.sf_norm is not None:
            self._depthwise_conv = _SFConvParams(spec.cexp, spec.k)
        else:
            self._depthwise_conv = nn.Conv2d(spec.cexp, spec.cexp, spec.k, groups=spec.cexp, bias=False)
        self._bn1 = nn.BatchNorm2d(spec.cexp, momentum=momentum, eps=eps)
        self._se_reduce = nn.Conv2d(spec.cexp, spec.cse, 1)
        self._se_expand = nn.Conv2d(spec.cse, spec.cexp, 1)
        self._project_conv = nn.Conv2d(spec.cexp, spec.cout, 1, bias=False)
        self._bn2 = nn.BatchNorm2d(spec.cout, momentum=momentum, eps=eps)


class _Backbone(nn.Module):
    """model/efficientnet/model.py:166-231 with include_top=False."""

    def __init__(self, arch):
        super().__init__()
        eps, mom = arch["bn_eps"], arch["bn_momentum"]
        self._conv_stem = nn.Conv2d(3, arch["stem"]["cout"], 3, stride=2, bias=False)
        self._bn0 = nn.BatchNorm2d(arch["stem"]["cout"], momentum=mom, eps=eps)
        self._blocks = nn.ModuleList([_MBConvParams(s, eps, mom) for s in arch["blocks"]])
        self._conv_head = nn.Conv2d(arch["head"]["cin"], arch["head"]["cout"], 1, bias=False)
        self._bn1 = nn.BatchNorm2d(arch["head"]["cout"], momentum=mom, eps=eps)


class Classifier(nn.Module):
    """model/modules.py:24-32."""

    def __init__(self, depth=512, num_classes=2):
        super().__init__()
        self.fc = nn.Linear(depth, num_classes)
        self.fc.weight.data.normal_(0, 0.01)
        self.fc.bias.data.fill_(0.0)


class _FilterParams(nn.Module):
    """model/modules.py:79-89 / 108-118 (layer1 = conv + norm + act, layer2 = conv + sigmoid)."""

    def __init__(self, cin, k, d_in, affine, bias):
        super().__init__()
        self.layer1 = nn.Sequential(nn.Conv2d(cin, cin, k, 1, k // 2, bias=bias), nn.BatchNorm2d(cin, affine=affine),
                                    nn.Identity())
        self.layer2 = nn.Sequential(nn.Conv2d(d_in, 1, 1, bias=bias), nn.Identity())


def _decoder(cin, cout, affine, bias, last):
    """model/unidefense.py:59-102: indices 0,1,3,4,6,7(,9) carry parameters."""
    mods = [nn.Conv2d(cin, cout, 3, 1, 1, bias=bias), nn.InstanceNorm2d(cout, affine=affine), nn.Identity(),
            nn.ConvTranspose2d(cout, cout, 3, 2, 1, output_padding=1, bias=bias),
            nn.InstanceNorm2d(cout, affine=affine), nn.Identity(),
            nn.Conv2d(cout, cout, 3, 1, 1, bias=bias), nn.InstanceNorm2d(cout, affine=affine), nn.Identity()]
    if last:
        mods += [nn.Conv2d(cout, 3, 3, 1, 1, bias=bias), nn.Identity()]
    return nn.Sequential(*mods)


# ---------------------------------------------------------------------------------------------
# the single autograd node wrapping the taped HIP forward/backward
# ---------------------------------------------------------------------------------------------
_OUT_KEYS = ("cls_out", "rec", "factorization", "triplet0", "triplet1", "triplet2", "freq_mask", "spat_mask",
             "spatial", "freq")


# training mode: MBConv blocks as fused tape nodes with deferred BatchNorms (mbconv.mbconv_fused); cfg.fused_mbconv = False
# runs the operator-by-operator path (same results: tests/test_z_fused_selfcheck_gpu.py compares the two)
def _fused_mbconv():
    return cfg.fused_mbconv


def _half_storage(model):
    """fp16 activation storage in the MBConv trunk: `model.half_storage = True` (or cfg.half_storage)."""
    return bool(getattr(model, "half_storage", cfg.half_storage))


_MULTI_ADD_MIN = 8          # fewer accumulating parameters than this: leave them to autograd


def _accumulate_in_place(model, params, grads):
    """A backward onto EXISTING .grad buffers — the train step's second backward() under its one zero_grad()
    (engine/abstract_engine.py:281, 374; forgery_engine.py:241) — would have autograd's AccumulateGrad add every gradient with a
    launch of its own: 504 launches, 2.7 ms of a 64 ms step.  The same `grad += new` (in place, as AccumulateGrad does when no
    graph is being built) for all of them in ceil(n / 120) launches; those parameters report None to autograd, the rest
    (no .grad yet, other dtype / layout, a tensor hook) take the usual road.  OPT-IN (`model._ud_inplace_accumulate`, set by the
    engine's train step): a wrapper that hangs its gradient exchange on the AccumulateGrad nodes — torch's
    DistributedDataParallel — must see every gradient pass through autograd."""
    if not getattr(model, "_ud_inplace_accumulate", False) or torch.is_grad_enabled():
        return grads
    idx = [i for i, (p, g) in enumerate(zip(params, grads))
           if g is not None and p.grad is not None and p.grad.dtype == torch.float32 and g.dtype == torch.float32
           and p.grad.is_contiguous() and p.grad.shape == g.shape and p.grad.device == g.device and not p.grad.requires_grad
           and not p._backward_hooks and not getattr(p, "_post_accumulate_grad_hooks", None)]
    if len(idx) < _MULTI_ADD_MIN:
        return grads
    K.multi_add([params[i].grad for i in idx], [grads[i].contiguous() for i in idx])
    grads = list(grads)
    for i in idx:
        grads[i] = None
    return grads


class _NetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, noise_x, rng, *params):
        K.begin_forward(model)     # fresh zero blocks (a captured step fills every block it carves from); weight planes in two launches
        tape = T.Tape()
        # x.grad: the input image is tracked when it requires grad and feeds the encoder itself (a perturbed copy does not
        # pass a gradient back: no gradient through the perturbation functions); a model with no parameter requiring grad in
        # eval mode (frozen, the tape exists only for x) launches no weight-gradient work
        if ctx.needs_input_grad[1] and noise_x is None:
            tape.input = x
        tape.wgrad_on = model.training or any(ctx.needs_input_grad[4:])
        debug = getattr(model, "_debug_watch", False)
        if debug:
            tape.kinks = {}
        try:
            outs = model._run(x, tape, rng, noise_x)
            tape.weight_snapshot = K.weight_batch_snapshot()
        finally:
            K.end_forward()
        if debug:                                            # tests: capture activation gradients / ReLU patterns
            tape.watch = {id(t): k for k, t in outs["_feats"].items()}
            model._debug_tape = tape
            model._debug_feats = outs["_feats"]
            names = {id(p): n[: -len(".weight")] for n, p in model.named_parameters() if n.endswith(".weight")}
            model._debug_kinks = {names.get(k, k): (y > 0) for k, y in tape.kinks.items()}
        ctx.tape = tape
        ctx.outs = outs
        ctx.params = params
        ctx.x_tracked = tape.input is not None
        ctx.model = model
        ctx.keys = model._out_keys
        return tuple(outs[k] for k in ctx.keys)

    @staticmethod
    def backward(ctx, *gouts):
        tape, outs, model = ctx.tape, ctx.outs, ctx.model
        K.reset_zero_pool()
        # data parallel (engine/parallel.py): scaling the incoming gradient by 1/world turns the reducer's SUM into
        # the mean; gradients are handed over as they become final so that their all-reduce overlaps the rest of
        # this backward (use counts per parameter are learned on the first backward, which reduces at its end).  A frozen
        # model's backward (tape.wgrad_on False: only x.grad) has no parameter gradient to exchange: it leaves the reducer,
        # its prescale and the learned use counts alone
        reducer = getattr(model, "_grad_reducer", None) if tape.wgrad_on else None
        scale = getattr(model, "_grad_prescale", 1.0) if reducer is not None else 1.0
        uses = getattr(model, "_param_uses", None)
        if reducer is not None:
            reducer.begin()
            if uses is not None:
                tape.param_uses, tape.param_ready = uses, reducer.ready
        for k, g in zip(ctx.keys, gouts):
            if g is not None:
                g = g.contiguous().to(torch.float32)
                tape.add_grad(outs[k], g if scale == 1.0 else g * scale)
        tape.backward()
        grads = [tape.param_grads.get(p) if p.requires_grad else None for p in ctx.params]
        if reducer is not None:
            if uses is None:
                model._param_uses = dict(tape.param_seen)
            elif uses != tape.param_seen:
                raise RuntimeError("data parallel: the set of parameter-gradient contributions changed between "
                                   "backward passes; streamed buckets would hold partial gradients")
            for p, g in zip(reversed(ctx.params), reversed(grads)):
                if g is not None and id(p) not in reducer.done:
                    reducer.ready(id(p), g)
            red = reducer.finish()
            grads = [None if g is None else red[id(p)] for p, g in zip(ctx.params, grads)]
        grads = _accumulate_in_place(model, ctx.params, grads)
        dx = tape.input_grad if ctx.x_tracked else None
        if dx is not None and scale != 1.0:
            dx = K.axpby(dx, 1.0 / scale)          # x.grad stays the rank's own gradient (as with DistributedDataParallel)
        tape.input = tape.input_grad = None
        ctx.tape = ctx.outs = ctx.model = None
        return (None, dx, None, None) + tuple(grads)


class RunnerMethods:
    """The graph-replayed runners of a model, each cached per argument tuple in a dictionary of its own (unidefense_amd/infer.py,
    unidefense_amd/attack.py).  precision "fp16": UDEB4 only (the ResNet variants have no half-storage path: ValueError)."""

    def inference_runner(self, batch, size, precision="fp32"):
        """The graph-captured eval forward for [batch, 3, size, size] inputs (InferenceRunner); precision "fp16": the MBConv
        trunk in half storage (mbconv.mbconv_eval_half)."""
        from ..infer import inference_runner
        return inference_runner(self, batch, size, precision)

    def input_grad_runner(self, batch, size, objective="cross_entropy", precision="fp32", grad_scale=None):
        """The graph-replayed gradient of objective(model(x), y) with respect to x for [batch, 3, size, size] inputs
        (InputGradRunner).  precision "fp16": the MBConv trunk's forward and backward in half storage (mbconv.mbconv_frozen_half),
        the objective scaled by grad_scale (default 1024) and the result unscaled."""
        from ..attack import input_grad_runner
        return input_grad_runner(self, batch, size, objective, precision, grad_scale)

    def attack_runner(self, batch, size, **kwargs):
        """The graph-replayed FGSM / PGD attack for [batch, 3, size, size] inputs (AttackRunner; kwargs: norm, eps, steps, step,
        random_start, targeted, clip, objective, precision, grad_scale)."""
        from ..attack import attack_runner
        return attack_runner(self, batch, size, **kwargs)

    def apgd_runner(self, batch, size, **kwargs):
        """The graph-replayed Auto-PGD (APGD-CE) attack for [batch, 3, size, size] inputs (APGDRunner; kwargs: norm, eps, steps,
        restarts, random_start, rho, alpha, targeted, clip, objective, precision, grad_scale)."""
        from ..attack import apgd_runner
        return apgd_runner(self, batch, size, **kwargs)

    def fmn_runner(self, batch, size, **kwargs):
        """The graph-replayed Fast Minimum-Norm attack for [batch, 3, size, size] inputs: per sample the smallest perturbation
        that flips it (FMNRunner; kwargs: norm, steps, alpha_init, alpha_final, gamma_init, gamma_final, targeted, clip,
        objective, precision, grad_scale)."""
        from ..attack import fmn_runner
        return fmn_runner(self, batch, size, **kwargs)

    def sparse_fmn_runner(self, batch, size, **kwargs):
        """The graph-replayed sparse minimum-norm attack for [batch, 3, size, size] inputs: per sample the smallest L1 distance
        or the smallest number of changed elements that flips it (SparseFMNRunner; kwargs: norm ("l1" / "l0"), steps,
        alpha_init, alpha_final, gamma_init, gamma_final, targeted, clip, objective, precision, grad_scale)."""
        from ..attack import sparse_fmn_runner
        return sparse_fmn_runner(self, batch, size, **kwargs)

    def square_runner(self, batch, size, **kwargs):
        """The graph-replayed Square attack (black-box, L-infinity, forward only) for [batch, 3, size, size] inputs
        (SquareRunner; kwargs: eps, steps, p_init, restarts, early_stop, check_every, clip, objective, precision)."""
        from ..attack import square_runner
        return square_runner(self, batch, size, **kwargs)

    def corruption_runner(self, batch, size, kind, **kwargs):
        """A common corruption (JPEG, blur, noise, pixelation, contrast, saturation, blocks, or a chain of them) in front of the
        graph-replayed eval forward for [batch, 3, size, size] inputs (unidefense_amd/corrupt.py: CorruptionRunner; kwargs:
        level, param, precision, subsampling)."""
        from ..corrupt import corruption_runner
        return corruption_runner(self, batch, size, kind, **kwargs)

    def spatial_runner(self, batch, size, **kwargs):
        """The graph-replayed worst case over rotations, shifts, scales and mirrors (black-box, forward only) for [batch, 3, size,
        size] inputs (unidefense_amd/spatial.py: SpatialRunner; kwargs: max_angle, max_shift, scales, flip, search, grid, k,
        border, objective, precision)."""
        from ..spatial import spatial_runner
        return spatial_runner(self, batch, size, **kwargs)

    def universal_runner(self, batch, size, **kwargs):
        """The graph-replayed universal perturbation — one pattern of size eps for every image, held by the runner across calls
        — for [batch, 3, size, size] inputs (unidefense_amd/universal.py: UniversalRunner; kwargs: norm, eps, steps, step, beta,
        source, clip, precision, grad_scale, reduce)."""
        from ..universal import universal_runner
        return universal_runner(self, batch, size, **kwargs)

    def patch_runner(self, batch, size, **kwargs):
        """The graph-replayed adversarial patch — one small texture pasted into every image at a random place, roll and size,
        held by the runner across calls — for [batch, 3, size, size] inputs (unidefense_amd/patch.py: PatchRunner; kwargs:
        patch, shape, alpha, steps, step, max_angle, scales, region, beta, source, clip, precision, grad_scale, reduce)."""
        from ..patch import patch_runner
        return patch_runner(self, batch, size, **kwargs)

    def flow_runner(self, batch, size, **kwargs):
        """The graph-replayed flow-field (stAdv) attack — a per-pixel displacement field of at most max_flow pixels, ascended
        through a differentiable warp — for [batch, 3, size, size] inputs (unidefense_amd/flow.py: FlowRunner; kwargs: max_flow,
        steps, step, tau, tv_eps, targeted, objective, precision, grad_scale)."""
        from ..flow import flow_runner
        return flow_runner(self, batch, size, **kwargs)

    def band_runner(self, batch, size, **kwargs):
        """The graph-replayed frequency-band attack — L2 PGD whose perturbation is confined to one band of the image's 2-D DCT —
        for [batch, 3, size, size] inputs (unidefense_amd/band.py: BandRunner; kwargs: band, shape, mask, eps, steps, step,
        targeted, clip, objective, precision, grad_scale)."""
        from ..band import band_runner
        return band_runner(self, batch, size, **kwargs)

    def certify_runner(self, batch, size, **kwargs):
        """The graph-replayed randomized-smoothing certificate — per sample a radius inside which the smoothed decision provably
        does not change — for [batch, 3, size, size] inputs (unidefense_amd/smooth.py: CertifyRunner; kwargs: sigma, noise, n0, n,
        alpha, seed, logits, precision)."""
        from ..smooth import certify_runner
        return certify_runner(self, batch, size, **kwargs)

    def hsj_runner(self, batch, size, **kwargs):
        """The graph-replayed decision-based minimum-norm attack (HopSkipJump: black-box, the hard label only, forward only) for
        [batch, 3, size, size] inputs: per sample the smallest L2 / L-infinity perturbation found that changes the decision
        (unidefense_amd/hsj.py: HSJRunner; kwargs: norm, steps, probes, max_probes, bisect, halvings, init_trials, seed, clip,
        precision, logits)."""
        from ..hsj import hsj_runner
        return hsj_runner(self, batch, size, **kwargs)

    def attribution_runner(self, batch, size, **kwargs):
        """The graph-replayed attribution — integrated gradients, or SmoothGrad / a plain saliency map: which pixels the score of
        the label rests on, with the completeness defect `gap` — for [batch, 3, size, size] inputs (unidefense_amd/attrib.py:
        AttributionRunner; kwargs: method, steps, rule, baseline, samples, sigma, score, reduce, seed, precision, grad_scale)."""
        from ..attrib import attribution_runner
        return attribution_runner(self, batch, size, **kwargs)

    def deletion_runner(self, batch, size, **kwargs):
        """The graph-replayed deletion / insertion curve that scores a heat map: the class probability while the map's top pixels
        are replaced by the baseline, or inserted into it (unidefense_amd/attrib.py: DeletionRunner; kwargs: fractions, mode,
        baseline, score, precision)."""
        from ..attrib import deletion_runner
        return deletion_runner(self, batch, size, **kwargs)


class UniDefenseModelEb4(RunnerMethods, nn.Module):
    """UniDefense model with EfficientNet backbone (reference: model/unidefense.py:28-256)."""

    path = "model/unidefense.py"
    _out_keys = _OUT_KEYS
    _triplet_keys = ("triplet0", "triplet1", "triplet2")

    def __init__(self,
                 extractor,
                 extractor_weights: Optional[str] = None,
                 bias: bool = False,
                 drop_rate: float = 0.2,
                 affine: bool = True,
                 num_classes: int = 1,
                 delimiter: Optional[List] = None,
                 freq_norm: str = 'ortho',
                 **kwargs):
        super().__init__()
        self.arch = build_arch(extractor, freq_norm, kwargs.pop("image_size", None))
        if "drop_connect_rate" in kwargs:
            self.arch["drop_connect_rate"] = kwargs.pop("drop_connect_rate")
        for k_ in ("batch_norm_momentum", "batch_norm_epsilon"):
            if k_ in kwargs:
                v = kwargs.pop(k_)
                if k_ == "batch_norm_momentum":
                    self.arch["bn_momentum"] = 1 - v
                else:
                    self.arch["bn_eps"] = v
        if kwargs:
            raise TypeError(f"unsupported override params: {sorted(kwargs)}")
        self.backbone = _Backbone(self.arch)
        num_features = self.arch["head"]["cout"]
        self.freq_norm = freq_norm
        self.drop_rate = drop_rate

        self.dec_block1 = _decoder(160, 80, affine, bias, False)
        self.dec_block2 = _decoder(80, 40, affine, bias, False)
        self.dec_block3 = _decoder(40, 20, affine, bias, True)

        self.bottleneck = nn.BatchNorm1d(num_features)
        self.bottleneck.bias.requires_grad_(False)
        nn.init.constant_(self.bottleneck.weight, 1.0)
        nn.init.constant_(self.bottleneck.bias, 0.0)

        self.delimiter = delimiter or DELIMITER_DICT[extractor]
        self.classifier = Classifier(num_features, num_classes)

        att_depth = 272
        self.freq_filter = _FilterParams(att_depth * 2, 1, 8, affine, bias)
        self.spat_filter = _FilterParams(att_depth, 3, 5, affine, bias)
        self.fuse_coef = nn.Parameter(torch.tensor(0.))

        if extractor_weights is not None:
            self.load_backbone_weights(extractor_weights)

    # -- pretrained backbone (model/efficientnet/utils.py:589-634): missing sf_coef / freq_conv keys tolerated
    def load_backbone_weights(self, path):
        sd = torch.load(path, map_location="cpu")
        sd.pop("_fc.weight", None)
        sd.pop("_fc.bias", None)
        ret = self.backbone.load_state_dict(sd, strict=False)
        bad = [k for k in ret.missing_keys if "sf_coef" not in k and "freq_conv" not in k]
        if bad or ret.unexpected_keys:
            raise RuntimeError(f"pretrained weights mismatch: missing {bad}, unexpected {ret.unexpected_keys}")

    def forward(self, x, pert_real_list=None, pert_fake_list=None, preserve_color=None, rng=None, **kwargs):
        """Returns {'cls_out','rec','loss_dict'} like the reference (model/unidefense.py:174-256).
        rng: optional dict of explicit keep-masks (NCHW-shaped like the reference's tensors):
        'drop_connect' {block: [N]}, 'dec_keep' [N,160,h,w], 'emb_keep' [N,272,h,w], 'feat_keep' [N,F]."""
        # the perturbed copy feeds the encoder only; the attention residuals and the reconstruction losses keep the
        # clean input (model/unidefense.py:200, :219, :243-248).  kwargs['noise_x']: an already perturbed copy (the
        # graph-captured engine step perturbs outside the captured region, engine/abstract_engine.py)
        noise_x = kwargs.get("noise_x") if self.training else None
        if noise_x is not None:
            noise_x = noise_x.contiguous().to(torch.float32)
        elif self.training and pert_real_list is not None and pert_fake_list is not None:
            from . import perturb
            with torch.no_grad():
                noise_x = perturb.perturb_input(x, pert_real_list, pert_fake_list, preserve_color)
            noise_x = noise_x.contiguous().to(torch.float32)
        if rng is None and getattr(self, "rng_queue", None):
            rng = self.rng_queue.pop(0)        # parity tests: explicit masks for successive forward calls
        if not x.is_cuda:
            raise RuntimeError("unidefense_amd runs on the GPU only (no CPU path); move the model and input to cuda")
        x = x.contiguous().to(torch.float32)
        # a tape is built whenever autograd would record: training, or an eval-mode forward outside no_grad() whose
        # parameters or input require gradients (fine-tuning on frozen BatchNorm statistics; x.grad of a frozen model for an
        # attack or a saliency map; the reference is plain autograd)
        if torch.is_grad_enabled() and (self.training or x.requires_grad or any(p.requires_grad for p in self.parameters())):
            params = tuple(self.parameters())
            vals = _NetFunction.apply(self, x, noise_x, rng, *params)
            outs = dict(zip(self._out_keys, vals))
        else:
            with torch.no_grad():
                K.begin_forward(self)
                try:
                    outs = self._run(x, None, rng, noise_x)
                finally:
                    K.end_forward()
        pending = self.__dict__.pop("_nbt_pending", None)
        if pending:
            torch._foreach_add_(pending, 1)
        loss_dict = {
            "factorization": outs["factorization"],
            "triplet": [outs[k] for k in self._triplet_keys],
            "freq_mask": outs["freq_mask"].permute(0, 3, 1, 2),      # [N,h,w,1] -> [N,1,h,w]
            "spat_mask": outs["spat_mask"].permute(0, 3, 1, 2),
            "spatial": outs["spatial"],
            "freq": outs["freq"],
        }
        return {"cls_out": outs["cls_out"], "rec": outs["rec"], "loss_dict": loss_dict}

    # ---------------------------------------------------------------------------------------
    def _bn(self, tape, x, bn, act):
        training = self.training
        if training and bn.num_batches_tracked is not None:
            # bumped once per forward with ONE multi-tensor launch (forward()), not one launch per BatchNorm
            self.__dict__.setdefault("_nbt_pending", []).append(bn.num_batches_tracked)
        # SyncBatchNorm semantics when a data-parallel wrapper set a process group, or when the container was
        # converted by torch.nn.SyncBatchNorm.convert_sync_batchnorm (engine/forgery_engine.py:142)
        group = self._sync_group(bn)
        return T.batchnorm_act(tape, x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                               bn.momentum if bn.momentum is not None else 0.1, training, act, group,
                               getattr(self, "_bn_exchange", None))

    def _mbconv(self, tape, x, blk, keep, keep_prob):
        """MBConvBlock.forward (model/efficientnet/model.py:94-135)."""
        sp = blk.spec
        inp = x
        if sp.expand != 1:
            x = T.conv1x1(tape, x, blk._expand_conv.weight)
            x = self._bn(tape, x, blk._bn0, 1)
        dw = blk._depthwise_conv
        if sp.sf_norm is not None:
            x = T.sfconv_dw(tape, x, dw.weight, dw.freq_conv.weight, dw.sf_coef, sp.stride, sp.pad, sp.sf_norm)
        else:
            x = T.dwconv(tape, x, dw.weight, sp.stride, sp.pad)
        x = self._bn(tape, x, blk._bn1, 1)
        x = T.squeeze_excite(tape, x, blk._se_reduce.weight, blk._se_reduce.bias, blk._se_expand.weight,
                             blk._se_expand.bias)
        x = T.conv1x1(tape, x, blk._project_conv.weight)
        x = self._bn(tape, x, blk._bn2, 0)
        if sp.skip:
            if self.training and keep is not None:
                x = T.residual(tape, x, inp, keep, keep_prob)
            else:
                x = T.residual(tape, x, inp)
        return x

    # widest block input the eval-mode node takes: the expand conv runs on the FMA pipe inside ud_mb_eval_dw, which pays at the
    # thin block group 1 (24 / 32 inputs) but not at the last group (272 / 448 inputs: 729 us per block at bs 96 on 8 x 8 maps,
    # profiles/r07/infer.txt), where the expand GEMM on the matrix pipe + the composed kernels stay
    EVAL_NODE_MAX_CIN = 32
    # the same for the half-storage node of the fp16 InferenceRunner (ud_mb_eval_dw_h: the expand conv on fp16 MFMA), from the A/B
    # of tools/bench_infer.py --ab-node-h (profiles/r08/infer_fp16.txt): whole fp16 replay at 256^2 bs 96 16.93 ms without the node,
    # 17.00 with it on group 1 (Ci 24 / 32), 17.20 also on group 7 (Ci 272 / 448); 380^2 bs 96 42.95 / 43.12 / 43.89
    EVAL_NODE_H_MAX_CIN = 0          # measured slower than the composed half kernels on both groups: off

    def _blocks(self, tape, x, stage, rng, mode, lazy_in=None):
        """forward_backbone_block (model/unidefense.py:159-172).  mode: the mbconv.TrunkMode _run chose; a block its node does not
        take runs on the operators (_mbconv)."""
        start = self.delimiter[stage - 1] if stage > 0 else 0
        end = self.delimiter[stage]
        nblk = len(self.backbone._blocks)
        rate0 = self.arch["drop_connect_rate"]
        for idx in range(start, end):
            rate = rate0 * float(idx) / nblk if rate0 else 0.0
            keep = rng["drop_connect"].get(idx) if (self.training and rate) else None
            blk = self.backbone._blocks[idx]
            wt = mode.wt[id(blk._depthwise_conv.weight)]
            # an SF block on a map side fft.hip has no in-register transform for (95 at 380 x 380) is not for the fused / half nodes
            sf_ok = blk.spec.sf_norm is None or K.fft_kernel_size(x.shape[1])
            if mode.kind == MB.FUSED and sf_ok:
                # training mode: one tape node per block, BatchNorms deferred into their consumers (mbconv.mbconv_fused)
                pend = self.__dict__.setdefault("_nbt_pending", [])
                pend.extend(b.num_batches_tracked for b in (getattr(blk, "_bn0", None), blk._bn1, blk._bn2)
                            if b is not None and b.num_batches_tracked is not None)
                nxt = self.backbone._blocks[idx + 1] if idx + 1 < end else None          # (within the stage: its input IS this output)
                x = MB.mbconv_fused(tape, x, blk, keep, 1.0 - rate, wt, mode.dp, lazy_in if idx == 0 else None, next_blk=nxt)
            elif mode.kind == MB.HALF and sf_ok and tape is not None:
                # an fp16 gradient runner (unidefense_amd/attack.py): the fp16 runners' forward (below) as ONE tape node with the
                # frozen half backward
                x = MB.mbconv_frozen_half(tape, x, blk, wt, lazy_in if idx == start else None)
            elif mode.kind == MB.HALF and sf_ok:
                # the fp16 runners' forward: half storage, eval-form BatchNorms, no statistics (the SF block left out above
                # takes the operator path below, in fp32 between two casts)
                x = MB.mbconv_eval_half(x, blk, wt, lazy_in if idx == start else None, self.EVAL_NODE_H_MAX_CIN)
            elif mode.kind == MB.EVAL_NODE and MB.eval_block_ok(blk, type(self).EVAL_NODE_MAX_CIN):
                # eval-mode node of an InferenceRunner's forward (unidefense_amd/infer.py): expand conv inside the depthwise pass
                x = MB.mbconv_eval(x, blk, wt)
            else:
                dt = x.dtype                                   # the operator path computes in fp32 storage
                if dt != torch.float32:
                    x = T.cast(tape, x, torch.float32)
                x = self._mbconv(tape, x, blk, keep, 1.0 - rate)
                if dt != torch.float32:
                    x = T.cast(tape, x, dt)
        return x

    def _sync_group(self, bn):
        group = getattr(self, "_sync_bn_group", None)
        if group is None and isinstance(bn, nn.SyncBatchNorm) and torch.distributed.is_initialized():
            group = bn.process_group or torch.distributed.group.WORLD
        return group

    def _decoder(self, tape, x, dec, last):
        # conv biases (bias=True) and norm affines (affine=False: weight / bias are None) follow the constructor variant
        x = T.bias_add(tape, T.conv_dense(tape, x, dec[0].weight, 1, 1, 1, x.shape[1], x.shape[2]), dec[0].bias)
        x = T.instancenorm_act(tape, x, dec[1].weight, dec[1].bias, dec[1].eps, 1)
        x = T.bias_add(tape, T.conv_transpose_s2(tape, x, dec[3].weight), dec[3].bias)
        x = T.instancenorm_act(tape, x, dec[4].weight, dec[4].bias, dec[4].eps, 1)
        x = T.bias_add(tape, T.conv_dense(tape, x, dec[6].weight, 1, 1, 1, x.shape[1], x.shape[2]), dec[6].bias)
        x = T.instancenorm_act(tape, x, dec[7].weight, dec[7].bias, dec[7].eps, 1)
        if last:
            x = T.bias_add(tape, T.conv_dense(tape, x, dec[9].weight, 1, 1, 1, x.shape[1], x.shape[2]), dec[9].bias)
        return x

    def _attention(self, tape, pred_planes, x_planes, emb, rng):
        """UniDefenseModelEb4.attention (model/unidefense.py:125-157); pred carries no gradient, x when the tape tracks it."""
        N, h, w, Cc = emb.shape
        norm = self.freq_norm
        freq_diff, spat_diff, dg = T.attention_diffs(tape, pred_planes, x_planes, h, w, norm)   # [N,h,w/2+1,6], [N,h,w,3]
        emb_freq = T.rfft2_cat(tape, emb, norm)                         # [N,h,w/2+1,2C]
        ff = self.freq_filter
        proj = T.bias_add(tape, T.conv1x1(tape, emb_freq, ff.layer1[0].weight), ff.layer1[0].bias)
        proj = self._bn(tape, proj, ff.layer1[1], 1)
        f_out, freq_mask = T.dynamic_filter(tape, emb_freq, proj, freq_diff, ff.layer2[0].weight, ff.layer2[0].bias, dg)
        freq_filtered = T.irfft2_split(tape, f_out, norm)

        sfm = self.spat_filter
        proj = T.bias_add(tape, T.conv_dense(tape, emb, sfm.layer1[0].weight, 1, 1, 1, h, w), sfm.layer1[0].bias)
        proj = self._bn(tape, proj, sfm.layer1[1], 1)
        s_out, spat_mask = T.dynamic_filter(tape, emb, proj, spat_diff, sfm.layer2[0].weight, sfm.layer2[0].bias, dg)

        out = T.gate_mix(tape, s_out, freq_filtered, self.fuse_coef)
        e = emb
        if self.training and self.drop_rate > 0:
            e = T.dropout_mask(tape, emb, self._keep_mask(rng, "emb_keep", emb, 1.0 - self.drop_rate), self.drop_rate)
        out = T.add(tape, out, e)
        return out, freq_mask, spat_mask

    @staticmethod
    def _to_pix_mask(m):
        """NCHW keep-mask -> pixel-major."""
        return m.permute(0, 2, 3, 1).contiguous() if m.dim() == 4 else m.contiguous()

    def _prepare_rng(self, rng, n, device):
        """Resolve the drop-connect keep vectors (given or freshly drawn); the dropout keep-masks are
        resolved lazily by _keep_mask once the activation shapes are known."""
        out = {"drop_connect": {}, "_given": rng or {}}
        if not self.training:
            return out
        rate0 = self.arch["drop_connect_rate"]
        nblk = len(self.arch["blocks"])
        given = out["_given"].get("drop_connect", {})
        todo = [(idx, rate0 * float(idx) / nblk) for idx, b in enumerate(self.arch["blocks"])
                if b.skip and rate0 and idx > 0]
        fresh = None
        if any(given.get(idx) is None for idx, _ in todo):
            # all Bernoulli draws of the step in ONE launch (torch.bernoulli of a probability tensor; rounds 1-4: rand, compare, cast)
            # one probability tensor per (device, batch size), NEVER replaced: a captured step bakes its address in, and hipGraphs
            # do not keep their inputs alive — a cache of one entry would hand a replay of the earlier shape freed memory
            cache = self.__dict__.setdefault("_dc_keep_p", {})
            keep_p = cache.get((device, n))
            if keep_p is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("drop-connect probabilities for a new batch size inside a graph capture: run one eager "
                                       "step with this shape first (the engine and bench.py do)")
                keep_p = cache[(device, n)] = torch.tensor([1.0 - r for _, r in todo], device=device).view(-1, 1).expand(-1, n).contiguous()
            fresh = torch.bernoulli(keep_p)
        for j, (idx, rate) in enumerate(todo):
            k_ = given.get(idx)
            out["drop_connect"][idx] = k_.to(device=device, dtype=torch.float32).contiguous() if k_ is not None \
                else fresh[j]
        return out

    def _keep_mask(self, rng, name, like, keep_p):
        """Keep-mask for a dropout site: the caller-supplied NCHW mask (converted) or a fresh Bernoulli draw."""
        m = rng["_given"].get(name)
        if m is not None:
            m = self._to_pix_mask(m.to(device=like.device, dtype=torch.float32))
            assert m.shape == like.shape, (name, tuple(m.shape), tuple(like.shape))
            return m
        return torch.empty(like.shape, dtype=torch.float32, device=like.device).bernoulli_(keep_p)      # one launch

    def _run(self, x, tape, rng, noise_x=None):
        """The whole forward on HIP kernels.  x: [N,3,H,W] planes; noise_x: perturbed encoder input or None."""
        N, _, H, W = x.shape
        arch = self.arch
        bb = self.backbone
        st = arch["stem"]
        pl, pt = st["pad"][0], st["pad"][2]
        Ho, Wo = T.conv_out_hw(H, W, 3, 2, st["pad"])
        rng = self._prepare_rng(rng, N, x.device)
        ws = [blk._depthwise_conv.weight for blk in bb._blocks]
        wts = K.dw_weights_tapmajor(ws)                                  # all depthwise weights to tap-major, one launch
        T.DW_WT = {id(w): (w, w._version, wts[id(w)]) for w in ws}       # looked up by the unfused tape.dwconv

        x_pix = K.planes_to_pix(x if noise_x is None else noise_x)       # [N,H,W,3]
        x_in = x if noise_x is None else None                            # the stem's data gradient goes to x (tape.input)
        # Half storage (BASELINE configs[4]): the MBConv trunk keeps its activations and their gradients in fp16 (fp32
        # registers, fp64 BatchNorm sums, fp32 weights / weight gradients, fp16 MFMA); stem conv, decoder, attention,
        # head and losses stay fp32 — T.cast at the boundaries.  Fused training path only.
        fused = self.training and _fused_mbconv()
        # the fp16 InferenceRunner (unidefense_amd/infer.py): the eval forward with the same storage boundaries; with a tape: the fp16
        # InputGradRunner / AttackRunner (unidefense_amd/attack.py), whose frozen backward stays in half storage too
        ev16 = not self.training and bool(self.__dict__.get("_eval_half"))
        st16 = (fused and _half_storage(self)) or ev16
        f32 = torch.float32
        if fused:
            dp = T.DataParallelCtx(self._sync_group(bb._bn0), getattr(self, "_bn_exchange", None))
            mode = MB.TrunkMode(MB.FUSED, wts, dp)
            if bb._bn0.num_batches_tracked is not None:
                self.__dict__.setdefault("_nbt_pending", []).append(bb._bn0.num_batches_tracked)
            h, lazy = MB.stem_fused(tape, x_pix, bb._conv_stem.weight, bb._bn0, 2, pt, pl, Ho, Wo, dp,
                                   torch.float16 if st16 else f32, x_planes=x_in)
            x_b0 = self._blocks(tape, h, 0, rng, mode, lazy)
        elif ev16:
            # the stem conv's output rounded once to half; its eval BatchNorm + swish applied on load by block 0's depthwise conv
            mode = MB.TrunkMode(MB.HALF, wts)
            stem_bn = K.EvalBN(bb._bn0, 1)
            if tape is None:
                h = T.conv_dense(tape, x_pix, bb._conv_stem.weight, 2, pt, pl, Ho, Wo, need_dx=False).to(torch.float16)
                x_b0 = self._blocks(tape, h, 0, rng, mode, stem_bn)
            else:
                # recorded first, replayed last: block 0's depthwise pass hands back the gradient of the raw half stem output (already
                # through the stem's eval BatchNorm + swish), the cast makes it fp32 and ud_stem_dgrad completes x.grad
                h32 = T.conv_dense(tape, x_pix, bb._conv_stem.weight, 2, pt, pl, Ho, Wo, need_dx=False, x_planes=x_in)
                h = T.cast(tape, h32, torch.float16)
                x_b0 = self._blocks(tape, h, 0, rng, mode, MB.LazyInput(stem_bn, lambda dh, h=h: tape.add_grad(h, dh)))
        else:
            # an InferenceRunner's fp32 forward (unidefense_amd/infer.py) takes the eval node where it pays; else the operators
            node = tape is None and not self.training and self.__dict__.get("_eval_fused")
            mode = MB.TrunkMode(MB.EVAL_NODE if node else MB.OPERATORS, wts)
            h = T.conv_dense(tape, x_pix, bb._conv_stem.weight, 2, pt, pl, Ho, Wo, need_dx=False, x_planes=x_in)
            h = self._bn(tape, h, bb._bn0, 1)
            x_b0 = self._blocks(tape, h, 0, rng, mode)
        x_b1 = self._blocks(tape, x_b0, 1, rng, mode)
        x_b2 = self._blocks(tape, x_b1, 2, rng, mode)
        x_b3 = self._blocks(tape, x_b2, 3, rng, mode)
        x_b4h = self._blocks(tape, x_b3, 4, rng, mode)
        x_b4 = T.cast(tape, x_b4h, f32)

        d_in = x_b4
        # F.dropout(x_b4, 0.2), unidefense.py:213 (hard-coded rate; `_dec_dropout = False` lets a test switch the
        # only draw that drop_rate = 0 / drop_connect_rate = 0 leave, to compare two executions bit for bit)
        if self.training and getattr(self, "_dec_dropout", True):
            d_in = T.dropout_mask(tape, x_b4, self._keep_mask(rng, "dec_keep", x_b4, 0.8), 0.2)
        # the reconstruction branch (decoder -> rec -> spatial / frequency loss terms, unidefense.py:214-216, 244-253)
        dec1 = self._decoder(tape, d_in, self.dec_block1, False)
        dec2 = self._decoder(tape, dec1, self.dec_block2, False)
        dec3_pix = self._decoder(tape, dec2, self.dec_block3, True)
        dec3 = T.tanh_to_planes(tape, dec3_pix)                          # [N,3,128,128]
        t1 = T.mean_hw(tape, dec1)
        t2 = T.mean_hw(tape, dec2)
        rec = T.bilinear(tape, dec3, H, W)
        spatial, freq = T.rec_losses(tape, rec, x, self.freq_norm)

        x_b5 = T.cast(tape, self._blocks(tape, x_b4h, 5, rng, mode), f32)
        att, freq_mask, spat_mask = self._attention(tape, dec3, x, x_b5, rng)
        x_b6 = T.cast(tape, self._blocks(tape, T.cast(tape, att, torch.float16) if st16 else att, 6, rng, mode), f32)

        h = T.conv1x1(tape, x_b6, bb._conv_head.weight)
        h = self._bn(tape, h, bb._bn1, 1)
        pooled = T.mean_hw(tape, h)                                      # [N,1792]
        feat = self._bn(tape, pooled, self.bottleneck, 0)
        if self.training and self.drop_rate > 0:
            # in-place dropout in the reference: 'factorization' aliases the dropped tensor (:229-230)
            feat = T.dropout_mask(tape, feat, self._keep_mask(rng, "feat_keep", feat, 1.0 - self.drop_rate),
                                  self.drop_rate)
        cls_out = T.linear(tape, feat, self.classifier.fc.weight, self.classifier.fc.bias)

        t0 = T.mean_hw(tape, x_b4)
        return {"cls_out": cls_out, "rec": rec, "factorization": feat, "triplet0": t0, "triplet1": t1,
                "triplet2": t2, "freq_mask": freq_mask, "spat_mask": spat_mask,
                "spatial": spatial, "freq": freq,
                "_feats": {"x_b0": x_b0, "x_b1": x_b1, "x_b2": x_b2, "x_b3": x_b3, "x_b4": x_b4, "x_b5": x_b5,
                           "dec1": dec1, "dec2": dec2, "dec3": dec3, "att_out": att, "x_b6": x_b6,
                           "pooled": pooled}}

"""Graph-replayed input gradients and FGSM / PGD attacks on a frozen eval-mode detector: InputGradRunner, AttackRunner.

Both follow InferenceRunner's life cycle (unidefense_amd/infer.py): call 1 runs eagerly (it settles the on-line GEMM tuner and
every lazily made workspace of the forward AND the backward for the shape), call 2 captures one hipGraph on static buffers,
later calls copy the inputs in and replay.  The captured work is `autograd.grad(objective(model(x_buf), y_buf), x_buf)` on the
eval-mode model with every parameter frozen for the duration of the warm-up and the capture, so the backward is the tape's
frozen sequence (Tape.wgrad_on = False: no weight-gradient launch, no parameter gets a .grad).  K.begin_forward runs inside the
graph and every BatchNorm reads its running buffers in place, so a runner captured before an optimizer step, a load_state_dict
or a change of running statistics differentiates the updated model.

AttackRunner's graph holds ONE iteration — forward on the static leaf x_adv, objective, d/dx, and the step written into x_adv in
place by csrc/attack.hip (L-infinity: one launch; L2: norm, step, norm, projection) — and a call replays it `steps` times.

precision="fp16" (UDEB4 only; runner-scoped like InferenceRunner's): the MBConv trunk's forward AND backward in half storage —
every block is one tape node (tape.mbconv_frozen_half) whose forward is the fp16 InferenceRunner's (runner.out is bitwise that
runner's output) and whose backward goes through the eval-form BatchNorms as per-channel constants (csrc: ud_bn_eval_bwd,
ud_coldot_bn_eval, ud_se_scale_bwd_bn_eval, ud_dwtile_dgrad_eval; the training-form backward entry points keep refusing the eval
form).  The stem's data gradient, decoder, attention, head and objective stay fp32.  The objective is multiplied by grad_scale (a
power of two, default 1024: 99.95 % of the unscaled x-gradient's entries lie below fp16's smallest normal) before the backward and
the fp32 result divided by it inside the graph: runner.g is unscaled; a non-finite gradient stays non-finite.  The eager
model(x), the fp32 runners and the training step do not change.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from .infer import _MAX_RUNNERS, _check_precision, _eval_nodes

DEFAULT_GRAD_SCALE = 1024.0          # fp16 runners: the loss scale of the half-storage training tests

NORMS = ("linf", "l2")
OBJECTIVES = ("cross_entropy",)


def cross_entropy_sum(out, y):
    """The default objective: the SUM over the batch of each sample's classification loss (softmax cross-entropy for
    num_classes >= 2, binary cross-entropy on the single logit for num_classes == 1).  A sum, not a mean: each sample's
    gradient is then that of its own loss, whoever else is in the batch."""
    cls = out["cls_out"]
    if cls.shape[1] == 1:
        return F.binary_cross_entropy_with_logits(cls.squeeze(1), y.to(cls.dtype), reduction="sum")
    return F.cross_entropy(cls, y, reduction="sum")


def _objective(objective):
    if callable(objective):
        return objective
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES} or a callable (out, y) -> scalar, got {objective!r}")
    return cross_entropy_sum


@contextlib.contextmanager
def frozen(model):
    """Every parameter's requires_grad off inside, each parameter's own flag back on exit (also on an exception)."""
    flags = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)


def resolve_grad_scale(precision, grad_scale):
    """The factor on the objective: fp32 takes none (None or 1); fp16: a power of two > 0, DEFAULT_GRAD_SCALE when None."""
    if precision != "fp16":
        if grad_scale is not None and float(grad_scale) != 1.0:
            raise ValueError(f"grad_scale is the fp16 runners' loss scale: precision 'fp32' takes None or 1, got {grad_scale!r}")
        return 1.0
    if grad_scale is None:
        return DEFAULT_GRAD_SCALE
    g = float(grad_scale)
    if not (g > 0.0 and g != float("inf") and math.frexp(g)[0] == 0.5):
        raise ValueError(f"grad_scale must be a power of two > 0, got {grad_scale!r}")
    return g


def _detached(o):
    if isinstance(o, torch.Tensor):
        return o.detach()
    if isinstance(o, dict):
        return {k: _detached(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_detached(v) for v in o)
    return o


def resolve_step(eps, steps, step=None):
    """step=None: eps for one step (FGSM), 2.5 eps / steps otherwise"""
    if step is not None:
        return float(step)
    return float(eps) if steps == 1 else 2.5 * float(eps) / steps


class _GradRunnerBase:
    _what = "runner"

    def _init_model(self, model, batch, size, objective, precision="fp32", grad_scale=None):
        from .model import MODEL
        if not isinstance(model, tuple(MODEL.values())):
            raise ValueError(f"{self._what} takes a UDEB4 / UDR18 / UDR50 model, got {type(model).__name__}")
        _check_precision(model, precision)
        self.precision, self.half = precision, precision == "fp16"
        self.grad_scale = resolve_grad_scale(precision, grad_scale)
        self.objective = _objective(objective)
        if model.training:
            raise ValueError(f"{self._what} needs model.eval(): the captured forward reads the running statistics")
        p = next(model.parameters())
        if not p.is_cuda:
            raise ValueError(f"{self._what} needs a cuda model")
        self.model, self.batch, self.size = model, int(batch), int(size)
        self.shape = (self.batch, 3, self.size, self.size)
        self.device = p.device
        self.calls = 0
        self.graph = self.out = self.g = None

    def _check(self, x, y):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or not isinstance(y, torch.Tensor) or not y.is_cuda:
            raise ValueError(f"{self._what} takes cuda tensors")
        if tuple(x.shape) != self.shape or x.dtype != torch.float32:
            raise ValueError(f"input {tuple(x.shape)} {x.dtype} differs from the runner's key {self.shape} torch.float32")
        if tuple(y.shape) != (self.batch,) or y.dtype != torch.int64:
            raise ValueError(f"labels {tuple(y.shape)} {y.dtype} differ from the runner's key ({self.batch},) torch.int64")
        if self.model.training:
            raise ValueError("the model is in training mode: call model.eval() before the runner")

    def _grad(self, x, y):
        """forward + objective + d/dx on the leaf x: (gradient, detached output dict)"""
        if not self.half:
            out = self.model(x)
            g, = torch.autograd.grad(self.objective(out, y), x)
            return g, _detached(out)
        # fp16: the trunk's frozen half nodes (runner-scoped flag); the scaled objective keeps the half gradients off fp16's
        # subnormals, the fp32 result is unscaled in place (inside the graph when capturing)
        from . import kernels as K
        with _eval_nodes(self.model, half=True):
            out = self.model(x)
            g, = torch.autograd.grad(self.objective(out, y) * self.grad_scale, x)
        g = g.contiguous()
        return K.axpby(g, 1.0 / self.grad_scale, out=g), _detached(out)


class InputGradRunner(_GradRunnerBase):
    """runner = InputGradRunner(model, batch, size[, objective]); g = runner(x, y) with x [batch, 3, size, size] fp32 and y
    [batch] int64 on the model's GPU: the gradient of objective(model(x), y) with respect to x for the frozen eval-mode model.
    g and runner.out (the forward's output dict, detached) live in static buffers that the next call overwrites.
    objective: "cross_entropy" (cross_entropy_sum) or a callable (out, y) -> scalar that the caller guarantees capturable.
    precision: "fp32" or "fp16" (UDEB4: the trunk's forward and frozen backward in half storage); grad_scale: fp16's loss scale,
    a power of two (None: 1024); g is unscaled either way."""
    _what = "InputGradRunner"

    def __init__(self, model, batch, size, objective="cross_entropy", precision="fp32", grad_scale=None):
        self._init_model(model, batch, size, objective, precision, grad_scale)
        self.x = self.y = None

    def __call__(self, x, y):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up of what the graph records
                with frozen(self.model):
                    self.g, self.out = self._grad(x.detach().clone().contiguous().requires_grad_(), y)
                return self.g
            if self.graph is None:
                self.x = x.detach().clone().contiguous().requires_grad_()
                self.y = y.detach().clone()
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with frozen(self.model), torch.cuda.graph(g):
                    self.g, self.out = self._grad(self.x, self.y)
                self.graph = g
            else:
                with torch.no_grad():
                    self.x.copy_(x)
                    self.y.copy_(y)
        self.graph.replay()
        return self.g


class AttackRunner(_GradRunnerBase):
    """runner = AttackRunner(model, batch, size, norm="linf", eps=..., steps=10, ...); x_adv = runner(x, y[, generator]).

    `steps` iterations of  x_adv <- project(x_adv + step * direction(d objective / d x_adv))  from x_adv = x, ascending the
    objective of the true labels y (targeted=True: descending it towards the labels y):
      norm "linf": direction = sign, projection onto |x_adv - x|_inf <= eps, then onto clip;
      norm "l2"  : direction = g / |g|_2 per sample, projection onto |x_adv - x|_2 <= eps per sample, then onto clip.
    step=None: eps for steps == 1 (FGSM), 2.5 eps / steps otherwise.  random_start (linf only): x_adv starts at
    clamp(x + U(-eps, eps), clip), drawn outside the graph with torch's generator (`generator=` makes it reproducible).
    eps, step, clip and the norm are kernel arguments inside the graph: fixed per runner.  eps is in model-input units.
    x_adv and runner.g (the last iteration's gradient, taken at the x_adv BEFORE that iteration's step) are static buffers
    that the next call overwrites; runner.args holds the resolved arguments.  precision / grad_scale: as InputGradRunner."""
    _what = "AttackRunner"

    def __init__(self, model, batch, size, norm="linf", eps=None, steps=10, step=None, random_start=False, targeted=False,
                 clip=(-1.0, 1.0), objective="cross_entropy", precision="fp32", grad_scale=None):
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")
        if eps is None or not float(eps) >= 0.0:
            raise ValueError(f"eps must be >= 0, got {eps!r}")
        if int(steps) != steps or steps < 1:
            raise ValueError(f"steps must be an integer >= 1, got {steps!r}")
        if len(clip) != 2 or not float(clip[0]) < float(clip[1]):
            raise ValueError(f"clip must be (lo, hi) with lo < hi, got {clip!r}")
        if norm == "l2" and random_start:
            raise ValueError("random_start is built for norm 'linf' only")
        self._init_model(model, batch, size, objective, precision, grad_scale)
        self.norm, self.eps, self.steps = norm, float(eps), int(steps)
        self.step = resolve_step(eps, self.steps, step)
        self.random_start, self.targeted = bool(random_start), bool(targeted)
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.args = {"norm": norm, "eps": self.eps, "steps": self.steps, "step": self.step, "random_start": self.random_start,
                     "targeted": self.targeted, "clip": (self.lo, self.hi),
                     "objective": objective if isinstance(objective, str) else getattr(objective, "__name__", repr(objective)),
                     "precision": self.precision, "grad_scale": self.grad_scale}
        self.x0 = self.x_adv = self.y = self._ss = self._ws = None

    def _buffers(self, x, y):
        from . import kernels as K
        self.x0 = x.detach().clone().contiguous()
        self.x_adv = self.x0.clone().requires_grad_()
        self.y = y.detach().clone()
        if self.norm == "l2":
            per = 3 * self.size * self.size
            self._ss = torch.zeros(self.batch, dtype=torch.float64, device=self.device)
            self._ws = torch.zeros(max(K.sample_sumsq_ws_bytes(self.batch, per) // 8, 1), dtype=torch.float64, device=self.device)

    def _iteration(self):
        """one attack iteration on the static buffers: what the graph holds"""
        from . import kernels as K
        self.g, self.out = self._grad(self.x_adv, self.y)
        g = self.g.contiguous()
        signed = -self.step if self.targeted else self.step
        if self.norm == "linf":
            K.attack_step_linf(self.x_adv, self.x0, g, signed, self.eps, self.lo, self.hi)
        else:
            K.sample_sumsq(g, None, out=self._ss, ws=self._ws)
            K.attack_step_l2(self.x_adv, g, self._ss, signed)
            K.sample_sumsq(self.x_adv, self.x0, out=self._ss, ws=self._ws)
            K.attack_project_l2(self.x_adv, self.x0, self._ss, self.eps, self.lo, self.hi)

    def _start(self, x, y, generator):
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            if self.random_start:
                gdev = generator.device if generator is not None else self.device
                u = torch.rand(self.shape, generator=generator, device=gdev, dtype=torch.float32).to(self.device)
                self.x_adv.copy_((x + (u * 2.0 - 1.0) * self.eps).clamp_(self.lo, self.hi))
            else:
                self.x_adv.copy_(x)

    def __call__(self, x, y, generator=None):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up: the same iterations, a valid attack
                self._buffers(x, y)
                self._start(x, y, generator)
                with frozen(self.model):
                    for _ in range(self.steps):
                        self._iteration()
                return self.x_adv.detach()
            if self.graph is None:
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with frozen(self.model), torch.cuda.graph(g):
                    self._iteration()
                self.graph = g
            self._start(x, y, generator)
        for _ in range(self.steps):
            self.graph.replay()
        return self.x_adv.detach()


def _cached(model, slot, key, make):
    runners = model.__dict__.setdefault(slot, {})
    r = runners.pop(key, None)
    if r is None:
        r = make()
        while len(runners) >= _MAX_RUNNERS:
            del runners[next(iter(runners))]
    runners[key] = r                                 # most recently used last
    return r


def _precision_key(key, precision, grad_scale):
    """an fp32 runner's key is what it was before the runners took a precision; an fp16 runner's carries (precision, scale)"""
    return key if precision == "fp32" else key + (precision, resolve_grad_scale(precision, grad_scale))


def input_grad_key(batch, size, objective="cross_entropy", precision="fp32", grad_scale=None):
    return _precision_key((int(batch), int(size), objective), precision, grad_scale)


def attack_key(batch, size, norm="linf", eps=None, steps=10, step=None, random_start=False, targeted=False,
               clip=(-1.0, 1.0), objective="cross_entropy", precision="fp32", grad_scale=None):
    return _precision_key((int(batch), int(size), norm, eps, steps, step, bool(random_start), bool(targeted), tuple(clip),
                           objective), precision, grad_scale)


def input_grad_runner(model, batch, size, objective="cross_entropy", precision="fp32", grad_scale=None):
    """The model's InputGradRunner for the full argument tuple, made on first use; a model keeps at most _MAX_RUNNERS of them
    (a dictionary of their own: InferenceRunner's cache and keys are untouched)."""
    _check_precision(model, precision)
    key = input_grad_key(batch, size, objective, precision, grad_scale)
    return _cached(model, "_ud_grad_runners", key,
                   lambda: InputGradRunner(model, batch, size, objective, precision, grad_scale))


def attack_runner(model, batch, size, norm="linf", eps=None, steps=10, step=None, random_start=False, targeted=False,
                  clip=(-1.0, 1.0), objective="cross_entropy", precision="fp32", grad_scale=None):
    """The model's AttackRunner for the full argument tuple, made on first use; at most _MAX_RUNNERS are kept."""
    _check_precision(model, precision)
    key = attack_key(batch, size, norm, eps, steps, step, random_start, targeted, clip, objective, precision, grad_scale)
    return _cached(model, "_ud_attack_runners", key,
                   lambda: AttackRunner(model, batch, size, norm, eps, steps, step, random_start, targeted, clip, objective,
                                        precision, grad_scale))

"""Graph-replayed input gradients and FGSM / PGD / Auto-PGD / Square / FMN / sparse FMN attacks on a frozen eval-mode detector:
InputGradRunner, AttackRunner, APGDRunner, SquareRunner, FMNRunner, SparseFMNRunner.

All six sit on one base class (_Runner) and follow InferenceRunner's life cycle (unidefense_amd/infer.py): call 1 runs eagerly
(it settles the on-line GEMM tuner and every lazily made workspace of the forward AND the backward for the shape), call 2
captures the runner's iteration on static buffers (_Runner._capture), later calls copy the inputs in and replay.  An attack's
defaults are written once, in its class's signature: the *_key and *_runner accessors bind their arguments with it.

The gradient runners capture `autograd.grad(objective(model(x_buf), y_buf), x_buf)` (_Runner._grad) on the eval-mode model with
every parameter frozen for the duration of the warm-up and the capture, so the backward is the tape's frozen sequence
(Tape.wgrad_on = False: no weight-gradient launch, no parameter gets a .grad).  K.begin_forward runs inside the graph and every
BatchNorm reads its running buffers in place, so a runner captured before an optimizer step, a load_state_dict or a change of
running statistics differentiates the updated model.

AttackRunner's graph holds ONE iteration — forward on the static leaf x_adv, objective, d/dx, and the step written into x_adv in
place by csrc/attack.hip (L-infinity: one launch; L2: norm, step, norm, projection) — and a call replays it `steps` times.

precision="fp16" (UDEB4 only; runner-scoped like InferenceRunner's): the MBConv trunk's forward AND backward in half storage —
every block is one tape node (mbconv.mbconv_frozen_half) whose forward is the fp16 InferenceRunner's (runner.out is bitwise that
runner's output) and whose backward goes through the eval-form BatchNorms as per-channel constants (csrc: ud_bn_eval_bwd,
ud_coldot_bn_eval, ud_se_scale_bwd_bn_eval, ud_dwtile_dgrad_eval; the training-form backward entry points keep refusing the eval
form).  The stem's data gradient, decoder, attention, head and objective stay fp32.  The objective is multiplied by grad_scale (a
power of two, default 1024: 99.95 % of the unscaled x-gradient's entries lie below fp16's smallest normal) before the backward and
the fp32 result divided by it inside the graph: runner.g is unscaled; a non-finite gradient stays non-finite.  The eager
model(x), the fp32 runners and the training step do not change.

APGDRunner (Auto-PGD, APGD-CE): its graph holds one iteration whose per-sample control — which samples improved, whose step size
is halved, who restarts from their best point — is device state written by csrc/apgd.hip (ud_apgd_control: one thread per
sample; ud_apgd_update_linf: one pass), plus a forward-only graph that scores the last point; the best point per sample over all
iterations and restarts is returned.

SquareRunner (Square Attack, L-infinity, as in AutoAttack) is the black-box member: it needs the forward only — InferenceRunner's,
in either precision — and no gradient, so it cross-checks the gradient attacks above, which all differentiate the same frozen
backward.  Its graph holds one query: csrc/square.hip's ud_square_propose (settle the last proposal's window, write the next),
the forward, the per-sample objective and ud_square_control (keep or undo, who is still searched); every random choice is drawn by
torch outside the graph (square_draws) into device tables that the kernels index with the sample's own counter.

FMNRunner (Fast Minimum-Norm attack, linf and l2) is the minimum-norm member: where the others ask how far the loss rises at a
budget chosen in advance, it returns per sample the smallest perturbation that flips it (radius), so ONE run gives the robust
accuracy at every eps (robust_curve).  Its graph holds one iteration whose per-sample budget adapts on the device
(csrc/fmn.hip: ud_fmn_norm_parts, the four norms of the iteration in one streaming pass; ud_fmn_control, one thread per sample;
ud_fmn_update, step + projection in one pass), plus a forward-only closing graph; the step and shrink schedules
(fmn_schedule) are device tables that the control kernel indexes with the sample's own counter.

SparseFMNRunner (l1 and l0) is FMNRunner's sibling for the sparse threat models — a sticker, a retouched patch, a few edited
pixels: radius is sum |x_adv - x| or the number of changed elements.  The two share their body (_MinNormRunner); what differs is
the norm pass and control rules (csrc/sfmn.hip: ud_sfmn_norm_parts, ud_sfmn_control) and the projection, which needs a
per-sample selection over all 3 size^2 elements inside the graph: ud_sfmn_select (one workgroup per sample: the L1 ball's soft
threshold by a fixed-count bisection with sums in double, the L0 threshold by a radix select on integer counts) and
ud_sfmn_apply (one pass).  FMNRunner, ud_fmn_* and its norms are unchanged.
"""
import contextlib
import gc
import inspect
import math

import torch
import torch.nn.functional as F

from .infer import _MAX_RUNNERS, _check_model, _check_precision, _eval_nodes

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


# ---- argument refusals: each written once, raised by the constructors in their own order -------------------------------------
def _refuse_norm(norm):
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")


def _refuse_eps(eps):
    if eps is None or not float(eps) >= 0.0:
        raise ValueError(f"eps must be >= 0, got {eps!r}")


def _refuse_count(name, v, least):
    if not v >= least or int(v) != v:
        raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")


def _refuse_fraction(name, v):
    if not 0.0 < float(v) <= 1.0:
        raise ValueError(f"{name} must be in (0, 1], got {v!r}")


def _refuse_clip(clip):
    if len(clip) != 2 or not float(clip[0]) < float(clip[1]):
        raise ValueError(f"clip must be (lo, hi) with lo < hi, got {clip!r}")


def _objective_name(objective):
    return objective if isinstance(objective, str) else getattr(objective, "__name__", repr(objective))


class _Runner:
    """What the six runners share: the model checks, the input checks, the capture, the forward + d/dx with fp16's loss scale,
    and the per-sample pieces of the attacks with restarts."""
    _what = "runner"
    _backward = True                     # the captured work differentiates: the parameters are frozen around it

    def _init_model(self, model, batch, size, precision, arguments):
        """The one place a runner looks at its model: its kind and the precision; then arguments(), the runner's own refusals,
        which need no device; then eval mode and the device."""
        self.precision, self.half = precision, precision == "fp16"
        self.device = _check_model(self._what, model, precision, arguments)
        self.model, self.batch, self.size = model, int(batch), int(size)
        self.shape = (self.batch, 3, self.size, self.size)
        self.calls = 0
        self.graph = self.out = None

    def _init_loss(self, objective, grad_scale):
        """the gradient runners' arguments(): the loss scale and the objective"""
        self.grad_scale = resolve_grad_scale(self.precision, grad_scale)
        self.objective = _objective(objective)
        self.g = None

    def _check(self, x, y):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or not isinstance(y, torch.Tensor) or not y.is_cuda:
            raise ValueError(f"{self._what} takes cuda tensors")
        if tuple(x.shape) != self.shape or x.dtype != torch.float32:
            raise ValueError(f"input {tuple(x.shape)} {x.dtype} differs from the runner's key {self.shape} torch.float32")
        if tuple(y.shape) != (self.batch,) or y.dtype != torch.int64:
            raise ValueError(f"labels {tuple(y.shape)} {y.dtype} differ from the runner's key ({self.batch},) torch.int64")
        if self.model.training:
            raise ValueError("the model is in training mode: call model.eval() before the runner")

    def _capture(self, *bodies):
        """One hipGraph per body, captured in order on the static buffers after a device synchronise, the parameters frozen
        where the runner has a backward: the graphs."""
        torch.cuda.synchronize(self.device)
        graphs = [torch.cuda.CUDAGraph() for _ in bodies]
        # the cyclic collector must not run inside a capture: it would destroy whatever unreachable graphs, events and device
        # buffers earlier runners or models left behind, and a device call of a destructor is illegal while a stream captures
        # in the global error mode (the process aborts).  torch.cuda.graph collects once on entry; nothing may collect after it.
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with frozen(self.model) if self._backward else contextlib.nullcontext():
                for g, body in zip(graphs, bodies):
                    with torch.cuda.graph(g):
                        body()
        finally:
            if gc_was_on:
                gc.enable()
        return graphs

    def _nodes(self):
        return _eval_nodes(self.model, half=True) if self.half else contextlib.nullcontext()

    def _grad(self, x, value):
        """forward on the leaf x, f = value(out) (a scalar, or one value per sample: their sum is differentiated), d/dx:
        (gradient, detached output dict, f).  fp16: the trunk's frozen half nodes (runner-scoped flag); the scaled objective
        keeps the half gradients off fp16's subnormals, the fp32 result is unscaled in place (inside the graph when capturing)."""
        from . import kernels as K
        with self._nodes():
            out = self.model(x)
            f = value(out)
            total = f if f.dim() == 0 else f.sum()
            g, = torch.autograd.grad(total * self.grad_scale if self.half else total, x)
        if self.half:
            g = g.contiguous()
            K.axpby(g, 1.0 / self.grad_scale, out=g)
        return g, _detached(out), f

    def _each(self, out):
        """the per-sample objective on the static labels, [batch]"""
        f = self.objective(out, self.y)
        if not isinstance(f, torch.Tensor) or tuple(f.shape) != (self.batch,):
            raise ValueError(f"{self._what}'s objective must return a [{self.batch}] tensor, one value per sample, got "
                             f"{tuple(f.shape) if isinstance(f, torch.Tensor) else type(f).__name__}")
        return f

    def _draw(self, sample, generator):
        """sample = torch.rand / torch.randn of the input's shape, drawn on the generator's device"""
        gdev = generator.device if generator is not None else self.device
        return sample(self.shape, generator=generator, device=gdev, dtype=torch.float32).to(self.device)

    def _box_start(self, x, generator):
        """clamp(x + U(-eps, eps), clip)"""
        return (x + (self._draw(torch.rand, generator) * 2.0 - 1.0) * self.eps).clamp_(self.lo, self.hi)

    def _merge(self, restart, better):
        """the per-sample best of f_best over the restarts so far, outside the graph; better: torch.gt where f is maximised,
        torch.lt where it is minimised"""
        from . import kernels as K
        with torch.no_grad():
            if restart == 0:
                self.loss0.copy_(self.history[0])
                self.x_adv.copy_(self.x_best)
                self.best_loss.copy_(self._f_best)
            else:
                keep = better(self._f_best, self.best_loss).to(torch.int32)
                K.apgd_keep(self.x_adv, self.x_best, keep)
                self.best_loss.copy_(torch.where(keep.bool(), self._f_best, self.best_loss))


class InputGradRunner(_Runner):
    """runner = InputGradRunner(model, batch, size[, objective]); g = runner(x, y) with x [batch, 3, size, size] fp32 and y
    [batch] int64 on the model's GPU: the gradient of objective(model(x), y) with respect to x for the frozen eval-mode model.
    g and runner.out (the forward's output dict, detached) live in static buffers that the next call overwrites.
    objective: "cross_entropy" (cross_entropy_sum) or a callable (out, y) -> scalar that the caller guarantees capturable.
    precision: "fp32" or "fp16" (UDEB4: the trunk's forward and frozen backward in half storage); grad_scale: fp16's loss scale,
    a power of two (None: 1024); g is unscaled either way."""
    _what = "InputGradRunner"

    def __init__(self, model, batch, size, objective="cross_entropy", precision="fp32", grad_scale=None):
        self._init_model(model, batch, size, precision, lambda: self._init_loss(objective, grad_scale))
        self.x = self.y = None

    def _iteration(self, x, y):
        self.g, self.out, _ = self._grad(x, lambda out: self.objective(out, y))

    def __call__(self, x, y):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up of what the graph records
                with frozen(self.model):
                    self._iteration(x.detach().clone().contiguous().requires_grad_(), y)
                return self.g
            if self.graph is None:
                self.x = x.detach().clone().contiguous().requires_grad_()
                self.y = y.detach().clone()
                self.graph, = self._capture(lambda: self._iteration(self.x, self.y))
            else:
                with torch.no_grad():
                    self.x.copy_(x)
                    self.y.copy_(y)
        self.graph.replay()
        return self.g


class AttackRunner(_Runner):
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
        _refuse_norm(norm)
        _refuse_eps(eps)
        _refuse_count("steps", steps, 1)
        _refuse_clip(clip)
        if norm == "l2" and random_start:
            raise ValueError("random_start is built for norm 'linf' only")
        self._init_model(model, batch, size, precision, lambda: self._init_loss(objective, grad_scale))
        self.norm, self.eps, self.steps = norm, float(eps), int(steps)
        self.step = resolve_step(eps, self.steps, step)
        self.random_start, self.targeted = bool(random_start), bool(targeted)
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.args = {"norm": norm, "eps": self.eps, "steps": self.steps, "step": self.step, "random_start": self.random_start,
                     "targeted": self.targeted, "clip": (self.lo, self.hi), "objective": _objective_name(objective),
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
        self.g, self.out, _ = self._grad(self.x_adv, lambda out: self.objective(out, self.y))
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
            self.x_adv.copy_(self._box_start(x, generator) if self.random_start else x)

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
                self.graph, = self._capture(self._iteration)
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


def _arguments(cls):
    """cls's (batch, size, ...) bound as its constructor binds them, defaults filled in, as a name -> value dict in the
    constructor's order: the class's signature is the one place an attack's defaults are written"""
    sig = inspect.signature(cls.__init__)

    def bind(*args, **kwargs):
        b = sig.bind(None, None, *args, **kwargs)
        b.apply_defaults()
        return dict(list(b.arguments.items())[2:])
    return bind


_KEY_FORMS = {"batch": int, "size": int, "random_start": bool, "targeted": bool, "early_stop": bool, "clip": tuple}


def _key(a):
    """The cache key of the bound arguments a: an fp32 runner's is the arguments before the precision; an fp16 runner's carries
    (precision, scale) behind them, or (precision,) where the runner has no loss scale."""
    key = tuple(_KEY_FORMS.get(k, lambda v: v)(v) for k, v in a.items() if k not in ("precision", "grad_scale"))
    precision = a["precision"]
    if precision == "fp32":
        return key
    return key + ((precision, resolve_grad_scale(precision, a["grad_scale"])) if "grad_scale" in a else (precision,))


def _cached_runner(model, slot, a, make):
    _check_precision(model, a["precision"])
    return _cached(model, slot, _key(a), make)


_input_grad_arguments, _attack_arguments = _arguments(InputGradRunner), _arguments(AttackRunner)


def input_grad_key(*args, **kwargs):
    """arguments: InputGradRunner's after the model"""
    return _key(_input_grad_arguments(*args, **kwargs))


def attack_key(*args, **kwargs):
    """arguments: AttackRunner's after the model"""
    return _key(_attack_arguments(*args, **kwargs))


def input_grad_runner(model, *args, **kwargs):
    """The model's InputGradRunner for the full argument tuple (InputGradRunner's after the model), made on first use; a model
    keeps at most _MAX_RUNNERS of them (a dictionary of their own: InferenceRunner's cache and keys are untouched)."""
    a = _input_grad_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_grad_runners", a, lambda: InputGradRunner(model, *a.values()))


def attack_runner(model, *args, **kwargs):
    """The model's AttackRunner for the full argument tuple (AttackRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept."""
    a = _attack_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_attack_runners", a, lambda: AttackRunner(model, *a.values()))


# ---- Auto-PGD (APGD-CE, Croce & Hein 2020): per-sample step control, restarts from the best point, best-of ----------------------
_APGD_P1 = 22                        # hundredths of `steps`: the first checkpoint; the gaps shrink by 3 down to 6


def apgd_checkpoints(steps):
    """The checkpoint iterations for `steps` iterations, in integer arithmetic: p_0 = 0, p_1 = 22, p_{j+1} = p_j +
    max(p_j - p_{j-1} - 3, 6) hundredths; w_j = ceil(p_j steps / 100), deduplicated, those in [1, steps - 1]."""
    steps = int(steps)
    out, prev, p = [], 0, _APGD_P1
    while True:
        w = (p * steps + 99) // 100
        if w > steps - 1:
            return tuple(out)
        if w >= 1 and (not out or w != out[-1]):
            out.append(w)
        prev, p = p, p + max(p - prev - 3, 6)


def apgd_table(steps, rho):
    """(checkpoints, thresholds): checkpoint w_j's window is L_j = w_j - w_{j-1} (w_0 = 0) and its first condition
    cnt < rho L_j is, for an integer cnt, cnt < ceil(rho L_j): the integer the control kernel compares with."""
    ws = apgd_checkpoints(steps)
    thr = tuple(int(math.ceil(float(rho) * (w - (ws[j - 1] if j else 0)))) for j, w in enumerate(ws))
    return ws, thr


def cross_entropy_each(out, y):
    """cross_entropy_sum's terms: each sample's classification loss, [batch]"""
    cls = out["cls_out"]
    if cls.shape[1] == 1:
        return F.binary_cross_entropy_with_logits(cls.squeeze(1), y.to(cls.dtype), reduction="none")
    return F.cross_entropy(cls, y, reduction="none")


class APGDRunner(_Runner):
    """runner = APGDRunner(model, batch, size, norm="linf", eps=..., steps=100, restarts=1, ...); x_adv = runner(x, y[, generator]).

    Auto-PGD on the per-sample objective f (objective="cross_entropy": each sample's loss; or a callable (out, y) -> [batch];
    targeted=True ascends -f).  Per sample: step size eta = 2 eps, halved at the checkpoints apgd_checkpoints(steps) when f rose
    in fewer than rho of the window's iterations, or when neither eta nor the best f changed since the previous checkpoint; a
    halving restarts the sample from its best point; momentum alpha; direction and projection as AttackRunner's (linf: sign, box,
    clip; l2: g / |g|, ball, clip).  One hipGraph holds ONE iteration — forward, f, d sum(f) / dx, the per-sample control
    (ud_apgd_control: device state, no host round trip) and the update — and a restart replays it `steps` times, then replays
    a forward-only graph that scores the last point.  Restart 0 starts at clamp(x, clip) (random_start: at random); every
    later restart starts at random (linf: uniform in the box; l2: on the sphere of radius eps), drawn by torch outside the graph
    from `generator`; the per-sample best over all iterations and restarts is kept.

    Static buffers that the next call overwrites: x_adv (returned), best_loss [N] (f at x_adv), loss0 [N] (f at restart 0's
    start), eta [N] and history [steps + 1, N] (step sizes and f_k of the LAST restart; history[steps] is the closing
    evaluation), g (the last iteration's gradient), out (the last iteration's forward output); args: the resolved arguments.
    precision / grad_scale: as InputGradRunner."""
    _what = "APGDRunner"

    def __init__(self, model, batch, size, norm="linf", eps=None, steps=100, restarts=1, random_start=False, rho=0.75, alpha=0.75,
                 targeted=False, clip=(-1.0, 1.0), objective="cross_entropy", precision="fp32", grad_scale=None):
        _refuse_norm(norm)
        _refuse_eps(eps)
        _refuse_count("steps", steps, 1)
        _refuse_count("restarts", restarts, 1)
        _refuse_fraction("rho", rho)
        _refuse_fraction("alpha", alpha)
        _refuse_clip(clip)
        self._init_model(model, batch, size, precision, lambda: self._init_loss(objective, grad_scale))
        self.objective = objective if callable(objective) else cross_entropy_each
        self.norm, self.eps, self.steps, self.restarts = norm, float(eps), int(steps), int(restarts)
        self.random_start, self.targeted = bool(random_start), bool(targeted)
        self.rho, self.alpha = float(rho), float(alpha)
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.checkpoints, self._thr = apgd_table(self.steps, self.rho)
        self.args = {"method": "apgd", "norm": norm, "eps": self.eps, "steps": self.steps, "restarts": self.restarts,
                     "random_start": self.random_start, "rho": self.rho, "alpha": self.alpha, "targeted": self.targeted,
                     "clip": (self.lo, self.hi), "objective": _objective_name(objective),
                     "precision": self.precision, "grad_scale": self.grad_scale}
        self.closing_graph = None
        self.x0 = self.x = self.x_adv = self.y = None

    def _buffers(self, x, y):
        from . import kernels as K
        n, dev = self.batch, self.device
        self.x0 = x.detach().clone().contiguous()
        self.x = self.x0.clone().requires_grad_()                 # the static leaf: the current iterate
        self.x_prev, self.x_best, self.g_best = (torch.zeros_like(self.x0) for _ in range(3))
        self.x_adv = torch.zeros_like(self.x0)
        self.y = y.detach().clone()
        self.ist, self.fst = K.apgd_state(n, dev)
        self.history = torch.zeros(self.steps + 1, n, dtype=torch.float32, device=dev)
        self.best_loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.loss0 = torch.zeros(n, dtype=torch.float32, device=dev)
        self.eta = self.fst[K.APGD_F["eta"]]
        self._f_best = self.fst[K.APGD_F["f_best"]]
        self._improved = self.ist[K.APGD_I["improved"]]
        if self.norm == "l2":
            per = 3 * self.size * self.size
            self._z = torch.zeros_like(self.x0)
            self._gss, self._gss_best, self._dss = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3))
            self._ws = torch.zeros(max(K.sample_sumsq_ws_bytes(n, per) // 8, 1), dtype=torch.float64, device=dev)

    def _ascended(self, out):
        f = self._each(out)
        return -f if self.targeted else f

    def _iteration(self):
        """one APGD iteration on the static buffers: what the graph holds"""
        from . import kernels as K
        g, self.out, f = self._grad(self.x, self._ascended)
        self.g = g = g.contiguous()
        K.apgd_control(f.detach().float().contiguous(), self.ist, self.fst, self.history, self.steps, self.checkpoints, self._thr,
                       2.0 * self.eps, self.alpha)
        if self.norm == "linf":
            K.apgd_update_linf(self.x, self.x_prev, self.x_best, self.g_best, self.x0, g, self.ist, self.fst, self.eps, self.lo,
                               self.hi)
        else:
            K.sample_sumsq(g, None, out=self._gss, ws=self._ws)
            K.apgd_step_l2(self.x, self._z, self.x_best, self.g_best, self._gss_best, g, self._gss, self.ist, self.fst)
            K.sample_sumsq(self._z, self.x0, out=self._dss, ws=self._ws)
            K.attack_project_l2(self._z, self.x0, self._dss, self.eps, self.lo, self.hi)
            K.apgd_combine_l2(self.x, self.x_prev, self._z, self.fst)
            K.sample_sumsq(self.x, self.x0, out=self._dss, ws=self._ws)
            K.apgd_project_l2(self.x, self.x0, self._dss, self.fst, self.eps, self.lo, self.hi)

    def _closing(self):
        """the closing evaluation: forward only at the last point; if it beats the best, it becomes the best"""
        from . import kernels as K
        with torch.no_grad(), self._nodes():
            f = self._ascended(self.model(self.x))
        K.apgd_control(f.float().contiguous(), self.ist, self.fst, self.history, self.steps, self.checkpoints, self._thr,
                       2.0 * self.eps, self.alpha, closing=True)
        K.apgd_keep(self.x_best, self.x, self._improved)

    def _start(self, restart, generator):
        """the start point of a restart, drawn outside the graph; the iteration counters back to 0"""
        from . import kernels as K
        with torch.no_grad():
            x0 = self.x0
            if restart == 0 and not self.random_start:
                s = x0.clamp(self.lo, self.hi)
            elif self.norm == "linf":
                s = self._box_start(x0, generator)
            else:
                n = self._draw(torch.randn, generator)
                nrm = n.flatten(1).norm(dim=1).clamp_min(1e-12).view(-1, 1, 1, 1)
                s = (x0 + n * (self.eps / nrm)).clamp_(self.lo, self.hi)
            self.x.copy_(s)
            self.x_prev.copy_(s)
            self.ist[K.APGD_I["k"]].zero_()

    def __call__(self, x, y, generator=None):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up: the same launches, a valid attack
                self._buffers(x, y)
            elif self.graph is None:
                self.graph, self.closing_graph = self._capture(self._iteration, self._closing)
            with torch.no_grad():
                self.x0.copy_(x)
                self.y.copy_(y)
            for r in range(self.restarts):
                self._start(r, generator)
                if self.graph is None:
                    with frozen(self.model):
                        for _ in range(self.steps):
                            self._iteration()
                        self._closing()
                else:
                    for _ in range(self.steps):
                        self.graph.replay()
                    self.closing_graph.replay()
                self._merge(r, torch.gt)
        return self.x_adv


_apgd_arguments = _arguments(APGDRunner)


def apgd_key(*args, **kwargs):
    """arguments: APGDRunner's after the model"""
    return _key(_apgd_arguments(*args, **kwargs))


def apgd_runner(model, *args, **kwargs):
    """The model's APGDRunner for the full argument tuple (APGDRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _apgd_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_apgd_runners", a, lambda: APGDRunner(model, *a.values()))


# ---- Square Attack, L-infinity (Andriushchenko et al. 2020, as AutoAttack runs it): score-based, forward only --------------------
SQUARE_OBJECTIVES = ("margin", "cross_entropy")
_SQUARE_THRESHOLDS = (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)


def square_sizes(steps, size, p_init):
    """The window side s_j of proposal j = 0 .. steps - 1, evaluated by iteration k = j + 1: it = (k 10000) // steps,
    p = p_init / 2^m with m the number of thresholds (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000) that `it` exceeds,
    s = min(max(floor(sqrt(p size^2) + 0.5), 1), size).  Integers and float64 only: the same on any machine."""
    steps, size = int(steps), int(size)
    out = []
    for j in range(steps):
        it = ((j + 1) * 10000) // steps
        m = sum(1 for t in _SQUARE_THRESHOLDS if it > t)
        p = float(p_init) / 2.0 ** m
        out.append(min(max(int(math.floor(math.sqrt(p * size * size) + 0.5)), 1), size))
    return tuple(out)


def square_draws(steps, batch, size, p_init, generator=None):
    """Every random choice of one restart, drawn in this fixed order on the generator's device (None: torch's default CPU
    generator): sign0 [batch, 3, size] (+-1, fp32: the vertical stripes of the start, one sign per channel and column) from
    randint; u_h then u_w [steps, batch] float64 uniforms, h = floor(u_h (size - s_j + 1)) and w likewise (int64, inside
    [0, size - s_j]); sign [steps, batch, 3] (+-1, fp32) from randint.  Returns (sign0, h, w, sign).  A CPU generator with the
    same seed gives the same draws on any machine."""
    steps, batch, size = int(steps), int(batch), int(size)
    dev = generator.device if generator is not None else torch.device("cpu")
    side = torch.tensor(square_sizes(steps, size, p_init), dtype=torch.float64, device=dev).reshape(-1, 1)
    sign0 = torch.randint(0, 2, (batch, 3, size), generator=generator, device=dev).to(torch.float32) * 2.0 - 1.0
    room = size - side + 1.0
    u_h = torch.rand(steps, batch, generator=generator, device=dev, dtype=torch.float64)
    u_w = torch.rand(steps, batch, generator=generator, device=dev, dtype=torch.float64)
    h = torch.minimum(torch.floor(u_h * room), room - 1.0).to(torch.int64)
    w = torch.minimum(torch.floor(u_w * room), room - 1.0).to(torch.int64)
    sign = torch.randint(0, 2, (steps, batch, 3), generator=generator, device=dev).to(torch.float32) * 2.0 - 1.0
    return sign0, h, w, sign


def margin_each(out, y):
    """The margin of the true class, [batch]: z_y - max_{j != y} z_j; with a single logit (2 y - 1) z.  Positive while the sample
    is classified correctly."""
    z = out["cls_out"]
    if z.shape[1] == 1:
        return (2.0 * y.to(z.dtype) - 1.0) * z.squeeze(1)
    idx = y.reshape(-1, 1)
    own = z.gather(1, idx).squeeze(1)
    other = z.scatter(1, idx, float("-inf")).max(1).values
    return own - other


def _neg_cross_entropy_each(out, y):
    return -cross_entropy_each(out, y)


class SquareRunner(_Runner):
    """runner = SquareRunner(model, batch, size, eps=..., steps=5000, ...); x_adv = runner(x, y[, generator]).

    Square Attack in L-infinity on the per-sample objective f, which is MINIMISED (objective="margin": margin_each, the sample is
    fooled once f <= 0; "cross_entropy": minus each sample's loss; or a callable (out, y) -> [batch]).  The start is
    clamp(x + eps sign0, clip) with vertical stripes sign0; proposal j overwrites one s_j x s_j window (square_sizes) at a random
    place with x +- eps per channel, and is kept where f fell below the best so far.  With objective "margin" and early_stop a
    sample is searched (and its queries counted) only while its best f is positive.  One hipGraph holds ONE query — propose,
    forward (InferenceRunner's, under no_grad), f, control — and a restart replays it steps + 1 times, then settles the last
    window; every random choice comes from square_draws(steps, batch, size, p_init, generator) outside the graph.  restarts: each
    takes new draws, the per-sample lowest f is kept.  check_every (0: never): every that many replays the host reads the number
    of samples still searched and stops the restart at zero.  No tape, no gradient, nothing frozen.

    Static buffers that the next call overwrites: x_adv (returned), best_loss [N] (f at x_adv), loss0 [N] (f at restart 0's
    start), queries [N] (forwards that counted, summed over the restarts), history [steps + 1, N] and decisions [steps + 1, N]
    (f_k and kept-or-not of the LAST restart; rows past an early exit are zero), out (the last forward's output); args: the
    resolved arguments."""
    _what = "SquareRunner"
    _backward = False

    def __init__(self, model, batch, size, norm="linf", eps=None, steps=5000, p_init=0.8, restarts=1, early_stop=True,
                 check_every=0, clip=(-1.0, 1.0), objective="margin", precision="fp32"):
        def arguments():
            if norm != "linf":
                raise ValueError(f"norm must be 'linf': the L2 Square attack is not built, got {norm!r}")
            _refuse_eps(eps)
            _refuse_count("steps", steps, 1)
            _refuse_count("restarts", restarts, 1)
            _refuse_count("check_every", check_every, 0)
            _refuse_fraction("p_init", p_init)
            _refuse_clip(clip)
            if not callable(objective) and objective not in SQUARE_OBJECTIVES:
                raise ValueError(f"objective must be one of {SQUARE_OBJECTIVES} or a callable (out, y) -> [batch], got {objective!r}")
        self._init_model(model, batch, size, precision, arguments)
        self.objective = objective if callable(objective) else (margin_each if objective == "margin" else _neg_cross_entropy_each)
        self.norm, self.eps, self.steps, self.restarts = norm, float(eps), int(steps), int(restarts)
        self.p_init, self.check_every = float(p_init), int(check_every)
        self.early_stop = bool(early_stop)
        self._stop = self.early_stop and objective == "margin"        # only the margin has a threshold that means "fooled"
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.sizes = square_sizes(self.steps, self.size, self.p_init)
        self.args = {"method": "square", "norm": norm, "eps": self.eps, "steps": self.steps, "p_init": self.p_init,
                     "restarts": self.restarts, "early_stop": self.early_stop, "check_every": self.check_every,
                     "clip": (self.lo, self.hi), "objective": _objective_name(objective), "precision": self.precision}
        self.x0 = self.x_try = self.x_best = self.x_adv = self.y = None

    def _buffers(self, x, y):
        from . import kernels as K
        n, dev, steps = self.batch, self.device, self.steps
        self.x0 = x.detach().clone().contiguous()
        self.x_try, self.x_best, self.x_adv = (torch.zeros_like(self.x0) for _ in range(3))
        self.y = y.detach().clone()
        self.ist, self.fst = K.square_state(n, dev)
        self.history = torch.zeros(steps + 1, n, dtype=torch.float32, device=dev)
        self.decisions = torch.zeros(steps + 1, n, dtype=torch.int32, device=dev)
        self.best_loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.loss0 = torch.zeros(n, dtype=torch.float32, device=dev)
        self.queries = torch.zeros(n, dtype=torch.int32, device=dev)
        self._side = torch.tensor(self.sizes, dtype=torch.int32, device=dev)
        self._dh = torch.zeros(steps, n, dtype=torch.int32, device=dev)
        self._dw = torch.zeros(steps, n, dtype=torch.int32, device=dev)
        self._dsign = torch.ones(steps, n, 3, dtype=torch.float32, device=dev)
        self._f_best = self.fst[K.SQUARE_F["f_best"]]
        self._active = self.ist[K.SQUARE_I["active"]]

    def _propose(self, closing=False):
        from . import kernels as K
        K.square_propose(self.x_try, self.x_best, self.x0, self.ist, self._side, self._dh, self._dw, self._dsign, self.eps,
                         self.lo, self.hi, closing=closing)

    def _iteration(self):
        """one query on the static buffers: what the graph holds"""
        from . import kernels as K
        self._propose()
        with torch.no_grad(), _eval_nodes(self.model, self.half):
            out = self.model(self.x_try)
            f = self._each(out)
        self.out = _detached(out)
        K.square_control(f.detach().float().contiguous(), self.ist, self.fst, self.history, self.decisions, self.steps, self._stop)

    def _start(self, generator):
        """a restart's draws into the device tables and its start point, outside the graph; the state back to zero"""
        sign0, h, w, sign = square_draws(self.steps, self.batch, self.size, self.p_init, generator)
        with torch.no_grad():
            self._dh.copy_(h.to(self.device))
            self._dw.copy_(w.to(self.device))
            self._dsign.copy_(sign.to(self.device))
            s = (self.x0 + sign0.to(self.device).unsqueeze(2) * self.eps).clamp_(self.lo, self.hi)
            self.x_try.copy_(s)
            self.x_best.copy_(s)
            self.ist.zero_()
            self.history.zero_()
            self.decisions.zero_()

    def __call__(self, x, y, generator=None):
        from . import kernels as K
        self._check(x, y)
        self.calls += 1
        if self.calls == 1:                                       # eager warm-up: the same launches, a valid attack
            self._buffers(x, y)
        elif self.graph is None:
            self.graph, = self._capture(self._iteration)
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self.queries.zero_()
        for r in range(self.restarts):
            self._start(generator)
            for k in range(self.steps + 1):
                if self.graph is None:
                    self._iteration()
                else:
                    self.graph.replay()
                if self.check_every and (k + 1) % self.check_every == 0 and int(self._active.sum()) == 0:
                    break
            self._propose(closing=True)
            self._merge(r, torch.lt)
            self.queries.add_(self.ist[K.SQUARE_I["queries"]])
        return self.x_adv


_square_arguments = _arguments(SquareRunner)


def square_key(*args, **kwargs):
    """arguments: SquareRunner's after the model; Square has no loss scale: an fp16 runner's key carries (precision,)"""
    return _key(_square_arguments(*args, **kwargs))


def square_runner(model, *args, **kwargs):
    """The model's SquareRunner for the full argument tuple (SquareRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _square_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_square_runners", a, lambda: SquareRunner(model, *a.values()))


# ---- Fast Minimum-Norm attack (FMN, Pintor et al. 2021), linf and l2: the smallest perturbation that flips each sample -------------
FMN_OBJECTIVES = ("margin",)


def fmn_schedule(steps, alpha_init=1.0, alpha_final=None, gamma_init=0.05, gamma_final=0.001):
    """(alpha, gamma): the cosine schedules v_k = v1 + (v0 - v1)(1 + cos(pi k / steps)) / 2 for k = 0 .. steps - 1, computed in
    float64 on the host and rounded to fp32 (CPU tensors [steps]); alpha_final None: alpha_init / 100."""
    steps = int(steps)
    a0 = float(alpha_init)
    a1 = a0 / 100.0 if alpha_final is None else float(alpha_final)
    g0, g1 = float(gamma_init), float(gamma_final)
    c = [(1.0 + math.cos(math.pi * k / steps)) / 2.0 for k in range(steps)]
    return (torch.tensor([a1 + (a0 - a1) * v for v in c], dtype=torch.float64).to(torch.float32),
            torch.tensor([g1 + (g0 - g1) * v for v in c], dtype=torch.float64).to(torch.float32))


def robust_curve(radius, grid):
    """For each eps of grid the fraction of samples that no perturbation within eps flips: mean(radius > eps).  radius [N] as
    FMNRunner leaves it: +inf where nothing was found, 0 for a sample that the clean model gets wrong (never robust).  The
    comparison is made in radius's dtype (an fp32 radius of 0.1 is not above an eps of 0.1).  Returns a float64 tensor like grid."""
    radius = torch.as_tensor(radius).detach().reshape(-1).cpu()
    if not radius.is_floating_point():
        radius = radius.double()
    grid = torch.as_tensor(grid).detach().cpu().to(radius.dtype)
    return (radius.reshape(1, -1) > grid.reshape(-1, 1)).double().mean(1).reshape(grid.shape)


class _MinNormRunner(_Runner):
    """What FMNRunner and SparseFMNRunner share: the arguments and their refusals, the static buffers, the life cycle and the
    closing evaluation.  A subclass names its norms and method, its kernels' state rows (_rows), the cap on eps (_worst_of), the
    three launches that differ — _parts, _control, _project — and whatever state _project needs (_norm_buffers)."""
    _norms = ()
    _method = None

    def _refuse_norm(self, norm, size):
        raise NotImplementedError

    def _init(self, model, batch, size, norm, steps, alpha_init, alpha_final, gamma_init, gamma_final, targeted, clip, objective,
              precision, grad_scale):
        self._refuse_norm(norm, size)
        _refuse_count("steps", steps, 1)
        for name, v in (("alpha_init", alpha_init), ("alpha_final", alpha_init if alpha_final is None else alpha_final)):
            if not 0.0 < float(v) < float("inf"):
                raise ValueError(f"{name} must be a finite step length > 0, got {v!r}")
        for name, v in (("gamma_init", gamma_init), ("gamma_final", gamma_final)):
            if not 0.0 < float(v) < 1.0:
                raise ValueError(f"{name} must be in (0, 1), got {v!r}")
        _refuse_clip(clip)

        def arguments():
            self.grad_scale = resolve_grad_scale(precision, grad_scale)
            if not callable(objective) and objective not in FMN_OBJECTIVES:
                raise ValueError(f"objective must be one of {FMN_OBJECTIVES} or a callable (out, y) -> [batch], got {objective!r}")
        self._init_model(model, batch, size, precision, arguments)
        self.objective = objective if callable(objective) else margin_each
        self.g = None
        self.norm, self.steps, self.targeted = norm, int(steps), bool(targeted)
        self.alpha_init = float(alpha_init)
        self.alpha_final = self.alpha_init / 100.0 if alpha_final is None else float(alpha_final)
        self.gamma_init, self.gamma_final = float(gamma_init), float(gamma_final)
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.alpha, self.gamma = fmn_schedule(self.steps, self.alpha_init, self.alpha_final, self.gamma_init, self.gamma_final)
        self.args = {"method": self._method, "norm": norm, "steps": self.steps, "alpha_init": self.alpha_init,
                     "alpha_final": self.alpha_final, "gamma_init": self.gamma_init, "gamma_final": self.gamma_final,
                     "targeted": self.targeted, "clip": (self.lo, self.hi), "objective": _objective_name(objective),
                     "precision": self.precision, "grad_scale": self.grad_scale}
        self.closing_graph = None
        self.x0 = self.x = self.x_adv = self.y = self.radius = self.found = self.margin0 = None

    def _buffers(self, x, y):
        n, dev, per = self.batch, self.device, 3 * self.size * self.size
        state, I, F = self._rows()
        self.x0 = x.detach().clone().contiguous()
        self.x = self.x0.clone().requires_grad_()                 # the static leaf: the current iterate
        self.x_adv = torch.zeros_like(self.x0)                    # the best point per sample
        self.y = y.detach().clone()
        self.ist, self.fst = state(n, dev)
        self.history = torch.zeros(self.steps + 1, n, dtype=torch.float32, device=dev)
        self.eps_history = torch.zeros(self.steps, n, dtype=torch.float32, device=dev)
        self.margin0 = self.history[0]
        self.radius = self.fst[F["best"]]
        self.found = self.ist[I["found"]]
        self._k = self.ist[I["k"]]
        self._improved = self.ist[I["improved"]]
        self._fac = torch.zeros(n, dtype=torch.float64, device=dev)
        self._worst = torch.zeros(n, dtype=torch.float32, device=dev)
        self._alpha, self._gamma = self.alpha.to(dev), self.gamma.to(dev)
        self._per = per
        self._norm_buffers(n, dev, per)

    def _descended(self, out):
        f = self._each(out)
        return -f if self.targeted else f

    def _iteration(self):
        """one iteration on the static buffers: what the graph holds"""
        g, self.out, f = self._grad(self.x, self._descended)
        self.g = g = g.contiguous()
        self._parts(g)
        self._control(f)
        self._project(g)

    def _closing(self):
        """the closing evaluation: forward only at the last point; if it is adversarial and closer, it becomes the best"""
        from . import kernels as K
        with torch.no_grad(), self._nodes():
            f = self._descended(self.model(self.x))
        self._parts(None)
        self._control(f, closing=True)
        K.apgd_keep(self.x_adv, self.x, self._improved)

    def _start(self, x, y):
        """the start point, the cap on eps and the best point's default, outside the graph; the iteration counters back to 0"""
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self.x.copy_(x.clamp(self.lo, self.hi))
            self.x_adv.copy_(x)
            self._worst.copy_(self._worst_of(torch.maximum(self.x0 - self.lo, self.hi - self.x0).flatten(1)))
            self._k.zero_()

    def __call__(self, x, y):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up: the same launches, a valid attack
                self._buffers(x, y)
            elif self.graph is None:
                self.graph, self.closing_graph = self._capture(self._iteration, self._closing)
            self._start(x, y)
            if self.graph is None:
                with frozen(self.model):
                    for _ in range(self.steps):
                        self._iteration()
                    self._closing()
            else:
                for _ in range(self.steps):
                    self.graph.replay()
                self.closing_graph.replay()
        return self.x_adv


class FMNRunner(_MinNormRunner):
    """runner = FMNRunner(model, batch, size, norm="linf", steps=100, ...); x_adv = runner(x, y).

    Fast Minimum-Norm attack: per sample the smallest perturbation (in `norm`) that makes the objective f negative
    (objective="margin": margin_each, negative once the sample is misclassified; targeted=True: -margin_each with y the target; or
    a callable (out, y) -> [batch]).  Each sample carries its own budget eps on the device: while the sample is adversarial eps
    shrinks by (1 - gamma_k) (never above the best norm found), after it was lost again eps grows by (1 + gamma_k), and before
    anything was found eps is the linearised distance |x - x0| + |f| / |g|_dual; the step is alpha_k along -g / |g|_2, projected
    onto the eps-ball around x and onto clip; alpha_k and gamma_k follow fmn_schedule.  One hipGraph holds ONE iteration —
    forward, f, d sum(f) / dx, ud_fmn_norm_parts (the four norms in one pass), ud_fmn_control (one thread per sample),
    ud_fmn_update (linf: step, box and clip in one pass; l2: followed by ud_sample_sumsq + ud_fmn_project_l2) — and a call replays
    it `steps` times, then a forward-only graph that scores the last point.  No restarts, no random start: x starts at
    clamp(x, clip).

    Static buffers that the next call overwrites: x_adv (returned: the best adversarial point, x where none was found), radius [N]
    (its norm, +inf where none was found), found [N] int32, margin0 [N] (f at the start: history[0]), history [steps + 1, N] and
    eps_history [steps, N] (f_k and eps_k; history[steps] is the closing evaluation), g (the last iteration's gradient), out (the
    last forward's output); args: the resolved arguments.  precision / grad_scale: as InputGradRunner."""
    _what = "FMNRunner"
    _norms = NORMS
    _method = "fmn"

    def __init__(self, model, batch, size, norm="linf", steps=100, alpha_init=1.0, alpha_final=None, gamma_init=0.05,
                 gamma_final=0.001, targeted=False, clip=(-1.0, 1.0), objective="margin", precision="fp32", grad_scale=None):
        self._init(model, batch, size, norm, steps, alpha_init, alpha_final, gamma_init, gamma_final, targeted, clip, objective,
                   precision, grad_scale)

    def _refuse_norm(self, norm, size):
        _refuse_norm(norm)

    def _rows(self):
        from . import kernels as K
        return K.fmn_state, K.FMN_I, K.FMN_F

    def _norm_buffers(self, n, dev, per):
        from . import kernels as K
        self._ws = K.fmn_ws(self.x0, n, per)
        if self.norm == "l2":
            self._dss = torch.zeros(n, dtype=torch.float64, device=dev)
            self._ss_ws = K.fmn_sumsq_ws(self.x0, n, per)

    def _worst_of(self, far):
        return far.amax(1) if self.norm == "linf" else far.norm(dim=1)

    def _parts(self, g):
        from . import kernels as K
        K.fmn_norm_parts(self.x, self.x0, g, ws=self._ws)

    def _control(self, f, closing=False):
        from . import kernels as K
        K.fmn_control(f.detach().float().contiguous(), self._ws, self._per, self.ist, self.fst, self._fac, self.history,
                      self.eps_history, self._alpha, self._gamma, self._worst, self.norm, closing=closing)

    def _project(self, g):
        from . import kernels as K
        K.fmn_update(self.x, self.x_adv, self.x0, g, self.ist, self.fst, self._fac, self.norm, self.lo, self.hi)
        if self.norm == "l2":
            K.sample_sumsq(self.x, self.x0, out=self._dss, ws=self._ss_ws)
            K.fmn_project_l2(self.x, self.x0, self._dss, self.fst, self.lo, self.hi)


_fmn_arguments = _arguments(FMNRunner)


def fmn_key(*args, **kwargs):
    """arguments: FMNRunner's after the model"""
    return _key(_fmn_arguments(*args, **kwargs))


def fmn_runner(model, *args, **kwargs):
    """The model's FMNRunner for the full argument tuple (FMNRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _fmn_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_fmn_runners", a, lambda: FMNRunner(model, *a.values()))


# ---- Sparse minimum-norm attack: FMN's state machine with an L1 or an L0 budget (csrc/sfmn.hip) -----------------------------------
SPARSE_NORMS = ("l1", "l0")


class SparseFMNRunner(_MinNormRunner):
    """runner = SparseFMNRunner(model, batch, size, norm="l1", steps=100, ...); x_adv = runner(x, y).

    FMNRunner for the sparse norms — the same arguments, life cycle and static results, args["method"] == "sparse_fmn":
      norm "l1": radius = sum |x_adv - x| over the sample; the step is projected onto the L1 ball of the sample's eps around x
        (soft threshold of z - x), then onto clip;
      norm "l0": radius = the number of ELEMENTS of the [3, size, size] sample that differ from x (a float that is an exact
        integer; refused where 3 size^2 >= 2^24); eps is an integer: the eps largest |z - x| keep their step, every other element
        returns to x (ties at the threshold are all dropped), then clip.
    The budget follows FMN's rules with these pieces: before anything was found eps = |x - x0| + |f| / max |g| (l1: the dual
    norm is L-infinity) or the count + max(1, ceil(|f| / ((hi - lo) max |g|))) (l0: each coordinate moves f by at most
    (hi - lo) max |g|); an l0 budget shrinks and grows by at least one element; eps never exceeds sum max(x - lo, hi - x) (l1) or
    3 size^2 (l0).  The step is still alpha_k along -g / |g|_2: alpha_init (default 1.0) MUST be sized to the norm — an
    L2-normalised step of length 1 spread over every pixel moves an L1 distance of up to sqrt(3 size^2) but each single pixel
    hardly at all, so a sparse projection of it keeps almost nothing; the suite's fixtures use alpha_init 8 (l1) and 256 (l0) at
    128^2.  One hipGraph holds ONE iteration — forward, f, d sum(f) / dx, ud_sfmn_norm_parts, ud_sfmn_control, ud_sfmn_select
    (one workgroup per sample finds the threshold), ud_sfmn_apply (keep-best copy, step, projection and clip in one pass) — and a
    forward-only closing graph.  precision / grad_scale: as InputGradRunner."""
    _what = "SparseFMNRunner"
    _norms = SPARSE_NORMS
    _method = "sparse_fmn"

    def __init__(self, model, batch, size, norm="l1", steps=100, alpha_init=1.0, alpha_final=None, gamma_init=0.05,
                 gamma_final=0.001, targeted=False, clip=(-1.0, 1.0), objective="margin", precision="fp32", grad_scale=None):
        self._init(model, batch, size, norm, steps, alpha_init, alpha_final, gamma_init, gamma_final, targeted, clip, objective,
                   precision, grad_scale)

    def _refuse_norm(self, norm, size):
        from . import kernels as K
        if norm not in SPARSE_NORMS:
            raise ValueError(f"norm must be one of {SPARSE_NORMS}, got {norm!r}")
        if norm == "l0" and 3 * int(size) * int(size) >= K.SFMN_L0_MAX_PER:
            raise ValueError(f"norm 'l0' counts elements in fp32: 3 size^2 must stay below 2^24, got size {size!r}")

    def _rows(self):
        from . import kernels as K
        return K.sfmn_state, K.SFMN_I, K.SFMN_F

    def _norm_buffers(self, n, dev, per):
        from . import kernels as K
        self._ws = K.sfmn_ws(self.x0, n, per)
        self._thr = torch.zeros(n, dtype=torch.float64, device=dev)

    def _worst_of(self, far):
        return far.sum(1) if self.norm == "l1" else torch.full_like(far[:, 0], float(far.shape[1]))

    def _parts(self, g):
        from . import kernels as K
        K.sfmn_norm_parts(self.x, self.x0, g, ws=self._ws)

    def _control(self, f, closing=False):
        from . import kernels as K
        K.sfmn_control(f.detach().float().contiguous(), self._ws, self._per, self.ist, self.fst, self._fac, self.history,
                       self.eps_history, self._alpha, self._gamma, self._worst, self.norm, self.lo, self.hi, closing=closing)

    def _project(self, g):
        from . import kernels as K
        K.sfmn_select(self.x, self.x0, g, self.fst, self._fac, self._thr, self.norm)
        K.sfmn_apply(self.x, self.x_adv, self.x0, g, self.ist, self._fac, self._thr, self.norm, self.lo, self.hi)


_sparse_fmn_arguments = _arguments(SparseFMNRunner)


def sparse_fmn_key(*args, **kwargs):
    """arguments: SparseFMNRunner's after the model"""
    return _key(_sparse_fmn_arguments(*args, **kwargs))


def sparse_fmn_runner(model, *args, **kwargs):
    """The model's SparseFMNRunner for the full argument tuple (SparseFMNRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _sparse_fmn_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_sparse_fmn_runners", a, lambda: SparseFMNRunner(model, *a.values()))

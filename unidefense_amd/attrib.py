"""Attribution: which pixels a decision rests on, and a score that tells a meaningful map from a random one: AttributionRunner,
DeletionRunner, attribution_runner, deletion_runner, attribution_schedule, deletion_counts, trapezoid_auc and the numpy
restatements ref_attr_point, ref_attr_accumulate, ref_attr_finish, ref_rank_keys, ref_rank_select, ref_attr_mask.

Integrated gradients (Sundararajan, Taly and Yan 2017): attr = (x - b) * integral over a in [0, 1] of dF/dx at b + a (x - b), for
a per-sample score F of the frozen eval-mode detector and a baseline b.  What makes the map checkable is completeness: the
attributions sum to F(x) - F(b) when the integral is exact.  The runner forms that sum in double on the device (total) next to
F(x) and F(b) from a forward of their own, and leaves gap = total - (f_x - f_b): the quadrature defect a user reads to judge
`steps`.  The integral is a quadrature with `steps` nodes, Gauss-Legendre (exact for a polynomial integrand of degree 2 steps - 1)
or the midpoint rule; SmoothGrad (Smilkov et al. 2017) is its degenerate case — one node at a = 1, no (x - b) factor — averaged
over `samples` noisy copies; samples = 1, sigma = 0 is the plain saliency map.

The score of a map is the deletion / insertion curve (Petsiuk, Das and Saenko 2018, RISE): replace the top fraction of pixels,
in the map's order, by the baseline (or start from the baseline and insert them) and watch the class probability.  A faithful map
has a LOW deletion AUC and a HIGH insertion AUC; a random map is the control.  The order is a total one — the heat value, a NaN
last, ties to the lower pixel index — so the curve is a deterministic function of the map.

Both runners follow the siblings' life cycle (unidefense_amd/attack.py): call 1 eager, call 2 captures, later calls replay with no
host-device synchronisation inside the loop.  The per-sample counters live on the device (csrc/attrib.hip: ud_attr_control), so
ONE captured iteration serves the whole schedule; the noise of a noise tunnel is ud_smooth_noise's, a pure function of (seed, id,
iteration, element)."""
import math

import numpy as np
import torch

from .attack import _arguments, _cached_runner, _detached, _refuse_count, _Runner, frozen, margin_each, resolve_grad_scale
from .infer import _eval_nodes
from .smooth import _refuse_seed

METHODS = ("ig", "smoothgrad")
RULES = ("gauss_legendre", "midpoint")
BASELINES = ("black", "grey", "given")
BASELINE_VALUE = {"black": -1.0, "grey": 0.0}                # inputs live in [-1, 1]: black is the clip's lower bound
SCORES = ("margin", "logit")
REDUCES = ("sum", "abs")
MODES = ("deletion", "insertion")
DEFAULT_FRACTIONS = (0, .02, .05, .1, .2, .35, .5, .75, 1)


# ---- the quadrature ----------------------------------------------------------------------------------------------------------------
def attribution_schedule(steps, rule="gauss_legendre"):
    """(nodes, weights): float64 arrays [steps] of the rule on [0, 1].  "gauss_legendre": numpy's leggauss nodes t and weights v on
    [-1, 1] mapped by a = (t + 1) / 2, w = v / 2; "midpoint": a_i = (i + 1/2) / steps, w_i = 1 / steps.  The weights sum to 1."""
    _refuse_count("steps", steps, 1)
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    m = int(steps)
    if rule == "midpoint":
        return (np.arange(m, dtype=np.float64) + 0.5) / m, np.full(m, 1.0 / m, dtype=np.float64)
    t, v = np.polynomial.legendre.leggauss(m)
    return 0.5 * (t.astype(np.float64) + 1.0), 0.5 * v.astype(np.float64)


def deletion_counts(fractions, size):
    """kcount[j] = floor(fractions[j] size^2 + 1/2): the pixels replaced at point j of the curve, exact integers"""
    hw = int(size) * int(size)
    return [int(math.floor(float(f) * hw + 0.5)) for f in fractions]


def trapezoid_auc(curve, fractions):
    """float64 [N]: the trapezoid of curve [K, N] over fractions [K], sum over j in order of (f[j + 1] - f[j]) (c[j] + c[j + 1]) / 2"""
    c = np.asarray(curve, dtype=np.float64)
    f = np.asarray(fractions, dtype=np.float64)
    auc = np.zeros(c.shape[1:], dtype=np.float64)
    for j in range(len(f) - 1):
        auc = auc + (f[j + 1] - f[j]) * ((c[j] + c[j + 1]) / 2.0)
    return auc


# ---- numpy restatements of the kernels ---------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def ref_attr_point(x, b, xp, k, alpha, iters):
    """ud_attr_point restated: a new array like xp (the rows whose counter lies outside [0, iters) are xp's own); three float32
    operations per element, a == 1 is x and a == 0 is b by rule."""
    x, b, out = _np(x).astype(np.float32), _np(b).astype(np.float32), np.array(_np(xp), dtype=np.float32)
    k, alpha = _np(k), _np(alpha).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(x.shape[0]):
            if not 0 <= int(k[n]) < int(iters):
                continue
            a = alpha[int(k[n]) % len(alpha)]
            if a == np.float32(1):
                out[n] = x[n]
            elif a == np.float32(0):
                out[n] = b[n]
            else:
                d = (x[n] - b[n]).astype(np.float32)
                out[n] = (b[n] + (a * d).astype(np.float32)).astype(np.float32)
    return out


def ref_attr_accumulate(g, acc, k, w, iters):
    """ud_attr_accumulate restated: a new float64 array: acc + (double)w[k % steps] (double)g, one product and one add"""
    g, out = _np(g).astype(np.float32), np.array(_np(acc), dtype=np.float64)
    k, w = _np(k), _np(w).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(g.shape[0]):
            if 0 <= int(k[n]) < int(iters):
                out[n] = out[n] + w[int(k[n]) % len(w)] * g[n].astype(np.float64)
    return out


def ref_attr_finish(x, b, acc, mode="ig", reduce="sum", scale=1.0):
    """ud_attr_finish restated for x, b [N, 3, S, S] and acc float64: (attr float32, heat float32 [N, S, S], values float64): the
    double value per element ((x - b) acc scale, or acc scale for "grad"), its float32 rounding, and the channel sum in the order
    0, 1, 2.  total is any fixed-order sum of `values` per sample (math.fsum bounds them all)."""
    if mode not in ("ig", "grad") or reduce not in REDUCES:
        raise ValueError(f"mode must be 'ig' or 'grad' and reduce one of {REDUCES}, got {mode!r}, {reduce!r}")
    x, b, acc = _np(x).astype(np.float64), _np(b).astype(np.float64), _np(acc).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = acc * np.float64(scale) if mode == "grad" else ((x - b) * acc) * np.float64(scale)
        t = np.abs(v) if reduce == "abs" else v
        heat = (t[:, 0] + t[:, 1]) + t[:, 2]
        return v.astype(np.float32), heat.astype(np.float32), v


def ref_rank_keys(heat):
    """uint64 [N, HW]: the key of every pixel of heat [N, ...]: high word the order-preserving uint32 image of the float32 heat (a
    NaN: 0; -0 as +0), low word ~p"""
    h = np.ascontiguousarray(_np(heat), dtype=np.float32)
    h = h.reshape(h.shape[0], -1)
    u = h.view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    u[np.isnan(h)] = 0
    p = np.arange(h.shape[1], dtype=np.uint32)
    return (u.astype(np.uint64) << np.uint64(32)) | (~p).astype(np.uint64)[None, :]


def ref_rank_select(heat, kcount):
    """uint64 [K, N]: the key of the kcount[j]-th pixel in a stable argsort of -heat with NaN last (ties: the lower pixel index
    first); 2^64 - 1 for kcount[j] == 0.  Independent of ref_rank_keys' integer order: the two must agree."""
    h = np.ascontiguousarray(_np(heat), dtype=np.float32)
    h = h.reshape(h.shape[0], -1)
    keys = ref_rank_keys(h)
    thr = np.full((len(kcount), h.shape[0]), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    for n in range(h.shape[0]):
        nan = np.isnan(h[n])
        col = np.where(nan, np.float32(0), h[n]) + np.float32(0)           # -0 + 0 = +0: the two zeros tie
        order = np.argsort(-col.astype(np.float64), kind="stable")
        order = np.concatenate([order[~nan[order]], order[nan[order]]])    # NaN last, each group in index order
        for j, kc in enumerate(kcount):
            if int(kc) >= 1:
                thr[j, n] = keys[n, order[min(int(kc), h.shape[1]) - 1]]
    return thr


def ref_attr_mask(x, b, heat, thr, j, mode="deletion"):
    """ud_attr_mask restated for x, b [N, 3, S, S], heat [N, S, S], thr uint64 [K, N] and the per-sample rows j [N]: a copy of x
    with the pixels whose key >= thr[j[n], n] taken from b ("deletion"), or of b with them taken from x ("insertion")."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    x, b = _np(x).astype(np.float32), _np(b).astype(np.float32)
    keys = ref_rank_keys(heat).reshape(x.shape[0], 1, x.shape[2], x.shape[3])
    t = np.array([thr[int(j[n]), n] for n in range(x.shape[0])], dtype=np.uint64).reshape(-1, 1, 1, 1)
    top = np.broadcast_to(keys >= t, x.shape)
    return np.where(top, b, x) if mode == "deletion" else np.where(top, x, b)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refuse_choice(name, v, choices):
    if not isinstance(v, str) or v not in choices:
        raise ValueError(f"{name} must be one of {choices}, got {v!r}")


def _refuse_sigma(sigma):
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (0.0 <= float(sigma) < math.inf):
        raise ValueError(f"sigma must be finite and >= 0, got {sigma!r}")


def _refuse_score(score, names, form):
    if not callable(score) and score not in names:
        raise ValueError(f"score must be one of {names} or a callable {form} -> [batch], got {score!r}")


def _refuse_fractions(fractions):
    try:
        f = [float(v) for v in fractions]
    except (TypeError, ValueError):
        f = []
    if len(f) < 2 or not all(0.0 <= v <= 1.0 for v in f) or any(a > b for a, b in zip(f, f[1:])):
        raise ValueError(f"fractions must hold at least two non-decreasing values in [0, 1], got {fractions!r}")


def _score_name(score):
    return score if isinstance(score, str) else getattr(score, "__name__", repr(score))


def logit_each(out, y):
    """The logit of the class y, [batch]; with a single logit (2 y - 1) z"""
    z = out["cls_out"]
    if z.shape[1] == 1:
        return (2.0 * y.to(z.dtype) - 1.0) * z.squeeze(1)
    return z.gather(1, y.reshape(-1, 1)).squeeze(1)


def prob_each(out, y):
    """The softmax probability of the class y, [batch]; with a single logit sigmoid((2 y - 1) z)"""
    z = out["cls_out"]
    if z.shape[1] == 1:
        return torch.sigmoid((2.0 * y.to(z.dtype) - 1.0) * z.squeeze(1))
    return torch.softmax(z, 1).gather(1, y.reshape(-1, 1)).squeeze(1)


class _MapRunner(_Runner):
    """What the two runners share: the baseline, the stream ids, the per-sample score's shape check"""

    def _baseline(self, given):
        """the call's baseline as something copy_ broadcasts into the static [batch, 3, size, size] buffer"""
        if self.baseline != "given":
            if given is not None:
                raise ValueError(f"{self._what} was made with baseline={self.baseline!r}: a baseline tensor needs baseline='given'")
            return None
        if not isinstance(given, torch.Tensor) or not given.is_cuda or given.dtype != torch.float32 \
                or tuple(given.shape) not in (self.shape, self.shape[1:]):
            raise ValueError(f"baseline='given' takes a cuda float32 tensor {list(self.shape)} or {list(self.shape[1:])} at the "
                             f"call, got {tuple(given.shape) if isinstance(given, torch.Tensor) else type(given).__name__}")
        return given.detach()

    def _fill_baseline(self, given):
        if given is None:
            self.b.fill_(BASELINE_VALUE[self.baseline])
        else:
            self.b.copy_(given)

    def _scored(self, f):
        if not isinstance(f, torch.Tensor) or tuple(f.shape) != (self.batch,):
            raise ValueError(f"{self._what}'s score must return a [{self.batch}] tensor, one value per sample, got "
                             f"{tuple(f.shape) if isinstance(f, torch.Tensor) else type(f).__name__}")
        return f

    @staticmethod
    def _ids(ids, n, dev):
        if ids is None:
            return torch.arange(n, dtype=torch.int64, device=dev)
        if not isinstance(ids, torch.Tensor) or tuple(ids.shape) != (n,) or ids.dtype != torch.int64:
            raise ValueError(f"ids must be an int64 tensor [{n}], got {getattr(ids, 'dtype', type(ids).__name__)} "
                             f"{tuple(getattr(ids, 'shape', ()))}")
        return ids.to(dev).contiguous()


class AttributionRunner(_MapRunner):
    """runner = AttributionRunner(model, batch, size, method="ig", steps=32, rule="gauss_legendre", baseline="black", ...);
    attr = runner(x, y[, ids, baseline]).

    method "ig": attr = (x - b) sum_k w_k dF/dx(b + a_k (x - b)) with (a, w) = attribution_schedule(steps, rule); "smoothgrad":
    one node at a = 1 and no (x - b) factor (steps is 1 whatever was given).  baseline: "black" (-1, the clip's lower bound),
    "grey" (0) or "given": a [batch, 3, size, size] or [3, size, size] tensor passed at the call.  samples / sigma: a noise tunnel:
    iteration i of steps * samples takes node i % steps and, where sigma > 0, adds sigma z_i to the point — ud_smooth_noise's
    Gaussian of (seed, ids[n], i, element), so a sample's map does not depend on its batch position; the result is the mean over
    the samples.  score: "margin" (attack.margin_each), "logit" (the logit of y) or a callable (out, y, x_point) -> [batch] that the
    caller guarantees capturable; the SUM of the per-sample scores is differentiated, so each sample's gradient is its own.
    reduce: the heat map is the channel sum of attr ("sum") or of |attr| ("abs").  precision / grad_scale: as InputGradRunner.

    One hipGraph holds ONE iteration — ud_attr_point, the noise, forward + d/dx on the static leaf, ud_attr_accumulate,
    ud_attr_control — and a second, forward-only graph scores a static point: it is replayed on x and then on b.  ud_attr_finish
    runs after the loop.  A callable score that ignores the model's output still has the forward's tape consumed by the
    iteration's backward (a zero-weight link to cls_out).

    What the next call overwrites: attr [N, 3, S, S] fp32 (returned), heat [N, S, S] fp32, total [N] float64 (the sum of the
    attribution before its fp32 rounding), f_x, f_b [N] fp32 (the score at x and at the baseline), gap [N] float64 = total - (f_x -
    f_b) (ig: the completeness defect), path [iters, N] fp32 (the score at every point), acc (float64, the weighted gradient
    sum), g (the last gradient), out; args: the resolved arguments."""
    _what = "AttributionRunner"

    def __init__(self, model, batch, size, method="ig", steps=32, rule="gauss_legendre", baseline="black", samples=1, sigma=0.0,
                 score="margin", reduce="sum", seed=0, precision="fp32", grad_scale=None):
        def arguments():
            _refuse_choice("method", method, METHODS)
            _refuse_count("steps", steps, 1)
            _refuse_choice("rule", rule, RULES)
            _refuse_choice("baseline", baseline, BASELINES)
            _refuse_count("samples", samples, 1)
            if int(steps) * int(samples) >= 1 << 31:
                raise ValueError(f"steps * samples must stay below 2^31, got {steps!r} * {samples!r}")
            _refuse_sigma(sigma)
            _refuse_score(score, SCORES, "(out, y, x_point)")
            _refuse_choice("reduce", reduce, REDUCES)
            _refuse_seed(seed)
            self.grad_scale = resolve_grad_scale(precision, grad_scale)
        self._init_model(model, batch, size, precision, arguments)
        self.method, self.rule, self.baseline, self.reduce = method, rule, baseline, reduce
        self.steps = int(steps) if method == "ig" else 1
        self.samples, self.sigma, self.seed, self.score = int(samples), float(sigma), int(seed), score
        self.iters = self.steps * self.samples
        if method == "ig":
            self.nodes, self.weights = attribution_schedule(self.steps, rule)
        else:
            self.nodes, self.weights = np.ones(1, dtype=np.float64), np.ones(1, dtype=np.float64)
        self.scale = 1.0 / self.samples
        self.args = {"method": method, "steps": self.steps, "rule": rule, "baseline": baseline, "samples": self.samples,
                     "sigma": self.sigma, "score": _score_name(score), "reduce": reduce, "seed": self.seed,
                     "precision": self.precision, "grad_scale": self.grad_scale}
        self.g = self.x0 = self.b = self.xp = self.y = self.ids = self.ist = self.acc = self.path = None
        self.attr = self.heat = self.total = self.f_x = self.f_b = self.gap = self._scores_graph = None

    def _score(self, out, x_point):
        if callable(self.score):
            f = self._scored(self.score(out, self.y, x_point))
            # a callable may ignore the model's output; the zero-weight link keeps the forward's tape consumed by the backward
            # of the iteration that recorded it, as in every other gradient runner (f + 0 is f)
            return f + 0.0 * out["cls_out"].sum() if torch.is_grad_enabled() else f
        return self._scored(margin_each(out, self.y) if self.score == "margin" else logit_each(out, self.y))

    def _buffers(self, x):
        from . import kernels as K
        dev, per = self.device, 3 * self.size * self.size
        self.x0 = x.detach().clone().contiguous()
        self.b = torch.zeros_like(self.x0)
        self.xp = torch.zeros_like(self.x0).requires_grad_()
        self.y = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self.ids = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self.ist = torch.zeros(len(K.ATTR_I), self.batch, dtype=torch.int32, device=dev)
        self._k = self.ist[K.ATTR_I["k"]]
        self.acc = torch.zeros(self.shape, dtype=torch.float64, device=dev)
        self.path = torch.zeros(self.iters, self.batch, dtype=torch.float32, device=dev)
        self._alpha = torch.from_numpy(self.nodes.astype(np.float32)).to(dev)
        self._w = torch.from_numpy(self.weights).to(dev)
        self.attr = torch.zeros_like(self.x0)
        self.heat = torch.zeros(self.batch, self.size, self.size, dtype=torch.float32, device=dev)
        self.total = torch.zeros(self.batch, dtype=torch.float64, device=dev)
        self._ws = torch.zeros(max(K.attr_finish_ws_bytes(self.batch, per) // 8, 1), dtype=torch.float64, device=dev)
        self.f_x = torch.zeros(self.batch, dtype=torch.float32, device=dev)
        self.f_b = torch.zeros(self.batch, dtype=torch.float32, device=dev)
        self.xs = torch.zeros_like(self.x0)
        self._fs = torch.zeros(self.batch, dtype=torch.float32, device=dev)

    def _iteration(self):
        """one node of the path on the static buffers: what the graph holds"""
        from . import kernels as K
        K.attr_point(self.x0, self.b, self.xp, self._k, self._alpha, self.iters)
        if self.sigma > 0.0:
            K.smooth_noise(self.xp, self.xp, self.ids, self._k, 0, "gaussian", self.sigma, self.seed)
        self.g, self.out, f = self._grad(self.xp, lambda out: self._score(out, self.xp))
        K.attr_accumulate(self.g.contiguous(), self.acc, self._k, self._w, self.iters)
        K.attr_control(f.detach().float().contiguous(), self.ist, self.path)

    def _scored_at(self):
        """the forward-only graph: the score at the static point xs, one forward as in the siblings' closing graphs"""
        with torch.no_grad(), self._nodes():
            self._fs.copy_(self._score(self.model(self.xs), self.xs).detach().float())

    def _scores(self):
        """the score at x, then at the baseline: the forward-only graph (or its eager launches) twice, no synchronisation"""
        with torch.no_grad():
            for src, dst in ((self.x0, self.f_x), (self.b, self.f_b)):
                self.xs.copy_(src)
                if self._scores_graph is None:
                    self._scored_at()
                else:
                    self._scores_graph.replay()
                dst.copy_(self._fs)

    def _finish(self):
        from . import kernels as K
        with torch.no_grad():
            K.attr_finish(self.x0, self.b, self.acc, self.attr, self.heat, self.total, "ig" if self.method == "ig" else "grad",
                          self.reduce, self.scale, ws=self._ws)
            self.gap = self.total - (self.f_x.double() - self.f_b.double())
        return self.attr

    def __call__(self, x, y, ids=None, baseline=None):
        self._check(x, y)
        ids = self._ids(ids, self.batch, self.device)
        given = self._baseline(baseline)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:
                self._buffers(x)
            elif self.graph is None:
                self.graph, self._scores_graph = self._capture(self._iteration, self._scored_at)
            with torch.no_grad():
                self.x0.copy_(x)
                self.y.copy_(y)
                self.ids.copy_(ids)
                self._fill_baseline(given)
                self.ist.zero_()
                self.acc.zero_()
            if self.graph is None:                                 # eager warm-up: the same launches, a valid attribution
                with frozen(self.model):
                    for _ in range(self.iters):
                        self._iteration()
                    self._scores()
                return self._finish()
        for _ in range(self.iters):
            self.graph.replay()
        self._scores()
        return self._finish()


_attribution_arguments = _arguments(AttributionRunner)


def _hook_key(a, name):
    return dict(a, **{name: id(a[name]) if callable(a[name]) else a[name]})


def attribution_runner(model, *args, **kwargs):
    """The model's AttributionRunner for the full argument tuple (AttributionRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own.  A callable `score` is keyed by identity (the runner keeps it alive)."""
    a = _attribution_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_attribution_runners", _hook_key(a, "score"), lambda: AttributionRunner(model, *a.values()))


class DeletionRunner(_MapRunner):
    """runner = DeletionRunner(model, batch, size, fractions=(0, .02, ..., 1), mode="deletion", baseline="black", score="prob",
    precision="fp32"); auc = runner(x, y, heat[, baseline]).

    The deletion (insertion) curve of the heat map `heat` [batch, size, size] fp32: point j scores the image whose kcount[j] =
    deletion_counts(fractions, size)[j] top pixels — by heat, a NaN last, ties to the lower pixel index — are the baseline's
    ("deletion"), or the baseline with those pixels inserted from the image ("insertion").  score: "prob" (the softmax probability
    of y) or a callable (out, y, x_masked) -> [batch].  One ud_attr_rank_select per call finds every point's threshold; one
    captured query — ud_attr_mask, the eval forward (InferenceRunner's, in either precision), the score, ud_attr_control — is
    replayed len(fractions) times; one read follows.

    What the next call overwrites: auc [N] float64 (returned: trapezoid_auc(curve, fractions), on the host after the one read),
    curve [K, N] fp32, thr [K, N] int64 (the bits of the uint64 thresholds), xq (the last masked image), out."""
    _what = "DeletionRunner"
    _backward = False

    def __init__(self, model, batch, size, fractions=DEFAULT_FRACTIONS, mode="deletion", baseline="black", score="prob",
                 precision="fp32"):
        def arguments():
            _refuse_fractions(fractions)
            _refuse_choice("mode", mode, MODES)
            _refuse_choice("baseline", baseline, BASELINES)
            _refuse_score(score, ("prob",), "(out, y, x_masked)")
        self._init_model(model, batch, size, precision, arguments)
        self.fractions = tuple(float(f) for f in fractions)
        self.kcount = deletion_counts(self.fractions, self.size)
        self.mode, self.baseline, self.score = mode, baseline, score
        self.args = {"fractions": self.fractions, "kcount": tuple(self.kcount), "mode": mode, "baseline": baseline,
                     "score": _score_name(score), "precision": self.precision}
        self.x0 = self.b = self.xq = self.y = self.hmap = self.ist = self.thr = self.curve = self.auc = None

    def _buffers(self, x):
        from . import kernels as K
        dev, k = self.device, len(self.kcount)
        self.x0 = x.detach().clone().contiguous()
        self.b = torch.zeros_like(self.x0)
        self.xq = torch.zeros_like(self.x0)
        self.y = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self.hmap = torch.zeros(self.batch, self.size, self.size, dtype=torch.float32, device=dev)
        self.ist = torch.zeros(len(K.ATTR_I), self.batch, dtype=torch.int32, device=dev)
        self._kcount = torch.tensor(self.kcount, dtype=torch.int32, device=dev)
        self.thr = torch.zeros(k, self.batch, dtype=torch.int64, device=dev)
        self.curve = torch.zeros(k, self.batch, dtype=torch.float32, device=dev)

    def _iteration(self):
        """one point of the curve on the static buffers: what the graph holds"""
        from . import kernels as K
        K.attr_mask(self.x0, self.b, self.hmap, self.thr, self.ist, self.xq, self.mode)
        with torch.no_grad(), _eval_nodes(self.model, self.half):
            out = self.model(self.xq)
            f = self.score(out, self.y, self.xq) if callable(self.score) else prob_each(out, self.y)
            f = self._scored(f).detach().float().contiguous()
        self.out = _detached(out)
        K.attr_control(f, self.ist, self.curve)

    def __call__(self, x, y, heat, baseline=None):
        from . import kernels as K
        self._check(x, y)
        if not isinstance(heat, torch.Tensor) or not heat.is_cuda or heat.dtype != torch.float32 \
                or tuple(heat.shape) != (self.batch, self.size, self.size):
            raise ValueError(f"heat must be a cuda float32 tensor [{self.batch}, {self.size}, {self.size}], got "
                             f"{tuple(heat.shape) if isinstance(heat, torch.Tensor) else type(heat).__name__}")
        given = self._baseline(baseline)
        self.calls += 1
        if self.calls == 1:
            self._buffers(x)
        elif self.graph is None:
            self.graph, = self._capture(self._iteration)
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self.hmap.copy_(heat)
            self._fill_baseline(given)
            self.ist.zero_()
            K.attr_rank_select(self.hmap, self._kcount, self.thr)
        for _ in range(len(self.kcount)):
            if self.graph is None:
                self._iteration()
            else:
                self.graph.replay()
        auc = trapezoid_auc(self.curve.cpu().numpy(), self.fractions)        # the one read
        self.auc = torch.from_numpy(auc).to(self.device)
        return self.auc


_deletion_arguments = _arguments(DeletionRunner)


def deletion_runner(model, *args, **kwargs):
    """The model's DeletionRunner for the full argument tuple (DeletionRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own.  A callable `score` is keyed by identity."""
    a = _deletion_arguments(*args, **kwargs)
    _refuse_fractions(a["fractions"])                            # the key below reads them
    key = _hook_key(dict(a, fractions=tuple(float(f) for f in a["fractions"])), "score")
    return _cached_runner(model, "_ud_deletion_runners", key, lambda: DeletionRunner(model, *a.values()))

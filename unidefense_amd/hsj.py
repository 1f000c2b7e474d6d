"""Decision-based minimum-norm attack (HopSkipJump; Chen, Jordan and Wainwright 2020) from the model's hard label alone:
HSJRunner, hsj_runner, hsj_key, the schedule helpers hsj_probe_counts / hsj_queries / hsj_constants and the numpy restatements
ref_hsj, ref_hsj_propose, ref_hsj_estimate.

A verification service answers "real" or "fake" and nothing else.  Every other runner here reads more than that: the gradient
attacks differentiate the frozen backward, Square and the spatial search read the logit margin.  This one sees one bit per
forward — argmax != y — so it depends neither on the backward nor on the logits' scale: gradient masking or a saturated margin
hides from those runners and shows up here.  Like FMN it is a minimum-norm attack: it returns per-sample radii, which robust_curve
and test_robust's "eps" scoring consume.

All samples move in lock step through ONE schedule that the host knows in advance (hsj_queries); only values are per-sample
state on the device (csrc/hsj.hip, the rows of include/unidefense_hip.h).  With D = 3 size^2, (lo, hi) = clip, x0 the clean input:
  1. clean query at x0: where argmax != y the radius is 0 and the sample is done.
  2. start: one query at x_init where given; then up to init_trials queries at a uniform image in [lo, hi] for the samples still
     without an adversarial start (samples without one stay idle and return inf).
  3. bisection: `bisect` queries on alpha between x0 and x_cur (L2: x0 + alpha (x_cur - x0), alpha in [0, 1]; Linf: x_cur
     projected onto the alpha-box around x0, alpha in [0, |x_cur - x0|inf]); x_bd settles at the adversarial end, which has
     always been verified (if the end never moved, x_bd is x_cur itself).
  4. dist = the measured norm of x_bd - x0 (double); where it is below the best so far x_bd becomes x_adv; x_cur = x_bd.
  5. B_t = min(max_probes, floor(probes sqrt(t + 1))) probe queries at clamp(x_bd + delta u_b): u_b Philox uniform in (-1, 1)
     (Linf) or Philox Gaussian / sqrt(D) (L2); delta = 0.1 (hi - lo) at t = 0, dist / D afterwards, never below 2^-20 (hi - lo)
     (times sqrt(D) for L2).  The draw index is one counter for the whole call.
  6. v = sum_b (phi_b - mean phi) u_b in ascending b (all phi equal: +-sum u_b); the direction is sign(v) or v / |v|.
  7. step search: xi = dist / sqrt(t + 1), up to `halvings` queries at clamp(x_bd + xi dir); the first adversarial one becomes
     x_cur, otherwise xi halves; never a success: x_cur stays x_bd.
  8. back to 3; after the last iteration a closing bisection and step 4 once more.
Departures from the paper, both stated in DESIGN: an L2 direction is z / sqrt(D), not z / |z| (a probe is then one pass without
a reduction; only the probe's sign is used), and delta has a floor (at 256^2 dist / D / sqrt(D) per component is below one fp32
ulp of a pixel: the perturbation would be decided by rounding).

The B directions of an estimate never exist in memory: ud_hsj_estimate re-makes them in registers from the Philox counter
(seed, id, draw, element) that the probes used.  ids keys the noise, so a sample's attack is a function of (seed, id, the model's
decisions) and not of its row or of N.
"""
import math

import numpy as np
import torch

from .attack import _arguments, _cached_runner, _detached, _key, _refuse_clip, _refuse_count, _Runner
from .infer import _eval_nodes
from .smooth import _refuse_logits, _refuse_seed, ref_smooth_unit

NORMS = ("l2", "linf")
_NOISE_OF = {"l2": "gaussian", "linf": "uniform"}
_F32 = np.float32


# ---- the schedule: what the host knows in advance --------------------------------------------------------------------------------
def hsj_probe_counts(steps, probes, max_probes):
    """[B_0 .. B_{steps-1}], B_t = min(max_probes, floor(probes sqrt(t + 1))), in exact integers"""
    return [min(int(max_probes), math.isqrt(int(probes) * int(probes) * (t + 1))) for t in range(int(steps))]


def hsj_queries(steps, probes, max_probes, bisect, halvings, init_trials, x_init=False):
    """The number of forwards of one call: 1 (clean) + 1 (x_init) + init_trials + (steps + 1) bisect + sum B_t + steps halvings"""
    return (1 + int(bool(x_init)) + int(init_trials) + (int(steps) + 1) * int(bisect) + sum(hsj_probe_counts(steps, probes, max_probes))
            + int(steps) * int(halvings))


def hsj_constants(per, norm, steps, clip):
    """The fp32 constants of a run as numpy float32: delta0 = 0.1 (hi - lo), inv_d = 1 / D, dfloor = 2^-20 (hi - lo) (times sqrt(D)
    for L2), aux = 1 / sqrt(D), xis[t] = 1 / sqrt(t + 1); each computed in float64 and rounded once."""
    lo, hi = float(_F32(clip[0])), float(_F32(clip[1]))
    return {"lo": _F32(lo), "hi": _F32(hi), "delta0": _F32(0.1 * (hi - lo)), "inv_d": _F32(1.0 / per),
            "dfloor": _F32(2.0 ** -20 * (hi - lo) * (math.sqrt(per) if norm == "l2" else 1.0)), "aux": _F32(1.0 / math.sqrt(per)),
            "xis": np.array([1.0 / math.sqrt(t + 1) for t in range(int(steps))], dtype=np.float64).astype(np.float32)}


# ---- numpy restatements ---------------------------------------------------------------------------------------------------------------
def _clamp(v, lo, hi):
    """the kernels' NaN-transparent clamp: v < lo ? lo : v, then v > hi ? hi : v"""
    v = np.where(v < lo, lo, v)
    return np.where(v > hi, hi, v)


def ref_hsj_propose(mode, norm, a, b, s, t, lo, hi, plain=None):
    """One pass of ud_hsj_propose on the rows that take part, restated: a, b, t [n, per], s [n] (the pass's per-sample scalar),
    plain [n] bool ("settle": the rows whose upper end never moved).  float32 in, one rounding per operation, bitwise the kernel
    ("probe" with a float64 t: the whole expression in float64 at the fp32 values of a and s: the yardstick of the Gaussian
    probe)."""
    exact = t is not None and np.asarray(t).dtype == np.float64
    f = np.float64 if exact else np.float32
    lo, hi = f(lo), f(hi)
    if mode in ("copy", "copy_seek"):
        return np.array(a, dtype=np.float32)
    if mode == "noise":
        mid, half = _F32(0.5) * (_F32(lo) + _F32(hi)), _F32(0.5) * (_F32(hi) - _F32(lo))
        return _clamp(mid + half * np.asarray(t, np.float32), _F32(lo), _F32(hi)).astype(np.float32)
    s = np.asarray(s, dtype=np.float32).reshape(-1, 1)
    if mode in ("bisect", "settle"):
        a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
        if norm == "linf":
            out = _clamp(_clamp(a, b - s, b + s), _F32(lo), _F32(hi))
        else:
            out = _clamp(b + s * (a - b), _F32(lo), _F32(hi))
        if mode == "settle":
            out = np.where(np.asarray(plain, bool).reshape(-1, 1), a, out)
        return out.astype(np.float32)
    if mode == "probe":
        return _clamp(np.asarray(a, np.float32).astype(f) + s.astype(f) * np.asarray(t).astype(f), lo, hi).astype(f)
    if mode == "step":
        return _clamp(np.asarray(a, np.float32) + s * np.asarray(b, np.float32), _F32(lo), _F32(hi)).astype(np.float32)
    raise ValueError(f"unknown mode {mode!r}")


def _weights(phi):
    """float32 [B, n]: phi_b - mean phi with mean = float32(ones) * float32(1 / B); all equal: +1 (all ones) or -1 (all zeros)"""
    phi = np.asarray(phi) != 0
    B = phi.shape[0]
    ones = phi.sum(0)
    mean = ones.astype(np.float32) * (_F32(1.0) / _F32(B))
    w = phi.astype(np.float32) - mean[None, :]
    return np.where(ones[None, :] == B, _F32(1.0), np.where(ones[None, :] == 0, _F32(-1.0), w)).astype(np.float32)


def _estimate(phi, units, norm, exact=False):
    f = np.float64 if exact else np.float32
    w = _weights(phi).astype(f)
    acc = np.zeros(units[0].shape, dtype=f)
    for b, u in enumerate(units):                                # ascending b, one product and one add per term
        acc = acc + w[b][:, None] * np.asarray(u).astype(f)
    return np.sign(acc).astype(np.float32) if norm == "linf" else acc


def ref_hsj_estimate(phi, ids, draw0, per, norm, seed, exact=False):
    """ud_hsj_estimate restated for phi [B, n] (0 / 1), ids [n]: v [n, per] = sum_b w_b u_b in ascending b, u_b the unit noise of
    draw draw0 + b.  "linf": float32 and bitwise the kernel (the sign of the sum).  "l2": u_b from float64 library functions;
    exact=False rounds each u_b to float32 and sums in float32 (what the kernel does: its Box-Muller is in double too and rounded
    once, so its fp32 directions are these but for about one element in 10^8), exact=True keeps everything in float64 (the
    yardstick)."""
    phi = np.asarray(phi)
    units = (ref_smooth_unit(ids, draw0 + b, per, _NOISE_OF[norm], seed) for b in range(phi.shape[0]))
    if norm == "l2" and not exact:
        units = (u.astype(np.float32) for u in units)
    return _estimate(phi, list(units), norm, exact and norm == "l2")


def ref_hsj(decide, x, y, ids=None, norm="l2", steps=20, probes=100, max_probes=1000, bisect=12, halvings=10, init_trials=16,
            seed=0, clip=(-1.0, 1.0), x_init=None):
    """The whole schedule in numpy.  decide(x_try [N, ...] float32) -> the predicted class per sample (int [N]; -1: the row was
    invalid, which counts as not adversarial and sets bit 0 of flags).  Rows of x_try that a query does not use keep their last
    content, as on the device.  Returns a dict: radius, found, x_adv, queries, history, decisions, flags, plus dist (the last
    settled distance) — what HSJRunner leaves, as numpy arrays."""
    x = np.asarray(x, dtype=np.float32)
    shape, N = x.shape, x.shape[0]
    x0 = x.reshape(N, -1)
    per = x0.shape[1]
    y = np.asarray(y).reshape(N)
    ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    c = hsj_constants(per, norm, steps, clip)
    lo, hi = c["lo"], c["hi"]
    counts = hsj_probe_counts(steps, probes, max_probes)
    Q = hsj_queries(steps, probes, max_probes, bisect, halvings, init_trials, x_init is not None)
    decisions = np.full((Q, N), -1, dtype=np.int8)
    history = np.zeros((steps + 1, N), dtype=np.float32)
    queries, flags = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    x_try, x_cur, x_bd, v = (np.zeros_like(x0) for _ in range(4))
    x_adv = x0.copy()
    has = np.zeros(N, dtype=bool)
    best = np.full(N, np.inf, dtype=np.float32)
    dist = np.zeros(N, dtype=np.float32)
    k = draw = 0

    def judge(part):
        nonlocal k
        cls = np.asarray(decide(x_try.reshape(shape))).reshape(N)
        valid = cls >= 0
        bit = valid & (cls != y)
        flags[part & ~valid] |= 1
        queries[part] += 1
        decisions[k] = np.where(part, bit.astype(np.int8), -1)
        k += 1
        return bit & part

    def unit(rows, mode):
        return ref_smooth_unit(ids[rows], draw, per, mode, seed).astype(np.float32)

    def norms(a):
        d = a.astype(np.float64) - x0.astype(np.float64)
        return np.sqrt((d * d).sum(1)), np.abs(d).max(1)

    # 1. the clean query
    x_try[:] = x0
    done0 = judge(np.ones(N, dtype=bool))
    active = ~done0
    # 2. the start
    if x_init is not None:
        seek = active & ~has
        x_try[seek] = np.asarray(x_init, dtype=np.float32).reshape(N, -1)[seek]
        got = judge(seek)
        has |= got
        x_cur[got] = x_try[got]
    for _ in range(init_trials):
        seek = active & ~has
        if seek.any():
            x_try[seek] = ref_hsj_propose("noise", norm, None, None, None, unit(seek, "uniform"), lo, hi)
        got = judge(seek)
        has |= got
        x_cur[got] = x_try[got]
        draw += 1
    live = active & has
    n = int(live.sum())
    for t in range(steps + 1):
        # 3. bisection
        a_lo = np.zeros(N, dtype=np.float32)
        a_hi = np.ones(N, dtype=np.float32) if norm == "l2" else norms(x_cur)[1].astype(np.float32)
        moved = np.zeros(N, dtype=bool)
        for _ in range(bisect):
            mid = _F32(0.5) * (a_lo + a_hi)
            if n:
                x_try[live] = ref_hsj_propose("bisect", norm, x_cur[live], x0[live], mid[live], None, lo, hi)
            bit = judge(live)
            a_hi = np.where(bit, mid, a_hi)
            a_lo = np.where(live & ~bit, mid, a_lo)
            moved |= bit
        if n:
            x_bd[live] = ref_hsj_propose("settle", norm, x_cur[live], x0[live], a_hi[live], None, lo, hi, plain=~moved[live])
        # 4. the distance, keep-best
        l2, linf = norms(x_bd)
        dist = np.where(live, (l2 if norm == "l2" else linf).astype(np.float32), dist).astype(np.float32)
        keep = live & (dist < best)
        best = np.where(keep, dist, best)
        x_adv[keep] = x_bd[keep]
        x_cur[live] = x_bd[live]
        history[t] = np.where(live, best, np.where(done0, _F32(0.0), _F32(np.inf)))
        if t == steps:
            break
        d = np.full(N, c["delta0"], dtype=np.float32) if t == 0 else dist * c["inv_d"]
        delta = np.where(d > c["dfloor"], d, c["dfloor"]).astype(np.float32)
        xi = (dist * c["xis"][t]).astype(np.float32)
        # 5. probes
        B = counts[t]
        phi = np.zeros((B, N), dtype=np.int8)
        units = []
        s = delta * c["aux"] if norm == "l2" else delta
        for b in range(B):
            if n:
                units.append(unit(live, _NOISE_OF[norm]))
                x_try[live] = ref_hsj_propose("probe", norm, x_bd[live], None, s[live], units[-1], lo, hi)
            phi[b] = judge(live)
            draw += 1
        # 6. the estimate
        invn = np.ones(N, dtype=np.float32)
        if n:
            v[live] = _estimate(phi[:, live], units, norm)
            if norm == "l2":
                ss = (v.astype(np.float64) ** 2).sum(1)
                invn = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32)
        # 7. the step search
        done = np.zeros(N, dtype=bool)
        for _ in range(halvings):
            part = live & ~done
            if part.any():
                sc = xi * invn if norm == "l2" else xi
                x_try[part] = ref_hsj_propose("step", norm, x_bd[part], v[part], sc[part], None, lo, hi)
            got = judge(part)
            done |= got
            x_cur[got] = x_try[got]
            xi = np.where(part & ~got, _F32(0.5) * xi, xi).astype(np.float32)
    assert k == Q
    radius = history[steps].copy()
    return {"radius": radius, "found": np.isfinite(radius), "x_adv": x_adv.reshape(shape), "queries": queries, "history": history,
            "decisions": decisions, "flags": flags, "dist": dist}


# ---- the runner ------------------------------------------------------------------------------------------------------------------
class HSJRunner(_Runner):
    """runner = HSJRunner(model, batch, size, norm="l2", steps=20, probes=100, ...); radius = runner(x, y[, ids, x_init]).

    HopSkipJump on the hard label of every sample of x (cuda fp32 [batch, 3, size, size], y int64 [batch]): per sample the
    smallest L2 / Linf perturbation found that changes argmax.  ids (int64 [batch], default arange): each sample's noise stream —
    the attack on a sample is a function of (seed, id, the model's decisions), whatever its row or the batch's size.  x_init
    (like x, optional): a start point per sample, used where the model labels it differently from y; otherwise, and for the rest,
    init_trials uniform images are tried.  logits: a callable (out, x_try) -> [batch, C] fp32, default out["cls_out"]; only
    argmax of it reaches the attack (ud_hsj_control turns the row into one bit as its first act).

    One hipGraph per query kind — clean, init, noise, bisect, probe, step — each holding ud_hsj_propose(mode), the eval forward
    (InferenceRunner's, in either precision, under no_grad), the logits and ud_hsj_control(mode) (and the ud_apgd_keep that adopts
    an accepted point).  The host replays them by the schedule and launches the settle pass, ud_hsj_dist, ud_hsj_estimate and the
    keep-best copies between phases; there is no host-device synchronisation inside a call.  Call 1 runs the same launches
    eagerly, call 2 captures, later calls replay.  Nothing is frozen and there is no tape.

    What the next call overwrites: radius [N] fp32 (returned: the norm of x_adv - x measured on the device in double; 0 for a
    sample that is already misclassified, inf where no adversarial start was found), found [N] bool (radius < inf), x_adv (x where
    not found or where the radius is 0), queries [N] int32 (forwards that counted for the sample), history [steps + 1, N] (the
    best boundary distance after the first bisection and after every iteration: non-increasing), decisions [Q, N] int8 (one row
    per replayed query: 1 adversarial, 0 not, -1 the sample took no part), flags [N] int32 (bit 0: a counted query had a
    non-finite logit; it counted as not adversarial), out (the last forward's output); args: the resolved arguments."""
    _what = "HSJRunner"
    _backward = False

    def __init__(self, model, batch, size, norm="l2", steps=20, probes=100, max_probes=1000, bisect=12, halvings=10,
                 init_trials=16, seed=0, clip=(-1.0, 1.0), precision="fp32", logits=None, targeted=False):
        def arguments():
            from .lib import const
            if norm not in NORMS:
                raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")
            if targeted:
                raise ValueError("HSJRunner is untargeted: the targeted HopSkipJump is not built")
            for name, v, least in (("steps", steps, 1), ("probes", probes, 1), ("max_probes", max_probes, 1), ("bisect", bisect, 1),
                                   ("halvings", halvings, 1), ("init_trials", init_trials, 0)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")
                _refuse_count(name, v, least)
            if max_probes > const("UD_HSJ_MAX_PROBES"):
                raise ValueError(f"max_probes must be at most {const('UD_HSJ_MAX_PROBES')} (the estimate's weights live in LDS), "
                                 f"got {max_probes!r}")
            if hsj_queries(steps, probes, max_probes, bisect, halvings, init_trials, True) * int(batch) >= 1 << 31:
                raise ValueError("the schedule's queries times the batch must stay below 2^31")
            _refuse_seed(seed)
            _refuse_clip(clip)
            if not all(math.isfinite(float(c)) for c in clip):
                raise ValueError(f"clip must be finite, got {clip!r}")
            _refuse_logits(logits)
        self._init_model(model, batch, size, precision, arguments)
        self.norm, self.steps, self.probes, self.max_probes = norm, int(steps), int(probes), int(max_probes)
        self.bisect, self.halvings, self.init_trials, self.seed = int(bisect), int(halvings), int(init_trials), int(seed)
        self.logits = logits
        self.per = 3 * self.size * self.size
        self.k = hsj_constants(self.per, norm, self.steps, clip)
        self.lo, self.hi = float(self.k["lo"]), float(self.k["hi"])
        self.counts = hsj_probe_counts(self.steps, self.probes, self.max_probes)
        self.args = {"method": "hsj", "norm": norm, "steps": self.steps, "probes": self.probes, "max_probes": self.max_probes,
                     "bisect": self.bisect, "halvings": self.halvings, "init_trials": self.init_trials, "seed": self.seed,
                     "clip": (self.lo, self.hi), "logits": None if logits is None else getattr(logits, "__name__", repr(logits)),
                     "precision": self.precision}
        self.graphs = None
        self.x0 = self.x_adv = self.radius = self.found = self.queries = self.history = self.decisions = self.flags = None

    def queries_of(self, x_init=False):
        """the number of forwards of one call: the rows of `decisions`"""
        return hsj_queries(self.steps, self.probes, self.max_probes, self.bisect, self.halvings, self.init_trials, x_init)

    def _buffers(self, x, y):
        from . import kernels as K
        n, dev = self.batch, self.device
        self.x0 = x.detach().clone().contiguous()
        self.x_start, self.x_try, self.x_cur, self.x_bd, self.x_adv, self.v = (torch.zeros_like(self.x0) for _ in range(6))
        self.y = y.detach().clone()
        self.ids = torch.zeros(n, dtype=torch.int64, device=dev)
        self.ist, self.fst, self._nrm, self._phi, self._decisions, self.history = K.hsj_state(
            n, self.queries_of(True), self.steps, self.max_probes, dev)
        self._xis = torch.from_numpy(self.k["xis"]).to(dev)
        self._accept, self._keep = self.ist[K.HSJ_I["accept"]], self.ist[K.HSJ_I["keep"]]
        self.queries, self.flags = self.ist[K.HSJ_I["queries"]], self.ist[K.HSJ_I["flags"]]
        self.radius = self.fst[K.HSJ_F["radius"]]
        # kind -> (propose mode, a, b, control mode)
        # (a call's last forward is a bisection query: captured last, so that `out` is that graph's output)
        self._kinds = {"clean": ("copy", self.x0, None, "clean"), "init": ("copy_seek", self.x_start, None, "start"),
                       "noise": ("noise", None, None, "start_noise"), "probe": ("probe", self.x_bd, None, "probe"),
                       "step": ("step", self.x_bd, self.v, "step"), "bisect": ("bisect", self.x_cur, self.x0, "bisect")}

    def _logits(self, out):
        z = out["cls_out"] if self.logits is None else self.logits(out, self.x_try)
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[0] != self.batch or z.shape[1] < 1:
            raise ValueError(f"{self._what}'s logits must be a [{self.batch}, C] tensor, got "
                             f"{tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__}")
        return z.detach().float().contiguous()

    def _propose(self, mode, dst, a, b):
        from . import kernels as K
        K.hsj_propose(mode, self.norm, dst, a, b, self.ids, self.ist, self.fst, self.lo, self.hi, self.seed)

    def _control(self, mode, logits=None):
        from . import kernels as K
        K.hsj_control(mode, self.norm, self.ist, self.fst, logits=logits, y=self.y, nrm=self._nrm, phi=self._phi,
                      decisions=self._decisions, history=self.history, xis=self._xis, delta0=float(self.k["delta0"]),
                      inv_d=float(self.k["inv_d"]), dfloor=float(self.k["dfloor"]))

    def _query(self, kind):
        """one query of `kind` on the static buffers: what a graph holds"""
        from . import kernels as K
        pmode, a, b, cmode = self._kinds[kind]
        self._propose(pmode, self.x_try, a, b)
        with torch.no_grad(), _eval_nodes(self.model, self.half):
            out = self.model(self.x_try)
            z = self._logits(out)
        self.out = _detached(out)
        self._control(cmode, z)
        if cmode in ("start", "start_noise", "step"):
            K.apgd_keep(self.x_cur, self.x_try, self._accept)     # the accepted point becomes x_cur

    def _run(self, kind, times=1):
        for _ in range(times):
            if self.graphs is None:
                self._query(kind)
            else:
                self.graphs[kind].replay()

    def _check_like(self, t, name):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or tuple(t.shape) != self.shape or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a cuda fp32 tensor {self.shape}, got {getattr(t, 'dtype', type(t).__name__)} "
                             f"{tuple(getattr(t, 'shape', ()))}")

    def __call__(self, x, y, ids=None, x_init=None):
        from . import kernels as K
        from .smooth import CertifyRunner
        self._check(x, y)
        ids = CertifyRunner._ids(ids, self.batch, self.device)
        if x_init is not None:
            self._check_like(x_init, "x_init")
        self.calls += 1
        if self.calls == 1:                                       # eager warm-up: the same launches, a valid attack
            self._buffers(x, y)
        elif self.graphs is None:
            kinds = list(self._kinds)
            self.graphs = dict(zip(kinds, self._capture(*(lambda kind=kind: self._query(kind) for kind in kinds))))
        with torch.no_grad():
            self.x0.copy_(x)
            self.x_adv.copy_(x)
            self.y.copy_(y)
            self.ids.copy_(ids)
            self.ist.zero_()
            self.fst.zero_()
            self._decisions.fill_(-1)
            if x_init is not None:
                self.x_start.copy_(x_init)
        self._run("clean")
        if x_init is not None:
            self._run("init")
        self._run("noise", self.init_trials)
        draw = self.init_trials
        for t in range(self.steps + 1):
            K.hsj_dist(self.x_cur, self.x0, self._nrm, self.ist)
            self._control("begin")
            self._run("bisect", self.bisect)
            self._propose("settle", self.x_bd, self.x_cur, self.x0)
            K.hsj_dist(self.x_bd, self.x0, self._nrm, self.ist)
            self._control("dist")
            K.apgd_keep(self.x_adv, self.x_bd, self._keep)        # keep-best: history is non-increasing by construction
            K.apgd_keep(self.x_cur, self.x_bd, self._accept)      # the next search starts from the boundary point
            if t == self.steps:
                break
            B = self.counts[t]
            self._run("probe", B)
            K.hsj_estimate(self.v, self._phi, self.ids, B, draw, self.norm, self.seed, self.ist)
            draw += B
            if self.norm == "l2":
                K.hsj_dist(self.v, None, self._nrm, self.ist)
            self._control("vnorm")
            self._run("step", self.halvings)
        self.decisions = self._decisions[:self.queries_of(x_init is not None)]
        self.found = torch.isfinite(self.radius)
        return self.radius


_hsj_arguments = _arguments(HSJRunner)


def _hsj_key_arguments(a):
    if a.pop("targeted"):
        raise ValueError("HSJRunner is untargeted: the targeted HopSkipJump is not built")
    return dict(a, logits=None if a["logits"] is None else id(a["logits"]))


def hsj_key(*args, **kwargs):
    """arguments: HSJRunner's after the model; no loss scale: an fp16 runner's key carries (precision,); a callable `logits` is
    keyed by identity"""
    return _key(_hsj_key_arguments(_hsj_arguments(*args, **kwargs)))


def hsj_runner(model, *args, **kwargs):
    """The model's HSJRunner for the full argument tuple (HSJRunner's after the model), made on first use; at most _MAX_RUNNERS
    are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _hsj_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_hsj_runners", _hsj_key_arguments(dict(a)), lambda: HSJRunner(model, *a.values()))

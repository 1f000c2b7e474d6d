"""CPU: the Square attack (unidefense_amd/attack.py: SquareRunner; csrc/square.hip) — the window schedule, the draws, what the
runner and the entry points refuse before any GPU work, the accessor's cache — and the restatement of the algorithm that
tests/test_m_square_gpu.py compares the kernels and the runner against: ref_square_control (pure Python on Python floats, the
per-sample state machine), ref_square_propose (torch in the dtype of its inputs, operation by operation) and ref_square (the
whole attack on any per-sample objective)."""
import ctypes
import math

import pytest
import torch

UD_EINVAL = -1000
MODELS = ("UDEB4", "UDR18", "UDR50")
THRESHOLDS = (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000)


# ---- the definition, restated ------------------------------------------------------------------------------------------------
def ref_square_sizes(steps, size, p_init):
    """proposal j = 0 .. steps - 1 is evaluated by iteration k = j + 1: it = (k 10000) // steps, the fraction p_init is halved
    once per threshold that `it` exceeds, the side is the rounded square root of the fraction of the image, inside [1, size]"""
    out = []
    for k in range(1, steps + 1):
        it = (k * 10000) // steps
        p = p_init
        for t in THRESHOLDS:
            if it > t:
                p = p / 2
        out.append(min(max(int(math.floor(math.sqrt(p * size * size) + 0.5)), 1), size))
    return tuple(out)


class ref_square_control:
    """The per-sample state machine of one restart, in pure Python on Python floats (an fp32 value is exactly a Python float and
    only comparisons are made, so on fp32 inputs every array equals the kernel's).  step(f) consumes f_k for k = 0, 1, ...;
    past k = steps it changes nothing."""

    def __init__(self, N, steps, early_stop=True):
        self.N, self.steps, self.early_stop = N, steps, early_stop
        self.k = 0
        self.f_best = [0.0] * N
        self.accepted, self.active, self.queries = [0] * N, [0] * N, [0] * N
        self.history = [[0.0] * N for _ in range(steps + 1)]
        self.decisions = [[0] * N for _ in range(steps + 1)]

    def step(self, f):
        k = self.k
        if k > self.steps:
            return list(self.accepted)
        for n in range(self.N):
            fk = f[n]
            if k == 0:
                self.f_best[n], self.accepted[n], self.queries[n] = fk, 0, 1
            else:
                self.queries[n] += self.active[n]
                self.accepted[n] = 1 if self.active[n] and fk < self.f_best[n] else 0
                if self.accepted[n]:
                    self.f_best[n] = fk
            self.active[n] = (1 if self.f_best[n] > 0 else 0) if self.early_stop else 1
            self.history[k][n] = fk
            self.decisions[k][n] = self.accepted[n]
        self.k = k + 1
        return list(self.accepted)


def ref_square_propose(x_try, x_best, x0, k, accepted, sizes, h, w, sign, eps, lo, hi, closing=False):
    """What one ud_square_propose launch leaves in (x_try, x_best), in the dtype of the inputs, one torch operation per arithmetic
    operation: sample n with counter k[n] settles the window of proposal k[n] - 1 (row k[n] - 2 of the draws) by accepted[n], then,
    unless closing, writes the window of proposal k[n] (row k[n] - 1): clamp(x0 + sign eps, lo, hi).  k: an int or one per sample."""
    x_try, x_best = x_try.clone(), x_best.clone()
    N, steps = x_try.shape[0], len(sizes)
    ks = [k] * N if isinstance(k, int) else list(k)
    for n in range(N):
        kk = ks[n]
        if 2 <= kk <= steps + 1:
            s, r, c = sizes[kk - 2], int(h[kk - 2][n]), int(w[kk - 2][n])
            if accepted[n]:
                x_best[n, :, r:r + s, c:c + s] = x_try[n, :, r:r + s, c:c + s]
            else:
                x_try[n, :, r:r + s, c:c + s] = x_best[n, :, r:r + s, c:c + s]
        if not closing and 1 <= kk <= steps:
            s, r, c = sizes[kk - 1], int(h[kk - 1][n]), int(w[kk - 1][n])
            inc = torch.as_tensor(sign[kk - 1][n], dtype=x_try.dtype).reshape(3, 1, 1) * eps
            x_try[n, :, r:r + s, c:c + s] = torch.clamp(x0[n, :, r:r + s, c:c + s] + inc, lo, hi)
    return x_try, x_best


def ref_square(f, x, eps, steps, draws, p_init=0.8, lo=-1.0, hi=1.0, early_stop=True, decisions=None):
    """One restart of the whole attack on f(x) -> [N] per-sample values (minimised), in x's dtype, from the draws
    (sign0, h, w, sign) of square_draws.  decisions [steps + 1][N] given: they are applied instead of f's own (f may be None)."""
    sign0, h, w, sign = draws
    N, size = x.shape[0], x.shape[-1]
    sizes = ref_square_sizes(steps, size, p_init)
    start = torch.clamp(x + sign0.to(x.dtype).unsqueeze(2) * eps, lo, hi)
    x_try, x_best = start.clone(), start.clone()
    ctl = ref_square_control(N, steps, early_stop)
    accepted = [0] * N
    for k in range(steps + 1):
        x_try, x_best = ref_square_propose(x_try, x_best, x, k, accepted, sizes, h, w, sign, eps, lo, hi)
        if decisions is None:
            accepted = ctl.step([float(v) for v in f(x_try)])
        else:
            accepted = [int(v) for v in decisions[k]]
    x_try, x_best = ref_square_propose(x_try, x_best, x, steps + 1, accepted, sizes, h, w, sign, eps, lo, hi, closing=True)
    assert torch.equal(x_try, x_best) or bool(torch.isnan(x_try).any())
    return {"x_adv": x_best, "start": start, "best_loss": list(ctl.f_best), "history": ctl.history, "decisions": ctl.decisions,
            "queries": list(ctl.queries)}


# ---- the schedule and the draws ----------------------------------------------------------------------------------------------
def test_square_sizes():
    from unidefense_amd.attack import square_sizes
    assert square_sizes(20, 128, 0.8) == (40, 29, 20, 20, 14, 14, 14, 14, 10, 10, 10, 10, 7, 7, 7, 7, 5, 5, 5, 5)
    for steps, size, p in ((1, 8, 0.8), (5, 17, 1.0), (20, 128, 0.8), (100, 256, 0.8), (5000, 256, 0.8), (5000, 224, 0.05),
                           (7, 3, 0.3), (10000, 32, 0.1), (12345, 380, 0.8)):
        got = square_sizes(steps, size, p)
        assert got == ref_square_sizes(steps, size, p), (steps, size, p)
        assert len(got) == steps and all(1 <= s <= size for s in got)
        assert all(a >= b for a, b in zip(got, got[1:]))                    # the window never grows
    assert square_sizes(5000, 256, 0.8)[0] == 229 and square_sizes(5000, 256, 0.8)[-1] == 10
    assert set(square_sizes(50, 4, 0.01)) == {1}                            # never below one pixel


def test_square_draws_are_reproducible_and_inside_the_image():
    from unidefense_amd.attack import square_draws, square_sizes
    for steps, batch, size, p in ((20, 3, 17, 0.8), (5, 1, 8, 1.0), (200, 4, 64, 0.3)):
        a = square_draws(steps, batch, size, p, torch.Generator().manual_seed(7))
        b = square_draws(steps, batch, size, p, torch.Generator().manual_seed(7))
        c = square_draws(steps, batch, size, p, torch.Generator().manual_seed(8))
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert not all(torch.equal(u, v) for u, v in zip(a, c))
        sign0, h, w, sign = a
        assert tuple(sign0.shape) == (batch, 3, size) and tuple(sign.shape) == (steps, batch, 3)
        assert tuple(h.shape) == (steps, batch) and tuple(w.shape) == (steps, batch)
        assert sign0.dtype == torch.float32 and sign.dtype == torch.float32 and h.dtype == torch.int64 and w.dtype == torch.int64
        assert bool((sign0.abs() == 1).all()) and bool((sign.abs() == 1).all())
        room = size - torch.tensor(square_sizes(steps, size, p)).reshape(-1, 1)
        assert bool((h >= 0).all()) and bool((w >= 0).all()) and bool((h <= room).all()) and bool((w <= room).all())
    # the documented order: sign0, the uniforms of h, the uniforms of w, sign
    g = torch.Generator().manual_seed(3)
    s0 = torch.randint(0, 2, (2, 3, 9), generator=g).float() * 2 - 1
    room = 9 - torch.tensor(square_sizes(4, 9, 0.5), dtype=torch.float64).reshape(-1, 1) + 1
    hh = torch.floor(torch.rand(4, 2, generator=g, dtype=torch.float64) * room).long()
    ww = torch.floor(torch.rand(4, 2, generator=g, dtype=torch.float64) * room).long()
    sg = torch.randint(0, 2, (4, 2, 3), generator=g).float() * 2 - 1
    got = square_draws(4, 2, 9, 0.5, torch.Generator().manual_seed(3))
    assert all(torch.equal(u, v) for u, v in zip(got, (s0, hh, ww, sg)))
    # with a full-size window there is one place only
    _, h, w, _ = square_draws(3, 5, 4, 1.0, torch.Generator().manual_seed(1))
    sizes = square_sizes(3, 4, 1.0)
    assert all(bool((h[j] <= 4 - sizes[j]).all()) and bool((w[j] <= 4 - sizes[j]).all()) for j in range(3))


def test_margin_objective():
    from unidefense_amd.attack import margin_each
    z = torch.tensor([[2.0, -1.0], [0.5, 0.75], [1.0, 1.0]])
    y = torch.tensor([0, 0, 1])
    assert margin_each({"cls_out": z}, y).tolist() == [3.0, -0.25, 0.0]
    z3 = torch.tensor([[2.0, -1.0, 2.5], [0.5, 0.75, 0.0]])
    assert margin_each({"cls_out": z3}, torch.tensor([0, 1])).tolist() == [-0.5, 0.25]
    z1 = torch.tensor([[2.0], [-0.5], [3.0]])
    assert margin_each({"cls_out": z1}, torch.tensor([1, 0, 0])).tolist() == [2.0, 0.5, -3.0]


# ---- the references on hand-made cases ---------------------------------------------------------------------------------------
def test_reference_control_on_hand_sequences():
    nan = float("nan")
    c = ref_square_control(4, 4)
    #            falls        tie / rise   crosses zero   NaN inside
    seq = [[3.0, 2.0, 1.0, -1.0],
           [2.0, 2.0, 0.5, nan],
           [1.0, 2.5, -0.5, -2.0],
           [0.5, 1.5, -1.0, -3.0],
           [0.75, 1.0, -2.0, -4.0]]
    for f in seq:
        c.step(f)
    assert c.decisions == [[0, 0, 0, 0], [1, 0, 1, 0], [1, 0, 1, 0], [1, 1, 0, 0], [0, 1, 0, 0]]
    assert c.f_best == [0.5, 1.0, -0.5, -1.0] and c.active == [1, 1, 0, 0]
    assert c.queries == [5, 5, 3, 1]                       # sample 2 stops counting once fooled, sample 3 starts fooled
    assert c.history[1][0] == 2.0 and math.isnan(c.history[1][3]) and c.k == 5
    before = (list(c.f_best), list(c.queries), [list(r) for r in c.history])
    c.step([-9.0] * 4)                                     # past the last iteration: nothing
    assert (c.f_best, c.queries, c.history) == before and c.k == 5
    # early_stop off: always active, a fooled sample keeps descending
    c = ref_square_control(1, 3, early_stop=False)
    for f in ([-1.0], [-2.0], [nan], [-3.0]):
        c.step(f)
    assert c.decisions == [[0], [1], [0], [1]] and c.queries == [4] and c.f_best == [-3.0] and c.active == [1]
    # a NaN start compares false everywhere: never active under early_stop, never replaced without it
    c = ref_square_control(1, 2)
    for f in ([nan], [1.0], [0.5]):
        c.step(f)
    assert c.decisions == [[0], [0], [0]] and c.queries == [1] and math.isnan(c.f_best[0])
    c = ref_square_control(1, 2, early_stop=False)
    for f in ([nan], [1.0], [0.5]):
        c.step(f)
    assert c.decisions == [[0], [0], [0]] and c.queries == [3] and math.isnan(c.f_best[0])


def test_reference_propose_on_hand_values():
    N, size, eps = 1, 4, 0.25
    x0 = torch.zeros(N, 3, size, size)
    x0[0, :, 3, 3] = 0.9                                    # the clip bound is met at one pixel
    start = torch.full_like(x0, 0.125)
    sizes, h, w = (2, 2, 4), [[0], [1], [0]], [[0], [1], [0]]
    sign = [[[1.0, -1.0, 1.0]], [[-1.0, -1.0, 1.0]], [[1.0, 1.0, 1.0]]]
    xt, xb = ref_square_propose(start, start, x0, 0, [0], sizes, h, w, sign, eps, -1.0, 1.0)
    assert torch.equal(xt, start) and torch.equal(xb, start)                    # k = 0: nothing
    xt, xb = ref_square_propose(xt, xb, x0, 1, [0], sizes, h, w, sign, eps, -1.0, 1.0)
    assert torch.equal(xb, start) and xt[0, :, 0, 0].tolist() == [0.25, -0.25, 0.25] and float(xt[0, 0, 2, 2]) == 0.125
    keep = xt.clone()
    # accepted: x_best takes the window; the next window overlaps it in one pixel
    at, ab = ref_square_propose(xt, xb, x0, 2, [1], sizes, h, w, sign, eps, -1.0, 1.0)
    assert torch.equal(ab[0, :, :2, :2], keep[0, :, :2, :2]) and float(ab[0, 0, 2, 2]) == 0.125
    assert at[0, :, 1, 1].tolist() == [-0.25, -0.25, 0.25] and at[0, :, 0, 0].tolist() == [0.25, -0.25, 0.25]
    out = at != ab
    assert bool(out[0, :, 1:3, 1:3].any()) and not bool(out[0, :, 0, :].any()) and not bool(out[0, :, 3, :].any())
    # rejected: x_try goes back, except where the next window writes
    rt, rb = ref_square_propose(xt, xb, x0, 2, [0], sizes, h, w, sign, eps, -1.0, 1.0)
    assert torch.equal(rb, start) and float(rt[0, 0, 0, 0]) == 0.125 and rt[0, :, 1, 1].tolist() == [-0.25, -0.25, 0.25]
    # the full-size window, clipped at the marked pixel; then the closing form settles it
    ft, fb = ref_square_propose(at, ab, x0, 3, [0], sizes, h, w, sign, eps, -1.0, 1.0)
    assert float(ft[0, 0, 3, 3]) == 1.0 and float(ft[0, 0, 0, 0]) == 0.25 and torch.equal(fb, ab)
    ct, cb = ref_square_propose(ft, fb, x0, 4, [1], sizes, h, w, sign, eps, -1.0, 1.0, closing=True)
    assert torch.equal(ct, ft) and torch.equal(cb, ft)
    ct, cb = ref_square_propose(ft, fb, x0, 4, [0], sizes, h, w, sign, eps, -1.0, 1.0, closing=True)
    assert torch.equal(ct, fb) and torch.equal(cb, fb)
    # the closing form at an earlier counter only settles: no new window
    ct, cb = ref_square_propose(xt, xb, x0, 2, [0], sizes, h, w, sign, eps, -1.0, 1.0, closing=True)
    assert torch.equal(cb, start) and torch.equal(ct, start)
    ct, cb = ref_square_propose(xt, xb, x0, 2, [1], sizes, h, w, sign, eps, -1.0, 1.0, closing=True)
    assert torch.equal(cb, keep) and torch.equal(ct, keep)


def _toy(t):
    """per-sample objective: the mean of the image times a per-sample weight plus a half — linear, so a proposal is kept exactly
    when its window's signed change lowers the weighted mean"""
    wgt = torch.tensor([1.0, -1.0, 0.5]).to(t.dtype)[: t.shape[0]]
    return 0.5 + wgt * t.flatten(1).mean(1)


def test_ref_square_on_a_linear_objective():
    from unidefense_amd.attack import square_draws
    x = (torch.rand(3, 3, 16, 16, generator=torch.Generator().manual_seed(2), dtype=torch.float64) - 0.5) * 0.5
    eps, steps = 0.1, 60
    draws = square_draws(steps, 3, 16, 0.8, torch.Generator().manual_seed(11))
    r = ref_square(_toy, x, eps, steps, draws, early_stop=False)
    xa = r["x_adv"]
    assert float((xa - x).abs().max()) <= eps + 1e-15 and float(xa.min()) >= -1.0 and float(xa.max()) <= 1.0
    assert bool(((xa - x).abs() > eps - 1e-12).all())                  # every pixel sits on a vertex of the box
    f0, f1 = _toy(r["start"]), _toy(xa)
    assert f1.tolist() == r["best_loss"] and bool((f1 < f0).all())
    assert r["queries"] == [steps + 1] * 3
    hist, dec = r["history"], r["decisions"]
    for n in range(3):
        best = hist[0][n]
        for k in range(1, steps + 1):
            assert dec[k][n] == (1 if hist[k][n] < best else 0)
            best = min(best, hist[k][n])
        assert sum(d[n] for d in dec) >= 1
    # given decisions are applied as they are: the same image without the objective
    again = ref_square(None, x, eps, steps, draws, early_stop=False, decisions=dec)
    assert torch.equal(again["x_adv"], xa)
    # early_stop: a sample that starts fooled is left at the start point and costs one query
    lo_x = x - 3.0 * torch.tensor([1.0, -1.0, 0.5]).reshape(3, 1, 1, 1)
    lo_x = lo_x.clamp(-0.9, 0.9)
    e = ref_square(_toy, lo_x, eps, steps, draws)
    fooled = [n for n in range(3) if e["history"][0][n] <= 0]
    assert fooled
    for n in fooled:
        assert e["queries"][n] == 1 and torch.equal(e["x_adv"][n], e["start"][n])
    # zero budget: the clamped input
    z = ref_square(_toy, x * 5.0, 0.0, 5, square_draws(5, 3, 16, 0.8, torch.Generator().manual_seed(1)))
    assert torch.equal(z["x_adv"], (x * 5.0).clamp(-1.0, 1.0))


# ---- entry points: argument checks come before any HIP call ------------------------------------------------------------------
def test_square_entry_points_reject_bad_arguments():
    from unidefense_amd import lib
    h = lib.load()
    b = ctypes.c_void_p(16)               # never dereferenced
    nan = float("nan")

    def propose(ptrs=(b,) * 8, N=2, size=16, steps=5, eps=0.1, lo=-1.0, hi=1.0, closing=0):
        return h.ud_square_propose(*ptrs, N, size, steps, eps, lo, hi, closing, None)
    for i in range(8):
        assert propose(ptrs=tuple(None if j == i else b for j in range(8))) == UD_EINVAL
        assert propose(ptrs=tuple(None if j == i else b for j in range(8)), closing=1) == UD_EINVAL
    assert propose(N=0) == UD_EINVAL and propose(N=-1) == UD_EINVAL and propose(N=65536) == UD_EINVAL
    assert propose(size=0) == UD_EINVAL and propose(size=-4) == UD_EINVAL and propose(steps=0) == UD_EINVAL
    assert propose(eps=-0.1) == UD_EINVAL and propose(eps=nan) == UD_EINVAL
    assert propose(lo=1.0, hi=-1.0) == UD_EINVAL and propose(lo=nan) == UD_EINVAL and propose(hi=nan) == UD_EINVAL

    def control(ptrs=(b,) * 5, N=4, steps=5, early=1):
        return h.ud_square_control(*ptrs, N, steps, early, None)
    for i in range(5):
        assert control(ptrs=tuple(None if j == i else b for j in range(5))) == UD_EINVAL
    assert control(N=0) == UD_EINVAL and control(N=-2) == UD_EINVAL and control(steps=0) == UD_EINVAL
    assert control(steps=-1, early=0) == UD_EINVAL


def test_square_entry_points_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K, lib
    names = sorted(header().protos)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in ("ud_square_propose", "ud_square_control"):
        assert n in names and n in lib.EXPORTED and hasattr(handle, n), n
    assert sorted(lib.EXPORTED) == names
    assert K.SQUARE_I == {"k": 0, "accepted": 1, "active": 2, "queries": 3} and K.SQUARE_F == {"f_best": 0}
    const = header().consts
    for name, row in list(K.SQUARE_I.items()) + list(K.SQUARE_F.items()):      # the name maps are the header's rows
        pre = "UD_SQUARE_I_" if name in K.SQUARE_I else "UD_SQUARE_F_"
        short = name.upper().replace("F_BEST", "BEST")
        assert const[f"{pre}{short}"] == row, (name, row)


# ---- the runner: refusals that need no GPU -----------------------------------------------------------------------------------
def _model(name):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    return load_model(name)(num_classes=2, drop_rate=0.5, **kw).eval()


@pytest.fixture(scope="module", params=MODELS)
def model(request):
    return _model(request.param)


@pytest.mark.parametrize("kw,match", [(dict(norm="l2", eps=0.1), "L2 Square attack is not built"), (dict(norm=None, eps=0.1), "norm"),
                                      (dict(eps=-1e-3), "eps"), (dict(eps=float("nan")), "eps"), (dict(), "eps"),
                                      (dict(eps=None), "eps"),
                                      (dict(eps=0.1, steps=0), "steps"), (dict(eps=0.1, steps=-3), "steps"),
                                      (dict(eps=0.1, steps=2.5), "steps"),
                                      (dict(eps=0.1, restarts=0), "restarts"), (dict(eps=0.1, restarts=-1), "restarts"),
                                      (dict(eps=0.1, restarts=1.5), "restarts"),
                                      (dict(eps=0.1, check_every=-1), "check_every"), (dict(eps=0.1, check_every=2.5), "check_every"),
                                      (dict(eps=0.1, p_init=0.0), "p_init"), (dict(eps=0.1, p_init=1.01), "p_init"),
                                      (dict(eps=0.1, p_init=-0.5), "p_init"), (dict(eps=0.1, p_init=float("nan")), "p_init"),
                                      (dict(eps=0.1, clip=(1.0, -1.0)), "clip"), (dict(eps=0.1, clip=(0.0, 0.0)), "clip"),
                                      (dict(eps=0.1, clip=(0.0,)), "clip"),
                                      (dict(eps=0.1, objective="hinge"), "objective")])
def test_square_runner_refuses_bad_arguments(model, kw, match):
    from unidefense_amd.attack import SquareRunner, square_runner
    for make in (lambda: SquareRunner(model, 2, 64, **kw), lambda: square_runner(model, 2, 64, **kw),
                 lambda: model.square_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=match):
            make()
    assert not model.__dict__.get("_ud_square_runners")


def test_square_runner_allows_what_it_should_and_refuses_the_rest(model):
    """every allowed combination gets as far as the device check; training mode, a foreign model and a CPU model are refused"""
    from unidefense_amd.attack import SquareRunner
    for kw in (dict(eps=0.1), dict(eps=0.0, steps=1), dict(eps=0.1, p_init=1.0, restarts=3), dict(eps=0.1, check_every=10),
               dict(eps=0.1, early_stop=False, objective="cross_entropy"), dict(eps=0.1, norm="linf", clip=(0.0, 1.0)),
               dict(eps=0.1, objective=lambda out, y: out["cls_out"][:, 0])):
        with pytest.raises(ValueError, match="cuda"):
            SquareRunner(model, 2, 64, **kw)
        with pytest.raises(ValueError, match="cuda"):
            model.square_runner(2, 64, **kw)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            SquareRunner(model, 2, 64, eps=0.01)
        with pytest.raises(ValueError, match="eval"):
            model.square_runner(2, 64, eps=0.01)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="UDEB4 / UDR18 / UDR50"):
        SquareRunner(torch.nn.Linear(2, 2).eval(), 2, 64, eps=0.1)
    assert not model.__dict__.get("_ud_square_runners")


def test_square_runner_checks_the_precision_first(model):
    from unidefense_amd.attack import SquareRunner, square_runner
    eb4 = type(model).__name__ == "UniDefenseModelEb4"
    for mk in (lambda **kw: SquareRunner(model, 2, 128, **kw), lambda **kw: square_runner(model, 2, 128, **kw),
               lambda **kw: model.square_runner(2, 128, **kw)):
        with pytest.raises(ValueError, match="precision must be one of"):
            mk(eps=0.01, precision="bf16")
        with pytest.raises(ValueError, match="precision must be one of"):
            mk(eps=-1.0, norm="l2", precision="bf16")                     # before every other argument
        with pytest.raises(ValueError, match="cuda" if eb4 else type(model).__name__):
            mk(eps=0.01, precision="fp16")
        with pytest.raises(ValueError, match="eps" if eb4 else "fp16"):
            mk(eps=-1.0, precision="fp16")
        with pytest.raises(ValueError, match="cuda"):
            mk(eps=0.01, precision="fp32")
    model.train()
    try:
        with pytest.raises(ValueError, match="eval" if eb4 else "fp16"):
            SquareRunner(model, 2, 128, eps=0.01, precision="fp16")
    finally:
        model.eval()


def test_square_key():
    from unidefense_amd.attack import square_key
    k = square_key(2, 256, eps=0.01)
    assert k == (2, 256, "linf", 0.01, 5000, 0.8, 1, True, 0, (-1.0, 1.0), "margin")
    assert square_key(2, 256, eps=0.01, precision="fp32") == k
    k16 = square_key(2, 256, eps=0.01, precision="fp16")
    assert k16 != k and k16[: len(k)] == k and k16[len(k):] == ("fp16",)
    assert len({square_key(2, 256, eps=0.01, **kw) for kw in (dict(), dict(restarts=2), dict(p_init=0.5), dict(steps=10),
                                                             dict(early_stop=False), dict(check_every=5),
                                                             dict(objective="cross_entropy"), dict(clip=(0.0, 1.0)))}) == 8


class _Stub:
    def __init__(self, model, *args):
        self.args = args


def test_square_accessor_cache(monkeypatch):
    """identity per full argument tuple, oldest-first eviction at _MAX_RUNNERS, most recently used last — and the four other
    caches exactly as they were (the runner class is stubbed: building a real one needs a GPU)"""
    from unidefense_amd import attack, infer
    monkeypatch.setattr(attack, "SquareRunner", _Stub)
    m = _model("UDR18")
    s1, s2, s3, s4 = object(), object(), object(), object()
    m.__dict__["_ud_runners"] = {(2, 64): s1}
    m.__dict__["_ud_grad_runners"] = {(2, 64, "cross_entropy"): s2}
    m.__dict__["_ud_attack_runners"] = {"k": s3}
    m.__dict__["_ud_apgd_runners"] = {"a": s4}
    r = m.square_runner(2, 64, eps=0.1)
    assert m.square_runner(2, 64, eps=0.1) is r and m.square_runner(2, 64, norm="linf", eps=0.1, steps=5000, restarts=1) is r
    assert attack.square_runner(m, 2, 64, eps=0.1) is r
    assert r.args == (2, 64, "linf", 0.1, 5000, 0.8, 1, True, 0, (-1.0, 1.0), "margin", "fp32")
    others = [m.square_runner(2, 64, eps=0.1, steps=3), m.square_runner(2, 64, eps=0.2), m.square_runner(2, 64, eps=0.1, p_init=0.5),
              m.square_runner(2, 64, eps=0.1, restarts=2), m.square_runner(2, 64, eps=0.1, early_stop=False)]
    assert len({id(o) for o in others + [r]}) == 6
    cache = m.__dict__["_ud_square_runners"]
    assert len(cache) == infer._MAX_RUNNERS == 4
    assert m.square_runner(2, 64, eps=0.1) is not r                          # r was evicted
    keep = m.square_runner(2, 64, eps=0.1, early_stop=False)
    assert keep is others[-1]
    for e in (0.3, 0.4, 0.5):
        m.square_runner(2, 64, eps=e)
    assert m.square_runner(2, 64, eps=0.1, early_stop=False) is keep
    assert m.__dict__["_ud_runners"] == {(2, 64): s1}
    assert m.__dict__["_ud_grad_runners"] == {(2, 64, "cross_entropy"): s2}
    assert m.__dict__["_ud_attack_runners"] == {"k": s3}
    assert m.__dict__["_ud_apgd_runners"] == {"a": s4}

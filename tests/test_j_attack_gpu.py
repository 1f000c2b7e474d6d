"""GPU: the attack kernels (csrc/attack.hip) and the graph-replayed input-gradient / attack runners
(unidefense_amd/attack.py: InputGradRunner, AttackRunner; TrainEngine.test_robust).

Kernels: the L-infinity step bitwise against the torch fp32 expression, the norms and the L2 step / projection against the
float64 restatement of tests/test_attack_cpu.py.  Runners: the gradient against the float64 oracles' autograd, the attack's
consistency with its own gradient (exact), its budget (exact), its EFFECT judged by the float64 oracle's loss at the GPU's
x_adv, and what the runners must leave alone (parameter flags, .grad, buffers, the training step)."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import eb4, losses as OL, param_fill, r18, r50
from tests import oracle_util as ou
from tests.margins import within
from tests.test_attack_cpu import ref_project_l2, ref_sample_sumsq, ref_step_l2, ref_step_linf

pytestmark = pytest.mark.gpu

GRAD_BAR = 1e-3          # the suite's plain gradient bound: max|d| / max|ref| and relative L2
LO, HI = -1.0, 1.0
EPS2 = 2.0 / 255.0       # model-input units: after Normalize(0.5, 0.5) this is one 8-bit grey level


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou.fit_cpu_threads()
    return torch.device("cuda:0")


def _build(name, dev):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    m = load_model(name)(num_classes=2, drop_rate=0.5, **kw)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev)


_MODELS = {}


def _shared(name, dev):
    """one eval-mode model per class for the tests that only read it (that the runners leave it alone is a test below)"""
    if name not in _MODELS:
        _MODELS[name] = _build(name, dev).eval()
    return _MODELS[name]


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _errs(g, ref):
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    d = g - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())


# ---- the float64 oracle ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_state(name):
    if name == "UDEB4":
        return ou.oracle_state(0.0, 0.3, dtype=torch.float64)
    shapes = r18.r18_state_shapes(2) if name == "UDR18" else r50.r50_state_shapes(2)
    return param_fill.fill_state_dict(shapes, 0.0, 0.3, torch.float64)


def _oracle_fwd(name, x64, pins=None):
    sd = _oracle_state(name)
    if name == "UDEB4":
        return eb4.forward_eb4(sd, x64, training=False)
    return (r18.forward_r18 if name == "UDR18" else r50.forward_r50)(sd, x64, training=False, rng=pins)


def _loss64(name, x64, y, pins=None):
    """the float64 oracle's summed cross-entropy"""
    return F.cross_entropy(_oracle_fwd(name, x64, pins)["cls_out"], y, reduction="sum")


def _grad64(name, x64, y, pins=None):
    xg = x64.detach().clone().requires_grad_()
    g, = torch.autograd.grad(_loss64(name, xg, y, pins), xg)
    return g


def _oracle_attack(name, x, y, norm, eps, steps, step, targeted=False):
    """the same attack run entirely in the float64 oracle"""
    x0 = x.double()
    xa = x0.clone()
    s = -step if targeted else step
    for _ in range(steps):
        g = _grad64(name, xa, y)
        if norm == "linf":
            xa = ref_step_linf(xa, x0, g, s, eps, LO, HI)
        else:
            xa, _ = ref_step_l2(xa, g, s)
            xa, _ = ref_project_l2(xa, x0, eps, LO, HI)
    return xa


# ---- 3. ud_attack_step_linf: bitwise -----------------------------------------------------------------------------------------
def _linf_case(total, seed):
    gen = torch.Generator().manual_seed(seed)
    eps = 4.0 / 255.0
    x0 = torch.rand(total, generator=gen) * 2 - 1
    x = x0 + (torch.rand(total, generator=gen) * 2 - 1) * eps
    x[1::5] = (x0 + eps)[1::5]                       # on the ball's faces, formed as the kernel forms them
    x[2::5] = (x0 - eps)[2::5]
    x[3::11] = LO                                    # and on the clip bounds
    x[4::13] = HI
    g = torch.randn(total, generator=gen)
    g[::7] = 0.0                                     # exact zeros: sign(0) = 0
    g[5::14] = -0.0
    return x, x0, g, eps


@pytest.mark.parametrize("total", [1, 3, 5, 4097, 3 * 95 * 95 * 2, 3 * 256 * 256 * 32])
def test_step_linf_bitwise_vs_torch(total):
    from unidefense_amd import kernels as K
    dev = _dev()
    x, x0, g, eps = _linf_case(total, total % 1000 + 3)
    assert total < 8 or ((g == 0).any() and (g > 0).any() and (g < 0).any())
    for step, e in ((1.0 / 255.0, eps), (-1.0 / 255.0, eps), (eps, eps), (1.0 / 255.0, 0.0)):
        want = ref_step_linf(x, x0, g, step, e, LO, HI)              # torch fp32 ops: one rounding each
        got = K.attack_step_linf(x.clone().to(dev), x0.to(dev), g.to(dev), step, e, LO, HI)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), want), (total, step, e, int((got.cpu() != want).sum()))
        if e == 0.0:
            assert torch.equal(got.cpu(), x0.clamp(LO, HI))


def test_step_linf_keeps_a_nan_gradient_visible():
    from unidefense_amd import kernels as K
    dev = _dev()
    x, x0, g, eps = _linf_case(4097, 9)
    bad = [0, 6, 4095, 4096]                          # vector body and scalar tail
    g[bad] = float("nan")
    want = ref_step_linf(x, x0, g, 1.0 / 255.0, eps, LO, HI)         # torch.sign(NaN) = 0: differs at `bad` only
    got = K.attack_step_linf(x.clone().to(dev), x0.to(dev), g.to(dev), 1.0 / 255.0, eps, LO, HI).cpu()
    assert torch.isnan(got[bad]).all() and int(torch.isnan(got).sum()) == len(bad)
    keep = torch.ones(4097, dtype=torch.bool)
    keep[bad] = False
    assert torch.equal(got[keep], want[keep])


# ---- 4. norms, L2 step and projection ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [3, 27075, 196608, 433200])
@pytest.mark.parametrize("N", [1, 3, 96])
def test_sample_sumsq_vs_float64(N, per):
    """within per 2^-52 relative of numpy's float64 sum: non-negative terms added in double in another order — that is the
    worst case of either side"""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(N * 7 + per % 97)
    a = torch.randn(N, per, generator=gen)
    b = torch.randn(N, per, generator=gen) * 0.5
    ad, bd = a.to(dev), b.to(dev)
    for bb, bdev in ((None, None), (b, bd)):
        got = K.sample_sumsq(ad, bdev)
        again = K.sample_sumsq(ad, bdev)
        torch.cuda.synchronize()
        assert got.dtype == torch.float64 and tuple(got.shape) == (N,)
        assert torch.equal(got, again)
        want = ref_sample_sumsq(a, bb)
        rel = float(((got.cpu() - want).abs() / want).max())
        assert within(f"ud_sample_sumsq N {N} per {per} b {bb is not None}: rel / (per 2^-52)", rel / (per * 2.0 ** -52), 1.0)


@pytest.mark.parametrize("per", [3, 27075, 196608])
def test_l2_step_and_projection_vs_float64(per):
    from unidefense_amd import kernels as K
    dev = _dev()
    N = 3
    gen = torch.Generator().manual_seed(per % 89)
    x0 = torch.rand(N, per, generator=gen) * 2 - 1
    x = x0 + (torch.rand(N, per, generator=gen) * 2 - 1) * 0.05
    g = torch.randn(N, per, generator=gen)
    g[1] = 0.0                                            # a zero-gradient sample: the norm clamp, no move
    for step in (0.5, -0.25):
        want, inc = ref_step_l2(x, g, step)
        gss = K.sample_sumsq(g.to(dev))
        got = K.attack_step_l2(x.clone().to(dev), g.to(dev), gss, step).cpu()
        bound = 4 * 2.0 ** -24 * (x.double().abs() + inc.abs())
        worst = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
        assert within(f"ud_attack_step_l2 per {per} step {step}: |d| / (4 2^-24 (|x| + |increment|))", worst, 1.0)
        assert torch.equal(got[1], x[1])
    # projection: sample 0 and 2 far outside the ball, sample 1 inside it (factor exactly 1: unchanged before the clamp)
    eps = 0.5
    xa = x0 + g * 0.05
    xa[1] = x0[1] + (torch.rand(per, generator=gen) * 2 - 1) * (0.4 * eps / per ** 0.5)
    want, d = ref_project_l2(xa, x0, eps, LO, HI)
    dss = K.sample_sumsq(xa.to(dev), x0.to(dev))
    got = K.attack_project_l2(xa.clone().to(dev), x0.to(dev), dss, eps, LO, HI).cpu()
    nrm = torch.sqrt(ref_sample_sumsq(xa, x0))
    assert nrm[1] < eps and (per < 100 or (nrm[0] > eps and nrm[2] > eps)), nrm
    bound = 4 * 2.0 ** -24 * (x0.double().abs() + d.abs())
    worst = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
    assert within(f"ud_attack_project_l2 per {per}: |d| / (4 2^-24 (|x0| + |d|))", worst, 1.0)
    assert torch.equal(got[1], xa[1].clamp(LO, HI))
    zero = K.attack_project_l2(xa.clone().to(dev), x0.to(dev), dss, 0.0, LO, HI).cpu()
    assert torch.equal(zero, x0.clamp(LO, HI))


# ---- 5. InputGradRunner ------------------------------------------------------------------------------------------------------
CASES = [("UDEB4", 256, 1, 7), ("UDEB4", 256, 2, 7), ("UDR18", 128, 2, 5), ("UDR50", 256, 2, 5)]


def _pins(name, m, x):
    """ReLU patterns and max-pool winners of the HIP path's forward (as test_resnet_eval_input_grad_vs_oracle pins them)"""
    if name == "UDEB4":
        return None
    m._debug_watch = True
    try:
        m(x.clone().requires_grad_())
        kinks = {k: v.permute(0, 3, 1, 2).cpu() for k, v in m._debug_kinks.items()}
        feats = m._debug_feats
        if name == "UDR18":
            sel = feats["pool_sel"].permute(0, 3, 1, 2).cpu()
        else:
            sel = {"stem": feats["pool_sel_stem"].permute(0, 3, 1, 2).cpu(),
                   "emb": feats["pool_sel_emb"].permute(0, 3, 1, 2).cpu()}
        torch.cuda.synchronize()
    finally:
        m._debug_watch = False
    return {"pool_sel": sel, "relu_masks": kinks}


@pytest.mark.parametrize("name,size,n,seed", CASES)
def test_input_grad_runner_vs_oracle(name, size, n, seed):
    from unidefense_amd.attack import InputGradRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    xd, yd = x.to(dev), y.to(dev)
    ref = _grad64(name, x.double(), y, _pins(name, m, xd))
    r = InputGradRunner(m, n, size)
    eager = r(xd, yd).clone()
    reps = [r(xd, yd).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert r.graph is not None and r.calls == 4
    assert torch.isfinite(reps[0]).all()
    assert all(torch.equal(a, reps[0]) for a in reps[1:])
    assert set(r.out) == {"cls_out", "rec", "loss_dict"} and not r.out["cls_out"].requires_grad
    mx, l2 = _errs(reps[0], ref)
    print(f"  {name} {size} n={n}: max|d|/max|ref| {mx:.2e}  rel L2 {l2:.2e}")
    assert within(f"InputGradRunner {name} n={n} vs oracle, max|d| / max|ref|", mx, GRAD_BAR)
    assert within(f"InputGradRunner {name} n={n} vs oracle, rel L2", l2, GRAD_BAR)
    assert within(f"InputGradRunner {name} n={n} replay vs eager warm-up, rel L2", _rel_l2(reps[0], eager), 1e-5)
    assert all(p.grad is None for p in m.parameters())


def test_input_grad_runner_permuted_batch():
    """reduction="sum": each sample's gradient is that of its own loss, so a permuted batch gives the permuted gradient"""
    from unidefense_amd.attack import InputGradRunner
    dev = _dev()
    m = _shared("UDEB4", dev)
    x = param_fill.make_input(8, 256, 13).to(dev)
    y = param_fill.make_labels(8).to(dev)
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=dev)
    r = InputGradRunner(m, 8, 256)
    r(x, y)
    g = r(x, y).clone()
    gp = r(x[perm].contiguous(), y[perm].contiguous()).clone()
    assert within("InputGradRunner bs-8 permuted batch vs permuted gradient, rel L2", _rel_l2(gp, g[perm]), 1e-5)


def test_runner_call_refusals():
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    m = _shared("UDR18", dev)
    x = torch.zeros(2, 3, 128, 128, device=dev)
    y = torch.zeros(2, dtype=torch.int64, device=dev)
    for r in (InputGradRunner(m, 2, 128), AttackRunner(m, 2, 128, eps=EPS2, steps=1)):
        with pytest.raises(ValueError, match="cuda"):
            r(x.cpu(), y)
        with pytest.raises(ValueError, match="cuda"):
            r(x, y.cpu())
        with pytest.raises(ValueError, match="differs"):
            r(x[:1], y)
        with pytest.raises(ValueError, match="differs"):
            r(x.half(), y)
        with pytest.raises(ValueError, match="differ"):
            r(x, y.int())
        with pytest.raises(ValueError, match="differ"):
            r(x, y[:1])
        m.train()
        try:
            with pytest.raises(ValueError, match="training"):
                r(x, y)
        finally:
            m.eval()
        assert r.calls == 0


# ---- 6. the attack is consistent with its own gradient, exactly ---------------------------------------------------------------
@pytest.mark.parametrize("name,size,n,seed", CASES[1:3])
def test_fgsm_is_the_formula_on_the_runners_own_gradient(name, size, n, seed):
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    y = param_fill.make_labels(n).to(dev)
    r = AttackRunner(m, n, size, norm="linf", eps=EPS2, steps=1)
    assert r.step == EPS2
    r(x, y)
    xa = r(x, y).clone()
    assert r.graph is not None
    want = ref_step_linf(x, x, r.g, EPS2, EPS2, LO, HI)
    assert torch.equal(xa, want)
    assert float((xa - x).abs().max()) > 0.5 * EPS2
    ig = InputGradRunner(m, n, size)
    ig(x, y)
    d = _rel_l2(r.g, ig(x, y))
    assert within(f"AttackRunner.g vs InputGradRunner {name}, rel L2", d, 1e-5)


# ---- 7. budget, exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("name,size,n,seed,steps", [("UDR18", 128, 2, 5, 1), ("UDR18", 128, 2, 5, 3), ("UDR18", 128, 2, 5, 10),
                                                    ("UDEB4", 256, 2, 7, 3)])
def test_attack_stays_inside_its_budget(name, size, n, seed, steps, norm):
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    y = param_fill.make_labels(n).to(dev)
    assert float(x.min()) >= LO and float(x.max()) <= HI           # inside clip: the outer clamp only moves towards x0
    eps = EPS2 if norm == "linf" else 0.5
    r = AttackRunner(m, n, size, norm=norm, eps=eps, steps=steps)
    warm = r(x, y).clone()
    runs = [r(x, y).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert r.graph is not None
    assert torch.equal(runs[0], runs[1])
    per = 3 * size * size
    for xa in (warm, runs[0]):
        assert torch.isfinite(xa).all()
        assert float(xa.min()) >= LO and float(xa.max()) <= HI
        if norm == "linf":
            assert bool((xa >= x - eps).all()) and bool((xa <= x + eps).all())     # the bounds as the kernel forms them (fp32)
            assert float((xa - x).abs().max()) > 0.5 * eps
        else:
            nrm = torch.sqrt(ref_sample_sumsq(xa.cpu(), x.cpu()))
            slack = 2.0 ** -23 * per ** 0.5        # x0 + d f rounds to fp32 once per element: ABSOLUTE 2^-24 for |x| <= 1
            assert bool((nrm <= eps + slack).all()), (nrm, eps)
            assert bool((nrm > 0.1 * eps).all()), nrm
    within(f"AttackRunner {name} {norm} steps {steps}: replay vs eager warm-up x_adv, max|d| / eps (recorded)",
           float((runs[0] - warm).abs().max()) / eps, 2.0)


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_zero_budget_returns_the_clamped_input(norm):
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared("UDR18", dev)
    x = (param_fill.make_input(2, 128, 5) * 1.02).to(dev)          # a few values outside clip
    y = param_fill.make_labels(2).to(dev)
    assert float(x.max()) > HI
    r = AttackRunner(m, 2, 128, norm=norm, eps=0.0, steps=2)
    assert r.step == 0.0
    for _ in range(3):
        assert torch.equal(r(x, y), x.clamp(LO, HI))


def test_random_start_is_reproducible():
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared("UDR18", dev)
    x = param_fill.make_input(2, 128, 5).to(dev)
    y = param_fill.make_labels(2).to(dev)
    r = AttackRunner(m, 2, 128, norm="linf", eps=EPS2, steps=2, random_start=True)

    def run(seed):
        return r(x, y, generator=torch.Generator(device=dev).manual_seed(seed)).clone()
    run(0)
    a, b, c = run(1), run(1), run(2)
    assert torch.equal(a, b) and not torch.equal(a, c)
    cpu = r(x, y, generator=torch.Generator().manual_seed(1)).clone()           # a CPU generator is taken too
    assert torch.equal(cpu, r(x, y, generator=torch.Generator().manual_seed(1)))
    for xa in (a, c, cpu):
        assert bool((xa >= x - EPS2).all()) and bool((xa <= x + EPS2).all())
        assert float(xa.min()) >= LO and float(xa.max()) <= HI


# ---- 8. effect, judged by the oracle ------------------------------------------------------------------------------------------
# The bar 0.9 on gain_gpu / gain_ref: re-running the oracle's attack with uniform noise of 1e-4 max|g| in its gradient (4 x
# the x.grad error DESIGN 3j records) keeps >= 0.99 of the gain in every case below — UDEB4 FGSM 0.990, L-inf PGD 0.9905,
# L2 PGD 0.99999; UDR18 0.99992 / 0.999999; UDR50 FGSM (simulated for this file, make_input(2, 256, 5), gain_ref 31.25 on a
# loss of 108.0) 0.99990, and 0.99981 at 1e-3 max|g| — so 0.9 stands for UDR50 as well (>= 0.95 at 1e-4 max|g|).
EFFECT = [("UDEB4", 256, 1, 7, "linf", EPS2, 1, EPS2), ("UDR18", 128, 2, 5, "linf", EPS2, 1, EPS2),
          ("UDR50", 256, 2, 5, "linf", EPS2, 1, EPS2),
          ("UDR18", 128, 2, 5, "linf", EPS2, 3, 1.0 / 255.0), ("UDEB4", 256, 1, 7, "linf", EPS2, 3, 1.0 / 255.0),
          ("UDR18", 128, 2, 5, "l2", 0.5, 3, 0.25), ("UDEB4", 256, 1, 7, "l2", 1.0, 3, 0.5)]


@pytest.mark.parametrize("name,size,n,seed,norm,eps,steps,step", EFFECT)
def test_attack_effect_judged_by_the_oracle(name, size, n, seed, norm, eps, steps, step):
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    r = AttackRunner(m, n, size, norm=norm, eps=eps, steps=steps, step=step)
    r(x.to(dev), y.to(dev))
    xa = r(x.to(dev), y.to(dev)).cpu()
    with torch.no_grad():
        base = float(_loss64(name, x.double(), y))
        gain_gpu = float(_loss64(name, xa.double(), y)) - base
    xr = _oracle_attack(name, x, y, norm, eps, steps, step)
    with torch.no_grad():
        gain_ref = float(_loss64(name, xr, y)) - base
    ratio = gain_gpu / gain_ref
    print(f"  {name} {norm} eps {eps:.4g} steps {steps}: L64(x) {base:.6g}  gain_ref {gain_ref:.4g}  gain_gpu {gain_gpu:.4g}  "
          f"ratio {ratio:.5f}")
    if steps == 1:
        g64 = _grad64(name, x.double(), y)
        flips = float((torch.sign(r.g.cpu().double()) != torch.sign(g64)).double().mean())
        print(f"    share of elements whose sign differs from the oracle's: {flips:.4f}")
    assert gain_ref > 0
    assert within(f"attack effect {name} {norm} steps {steps}: 1 - gain_gpu / gain_ref", 1.0 - ratio, 0.1)


def test_targeted_attack_lowers_the_target_loss():
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    name, size, n = "UDR18", 128, 2
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, 5)
    y = param_fill.make_labels(n)
    yt = 1 - y
    r = AttackRunner(m, n, size, norm="linf", eps=EPS2, steps=1, targeted=True)
    r(x.to(dev), yt.to(dev))
    xa = r(x.to(dev), yt.to(dev)).cpu()
    xr = _oracle_attack(name, x, yt, "linf", EPS2, 1, EPS2, targeted=True)
    with torch.no_grad():
        base = float(_loss64(name, x.double(), yt))
        drop_gpu = base - float(_loss64(name, xa.double(), yt))
        drop_ref = base - float(_loss64(name, xr, yt))
    print(f"  targeted {name}: L64(x, y_target) {base:.6g}  drop_ref {drop_ref:.4g}  drop_gpu {drop_gpu:.4g}")
    assert drop_ref > 0
    assert within("targeted attack UDR18: 1 - drop_gpu / drop_ref", 1.0 - drop_gpu / drop_ref, 0.1)


# ---- 9. state is untouched ---------------------------------------------------------------------------------------------------
def _mixed_flags(m):
    for i, p in enumerate(m.parameters()):
        p.requires_grad_(i % 5 != 0 and p is not getattr(m.bottleneck, "bias", None))
    return [p.requires_grad for p in m.parameters()]


def _train_grads(m, x, tgt, dev):
    n = len(tgt)
    m.train()
    m.zero_grad(set_to_none=True)
    out = m(x, rng=ou.make_rng(n, 32, 0.5))
    OL.pass1_loss(out, tgt, n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_runners_leave_the_model_as_it_was():
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    n = 2
    x = param_fill.make_input(n, 256, 31).to(dev)
    y = param_fill.make_labels(n).to(dev)
    fresh = _build("UDEB4", dev)
    flags = _mixed_flags(fresh)
    _train_grads(fresh, x, y, dev)                   # the first step of a shape measures GEMM plans; the second runs on them
    want = _train_grads(fresh, x, y, dev)
    del fresh
    m = _build("UDEB4", dev).eval()
    assert _mixed_flags(m) == flags and not all(flags) and any(flags)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    for r in (AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2), AttackRunner(m, n, 256, norm="l2", eps=0.5, steps=2),
              InputGradRunner(m, n, 256)):
        for _ in range(3):
            r(x, y)
    torch.cuda.synchronize()
    assert [p.requires_grad for p in m.parameters()] == flags
    assert all(p.grad is None for p in m.parameters())
    assert not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    got = _train_grads(m, x, y, dev)
    assert got.keys() == want.keys() and len(got) > 300
    diff = [k for k in got if not torch.equal(got[k], want[k])]
    assert not diff, diff[:10]


def test_frozen_flags_come_back_after_a_failing_objective():
    from unidefense_amd.attack import InputGradRunner
    dev = _dev()
    m = _build("UDR18", dev).eval()
    flags = _mixed_flags(m)

    def broken(out, y):
        raise KeyError("objective failed")
    r = InputGradRunner(m, 2, 128, objective=broken)
    with pytest.raises(KeyError):
        r(param_fill.make_input(2, 128, 5).to(dev), param_fill.make_labels(2).to(dev))
    assert [p.requires_grad for p in m.parameters()] == flags


# ---- 10. a runner follows the model ------------------------------------------------------------------------------------------
def test_captured_runners_follow_an_optimizer_step():
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    n = 2
    m = _build("UDEB4", dev).eval()
    x = param_fill.make_input(n, 256, 51).to(dev)
    y = param_fill.make_labels(n).to(dev)
    ig = InputGradRunner(m, n, 256)
    at = AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2)
    for r in (ig, at):
        r(x, y)
    g0, a0 = ig(x, y).clone(), at(x, y).clone()
    assert ig.graph is not None and at.graph is not None
    # in-place AdamW step on every parameter and new running statistics of one BatchNorm
    torch.manual_seed(5)
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    opt = torch.optim.AdamW(params, lr=1e-3)
    ptrs = [p.data_ptr() for p in params]
    opt.step()
    assert ptrs == [p.data_ptr() for p in params]
    m.zero_grad(set_to_none=True)
    bn = m.backbone._blocks[3]._bn0
    bn.running_mean.add_(0.05)
    bn.running_var.mul_(1.5)
    g1, a1 = ig(x, y).clone(), at(x, y).clone()
    assert _rel_l2(g1, g0) > 1e-2                          # the step changed the function
    ig2 = InputGradRunner(m, n, 256)
    at2 = AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2)
    for r in (ig2, at2):
        r(x, y)
    assert torch.equal(g1, ig2(x, y))
    assert torch.equal(a1, at2(x, y))
    assert not torch.equal(a1, a0)


# ---- 11. the engine ----------------------------------------------------------------------------------------------------------
def _same_result(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


def _mean_ce(res):
    p = res["scores"].double()
    lb = res["labels"]
    return float(-torch.log(torch.where(lb == 0, p, 1.0 - p).clamp_min(1e-30)).mean())


def test_engine_test_robust():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    torch.manual_seed(0)
    eng = get_engine("FE")(copy.deepcopy(CONFIG), "Test")
    t0 = eng.test(batches=2)
    v0 = eng.validate(1, batches=2)
    with pytest.raises(ValueError, match="attack"):
        eng.test_robust(batches=2)
    res = eng.test_robust(batches=2, attack={"norm": "linf", "eps": 0.0, "steps": 2})
    assert set(res) == {"clean", "adv", "attack"}
    assert res["attack"]["eps"] == 0.0 and res["attack"]["steps"] == 2 and res["attack"]["norm"] == "linf"
    _same_result(res["clean"], t0)
    assert torch.equal(res["adv"]["scores"], res["clean"]["scores"])           # eps = 0: x_adv is x, bitwise
    assert torch.equal(res["adv"]["labels"], res["clean"]["labels"])
    _same_result(eng.test(batches=2), t0)
    _same_result(eng.validate(2, batches=2), v0)
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())


def test_engine_test_robust_raises_the_loss():
    """a UDR18 filled by param_fill, 3-step L-inf PGD at eps 2/255 from config['config']['attack']: the oracle's gain for this
    model is O(1) on a loss of 1.39, far from fp32 noise"""
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(CONFIG)
    cfg["model"] = {"name": "UDR18", "num_classes": 2, "drop_rate": 0.2}
    cfg["data"] = {"train_batch_size": 2, "size": 128}
    cfg["config"]["attack"] = {"norm": "linf", "eps": EPS2, "steps": 3}
    eng = get_engine("FE")(cfg, "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    res = eng.test_robust(batches=2)
    assert res["attack"]["step"] == 2.5 * EPS2 / 3
    clean, adv = _mean_ce(res["clean"]), _mean_ce(res["adv"])
    print(f"  mean cross-entropy of the scores: clean {clean:.4f}  adv {adv:.4f}")
    assert adv > clean
    assert within("test_robust UDR18: clean / adv mean cross-entropy", clean / adv, 1.0)

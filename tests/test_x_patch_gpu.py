"""GPU: the adversarial patch's kernels (csrc/patch.hip), PatchRunner (unidefense_amd/patch.py) and TrainEngine.test_patch.

Kernels: the paste bitwise against the numpy float32 restatement; the gather adjoint against the float64 scatter within one
fp32 rounding of a double sum, exactly zero where nothing weighs, the same bits twice; the update bitwise against the torch fp32
expression.  Every shape runs every placement (through the device row index k, which is part of what is tested), both masks,
aligned and one float off a 16-byte boundary.  Runner: the life cycle (eager, capture, replay: the same bits), the patch's
persistence and clip, what it leaves alone, the reduce hook, the clamped-loss rule on known losses, and its EFFECT judged by
the float64 oracle.  The stage: one cached runner, four score rows."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import param_fill
from tests.margins import within
from tests.test_j_attack_gpu import _build, _dev, _grad64, _loss64, _mixed_flags, _oracle_fwd, _shared
from unidefense_amd import patch as PT

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
SHAPES = [(1, 8, 1), (3, 20, 5), (2, 33, 8), (5, 95, 33), (2, 64, 64)]       # one texel; odd sides; no multiple of the 64 x 4 tile; several blocks
KERNEL_CASES = [s + (False,) for s in SHAPES] + [s + (True,) for s in SHAPES]


def _placements(S, P):
    """the ten placements every shape runs: identity (integer-aligned, scale 1), half a texel off, 90 degrees, 17 degrees at
    scale 0.6 and at 1.7, scale 0.25, scale 4 (rolled by 45 degrees: the widest window), a corner with part of the patch
    outside, fully outside, and scale 4 at the image centre (larger than the image wherever 4 P > S)"""
    t0, mid = (P - 1) / 2.0, (S - 1) / 2.0
    a = t0 + max((S - P) // 2, 0)
    return [PT.placement_q16(P, (a, a), 0.0, 1.0), PT.placement_q16(P, (a + 0.5, a - 0.5), 0.0, 1.0), PT.placement_q16(P, (math.floor(mid), math.floor(mid)), 90.0, 1.0),
            PT.placement_q16(P, (mid + 0.3, mid - 1.2), 17.0, 0.6), PT.placement_q16(P, (mid - 0.7, mid + 0.4), 17.0, 1.7),
            PT.placement_q16(P, (mid + 0.25, mid), -8.0, 0.25), PT.placement_q16(P, (mid - 1.1, mid + 2.3), 45.0, 4.0),
            PT.placement_q16(P, (0.4, S - 1.3), 33.0, 1.2), PT.placement_q16(P, (-4.0 * P - 8, S + 4.0 * P + 8), 10.0, 1.0),
            PT.placement_q16(P, (mid, mid), 30.0, 4.0)]


def _table(N, S, P):
    """[10, N, 16]: sample n of row k runs placement (k + n) % 10"""
    rows = _placements(S, P)
    return np.array([[rows[(k + n) % len(rows)] for n in range(N)] for k in range(len(rows))], dtype=np.int32)


def _place(t, dev, offset):
    """t on the device; offset: inside a larger buffer, one float behind a 16-byte boundary"""
    if not offset:
        return t.to(dev).contiguous()
    big = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
    out = big[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def _alphas(P):
    ragged = PT.patch_alpha(P, "circle") * (0.25 + 0.75 * torch.rand(P, P, generator=torch.Generator().manual_seed(P)))
    return [("square", PT.patch_alpha(P)), ("circle", ragged)]       # both shapes; the circle with uneven coverage inside


# ---- 1. ud_patch_paste: bitwise -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,P,offset", KERNEL_CASES)
def test_paste_bitwise_vs_numpy(N, S, P, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(N * 1000 + S * 10 + P)
    x = (torch.rand(N, 3, S, S, generator=gen) * 2 - 1) * 1.1         # a few values outside the clip: untouched pixels keep them
    patch = torch.rand(3, P, P, generator=gen) * 2 - 1
    patch.view(-1)[::7] = HI
    table = _table(N, S, P)
    rows = table.shape[0]
    td = torch.from_numpy(table).to(dev)
    xd = _place(x, dev, offset)
    for name, alpha in _alphas(P):
        pd, ad = _place(patch, dev, offset), _place(alpha, dev, offset)
        for k in range(rows):
            out = K.patch_paste(xd, pd, ad, td, torch.tensor([k, 77], dtype=torch.int32, device=dev), _place(torch.full_like(x, 9.0), dev, offset), LO, HI)
            want = PT.ref_patch_paste(x, patch, alpha, table[k], LO, HI)
            assert np.array_equal(_bits(out), _bits(want)), (name, k)
            outside = (k + np.arange(N)) % rows == 8                  # the fully-outside placement: x bit for bit
            assert np.array_equal(_bits(out.cpu().numpy()[outside]), _bits(x.numpy()[outside]))
        changed = sum(int((PT.ref_patch_paste(x, patch, alpha, table[k], LO, HI) != x.numpy()).sum()) for k in range(rows))
        assert changed > 0
        # the row index is clamped into the table
        for k, row in ((-5, 0), (rows, rows - 1), (1 << 30, rows - 1)):
            out = K.patch_paste(xd, pd, ad, td, torch.tensor([k], dtype=torch.int32, device=dev), torch.empty_like(xd), LO, HI)
            assert np.array_equal(_bits(out), _bits(PT.ref_patch_paste(x, patch, alpha, table[row], LO, HI)))
        # a NaN texel shows only under its taps
        bad = patch.clone()
        bad[1, P // 2, P // 3] = float("nan")
        for k in (0, 4, 6):
            out = K.patch_paste(xd, _place(bad, dev, offset), ad, td, torch.tensor([k], dtype=torch.int32, device=dev), torch.empty_like(xd), LO, HI)
            want = PT.ref_patch_paste(x, bad, alpha, table[k], LO, HI)
            assert np.array_equal(np.isnan(out.cpu().numpy()), np.isnan(want)) and not np.isnan(want[:, 0]).any() and not np.isnan(want[:, 2]).any()
            keep = ~np.isnan(want)
            assert np.array_equal(_bits(out.cpu().numpy()[keep]), _bits(want[keep]))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)                                   # x is only read
    with pytest.raises(ValueError, match="buffers of their own"):
        K.patch_paste(xd, pd, ad, td, torch.zeros(1, dtype=torch.int32, device=dev), xd, LO, HI)


# ---- 2. ud_patch_grad: one rounding of a double sum ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,P,offset", KERNEL_CASES)
def test_grad_vs_float64_scatter(N, S, P, offset):
    """|gp - ref| <= 2^-23 |ref| + 2^-40 sum |omega g| per element: ONE fp32 rounding of the double sum is 2^-24 |ref|, and the
    double sum itself is off by at most 225 2^-53 sum |omega g| < 2^-45 of it, whatever the order: a factor of two to spare on
    the first term and 32 on the second.  Where nothing weighs the texel the bound is zero: gp is exactly zero there."""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(N * 1000 + S * 10 + P + 1)
    g = torch.randn(N, 3, S, S, generator=gen) * torch.logspace(-3, 2, S).reshape(1, 1, 1, S)        # magnitudes apart inside a window
    table = _table(N, S, P)
    td = torch.from_numpy(table).to(dev)
    gd = _place(g, dev, offset)
    worst, zeros = 0.0, 0
    for name, alpha in _alphas(P):
        ad = _place(alpha, dev, offset)
        for k in range(table.shape[0]):
            kd = torch.tensor([k], dtype=torch.int32, device=dev)
            gp = K.patch_grad(gd, ad, td, kd, _place(torch.full((N, 3, P, P), 9.0), dev, offset))
            again = K.patch_grad(gd, ad, td, kd, _place(torch.full((N, 3, P, P), -9.0), dev, offset))
            ref, mag = PT.ref_patch_grad(g, alpha, table[k], magnitude=True)
            got = gp.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(again))           # no atomics: the same bits
            bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * mag
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(got[mag == 0] == 0), (name, k)              # every element written; zero coverage: exactly zero
            zeros += int((mag == 0).sum())
            if np.any(bound > 0):
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert zeros > 0
    print(f"  patch grad N {N} S {S} P {P} offset {offset}: worst |d| / (2^-23 |ref| + 2^-40 sum |omega g|) {worst:.3f}")
    assert within(f"patch grad N {N} S {S} P {P}: |d| / (2^-23 |ref| + 2^-40 sum |omega g|)", worst, 1.0)
    assert torch.equal(gd.cpu(), g)


# ---- 3. ud_patch_update: bitwise -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,offset", [(s[2], o) for s in SHAPES for o in (False, True)])
def test_update_bitwise_vs_torch(P, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(P)
    patch = torch.rand(3, P, P, generator=gen) * 2 - 1
    gsum = torch.randn(3, P, P, generator=gen)
    patch.view(-1)[1::5] = HI                        # on the clip's faces
    patch.view(-1)[2::5] = LO
    gsum.view(-1)[::7] = 0.0                         # exact zeros: sign(0) = 0
    gsum.view(-1)[5::14] = -0.0
    for step, lo, hi in ((1.0 / 32, LO, HI), (-1.0 / 32, LO, HI), (3.0, LO, HI), (0.1, 0.0, 1.0), (0.0, LO, HI)):
        want = torch.clamp(patch + step * torch.sign(gsum), lo, hi)                     # torch fp32 ops: one rounding each
        got = K.patch_update(_place(patch, dev, offset), _place(gsum, dev, offset), step, lo, hi)
        assert np.array_equal(_bits(got), _bits(want)), (P, step)
    bad = gsum.clone()
    bad.view(-1)[0] = float("nan")
    got = K.patch_update(_place(patch, dev, offset), _place(bad, dev, offset), 0.1, LO, HI).cpu()
    assert int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(got.view(-1)[0]))
    with pytest.raises(ValueError, match="buffers of their own"):
        p = patch.to(dev)
        K.patch_update(p, p, 0.1, LO, HI)


def test_public_paste_checks_its_table_on_the_host():
    dev = _dev()
    x = (torch.rand(3, 3, 20, 20, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    patch = torch.rand(3, 5, 5, generator=torch.Generator().manual_seed(2)) * 2 - 1
    params, table = PT.patch_placements(3, 20, 5, max_angle=40.0, scales=(0.5, 2.0), generator=torch.Generator().manual_seed(3))
    alpha = PT.patch_alpha(5, "circle")
    out = PT.paste(x, patch, table, alpha)
    assert out.data_ptr() != x.data_ptr() and np.array_equal(_bits(out), _bits(PT.ref_patch_paste(x, patch, alpha, table)))
    assert np.array_equal(_bits(PT.paste(x, patch.to(dev), table.numpy())), _bits(PT.ref_patch_paste(x, patch, PT.patch_alpha(5), table)))
    buf = torch.empty_like(x)
    assert PT.paste(x, patch, table, alpha, out=buf) is buf and torch.equal(buf, out)
    for col, v, text in ((12, 9, "reach"), (14, 1, "reserved")):
        bad = table.clone()
        bad[1, col] = v
        with pytest.raises(ValueError, match=text):
            PT.paste(x, patch, bad, alpha)
    with pytest.raises(ValueError, match="one placement per sample"):
        PT.paste(x, patch, table[:2], alpha)


# ---- 4. the runner ------------------------------------------------------------------------------------------------------------------
CASES = [("UDR18", 128, 4, 5, "fp32"), ("UDEB4", 256, 2, 7, "fp32"), ("UDEB4", 256, 2, 7, "fp16")]


def _inputs(size, n, seed, dev):
    return param_fill.make_input(n, size, seed).to(dev), param_fill.make_labels(n).to(dev)


def _fit(r, x, y, calls=1, seed=11, start=0.0):
    """the patch and x_adv after reset(start) and `calls` calls with a generator seeded once"""
    r.reset(start)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(calls):
        xa = r(x, y, gen)
    torch.cuda.synchronize()
    return r.patch.clone(), xa.clone()


@pytest.mark.parametrize("name,size,n,seed,precision", CASES)
def test_life_cycle_persistence_and_clip(name, size, n, seed, precision):
    dev = _dev()
    m = _shared(name, dev)
    x, y = _inputs(size, n, seed, dev)
    r = PT.PatchRunner(m, n, size, patch=24, shape="circle", steps=2, step=0.25, max_angle=30.0, scales=(0.7, 1.6), precision=precision)
    assert tuple(r.patch.shape) == (3, 24, 24) and not bool(r.patch.any()) and r.args["step"] == 0.25
    assert r.args["area"] == pytest.approx(24 ** 2 * 1.15 ** 2 / size ** 2, rel=1e-12) and PT.PatchRunner(m, n, size).args["step"] == 2.0 / 64
    with pytest.raises(ValueError, match="steps must be an integer >= 1"):
        PT.PatchRunner(m, n, size, steps=0)
    # call 1 (eager), 2 (capture) and 3 (replay), each from a reset() and the same seed: the same bits
    eager, xa_eager = _fit(r, x, y)
    assert r.graph is None and r.calls == 1
    p2, xa2 = _fit(r, x, y)
    p3, xa3 = _fit(r, x, y)
    assert r.graph is not None and r.update_graph is None and r.calls == 3
    assert torch.equal(p2, p3) and torch.equal(xa2, xa3)
    assert torch.equal(p2, eager) and torch.equal(xa2, xa_eager)
    assert tuple(r.history.shape) == (2, n) and bool((r.counted == 1).all()) and r.counted.dtype == torch.int32      # beta = inf: everyone steers
    assert tuple(r.placements.shape) == (3, n, 4) and r.placements.dtype == torch.float64
    want = PT.patch_placements(3 * n, size, 24, 30.0, (0.7, 1.6), generator=torch.Generator().manual_seed(11))
    assert torch.equal(r.placements.view(-1, 4), want[0]) and torch.equal(r.table.cpu().view(-1, 16), want[1])
    # x_adv is x with the patch as it stands pasted at the LAST row of placements
    assert np.array_equal(_bits(xa3), _bits(PT.ref_patch_paste(x.cpu(), p3.cpu(), r.alpha.cpu(), r.table[2].cpu(), LO, HI)))
    assert bool((p3.abs() <= 0.5).all()) and float(p3.abs().max()) == 0.5 and bool((p3[:, r.alpha == 0] == 0).all())
    # the patch persists: a second call goes on from the first's, another seed gives other placements and another patch
    twice, _ = _fit(r, x, y, calls=2)
    assert not torch.equal(twice, p3) and float((twice - p3).abs().max()) <= 0.5 and float(twice.abs().max()) > 0.5
    assert not torch.equal(_fit(r, x, y, seed=12)[0], p3)
    # ... and stays inside the clip, on its faces after enough steps; reset(tensor) is clamped into it
    many, xa = _fit(r, x, y, calls=4)
    assert float(many.min()) == LO and float(many.max()) == HI and float(xa.min()) >= LO and float(xa.max()) <= HI
    r.reset(torch.full((3, 24, 24), 3.0))
    assert bool((r.patch == HI).all())
    with pytest.raises(ValueError, match="a patch is"):
        r.reset(torch.zeros(3, 8, 8))
    # apply: any batch size, no backward, the runner's patch as it stands
    r.reset(many)
    other = param_fill.make_input(3, size, seed + 1).to(dev)
    params, table = r.draw(3, torch.Generator().manual_seed(5))
    got = r.apply(other, table=table)
    assert got.data_ptr() != other.data_ptr() and not got.requires_grad and torch.equal(r.patch, many)
    assert np.array_equal(_bits(got), _bits(PT.ref_patch_paste(other.cpu(), many.cpu(), r.alpha.cpu(), table, LO, HI)))
    assert torch.equal(r.apply(other, generator=torch.Generator().manual_seed(5)), got)
    with pytest.raises(ValueError, match="cuda"):
        r.apply(other.cpu())
    with pytest.raises(ValueError, match="batch"):
        r.apply(other[:, :, :-1])
    assert all(p.grad is None for p in m.parameters()) and not m.training


def test_runner_leaves_the_model_as_it_was():
    dev = _dev()
    m = _build("UDR18", dev).eval()
    flags = _mixed_flags(m)
    assert not all(flags) and any(flags)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    x, y = _inputs(128, 4, 5, dev)
    for r in (PT.PatchRunner(m, 4, 128, steps=2), PT.PatchRunner(m, 4, 128, patch=16, reduce=lambda g: None)):
        for _ in range(3):
            r(x, y, torch.Generator().manual_seed(1))
    torch.cuda.synchronize()
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters()) and not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())


def test_reduce_hook():
    dev = _dev()
    m = _shared("UDR18", dev)
    x, y = _inputs(128, 4, 5, dev)
    calls = []

    def zeroing(gsum):
        calls.append(tuple(gsum.shape))
        gsum.zero_()

    def identity(gsum):
        calls.append("identity")

    plain = PT.PatchRunner(m, 4, 128, patch=16, steps=2, step=0.25)
    _fit(plain, x, y)
    want, xa_want = _fit(plain, x, y)
    r = PT.PatchRunner(m, 4, 128, patch=16, steps=2, step=0.25, reduce=zeroing)
    start = (torch.rand(3, 16, 16, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    for call in range(3):                                           # eager, captured, replayed: two graphs with the hook between
        del calls[:]
        p, xa = _fit(r, x, y, start=start)
        assert calls == [(3, 16, 16)] * 2 and torch.equal(p, start), call            # gsum seen once per iteration; zeroed: no move
        assert np.array_equal(_bits(xa), _bits(PT.ref_patch_paste(x.cpu(), start.cpu(), r.alpha.cpu(), r.table[2].cpu(), LO, HI)))
    assert r.graph is not None and r.update_graph is not None
    r = PT.PatchRunner(m, 4, 128, patch=16, steps=2, step=0.25, reduce=identity)
    _fit(r, x, y)
    del calls[:]
    got, xa = _fit(r, x, y)
    assert calls == ["identity"] * 2 and torch.equal(got, want) and torch.equal(xa, xa_want)      # the bits of reduce=None


def test_clamped_loss_rule_on_known_losses():
    """history[0] is each sample's loss with the grey start patch pasted at row 0: the float64 oracle gives it, and beta is put
    between the oracle's losses, far from all of them"""
    dev = _dev()
    m = _shared("UDR18", dev)
    x, y = _inputs(128, 4, 5, dev)
    r = PT.PatchRunner(m, 4, 128, patch=16, steps=1, step=0.125, beta=1.0)
    for _ in range(3):                                              # eager, captured, replayed
        _fit(r, x, y)
        pasted = PT.ref_patch_paste(x.cpu(), np.zeros((3, 16, 16)), r.alpha.cpu(), r.table[0].cpu(), LO, HI)
        with torch.no_grad():
            each = F.cross_entropy(_oracle_fwd("UDR18", torch.from_numpy(pasted).double())["cls_out"], y.cpu(), reduction="none")
        assert float((each - 1.0).abs().min()) > 0.5, each           # (clean: 2.74, 3.48, 0.060, 0.047; a 16-pixel patch moves them little)
        steer = (each < 1.0).int().tolist()
        assert r.counted.cpu().tolist() == [steer] and 0 < sum(steer) < 4
        rel = float(((r.history[0].cpu().double() - each).abs() / each).max())
        assert within("PatchRunner UDR18 history[0] vs the oracle's per-sample loss, max rel", rel, 1e-3)
        # only the counted steered: the patch is the sign of THEIR adjoints' sum, in ascending n
        gsum = torch.zeros_like(r.patch)
        for n in range(4):
            if steer[n]:
                gsum = gsum + r.gp[n]
        assert torch.equal(r.gsum, gsum) and torch.equal(r.patch, 0.125 * torch.sign(gsum)) and r.args["beta"] == 1.0
    src = PT.PatchRunner(m, 4, 128, patch=16, steps=1, source=1)
    _fit(src, x, y)
    assert src.counted.cpu().tolist() == [(y == 1).int().cpu().tolist()] and src.args["source"] == 1


# ---- 5. effect, judged by the oracle -----------------------------------------------------------------------------------------------
# One sticker near the middle of the face: no roll, one pixel per texel, the centre free inside 0.8 pixels (the region is 46
# pixels wide, the bounding circle 45.25), so every iteration and the returned batch paste at fractional offsets of their own.
# Wider placement ranges make four sign steps on four samples a lottery, in the oracle itself: with max_angle 20 and scales
# (0.9, 1.4) the oracle's own gain moves by 4 to 70 per cent under the gradient noise below, and no bar on a GPU could stand.
EFFECT = dict(patch=32, steps=4, step=0.25, max_angle=0.0, scales=(1.0, 1.0), region=(0.3, 0.3, 0.66, 0.66))
NOISE = 1e-4                                                        # of max |g|: 4 x the x.grad error DESIGN 3j records


def _fit64(name, x, y, alpha, tables, noise=0.0):
    """ref_patch_fit with the float64 oracle's gradient (optionally with uniform noise of `noise` max|g|): (patch, x_adv)"""
    gen = torch.Generator().manual_seed(0)

    def grad(xa):
        xa = torch.from_numpy(xa).double()
        g = _grad64(name, xa, y)
        if noise:
            g = g + (torch.rand(g.shape, generator=gen, dtype=torch.float64) * 2 - 1) * noise * float(g.abs().max())
        return g.numpy(), np.zeros(len(y))                          # beta = inf: everyone steers, f is not looked at

    return PT.ref_patch_fit(grad, x.numpy(), np.zeros((3, EFFECT["patch"], EFFECT["patch"])), alpha, tables, EFFECT["step"], (LO, HI))


def _gain(name, x_adv, y, base):
    with torch.no_grad():
        return float(_loss64(name, torch.as_tensor(x_adv).double(), y)) - base


def test_effect_judged_by_the_oracle():
    """What the FIT gains: the float64 oracle's loss at the batch pasted with the patch, minus its loss at the same batch
    pasted with the START patch (reset(): mid-grey) at the same placements.  (Against the unpasted batch the grey patch alone
    moves this model's loss by -0.62: occlusion, which is no part of the fit.)  gain_gpu, at the GPU's returned batch, against
    gain_ref, the same fit run wholly in the oracle at the same placements.  The bar on 1 - gain_gpu / gain_ref is the suite's 0.1
    (test_attack_effect_judged_by_the_oracle).  It stands because uniform gradient noise of 1e-4 max|g|, four times the x.grad
    error DESIGN 3j records, moves the oracle's own gain by far less: 1.7e-2 of it (gain_ref 2.3375, noisy 2.2969; printed and
    asserted under a third of the bar).  A uniform-random patch at the same placements must gain under half of gain_ref
    (0.343: 0.147 of it)."""
    name, size, n, seed, precision = CASES[0]
    dev = _dev()
    m = _shared(name, dev)
    x, y = param_fill.make_input(n, size, seed), param_fill.make_labels(n)
    r = PT.PatchRunner(m, n, size, precision=precision, **EFFECT)
    _fit(r, x.to(dev), y.to(dev))
    patch, xa = _fit(r, x.to(dev), y.to(dev))
    tables, alpha = r.table.cpu().numpy(), r.alpha.cpu()
    grey = PT.ref_patch_paste(x, np.zeros((3, EFFECT["patch"], EFFECT["patch"])), alpha, tables[-1], LO, HI)
    with torch.no_grad():
        clean, base = float(_loss64(name, x.double(), y)), float(_loss64(name, torch.from_numpy(grey).double(), y))
    ref, xa_ref = _fit64(name, x, y, alpha, tables)
    gain_ref, gain_gpu = _gain(name, xa_ref, y, base), _gain(name, xa.cpu(), y, base)
    gain_noisy = _gain(name, _fit64(name, x, y, alpha, tables, NOISE)[1], y, base)
    random = torch.rand(3, EFFECT["patch"], EFFECT["patch"], generator=torch.Generator().manual_seed(0)) * 2 - 1
    gain_random = _gain(name, PT.ref_patch_paste(x, random, alpha, tables[-1], LO, HI), y, base)
    agree = float((patch.cpu().double() == torch.from_numpy(ref)).double().mean())
    print(f"  {name} {precision}: L64(x) {clean:.6g}  L64(x with the grey patch) {base:.6g}  gain_ref {gain_ref:.5g}  gain_gpu {gain_gpu:.5g}  "
          f"ratio {gain_gpu / gain_ref:.5f}  noisy oracle {gain_noisy:.5g} (ratio {gain_noisy / gain_ref:.5f})  random {gain_random:.4g} "
          f"({gain_random / gain_ref:.4f})  share of texels equal to the oracle's {agree:.4f}")
    assert gain_ref > 0
    assert within(f"patch effect {name}: the oracle's own gain under {NOISE:g} max|g| gradient noise, |1 - ratio|", abs(1.0 - gain_noisy / gain_ref), 0.1 / 3)
    assert within(f"patch effect {name} {precision}: 1 - gain_gpu / gain_ref", 1.0 - gain_gpu / gain_ref, 0.1)
    assert within(f"patch effect {name}: the uniform-random patch's gain / gain_ref", gain_random / gain_ref, 0.5)


# ---- 6. the stage ---------------------------------------------------------------------------------------------------------------------
def test_engine_test_patch():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(CONFIG)
    cfg["model"] = {"name": "UDR18", "num_classes": 2, "drop_rate": 0.2}
    cfg["data"] = {"train_batch_size": 2, "size": 128}
    cfg["config"]["patch"] = {"patch": 24, "shape": "circle", "steps": 2, "step": 0.5, "seed": 1}
    eng = get_engine("FE")(cfg, "Test")
    net = eng.model_without_ddp
    param_fill.fill_module_(net, sf_coef=0.0, fuse_coef=0.3)
    with pytest.raises(ValueError, match="patch takes PatchRunner's keyword arguments and 'seed'"):
        eng.test_patch(batches=1, fit_batches=1, epochs=1, patch={"patch": 24, "stepz": 3})
    res = eng.test_patch(batches=1, fit_batches=1, epochs=1)
    second = eng.test_patch(batches=1, fit_batches=1, epochs=1)
    assert len(net.__dict__["_ud_patch_runners"]) == 1                # ONE cached runner serves both calls
    assert set(res) == {"clean", "adv", "random", "occlusion", "attack"}
    a = res["attack"]
    assert {"method", "patch", "shape", "steps", "step", "max_angle", "scales", "region", "beta", "source", "clip", "precision", "area", "texture",
            "fooled", "fooled_random", "fooled_occlusion", "fit_counted"} <= set(a)
    assert a["method"] == "patch" and a["patch"] == 24 and a["steps"] == 2 and a["area"] == pytest.approx(24 ** 2 * 1.025 ** 2 / 128 ** 2, rel=1e-12)
    assert a["texture"].device.type == "cpu" and tuple(a["texture"].shape) == (3, 24, 24) and float(a["texture"].abs().max()) == 1.0
    assert a["fit_counted"] == [4, 4]
    for k in ("clean", "adv", "random", "occlusion"):
        assert tuple(res[k]["scores"].shape) == (4,) and torch.equal(res[k]["labels"], res["clean"]["labels"])
        assert torch.equal(res[k]["scores"], second[k]["scores"])     # reset, the same seed, a replayed fit: the same rows
    assert torch.equal(a["texture"], second["attack"]["texture"])
    assert len({tuple(res[k]["scores"].tolist()) for k in ("clean", "adv", "random", "occlusion")}) == 4
    for k in ("fooled", "fooled_random", "fooled_occlusion"):
        assert type(a[k]) is float
    # the held-out step is the iterator's step 2: the clean column is test()'s second batch
    assert torch.equal(res["clean"]["scores"], eng.test(batches=2)["scores"][4:])
    assert all(p.grad is None for p in net.parameters())

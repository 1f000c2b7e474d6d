"""The pass-2 input perturbation kernels (csrc/perturb.hip, model/perturb.py, the DFT-matrix plane transforms of kernels.py) at
the sizes where their edge code runs: ragged sort rows (partial sub-round, partial wave, L < 64, partial last round: 380 x 380
ends every row in one), odd sides, ties, grid-stride and multi-trip loops, H != W and the minimum sizes.  Inputs, references and
mutations come from tests/perturb_cases.py; tests/test_perturb_edges_cpu.py proves on the CPU that these comparisons can fail.

Every numeric comparison goes through tests.margins.within or tests.parity.yard_check.  Exact comparisons record the number of
entries that differ against a bar of 0.  Inputs are finite: NaN ordering is not part of the sort's contract."""
import os

import numpy as np
import pytest
import torch

from oracle import perturb as OP
from tests import oracle_util as ou
from tests import perturb_cases as pc
from tests.margins import within
from tests.parity import bar_of, rel_err, yard_check

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou.fit_cpu_threads()
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a))          # a copy: the cached inputs are read-only


def _exact(name, got, ref):
    """equality as floats (the sign of a zero does not count), the number of entries that differ recorded against 0"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (name, got.shape, ref.shape, got.dtype)
    assert np.isfinite(got).all(), name
    n_bad = int((got != ref).sum())
    print(f"  {name}: {n_bad} of {got.size} entries differ")
    assert within(name + " [entries that differ]", n_bad, 0) and np.array_equal(got, ref), \
        f"{name}: {n_bad} of {got.size} entries differ, first at {np.argwhere(got != ref)[:3].tolist()}"


def _yard_capped(name, got, ref64, ref32, cap):
    """yard_check with the bar cut at `cap` (a bar the project already holds the quantity to)"""
    yard = rel_err(ref32, ref64)
    scope = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::")[-1].split("[")[0]
    bar = min(cap, bar_of(f"{scope}/{name}", yard)[0])
    e = rel_err(got, ref64)
    print(f"  {name}: rel err {e:.3e}   fp32 yardstick {yard:.3e}   bar {bar:.3e}")
    within(name + " [yard]", yard, bar)
    assert within(name, e, bar), f"{name}: rel err {e:.3e} > bar {bar:.3e} (fp32 yardstick {yard:.3e})"


def _all(checks):
    """run every check of a test, so that each quantity is measured and recorded before the test fails"""
    bad = []
    for fn in checks:
        try:
            fn()
        except AssertionError as err:
            bad.append(str(err))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ a. exact distribution matching
@pytest.mark.parametrize("L", pc.EFDM_LENGTHS)
def test_efdm_bit_for_bit(L):
    """K.efdm against the fp32 restatement (stable argsort, sort, (c + om sv) - om c in float32): the kernel rounds every operation
    on its own in exactly that order (no FMA contraction, both zeros one sort key), so equality is the derived bar.  Before this
    test about a fifth of the entries were one ulp off at every L: the mix had been contracted into two FMAs."""
    from unidefense_amd import kernels as K
    dev = _dev()
    checks = []
    for family in pc.EFDM_FAMILIES:
        c, s, lm = pc.efdm_inputs(family, L)
        got = K.efdm(_t(c).to(dev), _t(s).to(dev), _t(lm).to(dev), pc.EFDM_ROWS_PER_SAMPLE).cpu().numpy()
        ref = pc.efdm_ref(c, s, lm, pc.EFDM_ROWS_PER_SAMPLE)
        checks.append(lambda f=family, g=got, r=ref: _exact(f"efdm {f} L={L}", g, r))
    _all(checks)


@pytest.mark.parametrize("shape", pc.SPATIAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spatial_transfer_bit_for_bit(shape):
    from unidefense_amd.model import perturb
    dev = _dev()
    n, c, h, w = shape
    checks = []
    for family in ("uniform", "levels8"):
        a, b = pc.image_pair(n, c, h, w, family)
        lm = pc.distinct_lmda(n)
        got = perturb.spatial_transfer_with(a.to(dev), b.to(dev), lm.to(dev)).cpu().numpy()
        ref = pc.efdm_ref(a.numpy().reshape(n * c, h * w), b.numpy().reshape(n * c, h * w), lm.numpy(), c).reshape(shape)
        checks.append(lambda f=family, g=got, r=ref: _exact(f"spatial {f} {shape}", g, r))
    _all(checks)


# ------------------------------------------------------------------------------------------------ b. spectrum mixing
@pytest.mark.parametrize("S,extra_pad", [(4, 0), (5, 0), (5, 4), (8, 0), (13, 0)])
def test_amp_mix_planted_spectra(S, extra_pad):
    """K.amp_mix on spectra with planted bins: exact zeros in A (phase 0: w (1 - l) |B| real, imaginary part exactly 0), a negative
    purely imaginary bin, a denormal bin; the padding columns of the output (allocated with `empty`) exactly 0"""
    from unidefense_amd import kernels as K
    dev = _dev()
    inp = pc.amp_inputs(S, extra_pad)
    Wh, Whp = inp["Wh"], inp["Whp"]
    r64, r32 = pc.amp_mix_ref(inp, torch.float64), pc.amp_mix_ref(inp, torch.float32)
    out = K.amp_mix(inp["A"].to(dev), inp["B"].to(dev), inp["lmda"].to(dev), S, pc.AMP_PLANES_PER_SAMPLE).cpu()
    assert tuple(out.shape) == (pc.AMP_PLANES, 2 * S, Whp) and torch.isfinite(out).all()
    got = {"re": out[:, :S, :Wh], "im": out[:, S:, :Wh]}

    def planted():
        for name, (p, ky, kx) in inp["planted"].items():
            re, im = float(got["re"][p, ky, kx]), float(got["im"][p, ky, kx])
            want_re, want_im = float(r64["re"][p, ky, kx]), float(r64["im"][p, ky, kx])
            print(f"  {name} ({p}, {ky}, {kx}): got ({re:.7g}, {im:.7g}) want ({want_re:.7g}, {want_im:.7g})")
            if name.startswith("zero"):
                assert within(f"{name} |im|", abs(im), 0.0) and want_re > 0, (name, im)
            if name == "negative imaginary":
                assert within(f"{name} |re|", abs(re), 0.0) and im < 0, (name, re, im)
    _all([lambda: yard_check("re", got["re"], r64["re"], r32["re"]), lambda: yard_check("im", got["im"], r64["im"], r32["im"]),
          planted, lambda: _exact("padding columns", out[:, :, Wh:].numpy(), np.zeros((pc.AMP_PLANES, 2 * S, Whp - Wh), np.float32))])


# ------------------------------------------------------------------------------------------------ c. plane transforms, GEMM path
@pytest.mark.parametrize("ortho", [True, False], ids=["ortho", "plain"])
@pytest.mark.parametrize("P", pc.DFT_PLANES)
@pytest.mark.parametrize("S", pc.DFT_SIDES)
def test_dft_planes_gemm_path(S, P, ortho):
    """K.dft_rfft2_planes / _adjoint outside {128, 256, 320}: the padded path (S % 4 != 0) included, against torch.fft.rfft2 and
    autograd through it"""
    from unidefense_amd import kernels as K
    dev = _dev()
    inp = pc.dft_inputs(S, P)
    Wh, Whp = inp["Wh"], inp["Whp"]
    r64, r32 = pc.dft_ref(inp, torch.float64, ortho), pc.dft_ref(inp, torch.float32, ortho)
    Y = K.dft_rfft2_planes(inp["x"].to(dev).contiguous(), ortho=ortho).cpu()
    assert tuple(Y.shape) == (P, 2 * S, Whp) and torch.isfinite(Y).all()
    adj = K.dft_rfft2_planes_adjoint(inp["G"].to(dev), S, ortho=ortho).cpu()
    assert tuple(adj.shape) == (P, S, S) and adj.is_contiguous() and torch.isfinite(adj).all()
    got = {"re": Y[:, :S, :Wh], "im": Y[:, S:, :Wh], "adj": adj}
    _all([lambda q=q: yard_check(q, got[q], r64[q], r32[q]) for q in ("re", "im", "adj")]
         + [lambda: _exact("padding columns", Y[:, :, Wh:].numpy(), np.zeros((P, 2 * S, Whp - Wh), np.float32))])


# ------------------------------------------------------------------------------------------------ d. amplitude transfer end to end
@pytest.mark.parametrize("n,S", pc.FREQ_CASES)
def test_freq_transfer_end_to_end(n, S):
    """freq_transfer_with against oracle.perturb.freq_style_transfer (float64); the yardstick is the same lines in torch float32.
    With the Nyquist weight applied to column S // 2 of an odd side (the kernel before this test) S = 13 is 0.27 off, S = 37 0.17."""
    from unidefense_amd.model import perturb
    dev = _dev()
    a, b = pc.image_pair(n, 3, S, S, "uniform")
    lm = pc.distinct_lmda(n)
    r64 = _t(OP.freq_style_transfer(a.double().numpy(), b.double().numpy(), lm.double().numpy().reshape(-1, 1, 1, 1)))
    r32 = pc.freq_ref(a, b, lm, torch.float32)
    got = perturb.freq_transfer_with(a.to(dev), b.to(dev), lm.to(dev)).cpu()
    assert torch.isfinite(got).all()
    yard_check("freq", got, r64, r32)


def test_freq_transfer_refuses_a_non_square_input():
    from unidefense_amd.model import perturb
    dev = _dev()
    a, b = pc.image_pair(2, 3, 37, 50, "uniform")
    with pytest.raises(ValueError):
        perturb.freq_transfer_with(a.to(dev), b.to(dev), pc.distinct_lmda(2).to(dev))


# ------------------------------------------------------------------------------------------------ e. colour transfer
@pytest.mark.parametrize("family", pc.CORAL_FAMILIES)
def test_coral_moments_within_the_fp64_summation_bound(family):
    """K.coral_moments against float64 numpy sums: every moment within HW 2^-52 of the sum of its absolute terms, the worst case
    of ANY two summation orders in fp64 (each is within (HW - 1) 2^-53 of the exact sum; the terms themselves are exact)"""
    from unidefense_amd import kernels as K
    dev = _dev()
    checks = []
    for (n, h, w) in pc.CORAL_SHAPES:
        x = pc.image_pair(n, 3, h, w, family)[0]
        ref, ref_abs = pc.moments_ref(x.numpy())
        xd = x.to(dev)
        for chunks in pc.MOMENT_CHUNKS:          # 3 x 5 has HW = 15: with 16 (and with 7) chunks some are empty
            got = K.coral_moments(xd, chunks=chunks).cpu().numpy()
            assert got.shape == ref.shape and got.dtype == np.float64
            worst = float((np.abs(got - ref) / ref_abs).max())
            checks.append(lambda v=worst, hw=h * w, c=chunks, s=(n, h, w): _moment(f"moments {s} chunks={c}", v, hw))
    _all(checks)


def _moment(name, worst, hw):
    bound = hw * 2.0 ** -52
    print(f"  {name}: |got - ref| / sum |terms| = {worst:.3e}   bound {bound:.3e}")
    assert within(name, worst, bound), (name, worst, bound)


@pytest.mark.parametrize("n,h,w", pc.CORAL_SHAPES)
def test_affine3_vs_float64(n, h, w):
    """K.affine3: one block at 3 x 5, 64 blocks without a loop up to HW = 16384, the grid-stride loop beyond"""
    from unidefense_amd import kernels as K
    dev = _dev()
    x, M = pc.image_pair(n, 3, h, w, "uniform")[0], pc.affine_matrix(n)
    got = K.affine3(x.to(dev), M.to(dev)).cpu()
    yard_check("affine3", got, pc.affine3_ref(x, M, torch.float64), pc.affine3_ref(x, M, torch.float32))


@pytest.mark.parametrize("family", pc.CORAL_FAMILIES)
@pytest.mark.parametrize("n,h,w", pc.CORAL_SHAPES)
def test_coral_vs_oracle(n, h, w, family):
    """perturb.coral against oracle.perturb.coral in float64; the bar is the smaller of the project's 5e-5 and the yardstick bar
    of the oracle run on float32 arrays.  The oracle's solver is perturb_cases.reference_svd: numpy's factors with the signs of
    the reference program's solver (torch.linalg.svd, float32).  With numpy-float64's own signs 7 of these 12 cases are 0.25 to
    1.7 off for ANY implementation that follows the reference program, which the step golden recorded from it requires."""
    from unidefense_amd.model import perturb
    dev = _dev()
    s, t = pc.image_pair(n, 3, h, w, family)
    r64, r32 = pc.coral_ref(s.numpy(), t.numpy(), np.float64), pc.coral_ref(s.numpy(), t.numpy(), np.float32)
    assert r32.dtype == np.float32
    got = perturb.coral(s.to(dev), t.to(dev)).cpu()
    assert torch.isfinite(got).all()
    _yard_capped("coral", got, _t(r64), _t(r32), pc.CORAL_OLD_BAR)


# ------------------------------------------------------------------------------------------------ f. downscale
@pytest.mark.parametrize("h,w", pc.DOWNSCALE_SHAPES)
def test_downscale_is_atens_two_interpolations(h, w):
    """the composed gather against F.interpolate(x 0.75) then F.interpolate(size): pure data movement, so torch.equal"""
    from unidefense_amd.model import perturb
    dev = _dev()
    x = pc.image_pair(2, 3, h, w, "uniform")[0]
    got = perturb.downscale(x.to(dev)).cpu()
    ref = pc.downscale_ref(x)
    _exact(f"downscale {h}x{w}", got.numpy(), ref.numpy())
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ g. blur
@pytest.mark.parametrize("shape", pc.BLUR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blur_small_and_ragged(shape):
    """3 pixels is the least a reflect padding of 2 takes: every tap of a 3-pixel side is a reflected one"""
    from unidefense_amd.model import perturb
    dev = _dev()
    x = pc.image_pair(*shape, "uniform")[0]
    got = perturb.random_blur(x.to(dev)).cpu().numpy()
    ref = OP.gaussian_blur5(x.numpy().astype(np.float64))
    err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f"  blur {shape}: rel err {err:.3e}")
    assert within(f"blur {shape}", err, pc.BLUR_BAR), err


@pytest.mark.parametrize("h,w", [(2, 5), (5, 2), (1, 1)])
def test_blur_refuses_sides_below_three(h, w):
    from unidefense_amd.lib import UDLibraryError
    from unidefense_amd.model import perturb
    dev = _dev()
    with pytest.raises(UDLibraryError):
        perturb.random_blur(torch.zeros(1, 3, h, w, device=dev))


# ------------------------------------------------------------------------------------------------ h. the branches of perturb_input
@pytest.mark.parametrize("color", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("branch", ["freq", "spat"])
def test_perturb_input_style_branches_unequal_counts(branch, color):
    """perturb_input on 3 real + 2 fake samples at 37 x 37 with the seeded draws replayed into the oracle.  Without the colour
    transfer the rank matching only moves values: bit-equal to the fp32 restatement.  The other bars: the yardstick of the oracle
    replayed on float32 arrays, and never above what tests/test_c_perturb.py holds the same branch to at 32 x 32."""
    from unidefense_amd.model import perturb
    dev = _dev()
    n, S = pc.BRANCH_N_REAL + pc.BRANCH_N_FAKE, pc.BRANCH_SIDE
    x = pc.image_pair(n, 3, S, S, "uniform")[0]
    seed = pc.seed_for(branch)
    name64, r64 = pc.replay_branch(x.double().numpy(), pc.BRANCH_PERT_REAL, pc.BRANCH_PERT_FAKE, seed, color, pc.reference_svd)
    name32, r32 = pc.replay_branch(x.numpy(), pc.BRANCH_PERT_REAL, pc.BRANCH_PERT_FAKE, seed, color, pc.reference_svd)
    assert name64 == name32 == branch and r32.dtype == np.float32
    torch.manual_seed(seed)
    got = perturb.perturb_input(x.to(dev), torch.tensor(pc.BRANCH_PERT_REAL), torch.tensor(pc.BRANCH_PERT_FAKE), color).cpu()
    assert torch.isfinite(got).all()
    if branch == "spat" and not color:
        torch.manual_seed(seed)
        torch.rand(1), torch.randint(0, 2, size=(1,))
        lm = (torch.rand((n, 1, 1)) / 2.0 + 0.5).reshape(-1).numpy()
        st = OP.style_batch(x.numpy(), pc.BRANCH_PERT_REAL, pc.BRANCH_PERT_FAKE)
        ref = pc.efdm_ref(x.numpy().reshape(n * 3, S * S), st.reshape(n * 3, S * S), lm, 3).reshape(x.shape)
        _exact("spat branch", got.numpy(), ref)
    _yard_capped(f"{branch}{' colour' if color else ''} branch", got, _t(r64), _t(r32),
                 pc.CORAL_OLD_BAR if color else {"freq": 1e-5, "spat": 1e-6}[branch])

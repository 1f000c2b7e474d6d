"""Seeded inputs, references and named mutations of the pass-2 input perturbation kernels (csrc/perturb.hip, model/perturb.py,
the DFT-matrix plane transforms of kernels.py) at the sizes where their edge code runs: ragged sort rows, odd sides, ties,
grid-stride loops, H != W, minimum sizes.  tests/test_perturb_edges_cpu.py (no GPU: proves that the comparisons can fail) and
tests/test_c_perturb_edges_gpu.py (holds the HIP kernels to them) both import it.

A reference is numpy or plain torch, written here or taken from oracle/perturb.py, and takes `mutation=`: a plausible kernel
bug, named in MUTATIONS.  A reference that backs a yardstick bar (tests/parity.py) is written once over a dtype, so that the
float32 yardstick comes from the same lines as the float64 reference.

A plain helper module: no conftest, no plugin, no pytest setting.
"""
import functools

import numpy as np
import torch

from oracle import perturb as OP

MUTATIONS = {
    "nyquist_weight_at_odd_side": "amp_mix halves column S // 2 for every S: an interior column when S is odd",
    "ties_in_reverse_order": "the sort is not stable: equal content values take their style values in reverse index order",
    "neg_zero_sorts_first": "the sort key orders -0.0 before +0.0; the stable reference treats the two as a tie",
    "last_partial_round_dropped": "the elements past the last full round of 4096 keep the content value",
    "coral_biased_std": "the colour statistics divide by n instead of n - 1",
    "affine_offset_dropped": "the colour map applies its 3 x 3 part and forgets the offset column",
}


def _check(mutation, *allowed):
    assert mutation is None or (mutation in MUTATIONS and mutation in allowed), mutation


def _seed(*key):
    """a seed that is a function of the key alone (str hashes are salted per process: spell the family out)"""
    s = 0
    for k in key:
        for ch in (k if isinstance(k, str) else str(int(k))):
            s = (s * 131 + ord(ch)) % 2147483647
        s = (s * 131 + 7) % 2147483647
    return s


# ------------------------------------------------------------------------------------------------ exact distribution matching
EFDM_LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5136, 8193)      # 5136 = 4096 + 1040: the tail of 380 x 380
EFDM_FAMILIES = ("uniform", "levels8", "three", "sorted", "reversed", "signs")
EFDM_ROWS, EFDM_ROWS_PER_SAMPLE = 6, 3
EFDM_LMDA = np.array([0.5625, 0.8], np.float32)
SORT_ROUND = 4096


def _distinct(rng, rows, L, lo=-1.0, hi=1.0):
    """rows x L distinct values of (lo, hi) in random order.  The style rows take another interval than the content rows, so
    that the style value of equal rank is never the content value itself."""
    return np.stack([(lo + (rng.permutation(L) + 0.5) / L * (hi - lo)) for _ in range(rows)]).astype(np.float32)


def _signs(rng, rows, L, zero_share):
    """negatives, positives, both zeros, denormals and +-1e30: all four digit passes and the sign flip of the key matter"""
    v = (rng.standard_normal((rows, L)) * 10.0 ** rng.integers(-3, 4, (rows, L))).astype(np.float32)
    u = rng.random((rows, L))
    den = (rng.integers(1, 1000, (rows, L)) * np.where(rng.random((rows, L)) < 0.5, -1.0, 1.0)).astype(np.float32) \
        * np.float32(1.4e-45)
    big = np.where(rng.random((rows, L)) < 0.5, -1e30, 1e30).astype(np.float32)
    v = np.where(u < zero_share, np.float32(0.0), v)
    v = np.where((u >= zero_share) & (u < 2 * zero_share), np.float32(-0.0), v)
    v = np.where((u >= 0.80) & (u < 0.92), den, v)
    v = np.where(u >= 0.96, big, v)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def efdm_inputs(family, L):
    """(content [6, L], style [6, L], lmda [2]) float32, a function of (family, L) alone.  Never modified by a caller."""
    rng = np.random.default_rng(_seed("efdm", family, L))
    R = EFDM_ROWS
    if family == "uniform":
        c, s = _distinct(rng, R, L), _distinct(rng, R, L, -0.7, 0.9)
    elif family == "levels8":                                  # 8-bit images: ties in content and in style
        c = (rng.integers(0, 256, (R, L)).astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
        s = (rng.integers(0, 256, (R, L)).astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
    elif family == "three":
        c = rng.choice(np.array([-0.5, 0.25, 0.75], np.float32), (R, L))
        s = _distinct(rng, R, L, -0.7, 0.9)
    elif family in ("sorted", "reversed"):
        c, s = np.sort(_distinct(rng, R, L), -1), _distinct(rng, R, L, -0.7, 0.9)
        if family == "reversed":
            c = c[:, ::-1]
    elif family == "signs":
        # few zeros in the style: the tied zeros of the content then take style values that differ from each other
        c, s = _signs(rng, R, L, 0.15), _signs(rng, R, L, 0.02)
    else:
        raise KeyError(family)
    c, s = np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32)
    for a in (c, s):
        assert np.isfinite(a).all()
        a.setflags(write=False)
    return c, s, EFDM_LMDA


def _key_neg_zero_first(c):
    """the order-preserving float -> uint32 map WITHOUT the merge of the two zeros: -0.0 gets a smaller key than +0.0"""
    u = np.ascontiguousarray(c, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def efdm_ref(content, style, lmda, rows_per_sample, mutation=None):
    """The fp32 restatement of ud_efdm on [rows, L]: a stable argsort of the content, a sort of the style, and
    (c + om * sv) - om * c with om = 1 - l, every operation rounded to float32 in that order (the kernel's _rn intrinsics)."""
    _check(mutation, "ties_in_reverse_order", "neg_zero_sorts_first", "last_partial_round_dropped")
    c = np.ascontiguousarray(content, np.float32)
    rows, L = c.shape
    if mutation == "ties_in_reverse_order":
        idx = L - 1 - np.argsort(c[:, ::-1], axis=-1, kind="stable")
    elif mutation == "neg_zero_sorts_first":
        idx = np.argsort(_key_neg_zero_first(c), axis=-1, kind="stable")
    else:
        idx = np.argsort(c, axis=-1, kind="stable")
    sv = np.sort(np.asarray(style, np.float32), axis=-1)
    matched = np.empty_like(c)
    np.put_along_axis(matched, idx, sv, -1)                    # the element of rank j gets the style value of rank j
    om = np.repeat(np.float32(1.0) - np.asarray(lmda, np.float32), rows_per_sample)[:, None]
    assert om.dtype == np.float32 and om.shape[0] == rows
    out = ((c + om * matched) - om * c).astype(np.float32)
    if mutation == "last_partial_round_dropped":
        out[:, L // SORT_ROUND * SORT_ROUND:] = c[:, L // SORT_ROUND * SORT_ROUND:]
    return out


SPATIAL_SHAPES = ((2, 3, 380, 380), (2, 3, 37, 50), (1, 3, 5, 7))


@functools.lru_cache(maxsize=None)
def image_pair(n, c, h, w, family="uniform", seed=0):
    """(a, b) float32 [n, c, h, w] torch images.  `uniform`: noise on (-1, 1).  `levels8`: 8-bit levels k / 127.5 - 1.
    `photo`: strongly correlated channels, mean 0.6 and std 0.05."""
    g = torch.Generator().manual_seed(_seed("image", family, n, c, h, w, seed))
    out = []
    for _ in range(2):
        if family == "uniform":
            t = torch.rand(n, c, h, w, generator=g) * 2 - 1
        elif family == "levels8":
            t = torch.randint(0, 256, (n, c, h, w), generator=g).float() / 127.5 - 1.0
        elif family == "photo":
            base = torch.randn(n, 1, h, w, generator=g)
            t = 0.6 + 0.05 * (0.97 * base + 0.24 * torch.randn(n, c, h, w, generator=g))
        else:
            raise KeyError(family)
        out.append(t.float().contiguous())
    return tuple(out)


def distinct_lmda(n):
    """n distinct mixing weights of [0.5, 1), float32"""
    return (0.5 + 0.45 * (torch.arange(n, dtype=torch.float32) + 0.5) / n).float()


# ------------------------------------------------------------------------------------------------ spectrum mixing
AMP_SIDES = (4, 5, 8, 13)
AMP_PLANES, AMP_PLANES_PER_SAMPLE = 6, 3
AMP_LMDA = torch.tensor([0.5625, 0.8])


def ceil4(v):
    return -(-v // 4) * 4


@functools.lru_cache(maxsize=None)
def amp_inputs(S, extra_pad=0):
    """A, B [P, 2S, Whp] in the dft_rfft2_planes layout with planted bins (`planted`: name -> (plane, ky, kx)) and finite
    garbage in the padding columns of both inputs."""
    Wh = S // 2 + 1
    Whp = ceil4(Wh) + extra_pad
    g = torch.Generator().manual_seed(_seed("amp", S, extra_pad))
    A = torch.randn(AMP_PLANES, 2 * S, Whp, generator=g)
    B = torch.randn(AMP_PLANES, 2 * S, Whp, generator=g)
    planted = {"zero dc": (0, 0, 0), "zero interior": (1, 1, 1), "zero last column": (4, S - 1, Wh - 1), "zero other sample": (5, 2, 1),
               "negative imaginary": (2, S - 1, 1), "denormal": (3, 1, Wh - 1)}
    for name, (p, ky, kx) in planted.items():
        if name.startswith("zero"):
            A[p, ky, kx], A[p, S + ky, kx] = 0.0, 0.0
            assert B[p, ky, kx] != 0 or B[p, S + ky, kx] != 0
        elif name == "negative imaginary":
            A[p, ky, kx], A[p, S + ky, kx] = 0.0, -0.75
        else:                                                  # modulus 5e-40: phase (-0.6, 0.8), which a flush to zero loses
            A[p, ky, kx], A[p, S + ky, kx] = -3e-40, 4e-40
            assert 0 < abs(float(A[p, ky, kx])) < 1.2e-38
    return {"A": A.contiguous(), "B": B.contiguous(), "lmda": AMP_LMDA, "S": S, "Wh": Wh, "Whp": Whp, "planted": planted}


def amp_mix_ref(inp, dt, mutation=None):
    """{"re", "im"} [P, S, Wh]: w * (l |A| + (1 - l) |B|) * A / |A| (|A| = 0: phase 0), w = 1 at kx = 0 and at the Nyquist
    column of an EVEN S only, 2 elsewhere"""
    _check(mutation, "nyquist_weight_at_odd_side")
    S, Wh = inp["S"], inp["Wh"]
    A, B = inp["A"].to(dt), inp["B"].to(dt)
    ar, ai, br, bi = A[:, :S, :Wh], A[:, S:, :Wh], B[:, :S, :Wh], B[:, S:, :Wh]
    ma, mb = torch.hypot(ar, ai), torch.hypot(br, bi)
    l = inp["lmda"].to(dt).repeat_interleave(AMP_PLANES_PER_SAMPLE).view(-1, 1, 1)
    amp = l * ma + (1.0 - l) * mb
    w = torch.full((Wh,), 2.0, dtype=dt)
    w[0] = 1.0
    if S % 2 == 0 or mutation == "nyquist_weight_at_odd_side":
        w[S // 2] = 1.0
    one, zero = torch.ones((), dtype=dt), torch.zeros((), dtype=dt)
    c, s = torch.where(ma > 0, ar / ma, one), torch.where(ma > 0, ai / ma, zero)
    return {"re": w * amp * c, "im": w * amp * s}


# ------------------------------------------------------------------------------------------------ plane transforms, GEMM path
DFT_SIDES = (13, 14, 37, 95)
DFT_PLANES = (1, 7)


@functools.lru_cache(maxsize=None)
def dft_inputs(S, P):
    Wh = S // 2 + 1
    Whp = ceil4(Wh)
    g = torch.Generator().manual_seed(_seed("dft", S, P))
    x = torch.randn(P, S, S, generator=g)
    G = torch.randn(P, 2 * S, Whp, generator=g)
    G[:, :, Wh:] = 0
    return {"x": x, "G": G.contiguous(), "S": S, "Wh": Wh, "Whp": Whp}


def dft_ref(inp, dt, ortho=True):
    """{"re", "im"}: torch.fft.rfft2 of the planes; {"adj"}: the gradient of sum(G * Y) through it (the adjoint)"""
    S, Wh = inp["S"], inp["Wh"]
    x = inp["x"].to(dt).requires_grad_()
    Y = torch.fft.rfft2(x, norm="ortho" if ortho else "backward")
    G = inp["G"].to(dt)
    (adj,) = torch.autograd.grad((Y.real * G[:, :S, :Wh]).sum() + (Y.imag * G[:, S:, :Wh]).sum(), x)
    return {"re": Y.real.detach(), "im": Y.imag.detach(), "adj": adj}


# ------------------------------------------------------------------------------------------------ amplitude transfer end to end
FREQ_CASES = ((2, 13), (3, 14), (2, 37), (2, 95), (2, 380))


def freq_ref(content, style, lmda, dt, mutation=None):
    """oracle.perturb.freq_style_transfer line by line in torch over a dtype (content, style [n, C, S, S]; lmda [n])"""
    _check(mutation, "nyquist_weight_at_odd_side")
    S = content.shape[-1]
    l = lmda.to(dt).view(-1, 1, 1, 1)
    fa = torch.fft.rfft2(content.to(dt), norm="ortho")
    fb = torch.fft.rfft2(style.to(dt), norm="ortho")
    amp = l * fa.abs() + (1.0 - l) * fb.abs()
    mixed = amp * torch.exp(1j * torch.angle(fa))
    if mutation == "nyquist_weight_at_odd_side" and S % 2 == 1:
        # the adjoint of rfft2 with weight 1 instead of 2 on column S // 2 = irfft2 of the spectrum with that column halved
        mixed = mixed.clone()
        mixed[..., S // 2] *= 0.5
    return torch.fft.irfft2(mixed, s=content.shape[-2:], norm="ortho")


# ------------------------------------------------------------------------------------------------ colour transfer
CORAL_SHAPES = ((2, 3, 5), (2, 37, 50), (2, 128, 128), (2, 129, 127), (4, 256, 256), (1, 380, 380))      # (n, H, W)
CORAL_FAMILIES = ("uniform", "photo")
CORAL_OLD_BAR = 5e-5          # what tests/test_c_perturb.py holds the colour branches to
MOMENT_CHUNKS = (1, 7, 16)


def moments_ref(x):
    """x [N, 3, H, W] float32 -> (sums [N, 9], sums of absolute terms [N, 9]) in float64: sum x_c (3), sum x_c x_d (00 01 02 11
    12 22).  The products of two float32 values are exact in float64, so only the order of the additions is open."""
    f = np.asarray(x, np.float64).reshape(x.shape[0], 3, -1)
    terms = [f[:, 0], f[:, 1], f[:, 2]] + [f[:, i] * f[:, j] for (i, j) in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return np.stack([t.sum(-1) for t in terms], 1), np.stack([np.abs(t).sum(-1) for t in terms], 1)


def affine_matrix(n):
    """[n, 3, 4] float32: a colour map near the identity with an offset, per sample"""
    g = torch.Generator().manual_seed(_seed("affine", n))
    return (torch.eye(3, 4).expand(n, 3, 4) + 0.3 * torch.randn(n, 3, 4, generator=g)).float().contiguous()


def affine3_ref(x, M, dt, mutation=None):
    """out[n, c] = sum_k M[n, c, k] x[n, k] + M[n, c, 3] on [N, 3, H, W]"""
    _check(mutation, "affine_offset_dropped")
    xf, m = x.to(dt).flatten(2), M.to(dt)
    out = m[:, :, :3] @ xf
    if mutation != "affine_offset_dropped":
        out = out + m[:, :, 3:]
    return out.view(x.shape)


def reference_svd(x):
    """numpy's SVD in the precision of x, every singular pair (u_i, v_i) given the sign that torch.linalg.svd gives it in
    float32 — the solver and the precision of the reference program's _mat_sqrt (utils/operation.py:15-17).

    Why: U sqrt(D) V flips with those signs, so the reference program's value is defined by its solver, and LAPACK's
    single-precision driver (torch, the reference, the product's host step) does not choose them like the double-precision one
    (numpy on float64) on near-degenerate covariances — noise images have three nearly equal singular values.  Measured: one
    image of tests/golden/udeb4_step_pert_n4.npz (recorded from the reference program) and 7 of the 12 colour cases below come
    out with another sign than numpy-float64's, an O(1) difference in the transferred image, although both are `the` SVD.
    The float64 factors are kept: only the signs are the reference solver's."""
    x = np.asarray(x)
    u, d, vh = np.linalg.svd(x)
    ut = torch.linalg.svd(torch.from_numpy(np.ascontiguousarray(x, np.float32)))[0].numpy().astype(u.dtype)
    sign = np.where((u * ut).sum(0) < 0, -1.0, 1.0).astype(u.dtype)
    return u * sign, d, vh * sign[:, None]


def coral_ref(source, target, dtype, mutation=None):
    """oracle.perturb.coral on arrays of `dtype` with the reference solver's signs (reference_svd); the mutation restates
    oracle.perturb.coral_one with the biased std"""
    _check(mutation, "coral_biased_std")
    s, t = np.asarray(source, dtype), np.asarray(target, dtype)
    if mutation is None:
        return OP.coral(s, t, svd=reference_svd)

    def stats(a):
        f = a.reshape(3, -1)
        mean = f.mean(-1, keepdims=True)
        std = f.std(-1, ddof=0, keepdims=True)
        fn = (f - mean) / std
        return fn, mean, std, fn @ fn.T + np.eye(3, dtype=a.dtype)

    def one(a, b):
        s_n, _, _, s_cov = stats(a)
        _, t_mean, t_std, t_cov = stats(b)
        out = OP.mat_sqrt(t_cov, reference_svd) @ (np.linalg.inv(OP.mat_sqrt(s_cov, reference_svd)) @ s_n)
        return (out * t_std + t_mean).reshape(a.shape)
    return np.stack([one(a, b) for a, b in zip(s, t)], 0)


# ------------------------------------------------------------------------------------------------ gathers and the blur
DOWNSCALE_SHAPES = ((2, 2), (3, 3), (5, 7), (37, 50), (95, 95), (380, 380))
BLUR_SHAPES = ((2, 3, 3, 3), (1, 3, 3, 50), (1, 3, 50, 3), (2, 3, 5, 7), (1, 3, 380, 380))
BLUR_BAR = 1e-6               # what tests/test_c_perturb.py holds the blur to


def downscale_ref(x):
    """the reference's own two calls (model/modules.py:19-21), nearest mode, on the CPU"""
    import torch.nn.functional as F
    return F.interpolate(F.interpolate(x, scale_factor=0.75), size=tuple(x.shape[-2:]))


# ------------------------------------------------------------------------------------------------ the branches of perturb_input
def replay_branch(x, pert_real, pert_fake, seed, color, svd=None):
    """The draws of model/unidefense.py:177-198 from the seeded global generator, fed to the oracle.  x: numpy [N, 3, H, W] of the
    precision the oracle is to run in; svd: the solver of the colour transfer (None: numpy's).  Returns (branch name, perturbed
    batch)."""
    dt = x.dtype
    torch.manual_seed(seed)
    style_branch = bool(torch.rand(1) > 0.5)
    if style_branch:
        st = OP.style_batch(x, pert_real, pert_fake)
        if color:
            st = OP.coral(st, x, svd)
        which = int(torch.randint(0, 2, size=(1,)))
        if which == 0:
            lm = (torch.rand((x.shape[0], 1, 1, 1)) / 2.0 + 0.5).numpy().astype(dt)
            return "freq", OP.freq_style_transfer(x, st, lm)
        lm = (torch.rand((x.shape[0], 1, 1)) / 2.0 + 0.5).numpy().astype(dt)
        return "spat", OP.spatial_style_transfer(x, st, lm)
    which = int(torch.randint(0, 3, size=(1,)))
    if which == 0:
        return "noise", OP.random_noise(x, torch.normal(0.0, 1e-4, size=x.shape).numpy().astype(dt))
    if which == 1:
        return "blur", OP.gaussian_blur5(x)
    return "down", OP.downscale(x)


def branch_of(seed):
    """the branch perturb_input takes after torch.manual_seed(seed) (leaves the global generator advanced)"""
    torch.manual_seed(seed)
    if bool(torch.rand(1) > 0.5):
        return ("freq", "spat")[int(torch.randint(0, 2, size=(1,)))]
    return ("noise", "blur", "down")[int(torch.randint(0, 3, size=(1,)))]


@functools.lru_cache(maxsize=None)
def seed_for(branch):
    """the smallest seed after which perturb_input takes `branch`"""
    state = torch.get_rng_state()
    try:
        return next(s for s in range(1000) if branch_of(s) == branch)
    finally:
        torch.set_rng_state(state)


BRANCH_N_REAL, BRANCH_N_FAKE, BRANCH_SIDE = 3, 2, 37
BRANCH_PERT_REAL, BRANCH_PERT_FAKE = (2, 0, 1), (1, 0)          # style partners: reals among reals, fakes among fakes

"""Proof, without a GPU, that the comparisons of tests/test_c_perturb_edges_gpu.py can fail: for every mutation of
tests/perturb_cases.py the mutated reference is further from the clean one than the bar the GPU test applies at the named
shape (an exact comparison rejects by differing at all), and is NOT where the table says so — which is why the suite was
blind to it at the sizes it had.  The bars are computed here exactly as on the GPU (parity.bar_of over the float32 yardstick
of the same reference lines).  Run with -s (or -rA) to see the table."""
import functools

import numpy as np
import pytest
import torch

from oracle import perturb as OP
from tests import parity
from tests import perturb_cases as pc

REJECT = 4.0          # a mutation that must show is at least this many bars away


def _rel(a, b):
    return parity.rel_err(torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b)))


def _yard_bar(scope, name, r32, r64, cap=None):
    yard = _rel(r32, r64)
    bar = parity.bar_of(f"{scope}/{name}", yard)[0]
    return yard, (bar if cap is None else min(cap, bar))


# ------------------------------------------------------------------------------------------------ the references themselves
def test_efdm_restatement_is_the_oracle_up_to_fp32_rounding():
    for family in pc.EFDM_FAMILIES:
        for L in (1, 65, 5136):
            c, s, lm = pc.efdm_inputs(family, L)
            ref = pc.efdm_ref(c, s, lm, pc.EFDM_ROWS_PER_SAMPLE)
            assert ref.dtype == np.float32 and np.isfinite(ref).all()
            l64 = np.repeat(lm.astype(np.float64), pc.EFDM_ROWS_PER_SAMPLE).reshape(2, 3, 1)
            o = OP.spatial_style_transfer(c.astype(np.float64).reshape(2, 3, 1, L), s.astype(np.float64).reshape(2, 3, 1, L), l64)
            assert _rel(ref.reshape(o.shape), o) <= 2e-7, (family, L)


@pytest.mark.parametrize("S", [4, 5, 13, 14])
def test_weighted_adjoint_of_the_mixed_spectrum_is_the_oracle(S):
    """amp_mix_ref (weight 2 on the interior columns, 1 at kx = 0 and at the Nyquist column of an even S) followed by the adjoint
    of rfft2 is oracle.perturb.freq_style_transfer; freq_ref is the same lines in torch"""
    a, b = pc.image_pair(2, 3, S, S, "uniform")
    lm = pc.distinct_lmda(2)
    want = OP.freq_style_transfer(a.double().numpy(), b.double().numpy(), lm.double().numpy().reshape(-1, 1, 1, 1))
    assert _rel(pc.freq_ref(a, b, lm, torch.float64), want) <= 1e-12
    Wh = S // 2 + 1

    def planes(t):
        Y = torch.fft.rfft2(t.double().view(6, S, S), norm="ortho")
        return torch.cat([Y.real, Y.imag], 1)
    mixed = pc.amp_mix_ref({"A": planes(a), "B": planes(b), "lmda": lm, "S": S, "Wh": Wh}, torch.float64)
    x = torch.zeros(6, S, S, dtype=torch.float64, requires_grad=True)
    Y = torch.fft.rfft2(x, norm="ortho")
    (adj,) = torch.autograd.grad((Y.real * mixed["re"]).sum() + (Y.imag * mixed["im"]).sum(), x)
    assert _rel(adj.view(2, 3, S, S), want) <= 1e-12


def test_clean_coral_reference_is_the_oracle_and_the_host_index_is_atens():
    s, t = pc.image_pair(2, 3, 3, 5, "uniform")
    assert np.array_equal(pc.coral_ref(s.numpy(), t.numpy(), np.float64), OP.coral(s.double().numpy(), t.double().numpy()))
    for (h, w) in pc.DOWNSCALE_SHAPES:
        x = pc.image_pair(2, 3, h, w, "uniform")[0]
        assert torch.equal(torch.from_numpy(OP.downscale(x.numpy())), pc.downscale_ref(x)), (h, w)


def test_reference_svd_is_an_svd_with_the_float32_solvers_signs():
    """the factors still multiply back to the matrix (a pair flips together), U sqrt(D) V equals what torch gives in float32 up to
    float32 accuracy, and with numpy's own signs some of the listed colour cases are O(1) away: the convention matters"""
    flipped = 0
    for family in pc.CORAL_FAMILIES:
        for (n, h, w) in pc.CORAL_SHAPES:
            for img in pc.image_pair(n, 3, h, w, family)[0].double().numpy():
                f = img.reshape(3, -1)
                fn = (f - f.mean(-1, keepdims=True)) / f.std(-1, ddof=1, keepdims=True)
                cov = fn @ fn.T + np.eye(3)
                u, d, vh = pc.reference_svd(cov)
                assert _rel((u * d) @ vh, cov) <= 1e-13
                u32, d32, vh32 = torch.linalg.svd(torch.from_numpy(cov).float())
                t32 = (u32 @ torch.diag(d32.sqrt()) @ vh32.t()).double().numpy()
                assert _rel(OP.mat_sqrt(cov, pc.reference_svd), t32) <= 1e-3, (family, n, h, w)
                flipped += _rel(OP.mat_sqrt(cov), t32) > 0.1
    print(f"  {flipped} covariances whose U sqrt(D) V flips between numpy-float64's signs and the float32 solver's")


def test_branch_seeds_exist_and_replay_is_deterministic():
    for b in ("freq", "spat", "noise", "blur", "down"):
        assert pc.branch_of(pc.seed_for(b)) == b
    x = pc.image_pair(5, 3, 9, 9, "uniform")[0].double().numpy()
    for b in ("freq", "spat"):
        for color in (False, True):
            n1, o1 = pc.replay_branch(x, pc.BRANCH_PERT_REAL, pc.BRANCH_PERT_FAKE, pc.seed_for(b), color)
            n2, o2 = pc.replay_branch(x, pc.BRANCH_PERT_REAL, pc.BRANCH_PERT_FAKE, pc.seed_for(b), color)
            assert n1 == n2 == b and np.array_equal(o1, o2) and o1.shape == x.shape


# ------------------------------------------------------------------------------------------------ the mutation table
def _efdm_row(mutation, family, L):
    c, s, lm = pc.efdm_inputs(family, L)
    clean = pc.efdm_ref(c, s, lm, pc.EFDM_ROWS_PER_SAMPLE)
    mut = pc.efdm_ref(c, s, lm, pc.EFDM_ROWS_PER_SAMPLE, mutation)
    return float((clean != mut).mean()), 0.0          # share of entries that differ as floats; the bar of np.array_equal


def _amp_row(mutation, S):
    inp = pc.amp_inputs(S)
    r64, r32, m64 = pc.amp_mix_ref(inp, torch.float64), pc.amp_mix_ref(inp, torch.float32), pc.amp_mix_ref(inp, torch.float64, mutation)
    rows = [(_rel(m64[q], r64[q]),) + _yard_bar("test_amp_mix_planted_spectra", q, r32[q], r64[q]) for q in ("re", "im")]
    err, _, bar = max(rows, key=lambda r: r[0] / r[2])
    return err, bar


def _freq_row(mutation, n, S):
    a, b = pc.image_pair(n, 3, S, S, "uniform")
    lm = pc.distinct_lmda(n)
    r64, r32 = pc.freq_ref(a, b, lm, torch.float64), pc.freq_ref(a, b, lm, torch.float32)
    _, bar = _yard_bar("test_freq_transfer_end_to_end", "freq", r32, r64)
    return _rel(pc.freq_ref(a, b, lm, torch.float64, mutation), r64), bar


def _coral_row(mutation, n, h, w, family):
    s, t = pc.image_pair(n, 3, h, w, family)
    r64, r32 = pc.coral_ref(s.numpy(), t.numpy(), np.float64), pc.coral_ref(s.numpy(), t.numpy(), np.float32)
    _, bar = _yard_bar("test_coral_vs_oracle", "coral", r32, r64, cap=pc.CORAL_OLD_BAR)
    return _rel(pc.coral_ref(s.numpy(), t.numpy(), np.float64, mutation), r64), bar


def _affine_row(mutation, n, h, w):
    x = pc.image_pair(n, 3, h, w, "uniform")[0]
    M = pc.affine_matrix(n)
    r64, r32 = pc.affine3_ref(x, M, torch.float64), pc.affine3_ref(x, M, torch.float32)
    _, bar = _yard_bar("test_affine3_vs_float64", "affine3", r32, r64)
    return _rel(pc.affine3_ref(x, M, torch.float64, mutation), r64), bar


# (mutation, where, row function, arguments, must it show there: True / False / None = recorded only)
TABLE = (
    ("nyquist_weight_at_odd_side", "amp_mix S=13", _amp_row, (13,), True),
    ("nyquist_weight_at_odd_side", "amp_mix S=5", _amp_row, (5,), True),
    ("nyquist_weight_at_odd_side", "amp_mix S=8", _amp_row, (8,), False),
    ("nyquist_weight_at_odd_side", "freq (2, 13)", _freq_row, (2, 13), True),
    ("nyquist_weight_at_odd_side", "freq (2, 37)", _freq_row, (2, 37), True),
    ("nyquist_weight_at_odd_side", "freq (3, 14): why the old suite was blind", _freq_row, (3, 14), False),
    ("ties_in_reverse_order", "efdm levels8 L=65", _efdm_row, ("levels8", 65), True),
    ("ties_in_reverse_order", "efdm levels8 L=5136", _efdm_row, ("levels8", 5136), True),
    ("ties_in_reverse_order", "efdm three L=1025", _efdm_row, ("three", 1025), True),
    ("ties_in_reverse_order", "efdm uniform L=5136 (no ties)", _efdm_row, ("uniform", 5136), False),
    ("neg_zero_sorts_first", "efdm signs L=65", _efdm_row, ("signs", 65), True),
    ("neg_zero_sorts_first", "efdm signs L=5136", _efdm_row, ("signs", 5136), True),
    ("neg_zero_sorts_first", "efdm levels8 L=5136 (no zeros of either sign)", _efdm_row, ("levels8", 5136), False),
    ("last_partial_round_dropped", "efdm uniform L=5136", _efdm_row, ("uniform", 5136), True),
    ("last_partial_round_dropped", "efdm uniform L=4097", _efdm_row, ("uniform", 4097), True),
    ("last_partial_round_dropped", "efdm uniform L=4096", _efdm_row, ("uniform", 4096), False),
    ("coral_biased_std", "coral 3 x 5 uniform", _coral_row, (2, 3, 5, "uniform"), True),
    ("coral_biased_std", "coral 3 x 5 photo", _coral_row, (2, 3, 5, "photo"), None),
    ("coral_biased_std", "coral 256 x 256 uniform", _coral_row, (4, 256, 256, "uniform"), None),
    ("affine_offset_dropped", "affine3 3 x 5", _affine_row, (2, 3, 5), True),
    ("affine_offset_dropped", "affine3 256 x 256", _affine_row, (4, 256, 256), True),
)


@functools.lru_cache(maxsize=None)
def _row(i):
    mutation, where, fn, args, _ = TABLE[i]
    return fn(mutation, *args)


def _shows(err, bar):
    return err > bar


@pytest.mark.parametrize("i", range(len(TABLE)), ids=[f"{m}-{w.split(':')[0].replace(' ', '_')}" for m, w, _, _, _ in TABLE])
def test_mutation_shows_where_the_table_says(i):
    mutation, where, _, _, must = TABLE[i]
    err, bar = _row(i)
    print(f"  {mutation} at {where}: err {err:.3g}, bar {bar:.3g}")
    if must is True:
        assert err >= REJECT * bar and err > 0, (mutation, where, err, bar)
    elif must is False:
        assert err == 0.0, (mutation, where, err, bar)          # the mutated reference IS the clean one there


def test_every_mutation_is_rejected_somewhere_and_print_the_table():
    print("\nmutation | where | difference (max-norm relative; efdm: share of entries that differ) | bar | seen")
    rejected = set()
    for i, (mutation, where, _, _, must) in enumerate(TABLE):
        err, bar = _row(i)
        seen = _shows(err, bar)
        if seen and must is True:
            rejected.add(mutation)
        print(f"  {mutation} | {where} | {err:.3g} | {bar:.3g} | {'yes' if seen else 'no'}"
              f"{'' if must is not None else '   (recorded, not required)'}")
    assert rejected == set(pc.MUTATIONS), set(pc.MUTATIONS) - rejected


def test_ties_shares_are_what_the_issue_measured():
    """about 17 % of the entries differ at L = 65 and 49 % at L = 5136 when the ties of 8-bit rows come out in reverse order"""
    assert 0.08 <= _efdm_row("ties_in_reverse_order", "levels8", 65)[0] <= 0.30
    assert 0.40 <= _efdm_row("ties_in_reverse_order", "levels8", 5136)[0] <= 0.60

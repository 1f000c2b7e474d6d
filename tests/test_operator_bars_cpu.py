"""Proof, without a GPU, that the yardstick bars of tests/parity.py discriminate: for every case of tests/operator_cases.py
and every quantity the bar the GPU test will apply is computed from the float32 / float64 references alone, and then
 * the yardstick itself passes it (trivially, MARGIN >= 1) and the number of quantities whose bar is the floor is reported;
 * every mutation listed for the case is REJECTED with 4x to spare: some quantity of ref(float64, mutation) is at least
   4 x its bar away from ref(float64) (an exact quantity rejects by differing at all);
 * every mutation marked `subtle` has a witness: a case that rejects it while no quantity of the mutated reference is more
   than 1e-3 away — the bar these operators were held to before could not see it.
The named bars of parity.EXPLICIT_BARS are applied here exactly as on the GPU (parity.bar_of), so a case must reject its
mutations under them as well.  Run with -s (or -rA) to see the table."""
import functools

import pytest
import torch

from tests import operator_cases as oc
from tests import parity

REJECT = 4.0


@functools.lru_cache(maxsize=None)
def _evaluate(name):
    """bars, yardsticks and mutation errors of one case: {"bars": {q: (yard, bar)}, "mut": {m: {q: err}}}"""
    case = oc.BY_NAME[name]
    inp, r64, r32 = oc.refs(case)
    assert set(r64) == set(r32)
    bars = {}
    for q in r64:
        if q in case.exact:
            bars[q] = (0.0, 0.0)
        else:
            yard = parity.rel_err(r32[q], r64[q])
            bars[q] = (yard, parity.bar_of(f"{name}/{q}", yard)[0])
    mut = {}
    for m in case.mutations:
        rm = case.ref(inp, torch.float64, m)
        assert set(rm) == set(r64)
        mut[m] = {q: parity.rel_err(rm[q], r64[q]) for q in r64}
    return {"bars": bars, "mut": mut}


def _ratio(err, bar):
    return err / bar if bar > 0 else (float("inf") if err > 0 else 0.0)


def _worst(res, m):
    """(largest err / bar over the quantities, that quantity, largest err) of mutation m in an evaluated case"""
    errs = res["mut"][m]
    q = max(errs, key=lambda k: _ratio(errs[k], res["bars"][k][1]))
    return _ratio(errs[q], res["bars"][q][1]), q, max(errs.values())


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_case_bars_pass_the_yardstick_and_reject_the_mutations(case):
    res = _evaluate(case.name)
    _, r64, r32 = oc.refs(case)
    for q, (yard, bar) in res["bars"].items():
        assert torch.isfinite(r64[q]).all() and torch.isfinite(r32[q]).all(), q
        assert yard <= bar <= parity.OLD_BAR, (q, yard, bar)          # the fp32 reference passes; never looser than before
        if q in case.exact:
            assert torch.equal(r32[q].double(), r64[q].double()), q   # exact quantities are exact in any precision
    for m in case.mutations:
        ratio, q, _ = _worst(res, m)
        print(f"  {case.name}: {m} rejected through {q}: err / bar = {ratio:.3g}")
        assert ratio >= REJECT, (m, res["mut"][m], res["bars"])


def test_every_mutation_has_a_rejecting_case_and_the_subtle_ones_a_witness():
    rejecting, witness = {}, {}
    on_floor = total = 0
    for case in oc.CASES:
        res = _evaluate(case.name)
        for q, (yard, bar) in res["bars"].items():
            if q not in case.exact:
                total += 1
                on_floor += bar == parity.FLOOR
        for m in case.mutations:
            ratio, q, worst_err = _worst(res, m)
            if ratio >= REJECT and ratio > rejecting.get(m, (0.0,))[0]:
                rejecting[m] = (ratio, case.name, q)
            if ratio >= REJECT and worst_err <= parity.OLD_BAR and ratio > witness.get(m, (0.0,))[0]:
                witness[m] = (ratio, case.name, q, worst_err)
    print(f"\n{len(oc.CASES)} cases, {total} quantities on a yardstick bar, {on_floor} of them on the floor ({parity.FLOOR:g})")
    print("mutation -> best rejecting case (quantity): err / bar")
    for m in oc.MUTATIONS:
        assert m in rejecting, f"{m}: no listed case rejects it at {REJECT}x"
        ratio, name, q = rejecting[m]
        print(f"  {m}: {name} ({q}): {ratio:.3g}")
    print("subtle mutations -> witness (rejected, yet every quantity within the old 1e-3 bar): largest error, err / bar")
    for m, subtle in oc.MUTATIONS.items():
        if subtle:
            assert m in witness, f"{m}: marked subtle, but every rejecting case shows it above {parity.OLD_BAR}"
            ratio, name, q, worst_err = witness[m]
            assert worst_err <= parity.OLD_BAR
            print(f"  {m}: {name} ({q}): {worst_err:.3g}, {ratio:.3g}")
        else:
            assert m not in witness, f"{m}: a case shows it within {parity.OLD_BAR}: mark it subtle"
    assert 0 < on_floor < total            # the floor is not doing all the work, and some yardsticks do sit under it


def test_explicit_bars_are_within_their_caps():
    n_named = 0
    for case in oc.CASES:
        for q, (yard, bar) in _evaluate(case.name)["bars"].items():
            cause = parity.bar_of(f"{case.name}/{q}", yard)[1]
            n_named += cause is not None
            assert bar <= (parity.EXPLICIT_CAP if cause else parity.OLD_BAR)
    for pat, margin, cause in parity.EXPLICIT_BARS:
        assert margin > parity.MARGIN and len(cause) > 20, pat
    total = sum(len(_evaluate(c.name)["bars"]) for c in oc.CASES)
    assert n_named <= parity.EXPLICIT_SHARE * total


def test_maxpool_reference_forms_agree():
    """the unfold form the tie mutation is written in is the max-pool: with the FIRST maximum it is ATen's, gradient included"""
    x = oc._pool_input((2, 8, 15, 15), "halves", 5).double().requires_grad_()
    gy = oc.rnd(2, 8, 8, 8, seed=6).double()
    flipped = oc._maxpool_last(x.flip(2, 3)).flip(2, 3)         # odd side: the windows map onto themselves, last becomes first
    ref = torch.nn.functional.max_pool2d(x, 3, 2, 1)
    assert torch.equal(flipped, ref)
    (g1,), (g2,) = torch.autograd.grad(flipped, x, gy), torch.autograd.grad(ref, x, gy)
    assert torch.equal(g1, g2)

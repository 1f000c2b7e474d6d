"""GPU side of the operator parity bars: every case of tests/operator_cases.py runs through the HIP operator
(unidefense_amd.tape) and each quantity is held to the yardstick bar of tests/parity.py — max(2e-6, 8 x the error of plain
torch float32 on the CPU against float64 on the same inputs) — or, where the case names it exact, compared bit for bit after
the cast to float32.  tests/test_operator_bars_cpu.py proves on the CPU that these bars reject the subtly wrong variants
listed with each case.  Every output must be finite (a channel of variance exactly 0 included)."""
import pytest
import torch

from tests import operator_cases as oc
from tests.margins import within
from tests.parity import rel_err, yard_check

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_operator_case(case):
    dev = _dev()
    inp, r64, r32 = oc.refs(case)
    got = case.run(inp, dev)
    assert set(got) == set(r64), (sorted(got), sorted(r64))
    bad = []
    for q in sorted(r64):
        g = got[q].detach().float().cpu()
        assert g.shape == r64[q].shape, (q, g.shape, r64[q].shape)
        assert torch.isfinite(g).all(), q
        try:
            if q in case.exact:
                e = rel_err(g, r64[q])
                print(f"  {q}: exact comparison, rel err {e:.3e}")
                assert within(q + " [exact]", e, 0.0) and torch.equal(g, r64[q].float()), f"{q}: not bit-equal ({e:.3e})"
            else:
                yard_check(q, g, r64[q], r32[q], scope=case.name)
        except AssertionError as err:                 # every quantity of the case is measured and recorded before it fails
            bad.append(str(err))
    assert not bad, bad

"""The yardstick bar of the operator-level parity tests.

A HIP operator is compared with a float64 reference of the same operation.  How far it may be from that reference is not a
constant: it is set by how far *plain torch in float32 on the CPU*, running the very same reference lines on the very same
inputs, is from float64 (the yardstick), times a margin for what legitimately differs between a HIP kernel and ATen's fp32
(summation order, FMA contraction, __expf-class intrinsics), and never below the project's own fp32 floor:

    yard = rel_err(ref32, ref64)            bar = max(FLOOR, MARGIN * yard)

FLOOR = 2e-6 is the bar tests/test_a_kernels_gpu.py::test_gemm_every_tile_configuration_and_split holds the split-bf16
GEMMs to (about 16 eps), MARGIN = 8.  Neither is tuned to what the kernels do; tests/test_operator_bars_cpu.py proves on
the CPU that the resulting bars reject subtly wrong operators (tests/operator_cases.py: the mutations) with 4x to spare.

A quantity whose legitimate error does not fit gets a NAMED bar in EXPLICIT_BARS: a cause (with its source line) and a
rule — a larger stated margin over the same yardstick, capped at EXPLICIT_CAP.  Never a copy of an observed value.

A plain helper module: no conftest, no plugin, no pytest setting.
"""
import re

FLOOR = 2e-6
MARGIN = 8.0
OLD_BAR = 1e-3            # what every one of these quantities was held to before (RTOL of tests/test_a_kernels_gpu.py)
EXPLICIT_CAP = 1e-4       # no named bar may exceed this in the max-norm metric
EXPLICIT_SHARE = 0.1      # ... and at most this share of all recorded yardstick quantities may have one


def rel_err(a, b):
    """max |a - b| / max |b|: the max-norm relative error every operator test of the suite uses"""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# (pattern on "<test function or case name>/<quantity>", margin over the yardstick, cause).  The bar of a match is
# min(EXPLICIT_CAP, max(FLOOR, margin * yard)).
EXPLICIT_BARS = ()


def bar_of(name, yard, floor=FLOOR, margin=MARGIN):
    """(bar, cause or None) of the quantity `name` ("<test or case>/<quantity>") whose fp32 yardstick is `yard`"""
    for pat, m, cause in EXPLICIT_BARS:
        if re.search(pat, name):
            assert m > margin, (name, m)
            return min(EXPLICIT_CAP, max(floor, m * yard)), cause
    return max(floor, margin * yard), None


def _scope():
    """test function name (without the parameter id) of the running test: the scope the EXPLICIT_BARS patterns match on"""
    import os
    cur = os.environ.get("PYTEST_CURRENT_TEST", "")
    return cur.split(" ")[0].split("::")[-1].split("[")[0]


def yard_check(name, got, ref64, ref32, floor=FLOOR, margin=MARGIN, scope=None):
    """Hold `got` to max(floor, margin * rel_err(ref32, ref64)) of ref64 (or to the quantity's named bar); both the kernel's
    error and the yardstick are recorded (tests/margins.py) under the same bar.  Returns (error, yardstick, bar)."""
    from tests.margins import within
    yard = rel_err(ref32, ref64)
    bar, cause = bar_of(f"{scope if scope is not None else _scope()}/{name}", yard, floor, margin)
    assert bar <= OLD_BAR, f"{name}: yardstick {yard:.3e} puts the bar at {bar:.3e}, looser than the {OLD_BAR} it replaces"
    e = rel_err(got, ref64)
    print(f"  {name}: rel err {e:.3e}   fp32 yardstick {yard:.3e}   bar {bar:.3e}{'   [named bar]' if cause else ''}")
    within(name + " [yard]", yard, bar)
    assert within(name, e, bar), f"{name}: rel err {e:.3e} > bar {bar:.3e} (fp32 yardstick {yard:.3e})"
    return e, yard, bar

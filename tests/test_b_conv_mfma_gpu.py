"""csrc/conv_mfma.hip — the decoder's direct 3x3 convolution on the matrix pipe (forward, data gradient, the transposed
stride-2 forward and its stride-2 data gradient), reached through kernels.conv_gather_nt with the dispatch threshold forced
to 1 and every instantiated (Cin, Cout, geometry) routed.

 * against F.conv2d / F.conv_transpose2d in float64, 1e-5 of max|ref| (the bar of the existing conv tests), on an output of
   12 x 20 (ragged against every tile, H != W, both parities on the edges) and one smaller than any tile whose every pixel
   touches the border (5 x 7; the transposed conv's output is 2 Hin x 2 Win and cannot be odd: its input is 3 x 7, the output
   6 x 14);
 * on hard inputs (randn, sign-randomised lognormal(sigma = 3), an all-zero image next to a 1e4-scaled one; weights at 1e-3):
   worst error / sum |a||b| against float64 at most 2 x that of the path it replaces on the same input, floor 2e-6 — the rule
   of test_prec2_has_fp32_gemm_accuracy;
 * the stage scale of the weights (it follows each stage's |w|max and rescales the accumulators by a power of two): taps and
   channel chunks 2^23 apart in both orders, a run of shrinking taps that reaches the cap on up-scaling, and a tiny tap followed
   by a huge one that reaches the clamp of the ratio — same error rule;
 * bitwise equal on a second run;
 * one decoder block (conv_dense 80 -> 40, InstanceNorm + swish, conv_transpose_s2 40 -> 40, InstanceNorm + swish, conv_dense
   40 -> 40, InstanceNorm + swish) through the tape with the new path on and off: y, dx and every dw within 1e-5.

The weight-gradient kernel (ud_conv_mfma_wgrad, through kernels.conv_gather_wgrad): every instantiated (gathered channels, Ma,
geometry) against float64 autograd on the same two output grids, 1e-5 of max|ref|; bitwise equal on a second run; and the dw
lines of the decoder block, which the new kernel computes in the `on` arm."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SAME = [(20, 20), (40, 20), (40, 40), (20, 40), (80, 40), (80, 80), (40, 80), (160, 80), (80, 160)]
TRANSPOSED = [(20, 20), (40, 40), (80, 80)]
STRIDE2 = [(20, 20), (40, 40), (80, 80)]
CASES = [("same", ci, co) for ci, co in SAME] + [("transposed_s2", ci, co) for ci, co in TRANSPOSED] + \
        [("stride2", ci, co) for ci, co in STRIDE2]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def to_pix(t):
    return t.permute(0, 2, 3, 1).contiguous()


def to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _problem(Kk, geom, n, ho, wo, ci, co, x, w):
    """(float64 reference function, geometry, weight matrix) of one conv; x [n, ci, hin, win], w in the module's layout"""
    if geom == "same":
        gm = Kk.conv_geom(n, ho, wo, ci, ho, wo, 3, 3, 1, 1, 1, 0)
        return (lambda a, b: F.conv2d(a, b, padding=1)), gm, w.permute(0, 2, 3, 1).reshape(co, 9 * ci)
    if geom == "transposed_s2":
        gm = Kk.conv_geom(n, ho // 2, wo // 2, ci, ho, wo, 3, 3, 2, 1, 1, 1)
        return (lambda a, b: F.conv_transpose2d(a, b, stride=2, padding=1, output_padding=1)), gm, \
            w.permute(1, 2, 3, 0).reshape(co, 9 * ci)
    gm = Kk.conv_geom(n, 2 * ho, 2 * wo, ci, ho, wo, 3, 3, 2, 1, 1, 0)
    return (lambda a, b: F.conv2d(a, b, stride=2, padding=1)), gm, w.permute(0, 2, 3, 1).reshape(co, 9 * ci)


def _in_hw(geom, ho, wo):
    return (ho, wo) if geom == "same" else (ho // 2, wo // 2) if geom == "transposed_s2" else (2 * ho, 2 * wo)


def _w_shape(geom, ci, co):
    return (ci, co, 3, 3) if geom == "transposed_s2" else (co, ci, 3, 3)


class _Route:
    """conv_gather_nt with the MFMA path forced on for every instantiated shape (on=True) or off"""

    def __init__(self, Kk, on):
        self.K, self.on = Kk, on

    def __enter__(self):
        Kk = self.K
        self.saved = Kk._CONV_MFMA, Kk._CONV_MFMA_MIN_M, Kk._CONV_MFMA_SHAPES, Kk._CONV_MFMA_WGRAD_SHAPES
        Kk._CONV_MFMA, Kk._CONV_MFMA_MIN_M, Kk._CONV_MFMA_SHAPES, Kk._CONV_MFMA_WGRAD_SHAPES = self.on, 1, None, None

    def __exit__(self, *exc):
        Kk = self.K
        Kk._CONV_MFMA, Kk._CONV_MFMA_MIN_M, Kk._CONV_MFMA_SHAPES, Kk._CONV_MFMA_WGRAD_SHAPES = self.saved


def _mode(geom):
    return {"same": 0, "transposed_s2": 1, "stride2": 2}[geom]


@pytest.mark.parametrize("geom,ci,co", CASES)
def test_conv_mfma_equals_float64(geom, ci, co):
    dev = _dev()
    from unidefense_amd import kernels as Kk
    from tests.margins import within
    assert Kk._call("ud_conv_mfma_supported", ci, co, _mode(geom)) == 1
    gen = torch.Generator().manual_seed(1000 * _mode(geom) + 10 * ci + co)
    for n, ho, wo in ((2, 12, 20), (1, 6, 14) if geom == "transposed_s2" else (1, 5, 7)):
        hi, wi = _in_hw(geom, ho, wo)
        x = torch.randn(n, ci, hi, wi, generator=gen)
        w = torch.randn(*_w_shape(geom, ci, co), generator=gen)
        ref_fn, gm, wmat = _problem(Kk, geom, n, ho, wo, ci, co, x, w)
        ref = ref_fn(x.double(), w.double())
        assert Kk._conv_mfma_mode(gm) == _mode(geom)
        with _Route(Kk, True):
            assert Kk._conv_mfma_takes(gm, co, n * ho * wo, x.to(dev), wmat.contiguous().to(dev))
            got = Kk.conv_gather_nt(to_pix(x).to(dev), wmat.contiguous().to(dev), gm)
        torch.cuda.synchronize()
        got = to_nchw(got).double().cpu()
        assert got.shape == ref.shape
        e = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"  conv_mfma {geom} {ci}->{co} out {n}x{ho}x{wo}: rel err {e:.3e}")
        assert within(f"conv_mfma {geom} {ci}->{co} out {ho}x{wo} vs fp64", e, 1e-5)


# (gathered channels, Ma): a conv's weight gradient gathers x (Cin) against dy (Cout); a transposed conv's gathers dy at stride 2
WGRAD_CASES = [("same", ci, ma) for ci, ma in [(160, 80), (80, 80), (80, 40), (40, 40), (40, 20), (20, 20)]] + \
              [("convT", c, c) for c in (80, 40, 20)]


def _wgrad_problem(Kk, geom, n, ho, wo, ci, ma, gen):
    """(a, gathered tensor, geometry, float64 weight gradient as [Ma, 9 * ci]) on an output grid of ho x wo"""
    if geom == "same":
        x = torch.randn(n, ci, ho, wo, generator=gen)
        dy = torch.randn(n, ma, ho, wo, generator=gen)
        w = torch.zeros(ma, ci, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), w, padding=1).backward(dy.double())
        gm = Kk.conv_geom(n, ho, wo, ci, ho, wo, 3, 3, 1, 1, 1, 0)
        return to_pix(dy).view(-1, ma), to_pix(x), gm, w.grad.permute(0, 2, 3, 1).reshape(ma, 9 * ci)
    # ConvTranspose2d(ma -> ci channels, k3, s2, p1, op1) on a ho x wo input: a = its input, dy (2 ho x 2 wo) gathered at stride 2
    x = torch.randn(n, ma, ho, wo, generator=gen)
    dy = torch.randn(n, ci, 2 * ho, 2 * wo, generator=gen)
    w = torch.zeros(ma, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(x.double(), w, stride=2, padding=1, output_padding=1).backward(dy.double())
    gm = Kk.conv_geom(n, 2 * ho, 2 * wo, ci, ho, wo, 3, 3, 2, 1, 1, 0)
    return to_pix(x).view(-1, ma), to_pix(dy), gm, w.grad.permute(0, 2, 3, 1).reshape(ma, 9 * ci)


@pytest.mark.parametrize("geom,ci,ma", WGRAD_CASES)
def test_conv_mfma_wgrad_equals_float64(geom, ci, ma):
    dev = _dev()
    from unidefense_amd import kernels as Kk
    from tests.margins import within
    mode = 0 if geom == "same" else 2
    assert Kk._call("ud_conv_mfma_wgrad_supported", ci, ma, mode) == 1
    gen = torch.Generator().manual_seed(77 + 10 * ci + ma + mode)
    for n, ho, wo in ((2, 12, 20), (1, 5, 7)):
        a, xg, gm, ref = _wgrad_problem(Kk, geom, n, ho, wo, ci, ma, gen)
        a, xg = a.contiguous().to(dev), xg.to(dev)
        with _Route(Kk, True):
            assert Kk._conv_mfma_wgrad_takes(gm, ma, n * ho * wo, a, xg)
            got = Kk.conv_gather_wgrad(a, xg, gm)
            again = Kk.conv_gather_wgrad(a, xg, gm)
        torch.cuda.synchronize()
        assert torch.equal(got, again)          # fixed-order partial sums: a second run is bitwise the first
        got = got.double().cpu()
        assert got.shape == ref.shape
        e = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"  conv_mfma_wgrad {geom} {ci}x{ma} grid {n}x{ho}x{wo}: rel err {e:.3e}")
        assert within(f"conv_mfma_wgrad {geom} {ci}x{ma} grid {ho}x{wo} vs fp64", e, 1e-5)


def test_conv_mfma_wgrad_many_tiles_per_workgroup():
    """2 x 64 x 64 pixels = 512 tiles: every workgroup walks several tiles and more than one partial is folded"""
    dev = _dev()
    from unidefense_amd import kernels as Kk
    from tests.margins import within
    gen = torch.Generator().manual_seed(5)
    a, xg, gm, ref = _wgrad_problem(Kk, "same", 2, 64, 64, 40, 20, gen)
    a, xg = a.contiguous().to(dev), xg.to(dev)
    with _Route(Kk, True):
        got = Kk.conv_gather_wgrad(a, xg, gm)
    torch.cuda.synchronize()
    e = ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"  conv_mfma_wgrad same 40x20 grid 2x64x64: rel err {e:.3e}")
    assert within("conv_mfma_wgrad same 40x20 grid 64x64 vs fp64", e, 1e-5)


def _hard_input(kind, shape, gen):
    if kind == "randn":
        return torch.randn(*shape, generator=gen)
    if kind == "lognormal":
        sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
        return sign * torch.exp(3 * torch.randn(*shape, generator=gen))
    x = torch.randn(*shape, generator=gen) * 1e4          # an all-zero image next to a 1e4-scaled one
    x[0] = 0
    return x


@pytest.mark.parametrize("kind", ["randn", "lognormal", "zero_and_1e4"])
@pytest.mark.parametrize("geom,c", [("same", 40), ("same", 80), ("transposed_s2", 40), ("transposed_s2", 80)])
def test_conv_mfma_has_fp32_gemm_accuracy_on_hard_inputs(geom, c, kind):
    """output 2 x 16 x 24: several tiles per image at every tile shape; the error is taken relative to sum |a||b|, the
    quantity an fp32 GEMM's error scales with"""
    dev = _dev()
    from unidefense_amd import kernels as Kk
    from tests.margins import within, record
    n, ho, wo = 2, 16, 24
    gen = torch.Generator().manual_seed(c + len(kind))
    hi, wi = _in_hw(geom, ho, wo)
    x = _hard_input(kind, (n, c, hi, wi), gen)
    w = torch.randn(*_w_shape(geom, c, c), generator=gen) * 1e-3
    ref_fn, gm, wmat = _problem(Kk, geom, n, ho, wo, c, c, x, w)
    want = ref_fn(x.double(), w.double())
    scale = ref_fn(x.double().abs(), w.double().abs()) + 1e-300
    xp, wm = to_pix(x).to(dev), wmat.contiguous().to(dev)
    errs = {}
    for on in (False, True):
        with _Route(Kk, on):
            o = Kk.conv_gather_nt(xp, wm, gm)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all()
        errs[on] = ((to_nchw(o).double().cpu() - want).abs() / scale).max().item()
    print(f"  {geom} {c}->{c} {kind}: err / sum|a||b|  replaced path {errs[False]:.3e}  conv_mfma {errs[True]:.3e}")
    record(f"replaced path {geom} {c}->{c} {kind} err / sum|a||b|", errs[False], float("inf"))
    assert within(f"conv_mfma {geom} {c}->{c} {kind} err / sum|a||b| (bar: the replaced path's x 2, floor 2e-6)",
                  errs[True], max(2e-6, 2 * errs[False]))
    if kind == "zero_and_1e4":
        with _Route(Kk, True):
            o = Kk.conv_gather_nt(xp, wm, gm)
        assert (o[0] == 0).all()          # the all-zero image's tiles carry their own scale


def _uneven_weights(kind, geom, w):
    """w scaled per tap (and per 40-channel chunk of the reduction, the stage of the 80-channel kernels)"""
    if kind == "mixed":          # neighbouring stages 2^23 apart, both directions
        taps = [1e2, 1e-5, 1e2, 1e-5, 1.0, 1e2, 1e-5, 1e-5, 1e2]
    elif kind == "shrinking":    # every stage far below the one before: up-scaling, up to the 2^80 cap
        taps = [1e2, 1e-2, 1e-6, 1e-9, 1e-12, 1e-15, 1e-18, 1e-21, 1e-24]
    else:                        # "tiny_then_huge": the scale falls by more than 2^126 in one step.  A scale shared by a tile
        # resolves 2^-25 of the largest weight in play, so the tiny taps are invisible next to the huge ones, as they are in
        # sum |a||b| — wherever a pixel sees a huge tap.  Taps 4, 5, 7, 8 are huge: every output pixel of both geometries sees
        # one of them (the corners of the padded conv see {4,5,7,8}, {3,4,6,7}, {1,2,4,5}, {0,1,3,4}; the parities of the
        # transposed conv {4}, {3,5}, {1,7}, {0,2,6,8}, its last row / column {7}, {6,8}, {5}, {2,8}, {8}).
        taps = [3e-37, 3e-37, 3e-37, 3e-37, 1e30, 1e30, 3e-37, 1e30, 1e30]
    w = w * torch.tensor(taps, dtype=w.dtype).view(1, 1, 3, 3)
    if kind == "mixed":
        red = 0 if geom == "transposed_s2" else 1          # the reduced channel's axis
        half = w.shape[red] // 2
        idx = [slice(None)] * 4
        idx[red] = slice(0, half)
        w[tuple(idx)] *= 1e-4
    return w


@pytest.mark.parametrize("kind", ["mixed", "shrinking", "tiny_then_huge"])
@pytest.mark.parametrize("geom,c", [("same", 40), ("same", 80), ("transposed_s2", 40)])
def test_conv_mfma_stage_scale_follows_uneven_weights(geom, c, kind):
    dev = _dev()
    from unidefense_amd import kernels as Kk
    from tests.margins import within, record
    n, ho, wo = 2, 16, 24
    gen = torch.Generator().manual_seed(3 * c + len(kind))
    hi, wi = _in_hw(geom, ho, wo)
    x = torch.randn(n, c, hi, wi, generator=gen)
    w = _uneven_weights(kind, geom, torch.randn(*_w_shape(geom, c, c), generator=gen))
    ref_fn, gm, wmat = _problem(Kk, geom, n, ho, wo, c, c, x, w)
    want = ref_fn(x.double(), w.double())
    scale = ref_fn(x.double().abs(), w.double().abs()) + 1e-300
    xp, wm = to_pix(x).to(dev), wmat.contiguous().to(dev)
    errs = {}
    for on in (False, True):
        with _Route(Kk, on):
            o = Kk.conv_gather_nt(xp, wm, gm)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all()
        errs[on] = ((to_nchw(o).double().cpu() - want).abs() / scale).max().item()
    print(f"  {geom} {c}->{c} weights {kind}: err / sum|a||b|  replaced path {errs[False]:.3e}  conv_mfma {errs[True]:.3e}")
    record(f"replaced path {geom} {c}->{c} weights {kind} err / sum|a||b|", errs[False], float("inf"))
    assert within(f"conv_mfma {geom} {c}->{c} weights {kind} err / sum|a||b| (bar: the replaced path's x 2, floor 2e-6)",
                  errs[True], max(2e-6, 2 * errs[False]))


@pytest.mark.parametrize("geom,ci,co", [("same", 80, 40), ("same", 20, 20), ("transposed_s2", 40, 40), ("stride2", 40, 40)])
def test_conv_mfma_is_deterministic(geom, ci, co):
    """forward and data gradient are this one kernel under the geometries above: a second run is bitwise the first"""
    dev = _dev()
    from unidefense_amd import kernels as Kk
    n, ho, wo = 2, 12, 20
    gen = torch.Generator().manual_seed(7)
    hi, wi = _in_hw(geom, ho, wo)
    x = torch.randn(n, ci, hi, wi, generator=gen)
    w = torch.randn(*_w_shape(geom, ci, co), generator=gen)
    _, gm, wmat = _problem(Kk, geom, n, ho, wo, ci, co, x, w)
    xp, wm = to_pix(x).to(dev), wmat.contiguous().to(dev)
    with _Route(Kk, True):
        a = Kk.conv_gather_nt(xp, wm, gm).clone()
        b = Kk.conv_gather_nt(xp, wm, gm)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_decoder_block_same_with_the_new_path_on_and_off():
    dev = _dev()
    from unidefense_amd import kernels as Kk
    from unidefense_amd import tape as T
    from tests.margins import within
    from tests.test_a_kernels_gpu import run_tape
    gen = torch.Generator().manual_seed(11)
    n, h = 2, 16
    x = to_pix(torch.randn(n, 80, h, h, generator=gen)).to(dev)
    w1 = (torch.randn(40, 80, 3, 3, generator=gen) * 0.05).to(dev)
    w2 = (torch.randn(40, 40, 3, 3, generator=gen) * 0.07).to(dev)
    w3 = (torch.randn(40, 40, 3, 3, generator=gen) * 0.07).to(dev)
    gy = to_pix(torch.randn(n, 40, 2 * h, 2 * h, generator=gen)).to(dev)

    def block(tape, a, p1, p2, p3):
        a = T.instancenorm_act(tape, T.conv_dense(tape, a, p1, 1, 1, 1, h, h), None, None, 1e-5, 1)
        a = T.instancenorm_act(tape, T.conv_transpose_s2(tape, a, p2), None, None, 1e-5, 1)
        return T.instancenorm_act(tape, T.conv_dense(tape, a, p3, 1, 1, 1, 2 * h, 2 * h), None, None, 1e-5, 1)

    # every conv of the block, forward and data gradient, is a shape the new path takes when it is on
    geoms = [(Kk.conv_geom(n, h, h, 80, h, h, 3, 3, 1, 1, 1, 0), 40), (Kk.conv_geom(n, h, h, 40, h, h, 3, 3, 1, 1, 1, 0), 80),
             (Kk.conv_geom(n, h, h, 40, 2 * h, 2 * h, 3, 3, 2, 1, 1, 1), 40), (Kk.conv_geom(n, 2 * h, 2 * h, 40, h, h, 3, 3, 2, 1, 1, 0), 40),
             (Kk.conv_geom(n, 2 * h, 2 * h, 40, 2 * h, 2 * h, 3, 3, 1, 1, 1, 0), 40)]
    res = {}
    for on in (False, True):
        with _Route(Kk, on):
            assert all(Kk._conv_mfma_takes(gm, co, gm.N * gm.Hout * gm.Wout, x) for gm, co in geoms) == on
            # the three weight gradients: dy x gathered x of the two convs, x x gathered dy (stride 2) of the transposed conv
            assert all(Kk._conv_mfma_wgrad_takes(gm, ma, gm.N * gm.Hout * gm.Wout, x)
                       for gm, ma in ((geoms[0][0], 40), (geoms[3][0], 40), (geoms[4][0], 40))) == on
            outs, gin, gp = run_tape(block, [x], [w1, w2, w3], lambda o: [gy])
        torch.cuda.synchronize()
        res[on] = [outs[0], gin[0]] + list(gp)
    assert not torch.equal(res[True][0], res[False][0])          # two different kernels computed y: not bitwise the same
    for name, a, b in zip(("y", "dx", "dw1", "dw2", "dw3"), res[True], res[False]):
        assert a is not None and b is not None and a.shape == b.shape
        e = ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()
        print(f"  decoder block {name}: new path vs old path rel {e:.3e}")
        assert within(f"decoder block {name}: conv_mfma on vs off", e, 1e-5)

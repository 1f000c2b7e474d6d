"""ud_param_fold_multi: the launches of a backward that only finish a parameter's gradient, collected by a tape's backward
(kernels.begin_wgrad_folds ... flush_wgrad_folds) and run as items of one launch.  The collected form keeps each kind's order of
summation, so every comparison with the immediate form here is torch.equal, not a tolerance."""
import pytest
import torch

from oracle import param_fill
from tests import oracle_util as ou

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _both(run):
    """run() once folding at once and once between begin and flush; returns (immediate, collected, number of items)"""
    from unidefense_amd import kernels as K
    from unidefense_amd.config import override
    with override(deterministic=True):
        K.reset_zero_pool()
        assert K._WGRAD_FOLDS is None
        ref = run()
        K.reset_zero_pool()
        K.begin_wgrad_folds()
        try:
            got = run()
            n = len(K._WGRAD_FOLDS)
            assert all(getattr(t, "_ud_deferred", False) for t in got) or n == 0
        finally:
            K.flush_wgrad_folds(end=True)
    torch.cuda.synchronize()
    assert K._WGRAD_FOLDS is None and not any(getattr(t, "_ud_deferred", False) for t in got)
    return ref, got, n


def _equal(ref, got):
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape and torch.equal(a, b), (i, tuple(a.shape), float((a - b).abs().max()))


def _expand_problem(K, dev, M, Ce, Cin, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Cin, generator=g).to(dev)
    w = (torch.randn(Ce, Cin, generator=g) / Cin ** 0.5).to(dev)
    e = (x @ w.t()).contiguous()
    dz = torch.randn(M, Ce, generator=g).to(dev)
    gamma, beta = (1.0 + 0.3 * torch.randn(Ce, generator=g)).to(dev), (0.2 * torch.randn(Ce, generator=g)).to(dev)

    def run():
        acc = K.zeros64(2 * Ce, x)
        K.colstats(e, acc)
        bn = K.DeferredBN(acc, Ce, M, gamma, beta, 1e-3, 1)
        sb = K.zeros64(2 * Ce, x)
        K.normbwd_sums(e.view(1, M, Ce), dz.view(1, M, Ce), None, 1.0, bn, True, 1, M, sb)
        return list(K.expand_bwd_fused(e, dz, bn, sb, None, x, w)[1:])          # dw, dgamma, dbeta
    return run


@pytest.mark.parametrize("Ce,Cin", [(144, 24), (192, 32)])
@pytest.mark.parametrize("M", [32, 64, 33 * 32])
def test_expand_conv_fold_collected_equals_immediate(M, Ce, Cin):
    """ud_pw_bwd_fused's partials + the dgamma / dbeta copies: one partial, two, and 33 (past the fold's 32-stride: its tail)"""
    from unidefense_amd import kernels as K
    dev = _dev()
    assert K._call("ud_pw_bwd_fused_grid", M) == M // 32
    ref, got, n = _both(_expand_problem(K, dev, M, Ce, Cin, M + Ce))
    assert n == 1
    _equal(ref, got)


@pytest.mark.parametrize("Ce,Co,se", [(144, 32, True), (192, 32, False), (336, 56, True), (192, 56, True)])
def test_project_conv_fold_collected_equals_immediate(Ce, Co, se):
    """ud_pj_bwd_fused_a / _a_se's column-chunked partials (336 / 192 columns in front of 56: chunks of 112 / 96), M = 64"""
    from unidefense_amd import kernels as K
    dev = _dev()
    N, HW = 2, 32
    g = torch.Generator().manual_seed(Ce + Co)
    d = (torch.randn(N, HW, Ce, generator=g) * 1.3 + 0.2).to(dev)
    w = (torch.randn(Co, Ce, generator=g) / Ce ** 0.5).to(dev)
    dp = torch.randn(N * HW, Co, generator=g).to(dev)
    s = torch.randn(N, Ce, generator=g).to(dev)
    gamma, beta = (1.0 + 0.3 * torch.randn(Ce, generator=g)).to(dev), (0.2 * torch.randn(Ce, generator=g)).to(dev)
    assert K._call("ud_pj_bwd_fused_ok", Ce, Co, HW) == 1

    def run():
        acc = K.zeros64(2 * Ce, d)
        K.colstats(d.view(-1, Ce), acc)
        bn = K.DeferredBN(acc, Ce, N * HW, gamma, beta, 1e-3, 1)
        if se:
            return [K.project_bwd_fused_a_se(d, bn, s, dp, w, N, HW, K.zeros64(5 * N * Ce, d))]
        return [K.project_bwd_fused_a(d, bn, s, dp, w, N, HW, K.zeros64(N * Ce, d))]
    ref, got, n = _both(run)
    assert n == 1
    _equal(ref, got)


class _SmallRoute:
    """conv weight gradients on csrc/conv_small.hip at any row count (and not on the MFMA kernel)"""

    def __enter__(self):
        from unidefense_amd import kernels as K
        self.saved = K._CONV_SMALL, K._CONV_SMALL_MIN_M, K._CONV_MFMA
        K._CONV_SMALL, K._CONV_SMALL_MIN_M, K._CONV_MFMA = True, 1, False

    def __exit__(self, *exc):
        from unidefense_amd import kernels as K
        K._CONV_SMALL, K._CONV_SMALL_MIN_M, K._CONV_MFMA = self.saved


def _param_layout(dw, g):
    return dw.view(dw.shape[0], g.KH, g.KW, g.Cin).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("ci,ma", [(20, 20), (20, 3), (3, 48)])
@pytest.mark.parametrize("n,h,w_", [(1, 3, 3), (2, 72, 64)])
def test_conv_small_wgrad_fold_collected_equals_immediate(ci, ma, n, h, w_):
    """ud_conv_small_wgrad's fp64 fold: one partial block (N = 1, a 3 x 3 map) and several (9216 rows: more than one block of
    rows), as the [Ma, 9 Cin] matrix and folded straight into the parameter's layout"""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(ci * 100 + ma + h)
    x = torch.randn(n, h, w_, ci, generator=gen).to(dev)
    a = torch.randn(n * h * w_, ma, generator=gen).to(dev)
    gm = K.conv_geom(n, h, w_, ci, h, w_, 3, 3, 1, 1, 1, 0)
    with _SmallRoute():
        ref, got, items = _both(lambda: [K.conv_gather_wgrad(a, x, gm), K.conv_wgrad_param(a, x, gm)])
    assert items == 2
    _equal(ref, got)
    assert torch.equal(got[1], _param_layout(got[0], gm))


class _MfmaRoute:
    """conv weight gradients on csrc/conv_mfma.hip for every instantiated shape, at any row count"""

    def __enter__(self):
        from unidefense_amd import kernels as K
        self.saved = K._CONV_MFMA, K._CONV_MFMA_MIN_M, K._CONV_MFMA_WGRAD_SHAPES
        K._CONV_MFMA, K._CONV_MFMA_MIN_M, K._CONV_MFMA_WGRAD_SHAPES = True, 1, None

    def __exit__(self, *exc):
        from unidefense_amd import kernels as K
        K._CONV_MFMA, K._CONV_MFMA_MIN_M, K._CONV_MFMA_WGRAD_SHAPES = self.saved


@pytest.mark.parametrize("ci,ma,n,h,w_", [(20, 20, 1, 5, 7), (40, 20, 2, 64, 64)])
def test_conv_mfma_wgrad_fold_collected_equals_immediate(ci, ma, n, h, w_):
    """ud_conv_mfma_wgrad's fp32 fold (the expand convs' order, no dgamma / dbeta): one partial (a 5 x 7 map) and several (2 x 64 x 64 pixels), as
    the matrix and folded straight into the parameter's layout"""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(ci + ma + h)
    x = torch.randn(n, h, w_, ci, generator=gen).to(dev)
    a = torch.randn(n * h * w_, ma, generator=gen).to(dev)
    gm = K.conv_geom(n, h, w_, ci, h, w_, 3, 3, 1, 1, 1, 0)
    with _MfmaRoute():
        assert K._conv_mfma_wgrad_takes(gm, ma, n * h * w_, a, x)
        ref, got, items = _both(lambda: [K.conv_gather_wgrad(a, x, gm), K.conv_wgrad_param(a, x, gm)])
    assert items == 2
    _equal(ref, got)
    assert torch.equal(got[1], _param_layout(got[0], gm))


@pytest.mark.parametrize("G,C,R", [(1, 20, 50), (3, 20, 50), (3, 36, 50), (5, 300, 50)])
def test_group_sum_collected_equals_immediate(G, C, R):
    """InstanceNorm's dgamma / dbeta over the G samples: G = 1 has no group sum (no item), channel counts that are no multiple of
    the workgroup's 256 (and more than one workgroup)"""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(G * 1000 + C)
    x = torch.randn(G * R, C, generator=gen).to(dev)
    dy = torch.randn(G * R, C, generator=gen).to(dev)
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=gen)).to(dev), (0.2 * torch.randn(C, generator=gen)).to(dev)
    mean, invstd = K.norm_stats(x, G, R, 1e-5)
    ref, got, items = _both(lambda: list(K.norm_bwd(x, dy, G, R, mean, invstd, gamma, beta, 1)[1:]))
    assert items == (1 if G > 1 else 0)
    _equal(ref, got)


@pytest.mark.parametrize("transposed,ci,co", [(False, 24, 40), (True, 40, 24), (True, 8, 12)])
def test_layout_item_equals_the_permuting_copy(transposed, ci, co):
    """a GEMM's conv weight gradient [A, 9 B] copied into the parameter's [A, B, 3, 3] by a layout item: F.conv2d (A = Cout, B = Cin)
    and ConvTranspose2d (A = Cin, B = Cout, the gradient gathered at stride 2), Cin != Cout"""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(ci + co)
    n, h, w_ = 2, 6, 10
    if transposed:          # the layer maps ci -> co channels on an h x w input
        a = torch.randn(n * h * w_, ci, generator=gen).to(dev)
        x = torch.randn(n, 2 * h, 2 * w_, co, generator=gen).to(dev)
        gm = K.conv_geom(n, 2 * h, 2 * w_, co, h, w_, 3, 3, 2, 1, 1, 0)
    else:
        a = torch.randn(n * h * w_, co, generator=gen).to(dev)
        x = torch.randn(n, h, w_, ci, generator=gen).to(dev)
        gm = K.conv_geom(n, h, w_, ci, h, w_, 3, 3, 1, 1, 1, 0)
    assert not K._conv_mfma_wgrad_takes(gm, a.shape[-1], n * h * w_, a, x)
    ref, got, items = _both(lambda: [K.conv_wgrad_param(a, x, gm)])
    assert items == 1 and K.FOLD_KINDS["layout"] == 5
    assert got[0].shape == (a.shape[-1], gm.Cin, 3, 3)
    _equal(ref, got)


def test_one_flush_of_more_items_than_one_launch_takes_mixed_kinds():
    """91 tiny items of four kinds in one flush: three launches of at most 44 items, every workgroup finding its item through
    the block prefix"""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    expand = _expand_problem(K, dev, 64, 144, 24, 3)
    xs = [torch.randn(3 * 10, 8 + 4 * (i % 3), generator=gen).to(dev) for i in range(12)]
    stats = [K.norm_stats(x, 3, 10, 1e-5) for x in xs]
    xd = torch.randn(2, 8, 8, 8, generator=gen).to(dev)
    gmx = torch.randn(2, 5, 5, 8, generator=gen).to(dev)
    gma = torch.randn(50, 12, generator=gen).to(dev)
    gm = K.conv_geom(2, 5, 5, 8, 5, 5, 3, 3, 1, 1, 1, 0)

    def run():
        out = []
        for r in range(13):
            for x, (mean, invstd) in zip(xs[r % 3::3], stats[r % 3::3]):
                ones = torch.ones(x.shape[1], device=dev)
                out += K.norm_bwd(x, x, 3, 10, mean, invstd, ones, ones, 0)[1:]
            out += expand()
            out.append(K.dwtile_bwd_weight(xd, xd, 3, 1, 1))
            out.append(K.conv_wgrad_param(gma, gmx, gm))
        return out
    ref, got, items = _both(run)
    assert items == 13 * (4 + 1 + 1 + 1) and items > 2 * 44
    _equal(ref, got)


# ---- the flush rules, on a tape --------------------------------------------------------------------------------------------------
def _tape_problem(dev):
    from unidefense_amd import kernels as K
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(3 * 40, 20, generator=gen).to(dev)
    dy = torch.randn(3 * 40, 20, generator=gen).to(dev)
    ga, be = torch.ones(20, device=dev), torch.zeros(20, device=dev)
    mean, invstd = K.norm_stats(x, 3, 40, 1e-5)
    return lambda: K.norm_bwd(x, dy, 3, 40, mean, invstd, ga, be, 0)[1:], ga, be


def _run_tape(build):
    """param_grads of a tape built by build(tape), backward folding at once and collecting"""
    from unidefense_amd import kernels as K
    from unidefense_amd.tape import Tape
    res = []
    for immediate in (True, False):
        tape = Tape()
        build(tape)
        if immediate:
            with K.immediate_folds():
                tape.backward()
        else:
            tape.backward()
        torch.cuda.synchronize()
        assert K._WGRAD_FOLDS is None
        res.append({k: v.clone() for k, v in tape.param_grads.items()})
    return res


def test_two_contributions_to_one_parameter_equal_the_immediate_result():
    dev = _dev()
    grads, ga, be = _tape_problem(dev)

    def build(tape):
        for _ in range(2):
            def node():
                dg, db = grads()
                tape.add_param_grad(ga, dg)
                tape.add_param_grad(be, db)
            tape.record(node)
    ref, got = _run_tape(build)
    assert set(ref) == set(got) == {ga, be}
    for p in ref:
        assert torch.equal(ref[p], got[p]) and float(ref[p].abs().max()) > 0


def test_a_backward_inside_a_node_equals_the_immediate_result():
    from unidefense_amd.tape import Tape
    dev = _dev()
    grads, ga, be = _tape_problem(dev)
    ga2 = torch.ones(20, device=dev)
    inner_grads = []

    def build(tape):
        def last():          # runs after the nested backward: the outer tape no longer collects, its gradient is folded at once
            tape.add_param_grad(be, grads()[1])

        def node():
            tape.add_param_grad(ga, grads()[0])          # pending when the inner backward starts: folded there, not dropped
            inner = Tape()
            inner.record(lambda: inner.add_param_grad(ga2, grads()[0]))
            inner.backward()
            inner_grads.append(inner.param_grads[ga2].clone())
        tape.record(last)
        tape.record(node)
    ref, got = _run_tape(build)
    for p in (ga, be):
        assert torch.equal(ref[p], got[p])
    assert torch.equal(inner_grads[0], inner_grads[1]) and torch.equal(inner_grads[1], got[ga])


def test_the_param_ready_hook_sees_the_folded_gradient():
    from unidefense_amd.tape import Tape
    dev = _dev()
    grads, ga, be = _tape_problem(dev)
    want = [t.clone() for t in grads()]
    seen = {}
    tape = Tape()
    tape.param_uses = {id(ga): 1, id(be): 1}
    tape.param_ready = lambda pid, g: seen.__setitem__(pid, g.clone())          # (the copy is ordered after the fold on the stream)

    def node():
        dg, db = grads()
        tape.add_param_grad(ga, dg)
        tape.add_param_grad(be, db)
    tape.record(node)
    tape.backward()
    torch.cuda.synchronize()
    assert torch.equal(seen[id(ga)], want[0]) and torch.equal(seen[id(be)], want[1])


# ---- the whole model -------------------------------------------------------------------------------------------------------------
def test_udeb4_parameter_gradients_collected_equal_immediate():
    """UDEB4, N = 2 at 256 x 256, one training forward + backward with every fold at once and one with the folds collected: all
    parameter gradients bit for bit"""
    from unidefense_amd import kernels as K
    from unidefense_amd.config import override
    from unidefense_amd.loss import LOSSES
    from unidefense_amd.model import load_model
    dev = _dev()
    n = 2
    m = load_model("UDEB4")(extractor="efficientnet-b4", num_classes=2, drop_rate=0.5)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    m = m.to(dev).train()
    x = param_fill.make_input(n, 256, seed=11).to(dev)
    tgt = param_fill.make_labels(n).to(dev)
    lam = ou.LAMBDAS

    def step(immediate):
        for p in m.parameters():
            p.grad = None
        out = m(x, rng=ou.make_rng(n, 12, 0.5))
        ld = out["loss_dict"]
        trip = sum(LOSSES["aw_triplet"](f, tgt) for f in ld["triplet"])
        total = LOSSES["cross_entropy"](out["cls_out"], tgt) + lam["lambda_mask"] * (ld["freq_mask"].mean() + ld["spat_mask"].mean()) \
            + lam["lambda_triplet"] * trip + lam["lambda_recons"] * ld["spatial"][: n // 2].mean() \
            + lam["lambda_freq"] * ld["freq"][: n // 2].mean()
        if immediate:
            with K.immediate_folds():
                total.backward()
        else:
            total.backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    with override(deterministic=True):
        ref = step(True)
        got = step(False)
    assert set(ref) == set(got) and len(ref) > 400
    bad = [k for k in ref if not torch.equal(ref[k], got[k])]
    assert not bad, (len(bad), bad[:8])

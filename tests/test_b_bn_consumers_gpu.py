"""GPU, operator level: the BatchNorm-on-load consumers of csrc/fused.hip at the row counts where their grouped row loops
(for_rows: kRowGroup = 4 rows loaded back to back, then computed; a row-by-row tail) and their two-part prologue (bn_issue /
bn_finish, the running statistics moved behind the loop) change path.  Every entry point against torch in float64, with the
tolerances tests/test_b_fused_kernels_gpu.py uses for the same kernel.

The row count R of a case is chosen from the kernels' own decomposition (csrc/colgeom.h make_geom_ex, restated below) so that a
thread walks exactly n rows: n = 1 (R = 1: every other row lane has none), 3, 4, 5 and 11 = group - 1, group, group + 1 and
2 group + 3 — for the element-wise geometry (geom_ew) or for the reducing one (plan_reduce), whichever the test is about.
C = 8 / 36 / 144: one column group, an uneven split (C4 = 9), several quads per row lane; G = 1 / 3."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-3
NT = 256


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b, zero_scale=1e-30):
    """max |a - b| / max |b|.  zero_scale: what the error is relative to where the reference is identically zero — a BatchNorm
    backward over a batch of ONE row is 0 = dz - mean(dz), and an fp32 kernel's error is relative to the terms it cancels"""
    a, b = a.detach().double(), b.detach().double().to(a.device)
    top = float(b.abs().max())
    return float((a - b).abs().max() / (top if top > 0.0 else zero_scale))


# ---- csrc/colgeom.h make_geom_ex, csrc/fused.hip plan_reduce / geom_ew: (rows per iteration, chunks, rows per chunk) ----
def _geom(G, R, C, target, max_p, min_rows, cw_limit=16):
    C4 = C // 4
    ngroups = -(-C4 // cw_limit)
    CW = -(-C4 // ngroups)
    rpi = NT // CW
    cgroups = -(-C4 // CW)
    want = max(1, target // (G * cgroups))
    maxp = max(1, -(-R // (rpi * min_rows)))
    P = min(want, maxp, max_p)
    return rpi, P, -(-R // P)


def _geom_ew(G, R, C):
    return _geom(G, R, C, 2048, 4096, 4, 128)


def _geom_mix(G, R, C):          # ud_normbwd_apply_mix: one fp64 atomic per workgroup
    return _geom(G, R, C, 512, 4096, 4)


def _geom_dot_eval(G, R, C):          # coldot_eval_geom
    return _geom(G, R, C, 1024, 64, 8)


def test_the_restated_geometry_is_the_sources():
    """the constants restated above, as the sources spell them"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unidefense_amd", "csrc")
    fused, colgeom = open(os.path.join(csrc, "fused.hip")).read(), open(os.path.join(csrc, "colgeom.h")).read()
    for text in ("geom_ew(int G, int R, int C, int min_rows = 4) { return make_geom_ex(G, R, C, 2048, 4096, min_rows, 128); }",
                 "RedGeom q = make_geom_ex(G, R, C, 512, 4096, 4);", "return make_geom_ex(G, R, C, 1024, 64, 8); }",
                 "constexpr int lim = 64;", "constexpr long big_elems = 1L << 20;", "make_geom_ex(G, R, C, 1024, lim, min_rows);",
                 "RedPlan{make_geom_ex(G, R, C, 2048, 512, min_rows), true}", "int min_rows = 8,"):
        assert text in fused, text
    for text in ("constexpr int UD_COL_NT = 256;", "int min_rows = 8, int cw_limit = 16)"):
        assert text in colgeom, text


def _geom_red(G, R, C, per_group):
    rpi, P, rpc = _geom(G, R, C, 1024, 64, 8)
    contrib = P if per_group else G * P
    big = (not per_group) and G * R * (C // 4) >= (1 << 20)
    if contrib <= 64 and not big:
        return rpi, P, rpc
    return _geom(G, R, C, 2048, 512, 8)


@functools.lru_cache(maxsize=None)
def _rows_for(n, kind, G, C):
    """smallest ragged R (a last row group that does not fill the row lanes, where one exists) at which a thread of the `kind`
    geometry ('ew', 'red' = one accumulator set, 'redg' = per group, 'mix' = ud_normbwd_apply_mix, 'dote' = ud_coldot_bn_eval) walks n rows at the most, and some thread exactly n"""
    geom = {"ew": _geom_ew, "red": lambda g, r, c: _geom_red(g, r, c, False), "redg": lambda g, r, c: _geom_red(g, r, c, True),
            "mix": _geom_mix, "dote": _geom_dot_eval}[kind]
    if n == 1:
        return 1
    for pc in range(1, 4097):
        for R in (n * geom(G, 1, C)[0] * pc - 1, n * geom(G, 1, C)[0] * pc):
            rpi, P, rpc = geom(G, R, C)
            if -(-min(rpc, R) // rpi) == n:
                return R
    raise AssertionError((n, kind, G, C))


GC = [(1, 8), (3, 8), (1, 36), (3, 36), (1, 144), (3, 144)]
NROWS = [1, 3, 4, 5, 11]
DT = [torch.float32, torch.float16]
IDS = ["fp32", "half"]


def _inputs(G, R, C, dt, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = (torch.randn(G, R, C, generator=g, device=dev) * 1.7 + 0.3).to(dt)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g, device=dev)
    beta = 0.1 * torch.randn(C, generator=g, device=dev)
    # ReLU's gradient is a step at z = 0: keep every z = bn(x) away from it, so that the fp32 kernel and the float64 formula
    # stand on the same side (moving x moves the moments: a few rounds; best effort where the batch is a single row)
    for _ in range(5):
        z = _ref_fwd(x, gamma, beta, 0)[1]
        near = z.abs() < 1e-3
        if not bool(near.any()):
            break
        x = torch.where(near, x.float() + 0.05, x.float()).to(dt)
    return g, x, gamma, beta


def _bn(K, x, gamma, beta, act, rm=None, rv=None, mom=0.0):
    G, R, C = x.shape
    acc = K.zeros64(2 * C, x)
    K.colstats(x.view(G * R, C), acc)
    return K.DeferredBN(acc, C, G * R, gamma, beta, EPS, act, mom, rm, rv)


def _moments(x):
    xd = x.double()
    n = xd.shape[0] * xd.shape[1]
    mean = xd.sum((0, 1)) / n
    var = ((xd * xd).sum((0, 1)) / n - mean * mean).clamp_min(0.0)
    return xd, mean, var


def _act(z, act):
    return z * torch.sigmoid(z) if act == 1 else z.clamp_min(0.0) if act == 2 else z


def _act_grad(z, act):
    if act == 1:
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    return (z > 0).double() if act == 2 else torch.ones_like(z)


def _ref_fwd(x, gamma, beta, act, mean=None, var=None):
    xd, m, v = _moments(x)
    mean, var = (m, v) if mean is None else (mean.double(), var.double())
    xh = (xd - mean) / torch.sqrt(var + EPS)
    z = xh * gamma.double() + beta.double()
    return _act(z, act), z, xh


def _tol(dt, fp32):
    """the bars of tests/test_b_fused_kernels_gpu.py: fp32 as given there per kernel; half storage 2e-3 (sums: 3e-3)"""
    return fp32 if dt == torch.float32 else 2e-3


def _unpack(pl, R, C):
    """[planes][R][padded C] fp16 of a Planes over R rows (P32 layout)"""
    return pl.buf.view(-1, pl.npanel, pl.panel // 32, 32)[:, :, :R].view(torch.float16).permute(0, 2, 1, 3).reshape(-1, R, pl.npanel * 32)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("G,C", GC)
def test_elementwise_forward_consumers(G, C, n, dt):
    """bn_apply, se_scale_bn, residual_bn (keep / skip given and NULL) for act 0, 1, 2 at n rows per thread of geom_ew; the
    updater moves the running statistics exactly once (the momentum formula from the sums), a later consumer leaves them alone"""
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    R = _rows_for(n, "ew", G, C)
    g, x, gamma, beta = _inputs(G, R, C, dt, 7 * n + C + G, dev)
    s = torch.randn(G, C, generator=g, device=dev)
    keep = torch.tensor([1.0, 0.0, 1.0][:G], device=dev)
    skip = torch.randn(G, R, C, generator=g, device=dev).to(dt)
    tol = _tol(dt, 5e-6)
    xd, mean, var = _moments(x)
    cnt = G * R
    for act in (0, 1, 2):
        ref, _, _ = _ref_fwd(x, gamma, beta, act)
        rm, rv = torch.full((C,), 0.25, device=dev), torch.full((C,), 2.0, device=dev)
        bn = _bn(K, x, gamma, beta, act, rm, rv, 0.1)
        y = K.bn_apply(x, bn, G, R, update=True)
        assert y.dtype == dt and _rel(y, ref) < tol
        rm1, rv1 = rm.clone(), rv.clone()
        assert _rel(rm1, 0.9 * 0.25 + 0.1 * mean) < 1e-5
        assert _rel(rv1, 0.9 * 2.0 + 0.1 * var * cnt / max(cnt - 1, 1)) < 1e-5
        yg = K.se_scale_bn(x, bn, s, G, R, want_absmax=(dt == torch.float32))
        assert _rel(yg, ref * torch.sigmoid(s.double())[:, None, :]) < tol
        if dt == torch.float32:
            assert float(yg._ud_absmax.view(torch.float32).max()) == float(yg.abs().max())
        for kp, sk in ((keep, skip), (None, skip), (keep, None), (None, None)):
            out = K.residual_bn(x, bn, kp, 1.25, sk, G, R, update=True)          # (update: already handed out — must not move them)
            want = ref * ((kp.double() * 1.25)[:, None, None] if kp is not None else 1.0) + (sk.double() if sk is not None else 0.0)
            assert _rel(out, want) < tol
        assert torch.equal(rm, rm1) and torch.equal(rv, rv1)
        # residual_bn as the BatchNorm's FIRST consumer
        rm2, rv2 = torch.full((C,), 0.25, device=dev), torch.full((C,), 2.0, device=dev)
        bn2 = _bn(K, x, gamma, beta, act, rm2, rv2, 0.1)
        K.residual_bn(x, bn2, keep, 1.25, skip, G, R, update=True)
        assert torch.equal(rm2, rm1) and torch.equal(rv2, rv1)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("G,C", GC)
def test_reducing_forward_consumers(G, C, n, dt):
    """colsum_bn (the updater among the reductions), coldot_bn for act 0, 1, 2 at n rows per thread of the per-group reduction"""
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    R = _rows_for(n, "redg", G, C)
    g, x, gamma, beta = _inputs(G, R, C, dt, 11 * n + C + G, dev)
    dy = torch.randn(G, R, C, generator=g, device=dev).to(dt)
    tol = _tol(dt, 5e-6)
    xd, mean, var = _moments(x)
    cnt = G * R
    for act in (0, 1, 2):
        ref, _, _ = _ref_fwd(x, gamma, beta, act)
        rm, rv = torch.full((C,), -0.5, device=dev), torch.full((C,), 0.5, device=dev)
        bn = _bn(K, x, gamma, beta, act, rm, rv, 0.01)
        pool = K.zeros64(G * C, x)
        K.colsum_bn(x, bn, G, R, pool, update=True)
        assert _rel(pool.view(G, C), ref.sum(1)) < tol
        assert _rel(rm, 0.99 * -0.5 + 0.01 * mean) < 1e-5
        assert _rel(rv, 0.99 * 0.5 + 0.01 * var * cnt / max(cnt - 1, 1)) < 1e-5
        rm1, rv1 = rm.clone(), rv.clone()
        dot = K.zeros64(G * C, x)
        K.coldot_bn(dy, x, bn, G, R, dot)
        assert _rel(dot.view(G, C), (dy.double() * ref).sum(1)) < tol
        K.colsum_bn(x, bn, G, R, K.zeros64(G * C, x), update=True)          # handed out already: no second move
        assert torch.equal(rm, rm1) and torch.equal(rv, rv1)
        if dt == torch.float32:
            pool2 = K.zeros64(G * C, x)
            amax = K.colsum_bn_amax(x, bn, G, R, pool2)
            assert _rel(pool2, pool) < 1e-12          # (fp64 atomics: the order of the adds is not fixed)
            assert float(amax.view(torch.float32).max()) == float(K.bn_apply(x, bn, G, R).abs().max())


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("kind", ["ew", "red", "mix"])
@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("G,C", GC)
def test_backward_consumers(G, C, n, kind, dt):
    """normbwd_sums (with / without the energy sum) -> normbwd_apply (fp32 tensor / GEMM planes), dy_is_dz 0 and 1, keep given
    and NULL, act 0, 1, 2; se_scale_bwd_bn; normbwd_apply_mix — at n rows per thread of the apply (ew), of the sums (red) or of
    the SF-mix apply (mix)"""
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    R = _rows_for(n, kind, G, C)
    g, x, gamma, beta = _inputs(G, R, C, dt, 13 * n + C + G, dev)
    dy = torch.randn(G, R, C, generator=g, device=dev).to(dt)
    keep = torch.tensor([1.0, 0.0, 1.0][:G], device=dev)
    tol, stol = _tol(dt, 2e-5), (2e-5 if dt == torch.float32 else 3e-3)
    cnt = G * R

    def bn_bwd(dz, xh):          # dx of a training BatchNorm from dz (float64), and the size of the terms it is a difference of
        s1, s2 = dz.sum((0, 1)), (dz * xh).sum((0, 1))
        k = gamma.double() / torch.sqrt(_moments(x)[2] + EPS)
        return k * (dz - s1 / cnt - xh * s2 / cnt), s1, s2, float((k * dz).abs().max())

    for act in (0, 1, 2):
        _, z, xh = _ref_fwd(x, gamma, beta, act)
        bn = _bn(K, x, gamma, beta, act)
        for kp in (keep, None):
            for is_dz in (False, True):
                dzr = dy.double() if is_dz else dy.double() * ((kp.double() * 1.25)[:, None, None] if kp is not None else 1.0) * _act_grad(z, act)
                dxr, s1, s2, terms = bn_bwd(dzr, xh)
                sacc, sacc3 = K.zeros64(2 * C, x), K.zeros64(3 * C, x)
                K.normbwd_sums(x, dy, kp, 1.25, bn, is_dz, G, R, sacc)
                K.normbwd_sums(x, dy, kp, 1.25, bn, is_dz, G, R, sacc3)
                for sa in (sacc, sacc3):
                    assert _rel(sa[:C], s1) < stol and _rel(sa[C:2 * C], s2) < stol
                en = dzr.pow(2).sum((0, 1))
                ok = en > 0
                assert bool((sacc3[2 * C:][~ok] == 0).all())
                if bool(ok.any()):
                    ratio = sacc3[2 * C:][ok] / en[ok]
                    assert float(ratio.min()) >= 1.0 - 1e-6 and float(ratio.max()) < 1.001
                dx, dg, db = K.normbwd_apply(x, dy, kp, 1.25, bn, is_dz, G, R, sacc, want_absmax=(dt == torch.float32))
                assert dx.dtype == dt and _rel(dx, dxr, terms) < tol
                assert _rel(db, s1) < stol and _rel(dg, s2) < stol
                if dt == torch.float32:
                    assert float(dx._ud_absmax.view(torch.float32).max()) == float(dx.abs().max())
                if dt == torch.float32 or C % 8 == 0:          # the planes destination (half: whole 8-channel runs)
                    pl, dg2, db2 = K.normbwd_apply_planes(x, dy, kp, 1.25, bn, is_dz, G, R, sacc3)
                    assert torch.equal(dg2, dg) and torch.equal(db2, db)
                    full = _unpack(pl, G * R, C)
                    assert float(full[:, :, C:].abs().max() if pl.npanel * 32 > C else 0.0) == 0.0
                    if dt == torch.float16:
                        # the same values as the row-major result (another instance of the kernel: to a half ulp)
                        assert float(pl.inv) == 1.0 and _rel(full[0, :, :C], dx.view(G * R, C), terms) < tol
                    else:
                        h, inv, yd = full[:, :, :C].double(), float(pl.inv), dx.view(G * R, C).double()
                        top = float(yd.abs().max())
                        if top > 0:
                            loose = 2.0 ** 15 / (top / inv)
                            assert loose >= 1.0
                            assert float(((h[0] + h[1] / 2048.0) * inv - yd).abs().max()) <= 2.0 ** -21 * top * loose
        # the SE gate's backward in front of the BatchNorm, and its apply
        s = torch.randn(G, C, generator=g, device=dev)
        dpool = torch.randn(G, C, generator=g, device=dev)
        dzr = (dy.double() * torch.sigmoid(s.double())[:, None, :] + dpool.double()[:, None, :] / R) * _act_grad(z, act)
        sacc = K.zeros64(2 * C, x)
        dz = K.se_scale_bwd_bn(dy, x, bn, s, dpool, 1.0 / R, G, R, sacc)
        assert dz.dtype == dt and _rel(dz, dzr) < tol
        dzs = dz.double()          # the sums are those of the STORED gradient
        assert _rel(sacc[:C], dzs.sum((0, 1))) < stol and _rel(sacc[C:], (dzs * xh).sum((0, 1))) < stol
        # the SF-mix apply: dd, the gate's dot and the energy of dd
        diff = torch.randn(G, R, C, generator=g, device=dev).to(dt)
        ddr, s1, s2, terms = bn_bwd(dzs, xh)
        for want_energy in (False, True):
            dacc = K.zeros64(64, x)
            energy = K.zeros64(C, x) if want_energy else None
            dd, dg, db = K.normbwd_apply_mix(x, dz, bn, G, R, sacc, diff, dacc, energy=energy)
            assert _rel(dd, ddr, terms) < tol
            dot = (dd.double() * diff.double())
            assert abs(float(dacc.sum()) - float(dot.sum())) <= stol * float(dot.abs().sum())
            if want_energy:
                en = dd.double().pow(2).sum((0, 1))
                ok = en > 0
                if bool(ok.any()):          # (a batch of one row: dd = 0)
                    ratio = energy[ok] / en[ok]
                    lo = 1.0 - (1e-6 if dt == torch.float32 else 2e-3)          # (of the unrounded result: half storage rounds dd after)
                    assert float(ratio.min()) >= lo and float(ratio.max()) < 1.001 + (1.0 - lo)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("kind", ["ew", "dote"])
@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("G,C", GC)
def test_eval_form_reads_and_never_writes_the_running_buffers(G, C, n, kind, dt):
    """sum == NULL: the running statistics are the moments, read in place — by the forward consumers and by the frozen
    backward's three kernels — and bit for bit what they were afterwards"""
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    R = _rows_for(n, kind, G, C)          # n rows per thread of the element-wise kernels (ew) or of ud_coldot_bn_eval (dote)
    g, x, gamma, beta = _inputs(G, R, C, dt, 17 * n + C + G, dev)
    mod = torch.nn.BatchNorm2d(C, eps=EPS).to(dev)
    with torch.no_grad():
        mod.weight.copy_(gamma)
        mod.bias.copy_(beta)
        mod.running_mean.copy_(0.3 + 0.2 * torch.randn(C, generator=g, device=dev))
        mod.running_var.copy_(2.0 + torch.rand(C, generator=g, device=dev))
    rm0, rv0 = mod.running_mean.clone(), mod.running_var.clone()
    # (ReLU's step again, now with the running statistics as the moments: they do not move with x)
    x = torch.where(_ref_fwd(x, gamma, beta, 0, rm0, rv0)[1].abs() < 1e-3, x.float() + 0.05, x.float()).to(dt)
    s = torch.randn(G, C, generator=g, device=dev)
    dpool = torch.randn(G, C, generator=g, device=dev)
    dy = torch.randn(G, R, C, generator=g, device=dev).to(dt)
    skip = torch.randn(G, R, C, generator=g, device=dev).to(dt)
    tol = _tol(dt, 5e-6)
    btol = _tol(dt, 2e-5)
    for act in (0, 1, 2):
        bn = K.EvalBN(mod, act)
        ref, z, _ = _ref_fwd(x, gamma, beta, act, rm0, rv0)
        k = gamma.double() / torch.sqrt(rv0.double() + EPS)
        assert _rel(K.bn_apply(x, bn, G, R, update=True), ref) < tol
        assert _rel(K.se_scale_bn(x, bn, s, G, R), ref * torch.sigmoid(s.double())[:, None, :]) < tol
        assert _rel(K.residual_bn(x, bn, None, 1.0, skip, G, R, update=True), ref + skip.double()) < tol
        pool = K.zeros64(G * C, x)
        K.colsum_bn(x, bn, G, R, pool, update=True)
        assert _rel(pool.view(G, C), ref.sum(1)) < tol
        dot = K.zeros64(G * C, x)
        K.coldot_bn_eval(dy, x, bn, G, R, dot)
        assert _rel(dot.view(G, C), (dy.double() * ref).sum(1)) < tol
        dd = K.se_scale_bwd_bn_eval(dy, x, bn, s, dpool, 1.0 / R, G, R)
        want = (dy.double() * torch.sigmoid(s.double())[:, None, :] + dpool.double()[:, None, :] / R) * _act_grad(z, act) * k
        assert _rel(dd, want) < btol
        assert _rel(K.bn_eval_bwd(dy, x, bn, G, R), dy.double() * k * _act_grad(z, act)) < btol
        assert torch.equal(mod.running_mean, rm0) and torch.equal(mod.running_var, rv0)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("C", [8, 36, 144])
def test_per_group_statistics(C, n, dt):
    """ud_bn_ref.G > 1: one set of sums per group ([G][C], an instance norm) — every group normalised by its own moments"""
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    G = 3
    R = _rows_for(n, "ew", G, C)
    g, x, gamma, beta = _inputs(G, R, C, dt, 19 * n + C, dev)
    x = (x.float() * torch.tensor([0.5, 1.0, 3.0], device=dev)[:, None, None] + torch.tensor([1.0, -2.0, 0.0], device=dev)[:, None, None]).to(dt)
    acc = K.zeros64(2 * G * C, x)
    K.colstats(x.view(G * R, C), acc, G=G, R=R)

    class GroupBN(K.DeferredBN):
        def ref(self, update=False):
            r = super().ref(update)
            r.sumsq = self.acc.data_ptr() + 8 * G * self.C
            r.G = G
            return r

    tol = _tol(dt, 5e-6)
    s = torch.randn(G, C, generator=g, device=dev)
    for act in (0, 1, 2):
        bn = GroupBN(acc, C, R, gamma, beta, EPS, act)
        ref = torch.cat([_ref_fwd(x[i:i + 1], gamma, beta, act)[0] for i in range(G)])
        assert _rel(K.bn_apply(x, bn, G, R), ref) < tol
        assert _rel(K.se_scale_bn(x, bn, s, G, R), ref * torch.sigmoid(s.double())[:, None, :]) < tol
        pool = K.zeros64(G * C, x)
        K.colsum_bn(x, bn, G, R, pool)
        assert _rel(pool.view(G, C), ref.sum(1)) < tol


@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("G,C", [(1, 32), (3, 96), (1, 544)])          # 544: C4 = 136, two column groups of 68 quads
def test_gate_pass_writes_planes_at_group_boundaries(G, C, n):
    """ud_se_scale_bn_planes (fp32, whole 32-channel panels) and ud_se_scale_bn_plane_half re-assemble to ud_se_scale_bn's
    result; ud_residual_bn_planes' tensor equals ud_residual_bn's bit for bit"""
    import ctypes as Ct
    from unidefense_amd import kernels as K
    from unidefense_amd.lib import call as _call
    dev = _dev()
    K.reset_zero_pool()
    R = _rows_for(n, "ew", G, C)
    g, x, gamma, beta = _inputs(G, R, C, torch.float32, 23 * n + C, dev)
    s = torch.randn(G, C, generator=g, device=dev)
    for act in (0, 1, 2):
        bn = _bn(K, x, gamma, beta, act)
        pool = K.zeros64(G * C, x)
        amax = K.colsum_bn_amax(x, bn, G, R, pool)
        y = K.se_scale_bn(x, bn, s, G, R)
        pl = K.se_scale_bn_planes(x, bn, s, G, R, amax)
        h, inv, yd = _unpack(pl, G * R, C).double(), float(pl.inv), y.view(G * R, C).double()
        top = float(yd.abs().max())
        loose = 2.0 ** 15 / (top / inv)
        assert 1.0 <= loose < 8.0, loose
        assert float(((h[0] + h[1] / 2048.0) * inv - yd).abs().max()) <= 2.0 ** -21 * top * loose
        xh = x.half()
        bnh = _bn(K, xh, gamma, beta, act)
        plh = K.se_scale_bn_plane_half(xh, bnh, s, G, R)
        assert float(plh.inv) == 1.0 and torch.equal(_unpack(plh, G * R, C)[0], K.se_scale_bn(xh, bnh, s, G, R).view(G * R, C))
    for act in (0, 1, 2):
        bn0 = _bn(K, x, gamma, beta, act)
        for kp in (torch.tensor([1.0, 0.0, 1.0][:G], device=dev), None):
            ref = K.residual_bn(x, bn0, kp, 1.25, None, G, R, want_absmax=True)
            out, am = torch.empty_like(x), K.amax_slots(x, True)
            pl = K.Planes(G * R, C, x, 2, False)
            _call("ud_residual_bn_planes", K._p(x), Ct.byref(bn0.ref()), K._p(kp), 1.25, K._p(None), K._p(None), K._p(out), K._p(pl.buf),
                  pl.panel, pl.plane, K._p(pl.inv), G, R, C, K._p(am), K._stream())
            assert torch.equal(out, ref)
            h, inv, yd = _unpack(pl, G * R, C).double(), float(pl.inv), ref.view(G * R, C).double()
            top = float(yd.abs().max())
            loose = 2.0 ** 15 / (top / inv)
            assert loose >= 1.0
            assert float(((h[0] + h[1] / 2048.0) * inv - yd).abs().max()) <= 2.0 ** -21 * top * loose

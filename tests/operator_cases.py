"""One table of operator cases for tests/test_operator_bars_cpu.py (no GPU: proves that the yardstick bars of
tests/parity.py separate a right operator from a subtly wrong one) and tests/test_a_operator_bars_gpu.py (holds the HIP
operators to those bars).

A Case carries: `inputs()` (seeded, on the CPU, NCHW); `ref(inputs, dtype, mutation=None)` -> {quantity: tensor} in plain
torch (outputs, input gradients, parameter gradients, running buffers); `run(inputs, dev)` -> the same dict from the HIP
operator through unidefense_amd.tape; `mutations`: the names of the wrong variants this case must reject; `exact`: the
quantities compared bit for bit (after the cast to float32) instead of against a bar.

A MUTATION is a small change inside `ref`: a plausible kernel bug.  MUTATIONS maps its name to `subtle`: True when some
listed case shows it with every quantity within the old 1e-3 bar, i.e. the suite could not see it before.  Measured on the
CPU (tests/test_operator_bars_cpu.py prints the table):
 * subtle: bn_biased_running_var, bn_eps_1e-5_for_1e-3, bn_eps_1e-3_for_1e-5, preact_through_fp16, var_from_fp32_moments
   (1.6e-3 at mean 8 / std 0.05, so its witness is the mean-4 input: 4.6e-4), in_eps_dropped (5e-3 at a plane variance of
   1e-3, witness at 2e-2), se_mean_over_hw_plus_1 (witness at 32 x 32);
 * not subtle (a gross error wherever it shows; the old suite missed it because no operator test had the input or the call,
   not because of its bar): maxpool_last_tie (ties), relu_kink_ge_zero (exact zeros), bn_eval_dx_keeps_mean_terms (the
   eval-form backward), avgpool_divisor_off_by_window (sanity), and dw_weight_grad_missing_border_row: one input row of H
   carries about sqrt(1/H) of a weight gradient over random data, 0.1 to 0.5 at every listed size including 16 x 16, so no
   listed input makes it subtle.

Shapes are the smallest at which the kernels can still go wrong (odd sides, non-square maps, more than one workgroup, C not
a multiple of the 16-channel tile).  No case was dropped because a host wrapper refused its shape.
"""
import functools

import torch
import torch.nn.functional as F

MUTATIONS = {
    "bn_biased_running_var": True,
    "bn_eps_1e-5_for_1e-3": True,
    "bn_eps_1e-3_for_1e-5": True,
    "preact_through_fp16": True,
    "var_from_fp32_moments": True,
    "in_eps_dropped": True,
    "se_mean_over_hw_plus_1": True,
    "maxpool_last_tie": False,
    "relu_kink_ge_zero": False,
    "bn_eval_dx_keeps_mean_terms": False,
    "avgpool_divisor_off_by_window": False,
    "dw_weight_grad_missing_border_row": False,
}


class Case:
    def __init__(self, name, inputs, ref, run, mutations=(), exact=()):
        assert all(m in MUTATIONS for m in mutations), mutations
        self.name, self.inputs, self.ref, self.run = name, inputs, ref, run
        self.mutations, self.exact = tuple(mutations), frozenset(exact)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _refs(name):
    c = BY_NAME[name]
    inp = c.inputs()
    return inp, c.ref(inp, torch.float64), c.ref(inp, torch.float32)


def refs(case):
    """(inputs, ref(float64), ref(float32)) of a case: computed once per process, shared, never modified"""
    return _refs(case.name)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def to_pix(t):
    return t.permute(0, 2, 3, 1).contiguous() if t.dim() == 4 else t.contiguous()


def to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous() if t.dim() == 4 else t


def _act(z, act):
    return z * torch.sigmoid(z) if act == 1 else F.relu(z) if act == 2 else z


def _tape(fn, inputs, params, gouts):
    from tests.test_a_kernels_gpu import run_tape
    return run_tape(fn, inputs, params, lambda o: gouts)


# ------------------------------------------------------------------------------------------------ BatchNorm + act
def _bn_inputs(shape, family, seed):
    def make():
        C = shape[1]
        x = rnd(*shape, seed=seed)
        if family == "randn":
            x = x * 2 + 0.5
        elif family == "offset":                       # mean 8, std 0.05: E[x^2] - E[x]^2 cancels 4.5 digits
            x = x * 0.05 + 8
        elif family == "offset4":                      # mean 4, std 0.05: the same cancellation, 0.6 digits milder
            x = x * 0.05 + 4
        elif family == "constch":                      # channel 1 constant over the batch: variance exactly 0
            x = x * 2 + 0.5
            x[:, 1] = 1.5
        elif family == "head":                         # the [N, C] rows of the classifier's BatchNorm1d
            x = x + 1.0
        return {"x": x, "g": rnd(C, seed=seed + 1) * 0.1 + 1, "b": rnd(C, seed=seed + 2) * 0.1,
                "gy": rnd(*shape, seed=seed + 3), "rm": rnd(C, seed=seed + 4) * 0.3,
                "rv": torch.rand(C, generator=torch.Generator().manual_seed(seed + 5)) * 0.5 + 0.75}
    return make


def _bn_ref(eps, mom, act, training=True, affine=True):
    def ref(inp, dt, mutation=None):
        e = eps
        if mutation == "bn_eps_1e-5_for_1e-3":
            assert eps == 1e-3
            e = 1e-5
        if mutation == "bn_eps_1e-3_for_1e-5":
            assert eps == 1e-5
            e = 1e-3
        x = inp["x"].to(dt).requires_grad_()
        C = x.shape[1]
        dims, shape = [0] + list(range(2, x.dim())), [1, C] + [1] * (x.dim() - 2)
        g, b = (inp["g"].to(dt).requires_grad_(), inp["b"].to(dt).requires_grad_()) if affine else (None, None)
        rm, rv = inp["rm"].to(dt), inp["rv"].to(dt)
        out = {}
        if training:
            mean, var = x.mean(dims), x.var(dims, unbiased=False)
            if mutation == "var_from_fp32_moments":
                m1, m2 = x.detach().mean(dims).float().to(dt), (x.detach() ** 2).mean(dims).float().to(dt)
                var = var + ((m2 - m1 * m1).clamp_min(0) - var).detach()
            n = x.numel() // C
            unb = var.detach() * (1.0 if mutation == "bn_biased_running_var" else n / max(n - 1, 1))
            out["running_mean"] = (1 - mom) * rm + mom * mean.detach()
            out["running_var"] = (1 - mom) * rv + mom * unb
        else:
            mean, var = rm, rv
            out["running_mean"], out["running_var"] = rm.clone(), rv.clone()      # untouched: compared bit for bit
        invstd = 1.0 / torch.sqrt(var.reshape(shape) + e)
        xh = (x - mean.reshape(shape)) * invstd
        z = xh * g.reshape(shape) + b.reshape(shape) if affine else xh
        if mutation == "preact_through_fp16":
            z = z.to(torch.float16).to(dt)
        y = _act(z, act)
        gy = inp["gy"].to(dt)
        grads = torch.autograd.grad(y, [x] + ([g, b] if affine else []), gy, retain_graph=True)
        out["y"], out["dx"] = y.detach(), grads[0]
        if mutation == "bn_eval_dx_keeps_mean_terms":
            assert not training
            (dz,) = torch.autograd.grad(y, z, gy)
            gg = g.reshape(shape) if affine else 1.0
            out["dx"] = (gg * invstd * (dz - dz.mean(dims, keepdim=True) - xh * (dz * xh).mean(dims, keepdim=True))).detach()
        if affine:
            out["dgamma"], out["dbeta"] = grads[1], grads[2]
        return out
    return ref


def _bn_run(eps, mom, act, training=True, affine=True):
    def run(inp, dev):
        from unidefense_amd import tape as T
        rm, rv = inp["rm"].to(dev), inp["rv"].to(dev)
        params = [inp["g"].to(dev).requires_grad_(), inp["b"].to(dev).requires_grad_()] if affine else []

        def fn(t, a, *p):
            return T.batchnorm_act(t, a, p[0] if affine else None, p[1] if affine else None, rm, rv, eps, mom, training, act)
        outs, gin, gp = _tape(fn, [to_pix(inp["x"]).to(dev)], params, [to_pix(inp["gy"]).to(dev)])
        out = {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0]), "running_mean": rm, "running_var": rv}
        if affine:
            out["dgamma"], out["dbeta"] = gp[0], gp[1]
        return out
    return run


def _bn_cases():
    cases = []
    EB, HEAD = (1e-3, 0.01), (1e-5, 0.1)                # (eps, momentum): EfficientNet's BatchNorm2d, the head's BatchNorm1d
    subtle = ("bn_biased_running_var", "bn_eps_1e-5_for_1e-3")
    for act in (0, 1, 2):
        for (N, H, C) in ((4, 16, 144), (3, 5, 20)):
            muts = subtle + (("preact_through_fp16",) if act == 1 else ())
            cases.append(Case(f"bn {N}x{H}x{H}x{C} act{act}", _bn_inputs((N, C, H, H), "randn", 10 + act),
                              _bn_ref(*EB, act), _bn_run(*EB, act), muts))
        cases.append(Case(f"bn1d 2x1792 act{act}", _bn_inputs((2, 1792), "head", 20 + act), _bn_ref(*HEAD, act),
                          _bn_run(*HEAD, act), ("bn_biased_running_var", "bn_eps_1e-3_for_1e-5")))
    # BatchNorm2d(eps 1e-5, momentum 0.1) + ReLU of the ResNet variants: the well-conditioned witness of the reverse eps slip
    cases.append(Case("bn eps1e-5 3x5x5x20 act2", _bn_inputs((3, 20, 5, 5), "randn", 29), _bn_ref(*HEAD, 2),
                      _bn_run(*HEAD, 2), ("bn_biased_running_var", "bn_eps_1e-3_for_1e-5")))
    ev = dict(training=False)
    cases.append(Case("bn eval 3x5x5x20 act1", _bn_inputs((3, 20, 5, 5), "randn", 30), _bn_ref(*EB, 1, **ev),
                      _bn_run(*EB, 1, **ev), ("bn_eps_1e-5_for_1e-3", "bn_eval_dx_keeps_mean_terms", "preact_through_fp16"),
                      exact=("running_mean", "running_var")))
    na = dict(affine=False)
    cases.append(Case("bn no-affine 3x5x5x20 act1", _bn_inputs((3, 20, 5, 5), "randn", 31), _bn_ref(*EB, 1, **na),
                      _bn_run(*EB, 1, **na), subtle))
    for (N, H, C) in ((4, 16, 144), (2, 8, 1632)):
        cases.append(Case(f"bn offset-mean {N}x{H}x{H}x{C} act1", _bn_inputs((N, C, H, H), "offset", 32),
                          _bn_ref(*EB, 1), _bn_run(*EB, 1), ("var_from_fp32_moments",)))
    cases.append(Case("bn offset-mean-4 4x16x16x144 act1", _bn_inputs((4, 144, 16, 16), "offset4", 34), _bn_ref(*EB, 1),
                      _bn_run(*EB, 1), ("var_from_fp32_moments",)))
    cases.append(Case("bn constant-channel 3x5x5x20 act1", _bn_inputs((3, 20, 5, 5), "constch", 33), _bn_ref(*EB, 1),
                      _bn_run(*EB, 1), subtle))
    return cases


# ------------------------------------------------------------------------------------------------ InstanceNorm + swish
def _in_inputs(shape, family, seed):
    def make():
        C = shape[1]
        x = rnd(*shape, seed=seed)
        x = {"randn": x * 1.5 + 0.3, "offset": x * 0.05 + 8, "var1e-3": x * 0.0316 + 0.2, "var2e-2": x * 0.141 + 0.2}[family]
        return {"x": x, "g": rnd(C, seed=seed + 1) * 0.1 + 1, "b": rnd(C, seed=seed + 2) * 0.1, "gy": rnd(*shape, seed=seed + 3)}
    return make


def _in_ref(inp, dt, mutation=None):
    eps = 0.0 if mutation == "in_eps_dropped" else 1e-5
    x, g, b = (inp[k].to(dt).requires_grad_() for k in ("x", "g", "b"))
    mean, var = x.mean((2, 3), keepdim=True), x.var((2, 3), unbiased=False, keepdim=True)
    z = (x - mean) / torch.sqrt(var + eps) * g.reshape(1, -1, 1, 1) + b.reshape(1, -1, 1, 1)
    if mutation == "preact_through_fp16":
        z = z.to(torch.float16).to(dt)
    y = _act(z, 1)
    dx, dg, db = torch.autograd.grad(y, [x, g, b], inp["gy"].to(dt))
    return {"y": y.detach(), "dx": dx, "dgamma": dg, "dbeta": db}


def _in_run(inp, dev):
    from unidefense_amd import tape as T
    outs, gin, gp = _tape(lambda t, a, w_, b_: T.instancenorm_act(t, a, w_, b_, 1e-5, 1), [to_pix(inp["x"]).to(dev)],
                          [inp["g"].to(dev).requires_grad_(), inp["b"].to(dev).requires_grad_()], [to_pix(inp["gy"]).to(dev)])
    return {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0]), "dgamma": gp[0], "dbeta": gp[1]}


def _in_cases():
    rows = [((3, 16, 20), "randn", ("preact_through_fp16",)), ((2, 5, 80), "randn", ("preact_through_fp16",)),
            ((2, 128, 20), "randn", ()), ((2, 5, 80), "offset", ()), ((3, 16, 20), "offset", ()),
            ((2, 5, 80), "var1e-3", ("in_eps_dropped",)), ((3, 16, 20), "var2e-2", ("in_eps_dropped",))]
    return [Case(f"in {N}x{H}x{H}x{C} {fam}", _in_inputs((N, C, H, H), fam, 40 + i), _in_ref, _in_run, muts)
            for i, ((N, H, C), fam, muts) in enumerate(rows)]


# ------------------------------------------------------------------------------------------------ depthwise conv
def _dw_case(N, k, s, H, C, pad, muts):
    def inputs():
        x, w = rnd(N, C, H, H, seed=1), rnd(C, 1, k, k, seed=2, scale=0.3)
        Ho = (H + pad[2] + pad[3] - k) // s + 1
        return {"x": x, "w": w, "gy": rnd(N, C, Ho, Ho, seed=3)}

    def ref(inp, dt, mutation=None):
        x, w, gy = inp["x"].to(dt).requires_grad_(), inp["w"].to(dt).requires_grad_(), inp["gy"].to(dt)
        y = F.conv2d(F.pad(x, list(pad)), w, None, s, 0, 1, C)
        dx, dw = torch.autograd.grad(y, [x, w], gy)
        if mutation == "dw_weight_grad_missing_border_row":
            xm = x.detach().clone()
            xm[:, :, -1] = 0
            (dw,) = torch.autograd.grad(F.conv2d(F.pad(xm, list(pad)), w, None, s, 0, 1, C), w, gy)
        return {"y": y.detach(), "dx": dx, "dw": dw}

    def run(inp, dev):
        from unidefense_amd import tape as T
        outs, gin, gp = _tape(lambda t, a, b: T.dwconv(t, a, b, s, pad), [to_pix(inp["x"]).to(dev)], [inp["w"].to(dev)],
                              [to_pix(inp["gy"]).to(dev)])
        return {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0]), "dw": gp[0]}
    return Case(f"dwconv k{k} s{s} {N}x{H}x{H}x{C} pad{'-'.join(map(str, pad))}", inputs, ref, run, muts)


def _dw_cases():
    from oracle.eb4 import _same_pad          # the static TF-'SAME' rule the model pads with (95 -> 48: (1, 1) / (2, 2))
    assert _same_pad(95, 3, 2) == (1, 1) and _same_pad(95, 5, 2) == (2, 2)
    border = ("dw_weight_grad_missing_border_row",)
    cases = [_dw_case(2, 3, 1, 16, 48, (1, 1, 1, 1), border)]                # the workload shape of test_dwconv
    for k in (3, 5):
        for s in (1, 2):
            for H in (5, 9, 15):
                lo, hi = _same_pad(H, k, s)
                for C in (8, 48):
                    cases.append(_dw_case(2, k, s, H, C, (lo, hi, lo, hi), border if (H == 5 and C == 8) else ()))
    return cases


# ------------------------------------------------------------------------------------------------ dense 3x3 / transposed conv
def _conv_case(kind, N, H, W, Ci, Co, family):
    def inputs():
        wshape = (Co, Ci, 3, 3) if kind == "conv" else (Ci, Co, 3, 3)
        w = rnd(*wshape, seed=2, scale=0.1)
        if family == "lognormal":                      # sign-randomised lognormal(sigma = 3), as tests/test_b_conv_mfma_gpu.py
            g = torch.Generator().manual_seed(7)
            sign = torch.randint(0, 2, wshape, generator=g).float() * 2 - 1
            w = sign * torch.exp(3 * torch.randn(*wshape, generator=g)) * 1e-3
        up = 1 if kind == "conv" else 2
        return {"x": rnd(N, Ci, H, W, seed=1), "w": w, "gy": rnd(N, Co, up * H, up * W, seed=3)}

    def ref(inp, dt, mutation=None):
        x, w = inp["x"].to(dt).requires_grad_(), inp["w"].to(dt).requires_grad_()
        y = F.conv2d(x, w, None, 1, 1) if kind == "conv" else F.conv_transpose2d(x, w, None, 2, 1, 1)
        dx, dw = torch.autograd.grad(y, [x, w], inp["gy"].to(dt))
        return {"y": y.detach(), "dx": dx, "dw": dw}

    def run(inp, dev):
        from unidefense_amd import tape as T
        fn = (lambda t, a, b: T.conv_dense(t, a, b, 1, 1, 1, H, W)) if kind == "conv" else \
            (lambda t, a, b: T.conv_transpose_s2(t, a, b))
        outs, gin, gp = _tape(fn, [to_pix(inp["x"]).to(dev)], [inp["w"].to(dev)], [to_pix(inp["gy"]).to(dev)])
        return {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0]), "dw": gp[0]}
    return Case(f"{kind} {N}x{H}x{W} {Ci}->{Co} {family}", inputs, ref, run)


def _conv_cases():
    return [_conv_case(kind, 2, H, W, Ci, Co, fam) for kind in ("conv", "convT")
            for (H, W, Ci, Co, fam) in ((8, 5, 20, 20, "randn"), (7, 7, 40, 20, "randn"), (8, 5, 20, 20, "lognormal"))]


# ------------------------------------------------------------------------------------------------ squeeze-excite
def _se_case(C, Cs, H, muts):
    N = 3

    def inputs():
        return {"x": rnd(N, C, H, H, seed=1), "wr": rnd(Cs, C, 1, 1, seed=2, scale=0.1), "br": rnd(Cs, seed=3, scale=0.1),
                "we": rnd(C, Cs, 1, 1, seed=4, scale=0.3), "be": rnd(C, seed=5, scale=0.1), "gy": rnd(N, C, H, H, seed=6)}

    def ref(inp, dt, mutation=None):
        x, wr, br, we, be = (inp[k].to(dt).requires_grad_() for k in ("x", "wr", "br", "we", "be"))
        hw = H * H + (1 if mutation == "se_mean_over_hw_plus_1" else 0)
        s = x.sum((2, 3), keepdim=True) / hw
        s = F.conv2d(s, wr, br)
        s = F.conv2d(s * torch.sigmoid(s), we, be)
        y = torch.sigmoid(s) * x
        gr = torch.autograd.grad(y, [x, wr, br, we, be], inp["gy"].to(dt))
        return dict(zip(("y", "dx", "dWr", "dbr", "dWe", "dbe"), (y.detach(),) + gr))

    def run(inp, dev):
        from unidefense_amd import tape as T
        outs, gin, gp = _tape(lambda t, a, *p: T.squeeze_excite(t, a, *p), [to_pix(inp["x"]).to(dev)],
                              [inp[k].to(dev) for k in ("wr", "br", "we", "be")], [to_pix(inp["gy"]).to(dev)])
        return dict(zip(("y", "dx", "dWr", "dbr", "dWe", "dbe"), (to_nchw(outs[0]), to_nchw(gin[0])) + tuple(gp)))
    return Case(f"se C{C} Cs{Cs} {H}x{H}", inputs, ref, run, muts)


def _se_cases():
    m = ("se_mean_over_hw_plus_1",)
    return [_se_case(144, 6, 3, m), _se_case(24, 6, 1, m), _se_case(144, 6, 32, m)]


# ------------------------------------------------------------------------------------------------ pooling
def _pool_input(shape, family, seed):
    x = rnd(*shape, seed=seed)
    if family == "relu":                               # after BN + ReLU: tied zeros are the normal case
        return F.relu(x)
    if family == "halves":                             # ties at non-zero values
        return torch.round(x * 2) / 2
    return torch.full(shape, 0.5)                      # "equal": every window fully tied


def _maxpool_last(x):
    """3/2/1 max-pool whose gradient goes to the LAST maximum of the window in scan order (ATen, and the kernel: the first)"""
    p = F.pad(x, (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2).flatten(-2)      # [N, C, Ho, Wo, 9]
    hit = (p == p.max(-1, keepdim=True).values).flip(-1)
    last = (hit & (hit.int().cumsum(-1) == 1)).flip(-1)
    return torch.where(last, p, torch.zeros_like(p)).sum(-1)


def _maxpool_case(N, C, H, W, family, direct=False):
    def inputs():
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return {"x": _pool_input((N, C, H, W), family, 5), "gy": rnd(N, C, Ho, Wo, seed=6)}

    def ref(inp, dt, mutation=None):
        x = inp["x"].to(dt).requires_grad_()
        y = _maxpool_last(x) if mutation == "maxpool_last_tie" else F.max_pool2d(x, 3, 2, 1)
        (dx,) = torch.autograd.grad(y, x, inp["gy"].to(dt))
        return {"y": y.detach(), "dx": dx}

    def run(inp, dev):
        from unidefense_amd import kernels as K
        from unidefense_amd import tape as T
        xp, gp = to_pix(inp["x"]).to(dev), to_pix(inp["gy"]).to(dev)
        if direct:                                     # C not a multiple of 4: the kernels themselves (one channel per thread)
            y, arg = K.maxpool3s2_fwd(xp)
            return {"y": to_nchw(y), "dx": to_nchw(K.maxpool3s2_bwd(gp, arg, H, W))}
        outs, gin, _ = _tape(lambda t, a: T.maxpool3s2(t, a), [xp], [], [gp])
        return {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0])}
    return Case(f"maxpool {N}x{C}x{H}x{W} {family}{' direct' if direct else ''}", inputs, ref, run, ("maxpool_last_tie",),
                exact=("y",))


def _avgpool_case(H, W, k):
    N, C = 2, 8

    def inputs():
        return {"x": rnd(N, C, H, W, seed=7), "gy": rnd(N, C, H // k, W // k, seed=8)}

    def ref(inp, dt, mutation=None):
        x = inp["x"].to(dt).requires_grad_()
        y = F.adaptive_avg_pool2d(x, (H // k, W // k))
        if mutation == "avgpool_divisor_off_by_window":
            y = y * (k * k / float((k + 1) ** 2))
        (dx,) = torch.autograd.grad(y, x, inp["gy"].to(dt))
        return {"y": y.detach(), "dx": dx}

    def run(inp, dev):
        from unidefense_amd import tape as T
        outs, gin, _ = _tape(lambda t, a: T.avgpool(t, a, k), [to_pix(inp["x"]).to(dev)], [], [to_pix(inp["gy"]).to(dev)])
        return {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0])}
    return Case(f"avgpool k{k} {H}x{W}", inputs, ref, run, ("avgpool_divisor_off_by_window",))


def _pool_cases():
    cases = [_maxpool_case(N, C, H, W, fam) for (N, C, H, W) in ((2, 8, 15, 15), (1, 4, 7, 9), (2, 64, 16, 16))
             for fam in ("relu", "halves", "equal")]
    cases.append(_maxpool_case(1, 6, 7, 9, "relu", direct=True))
    return cases + [_avgpool_case(H, W, k) for (H, W) in ((8, 8), (4, 12)) for k in (1, 2, 4)]


# ------------------------------------------------------------------------------------------------ small elementwise ops
def _add_relu_case():
    N, C, H = 2, 8, 5

    def inputs():
        a = torch.round(rnd(N, C, H, H, seed=1) * 2) / 2
        b = torch.round(rnd(N, C, H, H, seed=2) * 2) / 2
        b[:, ::2] = -a[:, ::2]                         # half of the sums are exactly 0: the kink
        return {"a": a, "b": b, "gy": rnd(N, C, H, H, seed=3)}

    def ref(inp, dt, mutation=None):
        s = inp["a"].to(dt) + inp["b"].to(dt)
        gy = inp["gy"].to(dt)
        g = gy * ((s >= 0) if mutation == "relu_kink_ge_zero" else (s > 0)).to(dt)
        return {"y": F.relu(s), "da": g, "db": g.clone()}

    def run(inp, dev):
        from unidefense_amd import tape as T
        outs, gin, _ = _tape(lambda t, p, q: T.add_relu(t, p, q), [to_pix(inp["a"]).to(dev), to_pix(inp["b"]).to(dev)], [],
                             [to_pix(inp["gy"]).to(dev)])
        return {"y": to_nchw(outs[0]), "da": to_nchw(gin[0]), "db": to_nchw(gin[1])}
    return Case("add+relu exact zeros 2x5x5x8", inputs, ref, run, ("relu_kink_ge_zero",), exact=("y", "da", "db"))


def _concat_case():
    N, H = 2, 5

    def inputs():
        return {"a": rnd(N, 8, H, H, seed=1), "b": rnd(N, 12, H, H, seed=2), "gy": rnd(N, 20, H, H, seed=3)}

    def ref(inp, dt, mutation=None):
        gy = inp["gy"].to(dt)
        return {"y": torch.cat([inp["a"].to(dt), inp["b"].to(dt)], 1), "da": gy[:, :8].clone(), "db": gy[:, 8:].clone()}

    def run(inp, dev):
        from unidefense_amd import tape as T
        outs, gin, _ = _tape(lambda t, p, q: T.concat_channels(t, [p, q]), [to_pix(inp["a"]).to(dev), to_pix(inp["b"]).to(dev)],
                             [], [to_pix(inp["gy"]).to(dev)])
        return {"y": to_nchw(outs[0]), "da": to_nchw(gin[0]), "db": to_nchw(gin[1])}
    return Case("concat / slice 8+12 channels 2x5x5", inputs, ref, run, exact=("y", "da", "db"))


def _residual_case():
    N, C, H = 4, 8, 5

    def inputs():
        return {"x": rnd(N, C, H, H, seed=1), "skip": rnd(N, C, H, H, seed=2), "keep": torch.tensor([1.0, 0.0, 1.0, 1.0]),
                "gy": rnd(N, C, H, H, seed=3)}

    def ref(inp, dt, mutation=None):
        x, sk = inp["x"].to(dt).requires_grad_(), inp["skip"].to(dt).requires_grad_()
        y = x / 0.9 * inp["keep"].to(dt).view(-1, 1, 1, 1) + sk
        dx, dsk = torch.autograd.grad(y, [x, sk], inp["gy"].to(dt))
        return {"y": y.detach(), "dx": dx, "dskip": dsk}

    def run(inp, dev):
        from unidefense_amd import tape as T
        keep = inp["keep"].to(dev)
        outs, gin, _ = _tape(lambda t, a, b: T.residual(t, a, b, keep, 0.9),
                             [to_pix(inp["x"]).to(dev), to_pix(inp["skip"]).to(dev)], [], [to_pix(inp["gy"]).to(dev)])
        return {"y": to_nchw(outs[0]), "dx": to_nchw(gin[0]), "dskip": to_nchw(gin[1])}
    return Case("residual / drop-connect 4x5x5x8", inputs, ref, run)


def _gate_mix_case():
    shape = (3, 5, 5, 8)

    def inputs():
        return {"p": rnd(*shape, seed=1), "q": rnd(*shape, seed=2), "alpha": torch.tensor(0.3), "gy": rnd(*shape, seed=3)}

    def ref(inp, dt, mutation=None):
        p, q, al = (inp[k].to(dt).requires_grad_() for k in ("p", "q", "alpha"))
        a = torch.sigmoid(al)
        y = (1 - a) * p + a * q
        dp, dq, da = torch.autograd.grad(y, [p, q, al], inp["gy"].to(dt))
        return {"y": y.detach(), "dp": dp, "dq": dq, "dalpha": da}

    def run(inp, dev):
        from unidefense_amd import tape as T
        outs, gin, gp = _tape(lambda t, a, b, c: T.gate_mix(t, a, b, c), [inp["p"].to(dev), inp["q"].to(dev)],
                              [inp["alpha"].to(dev)], [inp["gy"].to(dev)])
        return {"y": outs[0], "dp": gin[0], "dq": gin[1], "dalpha": gp[0].reshape(())}
    return Case("gate-mix 3x5x5x8", inputs, ref, run)


CASES = (_bn_cases() + _in_cases() + _dw_cases() + _conv_cases() + _se_cases() + _pool_cases()
         + [_add_relu_case(), _concat_case(), _residual_case(), _gate_mix_case()])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

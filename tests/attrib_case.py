"""The known integrand of the attribution tests (tests/test_attrib_cpu.py, tests/test_v_attrib_gpu.py): the score
F(x) = sum x^3 / 3, whose gradient x^2 makes the integrated-gradients integrand quadratic in the path parameter, so two
Gauss-Legendre nodes integrate it exactly and the midpoint rule does not."""
import numpy as np
import torch

from unidefense_amd import attrib as A

N, SIZE = 3, 128
ROUNDINGS = 16 * 2.0 ** -24          # per element: a d, + b, the square (and autograd's 3 x^2 / 3) in fp32, alpha's own rounding


def cubic(out, y, xp):
    return (xp ** 3).flatten(1).sum(1) / 3


def inputs():
    """x, a baseline per sample, labels, stream ids: all different per sample"""
    g = torch.Generator().manual_seed(20261021)
    x = torch.rand(N, 3, SIZE, SIZE, generator=g) * 2 - 1
    b = torch.rand(N, 3, SIZE, SIZE, generator=g) * 2 - 1
    return x, b, torch.tensor([1, 0, 1]), torch.tensor([11, (1 << 32) + 5, 7])


def exact(x, b):
    """F(x) - F(b) per sample in float64"""
    x, b = x.double().numpy(), b.double().numpy()
    return ((x ** 3 - b ** 3) / 3).reshape(x.shape[0], -1).sum(1)


def restated(x, b, rule, steps=2):
    """(total, bar) per sample in float64 with the fp32-rounded nodes the device table holds: total = sum_e (x - b) sum_k w_k
    g_k, g_k = (b + a_k (x - b))^2; bar = ROUNDINGS sum_e |x - b| max_k |g_k|"""
    a, w = A.attribution_schedule(steps, rule)
    x, b = x.double().numpy(), b.double().numpy()
    d = x - b
    gs = [(b + float(np.float32(ak)) * d) ** 2 for ak in a]
    acc = sum(wk * g for wk, g in zip(w, gs))
    flat = lambda t: t.reshape(t.shape[0], -1)
    return flat(d * acc).sum(1), ROUNDINGS * flat(np.abs(d) * np.max(np.abs(np.stack(gs)), 0)).sum(1)

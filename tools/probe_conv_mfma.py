"""csrc/conv_mfma.hip against the path it replaces, per shape: isolated device time of kernels.conv_gather_nt for every
(Cin, Cout, geometry) the library instantiates, at the sizes of the UDEB4 256^2 batch-32 step (the decoder's forward convs,
their data gradients, the transposed convs and their stride-2 data gradients), replayed from a small hipGraph
(kernels._time_launches, as tools/probe_thin_x3.py).  The old path's time includes what it launches around the conv
(the zero fill in front of a split-K result).  Also prints the worst difference of the two results relative to max|old|."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unidefense_amd import kernels as K
dev = torch.device("cuda:0")
N = int(os.environ.get("UD_PROBE_BATCH", "32"))
# (label, Cin, Cout, output side, geometry class): 0 same, 1 transposed stride 2, 2 stride 2
SHAPES = (("fwd  80->80  same", 80, 80, 32, 0), ("fwd  80->40  same", 80, 40, 32, 0), ("dgrad 40->80 same", 40, 80, 32, 0),
          ("fwd  40->40  same", 40, 40, 64, 0), ("fwd  40->20  same", 40, 20, 64, 0), ("dgrad 20->40 same", 20, 40, 64, 0),
          ("fwd  20->20  same", 20, 20, 128, 0),
          ("convT 80->80", 80, 80, 32, 1), ("convT 40->40", 40, 40, 64, 1), ("convT 20->20", 20, 20, 128, 1),
          ("convT dgrad 40->40", 40, 40, 32, 2), ("convT dgrad 20->20", 20, 20, 64, 2),
          ("fwd 160->80 same", 160, 80, 16, 0), ("dgrad 80->160 same", 80, 160, 16, 0), ("convT dgrad 80->80", 80, 80, 16, 2))
REPEAT = int(os.environ.get("UD_PROBE_REPEAT", "3"))          # timings per arm, interleaved; the table shows min .. max


def run(on, x, w, g, fn=None):
    fn = fn or K.conv_gather_nt
    saved = K._CONV_MFMA, K._CONV_MFMA_MIN_M, K._CONV_MFMA_SHAPES, K._CONV_MFMA_WGRAD_SHAPES
    K._CONV_MFMA, K._CONV_MFMA_MIN_M, K._CONV_MFMA_SHAPES, K._CONV_MFMA_WGRAD_SHAPES = on, 1, None, None
    try:
        K.reset_zero_pool()
        out = fn(x, w, g).clone()
        K.reset_zero_pool()
        return out, K._time_launches(lambda: fn(x, w, g))
    finally:
        K._CONV_MFMA, K._CONV_MFMA_MIN_M, K._CONV_MFMA_SHAPES, K._CONV_MFMA_WGRAD_SHAPES = saved


def table(shapes, make, fn=None):
    print("%-20s %8s | %15s %15s %6s | %9s" % ("shape", "out px", "old us", "new us", "ratio", "max diff"))
    for row in shapes:
        label, px, p, q, g = make(*row)
        t_old, t_new = [], []
        for _ in range(REPEAT):
            old, t = run(False, p, q, g, fn)
            t_old.append(t * 1e3)
            new, t = run(True, p, q, g, fn)
            t_new.append(t * 1e3)
        d = ((new - old).abs().max() / old.abs().max()).item()
        med = lambda v: sorted(v)[len(v) // 2]
        print("%-20s %8d | %6.1f ..%6.1f %6.1f ..%6.1f %6.2f | %9.2e" % (label, px, min(t_old), max(t_old), min(t_new), max(t_new),
                                                                   med(t_old) / med(t_new), d), flush=True)



def make_nt(label, ci, co, ho, mode):
    hi = ho if mode == 0 else ho // 2 if mode == 1 else 2 * ho
    g = K.conv_geom(N, hi, hi, ci, ho, ho, 3, 3, 1 if mode == 0 else 2, 1, 1, 1 if mode == 1 else 0)
    return label, N * ho * ho, torch.randn(N, hi, hi, ci, device=dev), torch.randn(co, 9 * ci, device=dev) * 0.05, g


def make_wgrad(label, ci, ma, ho, mode):
    """weight gradient: a [pixels, ma] against ci gathered channels on a grid of ho x ho (mode 2: gathered at stride 2 from 2 ho)"""
    hi = ho if mode == 0 else 2 * ho
    g = K.conv_geom(N, hi, hi, ci, ho, ho, 3, 3, 1 if mode == 0 else 2, 1, 1, 0)
    return label, N * ho * ho, torch.randn(N * ho * ho, ma, device=dev), torch.randn(N, hi, hi, ci, device=dev), g


# (label, gathered channels, Ma, grid side, geometry class)
WSHAPES = (("wgrad 160x80 same", 160, 80, 16, 0), ("wgrad 80x80 same", 80, 80, 32, 0), ("wgrad 80x40 same", 80, 40, 32, 0),
           ("wgrad 40x40 same", 40, 40, 64, 0), ("wgrad 40x20 same", 40, 20, 64, 0), ("wgrad 20x20 same", 20, 20, 128, 0),
           ("wgrad convT 80", 80, 80, 16, 2), ("wgrad convT 40", 40, 40, 32, 2), ("wgrad convT 20", 20, 20, 64, 2))
which = os.environ.get("UD_PROBE_WHICH", "nt,wgrad")
if "nt" in which:
    table(SHAPES, make_nt)
if "wgrad" in which:
    table(WSHAPES, make_wgrad, K.conv_gather_wgrad)

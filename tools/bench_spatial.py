"""The warp kernel against the byte model, and SpatialRunner's cost per candidate against the forward replay it is built on.

    python tools/bench_spatial.py                                  # UDEB4 256^2 and 380^2, bs 32: one JSON line per row
    python tools/bench_spatial.py --sizes 256 --out profiles/r18/spatial_rows.txt
    python tools/bench_spatial.py --no-runner                      # the kernel only

Kernel: a warp is one launch that reads the batch once and writes it once, so its model is 2 N 3 S^2 4 B at 5.5 TB/s plus one
launch inside a replayed graph (4.5 us).  It is timed like the corruptions (tools/bench_corrupt.py): inside a
captured graph of --launches launches that rotate over enough (input, output) buffer pairs to exceed the 256 MiB Infinity Cache
twice; a window is one replay between device events, and the figure is the window over --launches: the kernel plus the gap to
the next one.  Rows: the identity, 10 degrees, 45 degrees at scale 0.9, scale 0.5 with a shift of a quarter of the side (still
staged: a tile's source box is 64 x 64 cells whatever the shift) and scale 0.25 (the direct path), border "reflect".

Runner: SpatialRunner and InferenceRunner, same model, shape and precision, warmed up and captured, then timed window by window,
alternating (a window: --iters replays ending in a device synchronise, host clock).  One replay of SpatialRunner's graph is one
candidate: warp, forward, objective, control.  InferenceRunner is unchanged by the warps, so its column stands for the tree
before them."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable
LAUNCH_US = 4.5           # one launch inside a replayed graph
CACHE_BYTES = 256 << 20   # Infinity Cache


def _transforms(size):
    return [("identity", dict()), ("10 deg", dict(angle=10.0)), ("45 deg, scale 0.9", dict(angle=45.0, scale=0.9)),
            ("scale 0.5, shift S/4", dict(scale=0.5, shift=(size / 4.0, size / 4.0))), ("scale 0.25 (direct)", dict(scale=0.25))]


def _kernel_rows(a, dev, emit):
    from unidefense_amd import corrupt as CR
    from unidefense_amd import kernels as K
    from unidefense_amd import spatial as SP
    for size in a.sizes:
        shape = (a.batch, 3, size, size)
        nbytes = a.batch * 3 * size * size * 4
        pairs = max(2, -(-2 * CACHE_BYTES // (2 * nbytes)))
        gen = torch.Generator(device=dev).manual_seed(1)
        xs = [torch.rand(shape, device=dev, generator=gen) * 2.0 - 1.0 for _ in range(pairs)]
        outs = [torch.empty(shape, device=dev) for _ in range(pairs)]
        lut = CR._lut(dev)
        row = torch.zeros(a.batch, dtype=torch.int32, device=dev)
        model_us = LAUNCH_US + 2 * nbytes / HBM_BPS * 1e6
        for name, kw in _transforms(size):
            mat = torch.tensor([SP.affine_q16(**kw)], dtype=torch.int64).to(torch.int32).to(dev)

            def launches():
                for i in range(a.launches):
                    K.warp_affine(xs[i % pairs], outs[i % pairs], lut, mat, row, a.border)
            launches()                                   # code objects
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launches()
            g.replay()
            torch.cuda.synchronize(dev)
            t = []
            for _ in range(a.windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1) * 1e3 / a.launches)
            emit({"kernel": "warp_affine", "transform": name, "border": a.border, "size": size, "batch": a.batch,
                  "us_min": round(min(t), 2), "us_median": round(statistics.median(t), 2), "us_max": round(max(t), 2),
                  "model_us": round(model_us, 2), "median_over_model": round(statistics.median(t) / model_us, 2),
                  "bytes": 2 * nbytes, "buffer_pairs": pairs, "launches_per_window": a.launches, "windows": a.windows})
        del xs, outs


def _window(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def _runner_rows(a, dev, emit):
    from unidefense_amd.infer import InferenceRunner
    from unidefense_amd.model import load_model
    from unidefense_amd.spatial import SpatialRunner
    m = load_model("UDEB4")(num_classes=2, drop_rate=0.5, extractor="efficientnet-b4")
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    m = m.to(dev).eval()
    size = a.sizes[0]
    x = param_fill.make_input(a.batch, size, 3).to(dev)
    y = param_fill.make_labels(a.batch).to(dev)
    for precision in a.precisions:
        inf = InferenceRunner(m, a.batch, size, precision)
        spa = SpatialRunner(m, a.batch, size, grid=(3, 1, 1), precision=precision)     # four candidates: the calls below stay short
        for _ in range(3):                       # the eager warm-up, the capture, one replay
            inf(x)
            spa(x, y)

        def replays(r):
            for _ in range(a.iters):
                r.graph.replay()
        ti, ts = [], []
        for _ in range(a.windows):
            ti.append(_window(lambda: replays(inf), dev) / a.iters)
            ts.append(_window(lambda: replays(spa), dev) / a.iters)
        mi, ms = statistics.median(ti), statistics.median(ts)
        emit({"runner": "spatial, per candidate", "model": "UDEB4", "size": size, "batch": a.batch, "precision": precision,
              "infer_ms_per_replay": round(mi, 3), "spatial_ms_per_candidate": round(ms, 3),
              "spatial_minus_infer_us": round((ms - mi) * 1e3, 1), "spatial_over_infer": round(ms / mi, 4),
              "infer_min_max_ms": [round(min(ti), 3), round(max(ti), 3)], "spatial_min_max_ms": [round(min(ts), 3), round(max(ts), 3)],
              "iters_per_window": a.iters, "windows": a.windows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 380])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--border", default="reflect")
    ap.add_argument("--launches", type=int, default=40, help="kernel launches per captured graph")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20, help="runner replays per timed window")
    ap.add_argument("--precisions", nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--no-runner", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    _kernel_rows(a, dev, emit)
    if not a.no_runner:
        _runner_rows(a, dev, emit)


if __name__ == "__main__":
    main()

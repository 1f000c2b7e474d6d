"""The flow-field attack's four kernels against their byte model, and FlowRunner's iteration against the PGD iteration.

    python tools/bench_flow.py                       # kernels at 256^2 and 380^2, bs 32; the runner at 256^2 fp32 and fp16
    python tools/bench_flow.py --only kernels --sizes 256
    python tools/bench_flow.py --only runner --precision fp16

Kernels: each entry point is captured into a hipGraph of `sets` x `reps` launches that rotate over `sets` buffer sets, the sets
together larger than twice the Infinity Cache (2 x 256 MiB), so that no launch finds its streams cached by the launch before;
a window is one replay between two device events; reported: the median window per launch, the windows' spread, and the byte
model per pixel (grad: reads g 12 + w 8 + x 12, writes gw 8; update: reads w 8 + gw 8 + x 12, writes w 8 (+ w_best 8 where
kept) + x_adv 12; warp: reads w 8 + x 12, writes 12) at HBM_BPS.  The flows are N(0, 0.7) pixels clamped to +-2: a tap lies next
to its own pixel, as in the attack.
Runner: FlowRunner and AttackRunner are warmed up (eager call, capturing call) and timed window by window, alternating: a
window is --iters replays of the captured iteration ending in a device synchronise, on the host clock."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable
CACHE = 256 << 20         # the Infinity Cache
MODEL = {"warp": (20, 12), "grad": (32, 8), "update_keep": (28, 36), "update_nokeep": (28, 28), "closing": (20, 12)}    # bytes per pixel (read, written)


def _kernel_rows(size, bs, reps, windows, dev):
    from unidefense_amd import kernels as K
    px = bs * size * size
    per_set = px * 4 * (3 + 3 + 2 + 2 + 2 + 3)
    sets = max(2, math.ceil(2 * CACHE / per_set) + 1)
    gen = torch.Generator(device=dev).manual_seed(size)
    S = []
    for _ in range(sets):
        x = torch.randn(bs, 3, size, size, generator=gen, device=dev)
        S.append({"x": x, "g": torch.randn_like(x) * 0.01, "xa": torch.empty_like(x),
                  "w": (torch.randn(bs, 2, size, size, generator=gen, device=dev) * 0.7).clamp_(-2, 2),
                  "wb": torch.zeros(bs, 2, size, size, device=dev), "gw": torch.randn(bs, 2, size, size, generator=gen, device=dev)})
    keep, nokeep = torch.ones(bs, dtype=torch.int32, device=dev), torch.zeros(bs, dtype=torch.int32, device=dev)
    f = torch.rand(bs, device=dev)
    ist, fst, hist = K.flow_state(bs, 200000, dev)                # more rows than launches: every launch takes the full path
    launches = {
        "warp": lambda s: K.flow_warp(s["x"], s["w"], s["xa"]),
        "grad": lambda s: K.flow_grad(s["g"], s["x"], s["w"], s["gw"], 1, 0.05, 1e-8),
        "update_keep": lambda s: K.flow_update(s["w"], s["wb"], s["gw"], keep, s["x"], s["xa"], 0.0, 2.0),      # step 0: w keeps its values
        "update_nokeep": lambda s: K.flow_update(s["w"], s["wb"], s["gw"], nokeep, s["x"], s["xa"], 0.0, 2.0),
        "closing": lambda s: K.flow_update(s["w"], s["wb"], None, nokeep, s["x"], s["xa"], 0.0, 2.0, closing=True),
        "control": lambda s: K.flow_control(f, ist, fst, hist),
    }
    rows = []
    for name, launch in launches.items():
        for s in S:                                               # warm-up: code objects loaded before the capture
            launch(s)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(reps):
                for s in S:
                    launch(s)
        graph.replay()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            torch.cuda.synchronize(dev)
            ts.append(a.elapsed_time(b) * 1e3 / (reps * sets))
        row = {"kernel": "ud_flow_" + name, "size": size, "batch": bs, "sets": sets, "set_MiB": round(per_set / 2 ** 20, 1),
               "launches_per_window": reps * sets, "windows": windows, "us_per_launch": round(statistics.median(ts), 2),
               "us_min_max": [round(min(ts), 2), round(max(ts), 2)]}
        if name in MODEL:
            rd, wr = MODEL[name]
            ideal = (rd + wr) * px / HBM_BPS * 1e6
            row.update(bytes_per_pixel=[rd, wr], ideal_us_at_5_5TBps=round(ideal, 2),
                       share_of_model=round(ideal / statistics.median(ts), 3))
        rows.append(row)
    return rows


def _model(dev):
    from unidefense_amd.model import load_model
    m = load_model("UDEB4")(num_classes=2, drop_rate=0.5, extractor="efficientnet-b4")
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev).eval()


def _window(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def _runner_row(m, precision, a, dev):
    from unidefense_amd.attack import AttackRunner
    from unidefense_amd.flow import FlowRunner
    bs, size = a.batch, a.runner_size
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    pgd = AttackRunner(m, bs, size, norm="linf", eps=2.0 / 255.0, steps=a.iters, precision=precision)
    flow = FlowRunner(m, bs, size, max_flow=2.0, steps=a.iters, precision=precision)
    for _ in range(2):                       # the eager warm-up, then the capture
        pgd(x, y)
        flow(x, y)

    def pgd_iters(n):
        pgd._start(x, y, None)
        for _ in range(n):
            pgd.graph.replay()

    def flow_iters(n):
        with torch.no_grad():
            flow.w.zero_()
            flow.ist.zero_()
            flow.x_adv.copy_(x)
        for _ in range(n):
            flow.graph.replay()
    tp, tf, tc = [], [], []
    for _ in range(a.windows):
        tp.append(_window(lambda: pgd_iters(a.iters), dev) / a.iters)
        tf.append(_window(lambda: flow_iters(a.iters), dev) / a.iters)
    for _ in range(3):
        tc.append(_window(lambda: flow(x, y), dev))
    mp, mf = statistics.median(tp), statistics.median(tf)
    return {"model": "UDEB4", "size": size, "batch": bs, "precision": precision, "iters_per_window": a.iters, "windows": a.windows,
            "pgd_ms_per_iter": round(mp, 3), "flow_ms_per_iter": round(mf, 3), "flow_minus_pgd_us": round((mf - mp) * 1e3, 1),
            "flow_over_pgd": round(mf / mp, 4), "pgd_min_max_ms": [round(min(tp), 3), round(max(tp), 3)],
            "flow_min_max_ms": [round(min(tf), 3), round(max(tf), 3)], "flow_call_ms": round(statistics.median(tc), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernels", "runner", "both"), default="both")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 380])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20, help="rounds over the buffer sets inside one captured window")
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default="both")
    ap.add_argument("--runner-size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window (>= 20)")
    ap.add_argument("--windows", type=int, default=5, help="windows (>= 5); the two runners alternate")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    if a.only in ("kernels", "both"):
        for size in a.sizes:
            for row in _kernel_rows(size, a.batch, a.reps, a.windows, dev):
                print(json.dumps(row), flush=True)
    if a.only in ("runner", "both"):
        m = _model(dev)
        for p in (("fp32", "fp16") if a.precision == "both" else (a.precision,)):
            print(json.dumps(_runner_row(m, p, a, dev)), flush=True)


if __name__ == "__main__":
    main()

"""A Square attack query against the forward replay it is built on: SquareRunner's captured iteration next to InferenceRunner's
graph, same model, shape and precision, in one process.

    python tools/bench_square.py                                   # UDEB4 256^2 bs 32, fp32 and fp16: one JSON line each
    python tools/bench_square.py --precision fp16 --steps 1000
    python tools/bench_square.py --trace-iters 30                  # replays only, for `rocprofv3 --kernel-trace --stats -- python ...`

Both runners are warmed up (eager call, capturing call) and then timed window by window, alternating: a window is --iters
replays ending in a device synchronise, on the host clock.  The Square windows are taken twice: from a fresh start (the
schedule's largest squares, side s_first) and with the per-sample counter set --iters before the end (its smallest, side
s_last).  Reported per precision: the median window of each per iteration, every window's spread, the differences, and the model
of what a query adds to the forward: the launch floor of two kernels (ud_square_propose, ud_square_control; DESIGN 3f: 4.5 us
each), the objective's few N-sized torch ops, and the propose bytes — at most 2 (s^2 + s'^2) 3 N 4 B of reads and writes for
consecutive windows of sides s' and s — at 5.5 TB/s.  `square_call_ms` is a whole SquareRunner call of --iters steps (draws,
copy-in, iters + 1 replays, the closing propose, the merge) for orientation.  InferenceRunner is unchanged by the Square attack,
so its column stands for the tree before it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

EPS = 8.0 / 255.0
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable
LAUNCH_US = 4.5           # one launch inside a replayed graph


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


def _row(m, precision, a, dev):
    from unidefense_amd import kernels as K
    from unidefense_amd.attack import SquareRunner
    from unidefense_amd.infer import InferenceRunner
    bs, size = a.batch, a.size
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    gen = torch.Generator().manual_seed(1)
    inf = InferenceRunner(m, bs, size, precision)
    sq = SquareRunner(m, bs, size, eps=EPS, steps=a.steps, early_stop=False, precision=precision)
    short = SquareRunner(m, bs, size, eps=EPS, steps=a.iters, early_stop=False, precision=precision)
    for _ in range(2):                       # the eager warm-up, then the capture
        inf(x)
        short(x, y, gen)
    # the long-schedule runner is warmed up and captured on a few iterations (a whole eager call would be `steps` eager forwards):
    # the same launches, the same graph
    sq.calls = 2
    sq._buffers(x, y)
    sq._start(gen)
    for _ in range(3):
        sq._iteration()
    torch.cuda.synchronize(dev)
    sq.graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(sq.graph):
        sq._iteration()

    def inf_iters(n):
        for _ in range(n):
            inf.graph.replay()

    def square_iters(n, first_k):
        sq._start(gen)
        if first_k:
            sq.ist[K.SQUARE_I["k"]].fill_(first_k)
        for _ in range(n):
            sq.graph.replay()
    late = a.steps - a.iters + 1
    if a.trace_iters:
        inf_iters(a.trace_iters)
        square_iters(a.trace_iters, 0)
        torch.cuda.synchronize(dev)
        return {"model": "UDEB4", "size": size, "batch": bs, "precision": precision, "trace_iters": a.trace_iters}
    ti, tf, tl, tc = [], [], [], []
    for _ in range(a.windows):
        ti.append(_window(lambda: inf_iters(a.iters), dev) / a.iters)
        tf.append(_window(lambda: square_iters(a.iters, 0), dev) / a.iters)
        tl.append(_window(lambda: square_iters(a.iters, late), dev) / a.iters)
    for _ in range(3):
        tc.append(_window(lambda: short(x, y, gen), dev))
    mi, mf, ml = statistics.median(ti), statistics.median(tf), statistics.median(tl)
    s_first, s_last = sq.sizes[0], sq.sizes[-1]

    def model_us(s):
        return 2 * LAUNCH_US + 2 * (2 * s * s) * 3 * bs * 4 / HBM_BPS * 1e6
    return {"model": "UDEB4", "size": size, "batch": bs, "precision": precision, "steps": a.steps, "iters_per_window": a.iters,
            "windows": a.windows, "infer_ms_per_iter": round(mi, 3), "square_first_ms_per_iter": round(mf, 3),
            "square_last_ms_per_iter": round(ml, 3), "s_first": s_first, "s_last": s_last,
            "first_minus_infer_us": round((mf - mi) * 1e3, 1), "last_minus_infer_us": round((ml - mi) * 1e3, 1),
            "square_first_over_infer": round(mf / mi, 4), "square_last_over_infer": round(ml / mi, 4),
            "infer_min_max_ms": [round(min(ti), 3), round(max(ti), 3)], "square_first_min_max_ms": [round(min(tf), 3), round(max(tf), 3)],
            "square_last_min_max_ms": [round(min(tl), 3), round(max(tl), 3)],
            "model_first_us": round(model_us(s_first), 2), "model_last_us": round(model_us(s_last), 2),
            "propose_bytes_max_first": 2 * (2 * s_first * s_first) * 3 * bs * 4,
            "infer_img_per_s": round(bs / mi * 1e3, 1), "square_first_queries_per_s": round(bs / mf * 1e3, 1),
            "square_call_ms": round(statistics.median(tc), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default="both")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5000, help="the schedule the windows are taken from")
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window (>= 20)")
    ap.add_argument("--windows", type=int, default=5, help="windows per runner (>= 5), alternating")
    ap.add_argument("--trace-iters", type=int, default=0,
                    help="after warm-up and capture, replay this many iterations of each runner and stop (kernel traces)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = _model(dev)
    for p in (("fp32", "fp16") if a.precision == "both" else (a.precision,)):
        print(json.dumps(_row(m, p, a, dev)), flush=True)


if __name__ == "__main__":
    main()

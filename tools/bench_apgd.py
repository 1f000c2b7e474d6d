"""APGD iteration against the fixed-step PGD iteration: APGDRunner's captured iteration next to AttackRunner's, same model,
shape and precision, in one process.

    python tools/bench_apgd.py                                   # UDEB4 256^2 bs 32, fp32 and fp16: one JSON line each
    python tools/bench_apgd.py --precision fp16 --norm l2
    python tools/bench_apgd.py --trace-iters 30                  # replays only, for `rocprofv3 --kernel-trace --stats -- python ...`

Both runners are warmed up (eager call, capturing call) and then timed window by window, alternating: a window is --iters
replays of the captured iteration from a fresh start point, ending in a device synchronise, on the host clock.  Reported per
precision: the median window of each per iteration, every window's spread, their difference, and the byte model of what an
APGD iteration adds behind the backward — ud_apgd_control (N-sized) and ud_apgd_update_linf: reads x, x_prev, x0, g and writes
x, x_prev (24 B per element), plus x_best, g_best written where a sample improved (+8 B) or read where it reset without
improving (+8 B); AttackRunner's ud_attack_step_linf moves 16 B per element.  `apgd_call_ms` is a whole APGDRunner call
(copy-in, `iters` replays, the closing forward, the merge) for orientation.  AttackRunner is unchanged by APGD, so its
column stands for the tree before it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

EPS = {"linf": 2.0 / 255.0, "l2": 0.5}
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable


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
    from unidefense_amd.attack import APGDRunner, AttackRunner
    bs, size, norm, eps = a.batch, a.size, a.norm, EPS[a.norm]
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    pgd = AttackRunner(m, bs, size, norm=norm, eps=eps, steps=a.iters, precision=precision)
    apgd = APGDRunner(m, bs, size, norm=norm, eps=eps, steps=a.iters, precision=precision)
    for _ in range(2):                       # the eager warm-up, then the capture
        pgd(x, y)
        apgd(x, y)

    def pgd_iters(n):
        pgd._start(x, y, None)
        for _ in range(n):
            pgd.graph.replay()

    def apgd_iters(n):
        apgd._start(0, None)
        for _ in range(n):
            apgd.graph.replay()
    if a.trace_iters:
        pgd_iters(a.trace_iters)
        apgd_iters(a.trace_iters)
        torch.cuda.synchronize(dev)
        return {"model": "UDEB4", "size": size, "batch": bs, "precision": precision, "norm": norm, "trace_iters": a.trace_iters,
                "warmup_iters": 2 * a.iters}
    tp, ta, tc = [], [], []
    for _ in range(a.windows):
        tp.append(_window(lambda: pgd_iters(a.iters), dev) / a.iters)
        ta.append(_window(lambda: apgd_iters(a.iters), dev) / a.iters)
    for _ in range(3):
        tc.append(_window(lambda: apgd(x, y), dev))
    total = bs * 3 * size * size
    mp, ma = statistics.median(tp), statistics.median(ta)
    row = {"model": "UDEB4", "size": size, "batch": bs, "precision": precision, "norm": norm, "iters_per_window": a.iters,
           "windows": a.windows, "pgd_ms_per_iter": round(mp, 3), "apgd_ms_per_iter": round(ma, 3),
           "apgd_minus_pgd_us": round((ma - mp) * 1e3, 1), "apgd_over_pgd": round(ma / mp, 4),
           "pgd_min_max_ms": [round(min(tp), 3), round(max(tp), 3)], "apgd_min_max_ms": [round(min(ta), 3), round(max(ta), 3)],
           "apgd_call_ms": round(statistics.median(tc), 2), "elements": total}
    if norm == "linf":
        row["update_bytes_min_max"] = [24 * total, 40 * total]
        row["update_ideal_us_at_5.5TBps"] = [round(24 * total / HBM_BPS * 1e6, 2), round(40 * total / HBM_BPS * 1e6, 2)]
        row["pgd_step_ideal_us_at_5.5TBps"] = round(16 * total / HBM_BPS * 1e6, 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default="both")
    ap.add_argument("--norm", choices=("linf", "l2"), default="linf")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
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

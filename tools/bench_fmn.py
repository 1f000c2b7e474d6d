"""FMN iteration against the fixed-step PGD iteration: FMNRunner's captured iteration (both norms) next to AttackRunner's
(PGD linf), same model, shape and precision, in one process; and the norm pass (ud_fmn_norm_parts) on its own.

    python tools/bench_fmn.py                                    # UDEB4 256^2 bs 32, fp32 and fp16: one JSON line each
    python tools/bench_fmn.py --precision fp16

The runners are warmed up (eager call, capturing call) and then timed window by window, alternating: a window is --iters
replays of the captured iteration from a fresh start point, ending in a device synchronise, on the host clock.  Reported per
precision: the median window of each per iteration, every window's spread, the differences, the launches an FMN iteration adds
behind the backward (linf: norm parts, control, update; l2: those plus ud_sample_sumsq's two and the projection), and the norm
pass alone — --norm-launches back-to-back launches between two events, 12 bytes per element (x, x0, g read once, nothing of
that size written).  The three tensors of the default shape are 75 MB together: they fit the last-level cache, so the figure
is what the pass achieves inside an iteration, where the backward has just written g, not a DRAM bandwidth.  AttackRunner is
unchanged by FMN, so its column stands for the tree before it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

LAUNCHES = {"linf": 3, "l2": 6}           # behind the backward; PGD linf: 1


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


def _norm_pass(x, g, launches):
    from unidefense_amd import kernels as K
    x0 = x.clone()
    for _ in range(5):
        K.fmn_norm_parts(x, x0, g)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        K.fmn_norm_parts(x, x0, g)
    end.record()
    end.synchronize()
    us = start.elapsed_time(end) * 1e3 / launches
    return us, 12.0 * x.numel() / (us * 1e-6) / 1e9


def _row(m, precision, a, dev):
    from unidefense_amd.attack import AttackRunner, FMNRunner
    bs, size = a.batch, a.size
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    pgd = AttackRunner(m, bs, size, norm="linf", eps=2.0 / 255.0, steps=a.iters, precision=precision)
    fmn = {norm: FMNRunner(m, bs, size, norm=norm, steps=a.iters, precision=precision) for norm in ("linf", "l2")}
    for _ in range(2):                       # the eager warm-up, then the capture
        pgd(x, y)
        for r in fmn.values():
            r(x, y)

    def pgd_iters(n):
        pgd._start(x, y, None)
        for _ in range(n):
            pgd.graph.replay()

    def fmn_iters(r, n):
        r._start(x, y)
        for _ in range(n):
            r.graph.replay()
    tp, tf = [], {"linf": [], "l2": []}
    for _ in range(a.windows):
        tp.append(_window(lambda: pgd_iters(a.iters), dev) / a.iters)
        for norm, r in fmn.items():
            tf[norm].append(_window(lambda: fmn_iters(r, a.iters), dev) / a.iters)
    mp = statistics.median(tp)
    row = {"model": "UDEB4", "size": size, "batch": bs, "precision": precision, "iters_per_window": a.iters, "windows": a.windows,
           "pgd_linf_ms_per_iter": round(mp, 3), "pgd_min_max_ms": [round(min(tp), 3), round(max(tp), 3)],
           "pgd_launches_behind_backward": 1, "elements": x.numel()}
    for norm in ("linf", "l2"):
        mf = statistics.median(tf[norm])
        row[f"fmn_{norm}_ms_per_iter"] = round(mf, 3)
        row[f"fmn_{norm}_min_max_ms"] = [round(min(tf[norm]), 3), round(max(tf[norm]), 3)]
        row[f"fmn_{norm}_minus_pgd_us"] = round((mf - mp) * 1e3, 1)
        row[f"fmn_{norm}_launches_behind_backward"] = LAUNCHES[norm]
    us, gbs = _norm_pass(x, fmn["linf"].g, a.norm_launches)
    row["norm_pass_us"], row["norm_pass_GBps_at_12B_per_element"] = round(us, 2), round(gbs, 1)
    row["found"] = {norm: int(r.found.sum()) for norm, r in fmn.items()}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default="both")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window (>= 20)")
    ap.add_argument("--windows", type=int, default=5, help="windows per runner (>= 5), alternating")
    ap.add_argument("--norm-launches", type=int, default=200, help="back-to-back launches of the norm pass between two events")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = _model(dev)
    for p in (("fp32", "fp16") if a.precision == "both" else (a.precision,)):
        print(json.dumps(_row(m, p, a, dev)), flush=True)


if __name__ == "__main__":
    main()

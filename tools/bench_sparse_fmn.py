"""Sparse FMN iteration split: what ud_sfmn_select + ud_sfmn_apply cost inside SparseFMNRunner's captured iteration, next to
the same runner's forward + backward and to FMNRunner's L2 iteration, same model, shape and precision, in one process.

    python tools/bench_sparse_fmn.py                     # UDEB4 256^2, bs 32 and bs 2, fp32: one JSON line each
    python tools/bench_sparse_fmn.py --batch 32 --precision fp16

Per batch size: the runners (FMN l2, sparse l1, sparse l0) are warmed up (eager call, capturing call) and timed window by
window, alternating, as tools/bench_fmn.py does: a window is --iters replays of the captured iteration from a fresh start point,
ending in a device synchronise, on the host clock.  Then, on the buffers the sparse runner's last iteration left (its own x, x0,
g, eps and fac: the budgets of a real run, not made-up ones), --launches back-to-back launches between two events of each
kernel that follows the backward: norm parts, control, select, apply.  forward + backward is the iteration minus those four.
The l1 select is timed twice more on made-up budgets (0.3 and 0.02 of each sample's sum |z - x0|) that make every sample run the
threshold descent, which the run's own budgets need not do.
The alpha_init values are the suite's (8 for l1, 256 for l0), so that the projections do project."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

ALPHA = {"l1": 8.0, "l0": 256.0}


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


def _timed(fn, launches):
    for _ in range(3):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / launches


def _kernels(r, launches):
    """us per launch of the four kernels behind the backward, on the runner's own buffers after its last replayed iteration;
    apply runs on copies of x and x_adv (it writes them), control on a counter row set back before every launch"""
    from unidefense_amd import kernels as K
    g = r.g.contiguous()
    x, xb = r.x.detach().clone(), r.x_adv.clone()
    f = r.history[0].clone()
    thr = r._thr.clone()

    def control():
        r._k.zero_()
        r._control(f)
    eps, fac = r.fst[K.SFMN_F["eps"]].clone(), r._fac.clone()
    out = {"norm_parts_us": _timed(lambda: K.sfmn_norm_parts(x, r.x0, g, ws=r._ws), launches),
           "control_us": _timed(control, launches)}
    r.fst[K.SFMN_F["eps"]].copy_(eps)                      # the budgets and steps of the run, not what the timing loop left
    r._fac.copy_(fac)
    out["select_us"] = _timed(lambda: K.sfmn_select(x, r.x0, g, r.fst, r._fac, thr, r.norm), launches)
    if r.norm == "l1":
        # the run's own budgets may project nothing (eps = 0: answered without a descent; eps above sum |z - x0|: one pass), so
        # the descent is also timed on made-up budgets that make every sample project: 0.3 and 0.02 of its sum |z - x0|
        a_sum = (x.double() - g.double() * r._fac.reshape(-1, 1, 1, 1) - r.x0.double()).abs().flatten(1).sum(1)
        for name, share in (("select_projecting_0.3_us", 0.3), ("select_projecting_0.02_us", 0.02)):
            r.fst[K.SFMN_F["eps"]].copy_((a_sum * share).float())
            out[name] = _timed(lambda: K.sfmn_select(x, r.x0, g, r.fst, r._fac, thr.clone(), r.norm), launches)
        r.fst[K.SFMN_F["eps"]].copy_(eps)
    out["apply_us"] = _timed(lambda: K.sfmn_apply(x.clone(), xb, r.x0, g, r.ist, r._fac, thr, r.norm, r.lo, r.hi), launches)
    out["clone_us"] = _timed(lambda: x.clone(), launches)
    out["apply_us"] -= out["clone_us"]
    out["projected_samples"] = int((thr >= 0).sum())
    return {k: (round(v, 2) if isinstance(v, float) else v) for k, v in out.items()}


def _row(m, bs, a, dev):
    from unidefense_amd.attack import FMNRunner, SparseFMNRunner
    size = a.size
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    runners = {"fmn_l2": FMNRunner(m, bs, size, norm="l2", steps=a.iters, precision=a.precision)}
    for norm in ("l1", "l0"):
        runners[f"sparse_{norm}"] = SparseFMNRunner(m, bs, size, norm=norm, steps=a.iters, alpha_init=ALPHA[norm],
                                                    precision=a.precision)
    for _ in range(2):                       # the eager warm-up, then the capture
        for r in runners.values():
            r(x, y)

    def iters(r, n):
        r._start(x, y)
        for _ in range(n):
            r.graph.replay()
    t = {k: [] for k in runners}
    for _ in range(a.windows):
        for k, r in runners.items():
            t[k].append(_window(lambda: iters(r, a.iters), dev) / a.iters)
    row = {"model": "UDEB4", "size": size, "batch": bs, "precision": a.precision, "iters_per_window": a.iters, "windows": a.windows,
           "elements_per_sample": 3 * size * size}
    for k in runners:
        row[f"{k}_ms_per_iter"] = round(statistics.median(t[k]), 3)
        row[f"{k}_min_max_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    for norm in ("l1", "l0"):
        r = runners[f"sparse_{norm}"]
        kern = _kernels(r, a.launches)
        behind = kern["norm_parts_us"] + kern["control_us"] + kern["select_us"] + kern["apply_us"]
        it = row[f"sparse_{norm}_ms_per_iter"] * 1e3
        row[f"sparse_{norm}_kernels"] = kern
        row[f"sparse_{norm}_forward_backward_ms"] = round((it - behind) / 1e3, 3)
        row[f"sparse_{norm}_select_apply_share"] = round((kern["select_us"] + kern["apply_us"]) / it, 4)
        if norm == "l1":                     # had every sample projected: the share of the slower made-up budget
            slow = max(kern["select_projecting_0.3_us"], kern["select_projecting_0.02_us"])
            row["sparse_l1_select_apply_share_projecting"] = round((slow + kern["apply_us"]) / (it - kern["select_us"] + slow), 4)
        row[f"sparse_{norm}_found"] = int(r.found.sum())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 2])
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window")
    ap.add_argument("--windows", type=int, default=5, help="windows per runner, alternating")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches of each kernel between two events")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = _model(dev)
    for bs in a.batch:
        print(json.dumps(_row(m, bs, a, dev)), flush=True)


if __name__ == "__main__":
    main()

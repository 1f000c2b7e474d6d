"""Attack iteration: the AttackRunner's graph replay against the loop a user would write without it, and the four kernels
of csrc/attack.hip on their own.

    python tools/bench_attack.py                         # one JSON line per row: per-iteration times of both loops
    python tools/bench_attack.py --kernels --rows UDEB4  # the four kernels at the row's shape (run it under
                                                         # `rocprofv3 --kernel-trace --stats -- python ...` for kernel times)

Rows (those of tools/bench_input_grad.py): UDEB4 256^2 bs 32, UDR50 320^2 bs 16, UDR18 256^2 bs 32.  Both loops run the same
L-infinity PGD iteration (summed cross-entropy, eps 2/255, step 1/255) on the same frozen eval-mode model in one process,
alternating window by window; a window is --iters iterations ending in a device synchronise, timed on the host clock (the
eager loop's cost includes its host gaps).  Reported: the median window of each, their ratio and the windows' spread.
  runner : AttackRunner(steps=iters)(x, y) — the copy-in and `iters` replays of the captured iteration
  eager  : autograd.grad of the objective on the frozen model, then torch sign / add / max / min / clamp / copy_

    python tools/bench_attack.py --precision both [--size 380 --batch 32]   # UDEB4: the fp16 runner against the fp32 runner
    python tools/bench_attack.py --precision fp16 --trace-iters 30          # replays only, for a rocprofv3 kernel trace

--precision fp16 / both (UDEB4 only): the captured iteration of AttackRunner(precision=...) — with `both` the two runners' windows
alternate in one process and the row reports the median of the --windows windows of each, their ratio and every window's spread."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

ROWS = (("UDEB4", 256, 32), ("UDR50", 320, 16), ("UDR18", 256, 32))
EPS, STEP, LO, HI = 2.0 / 255.0, 1.0 / 255.0, -1.0, 1.0
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable


def _model(name, dev):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    m = load_model(name)(num_classes=2, drop_rate=0.5, **kw)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev).eval()


def _eager_loop(m, x, y, iters):
    """what a user writes without the runner: returns a function running `iters` iterations from x"""
    from unidefense_amd.attack import cross_entropy_sum, frozen
    xa = x.clone().requires_grad_()
    lo_b, hi_b = x - EPS, x + EPS

    def run():
        with torch.no_grad():
            xa.copy_(x)
        with frozen(m):
            for _ in range(iters):
                g, = torch.autograd.grad(cross_entropy_sum(m(xa), y), xa)
                with torch.no_grad():
                    v = torch.add(xa, torch.sign(g), alpha=STEP)
                    xa.copy_(torch.clamp(torch.min(torch.max(v, lo_b), hi_b), LO, HI))
        return xa
    return run


def _window(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def _row(name, size, bs, a, dev):
    from unidefense_amd.attack import AttackRunner
    m = _model(name, dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    runner = AttackRunner(m, bs, size, norm="linf", eps=EPS, steps=a.iters, step=STEP)
    eager = _eager_loop(m, x, y, a.iters)
    for _ in range(2):                       # warm-up of both (the runner's second call captures)
        runner(x, y)
        eager()
    tr, te = [], []
    for _ in range(a.windows):
        tr.append(_window(lambda: runner(x, y), dev) / a.iters)
        te.append(_window(eager, dev) / a.iters)
    med_r, med_e = statistics.median(tr), statistics.median(te)
    d = float((runner(x, y) - eager()).abs().max())
    return {"model": name, "size": size, "batch": bs, "iters_per_window": a.iters, "windows": a.windows,
            "runner_ms_per_iter": round(med_r, 3), "eager_ms_per_iter": round(med_e, 3), "runner_over_eager": round(med_r / med_e, 4),
            "runner_min_max_ms": [round(min(tr), 3), round(max(tr), 3)], "eager_min_max_ms": [round(min(te), 3), round(max(te), 3)],
            "max_abs_diff_x_adv": d}


def _row_precision(size, bs, a, dev):
    """UDEB4: per-iteration time of the fp16 and / or the fp32 AttackRunner, windows alternating"""
    from unidefense_amd.attack import AttackRunner
    m = _model("UDEB4", dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    precs = ("fp32", "fp16") if a.precision == "both" else (a.precision,)
    runners = {p: AttackRunner(m, bs, size, norm="linf", eps=EPS, steps=a.iters, step=STEP, precision=p) for p in precs}
    for _ in range(2):                       # the eager warm-up, then the capture
        for r in runners.values():
            r(x, y)
    if a.trace_iters:
        for r in runners.values():
            r.steps = a.trace_iters          # replays of the captured iteration only
            r(x, y)
        torch.cuda.synchronize(dev)
        return {"model": "UDEB4", "size": size, "batch": bs, "trace_iters": a.trace_iters, "precision": list(precs),
                "warmup_iters": 2 * a.iters}
    t = {p: [] for p in precs}
    for _ in range(a.windows):
        for p, r in runners.items():
            t[p].append(_window(lambda: r(x, y), dev) / a.iters)
    row = {"model": "UDEB4", "size": size, "batch": bs, "iters_per_window": a.iters, "windows": a.windows}
    for p in precs:
        row[f"{p}_ms_per_iter"] = round(statistics.median(t[p]), 3)
        row[f"{p}_min_max_ms"] = [round(min(t[p]), 3), round(max(t[p]), 3)]
    if len(precs) == 2:
        row["fp32_over_fp16"] = round(statistics.median(t["fp32"]) / statistics.median(t["fp16"]), 4)
        row["linf_x_adv_fp16_vs_fp32"] = float((runners["fp16"](x, y) - runners["fp32"](x, y)).abs().max())
    return row


def _kernels(name, size, bs, a, dev):
    """the four kernels at the row's shape: bytes moved, bytes / 5.5 TB/s, and the time per launch from HIP events over
    --reps back-to-back launches (kernel times proper come from a rocprofv3 run of this mode)"""
    from unidefense_amd import kernels as K
    gen = torch.Generator().manual_seed(1)
    shape = (bs, 3, size, size)
    total = bs * 3 * size * size
    x0 = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
    xa = (x0 + 0.01 * torch.randn(shape, generator=gen).to(dev)).contiguous()
    g = torch.randn(shape, generator=gen).to(dev)
    ss = torch.empty(bs, dtype=torch.float64, device=dev)
    ws = torch.empty(max(K.sample_sumsq_ws_bytes(bs, 3 * size * size) // 8, 1), dtype=torch.float64, device=dev)
    K.sample_sumsq(g, None, out=ss, ws=ws)
    cases = (("ud_attack_step_linf", 16, lambda: K.attack_step_linf(xa, x0, g, STEP, EPS, LO, HI)),
             ("ud_sample_sumsq(a)", 4, lambda: K.sample_sumsq(g, None, out=ss, ws=ws)),
             ("ud_sample_sumsq(a, b)", 8, lambda: K.sample_sumsq(xa, x0, out=ss, ws=ws)),
             ("ud_attack_step_l2", 12, lambda: K.attack_step_l2(xa, g, ss, 1e-3)),
             ("ud_attack_project_l2", 12, lambda: K.attack_project_l2(xa, x0, ss, 0.5, LO, HI)))
    out = {"model": name, "size": size, "batch": bs, "elements": total, "reps": a.reps, "kernels": {}}
    for label, bpe, fn in cases:
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        out["kernels"][label] = {"bytes": bpe * total, "ideal_us_at_5.5TBps": round(bpe * total / HBM_BPS * 1e6, 2),
                                 "event_us_per_call": round(e0.elapsed_time(e1) * 1e3 / a.reps, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="UDEB4,UDR50,UDR18")
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window (>= 20)")
    ap.add_argument("--windows", type=int, default=5, help="windows per loop (>= 5), alternating")
    ap.add_argument("--kernels", action="store_true", help="launch the four kernels of csrc/attack.hip only")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default=None,
                    help="UDEB4: time AttackRunner(precision=...); both: the two runners' windows alternate in one process")
    ap.add_argument("--size", type=int, default=256, help="with --precision: the input side")
    ap.add_argument("--batch", type=int, default=32, help="with --precision: the batch size")
    ap.add_argument("--trace-iters", type=int, default=0,
                    help="with --precision: after warm-up and capture, replay this many iterations and stop (kernel traces)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.precision is not None:
        print(json.dumps(_row_precision(a.size, a.batch, a, dev)), flush=True)
        return
    for name, size, bs in ROWS:
        if name not in a.rows.split(","):
            continue
        row = (_kernels if a.kernels else _row)(name, size, bs, a, dev)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

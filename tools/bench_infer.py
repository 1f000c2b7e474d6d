"""Inference throughput: the eager eval forward (model.eval()(x) under no_grad) against the graph-captured InferenceRunner
(unidefense_amd/infer.py), in one process on one GPU.  Per row: ms per batch and img/s of both paths (median of --reps timed
windows of --steps calls each, after --warmup untimed calls).  Launch counts and per-kernel times come from a run under
rocprofv3 --kernel-trace --stats with --runner-only / --eager-only (profiles/r07/infer.txt).

  python tools/bench_infer.py                       # the four rows below
  python tools/bench_infer.py --rows udeb4-256-96 --runner-only --steps 20    # e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROWS = {"udeb4-256-64": ("UDEB4", 256, 64), "udeb4-256-96": ("UDEB4", 256, 96), "udeb4-380-96": ("UDEB4", 380, 96),
        "udr50-320-64": ("UDR50", 320, 64)}


def _model(name):
    from oracle import param_fill
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    m = load_model(name)(num_classes=2, drop_rate=0.5, **kw)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)          # non-trivial running statistics
    return m.cuda().eval()


def _time(fn, steps, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runner-only", action="store_true", help="skip the eager timing (profiling runs)")
    ap.add_argument("--eager-only", action="store_true", help="skip the runner (profiling runs)")
    args = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    for key in args.rows.split(","):
        name, size, bs = ROWS[key]
        torch.manual_seed(0)
        m = _model(name)
        x = torch.randn(bs, 3, size, size, device="cuda").clamp_(-1, 1)
        row = {"row": key, "model": name, "size": size, "batch": bs, "device": dev}
        if not args.runner_only:
            with torch.no_grad():
                t = _time(lambda: m(x), args.steps, args.warmup, args.reps)
            row.update(eager_ms=round(t, 3), eager_img_s=round(bs * 1000.0 / t, 1))
        if args.eager_only:
            print(json.dumps(row), flush=True)
            continue
        r = m.inference_runner(bs, size)
        r(x)                                   # eager warm-up
        r(x)                                   # capture + first replay
        t = _time(lambda: r(x), args.steps, args.warmup, args.reps)
        row.update(runner_ms=round(t, 3), runner_img_s=round(bs * 1000.0 / t, 1))
        if "eager_ms" in row:
            row["speedup"] = round(row["eager_ms"] / t, 3)
        print(json.dumps(row), flush=True)
        del r, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

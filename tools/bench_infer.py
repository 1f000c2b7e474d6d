"""Inference throughput: the eager eval forward (model.eval()(x) under no_grad) against the graph-captured InferenceRunner
(unidefense_amd/infer.py), in one process on one GPU.  Per row: ms per batch and img/s of both paths (median of --reps timed
windows of --steps calls each, after --warmup untimed calls).  Launch counts and per-kernel times come from a run under
rocprofv3 --kernel-trace --stats with --runner-only / --eager-only (profiles/r07/infer.txt).
--precision fp32 | fp16 | both: which runners a row times (fp16: UDEB4 only; the UDR50 row keeps fp32); with both, the two
runners' windows are taken alternately in the same process (profiles/r08/infer_fp16.txt).
--ab-node-h: the fp16 runner captured three times, UniDefenseModelEb4.EVAL_NODE_H_MAX_CIN = 0 (composed half kernels only), 32
(the half-storage eval node on block group 1) and 448 (also on the last group), timed alternately.

  python tools/bench_infer.py                       # the four rows below
  python tools/bench_infer.py --rows udeb4-256-96 --runner-only --steps 20    # e.g. under rocprofv3 --kernel-trace --stats
  python tools/bench_infer.py --rows udeb4-256-64,udeb4-256-96,udeb4-380-96 --precision both --runner-only
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


def _window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _time_alternating(fns, steps, warmup, reps):
    """median ms per call of each fn, its windows interleaved with the others' (box drift hits all of them alike)"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(_window(fn, steps))
    return [sorted(v)[len(v) // 2] for v in ms]


def _time(fn, steps, warmup, reps):
    return _time_alternating([fn], steps, warmup, reps)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runner-only", action="store_true", help="skip the eager timing (profiling runs)")
    ap.add_argument("--eager-only", action="store_true", help="skip the runner (profiling runs)")
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default="fp32", help="the runner(s) a row times")
    ap.add_argument("--ab-node-h", action="store_true", help="A/B of the half-storage eval node's block groups (fp16 runner)")
    args = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    for key in args.rows.split(","):
        name, size, bs = ROWS[key]
        torch.manual_seed(0)
        m = _model(name)
        x = torch.randn(bs, 3, size, size, device="cuda").clamp_(-1, 1)
        row = {"row": key, "model": name, "size": size, "batch": bs, "device": dev}
        if args.ab_node_h:
            from unidefense_amd.infer import InferenceRunner
            cls, keep, runners = type(m), type(m).EVAL_NODE_H_MAX_CIN, {}
            try:
                for cin in (0, 32, 448):
                    cls.EVAL_NODE_H_MAX_CIN = cin          # read while the runner warms up and captures
                    r = InferenceRunner(m, bs, size, "fp16")
                    r(x)
                    r(x)
                    runners[cin] = r
            finally:
                cls.EVAL_NODE_H_MAX_CIN = keep
            ts = _time_alternating([lambda r=r: r(x) for r in runners.values()], args.steps, args.warmup, args.reps)
            row.update({f"fp16_node_max_cin_{cin}_ms": round(t, 3) for cin, t in zip(runners, ts)})
            print(json.dumps(row), flush=True)
            del runners, r, m
            torch.cuda.empty_cache()
            continue
        if not args.runner_only:
            with torch.no_grad():
                t = _time(lambda: m(x), args.steps, args.warmup, args.reps)
            row.update(eager_ms=round(t, 3), eager_img_s=round(bs * 1000.0 / t, 1))
        if args.eager_only:
            print(json.dumps(row), flush=True)
            continue
        precs = {"fp32": ["fp32"], "fp16": ["fp16"], "both": ["fp32", "fp16"]}[args.precision]
        if name != "UDEB4":
            precs = ["fp32"]
        runners = []
        for prec in precs:
            r = m.inference_runner(bs, size, prec)
            r(x)                                   # eager warm-up
            r(x)                                   # capture + first replay
            runners.append(r)
        ts = _time_alternating([lambda r=r: r(x) for r in runners], args.steps, args.warmup, args.reps)
        for prec, t in zip(precs, ts):
            tag = "runner" if prec == "fp32" else "runner_fp16"
            row.update({f"{tag}_ms": round(t, 3), f"{tag}_img_s": round(bs * 1000.0 / t, 1)})
        if "eager_ms" in row and "runner_ms" in row:
            row["speedup"] = round(row["eager_ms"] / row["runner_ms"], 3)
        if "runner_ms" in row and "runner_fp16_ms" in row:
            row["fp16_speedup"] = round(row["runner_ms"] / row["runner_fp16_ms"], 3)
        print(json.dumps(row), flush=True)
        del runners, r, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

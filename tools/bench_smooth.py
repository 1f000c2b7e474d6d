"""Randomized smoothing: CertifyRunner's captured draw next to InferenceRunner's replay at the same model and batch, and the
noise kernel of csrc/smooth.hip on its own.

    python tools/bench_smooth.py                         # one JSON line per row: ms per draw, ms per forward, draws per second
    python tools/bench_smooth.py --kernels               # ud_smooth_noise alone, both modes: us per launch, GB/s of x read + out written

Rows: UDEB4 256^2 bs 96 fp32 and fp16, UDEB4 380^2 bs 96 fp32.  Both runners replay their graph on the same eval-mode model in
one process, alternating window by window; a window is --iters replays ending in a device synchronise, timed on the host clock
(the certificate's host tail, one read and the Clopper-Pearson bisection, is timed apart as tail_ms).  The draw is the forward
plus ud_smooth_noise, the logits copy and ud_smooth_vote: the difference is what the certificate costs per draw.

--kernels: the launch is timed inside a captured graph of --launches launches that rotate over enough (x, out) pairs to exceed
the 256 MB Infinity Cache, HIP events around --reps replays; the draw counter differs per launch."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

ROWS = (("UDEB4", 256, 96, "fp32"), ("UDEB4", 256, 96, "fp16"), ("UDEB4", 380, 96, "fp32"))
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable
LAUNCH_US = 4.5
CACHE_BYTES = 256 << 20


def _model(name, dev):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    m = load_model(name)(num_classes=2, drop_rate=0.5, **kw)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev).eval()


def _window(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def _row(name, size, bs, precision, a, dev):
    from unidefense_amd.infer import InferenceRunner
    from unidefense_amd.smooth import CertifyRunner
    m = _model(name, dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    infer = InferenceRunner(m, bs, size, precision)
    row = {"model": name, "size": size, "batch": bs, "precision": precision, "iters_per_window": a.iters, "windows": a.windows}
    runners = {noise: CertifyRunner(m, bs, size, sigma=0.25, noise=noise, n0=1, n=a.iters - 1, precision=precision)
               for noise in a.noises.split(",")}
    for _ in range(2):                       # the eager warm-up, then the capture
        infer(x)
        for r in runners.values():
            r(x)

    def draws(r):
        r.ist.zero_()
        r._counts.zero_()
        for _ in range(a.iters):
            r.graph.replay()

    def forwards():
        for _ in range(a.iters):
            infer.graph.replay()

    t = {k: [] for k in ("infer", *runners)}
    for _ in range(a.windows):
        t["infer"].append(_window(forwards, dev) / a.iters)
        for k, r in runners.items():
            t[k].append(_window(lambda: draws(r), dev) / a.iters)
    fwd = statistics.median(t["infer"])
    row["infer_ms"], row["infer_min_max_ms"] = round(fwd, 3), [round(min(t["infer"]), 3), round(max(t["infer"]), 3)]
    for k, r in runners.items():
        d = statistics.median(t[k])
        t0 = time.perf_counter()
        r._tail()
        row[k] = {"draw_ms": round(d, 3), "min_max_ms": [round(min(t[k]), 3), round(max(t[k]), 3)], "over_forward": round(d / fwd, 4),
                  "extra_us": round((d - fwd) * 1e3, 1), "draws_per_s": round(1e3 / d, 2), "img_per_s": round(bs * 1e3 / d, 1),
                  "tail_ms": round((time.perf_counter() - t0) * 1e3, 2)}
    per = 3 * size * size
    row["model_us"] = round(8 * bs * per / HBM_BPS * 1e6 + 2 * LAUNCH_US, 1)       # the noise pass's bytes + two launches
    return row


def _kernels(name, size, bs, precision, a, dev):
    from unidefense_amd import kernels as K
    per = 3 * size * size
    nbytes = 8 * bs * per
    pairs = max(2, -(-2 * CACHE_BYTES // nbytes))
    gen = torch.Generator().manual_seed(1)
    xs = [(torch.rand(bs, per, generator=gen) * 2 - 1).to(dev) for _ in range(pairs)]
    outs = [torch.empty_like(xs[0]) for _ in range(pairs)]
    ids = torch.arange(bs, dtype=torch.int64, device=dev)
    k = torch.zeros(bs, dtype=torch.int32, device=dev)
    out = {"size": size, "batch": bs, "per": per, "bytes": nbytes, "ideal_us_at_5.5TBps": round(nbytes / HBM_BPS * 1e6, 2),
           "pairs": pairs, "launches": a.launches, "reps": a.reps, "modes": {}}
    for mode in ("uniform", "gaussian"):
        def body():
            for i in range(a.launches):
                K.smooth_noise(xs[i % pairs], outs[i % pairs], ids, k, i, mode, 0.25, 7)
        body()
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        g.replay()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        us = statistics.median(times)
        out["modes"][mode] = {"us_per_launch": round(us, 2), "min_max_us": [round(min(times), 2), round(max(times), 2)],
                              "GBps": round(nbytes / us * 1e-3, 1), "Gelem_per_s": round(bs * per / us * 1e-3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="0,1,2", help="indices into ROWS")
    ap.add_argument("--noises", default="gaussian,uniform")
    ap.add_argument("--iters", type=int, default=20, help="replays per timed window")
    ap.add_argument("--windows", type=int, default=5, help="windows per runner, alternating")
    ap.add_argument("--kernels", action="store_true", help="ud_smooth_noise only")
    ap.add_argument("--launches", type=int, default=16, help="with --kernels: launches per captured graph")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    seen = set()
    for i in (int(v) for v in a.rows.split(",")):
        name, size, bs, precision = ROWS[i]
        if a.kernels and (size, bs) in seen:
            continue
        seen.add((size, bs))
        row = (_kernels if a.kernels else _row)(name, size, bs, precision, a, dev)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

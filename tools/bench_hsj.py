"""HopSkipJump (unidefense_amd/hsj.py): what a query costs on top of the forward, what the gradient estimate costs next to the
forwards it serves, and its radii next to FMN's.

    python tools/bench_hsj.py                  # one JSON line per row
    python tools/bench_hsj.py --parts queries  # queries | estimate | radii

queries : UDEB4 256^2 bs 96, fp32 and fp16: HSJRunner's captured query graphs (bisect, probe, step) next to InferenceRunner's
          replay on the same model in one process, alternating window by window (a window: --iters replays, one synchronise,
          host clock).  Every sample is live (a hook on the input's mean decides, so that the propose passes do their work).
estimate: ud_hsj_estimate alone at N 96, D = 3 x 256^2, B = 100 and 1000, both norms: HIP events around each launch.
radii   : UDR18 128^2 N 8: median radius of HSJ (steps 8, probes 50, bisect 16) and of FMN (100 steps) on the same batch."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402
from tools.bench_smooth import _model, _window  # noqa: E402


def _queries(precision, a, dev):
    from unidefense_amd import kernels as K
    from unidefense_amd.hsj import HSJRunner
    from unidefense_amd.infer import InferenceRunner
    bs, size = 96, 256
    m = _model("UDEB4", dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = torch.zeros(bs, dtype=torch.int64, device=dev)
    infer = InferenceRunner(m, bs, size, precision)
    row = {"part": "queries", "model": "UDEB4", "size": size, "batch": bs, "precision": precision, "iters_per_window": a.iters}

    def decide(out, xt):                                         # class 1 where the image's mean is above 0.25: x is 0, ones is 1
        mean = xt.mean((1, 2, 3))
        return torch.stack([0.25 - mean, mean - 0.25], 1)
    runners = {norm: HSJRunner(m, bs, size, norm=norm, steps=1, probes=2, max_probes=1000, bisect=2, halvings=2, init_trials=1,
                               precision=precision, logits=decide) for norm in ("l2", "linf")}
    for _ in range(2):                                           # the eager warm-up, then the capture
        infer(x)
        for r in runners.values():
            r(x, y, None, torch.ones_like(x))
    t = {"infer": []}
    kinds = [(norm, kind) for norm in runners for kind in ("bisect", "probe", "step")]
    for _ in range(a.windows):
        t["infer"].append(_window(lambda: [infer.graph.replay() for _ in range(a.iters)], dev) / a.iters)
        for norm, kind in kinds:
            r = runners[norm]
            # STEPDONE back to 0 once per window: the step pass does its work until the window's first accepted step, then
            # leaves early, so the "step" row understates a searching step query (the probe row is the like-for-like pass)
            r.ist[K.HSJ_I["stepdone"]].zero_()
            t.setdefault(f"{norm}_{kind}", []).append(_window(lambda: [r.graphs[kind].replay() for _ in range(a.iters)], dev) / a.iters)
    fwd = statistics.median(t["infer"])
    row["infer_ms"] = round(fwd, 3)
    for k, v in t.items():
        if k != "infer":
            d = statistics.median(v)
            row[k] = {"query_ms": round(d, 3), "over_forward": round(d / fwd, 4), "extra_us": round((d - fwd) * 1e3, 1),
                      "queries_per_s": round(1e3 / d, 2)}
    row["live"] = {norm: int((r.ist[0] * r.ist[1]).sum()) for norm, r in runners.items()}
    return row, fwd


def _estimate(fwd_ms, a, dev):
    from unidefense_amd import kernels as K
    N, per = 96, 3 * 256 * 256
    v = torch.empty(N, per, device=dev)
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    phi = torch.randint(0, 2, (1000, N), dtype=torch.int8, device=dev)
    rows = []
    for norm in ("linf", "l2"):
        for B in (100, 1000):
            K.hsj_estimate(v, phi, ids, B, 0, norm, 1)
            torch.cuda.synchronize(dev)
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                K.hsj_estimate(v, phi, ids, B, 0, norm, 1)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            ms = statistics.median(times)
            quads = N * per / 4 * B
            rows.append({"part": "estimate", "norm": norm, "B": B, "N": N, "per": per, "ms": round(ms, 3),
                         "min_max_ms": [round(min(times), 3), round(max(times), 3)], "Gquad_draws_per_s": round(quads / ms * 1e-6, 2),
                         "B_forwards_ms": None if fwd_ms is None else round(B * fwd_ms, 1),
                         "share_of_B_forwards": None if fwd_ms is None else round(ms / (B * fwd_ms), 5)})
    return rows


def _radii(dev):
    from unidefense_amd.hsj import HSJRunner
    from unidefense_amd.infer import _eval_nodes
    n, size = 8, 128
    m = _model("UDR18", dev)
    x = param_fill.make_input(n, size, 5).to(dev)

    def label(t):
        with torch.no_grad(), _eval_nodes(m, False):
            return m(t)["cls_out"].float().argmax(1)
    y = label(x)
    x_init, have = x.clone(), torch.zeros(n, dtype=torch.bool, device=dev)
    for cand in [param_fill.make_input(n, size, s).to(dev) for s in (6, 7, 8)] + [torch.full_like(x, v) for v in (-1.0, 1.0, 0.0)]:
        take = (label(cand) != y) & ~have
        x_init[take] = cand[take]
        have |= take
    row = {"part": "radii", "model": "UDR18", "size": size, "batch": n, "start_known": int(have.sum())}
    for norm in ("l2", "linf"):
        r = HSJRunner(m, n, size, norm=norm, steps=8, probes=50, bisect=16)
        t0 = time.perf_counter()
        radius = r(x, y, None, x_init).double().cpu()
        torch.cuda.synchronize(dev)
        f = m.fmn_runner(n, size, norm=norm)
        f(x, y)
        fr = f.radius.double().cpu()
        row[norm] = {"hsj_median": float(radius.median()), "hsj_found": int(r.found.sum()), "hsj_queries": r.queries_of(True),
                     "hsj_eager_s": round(time.perf_counter() - t0, 1), "fmn_median": float(fr.median()),
                     "fmn_found": int(f.found.sum()), "hsj": [round(float(v), 4) for v in radius], "fmn": [round(float(v), 4) for v in fr]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="queries,estimate,radii")
    ap.add_argument("--iters", type=int, default=10, help="replays per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    fwd = None
    if "queries" in parts:
        for precision in ("fp32", "fp16"):
            row, f = _queries(precision, a, dev)
            fwd = f if precision == "fp32" else fwd
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if "estimate" in parts:
        for row in _estimate(fwd, a, dev):
            print(json.dumps(row), flush=True)
    if "radii" in parts:
        print(json.dumps(_radii(dev)), flush=True)


if __name__ == "__main__":
    main()

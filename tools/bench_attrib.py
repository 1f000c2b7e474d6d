"""Attribution: AttributionRunner's captured iteration next to InputGradRunner's replay at the same model, batch and score, the
DeletionRunner's captured query next to InferenceRunner's replay, and the element-wise passes of csrc/attrib.hip on their own.

    python tools/bench_attrib.py                         # one JSON line per row

Rows: UDEB4 256^2 at bs 32 and bs 96, fp32 and fp16.  All runners replay their graphs on the same eval-mode model in one
process, alternating window by window; a window is --iters replays ending in a device synchronise, timed on the host clock.  The
iteration is the forward + d/dx plus ud_attr_point, ud_attr_accumulate, the score's copy and ud_attr_control; the query is the
forward plus ud_attr_mask, the softmax and ud_attr_control: the differences are what the path integral and the curve cost.
"passes": the iteration's three kernels (point, accumulate, control) alone in a captured graph of their own, HIP events around
--reps replays, next to the bytes they move (x, b read and xp written; g read, acc read and written: 32 bytes per element)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

ROWS = (("UDEB4", 256, 32, "fp32"), ("UDEB4", 256, 32, "fp16"), ("UDEB4", 256, 96, "fp32"), ("UDEB4", 256, 96, "fp16"))
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable


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


def _stats(ts):
    return {"ms": round(statistics.median(ts), 3), "min_max_ms": [round(min(ts), 3), round(max(ts), 3)]}


def _passes(r, a, dev):
    """the iteration's element-wise kernels alone, on the runner's own buffers"""
    from unidefense_amd import kernels as K
    g = r.g.contiguous()
    f = r.f_x

    def body():
        for _ in range(a.launches):
            K.attr_point(r.x0, r.b, r.xp, r._k, r._alpha, r.iters)
            K.attr_accumulate(g, r.acc, r._k, r._w, r.iters)
            K.attr_control(f, r.ist, r.path)
            r.ist.zero_()
    body()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    graph.replay()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    nbytes = 32 * r.x0.numel()
    return {"us_per_iteration": round(statistics.median(times), 2), "min_max_us": [round(min(times), 2), round(max(times), 2)],
            "bytes": nbytes, "ideal_us_at_5.5TBps": round(nbytes / HBM_BPS * 1e6, 2)}


def _row(name, size, bs, precision, a, dev):
    from unidefense_amd.attack import InputGradRunner, margin_each
    from unidefense_amd.attrib import AttributionRunner, DeletionRunner
    from unidefense_amd.infer import InferenceRunner
    m = _model(name, dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    heat = torch.rand(bs, size, size, generator=torch.Generator().manual_seed(1)).to(dev)
    grad = InputGradRunner(m, bs, size, objective=lambda out, yy: margin_each(out, yy).sum(), precision=precision)
    attr = AttributionRunner(m, bs, size, steps=a.iters, precision=precision)
    infer = InferenceRunner(m, bs, size, precision)
    curve = DeletionRunner(m, bs, size, fractions=tuple(i / (a.iters - 1) for i in range(a.iters)), precision=precision)
    for _ in range(2):                       # the eager warm-up, then the capture
        grad(x, y)
        attr(x, y)
        infer(x)
        curve(x, y, heat)

    def replays(graph, counters):
        def run():
            counters.zero_()
            for _ in range(a.iters):
                graph.replay()
        return run

    runs = {"input_grad": replays(grad.graph, attr.ist), "attribution": replays(attr.graph, attr.ist),
            "infer": replays(infer.graph, curve.ist), "deletion": replays(curve.graph, curve.ist)}
    t = {k: [] for k in runs}
    for _ in range(a.windows):
        for k, run in runs.items():
            t[k].append(_window(run, dev) / a.iters)
    row = {"model": name, "size": size, "batch": bs, "precision": precision, "iters_per_window": a.iters, "windows": a.windows}
    row.update({k: _stats(v) for k, v in t.items()})
    for mine, base in (("attribution", "input_grad"), ("deletion", "infer")):
        d, f = row[mine]["ms"], row[base]["ms"]
        row[mine].update(over_base=round(d / f, 4), extra_us=round((d - f) * 1e3, 1))
    row["passes"] = _passes(attr, a, dev)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="0,1,2,3", help="indices into ROWS")
    ap.add_argument("--iters", type=int, default=8, help="replays per timed window (the runner's steps)")
    ap.add_argument("--windows", type=int, default=5, help="windows per runner, alternating")
    ap.add_argument("--launches", type=int, default=8, help="iterations of the element-wise passes per captured graph")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for i in (int(v) for v in a.rows.split(",")):
        print(json.dumps(_row(*ROWS[i], a, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Frequency-band attack: BandRunner's captured iteration next to AttackRunner's L2 iteration at the same model and batch, and
the launches the band iteration adds, each on its own.

    python tools/bench_band.py                      # one JSON line: per-iteration times of both captured graphs and the ratio
    python tools/bench_band.py --kernels            # the added launches at the row's shape: event times, operands rotated

Row: UDEB4 256^2 bs 96.  Both runners hold one captured iteration on the same frozen eval-mode model in one process; the graphs
are replayed alternately window by window, a window being --iters replays ending in a device synchronise, timed on the host
clock.  AttackRunner's L2 iteration is forward + d/dx + two norms, a step and a projection (four element-wise launches and two
folds); BandRunner's is forward + d/dx + the keep-best (a few [batch] ops and two ud_apgd_keep) + ud_plane_dct2 forward +
ud_band_dots (+ fold) + ud_band_update + ud_plane_dct2 inverse with base and clip.  --kernels times each added launch alone
with HIP events; successive calls rotate over --sets sets of operands, more bytes than the 256 MB Infinity Cache holds, so that
no call finds its operands cached by the one before, as inside an iteration (where a forward + d/dx lies between them)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

NAME, SIZE, BATCH = "UDEB4", 256, 96
EPS, LO, HI = 1.0, -1.0, 1.0


def _model(dev):
    from unidefense_amd.model import load_model
    m = load_model(NAME)(num_classes=2, drop_rate=0.5, extractor="efficientnet-b4")
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev).eval()


def _window(graph, iters, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(iters):
        graph.replay()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3 / iters


def _row(a, dev):
    from unidefense_amd.attack import AttackRunner
    from unidefense_amd.band import BandRunner
    m = _model(dev)
    x = (param_fill.make_input(a.batch, SIZE, 3) * 0.5).to(dev)
    y = param_fill.make_labels(a.batch).to(dev)
    runners = {"attack_l2": AttackRunner(m, a.batch, SIZE, norm="l2", eps=EPS, steps=2, step=0.25),
               "band": BandRunner(m, a.batch, SIZE, band=(0.0, 0.125), eps=EPS, steps=2, step=0.25)}
    for _ in range(3):                       # the eager warm-up, the capture, a replayed call
        for r in runners.values():
            r(x, y)
    t = {k: [] for k in runners}
    for _ in range(a.windows):
        for k, r in runners.items():
            t[k].append(_window(r.graph, a.iters, dev))
    row = {"model": NAME, "size": SIZE, "batch": a.batch, "iters_per_window": a.iters, "windows": a.windows}
    for k in runners:
        row[f"{k}_ms_per_iter"] = round(statistics.median(t[k]), 3)
        row[f"{k}_min_max_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    row["band_over_attack_l2"] = round(statistics.median(t["band"]) / statistics.median(t["attack_l2"]), 4)
    return row


def _kernels(a, dev):
    from unidefense_amd import band as BD
    from unidefense_amd import kernels as K
    gen = torch.Generator().manual_seed(1)
    n, per, R = a.batch, 3 * SIZE * SIZE, a.sets
    x0 = (torch.rand(n, 3, SIZE, SIZE, generator=gen) - 0.5).to(dev)
    g0 = torch.randn(n, 3, SIZE, SIZE, generator=gen).to(dev)
    x, g = [x0.clone() for _ in range(R)], [g0.clone() for _ in range(R)]
    w, G, xa, best = ([torch.zeros_like(x0) for _ in range(R)] for _ in range(4))
    D, Dt = BD._matrices(dev, SIZE)
    mask = BD.band_mask(SIZE, 0.0, 0.125).to(dev)
    dots = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    ws = torch.zeros(max(K.band_dots_ws_bytes(n, per) // 8, 1), dtype=torch.float64, device=dev)
    ss = torch.zeros(n, dtype=torch.float64, device=dev)
    ssws = torch.zeros(max(K.sample_sumsq_ws_bytes(n, per) // 8, 1), dtype=torch.float64, device=dev)
    keep = torch.ones(n, dtype=torch.int32, device=dev)
    flops = 4.0 * SIZE ** 3 * 3 * n
    cases = (("ud_plane_dct2 forward, mask", flops, lambda i: K.plane_dct2(g[i], D, Dt, mask, out=G[i])),
             ("ud_plane_dct2 inverse, base + clip", flops,
              lambda i: K.plane_dct2(w[i], D, Dt, None, inverse=True, out=xa[i], base=x[i], clip=(LO, HI))),
             ("ud_band_dots", 0, lambda i: K.band_dots(w[i], G[i], out=dots, ws=ws)),
             ("ud_band_update", 0, lambda i: K.band_update(w[i], G[i], dots, 0.25, EPS)),
             ("ud_apgd_keep, every sample kept", 0, lambda i: K.apgd_keep(best[i], xa[i], keep)),
             ("ud_sample_sumsq (AttackRunner's norm)", 0, lambda i: K.sample_sumsq(g[i], None, out=ss, ws=ssws)))
    out = {"model": NAME, "size": SIZE, "batch": n, "reps": a.reps, "sets": R, "MB_per_tensor": round(4e-6 * n * per, 1), "kernels": {}}
    for label, fl, fn in cases:
        for i in range(R):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for k in range(a.reps):
            fn(k % R)
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.reps
        out["kernels"][label] = dict({"event_us_per_call": round(us, 1)}, **({"tflops": round(fl / us * 1e-6, 1)} if fl else {}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--iters", type=int, default=10, help="replays per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per runner, alternating")
    ap.add_argument("--kernels", action="store_true", help="the launches the band iteration adds, on their own")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sets", type=int, default=6, help="with --kernels: sets of operands the calls rotate over")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps((_kernels if a.kernels else _row)(a, dev)), flush=True)


if __name__ == "__main__":
    main()

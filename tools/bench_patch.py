"""Adversarial patch: PatchRunner's captured iteration next to UniversalRunner's at the same model and batch, and the three
kernels of csrc/patch.hip on their own.

    python tools/bench_patch.py                      # one JSON line: per-iteration times of both runners and their ratio
    python tools/bench_patch.py --kernels            # the three launches alone: bytes, bytes / 5.5 TB/s, event times

Row: UDEB4 256^2 bs 96 fp32, a patch of side 64 at the runner's default placement ranges.  Both runners hold one captured
iteration of the same frozen eval-mode model in one process (summed cross-entropy); after a call that fills their buffers the
GRAPHS are replayed, alternating window by window; a window is --iters replays ending in a device synchronise, timed on the host
clock; the figure is the median over --windows.  UniversalRunner's iteration is forward + d/dx + control + reduce (over 3 size^2
elements) + ONE update launch that reads x and writes x_adv; PatchRunner's is forward + d/dx + ud_patch_grad + control +
reduce (over 3 P^2) + ud_patch_update + ud_patch_paste, which also reads x once and writes x_adv once.

--kernels rotates every launch over --sets sets of operands (x, g, out: 75 MB each at this row), more than the 256 MB
Infinity Cache between two uses of the same buffer, so the times are HBM times; the placements are the runner's, freshly drawn."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

ROW = ("UDEB4", 256, 96, 64)
EPS, LO, HI = 4.0 / 255.0, -1.0, 1.0
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable


def _model(name, dev):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    m = load_model(name)(num_classes=2, drop_rate=0.5, **kw)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev).eval()


def _window(graphs, iters, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(iters):
        for g in graphs:
            g.replay()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3 / iters


def _row(name, size, bs, P, a, dev):
    from unidefense_amd.patch import PatchRunner
    from unidefense_amd.universal import UniversalRunner
    m = _model(name, dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    gen = torch.Generator().manual_seed(0)
    runners = {"universal": (UniversalRunner(m, bs, size, norm="linf", eps=EPS, steps=1, step=EPS / 4), ()),
               "patch": (PatchRunner(m, bs, size, patch=P, steps=1), (gen,))}
    for _ in range(3):                       # the eager warm-up, the capture, one replayed call: the buffers are filled
        for r, extra in runners.values():
            r(x, y, *extra)
    t = {k: [] for k in runners}
    for _ in range(a.windows):
        for k, (r, _) in runners.items():
            t[k].append(_window([r.graph], a.iters, dev))
    row = {"model": name, "size": size, "batch": bs, "patch": P, "area": round(runners["patch"][0].args["area"], 4),
           "iters_per_window": a.iters, "windows": a.windows}
    for k in runners:
        row[f"{k}_ms_per_iter"] = round(statistics.median(t[k]), 3)
        row[f"{k}_min_max_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    row["patch_over_universal"] = round(statistics.median(t["patch"]) / statistics.median(t["universal"]), 4)
    return row


def _kernels(name, size, bs, P, a, dev):
    from unidefense_amd import kernels as K
    from unidefense_amd import patch as PT
    gen = torch.Generator().manual_seed(1)
    per = 3 * size * size
    xs = [(torch.rand(bs, 3, size, size, generator=gen) * 2 - 1).to(dev) for _ in range(a.sets)]
    outs = [torch.empty_like(xs[0]) for _ in range(a.sets)]
    gs = [torch.randn(bs, 3, size, size, generator=gen).to(dev) for _ in range(a.sets)]
    gp = torch.zeros(bs, 3, P, P, device=dev)
    patch, gsum = (torch.rand(3, P, P, generator=gen) * 2 - 1).to(dev), torch.randn(3, P, P, generator=gen).to(dev)
    alpha = PT.patch_alpha(P).to(dev)
    params, table = PT.patch_placements(bs, size, P, generator=gen)
    table = table.view(1, bs, PT.ROW).to(dev)
    k = torch.zeros(1, dtype=torch.int32, device=dev)
    covered = float((params[:, 3] ** 2).sum()) * P * P               # pixels under the patches, summed over the batch
    turn = [0]

    def paste():
        i = turn[0] = (turn[0] + 1) % a.sets
        K.patch_paste(xs[i], patch, alpha, table, k, outs[i], LO, HI)

    def grad():
        i = turn[0] = (turn[0] + 1) % a.sets
        K.patch_grad(gs[i], alpha, table, k, gp)

    cases = (("ud_patch_paste", 4 * 2 * bs * per, paste),
             ("ud_patch_grad", int(4 * 3 * covered) + 4 * bs * 3 * P * P, grad),
             ("ud_patch_update", 4 * 3 * 3 * P * P, lambda: K.patch_update(patch, gsum, 1.0 / 32, LO, HI)))
    out = {"model": name, "size": size, "batch": bs, "patch": P, "sets": a.sets, "reps": a.reps, "kernels": {}}
    for label, nbytes, fn in cases:
        for _ in range(2 * a.sets):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        e1.synchronize()
        out["kernels"][label] = {"bytes": nbytes, "ideal_us_at_5.5TBps": round(nbytes / HBM_BPS * 1e6, 2),
                                 "event_us_per_call": round(e0.elapsed_time(e1) * 1e3 / a.reps, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="replays per timed window")
    ap.add_argument("--windows", type=int, default=7, help="windows per runner, alternating")
    ap.add_argument("--kernels", action="store_true", help="launch the kernels of csrc/patch.hip only")
    ap.add_argument("--sets", type=int, default=6, help="with --kernels: operand sets a launch rotates over")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--batch", type=int, default=ROW[2])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    name, size, _, P = ROW
    print(json.dumps((_kernels if a.kernels else _row)(name, size, a.batch, P, a, dev)), flush=True)


if __name__ == "__main__":
    main()

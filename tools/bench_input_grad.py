"""Gradient with respect to the input image: replay times of the graph-captured eval forward, the frozen forward + d/dx, the
same with the parameters requiring grad, and the training step (forward + backward of the pass-1 loss), per model.

    python tools/bench_input_grad.py                    # the three rows, one JSON line each
    python tools/bench_input_grad.py --trace frozen     # eager frozen forward + d/dx passes only (for rocprofv3 runs)

    python tools/bench_input_grad.py --precision both [--size 380 --batch 32]   # UDEB4: InputGradRunner fp16 against fp32

Rows: UDEB4 256^2 bs 32, UDR50 320^2 bs 16, UDR18 256^2 bs 32.  Each column: one eager warm-up, then a hipGraph capture and
--replays timed replays (HIP events; median per replay).
--precision fp32 / fp16 / both (UDEB4 only): InputGradRunner(precision=...)(x, y) calls (copy-in + one replay) of the summed
cross-entropy, in windows of --replays calls timed on the host clock around a device synchronise; with `both` the two runners'
windows alternate in one process; reported: the median of --windows windows each, their ratio and the windows' spread."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402
from tests import oracle_util as ou  # noqa: E402

ROWS = (("UDEB4", 256, 32), ("UDR50", 320, 16), ("UDR18", 256, 32))


def _model(name, dev):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    m = load_model(name)(num_classes=2, drop_rate=0.5, **kw)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev)


def _scalar(o):
    """a smooth scalar of every output (the objective of an attack or a saliency map is some such function)"""
    ld = o["loss_dict"]
    return (o["cls_out"] * o["cls_out"]).sum() + 10.0 * (o["rec"] * o["rec"]).mean() + ld["freq_mask"].mean() \
        + ld["spat_mask"].mean() + sum((f * f).mean() for f in ld["triplet"])


def _set_frozen(m, frozen):
    for n_, p in m.named_parameters():
        p.requires_grad_(not frozen and n_ != "bottleneck.bias")


def _columns(m, x, tgt):
    n = x.shape[0]
    xs = x.clone().requires_grad_()

    def eval_fwd():
        with torch.no_grad():
            m(x)

    def frozen_dx():
        torch.autograd.grad(_scalar(m(xs)), xs)

    def unfrozen_dx():
        _scalar(m(xs)).backward()

    def train_step():            # the pass-1 loss on the product's (capturable) loss kernels, as the engine's step
        from unidefense_amd.loss import LOSSES
        LOSSES["aw_triplet"].n_real = n // 2
        o = m(x)
        ld, lam = o["loss_dict"], ou.LAMBDAS
        loss = LOSSES["cross_entropy"](o["cls_out"], tgt) + lam["lambda_mask"] * (ld["freq_mask"].mean() + ld["spat_mask"].mean()) \
            + lam["lambda_triplet"] * sum(LOSSES["aw_triplet"](f, tgt) for f in ld["triplet"]) \
            + lam["lambda_recons"] * ld["spatial"][: n // 2].mean() + lam["lambda_freq"] * ld["freq"][: n // 2].mean()
        loss.backward()
    return (("eval_fwd_ms", "eval", True, eval_fwd), ("frozen_fwd_dx_ms", "eval", True, frozen_dx),
            ("params_fwd_dx_ms", "eval", False, unfrozen_dx), ("train_step_ms", "train", False, train_step))


def _time_captured(fn, replays):
    fn()                                   # the eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    del g
    return statistics.median(ts)


def _row_precision(a, dev):
    from unidefense_amd.attack import InputGradRunner
    m = _model("UDEB4", dev).eval()
    x = param_fill.make_input(a.batch, a.size, 3).to(dev)
    y = param_fill.make_labels(a.batch).to(dev)
    precs = ("fp32", "fp16") if a.precision == "both" else (a.precision,)
    runners = {p: InputGradRunner(m, a.batch, a.size, precision=p) for p in precs}
    for _ in range(3):                       # the eager warm-up, the capture, one replay
        for r in runners.values():
            r(x, y)
    t = {p: [] for p in precs}
    for _ in range(a.windows):
        for p, r in runners.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.replays):
                r(x, y)
            torch.cuda.synchronize(dev)
            t[p].append((time.perf_counter() - t0) * 1e3 / a.replays)
    row = {"model": "UDEB4", "size": a.size, "batch": a.batch, "calls_per_window": a.replays, "windows": a.windows}
    for p in precs:
        row[f"{p}_ms_per_call"] = round(statistics.median(t[p]), 3)
        row[f"{p}_min_max_ms"] = [round(min(t[p]), 3), round(max(t[p]), 3)]
    if len(precs) == 2:
        row["fp32_over_fp16"] = round(statistics.median(t["fp32"]) / statistics.median(t["fp16"]), 4)
        g32, g16 = runners["fp32"](x, y), runners["fp16"](x, y)
        row["rel_l2_fp16_vs_fp32"] = float((g16 - g32).norm() / g32.norm())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rows", default="UDEB4,UDR50,UDR18")
    ap.add_argument("--trace", choices=("frozen", "params"), default=None,
                    help="eager forward + d/dx passes only (no capture): the launches a rocprofv3 kernel trace counts")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--precision", choices=("fp32", "fp16", "both"), default=None,
                    help="UDEB4: time InputGradRunner(precision=...); both: the two runners' windows alternate in one process")
    ap.add_argument("--size", type=int, default=256, help="with --precision: the input side")
    ap.add_argument("--batch", type=int, default=32, help="with --precision: the batch size")
    ap.add_argument("--windows", type=int, default=5, help="with --precision: windows per runner")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.precision is not None:
        print(json.dumps(_row_precision(a, dev)), flush=True)
        return
    for name, size, bs in ROWS:
        if name not in a.rows.split(","):
            continue
        m = _model(name, dev)
        x = param_fill.make_input(bs, size, 3).to(dev)
        tgt = param_fill.make_labels(bs).to(dev)
        if a.trace:
            m.eval()
            _set_frozen(m, a.trace == "frozen")
            xs = x.clone().requires_grad_()
            for _ in range(a.passes):
                torch.autograd.grad(_scalar(m(xs)), xs)
            torch.cuda.synchronize()
            print(json.dumps({"model": name, "size": size, "batch": bs, "trace": a.trace, "passes": a.passes}), flush=True)
            continue
        row = {"model": name, "size": size, "batch": bs}
        for key, mode, frozen, fn in _columns(m, x, tgt):
            m.train(mode == "train")
            _set_frozen(m, frozen)
            m.zero_grad(set_to_none=True)
            row[key] = round(_time_captured(fn, a.replays), 3)
        _set_frozen(m, False)
        print(json.dumps(row), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

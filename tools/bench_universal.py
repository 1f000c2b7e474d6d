"""Universal perturbation: the UniversalRunner's captured iteration next to AttackRunner's at the same model and batch, the
three kernels of csrc/universal.hip on their own, and the held-out tables of TrainEngine.test_universal.

    python tools/bench_universal.py                      # one JSON line per row: per-iteration times of both runners
    python tools/bench_universal.py --kernels            # the kernels at the row's shape: bytes, bytes / 5.5 TB/s, event times
    python tools/bench_universal.py --tables             # clean / adv / control of a fit on synthetic batches, per model

Rows: UDEB4 256^2 bs 32, UDR18 128^2 bs 32.  Both runners run an L-infinity iteration (summed cross-entropy, eps 4/255) on the
same frozen eval-mode model in one process, alternating window by window; a window is one call of --iters iterations ending in
a device synchronise, timed on the host clock.  AttackRunner's iteration is forward + d/dx + ONE element-wise launch;
UniversalRunner's is forward + d/dx + control + reduce + update: the difference is what the batch reduction costs."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import param_fill  # noqa: E402

ROWS = (("UDEB4", 256, 32), ("UDR18", 128, 32))
EPS, LO, HI = 4.0 / 255.0, -1.0, 1.0
HBM_BPS = 5.5e12          # the bandwidth the project takes as achievable
ENGINE = {"config": {"warmup_step": 2, "lambda_triplet": 0.1, "lambda_recons": 0.1, "lambda_freq": 1.0, "lambda_mask": 0.1,
                     "lambda_fac": 0.1, "num_steps": 4, "log_steps": 2, "local_rank": 0,
                     "optimizer": {"name": "adamw", "lr": 1e-4, "betas": [0.9, 0.999], "weight_decay": 5e-6, "amsgrad": True},
                     "scheduler": {"name": "StepLR", "step_size": 22500, "gamma": 0.5}}}


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


def _row(name, size, bs, a, dev):
    from unidefense_amd.attack import AttackRunner
    from unidefense_amd.universal import UniversalRunner
    m = _model(name, dev)
    x = param_fill.make_input(bs, size, 3).to(dev)
    y = param_fill.make_labels(bs).to(dev)
    runners = {"attack": AttackRunner(m, bs, size, norm="linf", eps=EPS, steps=a.iters, step=EPS / 4),
               "universal": UniversalRunner(m, bs, size, norm="linf", eps=EPS, steps=a.iters, step=EPS / 4),
               "universal_l2": UniversalRunner(m, bs, size, norm="l2", eps=1.0, steps=a.iters, step=0.1)}
    for _ in range(2):                       # the eager warm-up, then the capture
        for r in runners.values():
            r(x, y)
    t = {k: [] for k in runners}
    for _ in range(a.windows):
        for k, r in runners.items():
            t[k].append(_window(lambda: r(x, y), dev) / a.iters)
    row = {"model": name, "size": size, "batch": bs, "iters_per_window": a.iters, "windows": a.windows}
    for k in runners:
        row[f"{k}_ms_per_iter"] = round(statistics.median(t[k]), 3)
        row[f"{k}_min_max_ms"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    row["universal_over_attack"] = round(statistics.median(t["universal"]) / statistics.median(t["attack"]), 4)
    return row


def _kernels(name, size, bs, a, dev):
    from unidefense_amd import kernels as K
    gen = torch.Generator().manual_seed(1)
    per = 3 * size * size
    x = (torch.rand(bs, per, generator=gen) * 2 - 1).to(dev)
    xa = torch.empty_like(x)
    g = torch.randn(bs, per, generator=gen).to(dev)
    w = torch.ones(bs, dtype=torch.int32, device=dev)
    delta, gsum = torch.zeros(per, device=dev), torch.zeros(per, device=dev)
    ist, wc, history, counted = K.uap_state(bs, 1, dev)
    f, y = torch.rand(bs, device=dev), torch.zeros(bs, dtype=torch.int64, device=dev)

    def control():
        ist.zero_()
        K.uap_control(f, y, wc, ist, history, counted, float("inf"))

    cases = (("ud_uap_reduce", 4 * (bs + 1) * per, lambda: K.uap_reduce(g, w, gsum)),
             ("ud_uap_update_linf", 4 * (2 * bs + 3) * per, lambda: K.uap_update_linf(delta, gsum, x, xa, EPS / 4, EPS, LO, HI)),
             ("ud_uap_apply", 4 * (2 * bs + 1) * per, lambda: K.uap_apply(delta, None, x, xa, EPS, LO, HI)),
             ("memset + ud_uap_control", 0, control))
    out = {"model": name, "size": size, "batch": bs, "per": per, "reps": a.reps, "kernels": {}}
    for label, nbytes, fn in cases:
        for _ in range(3):
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


def _mean_ce(res):
    p = res["scores"].double()
    return float(-torch.log(torch.where(res["labels"] == 0, p, 1.0 - p).clamp_min(1e-30)).mean())


def _table(name, size, bs, a, dev):
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(ENGINE)
    cfg["model"] = dict({"name": name, "num_classes": 2, "drop_rate": 0.2}, **({"extractor": "efficientnet-b4"} if name == "UDEB4" else {}))
    cfg["data"] = {"train_batch_size": a.table_batch // 2, "size": size}
    eng = get_engine("FE")(cfg, "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    out = {"model": name, "size": size, "batch": a.table_batch, "fit_batches": 4, "epochs": 2, "held_out_batches": 4, "rows": {}}
    for norm, eps in (("linf", EPS), ("l2", 1.0)):
        res = eng.test_universal(batches=4, fit_batches=4, epochs=2, universal={"norm": norm, "eps": eps, "steps": 2, "seed": 0})
        att = res["attack"]
        out["rows"][norm] = {"eps": eps, "linf": round(att["linf"], 6), "l2": round(att["l2"], 4), "fooled": att["fooled"],
                             "fooled_control": att["fooled_control"], "fit_counted": att["fit_counted"],
                             **{k: {"acc": round(res[k]["acc"], 4), "auc": round(float(res[k].get("AUC", float("nan"))), 4),
                                    "mean_ce": round(_mean_ce(res[k]), 4)} for k in ("clean", "adv", "control")}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="UDEB4,UDR18")
    ap.add_argument("--iters", type=int, default=20, help="iterations per timed window")
    ap.add_argument("--windows", type=int, default=5, help="windows per runner, alternating")
    ap.add_argument("--kernels", action="store_true", help="launch the kernels of csrc/universal.hip only")
    ap.add_argument("--tables", action="store_true", help="TrainEngine.test_universal on synthetic batches")
    ap.add_argument("--table-batch", type=int, default=16, help="with --tables: samples per batch (half real, half fake)")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, size, bs in ROWS:
        if name not in a.rows.split(","):
            continue
        row = (_kernels if a.kernels else _table if a.tables else _row)(name, size, bs, a, dev)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

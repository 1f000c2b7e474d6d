"""In-step plan search (round 6): coordinate descent over the GEMM plan table with the WHOLE replayed step as the objective.

The shipped plans (unidefense_amd/gemm_plans_gfx950.json) were measured per shape in isolation (kernels._tuned_plan / _p2_tune: a
few back-to-back launches of ONE shape in a small hipGraph).  Inside the step a launch runs between other kernels — clocks, L2 /
Infinity-Cache contents, the fills its plan needs — and the best form can differ: the tail pair of round 6 gained 0.06 ms by the
isolated probe and 0.15 ms in the step (profiles/r06/p3_tail_pair*.txt).  This tool re-captures the bench step with ONE plan entry
changed at a time and keeps a change only if the replayed step gets faster by a margin and stays so on a repeat.

  python tools/tune_in_step.py [--budget-min 40] [--kinds p2c,x3] [--out gpurun_out/plans_in_step.json] [bench-style --model/--size/--batch]

Writes the changed entries as a UD_GEMM_TUNE_CACHE-style JSON (merge with tools/merge_plans.py) and a log of every trial.
"""
import argparse
import collections
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Logged(dict):
    """the plan table, counting which keys the step looks up"""

    def __init__(self, *a):
        super().__init__(*a)
        self.hits = collections.Counter()

    def get(self, k, d=None):
        self.hits[k] += 1
        return super().get(k, d)

    def __contains__(self, k):
        self.hits[k] += 1
        return super().__contains__(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget-min", type=float, default=40.0)
    ap.add_argument("--kinds", default="p2c,x3")
    ap.add_argument("--out", default="gpurun_out/plans_in_step.json")
    ap.add_argument("--model", default="UDEB4")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--knobs", action="store_true", help="search the launch POLICIES instead of the GEMM plans: tiled / strip depthwise "
                                                        "kernels per block class, fused depthwise backward, two-pass transforms, "
                                                        "the adjoint-fused depthwise backward's sizes, the 32 x 32 transforms' form")
    ap.add_argument("--wide", action="store_true", help="every split-K factor of a shape, not only the current one's neighbours")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16"], help="f16: BASELINE configs[4] (fp16 MFMA + half storage; use --batch 64)")
    ap.add_argument("--margin", type=float, default=0.012, help="ms a candidate must win by (and 2/3 of it again on the repeat)")
    args = ap.parse_args()
    import bench
    from unidefense_amd import kernels as K
    from unidefense_amd.loss import LOSSES
    from unidefense_amd.model import load_model
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    ctor = dict(extractor="efficientnet-b4") if args.model == "UDEB4" else {}
    with contextlib.redirect_stdout(sys.stderr):
        model = load_model(args.model)(num_classes=2, drop_rate=0.5, **ctor).to(dev).train()
    if args.dtype == "f16":
        from unidefense_amd import lib as _udlib
        _udlib.call("ud_gemm_set_path", 3)
        model.half_storage = True
    bs = args.batch
    g = torch.Generator().manual_seed(100)
    x = (2.0 * torch.rand(bs, 3, args.size, args.size, generator=g) - 1.0).to(dev)
    tgt = torch.tensor([0] * (bs // 2) + [1] * (bs // 2), device=dev)
    LOSSES["aw_triplet"].n_real = bs // 2
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        for p in params:
            p.grad = None
        loss = bench.pass1_loss(model(x), tgt, bs // 2, LOSSES)
        (loss * 1024.0 if args.dtype == "f16" else loss).backward()
        return loss

    K._TUNED = Logged(K._TUNED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    K._TUNED.hits.clear()
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    used = [k for k in K._TUNED.hits if dict.__contains__(K._TUNED, k)]
    from unidefense_amd.config import cfg
    cfg.gemm_tune = False                                   # no on-line tuning from here on: the table is what we edit
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def measure():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            graph.replay()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) / args.reps
        del graph
        return t

    def candidates(key, val):
        """[(description, new value)] for one table entry"""
        out = []
        if key[0] == "p2c":
            if val is None:
                return out
            _, M, N, Kd = key[:4]
            for idx, (kind, (m, n, k)) in enumerate((("nt", (M, N, Kd)), ("nn", (M, Kd, N)), ("tn", (N, Kd, M)))):
                cur = tuple(val[idx])
                cands = [tuple(p) for p in K._p2_plans(kind, m, n, k)]
                if kind == "tn" and not args.wide:        # the split list is long: the current factor's neighbours + plain
                    s0 = cur[1] if cur[0] == "split" else 1
                    cands = [c for c in cands if c[0] != "split" or 0.4 * s0 <= c[1] <= 2.6 * s0]
                if kind == "nn":
                    cands = [c for c in cands if c[0] != "tail"]          # (a tail data gradient is not paired)
                for c in cands:
                    if c != cur:
                        nv = [tuple(v) for v in val]
                        nv[idx] = c
                        out.append((f"{kind} {'/'.join(map(str, cur))} -> {'/'.join(map(str, c))}", tuple(nv)))
        else:
            _, M, N, Kd = key[:4]
            cands = [None] + list(K._tune_candidates(M, N, Kd))
            if val is not None and not args.wide:         # neighbours of the current (tile, split), all tiles
                cands = [c for c in cands if c is None or 0.4 * val[1] <= c[1] <= 2.6 * val[1]]
            for c in cands:
                if c != val:
                    out.append((f"{val} -> {c}", c))
        return out

    def weight(key):
        _, M, N, Kd = key[:4]
        return 2.0 * M * N * Kd if key[0] == "p2c" else 4.0 * (M * Kd + M * N + N * Kd) * 50       # (x3 shapes: by bytes, roughly)

    def trial(desc, apply, revert, state):
        """one policy change: keep it if the replayed step gets faster by the margin and stays so on a repeat"""
        apply()
        try:
            t = measure()
        except Exception as e:                          # noqa: BLE001 — a combination the kernels refuse
            revert()
            torch.cuda.synchronize()
            print(f"  {desc}: failed ({type(e).__name__}: {str(e)[:80]})", flush=True)
            return False
        keep, mark = False, ""
        if t < state["base"] - args.margin:
            t2 = measure()
            revert()
            b2 = measure()
            if t2 < b2 - args.margin * 2 / 3:
                apply()
                keep, mark = True, "  <== kept"
                state["base"] = min(t, t2)
            else:
                mark = f"  (not confirmed: {t2:.3f} vs {b2:.3f})"
                state["base"] = b2
        else:
            revert()
        print(f"  {desc}: {t:.3f} ms (incumbent {state['base']:.3f}){mark}", flush=True)
        return keep

    if args.knobs:
        from unidefense_amd import lib as _lib
        from unidefense_amd import mbconv as MB
        seen_tile, seen_fused = [], []
        o_tile, o_fused = MB._dw_tile_policy, MB._dw_bwd_fused_policy

        def log_tile(sf, k, stride, H, half):
            key = (bool(sf), k, stride, H, bool(half))
            if key not in seen_tile:
                seen_tile.append(key)
            return o_tile(sf, k, stride, H, half)

        def log_fused(sf, k, stride, H, half):
            key = (bool(sf), k, stride, H, bool(half))
            if key not in seen_fused and stride == 1:
                seen_fused.append(key)
            return o_fused(sf, k, stride, H, half)
        MB._dw_tile_policy, MB._dw_bwd_fused_policy = log_tile, log_fused
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        MB._dw_tile_policy, MB._dw_bwd_fused_policy = o_tile, o_fused
        state = {"base": min(measure(), measure())}
        print(f"# policy search; baseline {state['base']:.3f} ms; {len(seen_tile)} depthwise block classes", flush=True)
        kept = []
        for key in seen_tile:
            cur = tuple(o_tile(*key))
            for pos, name in enumerate(("forward", "weight gradient", "data gradient")):
                new = tuple((not v) if i == pos else v for i, v in enumerate(cur))
                if trial(f"dw_tile{key} {name}: {cur[pos]} -> {new[pos]}",
                         lambda: MB._DW_TILE_OVERRIDE.__setitem__(key, new), lambda: MB._DW_TILE_OVERRIDE.pop(key, None), state):
                    kept.append(("mbconv._DW_TILE_OVERRIDE", key, new))
                    cur = new
        for key in seen_fused:
            cur = bool(o_fused(*key))
            if trial(f"dw_bwd_fused{key}: {cur} -> {not cur}",
                     lambda: MB._DW_BWD_FUSED_OVERRIDE.__setitem__(key, not cur), lambda: MB._DW_BWD_FUSED_OVERRIDE.pop(key, None), state):
                kept.append(("mbconv._DW_BWD_FUSED_OVERRIDE", key, not cur))
        for kind in ("rfft", "rfft_ex", "irfft", "irfft_mix"):
            for S in (32, 64):
                item = (kind, S, args.dtype == "f16")
                had = item in K._FFT2P_POLICY
                if trial(f"two-pass transform {item}: {had} -> {not had}",
                         (lambda: K._FFT2P_POLICY.discard(item)) if had else (lambda: K._FFT2P_POLICY.add(item)),
                         (lambda: K._FFT2P_POLICY.add(item)) if had else (lambda: K._FFT2P_POLICY.discard(item)), state):
                    kept.append(("kernels._FFT2P_POLICY", item, not had))
        sizes0 = K._IRFFT_DWBWD_SIZES
        for sizes in ((8,), (16,), ()):
            def set_sizes(v=sizes):
                K._IRFFT_DWBWD_SIZES = v
            if trial(f"adjoint-fused depthwise backward sizes {sizes0} -> {sizes}", set_sizes, lambda: set_sizes(sizes0), state):
                kept.append(("kernels._IRFFT_DWBWD_SIZES", sizes, True))
                sizes0 = sizes
        for mode in (1, 2):
            if trial(f"32 x 32 transforms: auto -> {'one lane per row' if mode == 1 else 'lane pairs'}",
                     lambda: _lib.call("ud_fft32_set_wave", mode), lambda: _lib.call("ud_fft32_set_wave", 0), state):
                kept.append(("ud_fft32_set_wave", mode, True))
        final = min(measure(), measure())
        print(f"# step {final:.3f} ms; kept: {kept}", flush=True)
        sys.stdout.flush()
        os._exit(0)

    kinds = args.kinds.split(",")
    keys = [k for k in used if (k[0] == "p2c" and "p2c" in kinds) or (k[0] != "p2c" and "x3" in kinds)]
    keys.sort(key=weight, reverse=True)
    t_start = time.perf_counter()
    base = min(measure(), measure())
    print(f"# {len(used)} plan entries looked up by the step, {len(keys)} searched; baseline {base:.3f} ms", flush=True)
    changed, trials = {}, 0
    for key in keys:
        if (time.perf_counter() - t_start) / 60.0 > args.budget_min:
            print("# budget spent", flush=True)
            break
        val = dict.__getitem__(K._TUNED, key)
        best_val, best_t = val, base
        for desc, nv in candidates(key, val):
            dict.__setitem__(K._TUNED, key, nv)
            try:
                t = measure()
            except Exception as e:                      # noqa: BLE001 — a plan the kernels refuse: skip it
                print(f"  {key}: {desc}: failed ({type(e).__name__})", flush=True)
                torch.cuda.synchronize()
                continue
            trials += 1
            mark = ""
            if t < best_t - args.margin:
                t2 = measure()                           # repeat the candidate and the incumbent
                dict.__setitem__(K._TUNED, key, best_val)
                b2 = measure()
                if t2 < b2 - args.margin * 2 / 3:
                    best_val, best_t, mark = nv, min(t, t2), "  <== kept"
                    base = best_t
                else:
                    mark = f"  (not confirmed: {t2:.3f} vs {b2:.3f})"
                    base = min(base, b2) if abs(b2 - base) < 0.05 else b2
                    best_t = base
            print(f"  {list(key)}: {desc}: {t:.3f} ms (incumbent {best_t:.3f}){mark}", flush=True)
            dict.__setitem__(K._TUNED, key, best_val)
        if best_val != val:
            changed[json.dumps(list(key))] = [list(v) for v in best_val] if key[0] == "p2c" else (list(best_val) if best_val else None)
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(changed, fh)
    final = min(measure(), measure())
    print(f"# {trials} trials in {(time.perf_counter() - t_start) / 60:.1f} min; {len(changed)} entries changed; step {final:.3f} ms", flush=True)
    for k, v in changed.items():
        print("#   ", k, "->", v)
    sys.stdout.flush()
    os._exit(0)


if __name__ == "__main__":
    main()

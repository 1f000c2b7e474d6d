"""Fold the parity-bar records of several full GPU-suite runs (tests/margins.py -> gpurun_out/margins/run_<tag>_<pid>.jsonl)
into one table: per test the quantity that came closest to its bar — largest observed value over the runs, the bar, the
margin (bar / observed) — and whether the observed values were IDENTICAL in every run (the suite runs in deterministic mode).
Quantities on a yardstick bar (tests/parity.py records "<quantity> [yard]" next to "<quantity>") are listed once more, each with
its kernel error, its fp32 yardstick and its bar side by side.
usage: python tools/margins_report.py <out.md> <tag> [<tag> ...]"""
import glob
import json
import os
import sys
from collections import defaultdict


def load(tag):
    rows = []
    for f in glob.glob(os.path.join("gpurun_out", "margins", f"run_{tag}_*.jsonl")):
        with open(f) as fh:
            rows += [json.loads(ln) for ln in fh if ln.strip()]
    return rows


YARD = " [yard]"


def yard_section(obs, bars, yard):
    """Every quantity on a yardstick bar: the kernel's error, the error of torch float32 on the CPU over the same reference
    lines (the yardstick), the bar = max(floor, margin x yardstick) or the quantity's named bar, and the two ratios."""
    rows = []
    for (test, name), y_by_tag in yard.items():
        e = max(max(v) for v in obs[(test, name)].values())
        y = max(max(v) for v in y_by_tag.values())
        bar = bars[(test, name)]
        rows.append((test, name, e, y, bar, e / y if y > 0 else (0.0 if e == 0 else float("inf")), e / bar))
    finite = [r for r in rows if r[5] != float("inf")]
    worst = max(finite, key=lambda r: r[5])
    above = [r for r in finite if r[4] > min(q[4] for q in rows)]          # bar set by the yardstick, not by the floor
    worst_above = max(above, key=lambda r: r[5]) if above else None
    closest = max(rows, key=lambda r: r[6])
    floor = min(r[4] for r in rows)
    lines = ["", "## Yardstick bars: kernel error, fp32 yardstick and bar side by side", "",
             f"{len(rows)} quantities; {sum(r[4] == floor for r in rows)} of them on the floor ({floor:.3g}).",
             f"Closest to its bar: {closest[6]:.2f} of the bar — `{closest[0].replace('tests/', '')}` — {closest[1]}.",
             f"Worst error / yardstick: {worst[5]:.2f} — `{worst[0].replace('tests/', '')}` — {worst[1]} "
             f"(error {worst[2]:.3g}, yardstick {worst[3]:.3g}, bar {worst[4]:.3g})."]
    if worst_above:
        lines.append(f"Worst error / yardstick among the quantities whose bar the yardstick sets (above the floor): "
                     f"{worst_above[5]:.2f} — `{worst_above[0].replace('tests/', '')}` — {worst_above[1]}.")
    lines += ["", "| test | quantity | kernel error | fp32 yardstick | bar | error / yardstick | error / bar |",
              "|---|---|---|---|---|---|---|"]
    for test, name, e, y, bar, r_y, r_b in sorted(rows):
        ry = "inf" if r_y == float("inf") else f"{r_y:.2f}"
        lines.append(f"| `{test.replace('tests/', '')}` | {name} | {e:.3g} | {y:.3g} | {bar:.3g} | {ry} | {r_b:.3f} |")
    return lines


def main():
    out, tags = sys.argv[1], sys.argv[2:]
    per_run = {t: load(t) for t in tags}
    # (test, name) -> {tag: [observed ...]}
    obs, bars = defaultdict(lambda: defaultdict(list)), {}
    for t, rows in per_run.items():
        for r in rows:
            k = (r["test"], r["name"])
            obs[k][t].append(r["observed"])
            bars[k] = r["bar"]
    # yardstick bars (tests/parity.py): "<quantity> [yard]" carries the fp32 yardstick under the same bar as "<quantity>";
    # those rows go side by side into their own table below, not into the per-test one
    yard = {(test, name[:-len(YARD)]): by_tag for (test, name), by_tag in obs.items() if name.endswith(YARD)}
    tests = defaultdict(list)
    for (test, name), by_tag in obs.items():
        if name.endswith(YARD):
            continue
        worst = max(max(v) for v in by_tag.values())
        same = len({tuple(v) for v in by_tag.values()}) == 1 and len(by_tag) == len(tags)
        bar = bars[(test, name)]
        ratio = worst / bar if bar > 0 else (0.0 if worst == 0 else float("inf"))        # bar 0: an exact comparison
        tests[test].append((ratio, name, worst, bar, same))
    lines = [f"# Parity bars of the GPU suite: observed maxima over {len(tags)} full runs ({', '.join(tags)})", "",
             f"{sum(len(v) for v in tests.values())} recorded quantities in {len(tests)} tests.  Per test: the quantity closest "
             "to its bar.  `same`: every recorded quantity of the test had bit-identical values in all runs.", "",
             "| test | quantity closest to its bar | observed (max over runs) | bar | margin | same in all runs |",
             "|---|---|---|---|---|---|"]
    n_same = 0
    tight = []
    for test in sorted(tests):
        qs = sorted(tests[test], reverse=True)
        ratio, name, worst, bar, _ = qs[0]
        all_same = all(q[4] for q in qs)
        n_same += all_same
        margin = (1.0 / ratio) if ratio > 0 else float("inf")
        if margin < 4.0:
            tight.append((margin, test, name))
        lines.append(f"| `{test.replace('tests/', '')}` | {name} | {worst:.3g} | {bar:.3g} | "
                     f"{'inf' if margin == float('inf') else '%.1fx' % margin} | {'yes' if all_same else 'NO'} |")
    lines += ["", f"Tests whose every recorded quantity was identical in all runs: {n_same} / {len(tests)}.", ""]
    if tight:
        lines.append("Bars with less than 4x margin (each explained in profiles/README.md):")
        lines += [f"* {m:.1f}x  `{t.replace('tests/', '')}` — {n}" for m, t, n in sorted(tight)]
    if yard:
        lines += yard_section(obs, bars, yard)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"{out}: {len(tests)} tests, {n_same} identical across runs, {len(tight)} with margin < 4x")


if __name__ == "__main__":
    main()

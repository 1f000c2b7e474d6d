"""CPU: writes tests/golden/smooth_counts_n5.npz, the recorded restatement behind the exact end-to-end test of CertifyRunner
(tests/test_s_smooth_gpu.py: test_exact_counts_with_a_known_classifier).

The known classifier is logits = (mean(x_noisy) - t_n, 0): a draw votes class 0 where the noisy image's mean exceeds the sample's
threshold.  The only freedom of the device is the order of its fp32 mean, so the seed and the thresholds are chosen HERE so that
over all 5 x 544 draws the restatement's |mean - t| never falls below 1e-5 (at least 40 times the reduction's rounding): each
threshold is the middle of a wide gap between two sorted means, the gap nearest to the quantile that gives the wanted vote
probability.  A seed whose counts are unsound (p_lower above the true probability: 1 in 1000 per sample by construction of the
bound), or whose p = 0.5 sample does not abstain, is skipped.  The full restatement takes about 15 s of numpy, which is why its
means are recorded; the test recomputes a few draws of every sample and compares them to the recorded ones bit for bit.

    python tools/smooth_fixture.py [--seed 20261020] [--out tests/golden/smooth_counts_n5.npz]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import param_fill  # noqa: E402
from tests.smooth_case import (ALPHA, IDS, INPUT_SEED, N0, NE, SIGMA, SIZE, N, decide,  # noqa: E402
                               restated_means)

TARGETS = (0.99, 0.9, 0.7, 0.5, 0.1)          # the vote probabilities P(mean > t) aimed at
GAP, CLEAR = 2.5e-5, 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "smooth_counts_n5.npz"))
    a = ap.parse_args()
    x = param_fill.make_input(N, SIZE, INPUT_SEED).numpy()
    per = x[0].size
    lam = float(np.float32(math.sqrt(3.0) * SIGMA))
    sd = lam / math.sqrt(3.0 * per)                               # of the mean of `per` uniforms on [-lam, lam]
    mu = x.reshape(N, -1).astype(np.float64).mean(1)
    ndtri = lambda p: float(torch.special.ndtri(torch.tensor(p, dtype=torch.float64)))     # noqa: E731
    phi = lambda z: 0.5 * math.erfc(-z / math.sqrt(2.0))                                    # noqa: E731
    for seed in range(a.seed, a.seed + 50):
        means = restated_means(x, IDS, range(N0 + NE), seed)
        t = np.empty(N, dtype=np.float32)
        for n in range(N):
            s = np.sort(means[n])
            wide = np.nonzero(np.diff(s) >= GAP)[0]
            mids = 0.5 * (s[wide] + s[wide + 1])
            want = mu[n] - ndtri(TARGETS[n]) * sd
            t[n] = np.float32(mids[np.argmin(np.abs(mids - want))])
        clear = float(np.abs(means - t.astype(np.float64)[:, None]).min())
        p_true = np.array([phi((mu[n] - float(t[n])) / sd) for n in range(N)])
        votes, counts0, counts, ca, predicted, p_lower, radius = decide(means, t)
        p_of_ca = np.where(ca == 0, p_true, 1.0 - p_true)
        ok = clear >= CLEAR and bool((p_lower <= p_of_ca).all()) and predicted[3] == -1 and predicted[4] == 1 \
            and predicted[:3].tolist() == [0, 0, 0]
        print(f"seed {seed}: clearance {clear:.3e}, p {np.round(p_true, 4).tolist()}, counts {counts.tolist()}, p_lower "
              f"{np.round(p_lower, 4).tolist()}, predicted {predicted.tolist()}, radius {np.round(radius, 4).tolist()}: "
              f"{'taken' if ok else 'skipped'}")
        if ok:
            np.savez(a.out, seed=np.int64(seed), input_seed=np.int64(INPUT_SEED), ids=np.array(IDS, dtype=np.int64), t=t,
                     p_true=p_true, means=means)
            print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")
            return
    raise SystemExit("no seed in the range gave a sound, clear case")


if __name__ == "__main__":
    main()

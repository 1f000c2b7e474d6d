"""The known-classifier case of tests/test_s_smooth_gpu.py and tools/smooth_fixture.py: its constants, the restatement's means and
CERTIFY's decision on them in float64 host math.  UDR18's input at 128 x 128, N = 5, uniform noise, sigma 0.25, n0 = 32, n = 512,
alpha = 0.001; the classifier is logits = (mean(x_noisy) - t_n, 0)."""
import math

import numpy as np

from unidefense_amd import smooth as S

N, SIZE, SIGMA, N0, NE, ALPHA, INPUT_SEED = 5, 128, 0.25, 32, 512, 0.001, 5
IDS = (3, (1 << 32) + 1, 0, 7, 12)


def restated_means(x, ids, draws, seed):
    """float64 [len(ids), len(draws)]: the mean of ref_smooth_noise's float32 image for every (sample, draw)"""
    lam = float(np.float32(math.sqrt(3.0) * SIGMA))
    out = np.empty((len(ids), len(draws)), dtype=np.float64)
    for i, (xi, sid) in enumerate(zip(x, ids)):
        rep = np.broadcast_to(xi.reshape(1, -1), (len(draws), xi.size))
        out[i] = S.ref_smooth_noise(rep, np.full(len(draws), sid), np.asarray(draws), "uniform", lam, seed).astype(np.float64).mean(1)
    return out


def decide(means, t):
    """(votes [draws, N], counts0, counts, predicted, p_lower, radius) of the known classifier, float64 host math"""
    votes = np.where(means.T - t.astype(np.float64)[None, :] > 0, 0, 1).astype(np.int32)
    counts0 = np.stack([(votes[:N0] == c).sum(0) for c in (0, 1)], 1).astype(np.int32)
    counts = np.stack([(votes[N0:] == c).sum(0) for c in (0, 1)], 1).astype(np.int32)
    ca = counts0.argmax(1)
    p_lower = np.array([S.clopper_pearson_lower(int(counts[n, ca[n]]), NE, ALPHA) for n in range(len(ca))])
    predicted = np.where(p_lower > 0.5, ca, -1).astype(np.int64)
    radius = S.certified_radius(p_lower, SIGMA, "uniform").numpy()
    return votes, counts0, counts, ca, predicted, p_lower, radius

"""The known-classifier case of tests/test_hsj_cpu.py and tests/test_u_hsj_gpu.py: a linear classifier sign(w . x - t_n) on
N = 5 inputs at 32 x 32 (D = 3072), evaluated in float64, with its closed-form minimum distances.

w has 48 large entries (every 64th coordinate, N(0, 1)) and 3024 small ones (0.002 N(0, 1)): the L-infinity attack has to get
the signs of the large ones right, which a few hundred probes can; the L2 estimate is rotation invariant, so its quality is
set by (probes / D) whatever w is.  x lies in [-0.5, 0.5] and the offsets w . x_n - t_n are small enough that the projection
onto the boundary stays inside clip = (-1, 1): |off| max|w| / |w|_2^2 and |off| / |w|_1 are both below 0.5."""
import numpy as np

N, SIZE, D = 5, 32, 3 * 32 * 32
GPU_SIZE = 128                                                   # the smallest size the GPU suite runs UDR18's forward at (DESIGN 3y says why not 32)
IDS = np.array([3, (1 << 32) + 1, 0, 7, 12], dtype=np.int64)
OFFSETS = {"l2": 8.0 * np.array([0.05, -0.08, 0.03, -0.06, 0.1]), "linf": 30.0 * np.array([0.05, -0.08, 0.03, -0.06, 0.1])}
# the schedules: CPU reaches the 1.25 bar of the closed form; GPU is the same construction at GPU_SIZE on a schedule of 130 queries (B_2 is capped)
CPU = {"l2": dict(steps=18, probes=200, max_probes=1000, bisect=20, halvings=8, init_trials=4, seed=3),
       "linf": dict(steps=12, probes=60, max_probes=1000, bisect=20, halvings=8, init_trials=16, seed=3)}
GPU = {"l2": dict(steps=3, probes=12, max_probes=18, bisect=16, halvings=4, init_trials=6, seed=3),
       "linf": dict(steps=3, probes=12, max_probes=18, bisect=16, halvings=4, init_trials=6, seed=3)}


def make(norm, size=SIZE):
    """x [N, 3, size, size] float32, w [D] float64, t [N] float64, y [N] int64 (the clean class), x_init (the next batch-mate, in
    cyclic order, that the classifier of sample n puts on the other side; none: the sample itself), closed [N]"""
    rng = np.random.default_rng(7)
    d = 3 * size * size
    x = (rng.random((N, 3, size, size), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    w = rng.standard_normal(d) * np.where(np.arange(d) % 64 == 0, 1.0, 0.002)
    off = OFFSETS[norm]
    m = x.reshape(N, -1).astype(np.float64) @ w
    t = m - off                                                  # w . x_n - t_n = off_n
    y = (off > 0).astype(np.int64)
    mate = np.arange(N)
    for n in range(N):
        for k in range(1, N):
            j = (n + k) % N
            if int(m[j] - t[n] > 0) != y[n]:
                mate[n] = j
                break
    closed = np.abs(off) / (np.linalg.norm(w) if norm == "l2" else np.abs(w).sum())
    assert np.abs(off).max() * np.abs(w).max() / (w @ w) < 0.5 and np.abs(off).max() / np.abs(w).sum() < 0.5      # the box is idle
    return {"x": x, "w": w, "t": t, "y": y, "ids": IDS, "x_init": x[mate].copy(), "mate": mate, "closed": closed, "off": off}


def decider(case, margins=None):
    """decide(x_try) -> the class per sample, in float64; margins: a list that receives every query's w . x - t"""
    def decide(xt):
        mg = np.asarray(xt).reshape(N, -1).astype(np.float64) @ case["w"] - case["t"]
        if margins is not None:
            margins.append(mg)
        return (mg > 0).astype(np.int64)
    return decide


def ref_hsj_control(mode, norm, ist, fst, rows_i, rows_f, logits=None, y=None, nrm=None, phi=None, decisions=None, history=None,
                    xis=None, delta0=0.0, inv_d=0.0, dfloor=0.0):
    """ud_hsj_control (csrc/hsj.hip) restated for tests/test_u_hsj_gpu.py, in place on the numpy arrays ist [13, N] int32, fst [8, N] float32 (rows_i / rows_f: the header's
    row names, kernels.HSJ_I / HSJ_F), phi / decisions int8, history float32, nrm float64 [2, N]: one Python loop per sample."""
    I, F = rows_i, rows_f
    N = ist.shape[1]
    l2 = norm == "l2"
    judges = mode in ("clean", "start", "start_noise", "bisect", "probe", "step")
    for n in range(N):
        live = bool(ist[I["active"], n]) and bool(ist[I["has"], n])
        if mode == "begin":
            if ist[I["active"], n] and not ist[I["has"], n]:
                ist[I["active"], n] = 0
            if live:
                fst[F["lo"], n], fst[F["hi"], n], ist[I["moved"], n] = 0.0, (1.0 if l2 else np.float32(nrm[1, n])), 0
            continue
        if mode == "dist":
            t = int(ist[I["t"], n])
            if live:
                dist = np.float32(np.sqrt(nrm[0, n])) if l2 else np.float32(nrm[1, n])
                keep = bool(dist < fst[F["best"], n])
                if keep:
                    fst[F["best"], n] = dist
                r = fst[F["best"], n]
                fst[F["dist"], n], ist[I["keep"], n], ist[I["accept"], n] = dist, int(keep), 1
                d = np.float32(delta0) if t == 0 else dist * np.float32(inv_d)
                fst[F["delta"], n] = d if d > np.float32(dfloor) else np.float32(dfloor)
                if 0 <= t < len(xis):
                    fst[F["xi"], n] = dist * np.float32(xis[t])
                ist[I["stepdone"], n] = 0
            else:
                r = np.float32(0.0) if ist[I["done0"], n] else np.float32(np.inf)
                ist[I["keep"], n] = ist[I["accept"], n] = 0
            ist[I["pb"], n], fst[F["radius"], n] = 0, r
            if 0 <= t < history.shape[0]:
                history[t, n] = r
            ist[I["t"], n] = t + 1
            continue
        if mode == "vnorm":
            if live:
                fst[F["invn"], n] = (np.float32(1.0 / np.sqrt(nrm[0, n])) if nrm[0, n] > 0 else 0.0) if l2 else 1.0
            continue
        assert judges, mode
        row = np.asarray(logits[n], dtype=np.float32)
        valid = not bool(np.isnan(row).any())
        cls = int(row[0] > 0) if row.size == 1 else int(np.argmax(np.where(np.isnan(row), -np.inf, row)))
        if row.size > 1 and np.isnan(row[0]):
            cls = 0                                              # (the class of an invalid row is never used)
        bit = int(valid and cls != int(y[n]))
        ist[I["accept"], n] = 0
        if mode == "clean":
            part = True
            ist[I["queries"], n], ist[I["done0"], n], ist[I["active"], n], ist[I["has"], n] = 1, bit, 1 - bit, 0
            fst[F["best"], n], fst[F["radius"], n] = np.inf, (0.0 if bit else np.inf)
        elif mode in ("start", "start_noise"):
            part = bool(ist[I["active"], n]) and not bool(ist[I["has"], n])
            if part:
                ist[I["queries"], n] += 1
                if bit:
                    ist[I["has"], n] = ist[I["accept"], n] = 1
            if mode == "start_noise":
                ist[I["draw"], n] += 1
        elif mode == "bisect":
            part = live
            if part:
                ist[I["queries"], n] += 1
                mid = np.float32(0.5) * (fst[F["lo"], n] + fst[F["hi"], n])
                if bit:
                    fst[F["hi"], n], ist[I["moved"], n] = mid, 1
                else:
                    fst[F["lo"], n] = mid
        elif mode == "probe":
            part = live
            pb = int(ist[I["pb"], n])
            if part:
                ist[I["queries"], n] += 1
                if 0 <= pb < phi.shape[0]:
                    phi[pb, n] = bit
            ist[I["pb"], n] = pb + 1
            ist[I["draw"], n] += 1
        else:
            part = live and not bool(ist[I["stepdone"], n])
            if part:
                ist[I["queries"], n] += 1
                if bit:
                    ist[I["stepdone"], n] = ist[I["accept"], n] = 1
                else:
                    fst[F["xi"], n] = np.float32(0.5) * fst[F["xi"], n]
        if part and not valid:
            ist[I["flags"], n] |= 1
        k = int(ist[I["k"], n])
        if 0 <= k < decisions.shape[0]:
            decisions[k, n] = bit if part else -1
        ist[I["k"], n] = k + 1

"""TEST INFRASTRUCTURE — goldens for UniDefenseModelRes18 (BASELINE configs[0]: ResNet18 backbone, 128x128,
bs 8) recorded from the REFERENCE imported from /root/reference (this container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python -m oracle.make_golden_r18
Writes tests/golden/udr18_n8.npz: eval-mode outputs and train-mode outputs + pass-1 losses + all parameter
gradient norms/heads ('full' and 'smooth' loss variants, like make_golden.py).  Randomness is pinned by
injecting seeded keep-masks at the reference's three F.dropout sites (model/unidefense.py:391, :359, :406).
Seeds (42, 142): smallest top-2 gap in the dynamic filters' torch.max is 3.6e-4 for this batch.
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import ref_import, param_fill          # noqa: E402
from oracle.make_golden import LAMBDAS             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N, SIZE, IN_SEED, MASK_SEED, DROP = 8, 128, 42, 142, 0.5


def make_rng_r18(n, seed, drop_rate=DROP):
    g = torch.Generator().manual_seed(seed)

    def bern(shape, keep):
        return (torch.rand(shape, generator=g) < keep).float()
    return {"dec_keep": bern((n, 448, 16, 16), 0.8), "emb_keep": bern((n, 512, 8, 8), 1.0 - drop_rate),
            "feat_keep": bern((n, 512), 1.0 - drop_rate)}


def pack(out, store, prefix):
    ld = out["loss_dict"]
    store[prefix + "cls_out"] = out["cls_out"].detach().numpy()
    store[prefix + "rec_pool8"] = torch.nn.functional.adaptive_avg_pool2d(out["rec"].detach(), 8).numpy()
    store[prefix + "factorization"] = ld["factorization"].detach().numpy()[:, :64]
    for k in ("freq_mask", "spat_mask", "spatial", "freq"):
        store[prefix + k] = ld[k].detach().numpy()
    for i, t in enumerate(ld["triplet"]):
        store[prefix + f"triplet{i}"] = t.detach().numpy()


def main():
    os.makedirs(OUT, exist_ok=True)
    ref_model, ref_loss = ref_import.import_reference()
    torch.manual_seed(0)
    m = ref_model.load_model("UDR18")(extractor="resnet18", num_classes=2, drop_rate=DROP)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    x = param_fill.make_input(N, SIZE, seed=IN_SEED)
    tgt = param_fill.make_labels(N)
    rng = make_rng_r18(N, MASK_SEED)
    store = {}
    m.eval()
    with torch.no_grad():
        pack(m(x), store, "eval_")
    F = torch.nn.functional
    orig = F.dropout
    variants = (("full", LAMBDAS), ("smooth", dict(LAMBDAS, lambda_recons=0.0, lambda_freq=0.0)))
    # the train passes once more with the reference run in FLOAT64 (keys prefixed 'f64_'): the scalar sf_coef gradients are
    # sums with heavy cancellation whose fp32 value depends on the CPU's kernels, their float64 value does not
    for prefix, dt, (variant, lam) in [(p, d, v) for p, d in (("", torch.float32), ("f64_", torch.float64)) for v in variants]:
        m.to(dt)
        queue = [("dec_keep", 0.2), ("emb_keep", DROP), ("feat_keep", DROP)]

        def fake_dropout(inp, p=0.5, training=True, inplace=False):
            name, pp = queue.pop(0)
            assert abs(pp - p) < 1e-12 and training, (name, p, pp)
            scale = rng[name].to(inp.dtype) / (1.0 - p)
            return inp.mul_(scale) if inplace else inp * scale
        F.dropout = fake_dropout
        try:
            m.train()
            out = m(x.to(dt))
        finally:
            F.dropout = orig
        assert not queue
        ld = out["loss_dict"]
        n_real = N // 2
        trip = sum(ref_loss.LOSSES["aw_triplet"](f, tgt) for f in ld["triplet"])
        cls = ref_loss.LOSSES["cross_entropy"](out["cls_out"], tgt)
        real_rec = ld["spatial"].narrow(0, 0, n_real).mean()
        real_freq = ld["freq"].narrow(0, 0, n_real).mean()
        total = cls + lam["lambda_mask"] * (ld["freq_mask"].mean() + ld["spat_mask"].mean()) + \
            lam["lambda_triplet"] * trip + lam["lambda_recons"] * real_rec + lam["lambda_freq"] * real_freq
        m.zero_grad()
        total.backward()
        if variant == "full":
            pack(out, store, prefix + "train_")
        for k, v in (("total_loss", total), ("cls_loss", cls), ("triplet_loss", trip), ("real_rec_loss", real_rec),
                     ("real_freq_loss", real_freq)):
            store[f"{prefix}{variant}_loss_{k}"] = np.array(v.item())
        names, norms, heads = [], [], []
        for k, p in m.named_parameters():
            if p.grad is None:
                continue
            names.append(k)
            norms.append(p.grad.double().norm().item())
            h = torch.zeros(8, dtype=dt)
            f = p.grad.flatten()[:8]
            h[: f.numel()] = f
            heads.append(h.numpy())
        store["grad_names"] = np.array(names)
        store[f"{prefix}{variant}_grad_norms"] = np.array(norms)
        store[f"{prefix}{variant}_grad_heads"] = np.stack(heads)
    store["meta"] = np.array([N, SIZE, IN_SEED, MASK_SEED], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "udr18_n8.npz"), **store)
    print("wrote udr18_n8.npz", len(names), "grads")


if __name__ == "__main__":
    main()

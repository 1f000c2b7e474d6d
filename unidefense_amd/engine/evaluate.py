"""The evaluation stages behind TrainEngine.test / test_robust / test_corrupted / test_spatial / test_universal / test_patch / test_flow / test_band / test_certified / test_attribution: one scoring
forward, one batch source, one loop-and-gather, one metrics dictionary, and a table of test_robust's methods.  The Evaluator
takes its model and iterator as arguments and imports nothing that loads the HIP library, so the stage rules run on the CPU
against stubs (tests/test_evaluate_cpu.py, tests/test_universal_cpu.py).  What every stage keeps: its order inside a batch, who owns which generator, the sequence of
gather_scores calls (each is a pair of collectives under data parallel), every refusal before the first launch, and no
host-device synchronisation inside the batch loop — .cpu() / float() / bool() happen after it."""
from functools import partial

import torch

from . import metrics


class Evaluator:
    """model: what model(x) calls (wrapped under data parallel); net: the un-wrapped model, owner of the runner accessors;
    iterator(step, batch, size, device) -> (x_real, y_real, x_fake, y_fake); inference_graph / inference_precision: the
    engine's two config keys; local_rank: rank 0 prints."""

    def __init__(self, model, net, iterator, batch, size, device, inference_graph=False, inference_precision="fp32", local_rank=0):
        self.model, self.net, self.iterator, self.batch, self.size, self.device = model, net, iterator, batch, size, device
        self.graphed, self.precision, self.local_rank = bool(inference_graph), inference_precision, local_rank

    @torch.no_grad()
    def score(self, x):
        """p(real) = softmax(cls_out)[:, 0] (forgery_engine.py:349,437)"""
        # one hipGraph replay per batch, or the model's inference forward: no tape, running statistics
        forward = self.net.inference_runner(x.shape[0], x.shape[-1], self.precision) if self.graphed else self.model
        return torch.softmax(forward(x)["cls_out"], 1)[:, 0]

    def batches(self, n, first=1):
        for step in range(first, first + n):
            xr, yr, xf, yf = self.iterator(step, self.batch, self.size, self.device)
            yield torch.cat([xr, xf], 0).contiguous(), torch.cat([yr, yf], 0)

    def run(self, n, body, first=1):
        """body(x, y) -> {name: per-sample tensor} for each of n batches (the iterator's steps first .. first + n - 1) -> {name:
        (all batches of all ranks, their labels)}.  One gather_scores per name, in the order body names them (engine/metrics.py:
        two device all_gathers each)."""
        cols, labels = {}, []
        for x, y in self.batches(n, first):
            for name, t in body(x, y).items():
                cols.setdefault(name, []).append(t)
            labels.append(y)
        labels = torch.cat(labels)
        return {name: metrics.gather_scores(torch.cat(parts), labels) for name, parts in cols.items()}

    def metrics(self, scores, labels, tag):
        """what test() returns for gathered (scores, labels), its line printed as `tag`"""
        sc, lb = scores.float().cpu().numpy(), labels.cpu().numpy()
        ret = {"scores": scores.cpu(), "labels": labels.cpu(), "acc": float(((sc < 0.5).astype(int) == lb).mean())}
        if len(set(lb.tolist())) == 2:                     # a ROC needs both classes
            ret.update(metrics.cal_metrics(lb, sc, threshold=0.5))
            if self.local_rank == 0:
                print("%s | EER %.4f, HTER %.4f, TPR 5%% %.4f, AUC %.4f, ACC %.4f" % (
                    tag, ret["EER"], ret["ACER"], ret["TPR5%"], ret["AUC"], ret["ACC"]))
        return ret

    def _result(self, cols, tag, args):
        return {"clean": self.metrics(*cols["clean"], "Test"), "adv": self.metrics(*cols["adv"], tag), "attack": args}

    def test(self, batches):
        return self.metrics(*self.run(batches, lambda x, y: {"scores": self.score(x)})["scores"], "Test")

    def test_robust(self, batches, attack):
        if not attack:
            raise ValueError("test_robust needs an attack: pass attack={...} or set config['config']['attack']")
        attack = dict(attack)
        method = attack.pop("method", "pgd")
        if method not in ROBUST and method not in ROBUST_DECISION:
            names = [repr(name) for name in ROBUST]
            raise ValueError(f"attack method must be {', '.join(names[:-1])} or {names[-1]}, got {method!r}")
        # the run refuses what it does before any batch is drawn
        run = (ROBUST.get(method) or ROBUST_DECISION[method])(self, attack)
        cols = self.run(batches, run.body)
        return self._result(cols, "Test(adv)", run.attack(cols))

    def test_corrupted(self, batches, kinds, levels, seed, subsampling, corrupt=None, resolve=None):
        """corrupt / resolve: corrupt.corrupt / corrupt.resolve unless a caller (a CPU test) brings host stand-ins"""
        from .. import corrupt as CR
        corrupt, resolve = corrupt or CR.corrupt, resolve or CR.resolve
        kinds, levels = list(kinds) if kinds else list(CR.CORRUPTIONS), tuple(levels)
        resolved = {k: {lv: resolve(k, lv)[0][1] for lv in levels} for k in kinds}        # refuses before any kernel runs
        if subsampling not in CR.SUBSAMPLINGS:
            raise ValueError(f"subsampling must be one of {CR.SUBSAMPLINGS}, got {subsampling!r}")
        # one device generator per call, consumed batch-major, then in (kind, level) insertion order; one x_cor buffer for all
        generator = None if seed is None else torch.Generator(device=self.device).manual_seed(int(seed))
        keys, x_cor = dict.fromkeys((k, lv) for k in kinds for lv in levels), None

        def body(x, y):
            nonlocal x_cor
            clean = self.score(x)
            x_cor = torch.empty_like(x) if x_cor is None or x_cor.shape != x.shape else x_cor
            return {"clean": clean, **{(k, lv): self.score(corrupt(x, k, lv, generator=generator, subsampling=subsampling, out=x_cor))
                                       for k, lv in keys}}

        cols = self.run(batches, body)
        ret = {"clean": self.metrics(*cols["clean"], "Test"), "corrupted": {}, "mean": {}, "corruptions": resolved}
        for k in kinds:
            ret["corrupted"][k] = {lv: self.metrics(*cols[(k, lv)], "Test(%s %d)" % (k, lv)) for lv in levels}
            both = [r for r in ret["corrupted"][k].values() if "AUC" in r]
            if both:
                ret["mean"][k] = {m: float(sum(r[m] for r in both) / len(both)) for m in ("AUC", "ACC")}
                if self.local_rank == 0:
                    print("Corrupted %-14s | mean AUC %.4f, mean ACC %.4f | AUC by level %s" % (
                        k, ret["mean"][k]["AUC"], ret["mean"][k]["ACC"],
                        " ".join("%d:%.4f" % (lv, ret["corrupted"][k][lv]["AUC"]) for lv in levels if "AUC" in ret["corrupted"][k][lv])))
        return ret

    def test_spatial(self, batches, spatial):
        spatial = dict(spatial) if spatial else {}
        seed = spatial.pop("seed", None)
        generator = None if seed is None else torch.Generator().manual_seed(int(seed))     # one CPU generator per call
        runner = None

        def body(x, y):
            nonlocal runner
            try:                                         # the runner first, then the clean score; only the accessor is wrapped
                runner = self.net.spatial_runner(x.shape[0], x.shape[-1], **spatial)
            except TypeError as e:                       # an unknown key is a bad dict, like a bad value
                raise ValueError(f"spatial takes SpatialRunner's keyword arguments and 'seed': {e}") from None
            clean = self.score(x)
            adv = self.score(runner(x, y, generator))
            best = runner.best.to(self.device)           # gathered in this order: best's five columns, the two losses, the scores
            return {**{i: best[:, i] for i in range(5)}, "best_loss": runner.best_loss.clone(), "loss0": runner.loss0.clone(),
                    "clean": clean, "adv": adv}

        cols = self.run(batches, body)
        held = cols["loss0"][0] > 0
        args = dict(runner.args, best=torch.stack([cols[i][0] for i in range(5)], 1).cpu(),
                    fooled=float((cols["best_loss"][0][held] <= 0).double().mean()) if bool(held.any()) else float("nan"))
        return self._result(cols, "Test(spatial)", args)

    def test_universal(self, batches, fit_batches, epochs, universal):
        universal = dict(universal) if universal else {}
        seed = universal.pop("seed", None)
        for name, v in (("batches", batches), ("fit_batches", fit_batches), ("epochs", epochs)):
            if not v >= 1 or int(v) != v:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            universal.setdefault("reduce", dist.all_reduce)      # every rank sums gsum in place: the same delta everywhere
        try:                                             # ONE runner holds the pattern; every refusal before the first batch
            runner = self.net.universal_runner(2 * self.batch, self.size, **universal)
        except TypeError as e:                           # an unknown key is a bad dict, like a bad value
            raise ValueError(f"universal takes UniversalRunner's keyword arguments and 'seed': {e}") from None
        generator = None if seed is None else torch.Generator().manual_seed(int(seed))     # one CPU generator per call
        runner.reset()
        counted = []
        for _ in range(int(epochs)):                     # the fit: the iterator's steps 1 .. fit_batches, epochs times over
            for x, y in self.batches(int(fit_batches)):
                runner(x, y)
                counted.append(runner.counted.sum(1))
        # the control, drawn once: a pattern of the same norm that was fitted on nothing
        args = runner.args
        delta, (lo, hi) = runner.delta, args["clip"]
        if args["norm"] == "linf":
            sign = torch.randint(0, 2, tuple(delta.shape), generator=generator).to(torch.float32) * 2.0 - 1.0
            control = sign.to(delta.device) * args["eps"]
        else:
            z = torch.randn(tuple(delta.shape), generator=generator, dtype=torch.float32).to(delta.device)
            control = z * (delta.norm() / z.norm().clamp_min(1e-12))

        def body(x, y):                                  # the held-out steps, scored three ways, gathered in this order
            return {"clean": self.score(x), "adv": self.score(runner.apply(x)),
                    "control": self.score((x + control).clamp_(lo, hi))}

        cols = self.run(int(batches), body, first=int(fit_batches) + 1)
        labels = cols["clean"][1]
        right = (cols["clean"][0] < 0.5).long() == labels

        def fooled(name):
            wrong = (cols[name][0] < 0.5).long() != labels
            return float(wrong[right].double().mean()) if bool(right.any()) else float("nan")

        d = delta.detach().cpu()
        args = dict(args, delta=d, linf=float(d.abs().max()), l2=float(d.double().norm()), fooled=fooled("adv"),
                    fooled_control=fooled("control"), fit_counted=[int(c) for c in torch.cat(counted).cpu()])
        return dict(self._result(cols, "Test(universal)", args), control=self.metrics(*cols["control"], "Test(control)"))

    def test_patch(self, batches, fit_batches, epochs, patch, paste=None):
        """paste: patch.paste unless a caller (a CPU test) brings a host stand-in"""
        from .. import patch as PT
        patch = dict(patch) if patch else {}
        seed = patch.pop("seed", None)
        for name, v in (("batches", batches), ("fit_batches", fit_batches), ("epochs", epochs)):
            if not v >= 1 or int(v) != v:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            patch.setdefault("reduce", dist.all_reduce)          # every rank sums gsum in place: the same patch everywhere
        try:                                             # ONE runner holds the patch; every refusal before the first batch
            runner = self.net.patch_runner(2 * self.batch, self.size, **patch)
        except TypeError as e:                           # an unknown key is a bad dict, like a bad value
            raise ValueError(f"patch takes PatchRunner's keyword arguments and 'seed': {e}") from None
        paste = paste or PT.paste
        generator = None if seed is None else torch.Generator().manual_seed(int(seed))     # one CPU generator per call
        runner.reset()
        counted = []
        for _ in range(int(epochs)):                     # the fit: the iterator's steps 1 .. fit_batches, epochs times over
            for x, y in self.batches(int(fit_batches)):
                runner(x, y, generator)
                counted.append(runner.counted.sum(1))
        # the two controls, made once: a patch fitted on nothing, and one that only hides what is under it
        args = runner.args
        texture, alpha, (lo, hi) = runner.patch, runner.alpha, args["clip"]
        random = (torch.rand(tuple(texture.shape), generator=generator, dtype=torch.float32) * (hi - lo) + lo).to(texture.device)
        middle = torch.full_like(texture, 0.5 * (lo + hi))

        def body(x, y):                                  # the held-out steps, scored four ways at ONE draw of placements
            table = PT.patch_placements(x.shape[0], self.size, args["patch"], args["max_angle"], args["scales"], args["region"],
                                        generator)[1]
            return {"clean": self.score(x), "adv": self.score(runner.apply(x, table=table)),
                    "random": self.score(paste(x, random, table, alpha, (lo, hi))),
                    "occlusion": self.score(paste(x, middle, table, alpha, (lo, hi)))}

        cols = self.run(int(batches), body, first=int(fit_batches) + 1)
        labels = cols["clean"][1]
        right = (cols["clean"][0] < 0.5).long() == labels

        def fooled(name):
            wrong = (cols[name][0] < 0.5).long() != labels
            return float(wrong[right].double().mean()) if bool(right.any()) else float("nan")

        args = dict(args, texture=texture.detach().cpu(), fooled=fooled("adv"), fooled_random=fooled("random"),
                    fooled_occlusion=fooled("occlusion"), fit_counted=[int(c) for c in torch.cat(counted).cpu()])
        return dict(self._result(cols, "Test(patch)", args), random=self.metrics(*cols["random"], "Test(random patch)"),
                    occlusion=self.metrics(*cols["occlusion"], "Test(occlusion)"))

    def test_flow(self, batches, flow):
        flow = dict(flow) if flow else {}
        runner = None

        def body(x, y):
            nonlocal runner
            try:                                         # the runner first, then the clean score; only the accessor is wrapped
                runner = self.net.flow_runner(x.shape[0], x.shape[-1], **flow)
            except TypeError as e:                       # an unknown key is a bad dict, like a bad value
                raise ValueError(f"flow takes FlowRunner's keyword arguments: {e}") from None
            clean = self.score(x)
            adv = self.score(runner(x, y))
            # the runner reuses its buffers: the flow's two sizes are cloned per batch, and gathered ahead of the scores
            return {"flow_linf": runner.flow_linf.clone(), "flow_tv": runner.flow_tv.clone(), "clean": clean, "adv": adv}

        cols = self.run(batches, body)
        labels = cols["clean"][1]
        right = (cols["clean"][0] < 0.5).long() == labels
        wrong = (cols["adv"][0] < 0.5).long() != labels
        linf, tv = cols["flow_linf"][0].double(), cols["flow_tv"][0].double()
        args = dict(runner.args, flow_linf_mean=float(linf.mean()), flow_linf_max=float(linf.max()), flow_tv_mean=float(tv.mean()),
                    flow_tv_max=float(tv.max()), fooled=float(wrong[right].double().mean()) if bool(right.any()) else float("nan"))
        return self._result(cols, "Test(flow)", args)

    def test_band(self, batches, band, band_filter=None):
        """band_filter: band.band_filter unless a caller (a CPU test) brings a host stand-in"""
        from .. import band as BD
        band = dict(band) if band else {}
        bands = band.pop("bands", None)
        bands = list(BD.DEFAULT_BANDS if bands is None else bands)
        if not batches >= 1 or int(batches) != batches:
            raise ValueError(f"batches must be an integer >= 1, got {batches!r}")
        for key in ("band", "mask"):
            if key in band:
                raise ValueError(f"band takes BandRunner's keyword arguments and 'bands': the stage sets {key!r} itself, per band")
        if not bands or any(not isinstance(b, (tuple, list)) or len(b) != 2 for b in bands):
            raise ValueError(f"bands must be a list of (lo, hi) pairs, got {bands!r}")
        bands = [tuple(b) for b in bands]
        # every mask before any batch (a bad band or shape is refused here); the last is the control's: the full spectrum
        masks = [BD.band_mask(self.size, lo, hi, band.get("shape", "radial")).to(self.device) for lo, hi in bands]
        masks.append(torch.ones_like(masks[0]))
        clip = band.get("clip", (-1.0, 1.0))
        try:                                             # only the binding is wrapped: an unknown key is a bad dict, like a bad value
            BD._band_arguments(2 * self.batch, self.size, mask=masks[-1], **band)
        except TypeError as e:
            raise ValueError(f"band takes BandRunner's keyword arguments and 'bands': {e}") from None
        # ONE runner (one pair of graphs) for the control and every band, and for every later call with these arguments: it
        # owns its mask, and the stage refills it through set_mask before each attack
        runner = self.net.band_runner(2 * self.batch, self.size, mask=masks[-1], **band)
        band_filter = band_filter or BD.band_filter
        names = ["control"] + list(range(len(bands)))

        def body(x, y):                                  # clean; the control; then per band: attacked, leak, removed
            cols = {"clean": self.score(x)}
            for name, m in zip(names, masks[-1:] + masks[:-1]):
                runner.set_mask(m)
                cols[("adv", name)] = self.score(runner(x, y))
                cols[("leak", name)] = runner.leak.clone()           # the runner reuses its buffers
                if name != "control":
                    cols[("removed", name)] = self.score(band_filter(x, 1.0 - m, clip))
            return cols

        cols = self.run(int(batches), body)
        labels = cols["clean"][1]
        right = (cols["clean"][0] < 0.5).long() == labels

        def fooled(name):
            wrong = (cols[("adv", name)][0] < 0.5).long() != labels
            return float(wrong[right].double().mean()) if bool(right.any()) else float("nan")

        def row(name, tag):
            return {"adv": self.metrics(*cols[("adv", name)], "Test(%s)" % tag), "fooled": fooled(name),
                    "leak": float(cols[("leak", name)][0].double().mean())}

        ret = {"clean": self.metrics(*cols["clean"], "Test"), "control": row("control", "band control"), "bands": [],
               "attack": dict(runner.args, bands=bands)}
        for i, (lo, hi) in enumerate(bands):
            tag = "band %g-%s" % (lo, "inf" if hi is None else "%g" % hi)
            ret["bands"].append(dict(row(i, tag), band=(lo, hi), removed=self.metrics(*cols[("removed", i)], "Test(%s removed)" % tag)))
            if self.local_rank == 0:
                print("%-17s | fooled %.4f (control %.4f), leak %.3g" % (
                    tag.capitalize(), ret["bands"][i]["fooled"], ret["control"]["fooled"], ret["bands"][i]["leak"]))
        return ret

    def test_certified(self, batches, certify):
        from ..smooth import certified_curve
        certify = dict(certify) if certify else {}
        grid = certify.pop("grid", None)
        if not batches >= 1 or int(batches) != batches:
            raise ValueError(f"batches must be an integer >= 1, got {batches!r}")
        try:                                             # ONE runner for every batch; every refusal before the first batch
            runner = self.net.certify_runner(2 * self.batch, self.size, **certify)
        except TypeError as e:                           # an unknown key is a bad dict, like a bad value
            raise ValueError(f"certify takes CertifyRunner's keyword arguments and 'grid': {e}") from None
        args = dict(runner.args)
        grid = torch.linspace(0.0, 4.0 * args["sigma"], 9, dtype=torch.float64) if grid is None \
            else torch.as_tensor(grid, dtype=torch.float64).reshape(-1)
        if grid.numel() < 1 or not bool((torch.isfinite(grid) & (grid >= 0)).all()):
            raise ValueError(f"grid must hold finite radii >= 0, got {grid.tolist()}")
        dist = torch.distributed
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
        seen = 0

        def body(x, y):                                  # the clean score, then the certificate; gathered radius, predicted, clean
            nonlocal seen
            clean = self.score(x)
            # a stream id per sample of the whole run: the certificate does not depend on where the sample sits in its batch
            ids = torch.arange(x.shape[0], dtype=torch.int64, device=x.device) + (seen * world + rank) * x.shape[0]
            seen += 1
            radius = runner(x, ids)
            # the runner reuses its buffers: radius and predicted are cloned per batch
            return {"radius": radius.clone(), "predicted": runner.predicted.clone(), "clean": clean}

        cols = self.run(int(batches), body)
        labels = cols["clean"][1].cpu()
        radius, predicted = cols["radius"][0].float().cpu(), cols["predicted"][0].long().cpu()
        right = predicted == labels
        ret = {"args": args, "radius": radius, "predicted": predicted, "abstained": float((predicted < 0).double().mean()),
               "accuracy": float(right.double().mean()),
               "median_radius": float(radius[right].double().median()) if bool(right.any()) else float("nan"),
               "grid": grid, "certified_accuracy": certified_curve(radius, predicted, labels, grid)}
        clean = self.metrics(*cols["clean"], "Test")
        if self.local_rank == 0:
            print("Test(certified %s, sigma %g) | ACC %.4f, abstained %.4f, median radius %.4f | certified ACC %s" % (
                args["norm"], args["sigma"], ret["accuracy"], ret["abstained"], ret["median_radius"],
                " ".join("%.3g:%.4f" % (e, a) for e, a in zip(grid.tolist(), ret["certified_accuracy"].tolist()))))
        return {"clean": clean, "certify": ret}

    def test_attribution(self, batches, attribution, noise=None):
        """noise: kernels.smooth_noise unless a caller (a CPU test) brings a host stand-in"""
        attribution = dict(attribution) if attribution else {}
        fractions = attribution.pop("fractions", None)
        if not batches >= 1 or int(batches) != batches:
            raise ValueError(f"batches must be an integer >= 1, got {batches!r}")
        curve = {} if fractions is None else {"fractions": tuple(fractions)}
        n = 2 * self.batch
        try:                                             # ONE runner of each kind for every batch; every refusal before the first batch
            runner = self.net.attribution_runner(n, self.size, **attribution)
        except TypeError as e:                           # an unknown key is a bad dict, like a bad value
            raise ValueError(f"attribution takes AttributionRunner's keyword arguments and 'fractions': {e}") from None
        if runner.args["baseline"] == "given":
            raise ValueError("the attribution stage has no baseline tensor to pass: baseline must be 'black' or 'grey'")
        curves = {mode: self.net.deletion_runner(n, self.size, mode=mode, baseline=runner.args["baseline"],
                                                 precision=self.precision, **curve) for mode in ("deletion", "insertion")}
        if noise is None:
            from ..kernels import smooth_noise as noise
        args = dict(runner.args, fractions=curves["deletion"].args["fractions"])
        dist = torch.distributed
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
        seen = 0

        def body(x, y):                                  # clean, the map, its two curves, the random map's two curves
            nonlocal seen
            clean = self.score(x)
            # a stream id per sample of the whole run: neither the tunnel's noise nor the random map depends on rank or batch
            ids = torch.arange(x.shape[0], dtype=torch.int64, device=x.device) + (seen * world + rank) * x.shape[0]
            seen += 1
            runner(x, y, ids)
            # the runners reuse their buffers: every column is cloned per batch
            heat, gap, span = runner.heat.clone(), runner.gap.clone(), runner.f_x.double() - runner.f_b.double()
            zeros = torch.zeros(x.shape[0], x.shape[-1] * x.shape[-1], dtype=torch.float32, device=x.device)
            random = noise(zeros, torch.empty_like(zeros), ids, None, 0, "uniform", 1.0, args["seed"]).reshape(heat.shape)
            cols = {}
            for name, h in (("ig", heat), ("random", random)):
                for mode in ("deletion", "insertion"):
                    cols[(mode, name)] = curves[mode](x, y, h).clone()
            return {**cols, "gap": gap, "span": span, "clean": clean}

        cols = self.run(int(batches), body)
        gap, span = cols["gap"][0].double().cpu(), cols["span"][0].double().cpu()
        ret = {"clean": self.metrics(*cols["clean"], "Test"), "attribution": args,
               "gap_rel": gap.abs() / span.abs().clamp_min(torch.finfo(torch.float64).tiny)}
        for mode in ("deletion", "insertion"):
            each = {name: cols[(mode, name)][0].double().cpu() for name in ("ig", "random")}
            ret[mode + "_auc"] = {**{name: float(t.mean()) for name, t in each.items()}, "per_sample": each}
        if self.local_rank == 0:
            print("Test(attribution %s, %d steps) | deletion AUC ig %.4f random %.4f | insertion AUC ig %.4f random %.4f | "
                  "median relative gap %.3g" % (args["method"], args["steps"], ret["deletion_auc"]["ig"], ret["deletion_auc"]["random"],
                                                ret["insertion_auc"]["ig"], ret["insertion_auc"]["random"],
                                                float(ret["gap_rel"].median())))
        return ret


# ---- test_robust's methods: ROBUST[method](ev, attack) refuses and resolves the dict (given without "method") and is the run:
# body(x, y) -> the batch's columns, attack(cols) -> the result's "attack" entry ------------------------------------------------
class _Attack:
    """One runner per batch from the model's `accessor`.  draws: where the generator seeded by the dict's "seed" lives —
    "device" (Auto-PGD draws its restarts there), "cpu" (Square: the same draws on any machine), or None: "pgd" takes no
    generator and never pops "seed", so a seed in a PGD dict still reaches AttackRunner and is refused there."""

    def __init__(self, accessor, draws, ev, attack, seed=...):
        if seed is ...:                                  # not an ensemble's: the dict's own, popped before the runner sees the dict
            seed = attack.pop("seed", None) if draws else None
        self.ev, self.accessor, self.kwargs, self.runner, self.extra = ev, accessor, attack, None, (None,) if draws else ()
        if seed is not None:
            self.extra = (torch.Generator(device=ev.device if draws == "device" else "cpu").manual_seed(int(seed)),)

    def adv(self, x, y):
        self.runner = getattr(self.ev.net, self.accessor)(x.shape[0], x.shape[-1], **self.kwargs)
        return self.ev.score(self.runner(x, y, *self.extra))

    def body(self, x, y):
        clean = self.ev.score(x)                         # the clean batch is scored before the model is asked for a runner
        return {"clean": clean, "adv": self.adv(x, y)}

    def attack(self, cols=None):
        return dict(self.runner.args)


class _Ensemble:
    """{name: {...} for each of the two members, "seed": ...}: both start from the clean batch, on generators seeded from the
    one "seed"; each sample keeps the score with the lower probability of its true label."""

    def __init__(self, names, ev, attack):
        seed, self.ev, self.method = attack.pop("seed", None), ev, "+".join(names)
        if set(attack) != set(names):
            takes = ", ".join("%r: {...}" % name for name in names)
            raise ValueError(f"attack method {self.method!r} takes {{{takes}, 'seed': ...}}, got the keys {sorted(attack)}")
        self.runs = {name: ROBUST[name](ev, dict(attack[name]), seed) for name in names}

    def body(self, x, y):
        clean = self.ev.score(x)
        s, s2 = [run.adv(x, y) for run in self.runs.values()]        # in the table's order: Auto-PGD runs and is scored before Square
        # the score is P(class 0): the true label's probability is lower where it is lower for y == 0, higher otherwise
        return {"clean": clean, "adv": torch.where(y == 0, torch.minimum(s, s2), torch.maximum(s, s2))}

    def attack(self, cols=None):
        return {"method": self.method, **{name: run.attack() for name, run in self.runs.items()}}


class _MinNorm:
    """"fmn" / "sparse_fmn" by the model's accessor, plus an optional "eps": "adv" is scored on x_adv where the attack flipped
    the sample within eps (found and radius <= eps; eps absent: every found sample) and on the clean input elsewhere."""

    def __init__(self, accessor, ev, attack):
        self.eps = attack.pop("eps", None)
        if self.eps is not None and not float(self.eps) >= 0.0:          # before any batch is drawn
            raise ValueError(f"eps must be >= 0, got {self.eps!r}")
        self.ev, self.accessor, self.kwargs, self.runner = ev, accessor, attack, None

    def body(self, x, y):
        clean = self.ev.score(x)
        runner = self.runner = getattr(self.ev.net, self.accessor)(x.shape[0], x.shape[-1], **self.kwargs)
        xa = runner(x, y)
        take = runner.found.bool() if self.eps is None else runner.found.bool() & (runner.radius <= float(self.eps))
        adv = self.ev.score(torch.where(take.reshape(-1, 1, 1, 1), xa, x))
        # the runner reuses its buffers: radius and found are cloned per batch, and gathered ahead of the scores
        return {"radius": runner.radius.clone(), "found": runner.found.clone(), "clean": clean, "adv": adv}

    def attack(self, cols):
        radius, found = cols["radius"][0].float().cpu(), cols["found"][0].to(torch.int32).cpu()
        return dict(self.runner.args, eps=None if self.eps is None else float(self.eps), radius=radius, found=found,
                    median_radius=float(radius.double().median()) if radius.numel() else float("nan"))


class _HSJ(_MinNorm):
    """"hsj": HopSkipJump from the hard label, scored like "fmn" (found, radius <= eps).  Each sample's x_init is the next
    batch-mate in cyclic order whose clean prediction differs from the sample's label (chosen from the clean scoring forward;
    none: the runner falls back to its noise trials); ids come from (batch index, rank, row), as test_certified's streams do."""

    def __init__(self, ev, attack):
        super().__init__("hsj_runner", ev, attack)
        from ..hsj import _hsj_arguments
        try:                                             # an unknown key is a bad dict, like a bad value: before any batch is drawn
            _hsj_arguments(2 * ev.batch, ev.size, **attack)
        except TypeError as e:
            raise ValueError(f"attack method 'hsj' takes HSJRunner's keyword arguments and 'eps': {e}") from None
        dist = torch.distributed
        self.rank, self.world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
        self.seen = 0

    def body(self, x, y):
        clean = self.ev.score(x)
        runner = self.runner = self.ev.net.hsj_runner(x.shape[0], x.shape[-1], **self.kwargs)
        n = x.shape[0]
        pred = (clean < 0.5).long()                      # the label test() scores: 1 where p(real) < 0.5
        mate = (torch.arange(n, device=x.device).reshape(-1, 1) + torch.arange(1, n + 1, device=x.device).reshape(1, -1)) % n
        differs = pred[mate] != y.reshape(-1, 1)         # [sample, offset]: the first True is the next such batch-mate
        first = differs.to(torch.int32).argmax(1)        # no True: offset n - 1 + 1 = the sample itself, which is no start
        first = torch.where(differs.any(1), first, torch.full_like(first, n - 1))
        x_init = x[mate[torch.arange(n, device=x.device), first]].contiguous()
        ids = torch.arange(n, dtype=torch.int64, device=x.device) + (self.seen * self.world + self.rank) * n
        self.seen += 1
        radius = runner(x, y, ids, x_init)
        take = runner.found if self.eps is None else runner.found & (radius <= float(self.eps))
        adv = self.ev.score(torch.where(take.reshape(-1, 1, 1, 1), runner.x_adv, x))
        # the runner reuses its buffers: radius and found are cloned per batch, and gathered ahead of the scores
        return {"radius": radius.clone(), "found": runner.found.clone(), "clean": clean, "adv": adv}


ROBUST = {"pgd": partial(_Attack, "attack_runner", None), "apgd": partial(_Attack, "apgd_runner", "device"),
          "square": partial(_Attack, "square_runner", "cpu"), "apgd+square": partial(_Ensemble, ("apgd", "square")),
          "fmn": partial(_MinNorm, "fmn_runner"), "sparse_fmn": partial(_MinNorm, "sparse_fmn_runner")}
# the decision-based member, in a table of its own: ROBUST stays the list of the score- and gradient-based methods
ROBUST_DECISION = {"hsj": _HSJ}



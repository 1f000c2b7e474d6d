"""Concrete engine behind ``engine.get_engine`` (reference: engine/forgery_engine.py, ocim_engine.py,
uniattack_engine.py — three copies of one train loop around AbstractEngine.train_unidefense_model that differ in
their dataset / metric / wandb plumbing, which is out of scope here, SURVEY.md §8 b / §5).

What this mirrors of the reference (file:line of forgery_engine.py):
  * config layout: ``config['model']`` = model name + ctor kwargs (:141), ``config['config']`` = optimizer / scheduler /
    warmup_step / lambda_* / local_rank (:133-160), ``config['data']['train_batch_size']`` = samples per class and rank;
  * model -> SyncBN + data parallel (:142-146; here HipDataParallel over RCCL when a process group exists),
    timm weight-decay groups + optimizer (:149-154), scheduler (:156), the four loss criteria (:157-162);
  * train(): zero_grad, one [real...; fake...] batch per step from two sources, linear lr warm-up (:271-274),
    train_unidefense_model, loss / accuracy trackers reduced over ranks (:279-287), a log line every log_steps.
What replaces the dataset classes: ``config['data']['iterator']`` — a callable ``(step, batch, size, device) ->
(images_real, labels_real, images_fake, labels_fake)``; without one, seeded synthetic batches of the configured size
(there is no dataset in this image).  test(): accuracy / real-class scores over ``config['data']['test_iterator']``
(or synthetic batches) with the inference forward — the reference's ROC metrics stay out.  Checkpoints: the reference's
file names and format (engine/checkpoint.py); ``config['config']['dir']`` enables the save at the end of train(),
``resume`` the load at construction.
"""
import os

import torch
import torch.distributed as dist

from ..loss import get_loss
from ..model import load_model
from .abstract_engine import AbstractEngine
from .checkpoint import load_checkpoint, save_checkpoint
from .evaluate import Evaluator
from .optim import build_optimizer, build_scheduler
from .parallel import wrap_data_parallel


def synthetic_batches(seed=0):
    """Default data source: x = 2*U(0,1)-1 faces, labels 0 = real, 1 = fake."""
    def it(step, batch, size, device):
        g = torch.Generator().manual_seed(seed * 1000003 + step)
        real = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
        fake = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
        return (real.to(device), torch.zeros(batch, dtype=torch.long, device=device),
                fake.to(device), torch.ones(batch, dtype=torch.long, device=device))
    return it


class TrainEngine(AbstractEngine):
    path = "engine/train_engine.py"

    def __init__(self, config, stage="Train"):
        super().__init__(config, stage)
        if not torch.cuda.is_available():
            raise RuntimeError("unidefense_amd engines run on an MI355X GPU only (no CPU path)")
        cfg = config["config"]
        self.local_rank = int(cfg.get("local_rank", os.environ.get("LOCAL_RANK", 0)))
        self.device = torch.device(f"cuda:{self.local_rank}")
        torch.cuda.set_device(self.device)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
            dist.init_process_group(cfg.get("distribute", {}).get("backend", "nccl"), device_id=self.device)
        model_cfg = dict(config["model"])
        self.model_name = model_cfg.pop("name")
        data_cfg = config.get("data", {})
        self.batch = int(data_cfg.get("train_batch_size", 16))
        self.size = int(data_cfg.get("size", 256))
        self.num_steps = int(cfg.get("num_steps", data_cfg.get("num_steps", 100)))
        self.log_steps = int(cfg.get("log_steps", data_cfg.get("log_steps", 50)))
        self.warmup_step = int(cfg.get("warmup_step", 0))
        self.train_iterator = data_cfg.get("iterator") or synthetic_batches(self.local_rank)
        self.test_iterator = data_cfg.get("test_iterator") or synthetic_batches(10007 + self.local_rank)

        self.best_step, self.best_auc, self.best_acc = 1, 0., 0.                    # forgery_engine.py:159-161
        self.model = load_model(self.model_name)(**model_cfg).to(self.device)
        # config.precision: "fp32" (default: fp32-accurate GEMMs, the reference's arithmetic) or "fp16" — BASELINE
        # configs[4]: fp16 MFMA operands with fp32 accumulation in every GEMM (ud_gemm path 3, process-wide) and, on the
        # EfficientNet model, fp16 storage of the MBConv trunk's activations; the GradScaler below is what keeps the half
        # gradients in range.  The reference has no such mode (autocast(enabled=False), abstract_engine.py:208).
        self.precision = str(cfg.get("precision", "fp32")).lower()
        if self.precision not in ("fp32", "fp16"):
            raise ValueError(f"config.precision must be 'fp32' or 'fp16', got {self.precision!r}")
        # The GEMM path is process-wide state of the library: an fp16 engine wants the fp16-MFMA kernel (3), an fp32 engine the
        # path in force when it is built (the library's UD_GEMM_PATH default or a caller's ud_gemm_set_path; never another engine's 3).  Building an engine does not touch it (an engine that still
        # lives keeps its arithmetic); each engine selects its own on entry to train() / test() / validate() / train_unidefense_model(), so two engines
        # of different precision in one process (an A/B run, a notebook) each compute in theirs.
        from .. import lib as _lib
        cur = _lib.call("ud_gemm_get_path")          # what the process (UD_GEMM_PATH at load) or a caller's ud_gemm_set_path chose
        self._gemm_path = 3 if self.precision == "fp16" else (cur if cur != 3 else 0)
        if self.precision == "fp16":
            self.model.half_storage = True
        self.model_without_ddp = self.model
        if dist.is_available() and dist.is_initialized():
            self.model = wrap_data_parallel(self.model, self.local_rank)           # SyncBN + gradient exchange
        if self.config["config"].get("resume"):
            # the test stage evaluates best_model.bin (forgery_engine.py:202), training resumes from latest_model.bin
            best = stage == "Test" and os.path.exists(self._ckpt_path(best=True))
            if os.path.exists(self._ckpt_path(best)):
                meta = self._load_ckpt(best=best, train=stage == "Train")
                self.best_step = int(meta.get("best_step", self.best_step) or self.best_step)
                self.best_auc = float(meta.get("best_auc", self.best_auc) or self.best_auc)
                self.best_acc = float(meta.get("best_acc", self.best_acc) or self.best_acc)
        if stage == "Train":
            self.base_lr = float(cfg["optimizer"]["lr"])
            self.optimizer = build_optimizer(self.model_without_ddp, cfg["optimizer"])
            self.scheduler = build_scheduler(self.optimizer, cfg.get("scheduler"))
            self.loss_criterion = {"softmax": get_loss("cross_entropy", self.device),
                                   "triplet": get_loss("aw_triplet", self.device),
                                   "kl_div": get_loss("kl_div", self.device),
                                   "fac": get_loss("factorization", self.device)}

    # ---- checkpoints in the reference's file names / format (forgery_engine.py:215-223) ------------------------------
    def _ckpt_path(self, best=False):
        return os.path.join(self.config["config"].get("dir", "."), "best_model.bin" if best else "latest_model.bin")

    def _any_rank(self, flag):
        """True on every rank iff `flag` is true on at least one (a no-op without a process group): decisions that guard a
        collective are taken from this, never from rank-local state such as the file system."""
        if not (dist.is_available() and dist.is_initialized()):
            return bool(flag)
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return bool(t.item())

    def _check_exchange(self):
        """A SyncBN peer exchange that timed out has poisoned this step's statistics (NaN): raise before anything is
        logged, validated or saved from them — on EVERY rank together, so that no rank is left waiting in the barrier /
        all_reduce that follows while another has already raised."""
        exchange = getattr(self.model, "bn_exchange", None)
        err = None
        if exchange is not None:
            try:
                exchange.check()
            except Exception as e:          # noqa: BLE001 — re-raised below, after the ranks have agreed
                err = e
        if self._any_rank(err is not None):
            raise err if err is not None else RuntimeError("SyncBN peer exchange failed on another rank")

    def _save_ckpt(self, step, best=False):
        self._check_exchange()
        if self.local_rank == 0:
            save_checkpoint(self.model_without_ddp, self._ckpt_path(best), step, self.best_step, self.best_auc,
                            self.best_acc)
        if dist.is_available() and dist.is_initialized():
            dist.barrier()              # the other ranks start the next step together with the writer (forgery_engine.py:219)

    def _load_ckpt(self, best=False, train=False):
        return load_checkpoint(self.model_without_ddp, self._ckpt_path(best))

    # ------------------------------------------------------------------------------------------------------------
    def _mean_over_ranks(self, values):
        t = torch.stack([v.detach().float().reshape(()) for v in values])
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(t)                      # one packed metric exchange per log step
            t /= dist.get_world_size()
        return t.tolist()

    def _select_gemm_path(self):
        from .. import lib as _lib
        if _lib.call("ud_gemm_get_path") != self._gemm_path:
            _lib.call("ud_gemm_set_path", self._gemm_path)

    def train(self):
        try:
            self._select_gemm_path()
            grad_scalar = torch.amp.GradScaler("cuda", init_scale=2 ** 10)        # forgery_engine.py:228
            sums, count, correct, seen, last = {}, 0, 0, 0, {}
            for cur_step in range(1, self.num_steps + 1):
                self.model.train()
                self.optimizer.zero_grad()
                xr, yr, xf, yf = self.train_iterator(cur_step, self.batch, self.size, self.device)
                in_data, in_tgt = torch.cat([xr, xf], 0).contiguous(), torch.cat([yr, yf], 0)
                if self.warmup_step != 0 and cur_step <= self.warmup_step:           # :271-274
                    for group in self.optimizer.param_groups:
                        group["lr"] = self.base_lr * float(cur_step) / self.warmup_step
                out = self.train_unidefense_model(in_data, in_tgt, cur_step, grad_scalar, yr.shape[0], yf.shape[0])
                for k, v in out.items():
                    if "loss" in k:
                        sums[k] = sums.get(k, 0.0) + v.detach()
                count += 1
                correct += (out["cls_out"].argmax(1) == in_tgt).sum()
                seen += in_tgt.numel()
                if cur_step % self.log_steps == 0 or cur_step == self.num_steps:
                    self._check_exchange()       # SyncBN peer exchange: a missing rank surfaces here, not as a silent NaN
                    keys = sorted(sums)
                    vals = self._mean_over_ranks([sums[k] / count for k in keys] + [correct / seen])
                    last = dict(zip(keys, vals[:-1]))
                    last["acc"], last["lr"], last["step"] = vals[-1], self.optimizer.param_groups[0]["lr"], cur_step
                    if self.local_rank == 0:
                        print("Train Iter (%d/%d), Loss %.4f, Triplet %.4f, Spat %.4f, Freq %.4f, ACC %.4f, LR %.6f" % (
                            cur_step, self.num_steps, last.get("total_loss", 0.0), last.get("triplet_loss", 0.0),
                            last.get("real_rec_loss", 0.0), last.get("real_freq_loss", 0.0), last["acc"], last["lr"]))
            if self.config["config"].get("dir"):
                # best_model.bin (what the reference's test stage reads, forgery_engine.py:202-207) is validate()'s to
                # choose, by validation AUC + ACC.  Only a run that never validated — no best file, no best record — gets
                # its final weights there, with the TRAIN accuracy of the last log window kept apart from the validation
                # record (best_auc / best_acc are validation numbers).
                self.last_train_acc = float(last.get("acc", 0.0))
                # (_save_ckpt ends in a barrier: the decision is rank 0's, broadcast — a rank that stats the directory a
                # moment after rank 0 created the file must not skip a barrier the others run)
                has_best = self._any_rank(self.local_rank == 0 and os.path.exists(self._ckpt_path(best=True)))
                if self.best_auc == 0.0 and self.best_acc == 0.0 and not has_best:
                    self.best_step = self.num_steps
                    self._save_ckpt(self.num_steps, best=True)
                self._save_ckpt(self.num_steps)
            return last
        except Exception:
            if dist.is_available() and dist.is_initialized():                          # :315-318
                dist.destroy_process_group()
            raise

    # ---- the evaluation stages: engine/evaluate.py runs them, these methods are their config defaults and contracts ---------
    def _evaluator(self):
        """This engine's GEMM path and eval mode, then the Evaluator.  config['config']['inference_graph'] (default false): the scoring
        forward replays the model's InferenceRunner graph (infer.py); 'inference_precision' ("fp32" default, "fp16"): that runner's."""
        self._select_gemm_path()
        self.model.eval()
        cfg = self.config["config"]
        return Evaluator(self.model, self.model_without_ddp, self.test_iterator, self.batch, self.size, self.device,
                         cfg.get("inference_graph", False), cfg.get("inference_precision", "fp32"), self.local_rank)

    def test(self, batches=4):
        """The reference's test stage (forgery_engine.py:423-452): p(real) = softmax(cls_out)[:, 0] of `batches` test batches
        (:349,437), gathered over the ranks with two device all_gathers (engine/metrics.py:gather_scores replaces
        dist.all_gather_object, :374-375) -> cal_metrics (EER, HTER = ACER, TPR@5 %, AUC, ACC, ...) over the frames of all ranks."""
        return self._evaluator().test(batches)

    def test_robust(self, batches=4, attack=None):
        """test() on clean and on attacked inputs: every test batch is scored as test() does, attacked with the true labels by
        the model's AttackRunner (unidefense_amd/attack.py) and scored again the same way.  attack (default
        config['config']['attack']): the runner's keyword arguments, e.g. {"norm": "linf", "eps": 4/255, "steps": 10} — eps in
        model-input units (after Normalize(0.5, 0.5) one 8-bit grey level is 2/255).  Returns {"clean": what test() returns,
        "adv": the same keys on x_adv, "attack": the resolved arguments, precision and grad_scale included}.  The attack dict's
        "precision": "fp16" (UDEB4; optional "grad_scale") runs the attack's frozen pass in half storage; inference_graph /
        inference_precision keep their meaning for the two scoring forwards.  Data parallel: each rank attacks its own batches on the un-wrapped model (a
        frozen pass has no collective of its own) and the scores are gathered over the ranks as in test().
        "method": "apgd" in the attack dict selects Auto-PGD (the model's APGDRunner: norm, eps, steps, restarts, rho, alpha, ...;
        an optional "seed" seeds the generator of its random restarts); "pgd", the default, is the fixed-step AttackRunner.
        "method": "square" selects the black-box Square attack (the model's SquareRunner: eps, steps, p_init, restarts, ...; an
        optional "seed" seeds the CPU generator of its draws).  "method": "apgd+square" takes {"apgd": {...}, "square": {...},
        "seed": ...}: both attacks start from the clean batch, both results are scored, and each sample keeps the score with the
        lower probability of its true label (the worst case over the ensemble); "attack" then holds both resolved dicts.
        "method": "fmn" selects the minimum-norm attack (the model's FMNRunner: norm, steps, alpha_init, gamma_init, ...) plus an
        optional "eps": "adv" is scored on x_adv for the samples the attack flipped within eps (found and radius <= eps; eps absent:
        every found sample) and on the clean input for the rest; "attack" then also holds "eps", "radius" (CPU tensor), "found"
        (CPU tensor) and "median_radius", gathered over the ranks in the scores' order (robust_curve(radius, grid) gives the
        robust accuracy at every eps from this one run).  "method": "sparse_fmn" is the same path on the model's SparseFMNRunner
        (norm "l1": radius and eps are sums of |x_adv - x|; "l0": numbers of changed elements).
        "method": "hsj" selects the decision-based minimum-norm attack (the model's HSJRunner, unidefense_amd/hsj.py: norm "l2" /
        "linf", steps, probes, max_probes, bisect, halvings, init_trials, seed, ...), which sees the hard label only; it is scored
        like "fmn" ("eps", "radius", "found", "median_radius").  Each sample starts from the next batch-mate (cyclic) whose clean
        prediction differs from the sample's label, or from the runner's noise trials where the batch holds none; the noise
        streams are keyed by (batch index, rank, row), so a sample's attack does not depend on the rank count."""
        return self._evaluator().test_robust(batches, attack if attack is not None else self.config["config"].get("attack"))

    def test_corrupted(self, batches=4, corruptions=None, levels=(1, 2, 3, 4, 5), seed=None, subsampling="420"):
        """test() on clean and on commonly corrupted inputs (unidefense_amd/corrupt.py): every test batch is scored as test()
        does (inference_graph / inference_precision keep their meaning), then once per (kind, level) on corrupt(x, kind, level) —
        one extra launch in front of the same scoring forward.  corruptions (default config['config']['corruptions'], then all
        seven): names of corrupt.CORRUPTIONS; levels: severities 1..5; seed: seeds the device generator of the noise fields and
        block positions; subsampling: JPEG's chroma format.  Returns {"clean": what test() returns, "corrupted": {kind: {level:
        the same keys}}, "mean": {kind: {"AUC", "ACC"}} averaged over the levels (where both classes are present),
        "corruptions": {kind: {level: the resolved parameter}}}.  Scores are gathered over the ranks as in test()."""
        kinds = corruptions if corruptions is not None else self.config["config"].get("corruptions")
        return self._evaluator().test_corrupted(batches, kinds, levels, seed, subsampling)

    def test_spatial(self, batches=4, spatial=None):
        """test() on clean inputs and on each sample's worst spatial candidate (unidefense_amd/spatial.py): every test batch is
        scored as test() does (inference_graph / inference_precision keep their meaning), searched with the true labels by the
        model's SpatialRunner and scored again the same way on its x_adv.  spatial (default config['config']['spatial'], then the
        runner's defaults): the runner's keyword arguments, e.g. {"max_angle": 10.0, "max_shift": 0.05, "grid": (7, 5, 3)}; an
        optional "seed" seeds the CPU generator of a random search.  Returns {"clean": what test() returns, "adv": the same keys on
        x_adv, "attack": the resolved arguments plus "best" (CPU [n, 5]: each sample's (angle, dx, dy, scale, flip)) and "fooled"
        (the fraction with best_loss <= 0 among the samples with loss0 > 0; NaN where there are none)}.  Scores, best and the
        two losses are gathered over the ranks as in test()."""
        return self._evaluator().test_spatial(batches, spatial if spatial is not None else self.config["config"].get("spatial"))

    def test_universal(self, batches=4, fit_batches=4, epochs=2, universal=None):
        """What ONE pattern of size eps costs on data it was not fitted on (unidefense_amd/universal.py): the model's
        UniversalRunner is reset and fitted on the test iterator's steps 1 .. fit_batches, `epochs` times over, with the true
        labels; the held-out steps fit_batches + 1 .. fit_batches + batches are then scored as test() does (inference_graph /
        inference_precision keep their meaning) three ways: clean, with the pattern (runner.apply), and with a control pattern
        of the same norm fitted on nothing (linf: random +-eps; l2: a Gaussian scaled to |delta|_2), drawn once from a CPU
        generator.  universal (default config['config']['universal']): the runner's keyword arguments, e.g. {"norm": "linf",
        "eps": 4/255, "steps": 1}; an optional "seed" seeds the control's generator.  Returns {"clean", "adv", "control": what
        test() returns, "attack": the resolved arguments plus "delta" (CPU [3, size, size]), "linf", "l2", "fooled" (the fraction
        of the held-out samples classified correctly clean that the pattern flips; NaN where there are none), "fooled_control"
        and "fit_counted" (the samples that steered each fit iteration, this rank's)}.  Under data parallel every rank's
        gradient sum is all-reduced inside the iteration, so all ranks hold the same pattern; scores are gathered as in
        test(), in the order clean, adv, control."""
        universal = universal if universal is not None else self.config["config"].get("universal")
        return self._evaluator().test_universal(batches, fit_batches, epochs, universal)

    def test_patch(self, batches=4, fit_batches=4, epochs=2, patch=None):
        """What ONE sticker costs wherever it lands (unidefense_amd/patch.py): the model's PatchRunner is reset and fitted on the
        test iterator's steps 1 .. fit_batches, `epochs` times over, with the true labels, at freshly drawn placements; the
        held-out steps fit_batches + 1 .. fit_batches + batches are then scored as test() does (inference_graph /
        inference_precision keep their meaning) four ways, all at the SAME freshly drawn placements: clean, with the fitted patch
        (runner.apply), with a uniform-random patch, and with a constant mid-range patch, which is plain occlusion.  patch
        (default config['config']['patch']): the runner's keyword arguments, e.g. {"patch": 48, "shape": "circle", "steps": 1};
        an optional "seed" seeds the one CPU generator of the placements and the random control.  Returns {"clean", "adv",
        "random", "occlusion": what test() returns, "attack": the resolved arguments (with "area", the patch's nominal share
        of the image) plus "texture" (CPU [3, P, P]), "fooled" (the fraction of the held-out samples classified correctly clean
        that the patch flips; NaN where there are none), "fooled_random", "fooled_occlusion" and "fit_counted" (the samples that
        steered each fit iteration, this rank's)}.  Under data parallel every rank's gradient sum is all-reduced inside the
        iteration, so all ranks hold the same patch; scores are gathered as in test(), in the order clean, adv, random,
        occlusion."""
        patch = patch if patch is not None else self.config["config"].get("patch")
        return self._evaluator().test_patch(batches, fit_batches, epochs, patch)

    def test_flow(self, batches=4, flow=None):
        """test() on clean inputs and on each sample's flow-field (stAdv) adversarial image (unidefense_amd/flow.py): every test
        batch is scored as test() does (inference_graph / inference_precision keep their meaning), attacked with the true labels
        by the model's FlowRunner — a per-pixel displacement field of at most max_flow pixels, ascended through a differentiable
        warp — and scored again the same way on its x_adv.  flow (default config['config']['flow'], then the runner's defaults):
        the runner's keyword arguments, e.g. {"max_flow": 2.0, "steps": 20, "tau": 0.05}.  Returns {"clean": what test() returns,
        "adv": the same keys on x_adv, "attack": the resolved arguments plus "flow_linf_mean" / "flow_linf_max" and "flow_tv_mean"
        / "flow_tv_max" (the best flows' largest displacement and smoothness term) and "fooled" (the fraction of the samples
        classified correctly clean that the flow flips; NaN where there are none)}.  The flows' two sizes and the scores are
        gathered over the ranks as in test(), in this order."""
        return self._evaluator().test_flow(batches, flow if flow is not None else self.config["config"].get("flow"))

    def test_band(self, batches=4, band=None):
        """In which frequency band the model is fragile (unidefense_amd/band.py): every test batch is scored as test() does
        (inference_graph / inference_precision keep their meaning), then attacked with the true labels by the model's BandRunner
        — L2 PGD whose perturbation is confined to one band of the image's 2-D DCT — once per band at the SAME eps, and once with
        a mask of ones: the full-spectrum control, which is plain L2 PGD.  Per band the batch is also scored with the band REMOVED
        and nothing attacked (band_filter(x, 1 - mask)).  band (default config['config']['band']): the runner's keyword arguments,
        e.g. {"eps": 1.0, "steps": 10, "shape": "radial"}, plus "bands", a list of (lo, hi) in cycles per pixel over the DCT's
        [0, 1) axis (default [(0, 1/8), (1/8, 1/4), (1/4, 1/2), (1/2, None)]); "precision": "fp16" (UDEB4) runs the attack's
        frozen pass in half storage.  One runner serves every band: it owns its mask and the stage refills it (set_mask).  Returns {"clean": what
        test() returns, "control": {"adv": the same keys on the control's x_adv, "fooled": the fraction of the samples classified
        correctly clean that it flips (NaN where there are none), "leak": the mean share of |x_adv - x|^2 outside the band after
        the clip}, "bands": one such row per band plus "band" and "removed" (test()'s keys with the band filtered out), "attack":
        the resolved arguments and "bands"}.  Scores are gathered over the ranks as in test(): clean, then the control's and
        each band's columns in order."""
        return self._evaluator().test_band(batches, band if band is not None else self.config["config"].get("band"))

    def test_certified(self, batches=4, certify=None):
        """A LOWER bound on robustness, where test_robust gives upper bounds (unidefense_amd/smooth.py): every test batch is scored
        as test() does (inference_graph / inference_precision keep their meaning), then certified by the model's CertifyRunner —
        n0 + n noisy forwards per batch, no labels.  certify (default config['config']['certify'], then the runner's defaults):
        the runner's keyword arguments, e.g. {"sigma": 0.25, "noise": "gaussian", "n0": 100, "n": 1000, "alpha": 0.001}, plus an
        optional "grid" of radii (default: nine points from 0 to 4 sigma).  Returns {"clean": what test() returns, "certify": the
        resolved "args", "radius" and "predicted" (CPU, -1: abstained), "abstained" (a fraction), "accuracy" (predicted == label;
        an abstention is wrong), "median_radius" over the correct samples, "grid" and "certified_accuracy" (per grid point the
        fraction classified correctly and certified beyond it)}.  Sample i of rank r's batch b draws the noise stream
        (b world + r) 2 batch + i; radius, predicted and the scores are gathered over the ranks as in test(), in this order."""
        return self._evaluator().test_certified(batches, certify if certify is not None else self.config["config"].get("certify"))

    def test_attribution(self, batches=4, attribution=None):
        """Which pixels the decisions rest on, and whether that map means anything (unidefense_amd/attrib.py): every test batch is
        scored as test() does, attributed by the model's AttributionRunner (integrated gradients by default), and the map is scored
        by its deletion and insertion curves (DeletionRunner) next to those of a RANDOM map — uniform noise keyed by the sample's
        stream id, so no torch generator is drawn.  attribution (default config['config']['attribution'], then the runner's
        defaults): the runner's keyword arguments, e.g. {"steps": 32, "rule": "gauss_legendre", "baseline": "black"}, plus an
        optional "fractions" for the curves.  Returns {"clean": what test() returns, "deletion_auc" and "insertion_auc": {"ig": the
        mean, "random": the mean, "per_sample": the two float64 tensors}, "gap_rel": |gap| / max(|f_x - f_b|, tiny) per sample (the
        completeness defect: raise "steps" where it is large), "attribution": the resolved arguments}.  A faithful map has a lower
        deletion AUC and a higher insertion AUC than the random one.  Sample i of rank r's batch b has the stream id
        (b world + r) 2 batch + i; the columns are gathered over the ranks as in test(), in a fixed order."""
        return self._evaluator().test_attribution(
            batches, attribution if attribution is not None else self.config["config"].get("attribution"))

    def validate(self, step, batches=4):
        """The reference's validate (forgery_engine.py:320-421) without the figure / wandb plumbing: metrics over all
        ranks, best-so-far record (AUC + ACC), best_model.bin / latest_model.bin on rank 0."""
        self._select_gemm_path()
        self._check_exchange()
        ret = self.test(batches)
        if "AUC" in ret and ret["AUC"] + ret["ACC"] > self.best_auc + self.best_acc:
            self.best_auc, self.best_acc, self.best_step = float(ret["AUC"]), float(ret["ACC"]), int(step)
            if self.config["config"].get("dir"):
                self._save_ckpt(step, best=True)
        if self.config["config"].get("dir"):
            self._save_ckpt(step, best=False)
        return ret

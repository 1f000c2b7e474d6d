"""Graph-captured inference forward: InferenceRunner.

The eval-mode forward (what TrainEngine.test() / .validate() run, and what a deployed detector runs) replayed as ONE hipGraph
per (batch, size): the first call runs one eager warm-up (it settles the on-line GEMM tuner and every lazily made workspace
for the shape), the second captures `model(x)` under no_grad into a graph with static input and output buffers, and every
call copies the input in and replays.  K.begin_forward runs inside the graph and every BatchNorm reads the module's running
buffers in place, so a runner captured before an optimizer step (or a load_state_dict, or a change of running statistics)
gives the updated model's output afterwards without being rebuilt.

UDEB4's block group 1 takes the eval-mode node (mbconv.mbconv_eval: the expand conv inside the depthwise pass,
csrc/evalblk.hip) during the runner's warm-up and capture; every other layer, and the ResNet variants as a whole, are captured
as their eager eval forward.

precision="fp16" (UDEB4 only): the MBConv trunk in half storage with the storage boundaries of the fp16 training mode — the stem
conv's output rounded once to half, the 32 blocks' activations fp16 in memory (fp32 arithmetic in registers, fp16 MFMA 1x1
convs with fp32 accumulation), the decoder, attention, head and losses fp32 — on eval-form BatchNorms with no batch statistics
(mbconv.mbconv_eval_half).  Selected by a runner-scoped flag; the eager eval forward and the fp32 runner do not change.
"""
import contextlib

import torch

_MAX_RUNNERS = 4          # captured keys a model keeps (model.inference_runner), oldest evicted first
PRECISIONS = ("fp32", "fp16")


@contextlib.contextmanager
def _eval_nodes(model, half=False):
    flag = "_eval_half" if half else "_eval_fused"
    prev = model.__dict__.get(flag, False)
    model.__dict__[flag] = True
    try:
        yield
    finally:
        model.__dict__[flag] = prev


def _check_precision(model, precision):
    from .model.unidefense import UniDefenseModelEb4
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    if precision == "fp16" and not isinstance(model, UniDefenseModelEb4):
        raise ValueError(f"precision 'fp16' is built for UDEB4 only; {type(model).__name__} has no half-storage path")


def _check_model(what, model, precision, arguments=None):
    """What every runner (`what`: its name) asks of its model, in this order: one of the three models and a precision it has;
    then arguments(), the runner's own refusals that need no device; then eval mode and a GPU.  Returns the model's device."""
    from .model import MODEL
    if not isinstance(model, tuple(MODEL.values())):
        raise ValueError(f"{what} takes a UDEB4 / UDR18 / UDR50 model, got {type(model).__name__}")
    _check_precision(model, precision)
    if arguments is not None:
        arguments()
    if model.training:
        raise ValueError(f"{what} needs model.eval(): the captured forward reads the running statistics")
    p = next(model.parameters())
    if not p.is_cuda:
        raise ValueError(f"{what} needs a cuda model")
    return p.device


class InferenceRunner:
    """runner = InferenceRunner(model, batch, size[, precision]); out = runner(x) with x [batch, 3, size, size] fp32 on the
    model's GPU; out is the dict model(x) returns under no_grad ({"cls_out", "rec", "loss_dict"}, every tensor fp32), held in the
    runner's static buffers: the next call overwrites it (clone what must outlive it).  precision: "fp32" or "fp16" (UDEB4)."""

    def __init__(self, model, batch, size, precision="fp32"):
        self.device = _check_model("InferenceRunner", model, precision)
        self.model, self.batch, self.size, self.precision = model, int(batch), int(size), precision
        self.half = precision == "fp16"
        self.shape = (self.batch, 3, self.size, self.size)
        self.calls = 0
        self.graph = self.x = self.out = None

    def _check(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError("InferenceRunner takes a cuda tensor")
        if tuple(x.shape) != self.shape or x.dtype != torch.float32:
            raise ValueError(f"input {tuple(x.shape)} {x.dtype} differs from the runner's key {self.shape} torch.float32")
        if self.model.training:
            raise ValueError("the model is in training mode: call model.eval() before the runner")

    @torch.no_grad()
    def __call__(self, x):
        self._check(x)
        self.calls += 1
        if self.calls == 1:
            with _eval_nodes(self.model, self.half):           # eager warm-up of the same forward the graph records
                return self.model(x.contiguous())
        if self.graph is None:
            self.x = x.detach().clone().contiguous()
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with _eval_nodes(self.model, self.half), torch.cuda.graph(g):
                self.out = self.model(self.x)
            self.graph = g
        else:
            self.x.copy_(x)
        self.graph.replay()
        return self.out


def inference_runner(model, batch, size, precision="fp32"):
    """The model's runner for (batch, size[, precision]), made on first use; a model keeps at most _MAX_RUNNERS of them."""
    _check_precision(model, precision)
    runners = model.__dict__.setdefault("_ud_runners", {})
    key = (int(batch), int(size)) if precision == "fp32" else (int(batch), int(size), precision)
    r = runners.pop(key, None)
    if r is None:
        r = InferenceRunner(model, batch, size, precision)
        while len(runners) >= _MAX_RUNNERS:
            del runners[next(iter(runners))]
    runners[key] = r                                 # most recently used last
    return r

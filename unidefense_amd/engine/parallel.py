"""Data parallelism for the HIP model: one process per GPU, RCCL over xGMI
(reference: SyncBatchNorm.convert_sync_batchnorm + DistributedDataParallel, engine/forgery_engine.py:142-146).

The path shards over the batch only.  Exchanges per backward:
  * parameter gradients — bucketed flat all-reduce.  The whole network is a single autograd node, so the exchange
    is driven from inside that node's backward (model/unidefense.py:_NetFunction): the tape hands every parameter
    gradient to the GradReducer the moment it is final (reverse parameter order); large gradients (>= 2 MB: the
    spectral 1x1 weights, 85 % of the bytes) are all-reduced in place, the small ones are packed into ~64 MB buckets;
    every all-reduce is launched ASYNCHRONOUSLY (it runs on the process group's own stream), so the exchange of
    the deep layers' gradients overlaps the backward of the shallow ones; the backward waits for all buckets at its
    end and returns views of the reduced flat buffers (no copy back).  The mean over ranks comes for free: the
    incoming loss gradient is scaled by 1/world before the tape runs (everything downstream is linear in it,
    including the SyncBN sums).
  * SyncBatchNorm statistics, enabled by ``sync_bn=True``.  Fused MBConv path (mbconv.mbconv_fused): the fp64
    accumulators (sum x, sum x^2) of a BatchNorm are summed over the ranks IN PLACE between the kernel that fills them
    and the kernels that consume them (tape.DataParallelCtx.reduce), likewise (sum dz, sum dz*xhat) in the backward —
    2C doubles each way.  Every rank must hold the SAME number of rows (the count is rows * world; engine/data.py pads the
    shards like DistributedSampler so that they do).  On one node the sum is BnExchange's single kernel over peer-mapped
    mailboxes (csrc/xchg.hip; rank-ordered, bit-identical on all ranks; sized for the model's widest BatchNorm);
    otherwise one dist.all_reduce.  Operator path (tape.batchnorm_act: attention / head / the ResNet models, e.g. BASELINE
    configs[3], UDR50 on 4 GPUs, engine/ocim_engine.py:130-133): the same fp64 sums through the same exchange
    (tape._syncbn_act on the deferred-BatchNorm kernels).
No other collective exists on the data path.
"""
import torch
import torch.distributed as dist
import torch.nn as nn

from .. import tape as T
from ..config import cfg


class GradReducer:
    """Sums gradients over the ranks of `group`, bucket by bucket, asynchronously.

    begin() -> ready(key, g) in the order gradients become final -> finish() -> {key: reduced g (a view of its
    bucket's flat buffer)}.  Device-agnostic (RCCL on GPUs, gloo in the CPU tests)."""

    def __init__(self, group, bucket_bytes, direct_bytes=2 << 20):
        self.group = group
        self.bucket_bytes = bucket_bytes
        # A gradient of at least this size is reduced IN PLACE as a collective of its own instead of being packed:
        # the spectral 1x1 weights (1344^2 .. 3264^2: 7 - 43 MB each) are 85 % of the 513 MB of gradients, and
        # copying them into a bucket would move them through HBM twice more for nothing.
        self.direct_bytes = direct_bytes
        self.begin()

    def begin(self):
        self.bucket, self.size, self.pending, self.done = [], 0, [], set()
        self.bytes = self.collectives = 0          # of this backward (bench.py's diagnostics)

    def ready(self, key, g):
        self.done.add(key)
        nbytes = g.numel() * g.element_size()
        self.bytes += nbytes
        if nbytes >= self.direct_bytes and g.is_contiguous():
            self.collectives += 1
            work = dist.all_reduce(g, group=self.group, async_op=True)
            self.pending.append((work, g.view(-1), [(key, g)]))
            return
        self.bucket.append((key, g))
        self.size += nbytes
        if self.size >= self.bucket_bytes:
            self.flush()

    def flush(self):
        if not self.bucket:
            return
        flat = torch.cat([g.reshape(-1) for _, g in self.bucket])
        self.collectives += 1
        work = dist.all_reduce(flat, group=self.group, async_op=True)
        self.pending.append((work, flat, self.bucket))
        self.bucket, self.size = [], 0

    def finish(self):
        self.flush()
        out = {}
        prof = T.DP_PROFILE if (T.DP_PROFILE is not None and torch.cuda.is_available()) else None
        if prof is not None:                 # the backward's own kernels end here; what follows is the EXPOSED part of the exchange
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for work, flat, bucket in self.pending:
            work.wait()                      # GPU: the current stream waits for the collective's stream
            off = 0
            for key, g in bucket:
                n = g.numel()
                out[key] = flat[off:off + n].view(g.shape)
                off += n
        if prof is not None:
            e1.record()
            prof["ar"].append((e0, e1, self.bytes, self.collectives))
        self.pending = []
        return out


class BnExchange:
    """One-shot SyncBatchNorm exchange (csrc/xchg.hip): the fp64 BatchNorm accumulators are summed over the ranks of ONE
    node by a single small kernel writing into peer-mapped mailboxes, instead of one RCCL collective per BatchNorm
    (~200 per step, each latency-bound).  Setup is collective over `group` (handles travel through all_gather_object);
    a self-test exchanges known vectors and every rank must see the exact sum, otherwise ALL ranks fall back to
    dist.all_reduce (`ok` False) — e.g. ranks on different nodes, where the IPC open fails.  `UD_SYNCBN_EXCHANGE=0`
    disables it."""

    MAX_DOUBLES = 8192          # default mailbox row: 2 * 3264 channels, the largest accumulator of the EfficientNet-b4 trunk
    SLOTS = 4
    # Wall-clock wait for the slowest peer before it is reported missing.  Ranks of a healthy job drift apart by seconds
    # (a data-loader stall, rank 0 writing a checkpoint, first-step GEMM tuning), so this is minutes — RCCL itself would
    # wait for ever; a timed-out exchange poisons its sums with NaN and check() raises.
    TIMEOUT_S = 600.0
    # ... except in the self-test at construction: every rank enters it straight out of a collective, so a peer whose words do
    # not arrive within seconds never will (mailbox mapped but not coherent across the link) — fall back to RCCL quickly
    # instead of sitting out ten minutes per probe inside the driver's bench run.
    SELF_TEST_TIMEOUT_S = 30.0

    def __init__(self, group, device, max_doubles=None):
        import ctypes as C
        from .. import lib
        self.group, self.device = group, device
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self.ok, self.base, self.opened = False, None, []
        self._timeout_s = self.TIMEOUT_S
        if max_doubles is not None:
            self.MAX_DOUBLES = max(int(max_doubles), 64)          # sized from the model (HipDataParallel)
        want = cfg.syncbn_exchange and device.type == "cuda"
        status, handle = 0, b""
        if want:
            base, buf = C.c_void_p(), C.create_string_buffer(64)
            status = lib.load().ud_xchg_create(self.world, self.MAX_DOUBLES, self.SLOTS, C.byref(base), buf)
            if status == 0:
                self.base, handle = base.value, buf.raw
        handles = [None] * self.world
        dist.all_gather_object(handles, (status == 0 and want, handle), group=group)
        good = all(h[0] for h in handles)
        ptrs = []
        if good:
            for r, (_, h) in enumerate(handles):
                if r == self.rank:
                    ptrs.append(self.base)
                    continue
                p = C.c_void_p()
                if lib.load().ud_xchg_open(h, C.byref(p)) != 0:
                    good = False
                    break
                self.opened.append(p.value)
                ptrs.append(p.value)
        flag = torch.tensor([1 if good else 0], device=device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag.item()) != 1:
            return
        self.peers = torch.tensor(ptrs, dtype=torch.int64, device=device)
        self.seq = torch.zeros(2, dtype=torch.int64, device=device)     # exchanges completed, workgroups arrived
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        self.ok = True
        self._timeout_s = self.SELF_TEST_TIMEOUT_S
        self.ok = self._self_test()
        self._timeout_s = self.TIMEOUT_S

    def _self_test(self):
        n = 1000
        good = True
        for it in range(2 * self.SLOTS + 1):            # every slot twice
            v = (torch.arange(n, device=self.device, dtype=torch.float64) + 1.0) * (self.rank + 1) + it
            self.allreduce(v)
            want = (torch.arange(n, device=self.device, dtype=torch.float64) + 1.0) * (self.world * (self.world + 1) / 2) \
                + it * self.world
            good = good and bool(torch.equal(v, want)) and int(self.err.item()) == 0
            if not good:                                # a rank that saw a wrong sum stops probing; its peers time out ONCE
                break                                   # on the next probe and stop too (every rank ends in the all_reduce below)
        # ... and from a replayed hipGraph, the way the captured train step issues them (device-side sequence counter)
        if good and not torch.cuda.is_current_stream_capturing():
            try:
                a = torch.zeros(512, dtype=torch.float64, device=self.device)
                src = torch.full((512,), float(self.rank + 1), dtype=torch.float64, device=self.device)
                torch.cuda.synchronize()
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                        a.copy_(src)
                        self.allreduce(a)
                        a.mul_(0.5)
                        self.allreduce(a)
                    for _ in range(3):
                        g.replay()
                torch.cuda.synchronize()
                tri = self.world * (self.world + 1) / 2.0                      # sum of (rank + 1)
                good = bool((a == 0.5 * tri * self.world).all()) and int(self.err.item()) == 0
            except Exception:                                                  # noqa: BLE001 — any failure: fall back
                good = False
        flag = torch.tensor([1 if good else 0], device=self.device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
        return int(flag.item()) == 1

    def allreduce(self, acc, local_out=None):
        """acc (contiguous fp64, <= MAX_DOUBLES): summed over the ranks in place, in rank order.  local_out: optional buffer of
        the same size that receives this rank's own values as they were before the sum (written by the same launch)."""
        from .. import kernels as K
        from .. import lib
        assert acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() <= self.MAX_DOUBLES
        assert local_out is None or (local_out.dtype == torch.float64 and local_out.is_contiguous() and local_out.numel() == acc.numel())
        lib.call("ud_xchg_allreduce", K._p(acc), acc.numel(), K._p(self.peers), self.rank, self.world, self.MAX_DOUBLES,
                 self.SLOTS, K._p(self.seq), K._p(self.err), int(self._timeout_s * 1000), K._p(local_out), K._stream())

    def check(self):
        """Host-side check (synchronises): a rank that timed out waiting for a peer raises here.  The engine calls it at
        every log step and BEFORE every checkpoint save / validation (the affected statistics are NaN, so nothing computed
        from them can pass for a result either)."""
        if not self.ok:
            return
        e = int(self.err.item())
        if e:
            raise RuntimeError(f"SyncBatchNorm exchange: rank {e - 1} did not arrive within {self.TIMEOUT_S:.0f} s "
                               f"(rank {self.rank} timed out); the step's BatchNorm sums were set to NaN")

    def close(self):
        from .. import lib
        for p in self.opened:
            lib.load().ud_xchg_close(p)
        self.opened = []
        if self.base:
            lib.load().ud_xchg_destroy(self.base)
            self.base = None
        self.ok = False


class HipDataParallel(nn.Module):
    """Minimal DDP replacement exposing ``.module`` like torch's wrapper."""

    def __init__(self, module: nn.Module, process_group=None, bucket_bytes: int = 64 << 20, sync_bn: bool = True):
        super().__init__()
        self.module = module
        self.process_group = process_group
        self.bucket_bytes = bucket_bytes
        self.world = dist.get_world_size(process_group)
        # same initial state on every rank (DDP broadcasts rank 0's parameters and buffers)
        with torch.no_grad():
            for t in list(module.parameters()) + list(module.buffers()):
                dist.broadcast(t.data, 0, group=process_group)
        self.force = cfg.force_collectives           # single-GPU exercise of the RCCL calls (tape.py)
        if self.world > 1 or self.force:
            module._grad_reducer = GradReducer(process_group, bucket_bytes)
            module._grad_prescale = 1.0 / self.world
        if sync_bn and (self.world > 1 or self.force):
            module._sync_bn_group = process_group if process_group is not None else dist.group.WORLD
            dev = next(module.parameters()).device
            if dev.type == "cuda":
                # mailbox rows sized for the widest BatchNorm of THIS model (sum | sum of squares: 2C doubles)
                widest = max([m.num_features for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)] + [1])
                self.bn_exchange = BnExchange(module._sync_bn_group, dev, max(BnExchange.MAX_DOUBLES, 2 * widest))
                module._bn_exchange = self.bn_exchange if self.bn_exchange.ok else None

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def sync_grads(self, grads):
        """grads: list of tensors (or None) in parameter order -> averaged over ranks (a new list; the one-shot
        form of what _NetFunction.backward streams)."""
        if self.world == 1 and not self.force:
            return grads
        red = GradReducer(self.process_group, self.bucket_bytes)
        for i in reversed(range(len(grads))):
            if grads[i] is not None:
                red.ready(i, grads[i])
        out = red.finish()
        return [None if g is None else out[i].mul_(1.0 / self.world) for i, g in enumerate(grads)]


def wrap_data_parallel(model: nn.Module, local_rank: int = 0, process_group=None, sync_bn: bool = True):
    return HipDataParallel(model, process_group, sync_bn=sync_bn)

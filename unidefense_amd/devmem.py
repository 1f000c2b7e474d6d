"""Device memory that outlives a single launch: the kernels' scratch buffers and the zero blocks their accumulators
are carved from.  Both are keyed by the device and shared by the launches of its ONE stream in order: a reduction's
finalize launch has consumed the scratch before the next reduction starts.
"""
import torch


class Scratch:
    """One grow-on-demand buffer of `dtype` per device (at least `min_elems` elements) that is NEVER freed.

    A captured graph bakes in the pointer it was captured with, and the runners and the train engine warm up eagerly
    first, so that pointer is an ordinary allocation, not part of the graph's private pool.  Were a superseded buffer
    released when a larger shape arrives, the caching allocator would hand its block to the next tensor of that size and
    an older graph's replay would write its partial sums into it: nothing faults, the block is still mapped.  So growth
    keeps the old buffer in `retired` for the life of the process.  Growth at least doubles, hence the retired buffers
    of a device together stay below the size of its current one."""

    def __init__(self, dtype, min_elems=0):
        self.dtype, self.min_elems = dtype, min_elems
        self.current = {}          # device index -> the buffer handed out now
        self.retired = {}          # device index -> every superseded buffer

    def get(self, ref, n):
        key = ref.device.index
        buf = self.current.get(key)
        if buf is None or buf.numel() < n:
            if buf is not None:
                self.retired.setdefault(key, []).append(buf)
                n = max(n, 2 * buf.numel())
            buf = self.current[key] = torch.empty(max(n, self.min_elems), dtype=self.dtype, device=ref.device)
        return buf


class ZeroPool:
    """Zero-initialised outputs carved from large zero blocks of `block_elems` elements: one fill launch per block instead of
    one (~5 us) per split-K result (~180 per step) or fp64 accumulator (~10 per MBConv block and pass).  A block is never
    reused, so every carve is still zero; offsets advance in multiples of `align`.  reset() at the start of a forward /
    backward makes a step captured into a hipGraph contain the fills of every block it carves from; a block filled outside
    a capture must not serve carves inside one (the replay would not re-zero it), nor vice versa.  A take of `own_elems` or
    more elements (or of none) is a torch.zeros of its own; one larger than a block gets a block of its size."""

    def __init__(self, dtype, block_elems, align, own_elems=None):
        self.dtype, self.block_elems, self.align, self.own_elems = dtype, block_elems, align, own_elems
        self._state = {}           # device index -> [block, next offset, filled inside a capture]

    def reset(self):
        self._state.clear()

    def take(self, n, like):
        """n zeros as a flat view (never recycled within a forward / backward)."""
        n = int(n)
        if self.own_elems is not None and (n >= self.own_elems or n == 0):
            return torch.zeros(n, dtype=self.dtype, device=like.device)
        key = like.device.index
        st = self._state.get(key)
        capturing = like.is_cuda and torch.cuda.is_current_stream_capturing()
        if st is None or st[1] + n > st[0].numel() or st[2] != capturing:
            st = self._state[key] = [torch.zeros(max(self.block_elems, n), dtype=self.dtype, device=like.device), 0, capturing]
        out = st[0][st[1]:st[1] + n]
        st[1] += (n + self.align - 1) // self.align * self.align
        return out

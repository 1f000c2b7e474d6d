"""unidefense_amd.devmem on CPU tensors: the scratch that is never freed and the zero pools (no kernel, no library)."""
import gc
import weakref

import pytest
import torch

from unidefense_amd.devmem import Scratch, ZeroPool

REF = torch.zeros(1)

# the two parameterisations of unidefense_amd/kernels.py
POOLS = {"fp32": dict(dtype=torch.float32, block_elems=8 << 20, align=64, own_elems=2 << 20),
         "fp64": dict(dtype=torch.float64, block_elems=1 << 20, align=32)}


@pytest.mark.parametrize("n,min_elems", [(5, 0), (5, 64), (100, 64)])
def test_scratch_first_allocation(n, min_elems):
    ws = Scratch(torch.float64, min_elems)
    buf = ws.get(REF, n)
    cap = max(n, min_elems)
    assert buf.dim() == 1 and buf.dtype == torch.float64 and buf.device == REF.device and buf.numel() == cap
    for m in (0, 1, n, cap):
        assert ws.get(REF, m).data_ptr() == buf.data_ptr()
    assert not ws.retired


def test_scratch_growth_retires_and_keeps_the_old_buffer():
    ws = Scratch(torch.float32, 16)
    old = ws.get(REF, 3)
    old_ptr, old_n = old.data_ptr(), old.numel()
    new = ws.get(REF, old_n + 1)
    assert new.data_ptr() != old_ptr and new.numel() >= max(old_n + 1, 2 * old_n)
    assert ws.get(REF, 5 * old_n).numel() >= 5 * old_n          # a request beyond the doubling is served in full
    retired = ws.retired[REF.device.index]
    assert retired[0] is old and len(retired) == 2
    alive = weakref.ref(old.untyped_storage())
    del old, retired
    gc.collect()
    assert alive() is not None and alive().data_ptr() == old_ptr


def test_scratch_retired_total_stays_below_the_current_buffer():
    ws = Scratch(torch.uint8)
    for n in (1, 3, 4, 9, 100, 101, 1000):
        cur = ws.get(REF, n)
        assert cur.numel() >= n
        assert sum(t.numel() for t in ws.retired.get(REF.device.index, [])) < cur.numel()


def _offset(view, first):
    return (view.data_ptr() - first.data_ptr()) // view.element_size()


@pytest.mark.parametrize("kind", list(POOLS))
def test_zero_pool_carves(kind):
    p = POOLS[kind]
    pool = ZeroPool(**p)
    sizes = [1, 63, 64, 0, 65, 1000, 31, 33]
    views = [pool.take(n, REF) for n in sizes]
    first = views[0]
    end = 0
    for n, v in zip(sizes, views):
        assert v.dtype == p["dtype"] and v.shape == (n,) and not v.any()
        if n == 0:
            continue
        assert v.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
        off = _offset(v, first)
        assert off % p["align"] == 0 and off >= end          # aligned, and past everything carved before
        end = off + n
    for i, v in enumerate(views):          # writes through one view reach no other
        v.fill_(i + 1)
    for i, v in enumerate(views):
        assert bool((v == i + 1).all())


@pytest.mark.parametrize("kind", list(POOLS))
def test_zero_pool_new_block_when_full_and_after_reset(kind):
    p = POOLS[kind]
    own = p.get("own_elems")
    big = (own - 1) if own else p["block_elems"] // 2 + 1          # the largest carves that still share a block
    pool = ZeroPool(**p)
    views = [pool.take(big, REF) for _ in range(p["block_elems"] // big)]
    blocks = {v.untyped_storage().data_ptr() for v in views}
    assert len(blocks) == 1
    for v in views:
        v.fill_(7.0)
    spill = pool.take(big, REF)          # does not fit any more
    assert spill.untyped_storage().data_ptr() not in blocks and not spill.any()
    for v in views:
        assert v.untyped_storage().data_ptr() in blocks and bool((v == 7.0).all())
    small = pool.take(8, REF)
    assert small.untyped_storage().data_ptr() == spill.untyped_storage().data_ptr()
    pool.reset()
    fresh = pool.take(8, REF)
    assert fresh.untyped_storage().data_ptr() != spill.untyped_storage().data_ptr() and not fresh.any()
    spill.fill_(3.0)
    small.fill_(4.0)
    assert bool((spill == 3.0).all()) and bool((small == 4.0).all()) and not fresh.any()


def test_zero_pool_own_tensor_from_own_elems():
    p = POOLS["fp32"]
    pool = ZeroPool(**p)
    a = pool.take(8, REF)
    own = pool.take(p["own_elems"], REF)
    assert own.shape == (p["own_elems"],) and not own.any()
    assert own.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()
    assert own.untyped_storage().nbytes() == own.numel() * own.element_size()          # a tensor of its own, not a view
    assert _offset(pool.take(8, REF), a) == p["align"]          # and the block's offset did not move
    assert pool.take(0, REF).shape == (0,)


def test_zero_pool_serves_more_than_a_block():
    p = POOLS["fp64"]
    pool = ZeroPool(**p)
    a = pool.take(8, REF)
    n = p["block_elems"] + 5
    v = pool.take(n, REF)
    assert v.shape == (n,) and v.dtype == torch.float64 and not v.any()
    assert v.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()
    assert pool.take(0, REF).shape == (0,)


def test_kernels_zero_functions():
    from unidefense_amd import kernels as K
    z = K.zeros((3, 5), REF)
    assert z.shape == (3, 5) and z.dtype == torch.float32 and not z.any()
    z64 = K.zeros64(7, REF)
    assert z64.dtype == torch.float64 and z64.shape == (7,) and not z64.any()
    assert K.zeros((0, 4), REF).shape == (0, 4)
    nxt = K.zeros((4,), REF)
    assert nxt.untyped_storage().data_ptr() == z.untyped_storage().data_ptr()
    K.reset_zero_pool()          # both pools start new blocks
    assert K.zeros((4,), REF).untyped_storage().data_ptr() != z.untyped_storage().data_ptr()
    assert K.zeros64(4, REF).untyped_storage().data_ptr() != z64.untyped_storage().data_ptr()
    K.reset_zero_pool()          # leave no CPU block behind for the pools' real users

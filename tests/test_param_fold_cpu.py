"""The host side of the collected parameter-gradient folds (kernels.begin_wgrad_folds / _defer_fold / flush_wgrad_folds and the
rules of Tape.add_param_grad), with the native calls stubbed: what is launched, with which items, and when."""
import ctypes

import pytest
import torch

from unidefense_amd import kernels as K
from unidefense_amd.tape import Tape


@pytest.fixture
def native(monkeypatch):
    """log of (entry point, items as dicts) of every stubbed native call, and of the host events the tests add"""
    log = []

    def call(name, *args):
        if name == "ud_param_fold_multi":
            arr, n = args[0], args[1]
            assert len(arr) == n
            log.append((name, [{f: getattr(a, f) for f, _ in a._fields_} for a in arr]))
        else:
            log.append((name, args))
        return 0
    monkeypatch.setattr(K, "_call", call)
    monkeypatch.setattr(K, "_stream", lambda: None)
    monkeypatch.setattr(K, "axpby", lambda a, sa, b, sb, out=None: (log.append(("axpby", None)), sa * a + sb * b)[1])
    assert K._WGRAD_FOLDS is None
    yield log
    assert K._WGRAD_FOLDS is None


def _producer():
    """a stand-in for K.norm_bwd's G > 1 tail: returns (dgamma, dbeta), as a group-sum item while folds are collected"""
    s = torch.zeros(2, 3, 8)
    dg, db = torch.zeros(8), torch.zeros(8)
    if K.folds_deferred():
        K._defer_fold("group", (dg, db), keep=(s,), part=s[0], aux=s[1], dgamma=dg, dbeta=db, nparts=3, n=8)
    else:
        K._call("immediate", dg, db)
    return dg, db


def _folds(log):
    return [e for e in log if e[0] == "ud_param_fold_multi"]


def test_items_carry_the_header_fields_and_one_flush_takes_them_all(native):
    p, q = torch.zeros(8), torch.zeros(8)
    tape = Tape()
    made = []

    def node():
        dg, db = _producer()
        assert dg._ud_deferred and db._ud_deferred
        made.append((dg, db))
        tape.add_param_grad(p, dg)
        tape.add_param_grad(q, _producer()[1])
    tape.record(node)
    tape.backward()
    (name, items), = _folds(native)
    assert len(items) == 2 and not any(e[0] == "immediate" for e in native)
    it = items[0]
    assert it["kind"] == K.FOLD_KINDS["group"] == 4 and (it["nparts"], it["n"], it["p0"]) == (3, 8, 0)
    addr = lambda ptr: ctypes.cast(ptr, ctypes.c_void_p).value
    dg, db = made[0]
    assert addr(it["dgamma"]) == dg.data_ptr() and addr(it["dbeta"]) == db.data_ptr() and addr(it["dst"]) is None
    assert addr(it["aux"]) - addr(it["part"]) == 3 * 8 * 4
    assert dg._ud_deferred is False and db._ud_deferred is False and tape.param_grads[p].data_ptr() == dg.data_ptr()


def test_a_second_contribution_flushes_before_it_is_added(native):
    p = torch.zeros(8)
    tape = Tape()
    for _ in range(2):
        tape.record(lambda: tape.add_param_grad(p, _producer()[0]))
    tape.backward()
    names = [e[0] for e in native if e[0] in ("ud_param_fold_multi", "axpby")]
    # the first gradient AND the incoming one are folded (one launch) before the sum reads them; nothing is left for the end
    assert names == ["ud_param_fold_multi", "axpby"]
    assert len(_folds(native)[0][1]) == 2 and not tape._deferred


def test_a_nested_backward_flushes_the_outer_items_first(native):
    p, q = torch.zeros(8), torch.zeros(8)
    tape, inner = Tape(), Tape()
    inner.record(lambda: inner.add_param_grad(q, _producer()[0]))

    def node():
        tape.add_param_grad(p, _producer()[0])
        native.append(("inner starts", None))
        inner.backward()
        native.append(("inner ends", None))
        tape.add_param_grad(q, _producer()[0])          # the outer tape no longer collects: folded at once
    tape.record(node)
    tape.backward()
    names = [e[0] for e in native]
    assert names == ["inner starts", "ud_param_fold_multi", "ud_param_fold_multi", "inner ends", "immediate"]
    assert [len(f[1]) for f in _folds(native)] == [1, 1]


def test_a_param_ready_hook_sees_a_folded_gradient(native):
    p = torch.zeros(8)
    tape = Tape()
    tape.param_uses = {id(p): 1}
    tape.param_ready = lambda pid, g: native.append(("ready", pid))
    tape.record(lambda: tape.add_param_grad(p, _producer()[0]))
    tape.backward()
    assert [e[0] for e in native] == ["ud_param_fold_multi", "ready"] and native[1][1] == id(p)


def test_flush_at_the_end_stops_collecting_when_a_node_raises(native):
    p = torch.zeros(8)
    tape = Tape()

    def bad():
        raise RuntimeError("node failed")
    tape.record(bad)
    tape.record(lambda: tape.add_param_grad(p, _producer()[0]))
    with pytest.raises(RuntimeError, match="node failed"):
        tape.backward()
    assert K._WGRAD_FOLDS is None and len(_folds(native)) == 1          # the pending item was still folded, then collection ended
    assert not K.folds_deferred()


def test_immediate_folds_makes_a_backward_fold_at_once(native):
    p = torch.zeros(8)
    tape = Tape()
    tape.record(lambda: tape.add_param_grad(p, _producer()[0]))
    with K.immediate_folds():
        tape.backward()
    assert [e[0] for e in native] == ["immediate"]
    tape = Tape()
    tape.record(lambda: tape.add_param_grad(p, _producer()[0]))
    tape.backward()          # ... and only inside the context
    assert [e[0] for e in native] == ["immediate", "ud_param_fold_multi"]

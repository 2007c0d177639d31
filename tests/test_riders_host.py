"""Who owns what rides on a TrainStep's backward (ops.TrainStep.attach / detach / riders_of) and what naruto_amd.capture.preserved puts
back -- on the host: the rider methods touch four fields of the step and nothing on the device."""

import ctypes as C
import gc
import weakref

import torch

from naruto_amd import _lib, ops
from naruto_amd.capture import preserved


class _Step:
    """The fields of ops.TrainStep that its rider methods touch."""
    attach, detach, riders_of, _ridden_by = (ops.TrainStep.__dict__[k] for k in ("attach", "detach", "riders_of", "_ridden_by"))

    def __init__(self):
        self.opt = _lib.NarutoFusedAdam()
        self.ba_poses = self._next_batch_keep = self._rider_owner = None


class _Owner:
    pass


def _riders():
    return (_lib.NarutoRayBatch(), ("keep-alives",)), _lib.NarutoBAPoses()


def test_detach_by_somebody_else_leaves_the_riders():
    ts, a, b = _Step(), _Owner(), _Owner()
    batch, poses = _riders()
    ts.attach(a, next_batch=batch, ba_poses=poses)
    assert ts.opt.next_batch == C.addressof(batch[0]) and ts.ba_poses is poses and ts.riders_of(a) == (batch, poses)
    assert ts.riders_of(b) == (None, None)
    assert not ts.detach(b)
    assert ts.opt.next_batch == C.addressof(batch[0]) and ts._next_batch_keep is batch and ts.ba_poses is poses and ts.riders_of(a) == (batch, poses)


def test_a_second_owner_replaces_the_first_and_keeps_its_riders():
    ts, a, b = _Step(), _Owner(), _Owner()
    batch_a, poses_a = _riders()
    batch_b, _ = _riders()
    ts.attach(a, next_batch=batch_a, ba_poses=poses_a)
    ts.attach(b, next_batch=batch_b)
    assert ts.riders_of(a) == (None, None) and ts.riders_of(b) == (batch_b, None)
    assert ts.ba_poses is None, "a's pose refinement went with a's ownership"
    assert not ts.detach(a)
    assert ts.opt.next_batch == C.addressof(batch_b[0]) and ts._next_batch_keep is batch_b and ts.riders_of(b) == (batch_b, None)


def test_the_owner_is_held_weakly():
    ts, a = _Step(), _Owner()
    batch, _ = _riders()
    ts.attach(a, next_batch=batch)
    gone = weakref.ref(a)
    del a
    gc.collect()
    assert gone() is None, "the step keeps its owner alive"
    assert ts.opt.next_batch == C.addressof(batch[0]) and ts._next_batch_keep is batch, "the riders live on the step, not on the owner"
    # nobody's riders any more: whoever detaches takes them off (the collector clears weak references before it runs the owner's finaliser)
    assert ts.detach(_Owner())
    assert not ts.opt.next_batch and ts._next_batch_keep is None


def test_detach_by_the_owner_clears_the_riders():
    ts, a = _Step(), _Owner()
    batch, poses = _riders()
    ts.attach(a, next_batch=batch, ba_poses=poses)
    assert ts.detach(a)
    assert not ts.opt.next_batch and ts._next_batch_keep is None and ts.ba_poses is None and ts.riders_of(a) == (None, None)
    assert not ts.detach(a)
    ts.attach(a)                                     # nothing to carry: nobody's step
    assert ts.riders_of(a) == (None, None) and ts._rider_owner is None


def test_preserved_restores_by_value_into_the_same_tensors():
    torch.manual_seed(0)
    p, q = torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3))
    extra = torch.arange(4.0)
    opt = torch.optim.Adam([p, q], lr=0.1)
    p.grad = torch.ones(5)
    opt.step()                                       # p has state before the block, q (no gradient yet) has none
    state_p = opt.state[p]
    want = {k: v.clone() for k, v in state_p.items()}
    want_p, want_q, want_extra = p.detach().clone(), q.detach().clone(), extra.clone()
    with preserved([p, q, extra], [opt]):
        q.grad = torch.ones(3)
        for _ in range(3):
            opt.step()
        extra += 1.0
        state_q = opt.state[q]
        inside = {k: v for k, v in state_q.items() if torch.is_tensor(v)}
        assert not torch.equal(p.detach(), want_p) and float(state_p["step"]) == 4.0 and inside
    assert torch.equal(p.detach(), want_p) and torch.equal(q.detach(), want_q) and torch.equal(extra, want_extra)
    assert opt.state[p] is state_p
    for k, v in want.items():
        assert opt.state[p][k] is state_p[k] and torch.equal(state_p[k], v), k
    assert opt.state[q] is state_q, "state created inside the block is kept ..."
    for k, v in inside.items():
        assert state_q[k] is v and not v.any(), f"... and zeroed: {k}"

"""What every hipGraph capture in this package does around the capture itself: keep the garbage collector out, warm the launches up
on a side stream, and put the training state back afterwards (``MappingTrainer.capture``, ``GraphedIteration``, ``TrackerHIP.capture``,
``FusedBA``)."""

from __future__ import annotations

import contextlib
import copy
import gc

import torch

# graphs dropped while somebody's stream capture was under way (a finaliser ran inside the capture: destroying a graph there ends the
# capture with an error); released by the next release_parked() outside a capture
_PARKED_GRAPHS = []


@contextlib.contextmanager
def no_collection():
    """Around a stream capture: the garbage there is is collected first, and the cyclic collector rests until the capture has ended --
    a finaliser that frees graphs or device memory (a dropped FusedBA / MappingTrainer) must not run inside it."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def parked(graphs):
    """Keep ``graphs`` alive until the next ``release_parked()`` outside a capture."""
    _PARKED_GRAPHS.append(graphs)


def release_parked():
    if _PARKED_GRAPHS and not torch.cuda.is_current_stream_capturing():
        del _PARKED_GRAPHS[:]


def warm_up(device, fn, n: int):
    """``fn(0) .. fn(n - 1)`` on a side stream, ordered behind and in front of the current one, then a device synchronisation: what
    torch asks for in front of a capture."""
    s = torch.cuda.Stream(device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(s):
        for i in range(n):
            fn(i)
    torch.cuda.current_stream(device).wait_stream(s)
    torch.cuda.synchronize(device)


@contextlib.contextmanager
def preserved(tensors, optimizers=()):
    """Warm-up and capture iterations must not change the training state: ``tensors`` and the optimisers' state are cloned on entry and
    copied back BY VALUE on a clean exit -- a captured graph holds the addresses, so every tensor stays the object it was.
    A ``FusedAdam``: ``step_dev``, both moments and ``lag`` per parameter, ``_n_steps``.  A ``torch.optim.Adam``: its state dictionary."""
    from .trainer import FusedAdam
    tensors = list(tensors)
    snap = [t.detach().clone() for t in tensors]
    opt_snap = []
    for opt in optimizers:
        if isinstance(opt, FusedAdam):
            opt_snap.append((opt.step_dev.clone(), opt._n_steps, [(s['exp_avg'].clone(), s['exp_avg_sq'].clone(), s['lag']) for s in opt.state.values()]))
        else:
            opt_snap.append(copy.deepcopy(opt.state_dict()))
    yield
    with torch.no_grad():
        for t, q in zip(tensors, snap):
            t.copy_(q)
        for opt, sn in zip(optimizers, opt_snap):
            if isinstance(opt, FusedAdam):
                opt.step_dev.copy_(sn[0])
                opt._n_steps = sn[1]
                for s, (m0, v0, lag) in zip(opt.state.values(), sn[2]):
                    s['exp_avg'].copy_(m0)
                    s['exp_avg_sq'].copy_(v0)
                    s['lag'] = lag
            else:
                # torch.optim.Adam creates its state lazily: a fresh optimiser has none before capture.  The captured graphs
                # hold the state tensors' ADDRESSES, so restore by value into the existing tensors.
                had = sn['state']
                index = {id(q): i for i, q in enumerate(q for gp in opt.param_groups for q in gp['params'])}
                for p_, stt in opt.state.items():
                    idx = index[id(p_)]
                    for k, val in stt.items():
                        if torch.is_tensor(val):
                            if idx in had and k in had[idx]:
                                val.copy_(had[idx][k])
                            else:
                                val.zero_()

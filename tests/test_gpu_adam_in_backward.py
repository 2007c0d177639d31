"""The Adam steps inside the backward, each directly against the fp64 twin of torch.optim.Adam (tests/adam_spec.py): adam_apply (the four MLP
weights, wgrad_reduce_body), adam_apply4 from bwd_finish_body (LDS-tiled table levels) and from k_bin_apply (binned table levels, bins
without items included), and uncert_reduce_body's step of the uncertainty grid.

TrainStep.fuse_adam(..., write_grads=True): the finishing launch writes each gradient AND steps on it, so one iteration from prepared state
gives (p, m, v) before, the gradient the step consumed, and (p, m, v) after -- compared per element under the twin's bound, parameters and
both moments, with the workload's own settings (decoder: lr 0.01, eps 1e-8, wd 1e-6; table: lr 0.01, eps 1e-15; grid: lr 1, betas (0.9,
0.999)) at steps 1, 2 and 1000 read from the iteration counter.  The gradient itself is pinned to the oracle elsewhere; this isolates the step.

The gradients here are the backward's own, not drawn: where a product of the step underflows (|g| below ~1e-18) the bound's premise (v a
normal fp32 number) does not hold; those few entries (asserted: under 1 %) are held to the tiny-gradient property of test_gpu_adam.py instead."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_spec as A
import helpers as H
from naruto_amd import _lib, synthetic as syn, trainer

pytestmark = pytest.mark.gpu

N_RAYS = 64
FLAT = ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1")
BIN = 8192                         # entries per bin of the binned scatter (k_bin_apply: one slice per workgroup)
F_W, F_TILED, F_BINNED, F_GRID = "3 adam_apply (MLP weights)", "4 adam_apply4 (tiled levels)", "5 adam_apply4 (k_bin_apply)", "6 uncert_reduce_body"


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    A.dump_worst()


def _np(t):
    return t.detach().reshape(-1).cpu().numpy().copy()


def _seed_moments(m, v, seed):
    """Non-zero moments as in adam_spec.make_inputs: m = 0.3 randn mag, v = (U + 0.05) mag^2, 10 % of the entries zero in both."""
    rs = np.random.RandomState(seed)
    n = m.numel()
    mag = 10.0 ** rs.uniform(-9, -3, n)
    mm = (0.3 * rs.randn(n) * mag).astype(np.float32)
    vv = ((rs.rand(n) + 0.05) * mag * mag).astype(np.float32)
    z = rs.rand(n) < 0.1
    mm[z] = 0
    vv[z] = 0
    m.copy_(torch.from_numpy(mm).reshape(m.shape))
    v.copy_(torch.from_numpy(vv).reshape(v.shape))


def _rays(cfg, gpu, octant):
    bound = np.asarray(cfg["mapping"]["bound"], np.float64)
    if not octant:
        r = syn.random_rays(N_RAYS, bound, seed=3, zero_depth_frac=0.1)
    else:
        # origins in the low corner of the box, looking further into that corner: no sample reaches the upper half of any axis
        rs = np.random.RandomState(5)
        lo, ext = bound[:, 0], bound[:, 1] - bound[:, 0]
        d = -np.abs(rs.normal(size=(N_RAYS, 3))) - 0.2
        r = {"rays_o": (lo + ext * rs.uniform(0.15, 0.3, size=(N_RAYS, 3))).astype(np.float32),
             "rays_d": (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32),
             "target_d": rs.uniform(0.3, 0.8, size=(N_RAYS, 1)).astype(np.float32),
             "target_rgb": rs.uniform(0, 1, size=(N_RAYS, 3)).astype(np.float32)}
    return tuple(torch.from_numpy(r[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d"))


class Run:
    """One iteration of a fresh MappingTrainer's TrainStep, re-fused with ``write_grads``, from prepared state.  ``uncert``: None, or
    (t_own, lag, rides) for the grid's optimiser."""

    def __init__(self, gpu, log2_T, t, write_grads=True, octant=False, smooth=True, uncert=None):
        cfg = H.office_cfg(log2_T, perturb=1.0)
        torch.manual_seed(7)
        tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), gpu, fused_adam=True)
        self.tr, self.cfg, model, opt = tr, cfg, tr.model, tr.map_optimizer
        params = model._params()
        with torch.no_grad():
            params["table"].mul_(500.0)                       # tcnn's U(-1e-4, 1e-4) init scaled up so that the table matters
            self.settings = {}
            for gp in opt.param_groups:
                for p in gp["params"]:
                    name = next(n for n, q in params.items() if q is p)
                    self.settings[name] = dict(lr=gp["lr"], betas=tuple(gp["betas"]), eps=gp["eps"], wd=gp["weight_decay"])
                    if t > 1:
                        _seed_moments(*opt.moments(p), seed=100 + len(self.settings))
            tr.iter_state[1] = t - 1                          # the forward advances the iteration counter; the backward reads it as the step number
            ts = tr.train_step_for(N_RAYS, smooth)
            self.ts = ts
            assert ts.opt is not None and ts.S == 43
            entries = {n: opt.moments(params[n]) + (s["lr"], s["eps"], s["wd"]) for n, s in self.settings.items()}
            ts.fuse_adam(entries, self.settings["table"]["betas"], opt.external_step, write_grads=write_grads)
            uo, grid = tr.uncert_optim, model.uncert_grid
            gp = uo.param_groups[0]
            self.settings["uncert_grid"] = dict(lr=gp["lr"], betas=tuple(gp["betas"]), eps=gp["eps"], wd=gp["weight_decay"])
            t_own, lag, rides = uncert if uncert is not None else (1, 0, False)
            if uncert is not None:
                rs = np.random.RandomState(9)
                acc = (rs.randn(grid.numel()) * 10.0 ** rs.uniform(-8, -2, grid.numel())).astype(np.float32)
                grid.grad.copy_(torch.from_numpy(acc).reshape(grid.shape))      # what earlier iterations left accumulated
                if t_own > 1:
                    _seed_moments(*uo.moments(grid), seed=200)
                uo.step_dev.copy_(torch.tensor([t_own + lag - 1, 0], dtype=torch.int32))
            # (fuse_adam replaced the NarutoFusedAdam struct: the grid's optimiser is attached again, always, before anything rides)
            ts.fuse_uncert_adam(*uo.moments(grid), uo.step_dev, gp["lr"], gp["eps"], gp["weight_decay"], gp["betas"], lag)
            assert ts.grads["uncert_grid"].data_ptr() == grid.grad.data_ptr()
            self.rays = _rays(cfg, gpu, octant)
            self.before = {n: tuple(_np(x) for x in (params[n],) + opt.moments(params[n])) for n in FLAT}
            self.before["uncert_grid"] = tuple(_np(x) for x in (grid,) + uo.moments(grid))
            self.acc_before = _np(grid.grad)
            self.rode = ts.uncert_step_rides(rides)
            assert self.rode is bool(rides)
            try:
                ts.run(self.rays[0], self.rays[1], self.rays[2], self.rays[3].reshape(-1))
            finally:
                ts.uncert_step_rides(False)
            torch.cuda.synchronize()
            assert int(opt.external_step[0]) == t, "the iteration counter is the step number"
            self.after = {n: tuple(_np(x) for x in (params[n],) + opt.moments(params[n])) for n in FLAT}
            self.after["uncert_grid"] = tuple(_np(x) for x in (grid,) + uo.moments(grid))
            self.acc_after = _np(grid.grad)
            self.word = uo.step_dev.tolist()
            self.grads = {n: _np(ts.grads[n]) for n in FLAT} if write_grads else None
            self.out = {k: _np(getattr(ts, k)) for k in ("rgb", "depth", "losses")}
            _sc, _res, self.size, self.off = model._handle().levels()


def _check_step(before, g, after, kw, t, what, form, sel=None):
    """after == twin(before, g) under the bound, on the entries ``sel``; -> the twin."""
    pick = (lambda x: x) if sel is None else (lambda x: x[sel])
    b = tuple(pick(x) for x in before)
    g = pick(g)
    got = tuple(pick(x) for x in after)
    tw = A.adam_twin(b[0], g, b[1], b[2], t=t, **kw)
    mask = A.bound_applies(b[0], g, b[1], b[2], **kw)
    assert mask.mean() >= 0.99, f"{what}: the bound's premise holds on {mask.mean():.4f} of the entries only"
    r = A.assert_within(got, tw, what, form, mask=mask)
    print(f"{what}: |error| / bound  p {r[0]:.3f}  m {r[1]:.3f}  v {r[2]:.3f}  ({int((~mask).sum())} of {mask.size} entries underflow)")
    if not mask.all():
        rest = ~mask
        S = float(np.float32(kw["lr"])) / (1.0 - float(np.float32(kw["betas"][0])) ** t)
        cap = S * np.abs(tw[1][rest]) / float(np.float32(kw["eps"])) * (1.0 + 1e-3) + np.spacing(np.abs(b[0][rest])).astype(np.float64)
        moved = np.abs(got[0][rest].astype(np.float64) - b[0][rest].astype(np.float64))
        assert all(np.isfinite(x[rest]).all() for x in got) and (moved <= cap).all(), f"{what}: an entry whose gradient underflows misbehaves"
    return tw


def _level_split(run):
    """float index ranges of the LDS-tiled levels (up to 2^17 entries) and of the binned ones."""
    n = run.before["table"][0].size
    tiled, binned = np.zeros(n, bool), np.zeros(n, bool)
    for l, sz in enumerate(run.size):
        (binned if sz > (1 << 17) else tiled)[2 * run.off[l]:2 * run.off[l + 1]] = True
    assert (tiled ^ binned).all()
    return tiled, binned


def _check_map_tensors(run, t, what):
    tiled, binned = _level_split(run)
    for name in FLAT[1:]:
        g = run.grads[name]
        assert np.abs(g).max() > 0, f"{what}: {name} received no gradient"
        _check_step(run.before[name], g, run.after[name], run.settings[name], t, f"{what} {name}", F_W)
    g = run.grads["table"]
    for sel, form, label in ((tiled, F_TILED, "tiled levels"), (binned, F_BINNED, "binned levels")):
        if sel.any():
            assert np.abs(g[sel]).max() > 0, f"{what}: the {label} received no gradient"
            _check_step(run.before["table"], g, run.after["table"], run.settings["table"], t, f"{what} table, {label}", form, sel=sel)
    return tiled, binned


def test_settings_are_the_workloads_rows(gpu):
    run = Run(gpu, 12, 1)
    f32 = lambda row: tuple(np.float32(x) for x in row)
    as_row = lambda s: f32((s["betas"][0], s["betas"][1], s["lr"], s["eps"], s["wd"]))
    for name in FLAT[1:]:
        assert as_row(run.settings[name]) == f32(A.ROWS["a"])
    assert as_row(run.settings["table"]) == f32(A.ROWS["b"]) and as_row(run.settings["uncert_grid"]) == f32(A.ROWS["c"])


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("log2_T", [12, 18])
def test_steps_in_the_finishing_launch_match_the_twin(gpu, log2_T, t):
    """log2 12: every level LDS-tiled (bwd_finish_body); log2 18: levels 7 .. 15 through the binned scatter (k_bin_apply)."""
    run = Run(gpu, log2_T, t)
    tiled, binned = _check_map_tensors(run, t, f"T 2^{log2_T} t {t}")
    assert binned.any() == (log2_T == 18) and tiled.any()
    # the grid's optimiser did not ride: its gradient accumulated, nothing else of it moved
    for a, b in zip(run.before["uncert_grid"], run.after["uncert_grid"]):
        assert np.array_equal(a, b)
    assert run.word == [0, 0]


def test_bins_without_items_are_stepped(gpu):
    """Rays confined to the low corner of the box, moments non-zero everywhere: a bin that received no item still takes the step with g = 0
    (its moments decay, its parameters move).  Without the smoothness term: its lattice (32^3 points, 0.1 m apart) reaches every slab of the
    box and with it every bin of the dense binned level."""
    t = 2
    run = Run(gpu, 18, t, octant=True, smooth=False)
    tiled, binned = _check_map_tensors(run, t, "corner rays")
    g, (p0, m0, v0), (p1, m1, v1) = run.grads["table"], run.before["table"], run.after["table"]
    empty = []
    for l, sz in enumerate(run.size):
        if sz <= (1 << 17):
            continue
        for c in range(-(-sz // BIN)):
            s = slice(2 * (run.off[l] + c * BIN), 2 * min(run.off[l] + (c + 1) * BIN, run.off[l + 1]))
            if not g[s].any():
                empty.append((l, c))
                assert np.abs(m0[s]).max() > 0 and not np.array_equal(m0[s], m1[s]) and not np.array_equal(p0[s], p1[s]), \
                    f"level {l} bin {c}: no items and no step"
    print(f"{len(empty)} bins without items, first {empty[:4]}")
    assert empty, "every bin received a gradient: the case does not test what it is for"


def test_forward_weight_image_holds_the_new_weights(gpu):
    """After the step, a second iteration whose forward reads the maintained image (fwd_image_fresh) and one whose forward stages the new
    weights itself give the same bits everywhere."""
    outs = []
    for fresh in (True, False):
        run = Run(gpu, 12, 2)
        ts = run.ts
        assert ts.fwd_image is not None
        plan = (C.c_uint32 * 8)()
        _lib.check(_lib.load().naruto_debug_train_plan(run.tr.model._handle().ptr, C.byref(ts.t), 1, 1, plan))
        assert plan[0] in (1, 3), f"launch form {plan[0]}: not a forward that reads the weight image"
        with torch.no_grad():
            assert ts.fwd_image_fresh(fresh) is fresh
            try:
                ts.run(run.rays[0], run.rays[1], run.rays[2], run.rays[3].reshape(-1))
            finally:
                ts.fwd_image_fresh(False)
            torch.cuda.synchronize()
        out = {k: _np(getattr(ts, k)) for k in ("rgb", "depth", "uncert_map", "losses", "raw", "z_vals")}
        params = run.tr.model._params()
        for n in FLAT:
            for x, what in zip((params[n],) + run.tr.map_optimizer.moments(params[n]), "pmv"):
                out[f"{n}.{what}"] = _np(x)
        assert not np.array_equal(out["sdf_w0.p"], run.after["sdf_w0"][0]) and not np.array_equal(run.before["sdf_w0"][0], run.after["sdf_w0"][0])
        outs.append(out)
    for k in outs[0]:
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32)), \
            f"{k}: the iteration whose forward read the weight image differs from the one that staged the new weights"


@pytest.mark.parametrize("log2_T", [12, 18])
def test_writing_the_gradients_changes_no_bit_of_the_step(gpu, log2_T):
    a, b = Run(gpu, log2_T, 2, write_grads=True), Run(gpu, log2_T, 2, write_grads=False)
    for name in FLAT:
        for x, y, what in zip(a.before[name], b.before[name], "pmv"):
            assert np.array_equal(x, y), f"{name} {what}: the two runs did not start from the same state"
        for x, y, what in zip(a.after[name], b.after[name], "pmv"):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{name} {what}: write_grads changes the step"
    assert not np.array_equal(a.before["table"][0], a.after["table"][0])


@pytest.mark.parametrize("lag", [0, 3])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_uncert_grid_step_in_the_finishing_launch(gpu, t, lag):
    """The grid's step rides (uncert_step_rides): lr 1, betas (0.9, 0.999), the word preset so that the grid's own step number is t (the
    launch is step t + lag).  The gradient it consumes is the accumulated one plus this iteration's sum: read from an identical run in which
    the step does not ride (the backward is bitwise reproducible; everything else of the two runs must agree)."""
    a, b = Run(gpu, 12, 5, uncert=(t, lag, True)), Run(gpu, 12, 5, uncert=(t, lag, False))
    for name in FLAT:
        for x, y in zip(a.after[name] + (a.grads[name],), b.after[name] + (b.grads[name],)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{name}: the riding step changed something else"
    for k in a.out:
        assert np.array_equal(a.out[k].view(np.uint32), b.out[k].view(np.uint32)), k
    assert np.array_equal(a.acc_before, b.acc_before) and b.word == [t + lag - 1, 0]
    for x, y in zip(b.before["uncert_grid"], b.after["uncert_grid"]):
        assert np.array_equal(x, y)
    g = b.acc_after                                           # accumulated + this iteration's sum, the same fp32 addition
    touched = g != a.acc_before
    assert touched.any() and not touched.all()
    kw = a.settings["uncert_grid"]
    _check_step(a.before["uncert_grid"], g, a.after["uncert_grid"], kw, t, f"grid t {t} lag {lag}", F_GRID)
    _check_step(a.before["uncert_grid"], a.acc_before, a.after["uncert_grid"], kw, t, f"grid t {t} lag {lag}, voxels no ray touched", F_GRID, sel=~touched)
    assert not a.acc_after.any(), "the accumulated gradient was not zeroed"
    assert a.word == [t + lag, 0], a.word
    wrong = A.adam_twin(a.before["uncert_grid"][0], g, *a.before["uncert_grid"][1:], t=t + 1, **kw)
    assert A.share_over_bound(a.after["uncert_grid"][0], wrong) >= 0.5, "a step number off by one would pass"

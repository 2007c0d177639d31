"""The uncertainty grid's Adam step in the backward's finishing launch (NarutoFusedAdam.uncert_step, MappingTrainer.uncert_in_finish): on the
iterations where the grid's optimiser steps, the thread that finishes voxel v's gradient applies the step and zeroes the gradient, instead of a
launch of k_adam_multi behind the backward.  Same arithmetic in the same order: a chain of ten iterations (grid steps at 5 and 10) run with the
fold and with the separate launch from identical state must leave identical bits everywhere -- the grid, its two moments, its step count, its
accumulated gradient, every map parameter and moment -- through MappingTrainer.capture(chain=...) and through FusedBA.call_iterations()."""
import pytest
import torch

import helpers as H
from naruto_amd import synthetic as syn, trainer
from test_gpu_fwd_image import _ba_scene

pytestmark = pytest.mark.gpu

CHAIN = [(i + 1) % 5 == 0 for i in range(10)]
N_RAYS = 64


def _cfg(n_samples_d):
    return H.office_cfg(12, perturb=1.0, n_samples_d=n_samples_d)


def _trainer(cfg, gpu, seed=7):
    torch.manual_seed(seed)
    return trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), gpu, fused_adam=True)


def _same_state(dst, src):
    dst.model.load_state_dict(src.model.state_dict())
    dst.iter_state.copy_(src.iter_state)


def _state(tr, ret):
    grid = tr.model.uncert_grid
    m, v = tr.uncert_optim.moments(grid)
    out = {"rgb": ret["rgb"].clone(), "depth": ret["depth"].clone(), "losses": ret["_losses"].clone(),
           "grid": grid.detach().clone(), "grid.exp_avg": m.clone(), "grid.exp_avg_sq": v.clone(), "grid.step": tr.uncert_optim.step_dev.clone(),
           "grid.grad": grid.grad.clone()}
    for n, p in tr.model.named_parameters():
        out["p." + n] = p.detach().clone()
    for i, gp in enumerate(tr.map_optimizer.param_groups):
        for j, p in enumerate(gp["params"]):
            mm, vv = tr.map_optimizer.moments(p)
            out[f"m.{i}.{j}"], out[f"v.{i}.{j}"] = mm.clone(), vv.clone()
    return out


def _assert_equal_states(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max |d| {(a[k].double() - b[k].double()).abs().max().item():.3e})"


def _assert_stepped(st, n_steps, what):
    assert int(st["grid.step"][0]) == n_steps and int(st["grid.step"][1]) == 0, (what, st["grid.step"].tolist())
    assert float(st["grid.exp_avg_sq"].abs().max()) > 0.0, f"{what}: the grid's optimiser never saw a gradient"
    assert float(st["grid.grad"].abs().max()) == 0.0, f"{what}: the accumulated gradient was not zeroed by the step that closes the chain"


@pytest.mark.parametrize("n_samples_d", [32, 117])            # 64 rays x 43 and 64 x 128
def test_chain_with_the_fold_gives_the_same_bits(gpu, n_samples_d):
    cfg = _cfg(n_samples_d)
    r = syn.random_rays(N_RAYS, cfg["mapping"]["bound"], seed=3, zero_depth_frac=0.1)
    rays = tuple(torch.from_numpy(r[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d"))
    twins = []
    for fold in (True, False):
        tr = _trainer(cfg, gpu)
        if twins:
            _same_state(tr, twins[0])
        tr.capture(N_RAYS, smooth=True, chain=CHAIN, uncert_in_finish=fold)
        assert tr.uncert_in_finish is fold
        assert tr._static["ts"].opt.uncert_step == 0             # outside an iteration nobody is told to step the grid
        twins.append(tr)
    a, b = twins
    _same_state(b, a)
    for tr in twins:
        for buf, x in zip(tr.ray_buffers(), rays):
            buf.copy_(x.reshape(buf.shape))
    ra, _ = a.step_chain()
    rb, _ = b.step_chain()
    sa, sb = _state(a, ra), _state(b, rb)
    _assert_stepped(sa, 2, "fold")
    _assert_stepped(sb, 2, "separate launch")
    _assert_equal_states(sa, sb, "one chain of ten iterations")
    ra, _ = a.step_chain()
    rb, _ = b.step_chain()
    _assert_equal_states(_state(a, ra), _state(b, rb), "two chains")


@pytest.mark.parametrize("n_samples_d", [32, 117])
def test_fused_ba_call_with_the_fold_gives_the_same_bits(gpu, n_samples_d):
    from naruto_amd.ba_loop import FusedBA
    cfg = _cfg(n_samples_d)
    cfg["mapping"].update(sample=N_RAYS, min_pixels_cur=4, filter_depth=True, keyframe_every=5, iters=len(CHAIN))
    twins = []
    for fold in (True, False):
        tr = _trainer(cfg, gpu)
        tr.uncert_in_finish = fold                             # (FusedBA captures through MappingTrainer.capture, which leaves the switch as it is)
        store, current, poses = _ba_scene(cfg, gpu)
        twins.append((FusedBA(tr, store, None, max_poses=16, use_graph=True), current, poses, fold))
    _same_state(twins[1][0].trainer, twins[0][0].trainer)
    out = []
    for ba, current, poses, fold in twins:
        for _ in range(2):
            ret, _loss = ba.global_BA(current, poses)             # prepare (captures on the first call) + call_iterations: one replay
        assert ba.trainer.chain_length() == len(CHAIN) and ba.trainer.uncert_in_finish is fold
        out.append(_state(ba.trainer, ret))
    assert int(out[0]["grid.step"][0]) >= 4 and int(out[0]["grid.step"][1]) == 0, out[0]["grid.step"].tolist()      # steps at 5 and 10 of both calls
    _assert_equal_states(out[0], out[1], "two global_BA calls")

"""FusedBA(optimize_poses=True): the pose optimiser inside global_BA on the device (naruto_amd/ba_loop.py states the contract; parity
unpinned).  Scene and oracle loop: tests/ba_pose_scene.py -- the AnalyticRoom camera ring, a field mapped from the true poses, five
keyframes + the current frame, poses 1.. perturbed by 1 degree / 2.5 cm.  The reference for values is the contract restated in torch
around the CPU oracle (B.OracleBA) on the device's own drawn rows (pose ids, targets and world directions read back from the batch
buffers; the camera-frame directions are the world ones rotated back with the matrices the batch was formed from) and an explicit
depth jitter.  Where a comparison is about poses the oracle's network parameters are copied from the device before every iteration
(whole-iteration parity of the network is test_gpu_parity.py's business); the poses evolve independently on the two sides."""
import copy
import gc

import numpy as np
import pytest
import torch

import ba_pose_scene as B
import helpers as H
from naruto_amd import _lib, trainer
from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
from naruto_amd.ba_loop import FusedBA
from naruto_amd.keyframe_store import KeyFrameStoreHIP

pytestmark = pytest.mark.gpu

S_ = 43


def _env(gpu, active=False, use_graph=False, prefetch=None, n_kf=B.N_KF, bf16=False, optimize_poses=None, feature_args=True, **mapping):
    mapping.setdefault("min_pixels_cur", 100)          # n_cur stays when a keyframe is added: no re-capture
    c = B.cfg(**mapping)
    if bf16:
        c["decoder"]["mlp_precision"] = "bf16"
    sc = B.scene(c)
    torch.manual_seed(33)
    tr = trainer.MappingTrainer(c, torch.tensor(c["mapping"]["bound"], dtype=torch.float32), gpu, B.UNCERT_VOXEL, fused_adam=True)
    B.load_trainer(tr)
    store = KeyFrameStoreHIP(c, B.HH, B.WW, num_kf=B.N_KF + 3, num_rays_to_save=B.R_SAVE, device=gpu, seed=11)
    frames = [B.frame(sc, k) for k in range(B.N_KF + 2)]
    for k in range(n_kf):
        store.add_keyframe(frames[k], filter_depth=True)
    smp = ActiveRaySamplerHIP(config=c, num_uncert_sample=64, oversample_mul=4) if active else None
    kw = dict(optimize_poses=optimize_poses) if feature_args else {}
    ba = FusedBA(tr, store, smp, max_poses=16, use_graph=use_graph, prefetch=prefetch, **kw)
    rs = np.random.RandomState(7)
    vol = (rs.uniform(0, 3, (49, 56, 35)) * (rs.uniform(size=(49, 56, 35)) < 0.5)).astype(np.float32) if active else None
    true = B.true_poses(sc, B.N_KF + 2)
    return {"cfg": c, "scene": sc, "tr": tr, "store": store, "frames": frames, "ba": ba, "vol": vol, "true": true, "n_kf": n_kf,
            "current": B.current_rays(frames[n_kf]), "poses": B.perturbed(true[:n_kf + 1]), "gpu": gpu}


def _done(*envs):
    """Tear an environment down NOW (its FusedBA, trainer and graphs form reference cycles: left to the cyclic collector they would be
    destroyed at an arbitrary later moment, possibly inside the next environment's stream capture)."""
    for env in envs:
        env["ba"].close()
        env.clear()
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(autouse=True)
def _collect_between_tests():
    yield
    gc.collect()


def _params(tr):
    return {n: p.detach().clone() for n, p in B.hip_params(tr.model).items()}


def _same_params(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: parameter {n} differs"


def _pose_ids(ba, P):
    pb = ba._pose
    ids = pb["ids"].cpu()
    if pb["src_rows"] is not None:
        ids = ids[pb["src_rows"].cpu().long()]
    else:
        ids = ids[:ba._eager_bufs[0].shape[0]]
    return torch.where(ids < 0, torch.full_like(ids, P - 1), ids)


def _refine_call(env, ora, poses, n_iters, rand_seed, pose6_oracle=None):
    """One EAGER call (prefetch off) with explicit jitter and the oracle loop alongside on the device's rows.  Returns the oracle loop and
    the device's trace."""
    ba, c, gpu = env["ba"], env["cfg"], env["gpu"]
    assert not ba.use_graph and not ba.prefetch
    P = poses.shape[0]
    n_cur, n_train = ba.prepare(env["current"], poses, env["vol"], optimize_poses=True)
    first = ba.last_pose_trace()
    o = B.OracleBA(ora, c, first["pose6"] if pose6_oracle is None else pose6_oracle)
    ts = ba.trainer._train_step(n_train, True)
    g = torch.Generator().manual_seed(rand_seed)
    ts.explicit_jitter(True)
    try:
        for i in range(n_iters):
            rand = torch.rand(n_train, S_, generator=g)
            ts.rand[:n_train * S_].copy_(rand.reshape(-1).to(gpu))
            B.sync_oracle(ora, ba.trainer.model)
            R_dev = ba.poses[:P, :3, :3].double().cpu()           # the matrices this iteration's batch is formed from
            ba.iteration(i)
            assert ba.trainer._train_step(n_train, True) is ts
            _, rays_d, rgb, dep = (b.cpu() for b in ba._eager_bufs)
            pid = _pose_ids(ba, P)
            d_cam = torch.einsum("nk,nkj->nj", rays_d.double(), R_dev[pid]).float()
            o.iteration(i, d_cam, pid, rgb, dep.reshape(-1), rand)
    finally:
        ts.explicit_jitter(False)
    return o, ba.last_pose_trace()


# --------------------------------------------------------------------------------------------- 1. the accumulated gradient
@pytest.mark.parametrize("active,accum,optim_cur", [(False, 5, True), (True, 5, True), (False, 1, False)])
def test_accumulated_pose_gradient_matches_oracle_autograd(gpu, active, accum, optim_cur):
    """After the first window (iterations 1 .. pose_accum_step, poses at their initial values) the traced [P,6] gradient equals the
    oracle's accumulated omega.grad / t.grad within helpers.grad_close, the omega and the t block separately; pose 0's row (and the
    current row with optim_cur off) is exactly zero and the pose untouched.  pose_accum_step = 1: a one-iteration window."""
    env = _env(gpu, active=active, prefetch=False, pose_accum_step=accum, optim_cur=optim_cur)
    ora = B.load_oracle(env["cfg"])
    P = env["poses"].shape[0]
    o, tr = _refine_call(env, ora, env["poses"], accum, 5)
    assert tr["n_steps"] == 1 and tr["iterations"] == accum and len(o.trace) == 1
    pose_o, grad_o = o.trace[0]
    assert torch.equal(tr["pose"][0], pose_o), "both sides start from the same (omega, t)"
    got = tr["grad"][0]
    print(f"active={active} accum={accum}: |d_omega| max {float(grad_o[:, :3].abs().max()):.4g} (err {float((got[:, :3] - grad_o[:, :3]).abs().max()):.3g}), "
          f"|d_t| max {float(grad_o[:, 3:].abs().max()):.4g} (err {float((got[:, 3:] - grad_o[:, 3:]).abs().max()):.3g})")
    H.grad_close(got[:, :3], grad_o[:, :3], "accumulated d_omega")
    H.grad_close(got[:, 3:], grad_o[:, 3:], "accumulated d_t")
    fixed = [0] + ([] if optim_cur else [P - 1])
    refined = env["ba"].refined_poses().cpu()
    for p in fixed:
        assert torch.equal(got[p], torch.zeros(6)), f"pose {p} is fixed: its gradient row is zero"
        assert torch.equal(refined[p], env["poses"][p]), f"pose {p} is fixed: the caller's bits"
    for p in range(1, P - 1):
        assert float(got[p].abs().max()) > 0 and not torch.equal(refined[p], tr["init_c2w"][p].cpu())


# --------------------------------------------------------------------------------------------- 2. the trajectory
def test_pose_trajectory_matches_oracle_loop(gpu):
    """A whole 10-iteration call (two pose steps, the network stepping every iteration): the poses after each pose step match the oracle
    loop's within 2e-5 on every stepped component whose reference gradient at that step exceeds 10 x test 1's bound; at most 5 % of
    the stepped components may be left out."""
    env = _env(gpu, prefetch=False)
    ora = B.load_oracle(env["cfg"])
    o, tr = _refine_call(env, ora, env["poses"], 10, 6)
    assert tr["n_steps"] == 2 and len(o.trace) == 2
    after_dev = [tr["pose"][1], tr["pose6"]]
    after_ora = [o.trace[1][0], o.pose6()]
    n_all = n_out = 0
    for s in range(2):
        keep = B.trajectory_mask(o.trace[s][1]) & o.mask[:, None]
        n_all += int(o.mask.sum()) * 6
        n_out += int(o.mask.sum()) * 6 - int(keep.sum())
        err = (after_dev[s] - after_ora[s]).abs()
        print(f"pose step {s}: max error on compared components {float(err[keep].max()):.3g}, left out {int(o.mask.sum()) * 6 - int(keep.sum())}")
        assert float(err[keep].max()) <= 2e-5, (s, err)
        assert torch.equal(after_dev[s][~o.mask], after_ora[s][~o.mask])
    assert n_out <= 0.05 * n_all, f"{n_out} of {n_all} stepped components left out"


# --------------------------------------------------------------------------------------------- 3. the mapping is untouched
@pytest.mark.parametrize("zero_lr", [False, True])
def test_mapping_is_untouched_inside_a_window(gpu, zero_lr):
    """With pose optimisation on, parameters, losses and drawn batches of iterations 1 .. pose_accum_step are bit-identical to a call
    with it off that is given the refining call's initial matrices; with lr_rot = lr_trans = 0 the same holds for the whole call and
    the returned poses equal the initial ones bit for bit."""
    lr = dict(lr_rot=0.0, lr_trans=0.0) if zero_lr else {}
    a = _env(gpu, active=True, **lr)
    b = _env(gpu, active=True, **lr)
    n = 10 if zero_lr else 5
    a["ba"].prepare(a["current"], a["poses"], a["vol"], optimize_poses=True)
    init = a["ba"].last_pose_trace()["init_c2w"]
    b["ba"].prepare(b["current"], init, b["vol"], optimize_poses=False)
    assert a["ba"]._pose_on and not b["ba"]._pose_on
    for i in range(n):
        (_, la), (_, lb) = a["ba"].iteration(i), b["ba"].iteration(i)
        assert float(la) == float(lb), f"iteration {i}: loss"
        for x, y in zip(a["ba"]._eager_bufs, b["ba"]._eager_bufs):
            assert torch.equal(x, y), f"iteration {i}: batch"
    _same_params(_params(a["tr"]), _params(b["tr"]), "refining vs plain call")
    assert torch.equal(a["tr"].iter_state, b["tr"].iter_state)
    if zero_lr:
        assert a["ba"].last_pose_trace()["n_steps"] == 2
        assert torch.equal(a["ba"].refined_poses(), init), "lr 0: the poses stay"


# --------------------------------------------------------------------------------------------- 4. the routes agree
def _call(env, n_calls=1, grow=False):
    ba = env["ba"]
    poses, current = env["poses"], env["current"]
    out = []
    for k in range(n_calls):
        if grow and k == 1:
            ba.store.add_keyframe(env["frames"][env["n_kf"]], filter_depth=True)
            current = B.current_rays(env["frames"][env["n_kf"] + 1])
            poses = torch.cat([ba.refined_poses().cpu(), B.perturbed(env["true"][:env["n_kf"] + 2])[-1:]], 0)
            graphs_before = ba.trainer._graphs
        ba.global_BA(current, poses, uncert_vol=env["vol"], optimize_poses=True)
        if grow and k == 1 and ba.use_graph:
            assert ba.trainer._graphs is graphs_before, "P grew, the ray count did not: no re-capture"
        out.append(ba.refined_poses().clone())
    torch.cuda.synchronize()
    return out, _params(env["tr"])


@pytest.mark.parametrize("active", [False, True])
def test_routes_agree_bit_for_bit(gpu, active, monkeypatch):
    """Eager, per-iteration graphs and the call graph give the same pose bits and parameter bits; prefetch on / off and keyed / unkeyed
    selection likewise; a second run from the same state repeats; a second call after P has grown (one more keyframe, same ray counts)
    replays without re-capture and still matches eager."""
    env = _env(gpu, active=active, prefetch=False)
    ref_poses, ref_params = _call(env, 2, grow=True)
    _done(env)
    assert not torch.equal(ref_poses[0], ref_poses[1][:-1])
    routes = {"eager again": dict(prefetch=False), "eager + prefetch": dict(prefetch=True), "call graph": dict(use_graph=True),
              "call graph, no prefetch": dict(use_graph=True, prefetch=False)}
    for name, kw in routes.items():
        env = _env(gpu, active=active, **kw)
        poses, params = _call(env, 2, grow=True)
        if env["ba"].use_graph:
            assert env["tr"].chain_length() == 10
        for k in range(2):
            assert torch.equal(poses[k], ref_poses[k]), f"{name}: poses of call {k}"
        _same_params(params, ref_params, name)
        _done(env)
    # per-iteration graphs: the same call iteration by iteration
    env = _env(gpu, active=active, use_graph=True)
    env["ba"].prepare(env["current"], env["poses"], env["vol"], optimize_poses=True)
    for i in range(10):
        env["ba"].iteration(i)
    assert torch.equal(env["ba"].refined_poses(), ref_poses[0]), "per-iteration graphs: poses"
    _done(env)
    if active:
        monkeypatch.setenv("NARUTO_BA_KEYED_SELECT", "0")
        env = _env(gpu, active=True, use_graph=True)
        assert not env["ba"].keyed
        poses, params = _call(env, 2, grow=True)
        assert torch.equal(poses[1], ref_poses[1]), "unkeyed selection: poses"
        _same_params(params, ref_params, "unkeyed selection")
        _done(env)


# --------------------------------------------------------------------------------------------- 5. it refines
def test_refinement_recovers_the_poses(gpu):
    """B.REFINE's schedule on the perturbed poses, the oracle loop alongside on the same draws (each side feeds its own refined poses
    into the next call): the oracle loop's mean errors drop below 0.7 x the start (else the schedule is no test) and the device's final
    errors are at most 1.25 x the oracle's + 0.02 degrees / 2 mm."""
    sch = B.REFINE
    env = _env(gpu, active=True, prefetch=False, lr_rot=sch["lr_rot"], lr_trans=sch["lr_trans"], pose_accum_step=sch["pose_accum_step"])
    ora = B.load_oracle(env["cfg"])
    true = env["true"][:env["n_kf"] + 1]
    poses_dev = env["poses"]
    poses_ora = env["poses"]
    from naruto_amd.tracking import matrices_to_pose6
    for k in range(sch["calls"]):
        o, _ = _refine_call(env, ora, poses_dev, 10, 100 + k, pose6_oracle=matrices_to_pose6(poses_ora).float())
        poses_dev = env["ba"].refined_poses().cpu()
        poses_ora = B.pose6_matrices(o.pose6()).float()
    e0, eh, eo = B.errors(env["poses"], true), B.errors(poses_dev, true), B.errors(poses_ora, true)
    print(f"BA pose refinement: start {e0[0]:.3f} deg {100 * e0[1]:.2f} cm; oracle {eo[0]:.3f} deg {100 * eo[1]:.2f} cm; HIP {eh[0]:.3f} deg {100 * eh[1]:.2f} cm")
    assert eo[0] < 0.7 * e0[0] and eo[1] < 0.7 * e0[1], "the oracle's own loop does not recover the poses: the schedule is not a test"
    assert eh[0] <= 1.25 * eo[0] + 0.02 and eh[1] <= 1.25 * eo[1] + 0.002, (eh, eo)


# --------------------------------------------------------------------------------------------- 6. off means off, and refusals
def test_off_means_off(gpu):
    """optimize_poses=False, or fewer than 2 keyframes: the poses returned are the caller's bits, nothing of the feature is attached
    to the training step, and the trajectory is the one of a FusedBA built without the feature's arguments."""
    plain = _env(gpu, active=True, use_graph=True, feature_args=False)
    plain["ba"].global_BA(plain["current"], plain["poses"], uncert_vol=plain["vol"])
    off = _env(gpu, active=True, use_graph=True, optimize_poses=False)
    off["ba"].global_BA(off["current"], off["poses"], uncert_vol=off["vol"], optimize_poses=False)
    assert not off["ba"]._pose_on and off["ba"]._bap is None and off["tr"]._static["ts"].ba_poses is None
    _same_params(_params(off["tr"]), _params(plain["tr"]), "optimize_poses=False")
    assert torch.equal(off["ba"].refined_poses().cpu(), off["poses"])
    with pytest.raises(RuntimeError, match="did not optimise"):
        off["ba"].last_pose_trace()
    one = _env(gpu, n_kf=1, optimize_poses=True)
    one["ba"].global_BA(one["current"], one["poses"], n_iters=3)
    assert not one["ba"]._pose_on and torch.equal(one["ba"].refined_poses().cpu(), one["poses"])
    ref = _env(gpu, n_kf=1, feature_args=False)
    ref["ba"].global_BA(ref["current"], ref["poses"], n_iters=3)
    _same_params(_params(one["tr"]), _params(ref["tr"]), "fewer than 2 keyframes")
    # on, then off on the same object: the training step goes back to the plain backward
    both = _env(gpu, active=True, use_graph=True)
    both["ba"].global_BA(both["current"], both["poses"], uncert_vol=both["vol"], optimize_poses=True)
    assert both["tr"]._static["ts"].ba_poses is not None
    both["ba"].global_BA(both["current"], both["poses"], uncert_vol=both["vol"], optimize_poses=False)
    assert both["tr"]._static["ts"].ba_poses is None
    assert torch.equal(both["ba"].refined_poses().cpu(), both["poses"])


def test_refusals_raise_before_any_launch(gpu):
    env = _env(gpu)
    ba = env["ba"]
    state0 = ba.trainer.iter_state.clone()
    args = (env["current"], env["poses"])
    cfg0 = copy.deepcopy(ba.config)
    ba.config["training"]["rot_rep"] = "quat"
    with pytest.raises(NotImplementedError, match="rot_rep"):
        ba.global_BA(*args, optimize_poses=True)
    ba.config["training"]["rot_rep"] = "axis_angle"
    ba.config["mapping"]["map_accum_step"] = 2
    with pytest.raises(NotImplementedError, match="map_accum_step"):
        ba.global_BA(*args, optimize_poses=True)
    ba.config["mapping"]["map_accum_step"] = 1
    ba.config["mapping"]["map_wait_step"] = 3
    with pytest.raises(NotImplementedError, match="map_wait_step"):
        ba.global_BA(*args, optimize_poses=True)
    ba.config["mapping"]["map_wait_step"] = 0
    assert ba.config == cfg0
    grp, ba.trainer.group = ba.trainer.group, object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        ba.global_BA(*args, optimize_poses=True)
    ba.trainer.group = grp
    act = _env(gpu, active=True)
    one = FusedBA(act["tr"], act["store"], act["ba"].sampler, max_poses=16, use_graph=False, one_launch_prologue=True)
    with pytest.raises(NotImplementedError, match="one_launch_prologue"):
        one.global_BA(act["current"], act["poses"], uncert_vol=act["vol"], optimize_poses=True)
    assert torch.equal(ba.trainer.iter_state, state0), "nothing ran"
    # the C entry points: NULL / out-of-range fields
    lib = _lib.load()
    import ctypes as C
    b = _lib.NarutoBAPoses()
    assert lib.naruto_ba_poses_init(C.byref(b), None) != 0 and b"max_poses" in lib.naruto_last_error()
    b.max_poses, b.pose_accum_step = 16, 5
    assert lib.naruto_ba_poses_init(C.byref(b), None) != 0 and b"NULL buffer" in lib.naruto_last_error()


# --------------------------------------------------------------------------------------------- 7. bf16 mode
def test_bf16_mode_refines_close_to_fp32(gpu):
    """After one call from the same state, draws and jitter the bf16 MLP mode's poses lie within 0.05 degrees / 2 mm of the fp32 mode's."""
    out = []
    for bf16 in (False, True):
        env = _env(gpu, active=True, use_graph=True, bf16=bf16)
        env["ba"].global_BA(env["current"], env["poses"], uncert_vol=env["vol"], optimize_poses=True)
        out.append(env["ba"].refined_poses().double().cpu())
        assert env["ba"].last_pose_trace()["n_steps"] == 2
        _done(env)
    worst = [max(B.errors(out[1], out[0], rows=[k])[j] for k in range(1, out[0].shape[0])) for j in (0, 1)]
    print(f"bf16 vs fp32 after one call: {worst[0]:.4f} deg {1000 * worst[1]:.3f} mm")
    assert worst[0] <= 0.05 and worst[1] <= 0.002, worst


# --------------------------------------------------------------------------------------------- 8. captures and the collector
def test_no_finaliser_runs_inside_a_capture(gpu, monkeypatch):
    """A dropped FusedBA (with its trainer and graphs, in reference cycles) is destroyed whenever the cyclic collector gets to it; inside
    another object's stream capture that would end the capture with an error.  prepare() collects BEFORE it captures and keeps the
    collector off until the capture has ended."""
    import weakref
    events = []
    dead = _env(gpu, use_graph=True, prefetch=False)
    dead["ba"].global_BA(dead["current"], dead["poses"], optimize_poses=True)
    torch.cuda.synchronize()
    weakref.finalize(dead["ba"], lambda: events.append("finalised"))
    dead.clear()
    env = _env(gpu, use_graph=True, prefetch=False)
    orig = env["tr"].capture

    def capture(*a, **kw):
        events.append("capture begins")
        assert not gc.isenabled()
        out = orig(*a, **kw)
        assert not gc.isenabled()
        return out
    monkeypatch.setattr(env["tr"], "capture", capture)
    assert gc.isenabled()
    env["ba"].global_BA(env["current"], env["poses"], optimize_poses=True)
    assert gc.isenabled()
    assert events == ["finalised", "capture begins"], events
    _done(env)

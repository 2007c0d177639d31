"""The tracked run on the device: the pose chain (naruto_amd.pose_chain), TrackerHIP.track_device, FusedBA(pose_init_on_device=True) and
CoSLAMNarutoHIP(track=True) over the scene of tests/test_gpu_slam.py (40 x 30 frames of cull_spec.room_mesh).

1. The pose chain's entry points against an fp64 numpy restatement.
2. Eleven tracked frames against a twin that drives the public pieces by hand: bit for bit, with the host's log map out of reach.
3. global_BA's write-back to est_c2w_data.
4. The tracker reads the weights as they are after a global_BA call.
5. A passive tracked run follows the camera.
6. A tracked run through the command line.

Run: timeout -k 10 600 python -m pytest tests/test_gpu_tracked_run.py -m gpu -q -s
"""
import copy
import math

import numpy as np
import pytest
import torch
import yaml

import cull_spec as CS
import helpers as H

pytestmark = pytest.mark.gpu

WW, HH, FOC = 40, 30, 30.0
ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
THETAS = (0.0, 1e-8, 1e-4, 0.5, 3.1, math.pi - 1e-6)
AXES = ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.3, -0.8, 0.5))
TRACKING = {"disable": False, "iter": 10, "sample": 256, "lr_rot": 1e-3, "lr_trans": 1e-3, "ignore_edge_W": 2, "ignore_edge_H": 2, "iter_point": 0,
            "wait_iters": 100, "const_speed": True, "best": True}


def _cfg(tracking=None, **mapping):
    c = H.office_cfg(12, perturb=1.0)
    cam = CS.camera(WW, HH, FOC)
    c["cam"].update(H=HH, W=WW, fx=FOC, fy=FOC, cx=cam["cx"], cy=cam["cy"], depth_trunc=100.0, near=0, far=5)
    c["mapping"]["bound"] = copy.deepcopy(ROOM)
    c["mapping"]["marching_cubes_bound"] = copy.deepcopy(ROOM)
    c["mapping"].update(sample=128, min_pixels_cur=16, keyframe_every=5, map_every=5, iters=10, first_iters=20, n_pixels=0.5, filter_depth=True)
    c["mapping"].update(mapping)
    c["tracking"] = dict(TRACKING, **(tracking or {}))
    c["mesh"].update(vis=500, voxel_eval=0.1, voxel_final=0.1)
    return c


def _rotation(axis, theta):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def _pose_set(n, seed=0):
    """n fp32 poses cycling through the angle set about the three axes, with translations of a few metres."""
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n):
        p = np.eye(4)
        p[:3, :3] = _rotation(AXES[(k // len(THETAS)) % len(AXES)], THETAS[k % len(THETAS)])
        p[:3, 3] = rs.uniform(-4.0, 4.0, 3)
        out.append(p)
    return torch.from_numpy(np.stack(out)).float()


def _close(got, ref, what):
    """Per entry 2^-23 max(1, |ref|): sums of products of O(1) terms in fp64, rounded to fp32 once."""
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    err = np.abs(got - ref)
    assert (err <= tol).all(), (what, float((err / tol).max()))


def _bits(a):
    return a.detach().cpu().contiguous().view(torch.int32)


def _look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4, dtype=np.float32)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64)).astype(np.float32)
    p[:3, 3] = pos
    return p


def _arc(n):
    out = []
    for k in range(n):
        a = 0.08 * k
        out.append(_look([1.2 + 0.5 * np.sin(a), 1.0 + 0.12 * k, 1.2 + 0.02 * k], CS.ROOM_CENTRE))
    return torch.from_numpy(np.stack(out))


def _sim(gpu, cam=None):
    from naruto_amd.simulator import MeshSimHIP
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    return MeshSimHIP((v, f), cam or CS.camera(WW, HH, FOC), erp_hw=(32, 64), face_w=32, far=100.0, device=gpu)


@pytest.fixture(scope="module")
def frames(gpu):
    poses = _arc(11)
    color, depth = _sim(gpu).simulate_batch(poses)
    assert bool((depth > 0).any())
    return poses, color, depth


# --------------------------------------------------------------------------------------------- 1. the pose chain
@pytest.mark.parametrize("P", [1, 2, 65])
def test_pose_log_and_scatter(gpu, P):
    from naruto_amd import pose_chain as PC
    from naruto_amd.tracking import matrices_to_pose6
    poses = _pose_set(P, seed=P)
    got = PC.pose_log(poses.to(gpu)).cpu()
    ref = matrices_to_pose6(poses).float()
    tol = 2.0 ** -22 * ref.double().abs() + 1e-12              # tests/test_tracked_run_host.py: a straddled rounding at most
    assert bool(((got.double() - ref.double()).abs() <= tol).all())
    out = torch.full((P + 2, 6), 7.0, device=gpu)              # into a given buffer: the rows past P keep their bits
    PC.pose_log(poses.to(gpu), out=out[:P])
    assert torch.equal(out[:P].cpu(), got) and bool((out[P:] == 7.0).all())
    # scatter: copies, exact; row 0 and every row the call does not own keep their bits
    every, n = 2, 131
    cur = n - 2
    base = torch.from_numpy(np.random.RandomState(3).standard_normal((n, 4, 4)).astype(np.float32))
    refined = torch.from_numpy(np.random.RandomState(4).standard_normal((P, 4, 4)).astype(np.float32))
    for optim_cur in (False, True):
        est = base.to(gpu)
        PC.pose_scatter(est, refined.to(gpu), P, every, cur, optim_cur)
        want = base.clone()
        for k in range(1, P - 1):
            want[k * every] = refined[k]
        if optim_cur and P >= 2:
            want[cur] = refined[P - 1]
        assert torch.equal(_bits(est), _bits(want)), (P, optim_cur)
        assert torch.equal(_bits(est[0]), _bits(base[0]))


@pytest.mark.parametrize("i", [1, 2])
@pytest.mark.parametrize("const_speed", [False, True])
def test_pose_predict(gpu, i, const_speed):
    from naruto_amd import pose_chain as PC
    from naruto_amd.tracking import matrices_to_pose6
    for start in range(0, len(THETAS) * len(AXES), 3):            # every angle of the set lands in rows i-2 and i-1 in turn
        base = _pose_set(len(THETAS) * len(AXES) + 4, seed=9)[start:start + 4].clone()
        est = base.to(gpu)
        pose6 = torch.full((6,), 5.0, device=gpu)
        PC.pose_predict(est, i, const_speed, pose6)
        a = base.double().numpy()
        if i == 1 or not const_speed:
            assert torch.equal(_bits(est[i]), _bits(base[i - 1]))
        else:
            _close(est[i], (a[i - 1] @ np.linalg.inv(a[i - 2])) @ a[i - 1], "predict")
        keep = [k for k in range(4) if k != i]
        assert torch.equal(_bits(est[keep]), _bits(base[keep]))
        # the tracker's initial pose is the log of the matrix AS STORED
        assert torch.equal(_bits(pose6), _bits(PC.pose_log(est[i:i + 1])[0]))
        ref6 = matrices_to_pose6(est[i:i + 1].cpu()).float()[0]
        assert bool(((pose6.cpu().double() - ref6.double()).abs() <= 2.0 ** -22 * ref6.double().abs() + 1e-12).all())


def test_pose_commit_and_resolve(gpu):
    from naruto_amd import pose_chain as PC
    every, n = 5, 12
    base = _pose_set(n, seed=5)
    rel0 = torch.from_numpy(np.random.RandomState(6).standard_normal((n, 4, 4)).astype(np.float32))
    tracked = _pose_set(20, seed=7)[13:15]
    for i, c2w in ((5, tracked[0]), (7, tracked[1])):              # a keyframe and a frame that is none
        est, rel = base.to(gpu), rel0.to(gpu)
        PC.pose_commit(est, rel, i, every, c2w.to(gpu))
        want = base.clone()
        want[i] = c2w
        assert torch.equal(_bits(est), _bits(want))
        keep = list(range(n))
        if i % every:
            keep.remove(i)
            _close(rel[i], c2w.double().numpy() @ np.linalg.inv(base[5].double().numpy()), "commit")
        assert torch.equal(_bits(rel[keep]), _bits(rel0[keep]))
    # resolve: keyframes are copies, the others rel @ est[kf]
    rel_ok = _pose_set(n, seed=8)
    for m in (1, 7, n):
        out = PC.pose_resolve(base.to(gpu), rel_ok.to(gpu), m, every)
        assert out.shape == (m, 4, 4)
        for k in range(m):
            if k % every == 0:
                assert torch.equal(_bits(out[k]), _bits(base[k]))
            else:
                _close(out[k], rel_ok[k].double().numpy() @ base[(k // every) * every].double().numpy(), "resolve")
    into = torch.full((n + 1, 4, 4), 3.0, device=gpu)
    PC.pose_resolve(base.to(gpu), rel_ok.to(gpu), n, every, out=into[:n])
    assert bool((into[n] == 3.0).all())


# --------------------------------------------------------------------------------------------- 2. the twin
def _params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


def test_eleven_tracked_frames_equal_the_hand_driven_twin(gpu, frames, monkeypatch):
    from naruto_amd import pose_chain as PC
    from naruto_amd import tracking, trainer
    from naruto_amd.ba_loop import FusedBA
    from naruto_amd.field import get_map_volumes
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    from naruto_amd.slam import CoSLAMNarutoHIP
    poses, color, depth = frames
    cfg = _cfg()
    slam = CoSLAMNarutoHIP(copy.deepcopy(cfg), voxel_size=0.1, active_ray=False, num_frames=11, seed=7, device=gpu, track=True)
    assert slam.tracker is not None and slam.ba.optimize_poses
    # ---- the twin: the same pieces, driven by hand
    cfg_t = copy.deepcopy(cfg)
    cfg_t["mapping"]["active_ray"] = False
    tr = trainer.MappingTrainer(cfg_t, torch.tensor(ROOM), gpu, uncert_voxel=0.1, fused_adam=True)
    tr.model.load_state_dict(slam.model.state_dict())
    tr.iter_state.copy_(slam.trainer.iter_state)
    store = KeyFrameStoreHIP(cfg_t, HH, WW, num_kf=3, num_rays_to_save=600, device=gpu, seed=7)
    ba = FusedBA(tr, store, None, max_poses=4, use_graph=False, optimize_poses=True)
    trk = tracking.TrackerHIP(tr.model, cfg_t, HH, WW, device=gpu, rng_seed=0)
    trk.rng.copy_(slam.tracker.rng)
    est = torch.zeros(11, 4, 4, device=gpu)
    rel = torch.zeros(11, 4, 4, device=gpu)
    refining = []

    def raising(*a, **k):
        raise AssertionError("the host's log map was called during a tracked step")
    for i in range(11):
        if i == 1:                     # from the first tracked frame on, the host's pose conversion is out of reach
            monkeypatch.setattr(tracking, "matrices_to_pose6", raising)
            monkeypatch.setattr(tracking, "matrix_to_axis_angle", raising)
        # the caller's pose is used for frame 0 only: later frames get one that is far off
        given = poses[0] if i == 0 else torch.eye(4)
        vols = slam.online_recon_step(i, color[i], depth[i], given)
        batch = {"frame_id": torch.tensor([i]), "rgb": color[i][None], "depth": depth[i][None], "direction": slam.rays_d[None]}
        current = torch.cat([batch["direction"], batch["rgb"], batch["depth"][..., None]], -1).reshape(-1, 7)
        want = None
        if i == 0:
            est[0] = poses[0].to(gpu)
            rel[0] = poses[0].to(gpu)

            def batches():
                for _ in range(20):
                    yield store.assemble_batch(0, current, est[0][None], 0, rng=tr.iter_state, n_cur=128, n_cur_pop=HH * WW)[:4]
            tr.first_frame_mapping(batches())
            store.add_keyframe(batch, filter_depth=True)
            want = get_map_volumes(tr.model.query_sdf, tr.model.bounding_box, 0.1)
        else:
            PC.pose_predict(est, i, True, trk.pose_init)
            PC.pose_commit(est, rel, i, 5, trk.track_device(slam.rays_d, color[i], depth[i]))
            if i % 5 == 0:
                p_all = torch.cat([est[0:i:5], est[i:i + 1]], 0)
                ba.global_BA(current, p_all, optimize_poses=True, pose_init_on_device=True)
                refining.append(ba._pose_on)
                if ba._pose_on:
                    PC.pose_scatter(est, ba.poses, p_all.shape[0], 5, i, True)
                want = get_map_volumes(tr.model.query_sdf, tr.model.bounding_box, 0.1)
                store.add_keyframe(batch, filter_depth=True)
        assert (vols is not None) == (want is not None)
        if want is not None:
            for name, got, w in zip(("uncert", "sdf"), vols, want):
                assert np.array_equal(got.cpu().numpy().view(np.int32), w.view(np.int32)), f"frame {i}: {name} volume"
        assert torch.equal(_bits(slam.est_c2w_data.tensor), _bits(est)), f"frame {i}: est"
        assert torch.equal(_bits(slam.est_c2w_data_rel.tensor), _bits(rel)), f"frame {i}: rel"
    assert refining == [False, True], "frame 5 sees one keyframe (no refinement, coslam.py:264), frame 10 two"
    assert torch.equal(slam.keyframeDatabase.rays.view(torch.int32), store.rays.view(torch.int32))
    assert slam.keyframeDatabase.frame_ids.tolist() == [0, 5, 10] == store.frame_ids.tolist()
    for (n, p), (_, q) in zip(slam.model.named_parameters(), tr.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"
    assert torch.equal(slam.model.uncert_grid.grad, tr.model.uncert_grid.grad)
    assert torch.equal(slam.trainer.iter_state, tr.iter_state) and torch.equal(slam.tracker.rng, trk.rng)
    assert len(slam.est_c2w_data) == 11 and sorted(slam.est_c2w_data_rel.keys()) == [0, 1, 2, 3, 4, 6, 7, 8, 9]
    assert bool(torch.isfinite(est).all()) and not torch.equal(est[10].cpu(), torch.eye(4)), "the poses are the tracker's, not the caller's"
    # resolved poses: the keyframes as they stand, the others relative to them
    res = slam.resolved_poses()
    assert torch.equal(_bits(res), _bits(PC.pose_resolve(est, rel, 11, 5)))
    assert torch.equal(_bits(res[[0, 5, 10]]), _bits(est[[0, 5, 10]]))
    slam.model.check_asserts(block=True)


# --------------------------------------------------------------------------------------------- 3. write-back
@pytest.mark.parametrize("optim_cur", [True, False])
def test_global_ba_writes_the_refined_poses_back(gpu, frames, optim_cur):
    from naruto_amd.slam import CoSLAMNarutoHIP
    poses, color, depth = frames
    slam = CoSLAMNarutoHIP(_cfg(optim_cur=optim_cur), voxel_size=0.1, active_ray=False, num_frames=11, seed=7, device=gpu, track=True)
    before = {}
    ba0 = slam.ba.global_BA

    def watching(*a, **k):
        before[len(before)] = slam.est_c2w_data.tensor.clone()
        return ba0(*a, **k)
    slam.ba.global_BA = watching
    for i in range(11):
        slam.online_recon_step(i, color[i], depth[i], poses[i])
    est, refined = slam.est_c2w_data.tensor, slam.ba.poses
    assert len(before) == 2 and slam.ba._pose_on and slam.ba._n_poses == 3
    assert torch.equal(_bits(est[5]), _bits(refined[1])) and not torch.equal(_bits(est[5]), _bits(before[1][5])), "keyframe 5 was refined and written back"
    assert torch.equal(_bits(est[0]), _bits(poses[0])), "the first pose keeps the caller's bits"
    if optim_cur:
        assert torch.equal(_bits(est[10]), _bits(refined[2])) and not torch.equal(_bits(est[10]), _bits(before[1][10]))
    else:
        assert torch.equal(_bits(est[10]), _bits(before[1][10])), "mapping.optim_cur off: the current frame keeps the tracked pose"
    others = [k for k in range(11) if k not in (5, 10)]
    assert torch.equal(_bits(est[others]), _bits(before[1][others]))


# --------------------------------------------------------------------------------------------- 4. fresh weights
def test_a_frame_after_global_ba_is_tracked_with_the_new_weights(gpu, frames):
    from naruto_amd import pose_chain as PC
    from naruto_amd.slam import CoSLAMNarutoHIP
    from naruto_amd.tracking import TrackerHIP
    poses, color, depth = frames
    cfg = _cfg()
    slam = CoSLAMNarutoHIP(copy.deepcopy(cfg), voxel_size=0.1, active_ray=False, num_frames=11, seed=7, device=gpu, track=True)
    for i in range(6):                                              # frame 5 maps: the weights move after the tracker was captured
        slam.online_recon_step(i, color[i], depth[i], poses[i])
    fresh = TrackerHIP(slam.model, copy.deepcopy(cfg), HH, WW, device=gpu, rng_seed=0)
    fresh.rng.copy_(slam.tracker.rng)
    est = slam.est_c2w_data.tensor.clone()
    PC.pose_predict(est, 6, True, fresh.pose_init)
    want = fresh.track_device(slam.rays_d, color[6], depth[6]).clone()
    slam.online_recon_step(6, color[6], depth[6], poses[6])
    assert torch.equal(_bits(slam.est_c2w_data.tensor[6]), _bits(want))
    assert not torch.equal(_bits(want), _bits(est[6])), "the tracker moved the predicted pose"
    with pytest.raises(KeyError, match="in order"):                 # a tracked frame starts from the one before it
        slam.online_recon_step(9, color[9], depth[9], poses[9])
    assert 9 not in slam.est_c2w_data


# --------------------------------------------------------------------------------------------- 5. it tracks
N_RUN = 21
# Mean translation error of the resolved poses over the 21 frames, measured on the first MI355X run of this test (8.958 mm, max 17.374 mm;
# staying at pose 0: 34.838 mm; ATE after alignment 0.475 cm rmse / 0.400 cm mean).  The bound is three times that: a 40 x 30 frame on a
# 2^12 table is noisy (the accuracy study's seeds are 5 % apart), and a change of the draw moves the figure without anything being wrong.
MEASURED_MEAN_ERR_M = 8.958e-3


def _ramp_arc(n):
    """A smooth arc around the sphere with a speed ramp: frame k moves 2 + 0.2 k mm along the arc (2 .. 6 mm, 4 mm on average) and the
    look-at direction turns with it, about 0.15 degrees per frame at the arc's radius of 1.6 m -- well inside what one tracking call
    can cover (iter x lr = 10 x 1e-3: 1 cm, 0.57 degrees), and the constant-speed prediction leaves only the ramp."""
    out, s = [], 0.0
    for k in range(n):
        s += (2.0 + 0.2 * k) * 1e-3
        a = s / 1.6
        out.append(_look([3.0 - 1.6 * np.cos(a), 2.5 - 1.6 * np.sin(a), 1.3 + 0.1 * s], CS.ROOM_CENTRE))
    return torch.from_numpy(np.stack(out))


def _passive_run(gpu):
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = _cfg(first_iters=100, sample=512, min_pixels_cur=128)
    slam = CoSLAMNarutoHIP(cfg, voxel_size=0.1, active_ray=False, num_frames=N_RUN, seed=3, device=gpu, track=True)
    sim = _sim(gpu, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")})
    traj = _ramp_arc(N_RUN)
    return slam, run_exploration(slam, sim, None, None, N_RUN, traj=traj), traj


def test_a_passive_run_follows_the_camera(gpu):
    slam, out, traj = _passive_run(gpu)
    est, gt = out["est_poses"], out["poses"]
    assert est.shape == (N_RUN, 4, 4) and torch.equal(gt, traj) and bool(torch.isfinite(est).all())
    err = (est[:, :3, 3].double() - gt[:, :3, 3].double()).norm(dim=1)
    still = (gt[:, :3, 3].double() - gt[0, :3, 3].double()).norm(dim=1)
    step = (gt[1:, :3, 3].double() - gt[:-1, :3, 3].double()).norm(dim=1)
    print("tracked run: mean translation error %.3f mm (max %.3f), staying at pose 0 %.3f mm; per-frame motion %.2f .. %.2f mm; ATE %s"
          % (float(err.mean()) * 1e3, float(err.max()) * 1e3, float(still.mean()) * 1e3, float(step.min()) * 1e3, float(step.max()) * 1e3, out["ate"]))
    assert float(err[0]) == 0.0, "frame 0 is the caller's pose"
    # not moving is what an untracked chain does: tracking has to beat it by a factor of two
    assert float(err.mean()) < 0.5 * float(still.mean())
    assert float(err.mean()) <= 3.0 * MEASURED_MEAN_ERR_M
    assert set(out["ate"]) == {"ate_rmse_cm", "ate_mean_cm"} and out["ate"]["ate_rmse_cm"] >= out["ate"]["ate_mean_cm"] > 0.0
    # a second run with the same seeds: the same poses and parameters, bit for bit
    want = _params(slam.model)
    slam2, out2, _ = _passive_run(gpu)
    assert torch.equal(_bits(out2["est_poses"]), _bits(est))
    for n, q in _params(slam2.model).items():
        assert torch.equal(q, want[n]), f"parameter {n}"


# --------------------------------------------------------------------------------------------- 6. the command line
def test_tracked_run_through_the_command_line(gpu, tmp_path):
    from naruto_amd import culling
    from naruto_amd.mesh import Mesh
    from naruto_amd.run import main
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    Mesh(np.asarray(v, np.float64), np.asarray(f, np.int64)).export(str(tmp_path / "room.ply"))
    cfg = _cfg(first_iters=100, sample=512, min_pixels_cur=128)
    cfg["cam"].update(cx=19.0, cy=14.0)
    with open(tmp_path / "cfg.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    out = main(["--config", str(tmp_path / "cfg.yaml"), "--mesh", str(tmp_path / "room.ply"), "--num_iter", "15", "--result_dir", str(tmp_path / "run"),
                "--start", "2.0", "4.0", "1.2", "--no_active_ray", "--seed", "5", "--track",
                "--planner", "gs_z_levels=[12]", "max_rot_deg=30", "rrt_max_iter=2000"])
    assert len(out["states"]) == 15 and out["est_poses"].shape == (15, 4, 4) and bool(torch.isfinite(out["est_poses"]).all())
    lines = dict(line.strip().split(",") for line in open(tmp_path / "run" / "results.txt"))
    assert set(lines) == {"traj_len(m)", "ate_rmse(cm)", "ate_mean(cm)"}
    assert float(lines["ate_rmse(cm)"]) == out["ate"]["ate_rmse_cm"] and float(lines["ate_mean(cm)"]) == out["ate"]["ate_mean_cm"]
    assert math.isfinite(float(lines["ate_rmse(cm)"])) and float(lines["ate_rmse(cm)"]) >= float(lines["ate_mean(cm)"]) >= 0.0
    ckpt = torch.load(out["ckpt_path"], weights_only=False)
    assert sorted(ckpt["pose"]) == list(range(15)), "the checkpoint's pose dict has every frame"
    assert sorted(ckpt["pose_rel"]) == [k for k in range(15) if k == 0 or k % 5]
    back = culling.poses_from_checkpoint(out["ckpt_path"])
    assert back.shape == (15, 4, 4) and torch.equal(back[0], out["poses"][0]), "raw poses: frame 0 is the caller's"

"""Depth odometry on the device (naruto_amd/odometry.py, csrc/naruto_odom.hip) against its numpy twin (tests/odometry_spec.py), and the
tracked run with motion_prior="depth_icp".  Frames come from MeshSimHIP over cull_spec.room_mesh(8, 16) unless a test needs a shape the
simulator is not needed for (the reduction's edges take drawn depth frames).

1. maps  2. rows and sums  3. iteration by iteration  4. early out  5. reproducibility  6. recovery  7. pose_predict_relative
8. the tracked run  9. the command line

Run: timeout -k 10 600 python -m pytest tests/test_gpu_odometry.py -m gpu -q -s
"""
import copy
import math

import numpy as np
import pytest
import torch
import yaml

import cull_spec as CS
import helpers as H
import odometry_spec as OS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CAM = CS.camera(160, 120, 120.0)


def _look(pos, at, yaw_deg=0.0):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64)) @ OS.rotation((0, 1, 0), math.radians(yaw_deg))
    p[:3, 3] = pos
    return p


def _sim(gpu, cam):
    from naruto_amd.simulator import MeshSimHIP
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    return MeshSimHIP((v, f), cam, erp_hw=(32, 64), face_w=32, far=100.0, device=gpu)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def case_frames(gpu):
    """Depth frames [7,120,160] on the device: the base pose and the six prototype motions from it."""
    base = _look(OS.CASE_POSITION, CS.ROOM_CENTRE)
    poses = np.stack([base] + [base @ rel for rel in OS.CASES]).astype(np.float32)
    _, depth = _sim(gpu, CAM).simulate_batch(torch.from_numpy(poses))
    assert float((depth[0] > 0).float().mean()) > 0.9
    return depth.contiguous()


def _odom(gpu, cam=CAM, **kw):
    from naruto_amd.odometry import DepthOdometryHIP
    return DepthOdometryHIP(cam, device=gpu, **kw)


# --------------------------------------------------------------------------------------------- 1. maps
@pytest.mark.parametrize("W,Hh", [(160, 120), (41, 31), (2, 2)])
def test_maps_equal_the_twin_in_every_bit(gpu, W, Hh):
    cam = CS.camera(W, Hh, 0.75 * W)
    base = _look(OS.CASE_POSITION, CS.ROOM_CENTRE).astype(np.float32)
    _, depth = _sim(gpu, cam).simulate_batch(torch.from_numpy(base[None]))
    d0 = depth[0].cpu().numpy().copy()
    assert (d0 > 0).all()
    od = _odom(gpu, cam)
    assert [s[:2] for s in od.level_shapes] == [(Hh, W), (Hh // 2, W // 2), (Hh // 4, W // 4)]
    frames = {"as rendered": d0}
    hole = d0.copy()
    hole[Hh // 4:Hh // 2 + 1, W // 4:W // 2 + 1] = 0.0                 # a missing block with odd edges
    frames["missing block"] = hole
    odd = d0.copy()
    odd[Hh // 2, W // 2] = np.nan
    odd[0, 0] = np.inf
    odd[Hh - 1, W - 1] = -1.0
    odd[0, W - 1] += 0.5                                                # a depth edge: the band and the jump rule
    frames["NaN, inf, negative, an edge"] = odd
    frames["whole frame missing"] = np.zeros_like(d0)
    for name, d in frames.items():
        got = od.frame_maps(torch.from_numpy(d).to(gpu)).cpu().numpy()
        twin = OS.frame_maps(d, cam)
        want = OS.pack_maps(twin)
        assert got.shape == want.shape == (od.maps_bytes // 4,)
        assert np.array_equal(_bits32(got), _bits32(want)), (name, int((_bits32(got) != _bits32(want)).sum()))
        for l in range(3):                                              # the views are the twin's arrays: depth, vertices, normals, validity
            dv, vv, nv = od.level_views(torch.from_numpy(got), l)
            assert np.array_equal(dv.numpy() > 0, twin[l][0] > 0) and np.array_equal((nv.numpy() != 0).any(-1), (twin[l][2] != 0).any(-1))
        if name == "whole frame missing":
            assert not (got != 0).any()
        elif min(W, Hh) > 2:
            assert (twin[0][2] != 0).any() and (twin[2][2] != 0).any(), "normals at every level"


# --------------------------------------------------------------------------------------------- 2. rows and sums
def _drawn_pair(Hh, W, seed):
    """Two smooth depth frames around 2 m that differ by a centimetre or so: many inliers under any small T."""
    rs = np.random.RandomState(seed)
    v, u = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    prev = 2.0 + 0.2 * np.sin(0.31 * u + 0.5) * np.cos(0.23 * v) + 0.003 * rs.standard_normal((Hh, W))
    cur = prev + 0.01 * np.cos(0.4 * u - 0.3 * v)
    return prev.astype(np.float32), cur.astype(np.float32)


def _accumulate_against_twin(gpu, Hh, W, T, prev, cur, tag):
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    od = _odom(gpu, cam, levels=1, iters=(1,))
    mp, mc = od.frame_maps(torch.from_numpy(prev).to(gpu)), od.frame_maps(torch.from_numpy(cur).to(gpu))
    tp, tc = OS.frame_maps(prev, cam, 1), OS.frame_maps(cur, cam, 1)
    rows = torch.full((Hh * W, 2), 7.0, dtype=torch.float64, device=gpu)
    state = od.init_state(T)
    sums = od.accumulate(0, mp, mc, state, rows=rows).cpu().numpy()
    idx, res, terms = OS.rows(T, OS.level_intrinsics(cam, 1)[0], tp[0], tc[0])
    r = rows.cpu().numpy()
    assert np.array_equal(r[:, 0].astype(np.int64), idx), (tag, "association")
    assert np.array_equal(_bits64(r[:, 1]), _bits64(res)), (tag, "residual")
    want = OS.reduce_sums(terms)
    assert np.array_equal(_bits64(sums), _bits64(want)), (tag, "sums", np.abs(sums - want).max())
    assert sums[28] == (idx >= 0).sum()
    return od, state, sums, idx


SMALL_T = OS.relative_motion((0.3, -0.8, 0.5), 1.0, OS.CASE_ALONG, 0.02)


# pixel counts 1; 7, 8, 9 (one thread's eight pixels); 255, 256, 257, 258 (one round of the workgroup's threads); 2047, 2048, 2049 (one
# workgroup's share); 19200 (a last workgroup that is part full); 540672 = 264 workgroups (the finishing launch's second round)
@pytest.mark.parametrize("Hh,W", [(1, 1), (1, 7), (2, 4), (3, 3), (15, 17), (16, 16), (1, 257), (6, 43), (23, 89), (32, 64), (3, 683), (120, 160), (704, 768)])
def test_rows_and_sums_equal_the_twin(gpu, Hh, W):
    prev, cur = _drawn_pair(Hh, W, seed=Hh * 1000 + W)
    # two pixels of yaw (the rows stay, so a frame of three rows keeps its inliers) and 4 mm along x and z
    T = OS.relative_motion((0, 1, 0), math.degrees(2.0 / max(W, Hh)), (0.6, 0.0, -0.74), 0.004)
    _, _, sums, idx = _accumulate_against_twin(gpu, Hh, W, T, prev, cur, (Hh, W))
    if Hh >= 3 and W >= 3:
        assert (idx >= 0).sum() > 0, "the case has inliers"
    if (Hh, W) == (120, 160):
        _, _, _, idx = _accumulate_against_twin(gpu, Hh, W, SMALL_T, prev, cur, (Hh, W, "general motion"))
        assert (idx >= 0).sum() > 0


def test_rows_on_the_rounding_edges_and_behind_the_camera(gpu):
    Hh, W, d0 = 24, 40, 2.0
    flat = np.full((Hh, W), d0, np.float32)
    f = float(max(W, Hh))
    # half a pixel sideways on a fronto-parallel plane: every projection lands on x.5, the left and right borders included
    for sx, sy in ((0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (-0.5, -0.5), (1.5, -2.5)):
        T = np.eye(4)
        T[0, 3], T[1, 3] = sx * d0 / f, -sy * d0 / f
        _, _, sums, idx = _accumulate_against_twin(gpu, Hh, W, T, flat, flat, ("edge", sx, sy))
        assert 0 < (idx >= 0).sum() < Hh * W
    # every point behind the camera: count 0, degenerate, T unchanged
    T = np.eye(4)
    T[:3, :3] = OS.rotation((0, 1, 0), math.pi)
    prev, cur = _drawn_pair(Hh, W, 5)
    od, state, sums, idx = _accumulate_against_twin(gpu, Hh, W, T, prev, cur, "behind")
    assert (idx == -1).all() and not sums.any()
    before = state.clone()
    od.step(0, state)
    got = od.read_state(state)
    assert got.status == ["degenerate"] and got.inliers == [0] and got.iterations == [0]
    assert torch.equal(state[:16].view(torch.int64), before[:16].view(torch.int64)) and float(state[16]) == 1.0


# --------------------------------------------------------------------------------------------- 3. iteration by iteration
def _step_bound(sums, T):
    """The host test's bounds carried through T <- exp(xi) T: |d xi| <= 256 eps k |xi| (two solvers), the exponential's own 64 eps (1 + |t|),
    each entry of the product a sum of four terms of size <= max|T| -- and as much again for the product's own rounding and fused
    multiply-adds the compiler may form in that scalar code."""
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    xi = np.linalg.solve(A, -sums[21:27])
    return 2.0 * 4.0 * max(1.0, np.abs(T).max()) * (256 * EPS * np.linalg.cond(A) * np.linalg.norm(xi) + 64 * EPS * (1.0 + np.linalg.norm(xi[3:])))


def test_iteration_by_iteration_against_the_twin(gpu, case_frames):
    od = _odom(gpu)
    mp, mc = od.frame_maps(case_frames[0]), od.frame_maps(case_frames[3])           # 10 cm / 10 degrees
    tp, tc = OS.frame_maps(case_frames[0].cpu().numpy(), CAM), OS.frame_maps(case_frames[3].cpu().numpy(), CAM)
    assert np.array_equal(_bits32(mp.cpu().numpy()), _bits32(OS.pack_maps(tp)))
    cams = OS.level_intrinsics(CAM, 3)
    state = od.init_state(None)
    compared = 0
    for k, cap in enumerate(od.iters):
        l = od.levels - 1 - k
        upd = 0
        for it in range(cap):
            s0 = state.cpu().numpy().copy()
            T = s0[:16].reshape(4, 4)
            if s0[16 + 8 * l] != 0.0:
                break
            sums = od.accumulate(l, mp, mc, state).cpu().numpy().copy()
            _, _, terms = OS.rows(T, cams[l], tp[l], tc[l])
            assert np.array_equal(_bits64(sums), _bits64(OS.reduce_sums(terms))), (l, it)
            od.step(l, state)
            s1 = state.cpu().numpy()
            Tn, done, status, upd, count, rmse = OS.step(sums, T, upd, cap)
            bound = _step_bound(sums, T)
            err = np.abs(s1[:16].reshape(4, 4) - Tn).max()
            assert err <= bound, (l, it, err, bound)
            w = s1[16 + 8 * l:24 + 8 * l]
            assert (w[0] != 0.0) == done and int(w[1]) == status and int(w[2]) == upd and w[3] == count and abs(w[4] - rmse) <= 4 * EPS * rmse
            compared += 1
    assert compared >= 8
    dm, dd = OS.motion_error(state.cpu().numpy()[:16].reshape(4, 4), OS.CASES[2])
    assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG


# --------------------------------------------------------------------------------------------- 4. early out
def test_launches_of_a_finished_level_write_nothing(gpu, case_frames):
    od = _odom(gpu)
    maps = od.frame_maps(case_frames[0])
    state = od.init_state(None)
    od.accumulate(2, maps, maps, state)                                # a frame against itself at T = identity: r = 0, xi = 0, converged
    od.step(2, state)
    got = od.read_state(state)
    assert got.status[2] == "converged" and got.iterations[2] == 1 and float(state[16 + 8 * 2]) == 1.0
    od.sums.fill_(3.25)
    od.workspace.fill_(-1.5)
    rows = torch.full((od.level_shapes[2][0] * od.level_shapes[2][1], 2), 9.0, dtype=torch.float64, device=gpu)
    before = state.clone()
    for _ in range(3):
        od.accumulate(2, maps, maps, state, rows=rows)
        od.step(2, state)
    assert torch.equal(state.view(torch.int64), before.view(torch.int64))
    assert bool((od.sums == 3.25).all()) and bool((od.workspace == -1.5).all()) and bool((rows == 9.0).all())
    od.accumulate(1, maps, maps, state)                                # another level is still live
    assert not bool((od.sums == 3.25).any())


# --------------------------------------------------------------------------------------------- 5. + 6. reproducibility, recovery
def test_estimates_repeat_bit_for_bit_and_recover_the_six_motions(gpu, case_frames):
    od = _odom(gpu)
    for k, rel in enumerate(OS.CASES):
        a = od.estimate(case_frames[0], case_frames[1 + k])
        state_a = od.state.clone()
        b = od.estimate(case_frames[0], case_frames[1 + k])
        assert torch.equal(state_a.view(torch.int64), od.state.view(torch.int64)), k
        assert a.transformation.dtype == np.float64 and a.transformation.shape == (4, 4) and np.array_equal(a.transformation, b.transformation)
        dm, dd = OS.motion_error(a.transformation, rel)
        print(f"case {k}: {dm * 1e3:.3f} mm, {dd:.4f} deg; {a.status}, iterations {a.iterations}, inliers {a.inliers}, rmse {a.rmse}")
        assert "degenerate" not in a.status and "running" not in a.status
        assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG, (k, dm, dd)
    # from a given initial transform: the true motion is a fixed point within the bound
    c = od.estimate(case_frames[0], case_frames[6], init=OS.CASES[5])
    assert OS.motion_error(c.transformation, OS.CASES[5])[0] <= OS.BOUND_M
    # two missing frames: degenerate at every level, T is the initial one
    zero = torch.zeros_like(case_frames[0])
    d = od.estimate(zero, zero, init=OS.CASES[0])
    assert d.status == ["degenerate"] * 3 and np.array_equal(d.transformation, OS.CASES[0])


# --------------------------------------------------------------------------------------------- 7. pose_predict_relative
def _close(got, ref, what):
    """Per entry 2^-23 max(1, |ref|): sums of products of O(1) terms in fp64, rounded to fp32 once (tests/test_gpu_tracked_run.py)."""
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    tol = 2.0 ** -23 * np.maximum(1.0, np.abs(ref))
    err = np.abs(got - ref)
    assert (err <= tol).all(), (what, float((err / tol).max()))


@pytest.mark.parametrize("i", [1, 3])
def test_pose_predict_relative(gpu, i):
    from naruto_amd import pose_chain as PC
    rs = np.random.RandomState(20 + i)
    for k, rel in enumerate([np.eye(4)] + OS.CASES):
        base = np.tile(np.eye(4), (5, 1, 1))
        for r in range(5):
            base[r, :3, :3] = OS.rotation(rs.standard_normal(3), rs.uniform(0.0, 3.1))
            base[r, :3, 3] = rs.uniform(-4.0, 4.0, 3)
        base = torch.from_numpy(base).float()
        est = base.to(gpu)
        state = torch.zeros(48, dtype=torch.float64, device=gpu)
        state[:16] = torch.from_numpy(rel.reshape(16)).to(gpu)
        pose6 = torch.full((6,), 5.0, device=gpu)
        PC.pose_predict_relative(est, i, state, pose6)
        _close(est[i], base[i - 1].double().numpy() @ rel, ("predict_relative", k))
        keep = [r for r in range(5) if r != i]
        assert torch.equal(est[keep].cpu().view(torch.int32), base[keep].view(torch.int32))
        assert torch.equal(pose6.cpu().view(torch.int32), PC.pose_log(est[i:i + 1])[0].cpu().view(torch.int32))
        if k == 0:
            assert torch.equal(est[i].cpu().view(torch.int32), base[i - 1].view(torch.int32)), "the identity moves the bits"
    with pytest.raises(Exception, match="first frame"):
        PC.pose_predict_relative(est, 0, state, pose6)


# --------------------------------------------------------------------------------------------- 8. the tracked run
N_RUN = 21
ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
TRACKING = {"disable": False, "iter": 10, "sample": 256, "lr_rot": 1e-3, "lr_trans": 1e-3, "ignore_edge_W": 2, "ignore_edge_H": 2, "iter_point": 0,
            "wait_iters": 100, "const_speed": True, "best": True}


def _cfg():
    c = H.office_cfg(12, perturb=1.0)
    c["cam"].update(H=CAM["H"], W=CAM["W"], fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"], depth_trunc=100.0, near=0, far=5)
    c["mapping"]["bound"] = copy.deepcopy(ROOM)
    c["mapping"]["marching_cubes_bound"] = copy.deepcopy(ROOM)
    c["mapping"].update(sample=512, min_pixels_cur=128, keyframe_every=5, map_every=5, iters=10, first_iters=100, n_pixels=0.05, filter_depth=True)
    c["tracking"] = dict(TRACKING)
    c["mesh"].update(vis=500, voxel_eval=0.1, voxel_final=0.1)
    return c


def _stop_and_go(n):
    """Position advances 3 cm along the arc (radius 1.6 m about the sphere) on even frames and stays on odd ones; the look-at direction is
    turned by +1.5 degrees on odd frames and back on even ones.  One tracking call reaches iter x lr = 1 cm and 0.57 degrees, so every
    change of velocity is three times that, and constant-speed extrapolation is wrong by as much at each frame."""
    out, s = [], 0.0
    for k in range(n):
        if k > 0 and k % 2 == 0:
            s += 0.03
        a = s / 1.6
        out.append(_look([3.0 - 1.6 * np.cos(a), 2.5 - 1.6 * np.sin(a), 1.3 + 0.1 * s], CS.ROOM_CENTRE, yaw_deg=1.5 * (k % 2)))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def _run(gpu, raising=False, **kw):
    from naruto_amd import tracking
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    slam = CoSLAMNarutoHIP(_cfg(), voxel_size=0.1, active_ray=False, num_frames=N_RUN, seed=3, device=gpu, track=True, **kw)
    sim = _sim(gpu, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")})
    traj = _stop_and_go(N_RUN)
    handed, saved = [], (tracking.matrices_to_pose6, tracking.matrix_to_axis_angle)

    def boom(*a, **k):
        raise AssertionError("the host's log map was called during a tracked step")

    def on_step(i, c2w, vols, state):
        if slam.odometry is not None and i > 0:
            handed.append(slam.odometry.state[:16].clone())
        if raising and i == 0:                 # from the first tracked frame on, the host's pose conversion is out of reach
            tracking.matrices_to_pose6, tracking.matrix_to_axis_angle = boom, boom
    try:
        out = run_exploration(slam, sim, None, None, N_RUN, traj=traj, on_step=on_step)
    finally:
        tracking.matrices_to_pose6, tracking.matrix_to_axis_angle = saved
    return slam, out, traj, handed


@pytest.fixture(scope="module")
def runs(gpu):
    return {"icp": _run(gpu, raising=True, motion_prior="depth_icp"), "const": _run(gpu, motion_prior="const_speed")}


def _mean_err(out):
    return float((out["est_poses"][:, :3, 3].double() - out["poses"][:, :3, 3].double()).norm(dim=1).mean())


def test_depth_icp_hands_the_tracker_the_true_motion(gpu, runs):
    slam, out, traj, handed = runs["icp"]
    assert slam.motion_prior == "depth_icp" and len(handed) == N_RUN - 1
    gt = traj.double().numpy()
    worst = [0.0, 0.0]
    for i in range(1, N_RUN):
        dm, dd = OS.motion_error(handed[i - 1].cpu().numpy().reshape(4, 4), np.linalg.inv(gt[i - 1]) @ gt[i])
        worst = [max(worst[0], dm), max(worst[1], dd)]
    print(f"depth_icp prior against the true relative motion, worst of {N_RUN - 1} frames: {worst[0] * 1e3:.3f} mm, {worst[1]:.4f} deg")
    assert worst[0] <= OS.BOUND_M and worst[1] <= OS.BOUND_DEG


def test_depth_icp_halves_the_tracked_error_of_const_speed(gpu, runs):
    """Measured on an MI355X (first run of this test): depth_icp 8.383 mm, const_speed 154.116 mm, not moving 143.465 mm; ATE 0.597 cm rmse
    against 8.423 cm.  The prior itself: at most 0.783 mm / 0.0217 degrees from the true relative motion over the 20 frames."""
    _, icp, traj, _ = runs["icp"]
    _, const, _, _ = runs["const"]
    gt = traj[:, :3, 3].double()
    still = float((gt - gt[0]).norm(dim=1).mean())
    e_icp, e_const = _mean_err(icp), _mean_err(const)
    print(f"mean translation error after tracking: depth_icp {e_icp * 1e3:.3f} mm, const_speed {e_const * 1e3:.3f} mm, not moving {still * 1e3:.3f} mm; "
          f"ATE depth_icp {icp['ate']}, const_speed {const['ate']}")
    assert bool(torch.isfinite(icp["est_poses"]).all()) and torch.equal(icp["poses"], traj)
    assert e_icp < 0.5 * e_const
    assert e_icp < 0.5 * still


def test_the_tracked_runs_repeat_and_the_default_keeps_its_bits(gpu, runs):
    slam, icp, _, handed = runs["icp"]
    slam2, again, _, handed2 = _run(gpu, motion_prior="depth_icp")
    assert torch.equal(again["est_poses"].view(torch.int32), icp["est_poses"].view(torch.int32))
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(handed, handed2))
    for (n, p), (_, q) in zip(slam.model.named_parameters(), slam2.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"
    slam_c, const, _, _ = runs["const"]
    slam_d, default, _, _ = _run(gpu)
    assert slam_d.motion_prior == "const_speed" and slam_d.odometry is None and slam_c.odometry is None
    assert torch.equal(slam_d.est_c2w_data.tensor.view(torch.int32), slam_c.est_c2w_data.tensor.view(torch.int32))
    assert torch.equal(default["est_poses"].view(torch.int32), const["est_poses"].view(torch.int32))
    assert not torch.equal(default["est_poses"], icp["est_poses"])


def test_motion_prior_is_refused_without_tracking(gpu):
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = _cfg()
    cfg["tracking"]["disable"] = True
    for prior in ("depth_icp", "const_speed"):
        with pytest.raises(ValueError, match="track=True"):
            CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=4, device=gpu, motion_prior=prior)
    with pytest.raises(ValueError, match="motion_prior"):
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=4, device=gpu, track=True, motion_prior="optical_flow")


# --------------------------------------------------------------------------------------------- 9. the command line
def test_depth_icp_through_the_command_line(gpu, tmp_path):
    from naruto_amd.mesh import Mesh
    from naruto_amd.run import main
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    Mesh(np.asarray(v, np.float64), np.asarray(f, np.int64)).export(str(tmp_path / "room.ply"))
    cfg = _cfg()
    cfg["cam"].update(H=30, W=40, fx=30.0, fy=30.0, cx=19.0, cy=14.0)
    cfg["mapping"].update(n_pixels=0.5)
    with open(tmp_path / "cfg.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    common = ["--config", str(tmp_path / "cfg.yaml"), "--mesh", str(tmp_path / "room.ply"), "--num_iter", "12", "--start", "2.0", "4.0", "1.2",
              "--no_active_ray", "--seed", "5", "--track", "--planner", "gs_z_levels=[12]", "max_rot_deg=30", "rrt_max_iter=2000"]
    keys = {}
    for name, extra in (("icp", ["--motion_prior", "depth_icp"]), ("track", [])):
        out = main(common[:6] + ["--result_dir", str(tmp_path / name)] + common[6:-4] + extra + common[-4:])
        assert out["est_poses"].shape == (12, 4, 4) and bool(torch.isfinite(out["est_poses"]).all())
        keys[name] = set(dict(line.strip().split(",") for line in open(tmp_path / name / "results.txt")))
    assert keys["icp"] == keys["track"] == {"traj_len(m)", "ate_rmse(cm)", "ate_mean(cm)"}

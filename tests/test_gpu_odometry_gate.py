"""The odometry prior's scored starts and verdict on the device (naruto_amd/odometry.py, csrc/naruto_odom.hip: k_odom_score,
k_odom_candidates, k_odom_choose, k_odom_verdict) against the numpy twin (tests/odometry_gate_spec.py), and the tracked run with
prior_gate=True.

1. sums  2. cross-checks against the accumulate kernels  3. the one-thread kernels  4. the study's pairs  5. reproducibility
6. the tracked run  7. the command line

Run: timeout -k 10 600 python -m pytest tests/test_gpu_odometry_gate.py -m gpu -q -s
"""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

import cull_spec as CS
import helpers as H
import odometry_gate_spec as GS
import odometry_rgbd_spec as RS
import odometry_spec as OS

pytestmark = pytest.mark.gpu

Y = (0.0, 1.0, 0.0)
SMALL_T = OS.relative_motion((0.3, -0.8, 0.5), 1.0, OS.CASE_ALONG, 0.02)
BEHIND = OS.relative_motion(Y, 180.0, OS.CASE_ALONG, 0.0)
NAN_T = np.full((4, 4), np.nan)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64))
    p[:3, 3] = pos
    return p


def _sim(gpu, cam):
    from naruto_amd.simulator import MeshSimHIP
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    return MeshSimHIP((v, f), cam, erp_hw=(32, 64), face_w=32, far=100.0, device=gpu)


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


# --------------------------------------------------------------------------------------------- 1. sums
# pixel counts 1, 4, 255, 256, 257 (one round of the workgroup's threads), 2048, 2049 (one workgroup's share), 19200 (ten workgroups)
@pytest.mark.parametrize("Hh,W", [(1, 1), (2, 2), (15, 17), (16, 16), (1, 257), (32, 64), (3, 683), (120, 160)])
def test_sums_equal_the_twin_in_every_bit(gpu, Hh, W):
    from naruto_amd.odometry import DepthOdometryHIP, RGBDOdometryHIP
    dp, dc, cp, cc = RS.drawn_pair(Hh, W, seed=Hh * 1000 + W)
    if Hh >= 3 and W >= 8:
        dc[Hh // 2, W // 3:W // 3 + 3] = 0.0                               # a hole
        dp[Hh // 3, W // 2] = np.nan                                       # a NaN depth
        dc[Hh - 1, W - 2] = np.nan
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    T = OS.relative_motion(Y, math.degrees(2.0 / max(W, Hh)), (0.6, 0.0, -0.74), 0.004)   # two pixels of yaw, 4 mm
    sets = {1: [T], 2: [NAN_T, T], 4: [T, BEHIND, T, NAN_T]}
    good = {1: 0, 2: 1, 4: 0}
    trunc = 0.004                                                           # below many of the residuals (the frames differ by a centimetre)
    ods = {"depth": (DepthOdometryHIP(cam, levels=1, iters=(1,), device=gpu), 0.0),
           "rgbd, weight 0": (RGBDOdometryHIP(cam, levels=1, iters=(1,), photo_weight=0.0, device=gpu), 0.0),
           "rgbd": (RGBDOdometryHIP(cam, levels=1, iters=(1,), device=gpu), RS.PHOTO_WEIGHT)}
    tp, tc = RS.frame_maps(dp, cp, cam, 1), RS.frame_maps(dc, cc, cam, 1)
    ddp, ddc, dcp, dcc = _dev(gpu, dp, dc, cp, cc)
    for name, (od, w) in ods.items():
        rgbd = name != "depth"
        mp, mc = (od.frame_maps(ddp, dcp), od.frame_maps(ddc, dcc)) if rgbd else (od.frame_maps(ddp), od.frame_maps(ddc))
        twin_p, twin_c = (tp, tc) if rgbd else (tp[0], tc[0])
        alone = None
        for K, cands in sets.items():
            got = od.score(mp, mc, np.stack(cands), level=0, trunc=trunc).cpu().numpy()
            want = GS.score(np.stack(cands), cam, 0, twin_p, twin_c, trunc, levels=1, photo_weight=w)
            assert got.shape == want.shape == (1 + 4 * K,)
            assert np.array_equal(_bits64(got), _bits64(want)), (name, K, got, want)
            g = got[1 + 4 * good[K]:5 + 4 * good[K]]
            if alone is None:
                alone = (got[0], g.copy())
            assert got[0] == alone[0] and np.array_equal(_bits64(g), _bits64(alone[1])), (name, K, "the good candidate's sums beside the others")
            for k, c in enumerate(cands):
                if c is NAN_T or c is BEHIND:
                    assert not got[1 + 4 * k:5 + 4 * k].any(), (name, K, k)
            if K == 4:
                assert np.array_equal(_bits64(got[1:5]), _bits64(got[9:13])), "two identical candidates"
        if Hh >= 15 and W >= 16:
            assert alone[1][0] > 0 and alone[1][1] < trunc * trunc * alone[1][0], (name, "rows, some below the truncation")
            assert (alone[1][2] > 0) == (name == "rgbd"), name


# --------------------------------------------------------------------------------------------- 2. cross-checks
@pytest.mark.parametrize("Hh,W", [(23, 89), (120, 160)])
def test_score_equals_the_accumulate_kernels_in_every_bit(gpu, Hh, W):
    from naruto_amd.odometry import DepthOdometryHIP, RGBDOdometryHIP
    dp, dc, cp, cc = RS.drawn_pair(Hh, W, seed=7)
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    ddp, ddc, dcp, dcc = _dev(gpu, dp, dc, cp, cc)
    od = DepthOdometryHIP(cam, levels=2, iters=(1, 1), device=gpu)
    mp, mc = od.frame_maps(ddp), od.frame_maps(ddc)
    rod = RGBDOdometryHIP(cam, levels=2, iters=(1, 1), device=gpu)
    rmp, rmc = rod.frame_maps(ddp, dcp), rod.frame_maps(ddc, dcc)
    for level in (0, 1):
        state = od.init_state(SMALL_T)
        acc = od.accumulate(level, mp, mc, state).cpu().numpy()
        got = od.score(mp, mc, state[:16], level=level, trunc=float(od.desc.max_dist)).cpu().numpy()
        assert acc[28] > 0 and np.array_equal(_bits64(got[1:3]), _bits64(acc[[28, 27]])), (level, got, acc[27:])
        state = rod.init_state(SMALL_T)
        acc = rod.accumulate(level, rmp, rmc, state).cpu().numpy()
        got = rod.score(rmp, rmc, state[:16], level=level, trunc=float(rod.desc.max_dist)).cpu().numpy()
        assert acc[29] > 0 and acc[30] > 0 and np.array_equal(_bits64(got[[1, 3, 4]]), _bits64(acc[[29, 30, 31]])), (level, got, acc[29:])


# --------------------------------------------------------------------------------------------- 3. the one-thread kernels
def test_candidates_are_state_inits_constant_speed_transform(gpu):
    from naruto_amd.odometry import DepthOdometryHIP
    od = DepthOdometryHIP(CS.camera(16, 12, 12.0), device=gpu)
    rs = np.random.RandomState(4)
    est = np.tile(np.eye(4), (5, 1, 1))
    for r in range(5):
        est[r, :3, :3] = OS.rotation(rs.standard_normal(3), rs.uniform(0.0, 3.1))
        est[r, :3, 3] = rs.uniform(-4.0, 4.0, 3)
    est = torch.from_numpy(est).float().to(gpu)
    eye = np.eye(4).reshape(16)
    for i in (0, 1, 2, 4):
        c = od.candidates(est, i).cpu().numpy()
        want = od.init_state(est=est, i=i, const_speed=True).cpu().numpy()[:16]
        assert np.array_equal(c[0], eye) and np.array_equal(_bits64(c[1]), _bits64(want)), i
        assert np.array_equal(c[1], eye) == (i < 2)
    with pytest.raises(Exception, match="frame 5 of 5"):
        od.candidates(est, 5)


@pytest.fixture(scope="module")
def pairs(gpu):
    """The study's frames on the device: {scene: (camera, depth frames [4,H,W]: the base pose, yaw -18, 5 degrees / 3 cm, yaw 90)}."""
    rels = [np.eye(4), OS.relative_motion(Y, -18.0, OS.CASE_ALONG, 0.0), OS.relative_motion((0.3, -0.8, 0.5), 5.0, OS.CASE_ALONG, 0.03),
            OS.relative_motion(Y, 90.0, OS.CASE_ALONG, 0.0)]
    out = {}
    for scene, (cam, pos, at) in {"A": (CS.camera(160, 120, 120.0), OS.CASE_POSITION, CS.ROOM_CENTRE),
                                  "B": (CS.camera(80, 60, 60.0), (0.5, 1.0, 1.5), (3.0, 1.0, 0.2))}.items():
        poses = np.stack([_look(pos, at) @ r for r in rels]).astype(np.float32)
        _, depth = _sim(gpu, cam).simulate_batch(torch.from_numpy(poses))
        out[scene] = (cam, depth.contiguous(), rels)
    return out


def _by_hand(od, mp, mc, cands, g):
    """The gated sequence launch by launch, reading back between the launches: what each one-thread kernel saw and what it wrote."""
    coarse = od.score(mp, mc, cands, level=od.levels - 1, trunc=g.score_trunc).cpu().numpy().copy()
    state = torch.full((48,), 7.0, dtype=torch.float64, device=mp.device)
    record = torch.full((16,), 7.0, dtype=torch.float64, device=mp.device)
    od.choose(len(cands), g.score_trunc, state, record)
    chosen_state, head = state.cpu().numpy().copy(), record.cpu().numpy().copy()
    od.run_levels(mp, mc, state)
    before = state.cpu().numpy().copy()
    fine = od.score(mp, mc, state[:16], level=0, trunc=float(od.desc.max_dist)).cpu().numpy().copy()
    od.verdict(g, state, record)
    return SimpleNamespace(coarse=coarse, chosen_state=chosen_state, head=head, before=before, fine=fine, after=state.cpu().numpy(),
                               record=record.cpu().numpy())


def test_choose_and_verdict_records_equal_the_twin(gpu, pairs):
    from naruto_amd.odometry import DepthOdometryHIP, OdometryGate
    cam, depth, rels = pairs["B"]
    od = DepthOdometryHIP(cam, device=gpu)
    maps = [od.frame_maps(d) for d in depth]
    g, tg = OdometryGate(), GS.gate()
    assert g.abi().min_trace == tg.min_trace
    cases = {"recovered": (1, [np.eye(4), rels[1]]), "tie": (2, [rels[2], rels[2]]), "NaN beside a good one": (2, [NAN_T, np.eye(4)]),
             "no overlap": (3, [np.eye(4), rels[1]]), "NaN alone": (2, [NAN_T]), "four": (2, [rels[1], BEHIND, np.eye(4), rels[2]])}
    for name, (k, cands) in cases.items():
        cands = np.stack(cands)
        r = _by_hand(od, maps[0], maps[k], cands, g)
        chosen, T0, head = GS.choose(r.coarse, cands, tg.score_trunc)
        assert np.array_equal(_bits64(r.head), _bits64(head)), (name, r.head, head)
        want_state = od.init_state(cands[chosen]).cpu().numpy() if np.isfinite(cands[chosen]).all() else None
        if want_state is not None:
            assert np.array_equal(_bits64(r.chosen_state), _bits64(want_state)), (name, "the state after choose is state_init's")
        else:
            assert np.isnan(r.chosen_state[:16]).all() and not r.chosen_state[16:].any()
        T, record = GS.verdict(tg, r.fine, r.before[:16], r.before[17], cands, head)
        assert np.array_equal(_bits64(r.record), _bits64(record)), (name, r.record, record)
        assert np.isfinite(r.record).all(), name
        if r.record[0] == 1.0:
            assert np.array_equal(_bits64(r.after), _bits64(r.before)), (name, "PASS leaves the state")
        else:
            got, want = r.after[:16], cands[chosen].reshape(16)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]), (name, "FAIL: the chosen start")
            assert np.array_equal(_bits64(r.after[16:]), _bits64(r.before[16:]))
        print(f"{name}: chosen {chosen}, costs {head[2:6]}, verdict {r.record[0]}, overlap {r.record[7] / max(r.record[6], 1):.3f}, rmse {r.record[8] * 1e3:.3f} mm")
        if name == "recovered":
            assert chosen == 1 and r.record[0] == 1.0
        if name == "tie":
            assert chosen == 0 and head[2] == head[3]
        if name == "NaN beside a good one":
            assert chosen == 1 and r.record[0] == 1.0
        if name in ("no overlap", "NaN alone"):
            assert r.record[0] == 0.0
    # an all-missing current frame: every cost is 1, the lowest index, FAIL
    zero = od.frame_maps(torch.zeros_like(depth[0]))
    for mp, mc in ((maps[0], zero), (zero, maps[0])):
        r = _by_hand(od, mp, mc, np.stack([rels[2], np.eye(4)]), g)
        assert r.head[1] == 0.0 and r.record[0] == 0.0 and np.isfinite(r.record).all() and np.array_equal(r.after[:16], rels[2].reshape(16))


def test_rgbd_choose_adds_the_photometric_cost_and_the_record_keeps_its_figures(gpu):
    from naruto_amd.odometry import OdometryGate, RGBDOdometryHIP
    Hh, W = 60, 80
    dp, dc, cp, cc = RS.drawn_pair(Hh, W, seed=11)
    cam = CS.camera(W, Hh, float(W))
    od = RGBDOdometryHIP(cam, device=gpu)
    ddp, ddc, dcp, dcc = _dev(gpu, dp, dc, cp, cc)
    mp, mc = od.frame_maps(ddp, dcp), od.frame_maps(ddc, dcc)
    tp, tc = RS.frame_maps(dp, cp, cam), RS.frame_maps(dc, cc, cam)
    g, tg = OdometryGate(), GS.gate()
    for cands in (np.stack([np.eye(4), SMALL_T]), np.stack([BEHIND, NAN_T, SMALL_T]), np.stack([SMALL_T, SMALL_T])):
        r = _by_hand(od, mp, mc, cands, g)
        want = GS.score(cands, cam, 2, tp, tc, tg.score_trunc, photo_weight=RS.PHOTO_WEIGHT)
        assert np.array_equal(_bits64(r.coarse), _bits64(want))
        chosen, T0, head = GS.choose(r.coarse, cands, tg.score_trunc, True, float(od.photo.max_diff))
        assert np.array_equal(_bits64(r.head), _bits64(head)), (r.head, head)
        geo_only = GS.choose(r.coarse, cands, tg.score_trunc)[2]
        assert (head[2:2 + len(cands)] >= geo_only[2:2 + len(cands)]).all() and (head[2:2 + len(cands)] <= 2.0).all()
        T, record = GS.verdict(tg, r.fine, r.before[:16], r.before[17], cands, head)
        assert np.array_equal(_bits64(r.record), _bits64(record)), (r.record, record)
        assert r.record[12] > 0 and r.record[13] > 0 and np.isfinite(r.record).all()
        assert np.array_equal(_bits64(r.fine), _bits64(GS.score(r.before[:16].reshape(1, 4, 4), cam, 0, tp, tc, float(np.float32(0.25)), photo_weight=RS.PHOTO_WEIGHT)))


# --------------------------------------------------------------------------------------------- 4. the study's pairs
def test_the_pairs_no_fixed_start_recovers(gpu, pairs):
    from naruto_amd.odometry import DepthOdometryHIP
    yaw18 = OS.relative_motion(Y, 18.0, OS.CASE_ALONG, 0.0)
    for scene, losing, last in (("A", yaw18, yaw18), ("B", np.eye(4), pairs["B"][2][1])):
        cam, depth, rels = pairs[scene]
        od = DepthOdometryHIP(cam, device=gpu)
        mp, mc = od.frame_maps(depth[0]), od.frame_maps(depth[1])
        lost = od.read_state(od.estimate_device(mp, mc, init=losing)).transformation
        dm, dd = OS.motion_error(lost, rels[1])
        print(f"scene {scene}, yaw -18 from the losing start: {dm * 1e3:.3f} mm {dd:.4f} deg")
        assert dm > OS.BOUND_M or dd > OS.BOUND_DEG
        state = od.estimate_gated_device(mp, mc, candidates=np.stack([np.eye(4), last]))
        rec = od.record.cpu().numpy()
        dm, dd = OS.motion_error(state.cpu().numpy()[:16].reshape(4, 4), rels[1])
        print(f"  gated: start {int(rec[1])}, costs {rec[2:4]}, {dm * 1e3:.3f} mm {dd:.4f} deg, verdict {rec[0]}")
        assert rec[0] == 1.0 and dm <= OS.BOUND_M and dd <= OS.BOUND_DEG
        # no overlap: FAIL, and the chosen start is what the state holds
        cands = np.stack([np.eye(4), last])
        out = od.estimate_gated(depth[0], depth[3], candidates=cands)
        assert not out.passed and np.array_equal(out.T, cands[out.chosen]) and np.isfinite(out.record).all() and len(out.costs) == 2


# --------------------------------------------------------------------------------------------- 5. reproducibility
def test_gated_estimates_repeat_bit_for_bit(gpu, pairs):
    from naruto_amd.odometry import DepthOdometryHIP, RGBDOdometryHIP
    cam, depth, rels = pairs["B"]
    color = torch.stack([torch.from_numpy(RS.drawn_pair(cam["H"], cam["W"], 1)[2 + k]) for k in (0, 1)]).to(gpu)
    cands = np.stack([np.eye(4), rels[1]])
    for od, frames in ((DepthOdometryHIP(cam, device=gpu), (depth[0], depth[1])),
                       (RGBDOdometryHIP(cam, device=gpu), ((depth[0], color[0]), (depth[1], color[1])))):
        a = od.estimate_gated(frames[0], frames[1], candidates=cands)
        state = od.state.clone()
        b = od.estimate_gated(frames[0], frames[1], candidates=cands)
        assert torch.equal(state.view(torch.int64), od.state.view(torch.int64)) and np.array_equal(_bits64(a.record), _bits64(b.record))
        assert np.isfinite(a.record).all() and a.record[6] > 0


# --------------------------------------------------------------------------------------------- 6. the tracked run
N_RUN, JUMP = 8, 4
ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
TRACKING = {"disable": False, "iter": 10, "sample": 256, "lr_rot": 1e-3, "lr_trans": 1e-3, "ignore_edge_W": 2, "ignore_edge_H": 2, "iter_point": 0,
            "wait_iters": 100, "const_speed": True, "best": True}


def _cfg():
    c = H.office_cfg(12, perturb=1.0)
    c["cam"].update(H=30, W=40, fx=30.0, fy=30.0, cx=19.0, cy=14.0, depth_trunc=100.0, near=0, far=5)
    c["mapping"]["bound"] = copy.deepcopy(ROOM)
    c["mapping"]["marching_cubes_bound"] = copy.deepcopy(ROOM)
    c["mapping"].update(sample=512, min_pixels_cur=128, keyframe_every=5, map_every=5, iters=10, first_iters=100, n_pixels=0.5, filter_depth=True)
    c["tracking"] = dict(TRACKING)
    c["mesh"].update(vis=500, voxel_eval=0.1, voxel_final=0.1)
    return c


def _trajectory():
    """Half a degree of yaw and 2 cm per frame, a jump of -60 degrees at frame JUMP, no motion at the frame after it, then on as before
    (on the twin at 40 x 30: the jump is the only FAIL, the other frames have overlap >= 0.64 and rmse <= 1.8 mm)."""
    step, jump = OS.relative_motion(Y, 0.5, OS.CASE_ALONG, 0.02), OS.relative_motion(Y, -60.0, OS.CASE_ALONG, 0.0)
    poses = [_look(OS.CASE_POSITION, CS.ROOM_CENTRE)]
    for i in range(1, N_RUN):
        poses.append(poses[-1] @ (jump if i == JUMP else np.eye(4) if i == JUMP + 1 else step))
    return torch.from_numpy(np.stack(poses).astype(np.float32))


def test_a_tracked_run_flags_the_jump_alone_and_never_waits_for_the_host(gpu):
    from naruto_amd import tracking
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    with pytest.raises(ValueError, match="prior_gate"):
        CoSLAMNarutoHIP(_cfg(), num_frames=4, device=gpu, track=True, prior_gate=True)
    with pytest.raises(ValueError, match="prior_gate"):
        CoSLAMNarutoHIP(_cfg(), num_frames=4, device=gpu, track=True, motion_prior="const_speed", prior_gate=True)
    slam = CoSLAMNarutoHIP(_cfg(), voxel_size=0.1, active_ray=False, num_frames=N_RUN, seed=3, device=gpu, track=True, motion_prior="depth_icp", prior_gate=True)
    assert slam.prior_log.shape == (N_RUN, 16) and slam.prior_log.dtype == torch.float64
    sim = _sim(gpu, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")})
    traj = _trajectory()
    saved = (tracking.matrices_to_pose6, tracking.matrix_to_axis_angle)

    def boom(*a, **k):
        raise AssertionError("the host's log map was called during a tracked step")

    def on_step(i, c2w, vols, state):
        if i == 0:                                  # from the first tracked frame on, the host's pose conversion is out of reach
            tracking.matrices_to_pose6, tracking.matrix_to_axis_angle = boom, boom
    try:
        out = run_exploration(slam, sim, None, None, N_RUN, traj=traj, on_step=on_step)
    finally:
        tracking.matrices_to_pose6, tracking.matrix_to_axis_angle = saved
    log = out["prior_log"].numpy()
    for i in range(1, N_RUN):
        print(f"frame {i}: verdict {log[i, 0]}, start {int(log[i, 1])}, costs {log[i, 2:4]}, overlap {log[i, 7] / max(log[i, 6], 1):.3f}, rmse {log[i, 8] * 1e3:.3f} mm, "
              f"|t| {log[i, 9]:.4f}, trace {log[i, 10]:.4f}, status {int(log[i, 11])}")
    assert log.shape == (N_RUN, 16) and not log[0].any() and np.isfinite(log).all()
    assert [i for i in range(1, N_RUN) if log[i, 0] == 0.0] == [JUMP]
    assert (log[1:, 6] > 0).all() and bool(torch.isfinite(out["est_poses"]).all())
    assert torch.equal(slam.prior_log.cpu(), out["prior_log"])


# --------------------------------------------------------------------------------------------- 7. the command line
def test_prior_gate_through_the_command_line(gpu, tmp_path):
    from naruto_amd.mesh import Mesh
    from naruto_amd.run import main
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    Mesh(np.asarray(v, np.float64), np.asarray(f, np.int64)).export(str(tmp_path / "room.ply"))
    with open(tmp_path / "cfg.yaml", "w") as fh:
        yaml.safe_dump(_cfg(), fh)
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--mesh", str(tmp_path / "room.ply"), "--num_iter", "12", "--result_dir", str(tmp_path / "out"),
            "--start", "2.0", "4.0", "1.2", "--no_active_ray", "--seed", "5", "--track", "--motion_prior", "rgbd_icp", "--prior_gate",
            "--planner", "gs_z_levels=[12]", "max_rot_deg=30", "rrt_max_iter=2000"]
    out = main(argv)
    log = out["prior_log"].numpy()
    assert log.shape == (12, 16) and np.isfinite(log).all() and not log[0].any() and (log[1:, 6] > 0).all()
    rows = dict(line.strip().split(",") for line in open(tmp_path / "out" / "results.txt"))
    assert set(rows) == {"traj_len(m)", "ate_rmse(cm)", "ate_mean(cm)", "prior_failed_frames"}
    assert int(rows["prior_failed_frames"]) == int((log[1:, 0] == 0.0).sum())
    with pytest.raises(ValueError, match="prior_gate"):
        main(argv[:argv.index("--motion_prior")] + ["--prior_gate"] + argv[argv.index("--planner"):])

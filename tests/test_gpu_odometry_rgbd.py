"""RGB-D odometry on the device (naruto_amd.odometry.RGBDOdometryHIP, csrc/naruto_odom.hip) against its numpy twin
(tests/odometry_rgbd_spec.py), and the tracked run with motion_prior="rgbd_icp".  Frames come from MeshSimHIP over the coloured room
(cull_spec.room_mesh(8, 16) subdivided to 0.5 m: 1 652 vertices) and the coloured wall of the twin, unless a test needs a shape the
simulator is not needed for (the reduction's edges take drawn frames).

1. maps  2. rows and sums  3. edges  4. photo_weight = 0  5. iteration by iteration  6. early out  7. reproducibility and recovery
8. the tracked run along a wall  9. the command line

Run: timeout -k 10 600 python -m pytest tests/test_gpu_odometry_rgbd.py -m gpu -q -s
"""
import copy
import math

import numpy as np
import pytest
import torch
import yaml

import cull_spec as CS
import helpers as H
import odometry_rgbd_spec as RS
import odometry_spec as OS
import subdivide_spec as SUB

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CAM = CS.camera(160, 120, 120.0)


def _look(pos, at, yaw_deg=0.0):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64)) @ OS.rotation((0, 1, 0), math.radians(yaw_deg))
    p[:3, 3] = pos
    return p


def _room():
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    v, f, _, _, _ = SUB.subdivide_to_size(np.asarray(v, np.float32), f, 0.5)
    assert len(v) == 1652
    return v, f, RS.smooth_colours(v)


def _sim(gpu, cam, mesh):
    from naruto_amd.simulator import MeshSimHIP
    return MeshSimHIP(mesh, cam, erp_hw=(32, 64), face_w=32, far=100.0, device=gpu)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _rgbd(gpu, cam=CAM, **kw):
    from naruto_amd.odometry import RGBDOdometryHIP
    return RGBDOdometryHIP(cam, device=gpu, **kw)


def _depth_odom(gpu, cam=CAM, **kw):
    from naruto_amd.odometry import DepthOdometryHIP
    return DepthOdometryHIP(cam, device=gpu, **kw)


@pytest.fixture(scope="module")
def room_frames(gpu):
    """(colour [7,120,160,3], depth [7,120,160]) on the device: the base pose in the coloured room and the six prototype motions from it."""
    base = _look(OS.CASE_POSITION, CS.ROOM_CENTRE)
    poses = np.stack([base] + [base @ rel for rel in OS.CASES]).astype(np.float32)
    color, depth = _sim(gpu, CAM, _room()).simulate_batch(torch.from_numpy(poses))
    assert float((depth[0] > 0).float().mean()) > 0.9 and float(color[0].std()) > 0.05
    return color.contiguous(), depth.contiguous()


@pytest.fixture(scope="module")
def wall_frames(gpu):
    """(colour [4,120,160,3], depth [4,120,160], relative motions as the float32 poses carry them): the wall head on from 1.5 m."""
    base = RS.wall_pose()
    poses = np.stack([base] + [base @ rel for rel in RS.WALL_MOTIONS]).astype(np.float32)
    color, depth = _sim(gpu, CAM, RS.wall_mesh()).simulate_batch(torch.from_numpy(poses))
    assert bool((depth > 0).all())
    gt = poses.astype(np.float64)
    return color.contiguous(), depth.contiguous(), [np.linalg.inv(gt[0]) @ gt[k] for k in range(1, 4)]


# --------------------------------------------------------------------------------------------- 1. maps
@pytest.mark.parametrize("W,Hh", [(160, 120), (41, 31), (5, 4), (2, 2)])
def test_maps_equal_the_twin_in_every_bit(gpu, W, Hh):
    """Every finite value on the bits; a NaN (inf - inf, or the NaN pixel itself) where the twin has a NaN -- its sign and payload are no
    part of the contract."""
    cam = CS.camera(W, Hh, 0.75 * W)
    base = _look(OS.CASE_POSITION, CS.ROOM_CENTRE).astype(np.float32)
    color, depth = _sim(gpu, cam, _room()).simulate_batch(torch.from_numpy(base[None]))
    d0, c0 = depth[0].cpu().numpy().copy(), color[0].cpu().numpy().copy()
    assert (d0 > 0).all()
    od, dod = _rgbd(gpu, cam), _depth_odom(gpu, cam)
    assert [s[:2] for s in od.level_shapes] == [(Hh, W), (Hh // 2, W // 2), (Hh // 4, W // 4)]
    assert od.maps_bytes == 10 * 4 * sum(h * w for h, w, _ in od.level_shapes) and od.depth_maps_bytes == dod.maps_bytes
    hole = d0.copy()
    hole[Hh // 4:Hh // 2 + 1, W // 4:W // 2 + 1] = 0.0                 # a missing block with odd edges
    odd = c0.copy()
    odd[Hh // 2, W // 2, 1] = np.nan
    odd[0, 0, 2] = np.inf
    frames = {"as rendered": (d0, c0), "missing depth block": (hole, c0), "a NaN and an inf colour pixel": (d0, odd),
              "whole frame missing": (np.zeros_like(d0), np.zeros_like(c0))}
    for name, (d, c) in frames.items():
        got = od.frame_maps(torch.from_numpy(d).to(gpu), torch.from_numpy(c).to(gpu)).cpu().numpy()
        twin = RS.frame_maps(d, c, cam)
        want = RS.pack_maps(twin)
        assert got.shape == want.shape == (od.maps_bytes // 4,)
        assert np.array_equal(RS.canonical(got), RS.canonical(want)), (name, int((RS.canonical(got) != RS.canonical(want)).sum()))
        nd = dod.maps_bytes // 4
        depth_only = dod.frame_maps(torch.from_numpy(d).to(gpu)).cpu().numpy()
        assert np.array_equal(got[:nd].view(np.int32), depth_only.view(np.int32)), (name, "the depth part is DepthOdometryHIP's")
        for l in range(3):
            views = od.level_views(torch.from_numpy(got), l)
            assert len(views) == 6
            for k in range(3):
                assert np.array_equal(RS.canonical(views[3 + k].numpy()), RS.canonical(twin[1][l][k])), (name, l, k)
        if name == "whole frame missing":
            assert not (got != 0).any()
        elif name == "a NaN and an inf colour pixel":
            assert np.isnan(got[nd:]).any() and np.isinf(got[nd:]).any()
        elif min(W, Hh) > 4:
            assert (twin[1][0][1] != 0).any() and (twin[1][2][2] != 0).any(), "gradients at every level"


# --------------------------------------------------------------------------------------------- 2. rows and sums
def _accumulate_against_twin(gpu, cam, T, frames, tag, levels=1, **kw):
    """One evaluation at level 0 on the device and on the twin: rows and the 32 sums on the bits."""
    prev, cur, cprev, ccur = frames
    Hh, W = prev.shape
    od = _rgbd(gpu, cam, levels=levels, iters=(1,) * levels, **kw)
    mp = od.frame_maps(torch.from_numpy(prev).to(gpu), torch.from_numpy(cprev).to(gpu))
    mc = od.frame_maps(torch.from_numpy(cur).to(gpu), torch.from_numpy(ccur).to(gpu))
    tp, tc = RS.frame_maps(prev, cprev, cam, levels), RS.frame_maps(cur, ccur, cam, levels)
    rows = torch.full((Hh * W, 4), 7.0, dtype=torch.float64, device=gpu)
    state = od.init_state(T)
    sums = od.accumulate(0, mp, mc, state, rows=rows).cpu().numpy()
    weight = kw.get("photo_weight", RS.PHOTO_WEIGHT)
    gi, gr, pi, rI, terms = RS.rows_rgbd(T, OS.level_intrinsics(cam, levels)[0], tp[0][0], tc[0][0], tp[1][0], tc[1][0], photo_weight=weight)
    r = rows.cpu().numpy()
    assert np.array_equal(r[:, 0].astype(np.int64), gi), (tag, "geometric association")
    assert np.array_equal(_bits64(r[:, 1]), _bits64(gr)), (tag, "geometric residual")
    assert np.array_equal(r[:, 2].astype(np.int64), pi), (tag, "photometric association", int((r[:, 2].astype(np.int64) != pi).sum()))
    assert np.array_equal(_bits64(r[:, 3]), _bits64(rI)), (tag, "photometric residual")
    want = RS.reduce_sums(terms)
    assert sums.shape == (32,) and np.array_equal(_bits64(sums), _bits64(want)), (tag, "sums", np.abs(sums - want).max())
    assert sums[29] == (gi >= 0).sum() and sums[30] == (pi >= 0).sum() and sums[28] == sums[29] + sums[30]
    return SimpleRun(od=od, state=state, sums=sums, gi=gi, pi=pi, maps=(mp, mc))


class SimpleRun:
    def __init__(self, **kw):
        self.__dict__.update(kw)


SMALL_T = OS.relative_motion((0.3, -0.8, 0.5), 1.0, OS.CASE_ALONG, 0.02)


# the smallest frames with no interior pixel ((1,1), (3,3), (3,683)), with one ((4,4)) and with a few ((4,5), (5,5)); then pixel counts at
# the edges of a thread's eight pixels, a workgroup's round and share, a part-full last workgroup and the finishing launch's second round
@pytest.mark.parametrize("Hh,W", [(1, 1), (3, 3), (3, 683), (4, 4), (4, 5), (5, 5), (6, 43), (15, 17), (16, 16), (1, 257), (32, 64), (120, 160), (704, 768)])
def test_rows_and_sums_equal_the_twin(gpu, Hh, W):
    frames = RS.drawn_pair(Hh, W, seed=Hh * 1000 + W)
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    # two pixels of yaw (the rows stay, so a frame of three rows keeps its inliers) and 4 mm along x and z
    T = OS.relative_motion((0, 1, 0), math.degrees(2.0 / max(W, Hh)), (0.6, 0.0, -0.74), 0.004)
    run = _accumulate_against_twin(gpu, cam, T, frames, (Hh, W))
    print(f"{Hh} x {W}: {int(run.sums[29])} geometric rows, {int(run.sums[30])} photometric rows")
    if Hh < 4 or W < 4:
        assert run.sums[30] == 0
    if Hh >= 5 and W >= 5:
        assert run.sums[30] > 0
    if Hh >= 3 and W >= 3:
        assert run.sums[29] > 0
    known = {(4, 5): 2, (5, 5): 3, (6, 43): 122, (15, 17): 159, (120, 160): 18292}      # the twin's counts for these drawn pairs
    assert run.sums[30] == known.get((Hh, W), run.sums[30])
    if (Hh, W) == (120, 160):
        run = _accumulate_against_twin(gpu, cam, SMALL_T, frames, (Hh, W, "general motion"))
        assert run.sums[29] > 0 and run.sums[30] > 0


# --------------------------------------------------------------------------------------------- 3. edges
def _plane(Hh, W, d0):
    """A fronto-parallel plane with a gentle texture, the same image in both frames.  With f = 32 and d0 = 2 every vertex, every
    projection and so every bilinear weight below is exact in binary."""
    v, u = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    col = np.stack([0.5 + 0.3 * np.sin(0.21 * u + 0.3 * k) * np.cos(0.17 * v + 0.2 * k) for k in range(3)], -1).astype(np.float32)
    flat = np.full((Hh, W), d0, np.float32)
    return flat, flat, col, col


def test_rows_on_the_pixel_edges_and_behind_the_camera(gpu):
    Hh, W, d0, f = 24, 40, 2.0, 32.0
    cam = CS.camera(W, Hh, f)
    frames = _plane(Hh, W, d0)
    interior = slice(3 * W, (Hh - 3) * W)
    # whole pixels (a = 0 exactly) and half pixels (the x.5 association edge), the borders included
    for sx, sy in ((0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 2.0), (0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (-0.5, -0.5), (1.5, -2.5)):
        T = np.eye(4)
        T[0, 3], T[1, 3] = sx * d0 / f, -sy * d0 / f
        run = _accumulate_against_twin(gpu, cam, T, frames, ("edge", sx, sy))
        assert 0 < run.sums[30] < Hh * W and 0 < run.sums[29] < Hh * W
        if sy == 0.0 and sx == math.floor(sx):
            # pixel u projects to u + sx exactly: u0 = 1 and u0 + 1 = w - 2 are taken, one beyond each is not
            got = (run.pi.reshape(Hh, W)[3:Hh - 3] >= 0)
            want = np.array([1 <= u + sx and u + sx + 1 <= W - 2 for u in range(W)])
            assert (got == want[None, :]).all(), (sx, got[0], want)
            assert want[int(1 - sx)] and not want[int(1 - sx) - 1] and want[int(W - 3 - sx)] and not want[int(W - 3 - sx) + 1]
    # every point behind the camera: all 32 sums 0, degenerate, T unchanged
    T = np.eye(4)
    T[:3, :3] = OS.rotation((0, 1, 0), math.pi)
    run = _accumulate_against_twin(gpu, cam, T, RS.drawn_pair(Hh, W, 5), "behind")
    assert (run.gi == -1).all() and (run.pi == -1).all() and not run.sums.any()
    before = run.state.clone()
    run.od.step(0, run.state)
    got = run.od.read_state(run.state)
    assert got.status == ["degenerate"] and got.inliers == [0] and got.iterations == [0] and got.geometric_rows == 0 and got.photometric_rows == 0
    assert torch.equal(run.state[:16].view(torch.int64), before[:16].view(torch.int64)) and float(run.state[16]) == 1.0


# --------------------------------------------------------------------------------------------- 4. photo_weight = 0
@pytest.mark.parametrize("Hh,W", [(6, 43), (120, 160)])
def test_weight_zero_is_the_depth_odometry_in_every_bit(gpu, Hh, W):
    frames = RS.drawn_pair(Hh, W, seed=Hh * 1000 + W)
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    run = _accumulate_against_twin(gpu, cam, SMALL_T, frames, (Hh, W, "weight 0"), photo_weight=0.0)
    dod = _depth_odom(gpu, cam, levels=1, iters=(1,))
    nd = dod.maps_bytes // 4
    want = dod.accumulate(0, run.maps[0][:nd], run.maps[1][:nd], dod.init_state(SMALL_T)).cpu().numpy()
    assert want[28] > 0 and np.array_equal(_bits64(run.sums[:29]), _bits64(want))
    assert run.sums[29] == want[28] and run.sums[30] == 0.0 and run.sums[31] == 0.0 and (run.pi == -1).all()


# --------------------------------------------------------------------------------------------- 5. iteration by iteration
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


def test_iteration_by_iteration_against_the_twin(gpu, room_frames):
    color, depth = room_frames
    od = _rgbd(gpu)
    mp, mc = od.frame_maps(depth[0], color[0]), od.frame_maps(depth[3], color[3])           # 10 cm / 10 degrees
    tp = RS.frame_maps(depth[0].cpu().numpy(), color[0].cpu().numpy(), CAM)
    tc = RS.frame_maps(depth[3].cpu().numpy(), color[3].cpu().numpy(), CAM)
    assert np.array_equal(RS.canonical(mp.cpu().numpy()), RS.canonical(RS.pack_maps(tp)))
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
            terms = RS.rows_rgbd(T, cams[l], tp[0][l], tc[0][l], tp[1][l], tc[1][l])[4]
            assert np.array_equal(_bits64(sums), _bits64(RS.reduce_sums(terms))), (l, it)
            assert sums[29] > 0 and sums[30] > 0 and sums[28] == sums[29] + sums[30]
            od.step(l, state)
            s1 = state.cpu().numpy()
            Tn, done, status, upd, count, rmse = OS.step(sums[:29], T, upd, cap)
            bound = _step_bound(sums, T)
            err = np.abs(s1[:16].reshape(4, 4) - Tn).max()
            assert err <= bound, (l, it, err, bound)
            w = s1[16 + 8 * l:24 + 8 * l]
            assert (w[0] != 0.0) == done and int(w[1]) == status and int(w[2]) == upd and w[3] == count and abs(w[4] - rmse) <= 4 * EPS * rmse
            compared += 1
    assert compared >= 8
    dm, dd = OS.motion_error(state.cpu().numpy()[:16].reshape(4, 4), OS.CASES[2])
    assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG


# --------------------------------------------------------------------------------------------- 6. early out
def test_launches_of_a_finished_level_write_nothing(gpu, room_frames):
    color, depth = room_frames
    od = _rgbd(gpu)
    maps = od.frame_maps(depth[0], color[0])
    state = od.init_state(None)
    od.accumulate(2, maps, maps, state)                                # a frame against itself at T = identity: r = 0, xi = 0, converged
    od.step(2, state)
    got = od.read_state(state)
    assert got.status[2] == "converged" and got.iterations[2] == 1 and float(state[16 + 8 * 2]) == 1.0
    assert got.photometric_rows > 0 and got.inliers[2] == got.geometric_rows + got.photometric_rows
    od.sums.fill_(3.25)
    od.workspace.fill_(-1.5)
    rows = torch.full((od.level_shapes[2][0] * od.level_shapes[2][1], 4), 9.0, dtype=torch.float64, device=gpu)
    before = state.clone()
    for _ in range(3):
        od.accumulate(2, maps, maps, state, rows=rows)
        od.step(2, state)
    assert torch.equal(state.view(torch.int64), before.view(torch.int64))
    assert bool((od.sums == 3.25).all()) and bool((od.workspace == -1.5).all()) and bool((rows == 9.0).all())
    od.accumulate(1, maps, maps, state)                                # another level is still live
    assert not bool((od.sums == 3.25).any())


# --------------------------------------------------------------------------------------------- 7. reproducibility, recovery
def test_estimates_repeat_bit_for_bit_and_recover_the_six_motions(gpu, room_frames):
    color, depth = room_frames
    od = _rgbd(gpu)
    for k, rel in enumerate(OS.CASES):
        a = od.estimate(depth[0], color[0], depth[1 + k], color[1 + k])
        state_a = od.state.clone()
        b = od.estimate(depth[0], color[0], depth[1 + k], color[1 + k])
        assert torch.equal(state_a.view(torch.int64), od.state.view(torch.int64)), k
        assert a.transformation.dtype == np.float64 and a.transformation.shape == (4, 4) and np.array_equal(a.transformation, b.transformation)
        dm, dd = OS.motion_error(a.transformation, rel)
        print(f"room case {k}: {dm * 1e3:.3f} mm, {dd:.4f} deg; {a.status}, iterations {a.iterations}, inliers {a.inliers}, "
              f"rows {a.geometric_rows} + {a.photometric_rows}")
        assert "degenerate" not in a.status and "running" not in a.status
        assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG, (k, dm, dd)


def test_the_wall_is_degenerate_for_depth_and_recovered_with_colour(gpu, wall_frames):
    """The test that fails without the feature in substance: on the wall the depth odometry leaves T where it started, 30 / 50 / 80 mm
    from the true motion; the photometric rows pin the three free motions."""
    color, depth, rels = wall_frames
    od, dod = _rgbd(gpu), _depth_odom(gpu)
    for k, rel in enumerate(rels):
        d = dod.estimate(depth[0], depth[1 + k])
        assert d.status == ["degenerate"] * 3 and np.array_equal(d.transformation, np.eye(4)), (k, d.status)
        a = od.estimate(depth[0], color[0], depth[1 + k], color[1 + k])
        dm, dd = OS.motion_error(a.transformation, rel)
        print(f"wall motion {k}: depth only degenerate, {OS.motion_error(d.transformation, rel)[0] * 1e3:.1f} mm off; RGB-D {dm * 1e3:.4f} mm, {dd:.5f} deg; "
              f"{a.status}, iterations {a.iterations}, rows {a.geometric_rows} + {a.photometric_rows}")
        assert "degenerate" not in a.status and "running" not in a.status
        assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG, (k, dm, dd)


# --------------------------------------------------------------------------------------------- 8. the tracked run along a wall
N_RUN = 21
ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
TRACKING = {"disable": False, "iter": 10, "sample": 256, "lr_rot": 1e-3, "lr_trans": 1e-3, "ignore_edge_W": 2, "ignore_edge_H": 2, "iter_point": 0,
            "wait_iters": 100, "const_speed": True, "best": True}
REACH_M, REACH_DEG = 0.01, 0.57                                        # one tracking call: iter x lr


def _cfg():
    c = H.office_cfg(12, perturb=1.0)
    c["cam"].update(H=CAM["H"], W=CAM["W"], fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"], depth_trunc=100.0, near=0, far=5)
    c["mapping"]["bound"] = copy.deepcopy(ROOM)
    c["mapping"]["marching_cubes_bound"] = copy.deepcopy(ROOM)
    c["mapping"].update(sample=512, min_pixels_cur=128, keyframe_every=5, map_every=5, iters=10, first_iters=100, n_pixels=0.05, filter_depth=True)
    c["tracking"] = dict(TRACKING)
    c["mesh"].update(vis=500, voxel_eval=0.1, voxel_final=0.1)
    return c


def _along_the_wall(n):
    """1.2 m in front of the wall x = 0, looking straight at it: 3 cm along the wall (y) on even frames, +1.5 degrees of yaw on odd frames
    and back on even ones.  Every change of velocity is three times one tracking call's reach."""
    out, s = [], 0.0
    for k in range(n):
        if k > 0 and k % 2 == 0:
            s += 0.03
        out.append(_look([1.2, 2.2 + s, 1.4], [0.0, 2.2 + s, 1.4], yaw_deg=1.5 * (k % 2)))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def _run(gpu, raising=False, **kw):
    from naruto_amd import tracking
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    slam = CoSLAMNarutoHIP(_cfg(), voxel_size=0.1, active_ray=False, num_frames=N_RUN, seed=3, device=gpu, track=True, **kw)
    sim = _sim(gpu, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}, RS.wall_in_room())
    traj = _along_the_wall(N_RUN)
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
    return {"rgbd": _run(gpu, raising=True, motion_prior="rgbd_icp"), "depth": _run(gpu, motion_prior="depth_icp")}


def _prior_errors(run):
    _, _, traj, handed = run
    gt = traj.double().numpy()
    assert len(handed) == N_RUN - 1
    return [OS.motion_error(handed[i - 1].cpu().numpy().reshape(4, 4), np.linalg.inv(gt[i - 1]) @ gt[i]) for i in range(1, N_RUN)]


def _mean_err(out):
    return float((out["est_poses"][:, :3, 3].double() - out["poses"][:, :3, 3].double()).norm(dim=1).mean())


def test_rgbd_icp_hands_the_tracker_the_true_motion_along_a_wall(gpu, runs):
    from naruto_amd.odometry import RGBDOdometryHIP
    slam = runs["rgbd"][0]
    assert slam.motion_prior == "rgbd_icp" and isinstance(slam.odometry, RGBDOdometryHIP)
    errs = _prior_errors(runs["rgbd"])
    worst = (max(e[0] for e in errs), max(e[1] for e in errs))
    print(f"rgbd_icp prior against the true relative motion, worst of {N_RUN - 1} frames: {worst[0] * 1e3:.3f} mm, {worst[1]:.4f} deg")
    assert worst[0] <= OS.BOUND_M and worst[1] <= OS.BOUND_DEG
    assert bool(torch.isfinite(runs["rgbd"][1]["est_poses"]).all()) and torch.equal(runs["rgbd"][1]["poses"], runs["rgbd"][2])


def test_depth_icp_is_out_of_the_trackers_reach_along_a_wall(gpu, runs):
    """Measured on an MI355X (first run of these tests).  The priors: rgbd_icp at most 0.044 mm / 0.0195 degrees from the true relative
    motion over the 20 frames; depth_icp further than one tracking call's reach on 20 of 20 (worst 44.5 mm / 2.23 degrees).  AFTER
    tracking the gain is small: mean translation error rgbd_icp 34.846 mm against depth_icp 48.291 mm (ATE 2.245 cm rmse against
    3.246 cm), a ratio of 1.4, where the room run of tests/test_gpu_odometry.py has 18.  That the error after tracking be below half of
    depth_icp's was therefore NOT made an assertion: with a prior within 0.05 mm the 35 mm are the tracker's own on a plane (the field
    it tracks against constrains the in-plane motions by colour alone), a limit of the tracker and not of the prior.  Both values are
    printed."""
    assert runs["depth"][0].motion_prior == "depth_icp"
    e_rgbd, e_depth = _mean_err(runs["rgbd"][1]), _mean_err(runs["depth"][1])
    print(f"mean translation error after tracking along the wall: rgbd_icp {e_rgbd * 1e3:.3f} mm, depth_icp {e_depth * 1e3:.3f} mm; "
          f"ATE rgbd_icp {runs['rgbd'][1]['ate']}, depth_icp {runs['depth'][1]['ate']}")
    errs = _prior_errors(runs["depth"])
    far = sum(1 for dm, dd in errs if dm > REACH_M or dd > REACH_DEG)
    print(f"depth_icp prior further than {REACH_M * 1e3:.0f} mm or {REACH_DEG} deg from the true relative motion on {far} of {N_RUN - 1} frames; "
          f"worst {max(e[0] for e in errs) * 1e3:.1f} mm, {max(e[1] for e in errs):.2f} deg")
    assert far >= (N_RUN - 1) // 2


def test_the_rgbd_tracked_run_repeats_bit_for_bit(gpu, runs):
    slam, first, _, handed = runs["rgbd"]
    slam2, again, _, handed2 = _run(gpu, motion_prior="rgbd_icp")
    assert torch.equal(again["est_poses"].view(torch.int32), first["est_poses"].view(torch.int32))
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(handed, handed2))
    for (n, p), (_, q) in zip(slam.model.named_parameters(), slam2.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"
    assert not torch.equal(first["est_poses"], runs["depth"][1]["est_poses"])


def test_an_unknown_motion_prior_is_still_refused(gpu):
    from naruto_amd.slam import CoSLAMNarutoHIP
    with pytest.raises(ValueError, match="motion_prior"):
        CoSLAMNarutoHIP(_cfg(), num_frames=4, device=gpu, track=True, motion_prior="optical_flow")
    cfg = _cfg()
    cfg["tracking"]["disable"] = True
    with pytest.raises(ValueError, match="track=True"):
        CoSLAMNarutoHIP(cfg, num_frames=4, device=gpu, motion_prior="rgbd_icp")


# --------------------------------------------------------------------------------------------- 9. the command line
def test_rgbd_icp_through_the_command_line(gpu, tmp_path):
    from naruto_amd.mesh import Mesh
    from naruto_amd.run import main
    v, f, c = _room()
    rgba = np.concatenate([np.rint(c * 255.0), np.full((len(c), 1), 255.0)], 1).astype(np.uint8)
    Mesh(np.asarray(v, np.float64), np.asarray(f, np.int64), rgba).export(str(tmp_path / "room.ply"))
    cfg = _cfg()
    cfg["cam"].update(H=30, W=40, fx=30.0, fy=30.0, cx=19.0, cy=14.0)
    cfg["mapping"].update(n_pixels=0.5)
    with open(tmp_path / "cfg.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    common = ["--config", str(tmp_path / "cfg.yaml"), "--mesh", str(tmp_path / "room.ply"), "--num_iter", "12", "--start", "2.0", "4.0", "1.2",
              "--no_active_ray", "--seed", "5", "--track", "--planner", "gs_z_levels=[12]", "max_rot_deg=30", "rrt_max_iter=2000"]
    keys = {}
    for name, extra in (("rgbd", ["--motion_prior", "rgbd_icp"]), ("track", [])):
        out = main(common[:6] + ["--result_dir", str(tmp_path / name)] + common[6:-4] + extra + common[-4:])
        assert out["est_poses"].shape == (12, 4, 4) and bool(torch.isfinite(out["est_poses"]).all())
        keys[name] = set(dict(line.strip().split(",") for line in open(tmp_path / name / "results.txt")))
    assert keys["rgbd"] == keys["track"] == {"traj_len(m)", "ate_rmse(cm)", "ate_mean(cm)"}

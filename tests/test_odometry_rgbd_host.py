"""RGB-D odometry without a GPU: the numpy twin (tests/odometry_rgbd_spec.py) alone -- its properties, the photometric row against finite
differences of the residual, the wall scene where the depth odometry is degenerate -- and the entry points' argument validation through
the built library.

Run: python -m pytest tests/test_odometry_rgbd_host.py -q -s
"""
import ctypes as C
import math

import numpy as np
import pytest

import cull_spec as CS
import odometry_rgbd_spec as RS
import odometry_spec as OS
import sim_spec as SS

CAM = CS.camera(160, 120, 120.0)
SMALL = CS.camera(40, 30, 30.0)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_drawn = RS.drawn_pair


# ---------------------------------------------------------------------------------------------------------------- twin properties
def test_a_constant_image_gives_zero_gradients_and_rows_of_zeros():
    Hh, W = 24, 40
    cam = CS.camera(W, Hh, 40.0)
    prev, cur, _, _ = _drawn(Hh, W, 1)
    col = np.full((Hh, W, 3), 0.625, np.float32)
    mp, mc = RS.frame_maps(prev, col, cam, 2), RS.frame_maps(cur, col, cam, 2)
    for I, gx, gy in mp[1]:
        assert not gx.any() and not gy.any() and (I == I[0, 0]).all()
    T = OS.relative_motion((0.3, -0.8, 0.5), 1.0, OS.CASE_ALONG, 0.02)
    gi, gr, pi, rI, terms = RS.rows_rgbd(T, OS.level_intrinsics(cam, 2)[0], mp[0][0], mc[0][0], mp[1][0], mc[1][0])
    assert (pi >= 0).sum() > 100 and not rI.any()
    photo = terms[:, 1]
    assert not photo[:, :28].any() and np.array_equal(photo[:, 28], (pi >= 0).astype(float)) and np.array_equal(photo[:, 30], photo[:, 28])
    sums = RS.reduce_sums(terms)
    assert sums[28] == sums[29] + sums[30] and sums[30] == (pi >= 0).sum() and sums[31] == 0.0


@pytest.mark.parametrize("Hh,W", [(1, 1), (3, 3), (6, 43), (15, 17), (40, 70)])
def test_weight_zero_gives_the_depth_twins_sums_in_every_bit(Hh, W):
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    prev, cur, cp, cc = _drawn(Hh, W, Hh * 1000 + W)
    mp, mc = RS.frame_maps(prev, cp, cam, 1), RS.frame_maps(cur, cc, cam, 1)
    T = OS.relative_motion((0, 1, 0), math.degrees(2.0 / max(W, Hh)), (0.6, 0.0, -0.74), 0.004)
    lc = OS.level_intrinsics(cam, 1)[0]
    gi, gr, pi, rI, terms = RS.rows_rgbd(T, lc, mp[0][0], mc[0][0], mp[1][0], mc[1][0], photo_weight=0.0)
    idx, res, dterms = OS.rows(T, lc, mp[0][0], mc[0][0])
    sums, want = RS.reduce_sums(terms), OS.reduce_sums(dterms)
    assert np.array_equal(_bits64(sums[:29]), _bits64(want)) and np.array_equal(gi, idx) and np.array_equal(_bits64(gr), _bits64(res))
    assert sums[29] == want[28] and sums[30] == 0.0 and sums[31] == 0.0 and (pi == -1).all()
    # with the weight on, the same pixels' geometric rows stand and photometric rows join them where the frame has interior pixels
    _, _, pi, _, terms = RS.rows_rgbd(T, lc, mp[0][0], mc[0][0], mp[1][0], mc[1][0])
    sums = RS.reduce_sums(terms)
    assert sums[29] == want[28] and sums[28] == sums[29] + sums[30] and sums[30] == (pi >= 0).sum()
    assert (sums[30] == 0) if (Hh < 4 or W < 4) else (sums[30] > 0)


# ---------------------------------------------------------------------------------------------------------------- finite differences
def test_the_photometric_row_against_finite_differences_of_the_residual():
    """On an image that is linear in (u, v) the central differences and both bilinear samples are exact, so the residual
    w (I_prev(project(exp(xi) T p)) - I_cur) is a smooth function of xi and J = [q x g, g] is its derivative at xi = 0.  Central
    differences of step 1e-6 carry an error of the order of step^2 x the third derivative plus eps / step: 1e-9 relative to |J| = O(1)."""
    Hh, W = 48, 64
    cam = CS.camera(W, Hh, 60.0)
    prev, cur, _, _ = _drawn(Hh, W, 7)
    v, u = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ramp = (0.2 + 0.006 * u + 0.004 * v)[..., None] * np.ones(3)
    col_prev, col_cur = (ramp / 1.0).astype(np.float64), (ramp + 0.01).astype(np.float64)
    mp, mc = RS.frame_maps(prev, col_prev, cam, 1), RS.frame_maps(cur, col_cur, cam, 1)
    # the float32 ramp is not exactly linear: carry the maps in fp64 for this test (the twin reads them as doubles anyway)
    I = (0.299 + 0.587 + 0.114) * ramp[..., 0]
    gx, gy = np.zeros_like(I), np.zeros_like(I)
    gx[:, 1:-1], gy[1:-1, :] = (I[:, 2:] - I[:, :-2]) * 0.5, (I[2:, :] - I[:-2, :]) * 0.5
    ip, ic = (I, gx, gy), (I + 0.01, gx, gy)
    lc = OS.level_intrinsics(cam, 1)[0]
    T = OS.relative_motion((0.3, -0.8, 0.5), 1.5, OS.CASE_ALONG, 0.03)
    lam = float(np.float32(RS.PHOTO_WEIGHT))
    ok, j, rI, q, g = RS.photo_rows(T, lc, mp[0][0], mc[0][0], ip, ic)
    J = np.concatenate([np.cross(q, g), g], 1)
    assert ok.sum() > 1000
    step = 1e-6
    worst = 0.0
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = step
        okp, _, rp, _, _ = RS.photo_rows(OS.se3_exp(xi) @ T, lc, mp[0][0], mc[0][0], ip, ic)
        okm, _, rm, _, _ = RS.photo_rows(OS.se3_exp(-xi) @ T, lc, mp[0][0], mc[0][0], ip, ic)
        both = ok & okp & okm
        fd = lam * (rp - rm) / (2.0 * step)
        err = np.abs(fd - J[:, k])[both].max()
        scale = np.abs(J[both]).max()
        worst = max(worst, err / scale)
        assert both.sum() > 1000 and err <= 1e-6 * scale, (k, err, scale)
    print(f"photometric J against central differences: worst relative error {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------- the wall
@pytest.fixture(scope="module")
def wall_frames():
    """{(W, H): (depth [4,H,W], colour [4,H,W,3])}: the base view of the wall and the three motions from it."""
    v, f, c = RS.wall_mesh()
    base = RS.wall_pose()
    poses = np.stack([base] + [base @ rel for rel in RS.WALL_MOTIONS]).astype(np.float32)
    out = {}
    for cam in (CAM, SMALL):
        depth, colour, _ = SS.render_rgbd(v, f, c, poses, cam)
        assert (depth > 0).all()
        out[(cam["W"], cam["H"])] = (depth, colour)
    return poses, out


@pytest.mark.parametrize("cam", [CAM, SMALL], ids=["160x120", "40x30"])
def test_the_wall_is_degenerate_for_depth_and_pinned_by_the_image(wall_frames, cam):
    poses, frames = wall_frames
    depth, colour = frames[(cam["W"], cam["H"])]
    gt = poses.astype(np.float64)
    prev = RS.frame_maps(depth[0], colour[0], cam)
    for k in range(3):
        rel = np.linalg.inv(gt[0]) @ gt[1 + k]
        cur = RS.frame_maps(depth[1 + k], colour[1 + k], cam)
        T, status, its = OS.estimate(prev[0], cur[0], cam)
        assert status == [OS.DEGENERATE] * 3 and np.array_equal(T, np.eye(4)), "depth alone: every level degenerate, T unchanged"
        T, status, its = RS.estimate(prev, cur, cam)
        dm, dd = OS.motion_error(T, rel)
        print(f"{cam['W']} x {cam['H']} wall motion {k}: depth-only error {np.linalg.norm(rel[:3, 3]) * 1e3:.1f} mm (T unchanged); "
              f"RGB-D {dm * 1e3:.4f} mm, {dd:.5f} deg; status {[OS.STATUS[s] for s in status]}, iterations {its}")
        assert OS.DEGENERATE not in status
        assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG, (k, dm, dd)


# ---------------------------------------------------------------------------------------------------------------- argument validation
def test_entry_points_validate_their_arguments(built_lib):
    from naruto_amd import _lib
    lib = _lib.load()

    def desc(**kw):
        d = dict(H=30, W=40, levels=3, iters=(C.c_uint32 * _lib.ODOM_MAX_LEVELS)(10, 5, 4, 0), fx=30.0, fy=30.0, cx=19.5, cy=14.5, max_dist=0.25,
                 jump=0.15, band=0.1)
        d.update(kw)
        return _lib.NarutoOdomDesc(**d)

    good = desc()
    pixels = 30 * 40 + 15 * 20 + 7 * 10
    assert lib.naruto_odom_rgbd_maps_bytes(C.byref(good)) == lib.naruto_odom_maps_bytes(C.byref(good)) + 3 * 4 * pixels == 10 * 4 * pixels
    assert lib.naruto_odom_rgbd_workspace_bytes(C.byref(good)) == 1 * _lib.ODOM_RGBD_SUMS * 8 and _lib.ODOM_RGBD_SUMS == 32
    big = desc(H=680, W=1200)
    assert lib.naruto_odom_rgbd_workspace_bytes(C.byref(big)) == -(-680 * 1200 // 2048) * 32 * 8
    for bad in (desc(levels=0), desc(levels=5), desc(H=0), desc(fx=float("nan")), desc(fy=-1.0), desc(max_dist=float("nan")), desc(band=-0.1)):
        assert lib.naruto_odom_rgbd_maps_bytes(C.byref(bad)) == 0 and lib.naruto_odom_rgbd_workspace_bytes(C.byref(bad)) == 0
        assert lib.naruto_odom_rgbd_frame_maps(C.byref(bad), 8, 8, 8, None) != 0
    assert lib.naruto_odom_rgbd_maps_bytes(None) == 0
    # NULL pointers are refused before anything is launched (8 stands for an address that is never read)
    for args in ((None, 8, 8, 8), (C.byref(good), None, 8, 8), (C.byref(good), 8, None, 8), (C.byref(good), 8, 8, None)):
        assert lib.naruto_odom_rgbd_frame_maps(*args, None) != 0
    photo = _lib.NarutoOdomPhoto(weight=0.1, max_diff=0.3)
    ok = [C.byref(good), C.byref(photo), 0, 8, 8, 8, 8, 8, None, None]
    for k in (0, 1, 3, 4, 5, 6, 7):
        args = list(ok)
        args[k] = None
        assert lib.naruto_odom_rgbd_accumulate(*args) != 0, k
        assert b"odom_rgbd_accumulate" in lib.naruto_last_error()
    for level in (3, 4, 2 ** 31):
        args = list(ok)
        args[2] = level
        assert lib.naruto_odom_rgbd_accumulate(*args) != 0 and b"level" in lib.naruto_last_error()
    for w, m in ((float("nan"), 0.3), (-0.1, 0.3), (float("inf"), 0.3), (0.1, float("nan")), (0.1, -1.0)):
        args = list(ok)
        args[1] = C.byref(_lib.NarutoOdomPhoto(weight=w, max_diff=m))
        assert lib.naruto_odom_rgbd_accumulate(*args) != 0 and b"photometric" in lib.naruto_last_error(), (w, m)

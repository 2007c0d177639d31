"""Depth odometry without a GPU: the solver's own code on the host (naruto_debug_odom_solve) against numpy / scipy, the degenerate rule,
and the numpy twin (tests/odometry_spec.py) alone on the six prototype motions and over a ladder of larger ones.

Bound of the solve.  A = J^T J is symmetric positive definite with condition number k = cond_2(A).  Cholesky's solution is the exact one of
(A + dA) x = b with |dA| <= g(3n+1) |L||L^T| (Higham, Accuracy and Stability, Thm 10.4) and || |L||L^T| ||_2 <= n ||A||_2, so
||x - x*|| / ||x*|| <= n (3n+1) eps k = 114 eps k for n = 6; np.linalg.solve (LU with partial pivoting) obeys a bound of the same form in
practice.  The test allows their sum rounded up: 256 eps k.  The exponential is compared at the solver's OWN xi, where only its evaluation
error remains: a few dozen rounded operations on entries of size <= 1 + |t|, bound 64 eps (1 + |t|).

Run: python -m pytest tests/test_odometry_host.py -q -s
"""
import ctypes as C

import numpy as np
import pytest

import cull_spec as CS
import odometry_spec as OS

EPS = 2.0 ** -52


def _solve(sums):
    from naruto_amd import _lib
    s = _lib.NarutoOdomSolve(sums=(C.c_double * 29)(*[float(v) for v in sums]), status=-1)
    _lib.check(_lib.load().naruto_debug_odom_solve(C.byref(s)), "naruto_debug_odom_solve")
    return s.status, np.array(s.xi[:]), np.array(s.dT[:]).reshape(4, 4)


def _system(rs, n, scale_rot=1.0, rank=6):
    """Sums of n drawn rows J (and residuals): a well-conditioned 6 x 6 unless ``rank`` < 6 (rows from a rank-dimensional subspace)."""
    J = rs.standard_normal((n, 6)) * np.array([scale_rot] * 3 + [1.0] * 3)
    if rank < 6:
        J = (J @ rs.standard_normal((6, rank))) @ rs.standard_normal((rank, 6))
    r = rs.standard_normal(n) * 0.05
    A, b = J.T @ J, J.T @ r
    return np.array([A[i, j] for i in range(6) for j in range(i, 6)] + list(b) + [float(r @ r), float(n)]), A, b


def _twist(xi):
    w, t = xi[:3], xi[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    M[:3, 3] = t
    return M


@pytest.mark.parametrize("seed", range(8))
def test_solve_against_numpy_and_expm(seed):
    from scipy.linalg import expm
    rs = np.random.RandomState(seed)
    sums, A, b = _system(rs, 40 + 25 * seed, scale_rot=(1.0, 3.0, 0.3)[seed % 3])
    status, xi, dT = _solve(sums)
    assert status == OS.RUNNING
    ref = np.linalg.solve(A, -b)
    k = np.linalg.cond(A)
    err = np.linalg.norm(xi - ref) / np.linalg.norm(ref)
    print(f"seed {seed}: cond {k:.3g}, relative error {err:.3g}, bound {256 * EPS * k:.3g}")
    assert k < 1e4 and err <= 256 * EPS * k
    E = expm(_twist(xi))
    assert np.abs(dT - E).max() <= 64 * EPS * (1.0 + np.linalg.norm(xi[3:]))
    assert np.array_equal(dT[3], [0.0, 0.0, 0.0, 1.0])
    # the twin's step arithmetic is the same solver
    st, xi_t = OS.solve(sums)
    assert st == OS.RUNNING and np.linalg.norm(np.array(xi_t) - xi) / np.linalg.norm(ref) <= 256 * EPS * k
    assert np.abs(OS.se3_exp(xi) - E).max() <= 64 * EPS * (1.0 + np.linalg.norm(xi[3:]))


@pytest.mark.parametrize("theta", [0.0, 1e-9, 9.9e-3, 1.01e-2, 0.5, 3.0])
def test_exponential_across_the_series_threshold(theta):
    from scipy.linalg import expm
    xi = np.concatenate([theta * np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5]), [0.4, -0.2, 0.7]])
    # a system whose solution is xi: A = I, b = -xi
    sums = np.array([1.0 if i == j else 0.0 for i in range(6) for j in range(i, 6)] + list(-xi) + [1.0, 6.0])
    status, got, dT = _solve(sums)
    assert status == OS.RUNNING and np.array_equal(got, xi)
    assert np.abs(dT - expm(_twist(xi))).max() <= 64 * EPS * (1.0 + np.linalg.norm(xi[3:]))


def test_the_degenerate_rule():
    rs = np.random.RandomState(11)
    sums, _, _ = _system(rs, 50)
    for count, want in ((5.0, OS.DEGENERATE), (6.0, OS.RUNNING), (0.0, OS.DEGENERATE), (float("nan"), OS.DEGENERATE)):
        s = sums.copy()
        s[28] = count
        status, xi, dT = _solve(s)
        assert status == want == OS.solve(s)[0], count
        if want == OS.DEGENERATE:
            assert not xi.any() and np.array_equal(dT, np.eye(4))
    # a rank-5 system: the rows span five dimensions, the last pivot is rounding noise below 1e-12 x the largest diagonal entry
    s5, A5, _ = _system(rs, 50, rank=5)
    assert np.linalg.matrix_rank(A5) == 5
    status, xi, dT = _solve(s5)
    assert status == OS.DEGENERATE == OS.solve(s5)[0] and not xi.any() and np.array_equal(dT, np.eye(4))
    # points on a plane seen head on: rotation about the normal and translation in the plane are free -> a zero pivot
    J = np.zeros((30, 6))
    J[:, 5] = 1.0
    J[:, 0], J[:, 1] = rs.standard_normal(30), rs.standard_normal(30)
    A = J.T @ J
    sp = np.array([A[i, j] for i in range(6) for j in range(i, 6)] + [0.0] * 6 + [0.0, 30.0])
    assert _solve(sp)[0] == OS.DEGENERATE == OS.solve(sp)[0]
    # NaN sums are degenerate, not a NaN transform
    sn = sums.copy()
    sn[0] = float("nan")
    status, xi, dT = _solve(sn)
    assert status == OS.DEGENERATE and np.array_equal(dT, np.eye(4))


# ---------------------------------------------------------------------------------------------------------------- the twin alone
CAM = CS.camera(160, 120, 120.0)


def _look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64))
    p[:3, 3] = pos
    return p


@pytest.fixture(scope="module")
def scene():
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    base = _look(OS.CASE_POSITION, CS.ROOM_CENTRE)
    return v, f, base


def _maps(scene, rel, cam=CAM):
    v, f, base = scene
    depth = CS.render_depth(v, f, (base @ rel).astype(np.float32)[None], cam, near=0.01, far=100.0)[0]
    return OS.frame_maps(depth, cam)


def test_the_twin_recovers_the_six_prototype_motions(scene):
    prev = _maps(scene, np.eye(4))
    assert (prev[0][0] > 0).mean() > 0.9 and (np.abs(prev[0][2]).sum(-1) > 0).mean() > 0.8, "the scene fills the frame and has normals"
    worst = [0.0, 0.0]
    for k, rel in enumerate(OS.CASES):
        T, status, its = OS.estimate(prev, _maps(scene, rel), CAM)
        dm, dd = OS.motion_error(T, rel)
        print(f"case {k}: {dm * 1e3:.3f} mm, {dd:.4f} deg; status {[OS.STATUS[s] for s in status]}, iterations {its}")
        worst = [max(worst[0], dm), max(worst[1], dd)]
        assert OS.DEGENERATE not in status
        assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG, (k, dm, dd)
    print(f"worst of six: {worst[0] * 1e3:.3f} mm, {worst[1]:.4f} deg")


def test_the_twins_basin_table(scene):
    """Printed, not bounded: the largest yaw / translation of a fixed ladder the twin recovers to 5 mm / 0.25 degrees at 160 x 120, and
    the same at 80 x 60 (the basin grows with resolution)."""
    for cam in (CAM, CS.camera(80, 60, 60.0)):
        prev = _maps(scene, np.eye(4), cam)
        last = {}
        for name, ladder, make in (("yaw about y", (5.0, 10.0, 20.0, 30.0, 40.0), lambda a: OS.relative_motion((0, 1, 0), a, OS.CASE_ALONG, 0.0)),
                                   ("translation", (0.05, 0.1, 0.2, 0.4, 0.8), lambda d: OS.relative_motion((0, 1, 0), 0.0, OS.CASE_ALONG, d))):
            for s in ladder:
                rel = make(s)
                T, status, _ = OS.estimate(prev, _maps(scene, rel, cam), cam)
                dm, dd = OS.motion_error(T, rel)
                ok = dm <= OS.BOUND_M and dd <= OS.BOUND_DEG
                print(f"{cam['W']} x {cam['H']} {name} {s:g}: {dm * 1e3:.3f} mm {dd:.4f} deg {'recovered' if ok else 'LOST'}")
                if not ok:
                    break
                last[name] = s
            print(f"{cam['W']} x {cam['H']}: {name} recovered up to {last.get(name)}")

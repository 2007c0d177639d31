"""CPU tests of the rigid-alignment path (csrc/naruto_icp.h / naruto_icp.hip, naruto_amd.evaluation.icp): the C ABI's symbols and argument
validation, the Kabsch solver run on the host (naruto_debug_icp_solve) against the numpy twin, and the twin on its own.  Nothing here
needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import icp_spec as IS
import recon_spec as RS

NAMES = ("naruto_icp_transform", "naruto_icp_accumulate_workspace", "naruto_icp_accumulate", "naruto_icp_step", "naruto_debug_icp_solve")


def _solve(lib, sums, origin=None):
    s = (C.c_double * 17)(*[float(x) for x in sums])
    o = None if origin is None else (C.c_double * 3)(*[float(x) for x in origin])
    dT = (C.c_double * 16)()
    status = C.c_int32(-1)
    assert lib.naruto_debug_icp_solve(s, o, dT, C.byref(status)) == 0
    return np.array(dT[:], dtype=np.float64).reshape(4, 4), int(status.value)


def _pairs(n, seed, angle=7.0, noise=0.01):
    """n source points in a 2 x 1.5 x 1 m box around (3, 2.5, 1.4) and their images under a known rigid map, plus noise."""
    rs = np.random.RandomState(seed)
    centre = np.array([3.0, 2.5, 1.4])
    p = centre + rs.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 0.75, 0.5])
    M = IS.rigid(angle, 0.05, centre)
    q = p @ M[:3, :3].T + M[:3, 3] + rs.normal(0.0, noise, (n, 3))
    return p, q, centre


def test_symbols_are_declared_bound_and_exported(built_lib):
    from naruto_amd import _lib
    declared, defines = set(_lib.ABI.functions), _lib.ABI.defines          # include/naruto_hip.h as the binding read it
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(built_lib, name), name
    assert "naruto_icp.hip" in _lib.SOURCES and "naruto_icp.h" in _lib.SOURCES
    for s in ("naruto_icp.hip", "naruto_icp.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, s))
    for macro, value in (("NARUTO_ICP_SUMS", _lib.ICP_SUMS), ("NARUTO_ICP_STATE_DOUBLES", _lib.ICP_STATE_DOUBLES), ("NARUTO_ICP_RUNNING", _lib.ICP_RUNNING),
                         ("NARUTO_ICP_CONVERGED", _lib.ICP_CONVERGED), ("NARUTO_ICP_DEGENERATE", _lib.ICP_DEGENERATE),
                         ("NARUTO_ICP_MAX_ITERATION", _lib.ICP_MAX_ITERATION)):
        assert defines[macro] == value, macro
    assert _lib.ICP_STATUS[_lib.ICP_CONVERGED] == "converged" and _lib.ICP_STATUS[_lib.ICP_DEGENERATE] == "degenerate"


def test_entry_points_validate_arguments(built_lib):
    """Error codes, never a launch: nothing here touches a device."""
    lib = built_lib
    big = 2 ** 31
    o = (C.c_double * 3)(0.0, 0.0, 0.0)
    one = C.c_void_p(8)                                     # a non-NULL stand-in: every call below is refused before it is used
    # transform
    assert lib.naruto_icp_transform(0, one, 0, one, one, None) < 0 and b"zero points" in lib.naruto_last_error()
    assert lib.naruto_icp_transform(big, one, 0, one, one, None) < 0 and b"int32" in lib.naruto_last_error()
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert lib.naruto_icp_transform(10, args[0], 0, args[1], args[2], None) < 0 and b"NULL" in lib.naruto_last_error()
    # accumulate
    assert lib.naruto_icp_accumulate_workspace(0) == 0 and lib.naruto_icp_accumulate_workspace(big) == 0
    assert lib.naruto_icp_accumulate_workspace(1) >= 17 * 8 and lib.naruto_icp_accumulate_workspace(70001) >= 35 * 17 * 8
    assert lib.naruto_icp_accumulate(0, one, 10, one, one, one, 0.1, o, one, one, None) < 0 and b"zero points" in lib.naruto_last_error()
    assert lib.naruto_icp_accumulate(10, one, 0, one, one, one, 0.1, o, one, one, None) < 0 and b"zero points" in lib.naruto_last_error()
    assert lib.naruto_icp_accumulate(big, one, 10, one, one, one, 0.1, o, one, one, None) < 0 and b"int32" in lib.naruto_last_error()
    assert lib.naruto_icp_accumulate(10, one, big, one, one, one, 0.1, o, one, one, None) < 0 and b"int32" in lib.naruto_last_error()
    for bad in (float("nan"), -0.1, -float("inf")):
        assert lib.naruto_icp_accumulate(10, one, 10, one, one, one, bad, o, one, one, None) < 0 and b"distance" in lib.naruto_last_error()
    assert lib.naruto_icp_accumulate(10, one, 10, one, one, one, 0.1, None, one, one, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_icp_accumulate(10, one, 10, one, one, one, 0.1, (C.c_double * 3)(0.0, float("nan"), 0.0), one, one, None) < 0
    for k in range(6):
        ptrs = [one] * 6
        ptrs[k] = None
        assert lib.naruto_icp_accumulate(10, ptrs[0], 10, ptrs[1], ptrs[2], ptrs[3], 0.1, o, ptrs[4], ptrs[5], None) < 0 and b"NULL" in lib.naruto_last_error(), k
    # step
    assert lib.naruto_icp_step(one, 0, o, 30, 1e-6, 1e-6, one, None) < 0 and b"zero points" in lib.naruto_last_error()
    assert lib.naruto_icp_step(one, big, o, 30, 1e-6, 1e-6, one, None) < 0
    assert lib.naruto_icp_step(one, 10, o, 30, float("nan"), 1e-6, one, None) < 0 and lib.naruto_icp_step(one, 10, o, 30, 1e-6, float("nan"), one, None) < 0
    assert lib.naruto_icp_step(one, 10, None, 30, 1e-6, 1e-6, one, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_icp_step(None, 10, o, 30, 1e-6, 1e-6, one, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_icp_step(one, 10, o, 30, 1e-6, 1e-6, None, None) < 0 and b"NULL" in lib.naruto_last_error()
    # the host solver
    s = (C.c_double * 17)()
    dT = (C.c_double * 16)()
    st = C.c_int32(0)
    assert lib.naruto_debug_icp_solve(None, None, dT, C.byref(st)) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_debug_icp_solve(s, None, None, C.byref(st)) < 0 and lib.naruto_debug_icp_solve(s, None, dT, None) < 0


def test_icp_kernels_are_in_the_code_object_without_scratch(built_lib):
    from naruto_amd import _lib
    res = _lib.kernel_resources()
    for k in ("k_icp_transform<true>", "k_icp_transform<false>", "k_icp_accumulate", "k_icp_accumulate_finish", "k_icp_step"):
        assert k in res, k
    for k in ("k_icp_transform<true>", "k_icp_transform<false>", "k_icp_accumulate", "k_icp_accumulate_finish"):
        assert res[k].get("vgpr_spill_count", 0) == 0 and res[k].get("private_segment_fixed_size", 0) == 0, (k, res[k])
        assert res[k]["vgpr_count"] <= 128, (k, res[k])
    assert res["k_icp_accumulate"]["group_segment_fixed_size"] == 17 * 256 * 8


@pytest.mark.parametrize("n", [3, 257, 4099])
def test_solver_equals_the_twins_kabsch_on_well_conditioned_pairs(built_lib, n):
    """fp64 on inputs whose cross-covariance has s1 / s2 below 100 (the two leading singular pairs determine the rotation; three pairs
    are always coplanar, so s3 = 0 at n = 3): dT within 1e-12 of numpy's, an orthogonal R, det > 0."""
    from naruto_amd import _lib
    p, q, centre = _pairs(n, 100 + n)
    want = IS.kabsch(p, q)
    assert want is not None
    sv = np.linalg.svd((p - p.mean(0)).T @ (q - q.mean(0)), compute_uv=False)
    assert sv[0] / sv[1] < 100.0 and (n == 3 or sv[0] / sv[2] < 100.0)
    for origin in (centre, centre + 0.3):                   # the device passes the target box's centre: near the centroid, not on it
        dT, status = _solve(built_lib, IS.sums(p, q, np.zeros(n), origin), origin)
        assert status == _lib.ICP_RUNNING
        err = np.abs(dT - want).max()
        R = dT[:3, :3]
        orth = np.linalg.norm(R.T @ R - np.eye(3))
        print(f"n={n}: |dT - twin| {err:.3e}, |R^T R - I| {orth:.3e}, det {np.linalg.det(R):.16f}")
        assert err <= 1e-12
        assert orth <= 1e-14 and np.linalg.det(R) > 0.0
        assert np.array_equal(dT[3], [0.0, 0.0, 0.0, 1.0])


def test_solver_on_a_planar_cloud_equals_the_twin(built_lib):
    """All points in one plane: the cross-covariance has rank 2, its third singular pair is arbitrary, and the determinant correction
    decides the rotation.  Exact images (no noise), so the known map is recovered, as the twin recovers it."""
    from naruto_amd import _lib
    rs = np.random.RandomState(5)
    centre = np.array([3.0, 2.5, 1.4])
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, 0.8])
    p = centre + rs.uniform(-1, 1, (257, 1)) * e1 + rs.uniform(-1, 1, (257, 1)) * e2
    M = IS.rigid(11.0, 0.05, centre)
    q = p @ M[:3, :3].T + M[:3, 3]
    sv = np.linalg.svd((p - p.mean(0)).T @ (q - q.mean(0)), compute_uv=False)
    assert sv[2] < 1e-12 * sv[0] < sv[1]
    want = IS.kabsch(p, q)
    dT, status = _solve(built_lib, IS.sums(p, q, np.zeros(257), centre), centre)
    assert status == _lib.ICP_RUNNING
    R = dT[:3, :3]
    print("planar: |dT - twin|", np.abs(dT - want).max(), "|dT - known|", np.abs(dT - M).max())
    assert np.abs(dT - want).max() <= 1e-12 and np.abs(dT - M).max() <= 1e-12
    assert np.linalg.norm(R.T @ R - np.eye(3)) <= 1e-14 and np.linalg.det(R) > 0.0


def test_solver_on_a_mirrored_cloud_returns_a_rotation(built_lib):
    """q is the MIRROR image of p: the unconstrained optimum is a reflection; the determinant correction returns the best rotation, the
    twin's."""
    from naruto_amd import _lib
    p, _, centre = _pairs(257, 9)
    q = p.copy()
    q[:, 2] = 2.0 * centre[2] - q[:, 2]
    want = IS.kabsch(p, q)
    U, _, Vt = np.linalg.svd((p - p.mean(0)).T @ (q - q.mean(0)))
    assert np.linalg.det(Vt.T @ U.T) < 0.0                 # without the correction this input gives a reflection
    dT, status = _solve(built_lib, IS.sums(p, q, np.zeros(257), centre), centre)
    R = dT[:3, :3]
    assert status == _lib.ICP_RUNNING
    assert np.linalg.det(R) > 0.0 and abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.linalg.norm(R.T @ R - np.eye(3)) <= 1e-14
    print("mirrored: |dT - twin|", np.abs(dT - want).max())
    assert np.abs(dT - want).max() <= 1e-12


def test_solver_degenerate_inputs_return_the_identity(built_lib):
    from naruto_amd import _lib
    rs = np.random.RandomState(2)
    centre = np.array([3.0, 2.5, 1.4])
    line = centre + rs.uniform(-1, 1, (257, 1)) * np.array([0.3, -0.5, 0.8])
    M = IS.rigid(5.0, 0.02, centre)
    cases = {"collinear": (line, line @ M[:3, :3].T + M[:3, 3]), "two pairs": _pairs(2, 1)[:2]}
    for name, (p, q) in cases.items():
        assert IS.kabsch(p, q) is None, name
        dT, status = _solve(built_lib, IS.sums(p, q, np.zeros(len(p)), centre), centre)
        assert status == _lib.ICP_DEGENERATE, name
        assert np.array_equal(dT, np.eye(4)), name
    dT, status = _solve(built_lib, np.zeros(17))
    assert status == _lib.ICP_DEGENERATE and np.array_equal(dT, np.eye(4))
    dT, status = _solve(built_lib, np.full(17, np.nan))
    assert status == _lib.ICP_DEGENERATE and np.array_equal(dT, np.eye(4))


def table_clouds(n_target, n_source, angle, t):
    """A row of the test table, from the numpy restatement of the sampler: target = n_target surface samples of the room-plus-sphere
    mesh (seed 0), source = the first n_source of them displaced by the known rigid map.  -> (source, target, T_known)."""
    from naruto_amd import synthetic as syn
    v, f = syn.room_sphere_mesh(0.0, 0.8)
    target, _ = RS.sample_surface(v, f, np.cumsum(RS.face_areas(v, f)), n_target, 0)
    known = IS.rigid(angle, t, target.astype(np.float64).mean(0))
    return IS.transform(target[:n_source], known), target, known


@pytest.mark.parametrize("n_target,n_source,angle,t,iterations,fitness0", [(20000, 4099, 2.0, 0.03, 8, 0.9436), (4099, 4099, 1.0, 0.02, 4, None),
                                                                         (20000, 4099, 4.0, 0.06, 15, 0.679)])
def test_twin_converges_on_the_table_rows(n_target, n_source, angle, t, iterations, fitness0):
    source, target, known = table_clouds(n_target, n_source, angle, t)
    out = IS.icp(source, target)
    res = out["transformation"] @ known - np.eye(4)
    print(f"twin {n_target} x {n_source}, {angle} deg, {t} m: {out['iterations']} iterations, fitness {out['history'][0][0]:.4f} -> {out['fitness']}, "
          f"residual rotation {np.abs(res[:3, :3]).max():.2e}, translation {np.abs(res[:3, 3]).max():.2e} m")
    assert out["converged"] and out["status"] == "converged" and out["fitness"] == 1.0
    assert abs(out["iterations"] - iterations) <= 1 and len(out["history"]) == out["iterations"] + 1
    if fitness0 is not None:
        assert abs(out["history"][0][0] - fitness0) < 5e-4
    assert np.abs(res).max() <= 1e-6                        # one float32 ulp at 6 m is 4.8e-7; the twin reaches 1e-9
    assert out["inlier_rmse"] < 1e-6


def test_twin_stops_degenerate_without_inliers():
    target = np.random.RandomState(0).uniform(0, 1, (500, 3)).astype(np.float32)
    out = IS.icp(target[:50] + np.float32(3.0), target)
    assert out["status"] == "degenerate" and not out["converged"] and out["iterations"] == 0 and out["fitness"] == 0.0 and out["inlier_rmse"] == 0.0
    assert np.array_equal(out["transformation"], np.eye(4)) and out["history"] == [(0.0, 0.0)]

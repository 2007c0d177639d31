"""The tracked run's host side (no GPU): the pose chain's log map by the kernels' own code (naruto_debug_pose_log) against
tracking.matrices_to_pose6, evaluation.ate against a numpy restatement, the new entry points' argument checks, the --track switch and the
constructor's refusals."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers as H

THETAS = (0.0, 1e-8, 1e-4, 0.5, 3.1, math.pi - 1e-6)
AXES = ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.3, -0.8, 0.5))


def _rotation(axis, theta):
    """Rodrigues in fp64 numpy."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def _poses():
    out = []
    for n, axis in enumerate(AXES):
        for m, th in enumerate(THETAS):
            p = np.eye(4)
            p[:3, :3] = _rotation(axis, th)
            p[:3, 3] = [0.5 * n - 1.0, 2.0 + 0.25 * m, -0.125 * (n + m)]
            out.append(p)
    return torch.from_numpy(np.stack(out)).float()             # the fp32 matrices both sides start from


def test_log_map_equals_the_host_conversion(built_lib):
    from naruto_amd import pose_chain, tracking
    poses = _poses()
    got = pose_chain.pose_log_host(poses)
    ref = tracking.matrices_to_pose6(poses).float()
    assert got.shape == ref.shape == (len(AXES) * len(THETAS), 6) and got.dtype == torch.float32
    # both sides compute in fp64 from the same fp32 inputs and round once: a straddled rounding at most (2^-22 relative: one fp32 ulp
    # at the bottom of a binade); the floor covers a component that is mathematically zero
    tol = 2.0 ** -22 * ref.double().abs() + 1e-12
    err = (got.double() - ref.double()).abs()
    assert bool((err <= tol).all()), (float((err - tol).max()), got[(err > tol).any(1)], ref[(err > tol).any(1)])
    # the angles are the ones put in (a log map that returned its reference's garbage would pass the line above)
    ang = got[:, :3].double().norm(dim=1).reshape(len(AXES), len(THETAS))
    for m, th in enumerate(THETAS):
        assert bool(((ang[:, m] - th).abs() <= 1e-6 + 1e-3 * (th > 3.0)).all()), (th, ang[:, m])
    assert torch.equal(got[:, 3:], poses[:, :3, 3])
    # one matrix at a time gives the same bits as the batch
    assert torch.equal(pose_chain.pose_log_host(poses[7]), got[7:8])


def test_log_map_of_the_identity_is_exactly_zero(built_lib):
    from naruto_amd import pose_chain
    got = pose_chain.pose_log_host(torch.eye(4)[None])
    assert got.shape == (1, 6) and int(got.view(torch.int32).abs().sum()) == 0            # +0.0, six times


def _ate_numpy(est, gt):
    """The contract restated: Kabsch with the determinant correction, no scale; rmse and mean of the residual norms, in cm."""
    e, g = np.asarray(est, np.float64)[:, :3, 3], np.asarray(gt, np.float64)[:, :3, 3]
    ec, gc = e - e.mean(0), g - g.mean(0)
    U, _, Vt = np.linalg.svd(ec.T @ gc)
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    r = np.linalg.norm(ec @ R.T - gc, axis=1)
    return float(np.sqrt(np.mean(r ** 2)) * 100.0), float(np.mean(r) * 100.0)


def _trajectory(n=60):
    k = np.arange(n, dtype=np.float64)
    p = np.tile(np.eye(4), (n, 1, 1))
    p[:, :3, 3] = np.stack([1.0 + 0.05 * k, 2.0 + 0.5 * np.sin(0.2 * k), 1.2 + 0.01 * k * np.cos(0.1 * k)], 1)
    return p


def test_ate():
    from naruto_amd.evaluation import ate
    gt = _trajectory()
    # a rigidly moved copy: zero
    T = np.eye(4)
    T[:3, :3] = _rotation((0.2, 0.9, -0.4), 2.3)
    T[:3, 3] = [3.0, -1.0, 0.5]
    out = ate(T @ gt, gt)
    assert set(out) == {"ate_rmse_cm", "ate_mean_cm"}
    assert 0.0 <= out["ate_rmse_cm"] <= 1e-9 and 0.0 <= out["ate_mean_cm"] <= 1e-9, out
    # a known offset pattern on top of the rigid motion
    est = T @ gt
    k = np.arange(len(gt))
    est[:, :3, 3] += 0.03 * np.stack([np.sin(0.7 * k), np.cos(1.3 * k), ((k % 3) - 1.0)], 1)
    out = ate(torch.from_numpy(est).float().double(), torch.from_numpy(gt))
    rmse, mean = _ate_numpy(torch.from_numpy(est).float().double().numpy(), gt)
    assert 1.0 < mean < rmse < 6.0                                                       # centimetres, and a spread
    assert abs(out["ate_rmse_cm"] - rmse) <= 1e-10 * rmse and abs(out["ate_mean_cm"] - mean) <= 1e-10 * mean, (out, rmse, mean)
    # a mirrored trajectory is NOT aligned by a reflection: the determinant correction keeps R a rotation
    mirrored = gt.copy()
    mirrored[:, 2, 3] *= -1.0
    assert ate(mirrored, gt)["ate_rmse_cm"] > 1.0
    for n in (0, 1, 2):
        with pytest.raises(ValueError):
            ate(gt[:n], gt[:n])
    with pytest.raises(ValueError):
        ate(gt[:5], gt[:6])


def test_entry_points_check_their_arguments(built_lib):
    from naruto_amd import _lib
    lib, one = built_lib, C.c_void_p(64)                  # a non-NULL pointer no check dereferences: every call below returns before a launch

    def refused(rc, word):
        msg = lib.naruto_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    refused(lib.naruto_pose_log(1, None, one, None), "pose_log")
    refused(lib.naruto_pose_log(1, one, None, None), "pose_log")
    refused(lib.naruto_pose_log(0, one, one, None), "pose_log")
    refused(lib.naruto_pose_predict(None, 8, 1, 1, one, None), "pose_predict")
    refused(lib.naruto_pose_predict(one, 8, 1, 1, None, None), "pose_predict")
    refused(lib.naruto_pose_predict(one, 8, 0, 1, one, None), "pose_predict")
    refused(lib.naruto_pose_predict(one, 8, 8, 1, one, None), "pose_predict")
    refused(lib.naruto_pose_commit(None, one, 8, 1, 5, one, None), "pose_commit")
    refused(lib.naruto_pose_commit(one, None, 8, 1, 5, one, None), "pose_commit")
    refused(lib.naruto_pose_commit(one, one, 8, 1, 5, None, None), "pose_commit")
    refused(lib.naruto_pose_commit(one, one, 8, 0, 5, one, None), "pose_commit")
    refused(lib.naruto_pose_commit(one, one, 8, 8, 5, one, None), "pose_commit")
    refused(lib.naruto_pose_commit(one, one, 8, 1, 0, one, None), "pose_commit")
    refused(lib.naruto_pose_scatter(None, 11, one, 3, 5, 10, 1, None), "pose_scatter")
    refused(lib.naruto_pose_scatter(one, 11, None, 3, 5, 10, 1, None), "pose_scatter")
    refused(lib.naruto_pose_scatter(one, 11, one, 0, 5, 10, 1, None), "pose_scatter")
    refused(lib.naruto_pose_scatter(one, 11, one, 3, 0, 10, 1, None), "pose_scatter")
    refused(lib.naruto_pose_scatter(one, 11, one, 3, 5, 11, 1, None), "pose_scatter")           # the current frame past the tensor
    refused(lib.naruto_pose_scatter(one, 11, one, 5, 5, 10, 1, None), "pose_scatter")           # keyframe 3 would be frame 15 of 11
    refused(lib.naruto_pose_resolve(None, one, 4, 5, one, None), "pose_resolve")
    refused(lib.naruto_pose_resolve(one, None, 4, 5, one, None), "pose_resolve")
    refused(lib.naruto_pose_resolve(one, one, 4, 5, None, None), "pose_resolve")
    refused(lib.naruto_pose_resolve(one, one, 0, 5, one, None), "pose_resolve")
    refused(lib.naruto_pose_resolve(one, one, 4, 0, one, None), "pose_resolve")
    refused(lib.naruto_debug_pose_log(1, None, one), "debug_pose_log")
    refused(lib.naruto_debug_pose_log(1, one, None), "debug_pose_log")
    assert "naruto_posechain.hip" in _lib.SOURCES
    import naruto_amd
    assert naruto_amd.pose_chain.pose_resolve is not None                                       # the lazy table knows the module


def _cfg():
    c = H.office_cfg(12, perturb=1.0)
    c["cam"].update(H=30, W=40, fx=30.0, fy=30.0, cx=19.5, cy=14.5)
    c["mapping"].update(sample=128, min_pixels_cur=16, keyframe_every=5, map_every=5, iters=10, first_iters=20, n_pixels=0.5)
    return c


def test_track_switch_parses():
    from naruto_amd.run import parse_args
    base = ["--config", "c.yaml", "--mesh", "m.ply", "--num_iter", "5", "--result_dir", "out"]
    assert parse_args(base).track is False
    assert parse_args(base + ["--track"]).track is True


def test_constructor_refusals(monkeypatch):
    from naruto_amd import _lib
    from naruto_amd.slam import CoSLAMNarutoHIP
    touched = []

    def no_load():
        touched.append(1)
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    cfg = _cfg()
    cfg["tracking"] = {"disable": False}
    with pytest.raises(NotImplementedError, match="track=True.*TrackerHIP"):          # the config alone does not switch tracking on
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=11)
    cfg["tracking"] = {"disable": False, "iter_point": 1}
    with pytest.raises(NotImplementedError, match="iter_point"):
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=11, track=True)
    cfg["tracking"] = {"disable": True}
    cfg["training"]["rot_rep"] = "quat"
    with pytest.raises(NotImplementedError, match="rot_rep"):
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=11, track=True)
    assert not touched

"""Frame-to-model alignment without a GPU: the numpy twin (tests/field_registration_spec.py) on its analytic box room, and the header /
binding entries (nothing is launched).

The room is 4 x 3 x 2.5 m with trunc 0.1; frames of 40 x 30 and 80 x 60 pixels from two viewpoints; the vertex maps are float32, made by
odometry_spec.frame_maps as the device makes them, one level per frame size (a 2 x 2 mean of a plane's depth under perspective is not on
the plane, so a pyramid's coarser levels are not exact points of the room and could not meet the bound below).

The bound.  On exact points the fp64 loop reaches 1e-10 mm.  A float32 vertex moves a coordinate by at most 2^-24 x 5 m = 3e-7 m; the
least-squares pose averages those roundings, and no point can pull it further than its own rounding, so 0.01 mm = about 30 roundings and
0.001 degrees = 1.7e-5 rad x 1 m = 17 um at a metre are met with a wide margin; the measured errors are printed.

Run: python -m pytest tests/test_field_registration_host.py -q -s
"""
import math

import numpy as np
import pytest

import cull_spec as CS
import field_registration_spec as FS
import odometry_spec as OS

ROOM = FS.BoxRoom((4.0, 3.0, 2.5), trunc=0.1)
VIEWS = (((1.4, 1.2, 1.2), (4.0, 3.0, 0.4)), ((3.1, 2.0, 1.4), (0.0, 0.3, 0.2)))
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
GATE = FS.gate(max_trans=0.2, max_rot_deg=10.0)         # the prototype's starts reach 12 cm: the verdict is not what this file studies


def _look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64))
    p[:3, 3] = pos
    return p


def _f32_pose(p):
    """A pose whose entries are float32 numbers: est[i] is float32, and the start must be representable for the test to know it exactly."""
    return np.asarray(p, np.float32).astype(np.float64)


def _starts(true):
    out = []
    for k, (m, deg) in enumerate(FS.STARTS):
        if m == 0.0:
            out += [(f"{deg} deg about axis {a}", FS.perturb(true, 0.0, FS.START_ALONG, deg, AXES[a])) for a in range(3)]
        else:
            out.append((f"{m} m, {deg} deg", FS.perturb(true, m, FS.START_ALONG, deg, FS.START_AXIS)))
    return out


def _verts(cam, true):
    return {0: OS.frame_maps(ROOM.depth(true, cam), cam, levels=1)[0][1].reshape(-1, 3)}


def _align(verts, start, levels=(0,), iters=(10,), g=GATE, field=None, **kw):
    return FS.align(verts, start, field or ROOM.field, ROOM.trunc, ROOM.bbox_min, ROOM.bbox_max, levels, iters, g, **kw)


@pytest.mark.parametrize("W,Hh", [(40, 30), (80, 60)])
def test_the_twin_recovers_the_prototypes_perturbations(W, Hh):
    cam = CS.camera(W, Hh, 0.75 * W)
    worst = [0.0, 0.0]
    for pos, at in VIEWS:
        true = _look(pos, at)
        verts = _verts(cam, true)
        for name, start in _starts(true):
            start = _f32_pose(start)
            out = _align(verts, start)
            dm, dd = FS.pose_error(out["T"], true)
            worst = [max(worst[0], dm), max(worst[1], dd)]
            assert out["passed"] and out["status"][0] == OS.CONVERGED, (pos, name, out["status"], out["record"])
            assert out["iterations"][0] <= 7, (pos, name, out["iterations"])
            assert dm <= 1e-5 and dd <= 1e-3, (pos, name, dm, dd)
            assert out["record"][4] <= out["record"][3] and out["record"][2] >= 0.25 * out["record"][1]
    print(f"{W} x {Hh}: worst of {2 * 7} starts {worst[0] * 1e3:.3e} mm, {worst[1]:.3e} deg")


def test_a_start_half_a_metre_away_is_degenerate_and_refused():
    cam = CS.camera(40, 30, 30.0)
    true = _look(*VIEWS[0])
    verts = _verts(cam, true)
    start = _f32_pose(FS.perturb(true, 0.5, (0.62, 0.55, -0.56), 0.0, None))
    x, q, valid = FS.points(start, verts[0], ROOM.bbox_min, ROOM.bbox_max)
    sdf, _ = ROOM.field(x)
    assert valid.all() and (np.abs(sdf) == 1.0).all(), "every point is saturated"
    out = _align(verts, start)
    assert out["status"][0] == OS.DEGENERATE and not out["passed"] and out["record"][0] == 0.0 and out["record"][2] == 0.0
    assert np.array_equal(out["T"].view(np.int64), start.view(np.int64))
    assert out["record"][3] == -1.0 and out["record"][4] == -1.0, "no rows: the rmse is not a number and is recorded as -1"


def test_a_wall_seen_head_on_is_degenerate():
    cam = CS.camera(40, 30, 60.0)                                   # a narrow view from the room's middle straight at the wall x = 4
    true = np.eye(4)
    true[:3, :3] = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])    # the camera's -z is the field's +x
    true[:3, 3] = (2.0, 1.5, 1.25)
    verts = _verts(cam, true)
    q = FS.points(true, verts[0], ROOM.bbox_min, ROOM.bbox_max)[1]
    assert np.abs(q[:, 0] - 4.0).max() < 1e-5, "only the one wall is in view"
    start = _f32_pose(FS.perturb(true, 0.03, (1.0, 0.2, 0.1), 0.0, None))
    out = _align(verts, start)
    assert out["status"][0] == OS.DEGENERATE and not out["passed"]
    assert np.array_equal(out["T"].view(np.int64), start.view(np.int64))


def test_a_non_finite_field_value_removes_that_row_only():
    cam = CS.camera(40, 30, 30.0)
    true = _look(*VIEWS[1])
    verts = _verts(cam, true)[0]
    start = _f32_pose(FS.perturb(true, 0.03, FS.START_ALONG, 1.5, FS.START_AXIS))
    x, q, valid = FS.points(start, verts, ROOM.bbox_min, ROOM.bbox_max)
    sdf, d_x = ROOM.field(x)
    args = (ROOM.trunc, ROOM.bbox_min, ROOM.bbox_max)
    flag0, r0, t0 = FS.terms(sdf, d_x, q, valid, *args)
    good = np.flatnonzero(flag0)
    assert len(good) > 100
    picks = good[[3, 17, 40, 77, 90]]
    bad_sdf, bad_dx = sdf.copy(), d_x.copy()
    bad_sdf[picks[0]], bad_sdf[picks[1]] = np.nan, np.inf
    bad_dx[picks[2], 1], bad_dx[picks[3], 0], bad_dx[picks[4]] = np.nan, -np.inf, 0.0
    flag, r, t = FS.terms(bad_sdf, bad_dx, q, valid, *args)
    keep = np.ones(len(sdf), bool)
    keep[picks] = False
    assert not flag[picks].any() and not r[picks].any() and not t[picks, :29].any() and (t[picks, 29] == 1.0).all()
    assert np.array_equal(flag[keep], flag0[keep]) and np.array_equal(t[keep].view(np.int64), t0[keep].view(np.int64))
    sums = FS.reduce_sums(t)
    assert np.isfinite(sums).all() and sums[28] == flag0.sum() - 5 and sums[29] == valid.sum()


def test_a_fail_returns_the_starts_bits():
    cam = CS.camera(40, 30, 30.0)
    true = _look(*VIEWS[0])
    verts = _verts(cam, true)
    start = _f32_pose(FS.perturb(true, 0.05, FS.START_ALONG, 0.0, None))
    free = _align(verts, start)
    assert free["passed"] and FS.pose_error(free["T"], true)[0] < 1e-5
    for name, g in (("max_trans", FS.gate(max_trans=0.04, max_rot_deg=10.0)),):
        out = _align(verts, start, g=g)
        assert not out["passed"] and out["record"][0] == 0.0, name
        assert np.array_equal(out["T"].view(np.int64), start.view(np.int64)), name
        assert out["status"][0] == OS.CONVERGED and np.array_equal(out["record"][1:], free["record"][1:]), "the figures are the free run's"
    rot = _f32_pose(FS.perturb(true, 0.0, None, 3.0, (0, 1, 0)))
    out = _align(verts, rot, g=FS.gate(max_trans=0.2, max_rot_deg=2.0))
    assert not out["passed"] and np.array_equal(out["T"].view(np.int64), rot.view(np.int64))
    # a NaN fails its comparison
    nan = start.copy()
    nan[0, 3] = np.nan
    out = _align(verts, nan)
    assert not out["passed"] and np.array_equal(out["T"].view(np.int64), nan.view(np.int64)) and np.isfinite(out["record"]).all()


def test_commit_is_pose_predict_relatives_rounding_and_log():
    import torch
    from naruto_amd.tracking import matrices_to_pose6
    rs = np.random.RandomState(4)
    for k in range(12):
        T = np.eye(4)
        T[:3, :3] = OS.rotation(rs.standard_normal(3), rs.uniform(0.0, 3.1) if k else 0.0)
        T[:3, 3] = rs.uniform(-4.0, 4.0, 3)
        est, pose6 = FS.commit(T)
        assert est.dtype == np.float32 and np.array_equal(est, T.astype(np.float32))
        want = matrices_to_pose6(torch.from_numpy(est)[None])[0].numpy()
        assert pose6.dtype == np.float32 and np.abs(pose6 - want).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(want).max()), (k, pose6, want)
        assert np.array_equal(pose6[3:], est[:3, 3])


def test_the_header_and_the_binding_have_the_entries():
    import ctypes as C
    from naruto_amd import _lib
    names = ["naruto_sdfreg_workspace_bytes", "naruto_sdfreg_points", "naruto_sdfreg_accumulate", "naruto_sdfreg_init", "naruto_sdfreg_verdict",
             "naruto_sdfreg_commit"]
    for n in names:
        assert n in _lib.SIGNATURES, n
    assert _lib.SIGNATURES["naruto_sdfreg_workspace_bytes"] == (C.c_size_t, [C.POINTER(_lib.NarutoOdomDesc)])
    res, args = _lib.SIGNATURES["naruto_sdfreg_accumulate"]
    assert res is C.c_int and args[:4] == [C.POINTER(_lib.NarutoOdomDesc), C.POINTER(_lib.NarutoSdfRegDesc), C.c_uint32, C.c_int32] and len(args) == 13
    assert (_lib.SDFREG_SUMS, _lib.SDFREG_STATE_DOUBLES, _lib.SDFREG_RECORD) == (FS.SUMS, _lib.ODOM_STATE_DOUBLES + 16, FS.RECORD)
    fields = dict(_lib.NarutoSdfRegDesc._fields_)
    assert set(fields) == {"trunc", "sdf_gate", "bbox_min", "bbox_max", "n_levels", "levels", "iters"}
    assert C.sizeof(_lib.NarutoSdfRegDesc) == 4 * (2 + 6 + 1 + 2 * _lib.ODOM_MAX_LEVELS) and C.sizeof(_lib.NarutoSdfRegGate) == 24


def test_the_library_refuses_bad_arguments(built_lib):
    import ctypes as C
    from naruto_amd import _lib
    lib = built_lib
    od = _lib.NarutoOdomDesc(H=30, W=40, levels=3, iters=(C.c_uint32 * 4)(6, 6, 1, 0), fx=30.0, fy=30.0, cx=19.5, cy=14.5, max_dist=0.25, jump=0.15, band=0.1)
    assert lib.naruto_sdfreg_workspace_bytes(C.byref(od)) == 30 * 8

    def desc(**kw):
        d = dict(trunc=0.1, sdf_gate=0.9, bbox_min=(C.c_float * 3)(0, 0, 0), bbox_max=(C.c_float * 3)(4, 3, 2.5), n_levels=2,
                 levels=(C.c_uint32 * 4)(2, 1, 0, 0), iters=(C.c_uint32 * 4)(6, 6, 0, 0))
        d.update(kw)
        return _lib.NarutoSdfRegDesc(**d)
    one = 8                                                              # a non-NULL address: every call below is refused before any launch
    for why, d in (("trunc", desc(trunc=0.0)), ("trunc", desc(sdf_gate=float("nan"))), ("bounding box", desc(bbox_max=(C.c_float * 3)(4, 0, 2.5))),
                   ("levels", desc(n_levels=0)), ("levels", desc(levels=(C.c_uint32 * 4)(1, 2, 0, 0))), ("levels", desc(levels=(C.c_uint32 * 4)(3, 1, 0, 0))),
                   ("cap", desc(iters=(C.c_uint32 * 4)(6, 0, 0, 0)))):
        assert lib.naruto_sdfreg_points(C.byref(od), C.byref(d), 1, 1, one, one, one, one, one, None) != 0
        assert why in lib.naruto_last_error().decode(), (why, lib.naruto_last_error())
    assert lib.naruto_sdfreg_points(C.byref(od), C.byref(desc()), 3, 1, one, one, one, one, one, None) != 0
    assert lib.naruto_sdfreg_points(C.byref(od), C.byref(desc()), 1, 1, None, one, one, one, one, None) != 0
    assert lib.naruto_sdfreg_accumulate(C.byref(od), C.byref(desc()), 1, 1, one, one, one, one, one, None, one, None, None) != 0
    assert lib.naruto_sdfreg_init(one, 4, 4, one, None) != 0 and lib.naruto_sdfreg_commit(one, 4, 7, one, one, None) != 0
    g = _lib.NarutoSdfRegGate(max_trans=0.1, min_trace=2.9, min_overlap=0.25)
    assert lib.naruto_sdfreg_verdict(C.byref(desc()), C.byref(_lib.NarutoSdfRegGate(max_trans=-1.0, min_trace=2.9, min_overlap=0.25)), one, one, one, one, None) != 0
    assert lib.naruto_sdfreg_verdict(C.byref(desc()), C.byref(g), one, None, one, one, None) != 0


def test_model_align_is_refused_without_tracking():
    from naruto_amd.slam import CoSLAMNarutoHIP
    import helpers as H
    cfg = H.office_cfg(12)
    with pytest.raises(ValueError, match="track=True"):
        CoSLAMNarutoHIP(cfg, num_frames=4, model_align=True)

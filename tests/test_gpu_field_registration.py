"""Frame-to-model alignment on the device (naruto_amd/registration.py, csrc/naruto_sdfreg.hip) against its numpy twin
(tests/field_registration_spec.py), the CPU oracle, and through the tracked run with model_align=True.

1. points  2. accumulate  3. the chain on a real field  4. against the oracle  5. iteration by iteration  6. a finished level writes nothing
7. align_device repeats  8. end to end on the mapped room  9. the unmapped view  10. the run  11. refusals and the command line

The room, its config, the camera and the stop-and-go trajectory are tests/test_gpu_odometry.py's.

Run: timeout -k 10 900 python -m pytest tests/test_gpu_field_registration.py -m gpu -q -s
"""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch
import yaml

import cull_spec as CS
import field_registration_spec as FS
import odometry_spec as OS
import test_gpu_odometry as TO

pytestmark = pytest.mark.gpu

COUNTS = [1, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 1]
BOX_LO, BOX_HI = (-1.0, -2.0, -3.5), (1.0, 1.0, -0.5)
SMALL = CS.camera(40, 30, 30.0)


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _descs(n, lo=BOX_LO, hi=BOX_HI, trunc=0.1, sdf_gate=0.9):
    """A one-level pyramid of 1 x n pixels and the registration over it: the C ABI's two structs."""
    from naruto_amd import _lib
    od = _lib.NarutoOdomDesc(H=1, W=n, levels=1, iters=(C.c_uint32 * 4)(1, 0, 0, 0), fx=float(n), fy=float(n), cx=0.0, cy=0.0, max_dist=0.25, jump=0.15, band=0.1)
    reg = _lib.NarutoSdfRegDesc(trunc=trunc, sdf_gate=sdf_gate, bbox_min=(C.c_float * 3)(*lo), bbox_max=(C.c_float * 3)(*hi), n_levels=1,
                                levels=(C.c_uint32 * 4)(0, 0, 0, 0), iters=(C.c_uint32 * 4)(1, 0, 0, 0))
    return od, reg


def _state(gpu, T, done=0.0):
    s = torch.zeros(64, dtype=torch.float64, device=gpu)
    s[:16] = torch.from_numpy(np.asarray(T, np.float64).reshape(16).copy()).to(gpu)
    s[16] = done
    return s


# --------------------------------------------------------------------------------------------- 1. points
def _vertices(n, rs):
    """Camera-frame vertices around the box: inside, outside, missing (0,0,0), behind the camera; with T = identity q = p exactly, so the
    first ones sit exactly on each face of the box and one float32 step outside it."""
    lo, hi = np.asarray(BOX_LO, np.float32), np.asarray(BOX_HI, np.float32)
    v = (lo + (hi - lo) * rs.uniform(-0.15, 1.15, (n, 3))).astype(np.float32)
    mid, k = ((lo + hi) / np.float32(2)).astype(np.float32), 0
    for a in range(3):
        for face, away in ((lo[a], -np.inf), (hi[a], np.inf)):
            for val in (face, np.nextafter(face, np.float32(away))):
                if k < n:
                    v[k] = mid
                    v[k, a] = val
                    k += 1
    for j in range(k, n, 7):
        v[j] = 0.0                                                          # a missing vertex
    for j in range(k + 3, n, 11):
        v[j, 2] = abs(v[j, 2])                                              # behind the camera
    return v


@pytest.mark.parametrize("n", COUNTS)
def test_points_equal_the_twin_in_every_bit(gpu, n):
    from naruto_amd import _lib
    lib, rs = _lib.load(), np.random.RandomState(n)
    od, reg = _descs(n)
    v = _vertices(n, rs)
    maps = torch.zeros(7 * n, dtype=torch.float32, device=gpu)
    maps[n:4 * n] = torch.from_numpy(v.reshape(-1)).to(gpu)
    general = np.eye(4)
    general[:3, :3] = OS.rotation((0.3, -0.8, 0.5), 0.05)
    general[:3, 3] = (0.02, -0.03, 0.01)
    bad = general.copy()
    bad[1, 2] = np.nan
    for name, T in (("identity", np.eye(4)), ("general", general), ("a NaN in T", bad)):
        x = torch.full((n, 3), 7.0, device=gpu)
        q = torch.full((n, 3), 7.0, device=gpu)
        valid = torch.full((n,), 9, dtype=torch.uint8, device=gpu)
        rc = lib.naruto_sdfreg_points(C.byref(od), C.byref(reg), 0, 1, maps.data_ptr(), _state(gpu, T).data_ptr(), x.data_ptr(), q.data_ptr(), valid.data_ptr(), None)
        assert rc == 0, lib.naruto_last_error()
        torch.cuda.synchronize()
        wx, wq, wv = FS.points(T, v, BOX_LO, BOX_HI)
        assert np.array_equal(valid.cpu().numpy(), wv.astype(np.uint8)), (name, "valid")
        assert np.array_equal(_b32(x.cpu().numpy()), _b32(wx)), (name, "x")
        gq = q.cpu().numpy()
        assert np.array_equal(np.isnan(gq), np.isnan(wq)) and np.array_equal(_b32(np.nan_to_num(gq)), _b32(np.nan_to_num(wq))), (name, "q")
        if name == "identity" and n >= 255:
            # x decides: one float32 step beyond a low face is a negative x; beyond a high face (q - lo) / extent may still round to 1
            assert wv[0:12:2].all() and not wv[1:12:4].any(), "on a face is inside, one step below a low face is outside"
            assert 0 < wv.sum() < n
        if name == "a NaN in T":
            assert not wv.any() and (wx == 0.5).all()


# --------------------------------------------------------------------------------------------- 2. accumulate
def _synthetic(n, rs, kind):
    gate32 = np.float32(0.9)
    sdf = rs.uniform(-1.0, 1.0, n).astype(np.float32)
    d_x = (rs.standard_normal((n, 3)) * 20.0).astype(np.float32)
    q = rs.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    valid = (rs.uniform(size=n) < 0.8).astype(np.uint8)
    edge = [gate32, np.nextafter(gate32, np.float32(0)), np.nextafter(gate32, np.float32(2)), -gate32, np.nextafter(-gate32, np.float32(0)),
            np.nextafter(-gate32, np.float32(-2))]
    for k, val in enumerate(edge):
        if k < n:
            sdf[k], valid[k] = val, 1
    for j in range(6, n, 13):
        d_x[j] = 0.0
    for j, val in zip(range(7, n, 29), [np.nan, np.inf, -np.inf] * n):
        sdf[j] = val
    for j, val in zip(range(8, n, 31), [np.nan, np.inf, -np.inf] * n):
        d_x[j, j % 3] = val
    if kind == "all rejected":
        sdf[:] = np.float32(1.0)
    return sdf, d_x, q, valid


def _accumulate(gpu, n, sdf, d_x, q, valid, rows=True, state=None, gated=0):
    from naruto_amd import _lib
    lib = _lib.load()
    od, reg = _descs(n)
    su = torch.from_numpy(np.stack([sdf, np.full_like(sdf, 3.0)], -1)).to(gpu).contiguous()
    t = [su, torch.from_numpy(d_x).to(gpu), torch.from_numpy(q).to(gpu), torch.from_numpy(valid).to(gpu)]
    sums = torch.full((30,), 5.0, dtype=torch.float64, device=gpu)
    ws = torch.empty(lib.naruto_sdfreg_workspace_bytes(C.byref(od)) // 8, dtype=torch.float64, device=gpu)
    rw = torch.full((n, 2), 7.0, dtype=torch.float64, device=gpu) if rows else None
    state = _state(gpu, np.eye(4)) if state is None else state
    rc = lib.naruto_sdfreg_accumulate(C.byref(od), C.byref(reg), 0, gated, *(a.data_ptr() for a in t), state.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                      None if rw is None else rw.data_ptr(), None)
    assert rc == 0, lib.naruto_last_error()
    torch.cuda.synchronize()
    return sums.cpu().numpy(), None if rw is None else rw.cpu().numpy()


@pytest.mark.parametrize("n", COUNTS)
def test_accumulate_equals_the_twin_in_every_bit(gpu, n):
    assert -(-n // 2048) == {1: 1, 255: 1, 256: 1, 257: 1, 2047: 1, 2048: 1, 2049: 2, 4097: 3}[n]
    for kind in ("mixed", "all rejected"):
        sdf, d_x, q, valid = _synthetic(n, np.random.RandomState(100 + n), kind)
        sums, rows = _accumulate(gpu, n, sdf, d_x, q, valid)
        want, wrows = FS.accumulate(sdf, d_x, q, valid, 0.1, BOX_LO, BOX_HI)
        assert np.array_equal(_b64(rows), _b64(wrows)), (kind, "rows")
        assert np.array_equal(_b64(sums), _b64(want)), (kind, np.abs(sums - want).max())
        assert np.isfinite(sums).all() and sums[29] == valid.sum() and sums[28] == wrows[:, 0].sum()
        again, _ = _accumulate(gpu, n, sdf, d_x, q, valid, rows=False)
        assert np.array_equal(_b64(again), _b64(sums)), "two runs, and a run without rows, give the same bits"
        if kind == "all rejected":
            assert not sums[:29].any()
        elif n >= 6:
            assert list(wrows[:6, 0]) == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0], "|sdf| at the gate is rejected, one step below it accepted"
            assert n < 255 or sums[28] > 0


# --------------------------------------------------------------------------------------------- the mapped room
def _cfg(cam, mode="fp32"):
    c = TO._cfg()
    c["cam"].update(H=cam["H"], W=cam["W"], fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"])
    c["decoder"]["mlp_precision"] = mode
    return c


VIEW = (OS.CASE_POSITION, CS.ROOM_CENTRE)


def _first_frame(gpu, cam, mode="fp32"):
    """The room's field after first-frame mapping only, with the frame it was mapped from."""
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = _cfg(cam, mode)
    cfg["mapping"].update(n_pixels=0.5)
    cfg["tracking"]["disable"] = True
    slam = CoSLAMNarutoHIP(cfg, voxel_size=0.1, active_ray=False, num_frames=2, seed=3, device=gpu)
    pose = torch.from_numpy(TO._look(*VIEW).astype(np.float32))
    color, depth = TO._sim(gpu, cam).simulate_batch(pose[None])
    slam.online_recon_step(0, color[0], depth[0], pose)
    return slam, cfg, depth[0].contiguous(), pose.double().numpy()


@pytest.fixture(scope="module")
def small(gpu):
    return {mode: _first_frame(gpu, SMALL, mode) for mode in ("fp32", "bf16")}


def _reg(slam, cfg, cam, **kw):
    from naruto_amd.registration import FieldRegistrationHIP
    return FieldRegistrationHIP(slam.model, cfg, cam, **kw)


def _box(reg):
    return np.array(reg.desc.bbox_min[:], np.float32), np.array(reg.desc.bbox_max[:], np.float32)


def _device_field(reg, level):
    """The field as the twin's callable, answered by the device's own query launches at the twin's x."""
    def field(x):
        M = reg.pixels(level)
        assert x.shape == (M, 3)
        reg.x[:M].copy_(torch.from_numpy(x).to(reg.device))
        reg.query(level)
        torch.cuda.synchronize()
        return reg.sdf_uncert[:M, 0].cpu().numpy().copy(), reg.d_x[:M].cpu().numpy().copy()
    return field


START = FS.perturb(TO._look(*VIEW), 0.03, FS.START_ALONG, 1.5, FS.START_AXIS).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------------------- 3. the chain on a real field
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_evaluate_equals_the_twin_fed_with_the_devices_field(gpu, small, mode):
    slam, cfg, depth, _ = small[mode]
    reg = _reg(slam, cfg, SMALL)
    assert reg.levels == (2, 1) and reg.iters == (6, 6)
    maps = reg.frame_maps(depth)
    lo, hi = _box(reg)
    for level in (2, 1, 0) if mode == "fp32" else (1,):
        if level == 0:
            reg = _reg(slam, cfg, SMALL, levels=(1, 0), iters=(2, 2))
        M = reg.pixels(level)
        sums, rows = reg.evaluate(maps, START, level)
        verts = reg.pyramid.level_views(maps, level)[1].reshape(-1, 3).cpu().numpy()
        x, q, valid = FS.points(START, verts, lo, hi)
        assert np.array_equal(_b32(reg.x[:M].cpu().numpy()), _b32(x)) and np.array_equal(reg.valid[:M].cpu().numpy() != 0, valid)
        sdf, d_x = reg.sdf_uncert[:M, 0].cpu().numpy(), reg.d_x[:M].cpu().numpy()
        with torch.no_grad():
            ref = slam.model.query_sdf(reg.x[:M].clone(), return_uncert=True)
        assert torch.equal(ref.view(torch.int32), reg.sdf_uncert[:M].view(torch.int32)), "the chain's sdf is query_sdf's"
        want, wrows = FS.accumulate(sdf, d_x, q, valid, cfg["training"]["trunc"], lo, hi)
        assert np.array_equal(_b64(rows), _b64(wrows)) and np.array_equal(_b64(sums), _b64(want)), (mode, level, np.abs(sums - want).max())
        print(f"{mode} level {level}: {int(sums[28])} rows of {int(sums[29])} valid points, rmse {math.sqrt(sums[27] / max(sums[28], 1.0)) * 1e3:.3f} mm")
        assert sums[29] == valid.sum() and sums[28] > 0, (mode, level, sums[28:])


# --------------------------------------------------------------------------------------------- 4. against the oracle
def test_the_sums_agree_with_the_oracles_field_within_the_parity_budget(gpu, small):
    """The project asserts outputs and gradients within 1e-4 x max of the oracle; FS.sum_bounds carries that budget through each sum."""
    from oracle import spec_torch as S
    slam, cfg, depth, _ = small["fp32"]
    reg = _reg(slam, cfg, SMALL)
    level, lo, hi = 1, *_box(reg)
    M = reg.pixels(level)
    sums, _ = reg.evaluate(reg.frame_maps(depth), START, level)
    x, q, valid = reg.x[:M].cpu(), reg.q[:M].cpu().numpy(), reg.valid[:M].cpu().numpy()
    ora = S.OracleField(cfg, slam.bounding_box.cpu(), 0.1)
    m = slam.model
    with torch.no_grad():
        for dst, src in ((ora.table, m.embed_fn.params), (ora.sdf_w0, m.decoder.sdf_net.model[0].weight), (ora.sdf_w1, m.decoder.sdf_net.model[2].weight),
                         (ora.col_w0, m.decoder.color_net.model[0].weight), (ora.col_w1, m.decoder.color_net.model[2].weight), (ora.uncert_grid, m.uncert_grid)):
            dst.copy_(src.detach().cpu().reshape(dst.shape))
    xo = x.clone().requires_grad_(True)
    so = ora.query_sdf(xo)
    go, = torch.autograd.grad(so.sum(), xo)
    so, go = so.detach().numpy().astype(np.float32), go.numpy().astype(np.float32)
    d_sdf, d_grad = 1e-4 * float(np.abs(so).max()), 1e-4 * float(np.abs(go).max())
    print(f"device against oracle: sdf {np.abs(reg.sdf_uncert[:M, 0].cpu().numpy() - so).max():.3e} (budget {d_sdf:.3e}), "
          f"gradient {np.abs(reg.d_x[:M].cpu().numpy() - go).max():.3e} (budget {d_grad:.3e})")
    trunc = cfg["training"]["trunc"]
    want, _ = FS.accumulate(so, go, q, valid, trunc, lo, hi)
    bound = FS.sum_bounds(so, go, q, valid, trunc, lo, hi, d_sdf, d_grad)
    err = np.abs(sums[:29] - want[:29])
    print("worst sum error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound + 1e-12 * np.abs(want[:29])).all(), (err, bound)
    assert want[28] > 0 and sums[29] == want[29]


# --------------------------------------------------------------------------------------------- 5. iteration by iteration
def test_iteration_by_iteration_against_the_twin(gpu, small):
    slam, cfg, depth, _ = small["fp32"]
    reg = _reg(slam, cfg, SMALL)
    maps, (lo, hi), trunc = reg.frame_maps(depth), _box(reg), cfg["training"]["trunc"]
    est = torch.from_numpy(START.astype(np.float32))[None].to(gpu).contiguous()
    reg.init(est, 0)
    torch.cuda.synchronize()
    assert np.array_equal(reg.state.cpu().numpy()[:16], START.reshape(16)) and np.array_equal(reg.state.cpu().numpy()[48:], START.reshape(16))
    T, steps = START.copy(), 0
    for level, cap in zip(reg.levels, reg.iters):
        verts = reg.pyramid.level_views(maps, level)[1].reshape(-1, 3).cpu().numpy()
        upd, done = 0, False
        for _ in range(cap):
            before = reg.state.clone()
            reg.iterate(maps, level)
            torch.cuda.synchronize()
            if done:
                assert torch.equal(before.view(torch.int64), reg.state.view(torch.int64))
                continue
            Td = before[:16].cpu().numpy().reshape(4, 4)                    # the twin steps from the device's T: one step's error, not a chain's
            sums, _ = FS.evaluate(Td, verts, _device_field(reg, level), trunc, lo, hi)
            assert np.array_equal(_b64(reg.sums.cpu().numpy()), _b64(sums))
            T, done, status, upd, inl, rmse = OS.step(sums[:29], Td, upd, cap)
            got = reg.state.cpu().numpy()
            w = got[16 + 8 * level:24 + 8 * level]
            assert (w[0] != 0) == done and int(w[1]) == status and int(w[2]) == upd and w[3] == inl
            if status != OS.DEGENERATE:
                assert np.abs(got[:16].reshape(4, 4) - T).max() <= TO._step_bound(sums, Td), (level, upd)
                steps += 1
    assert steps >= 1, "the case has steps that move T"


# --------------------------------------------------------------------------------------------- 6. a finished level writes nothing
def test_launches_of_a_finished_level_write_nothing(gpu, small):
    slam, cfg, depth, _ = small["fp32"]
    reg = _reg(slam, cfg, SMALL)
    maps = reg.frame_maps(depth)
    est = torch.from_numpy(START.astype(np.float32))[None].to(gpu).contiguous()
    reg.init(est, 0)
    reg.state[16 + 8 * 1] = 1.0                                            # level 1 is done
    for t in (reg.x, reg.q, reg.sums, reg.workspace):
        t.fill_(3.0)
    reg.valid.fill_(9)
    keep = [t.clone() for t in (reg.x, reg.q, reg.valid, reg.sums, reg.workspace, reg.state)]
    reg.points(maps, 1)
    reg.accumulate(1)
    reg.pyramid.step(1, reg.state)
    torch.cuda.synchronize()
    for a, b in zip(keep, (reg.x, reg.q, reg.valid, reg.sums, reg.workspace, reg.state)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    reg.points(maps, 1, gated=False)                                       # the ungated form runs whatever the word says
    torch.cuda.synchronize()
    assert not torch.equal(keep[0], reg.x)
    # the synthetic form too: a gated accumulate over a done word leaves the sums as they were
    n = 300
    sdf, d_x, q, valid = _synthetic(n, np.random.RandomState(1), "mixed")
    sums, rows = _accumulate(gpu, n, sdf, d_x, q, valid, state=_state(gpu, np.eye(4), done=1.0), gated=1)
    assert (sums == 5.0).all() and (rows == 7.0).all()


# --------------------------------------------------------------------------------------------- 7. align_device repeats
def test_align_device_repeats_bit_for_bit(gpu, small):
    slam, cfg, depth, true = small["fp32"]
    reg = _reg(slam, cfg, SMALL)
    maps, out = reg.frame_maps(depth), []
    for _ in range(2):
        est = torch.zeros(3, 4, 4, device=gpu)
        est[1] = torch.from_numpy(START.astype(np.float32)).to(gpu)
        pose6, record = torch.zeros(6, device=gpu), torch.zeros(8, dtype=torch.float64, device=gpu)
        state = reg.align_device(maps, est, 1, pose6, record).clone()
        out.append((est.cpu(), pose6.cpu(), record.cpu(), state.cpu()))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    est, pose6, record, state = out[0]
    from naruto_amd import pose_chain as PC
    assert not est[0].any() and not est[2].any()
    assert torch.equal(pose6.view(torch.int32), PC.pose_log(est[1:2].to(gpu))[0].cpu().view(torch.int32)), "pose6 is the log of the stored matrix"
    want = state[:16].numpy().astype(np.float32).reshape(4, 4)
    assert np.array_equal(_b32(est[1].numpy()), _b32(want)), "est[i] is T rounded once"
    tw_est, tw_p6 = FS.commit(state[:16].numpy())
    assert np.array_equal(_b32(tw_est), _b32(est[1].numpy())) and np.abs(tw_p6 - pose6.numpy()).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(tw_p6).max())
    print("align_device at 40 x 30 after first-frame mapping: record", record.numpy(), "errors", FS.pose_error(state[:16].numpy().reshape(4, 4), true),
          "start", FS.pose_error(START, true))


# --------------------------------------------------------------------------------------------- the runs and the mapped room
def _run(gpu, **kw):
    return TO._run(gpu, **kw)


N_MAPPED, I_TRUE = 11, 8


@pytest.fixture(scope="module")
def mapped(gpu):
    """The stop-and-go scene's field after its first keyframes (frames 0, 5, 10), mapped FROM THE TRUE POSES (no tracking): a true pose is then
    the pose the map itself is registered to, which is what 'the rmse at the true pose' compares against.  Returns the slam object, its
    camera, and frame I_TRUE's true pose and depth (a frame between two keyframes)."""
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = TO._cfg()
    cfg["tracking"]["disable"] = True
    slam = CoSLAMNarutoHIP(cfg, voxel_size=0.1, active_ray=False, num_frames=N_MAPPED, seed=3, device=gpu)
    cam = {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
    traj = TO._stop_and_go(N_MAPPED)
    color, depth = TO._sim(gpu, cam).simulate_batch(traj)
    for i in range(N_MAPPED):
        slam.online_recon_step(i, color[i], depth[i], traj[i])
    return slam, cam, traj[I_TRUE].double().numpy(), depth[I_TRUE].contiguous()


@pytest.fixture(scope="module")
def runs(gpu):
    return {"aligned": _run(gpu, raising=True, motion_prior="depth_icp", model_align=True), "plain": _run(gpu, motion_prior="depth_icp", model_align=None)}


# --------------------------------------------------------------------------------------------- 8. end to end on the mapped room
PERTURBATIONS = ((0.01, 0.5), (0.03, 1.5), (0.05, 2.0))


def test_alignment_on_the_mapped_room(gpu, mapped):
    """Measured on an MI355X (first run of this test; DESIGN 7n keeps the table): rmse at the true pose 8.864 mm over 3673 rows.  From 1 cm /
    0.5 deg, 3 cm / 1.5 deg and 5 cm / 2 deg the alignment ends 3.77 mm / 0.126 deg, 3.79 mm / 0.127 deg and 3.79 mm / 0.127 deg from the true
    pose with a final rmse of 9.299, 9.300 and 9.300 mm over 4343 rows, against the bound 1.05 x 8.864 = 9.307 mm: met by 0.1 %.  The room's
    walls are the faces of the field's bounding box, so a tenth of the wall points enter or leave the valid set between the two poses."""
    slam, cam, true, depth = mapped
    reg = _reg(slam, slam.config, cam)
    maps = reg.frame_maps(depth)
    finest = reg.levels[-1]
    s_true, _ = reg.evaluate(maps, true, finest)
    rmse_true = math.sqrt(s_true[27] / s_true[28])
    print(f"rmse at the true pose {rmse_true * 1e3:.3f} mm over {int(s_true[28])} rows of {int(s_true[29])} valid points")
    for metres, deg in PERTURBATIONS:
        start = FS.perturb(true, metres, FS.START_ALONG, deg, FS.START_AXIS).astype(np.float32).astype(np.float64)
        out = reg.align(maps, start)
        e0, e1 = FS.pose_error(start, true), FS.pose_error(out.T, true)
        print(f"start {metres * 100:.0f} cm / {deg} deg: {e0[0] * 1e3:.2f} mm {e0[1]:.3f} deg -> {e1[0] * 1e3:.2f} mm {e1[1]:.3f} deg; "
              f"record {np.array2string(out.record, precision=5)}; status {out.status} iterations {out.iterations}")
        assert out.passed and out.record[0] == 1.0, (metres, deg, out.record)
        assert e1[0] < e0[0] and e1[1] < e0[1], (metres, deg, e0, e1)
        assert out.record[4] <= 1.05 * rmse_true, (metres, deg, out.record[4], rmse_true)


# --------------------------------------------------------------------------------------------- 9. the unmapped view
def test_a_lost_start_or_an_unmapped_view_is_refused(gpu, mapped):
    slam, cam, true, depth = mapped
    reg = _reg(slam, slam.config, cam)
    maps = reg.frame_maps(depth)
    far = FS.perturb(true, 0.5, (0.62, 0.55, -0.56), 0.0, None).astype(np.float32)
    outside = true.astype(np.float32).copy()
    outside[:3, 3] += np.float32(40.0)                                      # every point leaves the field's box: no valid point, no rows
    for name, start in (("0.5 m away", far), ("outside the box", outside)):
        est = torch.zeros(2, 4, 4, device=gpu)
        est[1] = torch.from_numpy(start).to(gpu)
        pose6, record = torch.zeros(6, device=gpu), torch.ones(8, dtype=torch.float64, device=gpu)
        reg.align_device(maps, est, 1, pose6, record)
        rec = record.cpu().numpy()
        print(name, "record", rec)
        assert rec[0] == 0.0 and np.isfinite(rec).all(), (name, rec)
        assert np.array_equal(_b32(est[1].cpu().numpy()), _b32(start)), name
        from naruto_amd import pose_chain as PC
        assert torch.equal(pose6.view(torch.int32), PC.pose_log(est[1:2])[0].view(torch.int32)), name
        if name == "outside the box":
            assert rec[1] == 0.0 and rec[2] == 0.0 and rec[7] == OS.DEGENERATE


# --------------------------------------------------------------------------------------------- 10. the run
def test_the_aligned_run_never_waits_for_the_hosts_log_map_and_repeats(gpu, runs):
    slam, out, traj, _ = runs["aligned"]                                   # ran with the raising replacements of the host's log map
    assert slam.aligner is not None and slam.align_log.shape == (TO.N_RUN, 8) and out["align_log"].shape == (TO.N_RUN, 8)
    log = out["align_log"].numpy()
    assert not log[0].any() and (log[1:, 1] > 0).all(), "frames 1 .. 20 have a record with valid points"
    assert np.isin(log[1:, 0], (0.0, 1.0)).all() and np.isfinite(log).all()
    slam2, again, _, _ = _run(gpu, motion_prior="depth_icp", model_align=True)
    assert torch.equal(again["est_poses"].view(torch.int32), out["est_poses"].view(torch.int32))
    assert torch.equal(again["align_log"].view(torch.int64), out["align_log"].view(torch.int64))
    for (n, p), (_, q) in zip(slam.model.named_parameters(), slam2.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"
    plain = runs["plain"][1]
    # measured on an MI355X (first run): aligned 8.844 mm, without 8.664 mm; 2 of 20 alignments refused; ATE rmse 0.360 cm against 0.609 cm
    print(f"mean translation error after tracking: aligned {TO._mean_err(out) * 1e3:.3f} mm, without {TO._mean_err(plain) * 1e3:.3f} mm; "
          f"{int((log[1:, 0] == 0).sum())} of {TO.N_RUN - 1} alignments refused; ATE aligned {out['ate']}, without {plain['ate']}")


def test_model_align_none_is_todays_run_in_every_bit(gpu, runs):
    slam, plain, _, handed = runs["plain"]
    assert slam.aligner is None and slam.align_log is None and "align_log" not in plain
    slam_t, today, _, handed_t = _run(gpu, motion_prior="depth_icp")       # the object as it is built without the keyword
    assert torch.equal(today["est_poses"].view(torch.int32), plain["est_poses"].view(torch.int32))
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(handed, handed_t))
    for (n, p), (_, q) in zip(slam.model.named_parameters(), slam_t.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"


# --------------------------------------------------------------------------------------------- 11. refusals and the command line
def test_model_align_is_refused_without_tracking(gpu):
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = TO._cfg()
    cfg["tracking"]["disable"] = True
    with pytest.raises(ValueError, match="track=True"):
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=4, device=gpu, model_align=True)
    with pytest.raises(ValueError, match="RegistrationGate"):
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=4, device=gpu, track=True, model_align="yes")


def test_model_align_through_the_command_line(gpu, tmp_path):
    from naruto_amd.mesh import Mesh
    from naruto_amd.run import main
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    Mesh(np.asarray(v, np.float64), np.asarray(f, np.int64)).export(str(tmp_path / "room.ply"))
    cfg = TO._cfg()
    cfg["cam"].update(H=30, W=40, fx=30.0, fy=30.0, cx=19.0, cy=14.0)
    cfg["mapping"].update(n_pixels=0.5)
    with open(tmp_path / "cfg.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    out = main(["--config", str(tmp_path / "cfg.yaml"), "--mesh", str(tmp_path / "room.ply"), "--result_dir", str(tmp_path / "aligned"), "--num_iter", "12",
                "--start", "2.0", "4.0", "1.2", "--no_active_ray", "--seed", "5", "--track", "--model_align", "--planner", "gs_z_levels=[12]", "max_rot_deg=30",
                "rrt_max_iter=2000"])
    assert out["est_poses"].shape == (12, 4, 4) and bool(torch.isfinite(out["est_poses"]).all()) and out["align_log"].shape == (12, 8)
    results = dict(line.strip().split(",") for line in open(tmp_path / "aligned" / "results.txt"))
    assert "align_failed_frames" in results and 0 <= int(float(results["align_failed_frames"])) <= 11

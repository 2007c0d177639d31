"""tests/tracking_spec.py, the fp64 twin of the fused camera tracker, pinned on the CPU: its rotation, rays and pose gradient against the
kernels' own host build (naruto_debug_rodrigues) and against fp64 autograd of naruto_amd.tracking.axis_angle_to_matrix; its Adam step
against naruto_debug_pose_adam (pose_adam_step, the code of k_track_step) and torch.optim.Adam; its schedule on hand-written loss lists;
its pixel rule against draw_pixels_host; and the premises of tests/test_gpu_tracking_edges.py's case matrix (launch forms, sample
budget, ReLU-kink rays, depth patterns), which need the oracle but no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import launch_forms as LF
import tracking_spec as TS

THETAS = [0.0, 9.9e-4, 9.9e-3, 1.01e-2, 1e-1, 1.0, 3.1, 3.5]
AXES = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (0.3, -0.8, 0.5), (-0.6, 0.1, 0.2)]


def _omega(theta, axis):
    a = np.asarray(axis, dtype=np.float64)
    return (a / np.linalg.norm(a) * theta).astype(np.float32)          # an fp32 omega, as the device holds it


def _debug_rodrigues(lib, w, G=None):
    wa = (C.c_double * 3)(*[float(x) for x in w])
    Ga = (C.c_double * 9)(*(np.zeros(9) if G is None else np.asarray(G, np.float64).reshape(-1)).tolist())
    Ro, dw = (C.c_double * 9)(), (C.c_double * 3)()
    assert lib.naruto_debug_rodrigues(wa, Ga, Ro, dw) == 0
    return np.array(Ro[:]).reshape(3, 3), np.array(dw[:])


def _ray_data(seed, n=37):
    rs = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32)
    return f(rs.normal(size=(n, 3))), f(rs.normal(size=(n, 3)) * 10.0 ** rs.uniform(-4, 0, (n, 1))), f(rs.normal(size=(n, 3)) * 10.0 ** rs.uniform(-4, 0, (n, 1)))


@pytest.mark.parametrize("theta", THETAS)
def test_rotation_and_rays_match_the_kernels_host_build(built_lib, theta):
    """rotation in fp64 within 1e-15 of naruto_pose.h's rodrigues (both sides of the series threshold theta^2 = 1e-4 included; below it
    within 8 ulp of every entry), the same
    fp32 matrix after the one rounding, and within 1e-12 of naruto_amd.tracking.axis_angle_to_matrix in fp64.  rays_from_pose: rays_o = t,
    rays_d the products rounded to fp32 one by one and added left to right -- restated here in scalar numpy float32 arithmetic."""
    from naruto_amd import tracking as TK
    for k, axis in enumerate(AXES):
        w = _omega(theta, axis)
        R_dev, _ = _debug_rodrigues(built_lib, w)
        w64 = torch.from_numpy(w.astype(np.float64))
        R = TS.rotation(w64).numpy()
        np.testing.assert_allclose(R, R_dev, rtol=0, atol=1e-15)
        if float(w64 @ w64) < TS.SERIES_BELOW:
            # the series branch, entry by entry (the off-diagonal ones are ~theta): a closed form's cancellation (1e-14 of them at
            # theta = 1e-2) or a series cut after two terms (8e-15 at theta = 1e-3) leaves 8 ulp
            np.testing.assert_allclose(R, R_dev, rtol=8 * 2.0 ** -52, atol=0)
        np.testing.assert_allclose(R, TK.axis_angle_to_matrix(w64).numpy(), rtol=0, atol=1e-12)
        pose = np.concatenate([w, np.float32([0.25, -1.5, 3.0])])
        assert np.array_equal(TS.rotation_f32(pose), R_dev.astype(np.float32))
        assert np.array_equal(TS.c2w_f32(pose)[:3, :3], R_dev.astype(np.float32)) and np.array_equal(TS.c2w_f32(pose)[:3, 3], pose[3:])
        assert np.array_equal(TS.c2w_f32(pose)[3], np.float32([0, 0, 0, 1]))
        d_cam = _ray_data(10 * k + 1)[0]
        ro, rd = TS.rays_from_pose(pose, d_cam)
        assert ro.dtype == np.float32 and rd.dtype == np.float32
        assert np.array_equal(ro, np.tile(pose[3:], (d_cam.shape[0], 1)))
        Rf = R_dev.astype(np.float32)
        for r in range(d_cam.shape[0]):
            for i in range(3):
                a = np.float32(d_cam[r, 0] * Rf[i, 0])
                b = np.float32(d_cam[r, 1] * Rf[i, 1])
                c = np.float32(d_cam[r, 2] * Rf[i, 2])
                assert rd[r, i] == np.float32(np.float32(a + b) + c)
        if theta == 0.0:
            assert np.array_equal(rd, d_cam)


@pytest.mark.parametrize("theta", THETAS)
def test_pose_gradient_matches_the_kernels_vjp_and_fp64_autograd(built_lib, theta):
    """pose_gradient's d_omega within 1e-12 of the sum of |terms| of rodrigues_vjp on G = sum d_rays_d (x) d_cam (and 1e-9 relative), its
    d_t the plain sum; from theta = 0.1 up also within the same bound of fp64 autograd through axis_angle_to_matrix (whose closed
    form loses digits below that).  The sum of |terms| dominates the gradient."""
    from naruto_amd import tracking as TK
    for k, axis in enumerate(AXES):
        w = _omega(theta, axis)
        d_cam, dro, drd = _ray_data(10 * k + 2)
        pose = np.concatenate([w, np.float32([0.5, 0.25, -2.0])])
        grad, terms = TS.pose_gradient(pose, d_cam, dro, drd)
        assert bool((np.abs(grad) <= terms * (1 + 1e-12)).all())
        G = drd.astype(np.float64).T @ d_cam.astype(np.float64)
        _, dw = _debug_rodrigues(built_lib, w, G)
        tol = 1e-12 * terms[:3] + 1e-9 * np.abs(dw)
        assert bool((np.abs(grad[:3] - dw) <= tol).all()), (grad[:3], dw)
        np.testing.assert_allclose(grad[3:], dro.astype(np.float64).sum(0), rtol=1e-14, atol=0)
        if theta >= 0.1:
            w64 = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
            t64 = torch.from_numpy(pose[3:].astype(np.float64)).requires_grad_(True)
            rays_d = torch.sum(torch.from_numpy(d_cam).double()[..., None, :] * TK.axis_angle_to_matrix(w64)[None], -1)
            rays_o = t64[None].expand(d_cam.shape[0], 3)
            ((rays_d * torch.from_numpy(drd).double()).sum() + (rays_o * torch.from_numpy(dro).double()).sum()).backward()
            want = torch.cat([w64.grad, t64.grad]).numpy()
            assert bool((np.abs(grad - want) <= 1e-12 * terms + 1e-9 * np.abs(want)).all()), (grad, want)


@pytest.mark.parametrize("start", ["random", "zero"])
def test_adam_step_matches_pose_adam_step_over_20_steps(built_lib, start):
    """20 steps of naruto_debug_pose_adam (fp32 moments, fp64 bias corrections) from a random pose and from the zero pose (where no ulp of
    the component hides an error of the step): after every step the device's pose within 2 ulp of the component + 2 ulp of lr of
    adam_step from the pose before it and the gradients so far -- the edge suite's bound (c).  A pure fp64 torch.optim.Adam fed the same
    gradients from the same start stays within 1e-6 lr per step taken (the twin's moments are rounded to fp32)."""
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    worst = 0.0
    for seed in range(24):
        rs = np.random.RandomState(seed)
        lr_r, lr_t = ((1e-3, 1e-3), (2e-3, 5e-4), (0.3, 0.3))[seed % 3]
        lr = np.array([lr_r] * 3 + [lr_t] * 3)
        p = (rs.normal(size=6) if start == "random" else np.zeros(6)).astype(np.float32)
        m, v = np.zeros(6, np.float32), np.zeros(6, np.float32)
        scale = 10.0 ** rs.uniform(-6, 1)
        pt = torch.from_numpy(p.astype(np.float64))
        wt, tt = pt[:3].clone().requires_grad_(True), pt[3:].clone().requires_grad_(True)
        opt = torch.optim.Adam([{"params": [wt], "lr": lr_r}, {"params": [tt], "lr": lr_t}], betas=TS.BETAS, eps=TS.EPS)
        grads = []
        for step in range(1, 21):
            g = (rs.normal(size=6) * scale * 10.0 ** rs.uniform(-1, 1, 6)).astype(np.float32)
            grads.append(g)
            before = p.copy()
            assert built_lib.naruto_debug_pose_adam(fp(p), fp(g), fp(m), fp(v), step, lr_r, lr_t, 0.9, 0.999, 1e-8) == 0
            want, _ = TS.adam_step(before, np.array(grads), lr_r, lr_t)
            tol = 2 * TS.ulp32(p) + 2 * TS.ulp32(lr)
            err = np.abs(p.astype(np.float64) - want)
            worst = max(worst, float((err / tol).max()))
            assert bool((err <= tol).all()), f"seed {seed} step {step}: {err / tol}"
            wt.grad, tt.grad = torch.from_numpy(g[:3].astype(np.float64)), torch.from_numpy(g[3:].astype(np.float64))
            opt.step()
            if start == "zero" and seed % 3 != 2:
                free = torch.cat([wt, tt]).detach().numpy()
                assert bool((np.abs(p - free) <= 1e-6 * lr * step + 2 * TS.ulp32(p)).all()), (seed, step)
    print(f"adam_step vs pose_adam_step ({start}): worst |error| / (2 ulp p + 2 ulp lr) = {worst:.3f}")


def test_adam_step_uses_each_blocks_learning_rate():
    g = np.full((1, 6), 0.37, np.float32)
    p, _ = TS.adam_step(np.zeros(6, np.float32), g, 2e-3, 5e-4)
    np.testing.assert_allclose(p[:3], -np.float64(np.float32(2e-3)), rtol=1e-6)
    np.testing.assert_allclose(p[3:], -np.float64(np.float32(5e-4)), rtol=1e-6)


def test_schedule_on_hand_written_losses():
    poses = [f"p{i}" for i in range(8)]
    # equal losses: the first is the best, every iteration (the first included) fails `loss < best`
    s = TS.schedule([1.0] * 8, poses, 2, True)
    assert s == {"stopped": True, "n": 3, "best_pose": "p0", "thresh": 3, "result": "p0"}
    assert TS.schedule([1.0] * 8, poses, 2, False)["result"] == "p2"
    s = TS.schedule([1.0] * 4, poses[:4], 100, True)
    assert (s["stopped"], s["n"], s["thresh"], s["result"]) == (False, 4, 4, "p0")
    # an improvement at the last allowed iteration: thresh reaches wait_iters = 2 at iteration 1, iteration 2 improves and resets it
    s = TS.schedule([1.0, 1.5, 0.9, 0.95, 0.97, 0.99, 0.5], poses[:7], 2, True)
    assert s == {"stopped": True, "n": 6, "best_pose": "p2", "thresh": 3, "result": "p2"}
    assert TS.schedule([1.0, 1.5, 0.9, 0.95, 0.97, 0.99, 0.5], poses[:7], 2, False)["result"] == "p5"
    # one iteration later it is too late
    s = TS.schedule([1.0, 1.5, 1.2, 0.9], poses[:4], 2, True)
    assert (s["stopped"], s["n"], s["result"]) == (True, 3, "p0")
    # wait_iters = 0: the first loss fails its own comparison, the call stops at iteration 0 whatever follows
    for best in (True, False):
        s = TS.schedule([1.0, 0.1, 0.01], poses[:3], 0, best)
        assert s == {"stopped": True, "n": 1, "best_pose": "p0", "thresh": 1, "result": "p0"}
    # steady improvement never stops; best: False returns the pose evaluated last
    s = TS.schedule([5.0, 4.0, 3.0], poses[:3], 0 + 1, False)
    assert (s["stopped"], s["n"], s["thresh"], s["best_pose"], s["result"]) == (False, 3, 0, "p2", "p2")


FRAMES = sorted({c["frame"] for c in TS.CASES})


@pytest.mark.parametrize("frame", FRAMES, ids=[f"{f[0]}x{f[1]}_{f[2]}_{f[3]}" for f in FRAMES])
def test_unflatten_matches_the_host_draw(built_lib, frame):
    """Every frame of the edge suite: unflatten of the keyed permutation's values is draw_pixels_host's pixel, pixel for pixel; every pixel
    lies in interior_pixels; drawing n_interior pixels returns the interior exactly once; the interior is what the margins leave."""
    from naruto_amd import tracking as TK
    Hh, Ww, eh, ew = frame
    inside = TS.interior_pixels(*frame)
    n_int = (Hh - 2 * eh) * (Ww - 2 * ew)
    assert len(inside) == n_int
    assert inside == {h * Ww + w for h in range(Hh) for w in range(Ww) if eh <= h < Hh - eh and ew <= w < Ww - ew}
    for n in sorted({1, min(7, n_int), n_int}):
        k = [built_lib.naruto_perm_index(i, n_int, 4242, 3, 4) for i in range(n)]
        pix = TS.unflatten(k, *frame)
        assert pix.tolist() == TK.draw_pixels_host(Hh, Ww, eh, ew, n, 4242, 3).tolist()
        assert set(pix.tolist()) <= inside and len(set(pix.tolist())) == n
        if n == n_int:
            assert sorted(pix.tolist()) == sorted(inside)
    # h fastest: consecutive interior indices walk down a column first
    if Hh - 2 * eh > 1:
        assert int(TS.unflatten(1, *frame) - TS.unflatten(0, *frame)) == Ww
    if Ww - 2 * ew > 1:
        assert int(TS.unflatten(Hh - 2 * eh, *frame) - TS.unflatten(0, *frame)) == 1


def test_the_case_matrix_covers_what_it_claims():
    ids = [c["id"] for c in TS.CASES]
    assert len(set(ids)) == len(ids)
    by = {c["id"]: c for c in TS.CASES}
    assert [by[f"N{n}"]["N"] for n in (1, 3, 255, 256, 257, 513)] == [1, 3, 255, 256, 257, 513]
    assert all(by[f"N{n}"]["frame"] == (24, 32, 2, 3) and (by[f"N{n}"]["nd"], by[f"N{n}"]["nr"]) == (2, 1) for n in (1, 3, 255, 256, 257, 513))
    assert {(c["nd"], c["nr"], c["N"], c["form"]) for c in TS.CASES if c["id"].startswith("S")} == \
        {(3, 2, 5, LF.SHORT), (53, 11, 5, LF.SHORT), (54, 11, 5, LF.WALK), (117, 11, 9, LF.WALK)}
    interior = lambda f: ((f[0] - 2 * f[2]), (f[1] - 2 * f[3]))
    assert by["borders0"]["frame"][2:] == (0, 0)
    assert interior(by["one_row"]["frame"])[0] == 1 and interior(by["one_column"]["frame"])[1] == 1
    assert by["whole_interior"]["N"] == int(np.prod(interior(by["whole_interior"]["frame"])))
    assert interior(by["one_pixel"]["frame"]) == (1, 1) and by["one_pixel"]["N"] == 1
    assert {c["mode"] for c in TS.CASES} == {"fp32", "bf16"} and (TS.WALK, TS.SHORT) == (LF.WALK, LF.SHORT)
    for c in TS.CASES:
        assert c["N"] * (c["nd"] + c["nr"]) * c["iters"] <= 6000, c["id"]
        assert c["device_pose"] or not isinstance(c["pose"], float) or c["pose"] <= 3.14      # track() re-derives omega in [0, pi]


@pytest.mark.parametrize("c", TS.CASES, ids=[c["id"] for c in TS.CASES])
def test_edge_case_premises_hold_on_the_cpu(built_lib, c):
    """What tests/test_gpu_tracking_edges.py assumes of each case, with the oracle alone: the training forward takes the named form
    (naruto_debug_train_plan on a host-only field of the case's MLP mode), the depth pattern is the stated one, the initial pose has
    the stated |omega|, the oracle's loss and gradients at iteration 0 are finite and non-zero, and at most 5 % of the rays (never all)
    have a sample on a ReLU kink -- and none comes within 4e-6 of one at any iteration of the oracle's own run of the call."""
    from naruto_amd import _lib, ops
    cfg = TS.case_cfg(c)
    h = ops.FieldHandle(log2_hashmap_size=12, per_level_scale=1.38, uncert_dims=(4, 5, 6), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1), trunc=0.1,
                        sc_factor=1.0, mlp_mode=c["mode"])
    t = _lib.NarutoTrainStep()
    t.n_rays, t.n_samples_d, t.n_range_d = c["N"], c["nd"], c["nr"]
    plan = LF.train_plan(h.ptr, t)
    assert plan[0] == c["form"] and (c["form"] != LF.WALK or plan[4] == c["tiles"]), (c["id"], plan)
    S_tot = c["nd"] + c["nr"]
    assert (c["form"] == LF.SHORT) == (S_tot <= 64)
    if c["id"].endswith("partial_walk"):
        assert S_tot % 64 != 0
    if c["id"].endswith("exact_walk"):
        assert S_tot % 64 == 0

    ora = H.make_oracle(cfg, 0.25, c["seed"])
    direction, rgb, dep, pose, rand = TS.case_frame(c, cfg)
    assert tuple(rand.shape) == (c["iters"], c["N"], S_tot)
    assert float(dep[dep > 0].min()) > 0.3 and float(dep.max()) < 4.0
    norm = direction.norm(dim=-1)
    assert float(norm.min()) > 0.89 and float(norm.max()) < 1.11
    pix = TS.host_draw(built_lib, c, c["rng_seed"], 0)
    assert set(pix.tolist()) <= TS.interior_pixels(*c["frame"]) and len(set(pix.tolist())) == c["N"]
    if c["one_depth"]:
        dep = TS.keep_one_depth(c, dep, pix)
        assert int((dep > 0).sum()) == 1
    d_cam, col, z = TS.gather(direction, rgb, dep, pix)
    if c["one_depth"]:
        assert int((z > 0).sum()) == 1
    elif c["zero_depth"] > 0:
        frac = float((dep == 0).float().mean())
        assert abs(frac - c["zero_depth"]) < 0.06 and 0 < int((z == 0).sum()) < c["N"], frac
    else:
        assert bool((z > 0).all())
    theta = float(pose[:3].double().norm())
    if c["pose"] == "zero":
        assert theta == 0.0
    elif isinstance(c["pose"], float):
        assert abs(theta - c["pose"]) < 1e-6 * c["pose"]
        assert (theta * theta < TS.SERIES_BELOW) == (c["pose"] < 1e-2)
    if c["pose"] == "outside":
        bb = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float64)
        # |direction| < 1.11 and z <= far: no sample can come back to the box
        assert bool((pose[3:].double() > bb[:, 1] + cfg["cam"]["far"] * 1.11).all())

    ev = TS.oracle_eval(ora, cfg, d_cam, col, z, pose, rand[0])
    assert np.isfinite(ev["loss"]) and bool(torch.isfinite(ev["d_pose"]).all())
    assert float(ev["d_pose"][:3].abs().max()) > 0 and float(ev["d_pose"][3:].abs().max()) > 0
    grad, terms = TS.pose_gradient(pose.numpy(), d_cam.numpy(), ev["d_rays_o"].numpy(), ev["d_rays_d"].numpy())
    # the twin's chain rule against the oracle's own autograd through the fp32 rays (the cast is the identity for autograd)
    assert bool((np.abs(grad - ev["d_pose"].numpy()) <= 1e-12 * terms + 1e-9 * np.abs(grad)).all())
    if c["mode"] != "fp32":
        return                      # the bf16 cases run the checks that do not depend on the MLP precision (c, d, f): no ray is compared
    kinks = TS.kink_rays(ora, cfg, ev)
    assert int(kinks.sum()) <= 0.05 * c["N"] and int(kinks.sum()) < c["N"], f"{c['id']}: {int(kinks.sum())} of {c['N']} rays on a ReLU kink"
    # check b sums every ray: no sample near a kink at any iteration of the oracle's own run of the call (the device's poses differ
    # from these by rounding, so the GPU test asserts the same at the poses it evaluates)
    dist = TS.trajectory_kink_distance(ora, cfg, d_cam, col, z, pose, rand)
    assert dist >= 4e-6, f"{c['id']}: a sample {dist:.2e} from a ReLU kink along the oracle's trajectory: choose another seed"

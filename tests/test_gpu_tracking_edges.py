"""TrackerHIP (naruto_track_draw, naruto_track_rays, naruto_track_backward) against tests/tracking_spec.py at its shape and pose edges.

Fields are oracle fields (helpers.make_oracle + make_hip_from_oracle), frames synthetic tensors, the jitter explicit.  Teacher forcing: for
every evaluated iteration i of the device's trace the oracle is evaluated AT the device's own pose[i], so no trajectory has to stay close:
  a  loss[i] against the oracle's total loss there (1e-5 + 1e-4 relative)
  b  d_pose[i] against oracle autograd (fp64 through R(omega)), helpers.grad_close on the omega block and on the t block
  c  pose[i+1] against tracking_spec.adam_step from pose[i] and the device's own d_pose[0..i]: 2 ulp of the component + 2 ulp of lr
  d  (iter = 1 calls) d_pose[0] against tracking_spec.pose_gradient of the device's own d_cam, d_rays_o, d_rays_d: 2^-23 |want| +
     1e-12 sum |terms| -- a reduction that drops or doubles a ray fails here
  e  (iter = 1 calls) d_rays_o / d_rays_d against oracle autograd w.r.t. the rays (helpers.grad_close over the rays without a sample on a
     ReLU kink: at most 5 % of a case's rays, asserted on the oracle before the device is read)
  f  after the call rays_o / rays_d are tracking_spec.rays_from_pose(pose, d_cam) and c2w the result pose's fp32 matrix, bit for bit
and per call: the drawn pixels (the keyed permutation through tracking_spec.unflatten) with the frame's values at them, the schedule
(tracking_spec.schedule over the device's own losses), the state words and the random word's advance.  The case matrix is
tracking_spec.CASES (its premises are checked on the CPU by tests/test_tracking_spec_host.py); the bf16 MLP cases run c, d and f, which
do not depend on the MLP precision.  "outside_the_box" puts every sample outside the scene box: the hash grid wraps there, so the
gradients are of ordinary size and must match like any other.

Check b sums every ray, so it needs a batch in which no sample's ReLU mask is rounding noise: the seeds keep the oracle's own trajectory
4e-6 away from every kink (asserted on the CPU), and the same is asserted here, on the oracle alone, at each pose the device evaluated.

What this suite found: k_track_rays / k_track_step formed rays_d with two fused multiply-adds (the clang HIP headers define __fmul_rn /
__fadd_rn as the plain operators and hipcc contracts them), not the three rounded products added left to right that the kernel's comment
and coslam.py:343 state; check f failed in the first case (N1).  track_write_ray now switches contraction off.

Worst |error| over the matrix next to its bound, measured on an MI355X (``pytest -s`` prints every case and this table):
  a  loss                 7.2e-07   bound 1.3e-04   (omega3.5)
  b  d_omega              2.3e-05   bound 5.6e-05   (whole_interior);   d_t  2.2e-06, bound 9.4e-06 (N255)
  c  Adam step            4.9e-08   bound 8.9e-08   (wait1_diverging_last, lr 0.3); 0.25 of the bound at lr 1e-3
  d  pose gradient        0         every component is the rounded fp64 sum, bit for bit
  e  d_rays_d             7.9e-06   bound 3.9e-05   (whole_interior);   d_rays_o  2.8e-07, bound 1.6e-06 (N513)
  f  rays_o, rays_d, c2w  0         (bit for bit, after the fix above)
"""
import copy

import numpy as np
import pytest
import torch

import helpers as H
import launch_forms as LF
import tracking_spec as TS
from naruto_amd import tracking as TK

pytestmark = pytest.mark.gpu

WORST = {}                  # check -> (|error| / bound, |error|, bound, case): the worst seen by this session's tests


def _note(check, err, bound, cid):
    """Record max |error| / bound of one comparison (arrays); returns the ratio."""
    err, bound = np.asarray(err, np.float64).reshape(-1), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err)).reshape(-1)
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    k = int(np.argmax(r)) if r.size else 0
    ratio = float(r[k]) if r.size else 0.0
    if ratio >= WORST.get(check, (-1.0,))[0]:
        WORST[check] = (ratio, float(err[k]) if r.size else 0.0, float(bound[k]) if r.size else 0.0, cid)
    return ratio


def _grad_ratio(got, want):
    """|got - want| / helpers.grad_close's bound (1e-4 of the largest wanted magnitude + 1e-3 relative), element by element."""
    got, want = torch.as_tensor(got).double().cpu().numpy(), torch.as_tensor(want).double().cpu().numpy()
    scale = max(float(np.abs(want).max()), 1e-12)
    return np.abs(got - want), 1e-4 * scale + 1e-3 * np.abs(want)


def _init_matrix(pose):
    out = torch.eye(4, dtype=torch.float64)
    out[:3, :3] = TS.rotation(pose[:3].double())
    out[:3, 3] = pose[3:].double()
    return out


def _setup(c, gpu, lib):
    cfg = TS.case_cfg(c)
    ora = H.make_oracle(cfg, 0.25, c["seed"])
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    direction, rgb, dep, pose, rand = TS.case_frame(c, cfg)
    if c["one_depth"]:
        dep = TS.keep_one_depth(c, dep, TS.host_draw(lib, c, c["rng_seed"], 0))
    return cfg, ora, m, (direction, rgb, dep), pose, rand


def _call(m, cfg, c, frame, pose, rand, gpu, iters):
    """One call of a fresh tracker with ``iters`` iterations -> the tracker and the returned pose (on the CPU)."""
    cfg = copy.deepcopy(cfg)
    cfg["tracking"]["iter"] = iters
    Hh, Ww = c["frame"][:2]
    trk = TK.TrackerHIP(m, cfg, Hh, Ww, rng_seed=c["rng_seed"])
    plan = LF.train_plan(m._handle().ptr, trk.ts.t)
    assert plan[0] == c["form"] and (c["form"] != LF.WALK or plan[4] == c["tiles"]), f"{c['id']}: the plan says {plan}"
    fr = [a.to(gpu) for a in frame]
    rand = rand[:iters].contiguous().to(gpu)
    if c["device_pose"]:
        trk.pose_init.copy_(pose)
        c2w = trk.track_device(*fr, rand=rand).clone()
        assert torch.equal(trk.pose_init.cpu(), pose)
    else:
        c2w = trk.track(*fr, _init_matrix(pose), rand=rand)
    torch.cuda.synchronize()
    return trk, c2w.cpu()


def _check_call(c, cfg, ora, lib, trk, c2w, frame, rand, iters):
    """Everything but d and e, for one call of ``iters`` iterations.  -> the oracle's evaluation at iteration 0."""
    cid, tk = c["id"], cfg["tracking"]
    fp32 = c["mode"] == "fp32"
    th = trk.last_trace()
    n = th["n_iter"]
    pose0 = trk.pose_init.cpu()
    if c["pose"] == "zero":
        assert torch.equal(pose0[:3], torch.zeros(3)), "the identity rotation must give omega = 0 exactly"
    elif isinstance(c["pose"], float):
        assert abs(float(pose0[:3].double().norm()) - c["pose"]) < 1e-5
    # the draw, and the random word: with explicit jitter only k_track_rays advances the counter
    pix = trk.drawn_pixels().cpu()
    assert torch.equal(pix, TS.host_draw(lib, c, c["rng_seed"], 0)), f"{cid}: not the keyed permutation's pixels, h fastest"
    assert set(pix.tolist()) <= TS.interior_pixels(*c["frame"]) and len(set(pix.tolist())) == c["N"]
    if c["N"] == len(TS.interior_pixels(*c["frame"])):
        assert sorted(pix.tolist()) == sorted(TS.interior_pixels(*c["frame"]))
    assert trk.rng.cpu().tolist() == [c["rng_seed"], 1], f"{cid}: the random word after the call is {trk.rng.cpu().tolist()}"
    d_cam, rgb, dep = TS.gather(*frame, pix)
    assert torch.equal(trk.d_cam.cpu(), d_cam) and torch.equal(trk.target_rgb.cpu(), rgb) and torch.equal(trk.target_d.cpu(), dep), \
        f"{cid}: d_cam / target_rgb / target_d are not the frame's values at the drawn pixels"
    # the schedule over the device's own losses
    assert torch.equal(th["pose"][0], pose0)
    want = TS.schedule(th["loss"].tolist(), th["pose"], tk["wait_iters"], tk["best"])
    assert (th["stopped"], th["thresh"]) == (want["stopped"], want["thresh"]) and n == want["n"], (cid, th["stopped"], th["thresh"], n, want)
    assert n == iters or th["stopped"]
    steps = n - 1 if th["stopped"] else n
    assert trk.state.cpu().tolist() == [steps, want["thresh"], int(want["stopped"]), iters], (cid, trk.state.cpu().tolist())
    assert torch.equal(th["best_pose"], want["best_pose"]) and th["best_loss"] == min(th["loss"].tolist())
    if tk["wait_iters"] == 0:
        assert trk.state.cpu().tolist() == [0, 1, 1, iters] and torch.equal(trk.pose.cpu(), pose0)
        assert np.array_equal(c2w.numpy(), TS.c2w_f32(pose0.numpy())), "wait_iters = 0: the result is the initial pose's fp32 matrix"
    # a, b, c: teacher forcing
    lr = np.array([tk["lr_rot"]] * 3 + [tk["lr_trans"]] * 3)
    ev0, line = None, []
    poses = torch.cat([th["pose"], trk.pose.cpu()[None]]) if not th["stopped"] else th["pose"]        # the pose after the last step
    for i in range(n):
        if fp32:
            ev = TS.oracle_eval(ora, cfg, d_cam, rgb, dep, th["pose"][i], rand[i])
            ev0 = ev if i == 0 else ev0
            # b's premise, on the oracle alone: d_pose sums every ray, so none may have a sample whose ReLU mask is rounding noise
            dist, n_kink = H.relu_kink_distance(ora, cfg, ev["rays_o"], ev["rays_d"], ev["z_vals"], ev["active"])
            assert n_kink == 0, f"{cid}: premise: at the pose of iteration {i} a sample is {dist:.2e} from a ReLU kink: choose another seed"
            ra = _note("a loss", abs(float(th["loss"][i]) - ev["loss"]), 1e-5 + 1e-4 * abs(ev["loss"]), cid)
            rw = _note("b d_omega", *_grad_ratio(th["d_pose"][i, :3], ev["d_pose"][:3]), cid)
            rt = _note("b d_t", *_grad_ratio(th["d_pose"][i, 3:], ev["d_pose"][3:]), cid)
            line.append(f"it{i} a {ra:.3f} b {rw:.3f}/{rt:.3f}")
            H.assert_close(th["loss"][i:i + 1], torch.tensor([ev["loss"]]), 1e-5, f"{cid}: loss {i}", rel=1e-4)
            H.grad_close(th["d_pose"][i, :3], ev["d_pose"][:3], f"{cid}: d_omega at iteration {i}")
            H.grad_close(th["d_pose"][i, 3:], ev["d_pose"][3:], f"{cid}: d_t at iteration {i}")
        if i + 1 < poses.shape[0]:
            step, _ = TS.adam_step(th["pose"][i].numpy(), th["d_pose"][:i + 1].numpy(), tk["lr_rot"], tk["lr_trans"])
            got = poses[i + 1].numpy()
            err, tol = np.abs(got.astype(np.float64) - step), 2 * TS.ulp32(got) + 2 * TS.ulp32(lr)
            line.append(f"c {_note('c Adam step', err, tol, cid):.3f}")
            assert bool((err <= tol).all()), f"{cid}: pose {i + 1} is not the Adam step from pose {i}: |error| / bound {err / tol}"
    # f: the rays and the result after the call
    ro, rd = TS.rays_from_pose(trk.pose.cpu().numpy(), trk.d_cam.cpu().numpy())
    ok_o, ok_d = np.array_equal(trk.rays_o.cpu().numpy(), ro), np.array_equal(trk.rays_d.cpu().numpy(), rd)
    _note("f rays", np.abs(trk.rays_d.cpu().numpy().astype(np.float64) - rd).max(), 0.0, cid)
    assert ok_o, f"{cid}: rays_o is not t"
    assert ok_d, f"{cid}: rays_d is not fl(fl(fl(dx R0) + fl(dy R1)) + fl(dz R2)) of the pose after the call"
    _note("f c2w", np.abs(c2w.numpy().astype(np.float64) - TS.c2w_f32(want["result"].numpy())).max(), 0.0, cid)
    assert np.array_equal(c2w.numpy(), TS.c2w_f32(want["result"].numpy())), f"{cid}: c2w is not the fp32 matrix of the result pose"
    assert torch.equal(trk.c2w.cpu(), c2w)
    print(f"EDGE {cid} iter={iters} n={n}: " + "; ".join(line))
    return ev0, (d_cam, rgb, dep), th


def _check_iteration0(c, cfg, ora, trk, ev0, th):
    """d and e on a call with iter = 1: the buffers are those of iteration 0."""
    cid = c["id"]
    if c["mode"] == "fp32":
        # e's premise, on the oracle alone
        kinks = TS.kink_rays(ora, cfg, ev0)
        assert int(kinks.sum()) <= 0.05 * c["N"] and int(kinks.sum()) < c["N"], f"{cid}: {int(kinks.sum())} of {c['N']} rays on a ReLU kink"
        keep = ~kinks
    want, terms = TS.pose_gradient(trk.pose_init.cpu().numpy(), trk.d_cam.cpu().numpy(), trk.d_rays_o.cpu().numpy(), trk.d_rays_d.cpu().numpy())
    got = th["d_pose"][0].numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float32).astype(np.float64))
    tol = 2.0 ** -23 * np.abs(want) + 1e-12 * terms
    rd_ = _note("d pose gradient of the rays' gradients", err, tol, cid)
    assert bool((err <= tol).all()), f"{cid}: d_pose[0] is not the sum over the device's own ray gradients: |error| / bound {err / np.maximum(tol, 1e-300)}"
    line = f"d {rd_:.3f}"
    if c["mode"] == "fp32":
        for name, dev, ref in (("d_rays_o", trk.d_rays_o, ev0["d_rays_o"]), ("d_rays_d", trk.d_rays_d, ev0["d_rays_d"])):
            assert float(ref[keep].abs().max()) > 0, f"{cid}: the oracle's {name} is 0: nothing is tested"
            r = _note(f"e {name}", *_grad_ratio(dev.cpu()[keep], ref[keep]), cid)
            line += f" e {name} {r:.3f}"
            H.grad_close(dev.cpu()[keep], ref[keep], f"{cid}: {name} (rays without a ReLU-kink sample)")
    print(f"EDGE {cid} iteration 0: {line} ({c['N'] - int(keep.sum()) if c['mode'] == 'fp32' else 0} kink rays)")


@pytest.mark.parametrize("c", TS.CASES, ids=[c["id"] for c in TS.CASES])
def test_tracker_edges(gpu, built_lib, c):
    """One case of tracking_spec.CASES: a call of the case's iterations (a, b, c, f, draw, schedule, state) and, where that is more than
    one, a second tracker's call with iter = 1 on the same pixels, pose and jitter (the same bits at iteration 0; then d and e)."""
    cfg, ora, m, frame, pose, rand = _setup(c, gpu, built_lib)
    trk, c2w = _call(m, cfg, c, frame, pose, rand, gpu, c["iters"])
    ev0, _, th = _check_call(c, cfg, ora, built_lib, trk, c2w, frame, rand, c["iters"])
    if c["iters"] > 1:
        cfg1 = copy.deepcopy(cfg)
        cfg1["tracking"]["iter"] = 1
        trk1, c2w1 = _call(m, cfg1, c, frame, pose, rand, gpu, 1)
        _, _, th1 = _check_call(c, cfg1, ora, built_lib, trk1, c2w1, frame, rand, 1)
        for k in ("loss", "pose", "d_pose"):
            assert torch.equal(th1[k][0], th[k][0]), f"{c['id']}: iteration 0 of the iter = 1 call differs in {k}"
        trk, th = trk1, th1
    _check_iteration0(c, cfg, ora, trk, ev0, th)


def test_two_calls_on_one_tracker(gpu, built_lib):
    """Device-drawn jitter, wait_iters = 1 and a divergent lr: the first call stops and leaves moments, thresh, the stopped flag and
    best_loss behind.  The second call starts as a fresh tracker does: a new tracker whose random word is set to what the first call left
    gives the same bits (trace, state, moments, best_loss, c2w), and its poses are Adam steps from zero moments (c).  Call k's pixels are
    the host draw at the counter read just before call k; the counter moves by 1 + iter per call (k_track_rays, then each forward); the
    two calls' pixel sets differ."""
    c = dict(next(x for x in TS.CASES if x["id"] == "wait1_diverging_best"), id="two_calls", rng_seed=4321)
    cfg, ora, m, frame, pose, _ = _setup(c, gpu, built_lib)
    fr = [a.to(gpu) for a in frame]
    Hh, Ww = c["frame"][:2]
    iters, tk = c["iters"], cfg["tracking"]

    def snapshot(t):
        torch.cuda.synchronize()
        th = t.last_trace()
        return th, [th[k] for k in ("loss", "pose", "d_pose", "best_pose")] + [a.cpu().clone() for a in (t.state, t.exp_avg, t.exp_avg_sq, t.best_loss, t.c2w,
                                                                                                      t.pose, t.rays_d, t.pix, t.rng)]

    trk = TK.TrackerHIP(m, cfg, Hh, Ww, rng_seed=c["rng_seed"])
    words, pixels, snaps = [], [], []
    for call in range(2):
        words.append(trk.rng.cpu().tolist())
        trk.track(*fr, _init_matrix(pose))
        th, snap = snapshot(trk)
        snaps.append((th, snap))
        pixels.append(trk.drawn_pixels().cpu())
        assert torch.equal(pixels[-1], TS.host_draw(built_lib, c, c["rng_seed"], words[-1][1])), f"call {call}: not the draw at counter {words[-1][1]}"
        assert trk.rng.cpu().tolist() == [c["rng_seed"], words[-1][1] + 1 + iters]
    assert words == [[c["rng_seed"], 0], [c["rng_seed"], 1 + iters]]
    assert set(pixels[0].tolist()) != set(pixels[1].tolist())
    th1 = snaps[0][0]
    assert th1["stopped"] and th1["n_iter"] >= 2 and th1["thresh"] == 2, f"the first call must stop and leave a dirty state: {th1['loss'].tolist()}"
    assert float(snaps[0][1][5].abs().max()) > 0 and float(snaps[0][1][6].abs().max()) > 0 and np.isfinite(float(snaps[0][1][7]))
    fresh = TK.TrackerHIP(m, cfg, Hh, Ww, rng_seed=c["rng_seed"])
    fresh.rng.copy_(torch.tensor(words[1], dtype=torch.int64))
    fresh.track(*fr, _init_matrix(pose))
    _, snap_f = snapshot(fresh)
    for k, (a, b) in enumerate(zip(snaps[1][1], snap_f)):
        assert torch.equal(a, b), f"the second call differs from a fresh tracker's in item {k}"
    th2 = snaps[1][0]
    want = TS.schedule(th2["loss"].tolist(), th2["pose"], tk["wait_iters"], tk["best"])
    assert (th2["stopped"], th2["thresh"], th2["n_iter"]) == (want["stopped"], want["thresh"], want["n"])
    lr = np.array([tk["lr_rot"]] * 3 + [tk["lr_trans"]] * 3)
    assert th2["n_iter"] >= 2
    for i in range(th2["n_iter"] - 1):
        step, _ = TS.adam_step(th2["pose"][i].numpy(), th2["d_pose"][:i + 1].numpy(), tk["lr_rot"], tk["lr_trans"])
        got = th2["pose"][i + 1].numpy()
        err, tol = np.abs(got.astype(np.float64) - step), 2 * TS.ulp32(got) + 2 * TS.ulp32(lr)
        _note("c Adam step", err, tol, c["id"])
        assert bool((err <= tol).all()), f"second call: pose {i + 1} is not an Adam step with fresh moments: {err / tol}"


def test_zz_report_worst_errors(gpu):
    """Prints the worst |error| / bound per check seen by the tests above (run last; asserts only that they ran)."""
    for k in sorted(WORST):
        r, e, b, cid = WORST[k]
        print(f"WORST {k}: |error| / bound {r:.4f} (|error| {e:.3e}, bound {b:.3e}) in {cid}")
    assert all(v[0] <= 1.0 for v in WORST.values())

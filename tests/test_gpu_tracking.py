"""TrackerHIP (naruto_amd.tracking): Co-SLAM tracking_render on the device.  Three naruto_amd.synthetic.AnalyticRoom frames are mapped
with MappingTrainer (as test_gpu_point_grads.py's recovery test does); a full 120 x 160 frame of camera 1 is then tracked from a pose
perturbed by ~1 degree and ~3 cm.  The reference is the contract of naruto_amd/tracking.py restated in torch on the CPU oracle
(oracle/spec_torch.py's field from the mapped parameters, autograd, torch.optim.Adam), on the tracker's own pixels and depth jitter."""
import copy

import numpy as np
import pytest
import torch

import helpers as H
from naruto_amd import synthetic as syn
from naruto_amd import trainer
from naruto_amd import tracking as TK
from tracking_spec import oracle_track as _oracle_track, schedule as _schedule

pytestmark = pytest.mark.gpu

HH, WW, FOC, N_CAM = 120, 160, 120.0, 12


def _oracle_from_hip(cfg, m):
    ora = H.make_oracle(cfg, 0.05, 0)
    with torch.no_grad():
        ora.table.copy_(m.embed_fn.params.detach().cpu())
        ora.sdf_w0.copy_(m.decoder.sdf_net.model[0].weight.detach().cpu())
        ora.sdf_w1.copy_(m.decoder.sdf_net.model[2].weight.detach().cpu())
        ora.col_w0.copy_(m.decoder.color_net.model[0].weight.detach().cpu())
        ora.col_w1.copy_(m.decoder.color_net.model[2].weight.detach().cpu())
        ora.uncert_grid.copy_(m.uncert_grid.detach().cpu())
    for p in ora.parameters():
        p.requires_grad_(False)
    return ora


def _batches(cfg, scene, gpu, n, seed):
    rs = np.random.RandomState(seed)
    frames = [scene.rays(k, N_CAM) for k in (0, 1, 2)]
    keys = ("rays_o", "rays_d", "target_rgb", "target_d")
    pool = {k: np.concatenate([f[k] for f in frames]) for k in keys}
    out = []
    for _ in range(n):
        idx = rs.randint(0, len(pool["target_d"]), 2048)
        out.append(tuple(torch.from_numpy(pool[k][idx]).to(gpu) for k in keys))
    return out


@pytest.fixture(scope="module")
def mapped(gpu):
    cfg = H.office_cfg(16, perturb=1.0)
    scene = syn.AnalyticRoom(cfg["mapping"]["bound"])
    torch.manual_seed(0)
    tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32), gpu, 0.1, fused_adam=True)
    tr.first_frame_mapping(_batches(cfg, scene, gpu, 300, 0))
    torch.cuda.synchronize()
    m = tr.model
    for p in m.parameters():
        p.requires_grad_(False)
    fr = scene.rays(1, N_CAM, H=HH, W=WW, f=FOC)
    pos, R = scene.pose(1, N_CAM)
    frame = (torch.tensor((fr["rays_d"].astype(np.float64) @ R).reshape(HH, WW, 3), dtype=torch.float32, device=gpu),
             torch.from_numpy(fr["target_rgb"].reshape(HH, WW, 3)).to(gpu), torch.from_numpy(fr["target_d"].reshape(HH, WW)).to(gpu))
    true = torch.eye(4, dtype=torch.float64)
    true[:3, :3], true[:3, 3] = torch.from_numpy(R), torch.from_numpy(pos)
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)

    def perturbed(deg, dt):
        p = true.clone()
        p[:3, :3] = TK.axis_angle_to_matrix(axis / axis.norm() * (deg * np.pi / 180.0)) @ true[:3, :3]
        p[:3, 3] += torch.tensor(dt, dtype=torch.float64)
        return p.float()
    return {"cfg": cfg, "model": m, "ora": _oracle_from_hip(cfg, m), "frame": frame, "true": true, "scene": scene,
            "init": perturbed(1.0, [0.02, -0.015, 0.015]), "init2": perturbed(0.7, [-0.01, 0.02, 0.01])}


def _cfg(base, **tk):
    cfg = copy.deepcopy(base)
    cfg["tracking"] = dict(TK.TRACKING_DEFAULTS, **tk)
    return cfg


def _rand(iters, seed, same=False):
    g = torch.Generator().manual_seed(seed)
    if same:
        return torch.rand(1, 1024, 43, generator=g).expand(iters, 1024, 43).contiguous()
    return torch.rand(iters, 1024, 43, generator=g)


def _err(c2w, true):
    """(degrees, metres) between a camera-to-world pose and the true one."""
    c2w = torch.as_tensor(c2w).detach().double().cpu()
    ang = float(TK.matrix_to_axis_angle(c2w[:3, :3].T @ true[:3, :3]).norm()) * 180.0 / np.pi
    return ang, float((c2w[:3, 3] - true[:3, 3]).norm())


def _gathered(trk, frame):
    pix = trk.drawn_pixels()
    return frame[0].reshape(-1, 3)[pix], frame[1].reshape(-1, 3)[pix], frame[2].reshape(-1)[pix]


# --------------------------------------------------------------------------------------------- 1. against the oracle
def test_tracker_matches_the_oracle_restatement(mapped, gpu):
    """100 iterations (lr 1e-3, explicit jitter): the first 5 poses within 2e-5 of the oracle's, the pose gradient at iteration 0 within
    helpers.grad_close of oracle autograd; the returned pose's error at most 1.25x the oracle's (+ 0.02 deg / 2 mm), and the oracle's own
    run recovers the pose.  The drawn pixels are the host mirror's (naruto_perm_index)."""
    cfg = _cfg(mapped["cfg"], iter=100)
    fr, true = mapped["frame"], mapped["true"]
    trk = TK.TrackerHIP(mapped["model"], cfg, HH, WW, rng_seed=11)
    rand = _rand(100, 5)
    c2w = trk.track(*fr, mapped["init"], rand=rand.to(gpu))
    th = trk.last_trace()
    assert torch.equal(trk.drawn_pixels().cpu(), TK.draw_pixels_host(HH, WW, 20, 20, 1024, 11, 0))
    d_cam, rgb, dep = (a.cpu() for a in _gathered(trk, fr))
    o = _oracle_track(mapped["ora"], cfg, d_cam, rgb, dep, trk.pose_init.cpu(), rand)
    assert th["n_iter"] == 100 and not th["stopped"]
    for i in range(5):
        H.assert_close(th["pose"][i], o["poses"][i], 2e-5, f"tracking pose {i}")
    H.assert_close(th["loss"][:5], torch.tensor(o["losses"][:5]), 1e-5, "tracking losses", rel=1e-4)
    H.grad_close(th["d_pose"][0], o["grads"][0], "d_pose at iteration 0")
    e0, eh, eo = _err(mapped["init"], true), _err(c2w, true), _err(TK.pose_matrix(o["result"].double()), true)
    print(f"tracking: start {e0[0]:.3f} deg {100 * e0[1]:.2f} cm; oracle {eo[0]:.3f} deg {100 * eo[1]:.2f} cm; HIP {eh[0]:.3f} deg {100 * eh[1]:.2f} cm")
    assert eo[0] < 0.7 * e0[0] and eo[1] < 0.7 * e0[1], "the oracle's own run does not recover the pose: the schedule is not a test"
    assert eh[0] <= 1.25 * eo[0] + 0.02 and eh[1] <= 1.25 * eo[1] + 0.002, (eh, eo)


def test_tracker_matches_the_modular_route(mapped, gpu):
    """The same iterations through NarutoFieldHIP.forward with (omega, t) leaves and torch Adam (the route of the point-gradient PR):
    poses and losses within the packed-vs-flat forward tolerance (2e-5 of the scale)."""
    cfg = _cfg(mapped["cfg"], iter=8)
    m, fr = mapped["model"], mapped["frame"]
    trk = TK.TrackerHIP(m, cfg, HH, WW, rng_seed=12)
    rand = _rand(8, 6).to(gpu)
    trk.track(*fr, mapped["init"], rand=rand)
    th = trk.last_trace()
    d_cam, rgb, dep = _gathered(trk, fr)
    w = trk.pose_init[:3].clone().requires_grad_(True)
    t = trk.pose_init[3:].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [w], "lr": 1e-3}, {"params": [t], "lr": 1e-3}], betas=(0.9, 0.999), eps=1e-8)
    poses, losses = [], []
    m.train()
    for i in range(8):
        rays_d = torch.sum(d_cam[..., None, :] * TK.axis_angle_to_matrix(w)[None], -1)
        ret = m.forward(t[None].expand(1024, 3), rays_d, rgb, dep[:, None], rand=rand[i])
        loss = trainer.get_loss_from_ret(m, cfg, ret)
        poses.append(torch.cat([w, t]).detach().cpu())
        losses.append(float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    for i in range(8):
        H.assert_close(th["pose"][i], poses[i], 2e-5 * max(1.0, float(poses[i].abs().max())), f"modular pose {i}")
    H.assert_close(th["loss"], torch.tensor(losses), 2e-5 * max(losses), "modular losses")


# --------------------------------------------------------------------------------------------- 3. schedule semantics
@pytest.mark.parametrize("best", [True, False])
def test_best_pose_and_wait_iters_follow_co_slam(mapped, gpu, best):
    """wait_iters = 2.  (a) lr 0 and one jitter for every iteration: the loss never improves, so thresh reaches 3 at iteration 2 and the
    call stops there; later iterations change nothing.  (b) lr_rot 0.3 (divergent): the recorded losses fed to the host restatement give
    the same best pose, thresh, stop and result; best: False returns the pose evaluated last, before the step."""
    fr = mapped["frame"]
    cfg = _cfg(mapped["cfg"], iter=10, wait_iters=2, lr_rot=0.0, lr_trans=0.0, best=best)
    trk = TK.TrackerHIP(mapped["model"], cfg, HH, WW, rng_seed=13)
    c2w = trk.track(*fr, mapped["init"], rand=_rand(10, 7, same=True).to(gpu))
    th = trk.last_trace()
    assert th["stopped"] and th["n_iter"] == 3 and th["thresh"] == 3
    assert int(trk.state[3]) == 10 and int(trk.state[0]) == 2
    assert len(set(th["loss"].tolist())) == 1
    assert torch.equal(th["pose"][2], trk.pose_init.cpu())
    H.assert_close(c2w, TK.pose_matrix(trk.pose_init.cpu().double()), 1e-6, "frozen result")

    cfg = _cfg(mapped["cfg"], iter=10, wait_iters=2, lr_rot=0.3, best=best)
    trk = TK.TrackerHIP(mapped["model"], cfg, HH, WW, rng_seed=14)
    c2w = trk.track(*fr, mapped["init"], rand=_rand(10, 8).to(gpu))
    th = trk.last_trace()
    want = _schedule(th["loss"].tolist(), th["pose"], 2, best)
    assert want["stopped"], f"lr_rot 0.3 did not stop the call: losses {th['loss'].tolist()}"
    assert th["stopped"] == want["stopped"] and th["n_iter"] == want["n"] and th["thresh"] == want["thresh"]
    assert torch.equal(th["best_pose"], want["best_pose"])
    H.assert_close(c2w, TK.pose_matrix(want["result"].double()), 1e-6, "result pose")


def test_divergent_lr_returns_the_initial_pose(mapped, gpu):
    cfg = _cfg(mapped["cfg"], iter=10, lr_rot=1.0)
    trk = TK.TrackerHIP(mapped["model"], cfg, HH, WW, rng_seed=15)
    c2w = trk.track(*mapped["frame"], mapped["init"], rand=_rand(10, 9).to(gpu))
    th = trk.last_trace()
    assert bool((th["loss"][1:] > th["loss"][0]).all()), f"lr_rot 1.0 did not diverge: {th['loss'].tolist()}"
    H.assert_close(c2w, TK.pose_matrix(trk.pose_init.cpu().double()), 1e-6, "initial pose")
    H.assert_close(c2w, mapped["init"], 1e-5, "initial pose (matrix)")


# --------------------------------------------------------------------------------------------- 4. isolation, graphs, bits
def test_tracking_leaves_the_field_alone(mapped, gpu):
    m = mapped["model"]
    snap = [(p.detach().clone(), None if p.grad is None else p.grad.clone()) for p in m.parameters()]
    assert any(g is not None for _, g in snap)
    trk = TK.TrackerHIP(m, _cfg(mapped["cfg"]), HH, WW, rng_seed=16)
    trk.track(*mapped["frame"], mapped["init"])
    torch.cuda.synchronize()
    for p, (v, g) in zip(m.parameters(), snap):
        assert torch.equal(p.detach(), v)
        assert (g is None and p.grad is None) or torch.equal(p.grad, g)


def test_mapping_is_unchanged_by_interleaved_tracking(mapped, gpu):
    cfg = mapped["cfg"]
    batches = _batches(cfg, mapped["scene"], gpu, 12, 1)

    def run(with_tracking):
        torch.manual_seed(1)
        tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32), gpu, 0.1, fused_adam=True)
        trk = TK.TrackerHIP(tr.model, _cfg(cfg, iter=5), HH, WW, rng_seed=17) if with_tracking else None
        for i, b in enumerate(batches):
            tr.step(*b, uncert_step=(i % 5 == 4))
            if trk is not None and i % 4 == 1:
                trk.track(*mapped["frame"], mapped["init"])
        torch.cuda.synchronize()
        return [p.detach().clone() for p in tr.parameters()] + [tr.iter_state.clone()]
    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


def test_graph_replay_equals_eager_and_runs_repeat_bit_for_bit(mapped, gpu):
    """Two consecutive frames (two initial poses) through one captured graph equal two eager calls of a tracker with the same seed, pose
    and trace; a second eager tracker repeats the first bit for bit.  The second call draws other pixels (the random word moved on)."""
    cfg = _cfg(mapped["cfg"], iter=10)
    fr = mapped["frame"]
    out = {}
    for name in ("eager", "again", "graph"):
        trk = TK.TrackerHIP(mapped["model"], cfg, HH, WW, rng_seed=21)
        if name == "graph":
            trk.capture()
        res = []
        for init in (mapped["init"], mapped["init2"]):
            c2w = trk.track(*fr, init)
            torch.cuda.synchronize()
            res.append((c2w.cpu(), trk.last_trace(), trk.drawn_pixels().cpu()))
        out[name] = res
    assert not torch.equal(out["eager"][0][2], out["eager"][1][2])
    for name in ("again", "graph"):
        for (c_a, t_a, p_a), (c_b, t_b, p_b) in zip(out["eager"], out[name]):
            assert torch.equal(c_a, c_b), name
            assert torch.equal(p_a, p_b), name
            for k in ("loss", "pose", "d_pose", "best_pose"):
                assert torch.equal(t_a[k], t_b[k]), (name, k)
    e0, e1 = _err(mapped["init"], mapped["true"]), _err(out["eager"][0][0], mapped["true"])
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)


def test_frame_tensors_are_checked(mapped, gpu):
    trk = TK.TrackerHIP(mapped["model"], _cfg(mapped["cfg"]), HH, WW, rng_seed=22)
    d, c, z = mapped["frame"]
    with pytest.raises(ValueError, match=r"\[120, 160, 3\]"):
        trk.track(d[:, :-1], c, z, mapped["init"])
    with pytest.raises(ValueError, match="float32"):
        trk.track(d, c, z.double(), mapped["init"])
    with pytest.raises(ValueError, match="rand"):
        trk.track(d, c, z, mapped["init"], rand=torch.rand(3, 1024, 43, device=gpu))


# --------------------------------------------------------------------------------------------- 6. bf16 MLP mode
def test_bf16_mode_tracks_close_to_fp32(mapped, gpu):
    """The bf16 MLP mode's forward and cotangents are bf16, its point gradients the exact network's: 40 iterations from the same pose,
    pixels and jitter land within 0.05 deg / 2 mm of the fp32 mode's pose and recover the pose too."""
    cfg = _cfg(mapped["cfg"], iter=40)
    cfg_bf = copy.deepcopy(cfg)
    cfg_bf["decoder"]["mlp_precision"] = "bf16"
    m_bf = H.make_hip_from_oracle(cfg_bf, mapped["ora"], gpu)
    rand = _rand(40, 10).to(gpu)
    c32 = TK.TrackerHIP(mapped["model"], cfg, HH, WW, rng_seed=31).track(*mapped["frame"], mapped["init"], rand=rand)
    cbf = TK.TrackerHIP(m_bf, cfg_bf, HH, WW, rng_seed=31).track(*mapped["frame"], mapped["init"], rand=rand)
    d = _err(cbf, c32.double().cpu())
    e0, e32, ebf = _err(mapped["init"], mapped["true"]), _err(c32, mapped["true"]), _err(cbf, mapped["true"])
    print(f"bf16 vs fp32: {d[0]:.4f} deg {100 * d[1]:.3f} cm; fp32 {e32}, bf16 {ebf}")
    assert d[0] <= 0.05 and d[1] <= 0.002, d
    assert ebf[0] < 0.7 * e0[0] and ebf[1] < 0.7 * e0[1]

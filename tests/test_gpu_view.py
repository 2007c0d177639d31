"""The view renderer on the device (naruto_amd/render.py): rays, surface search, the fused launch against its modular twin, the image
metrics against tests/view_spec.py, checkpoints read back into a field, and the evaluation of a run.  Small shapes only."""
import copy

import numpy as np
import pytest
import torch

import cull_spec as CS
import helpers as H
import view_spec as VS

pytestmark = pytest.mark.gpu

CAM = dict(H=20, W=24, fx=20.0, fy=20.0, cx=11.5, cy=9.5)          # principal point ((W - 1)/2, (H - 1)/2)
NPIX = CAM["H"] * CAM["W"]
YAWS = (0.0, 1.3, 2.9)
FIELD_OUT = ("rgb", "depth", "depth_var", "uncert_map", "acc_map")


def _cfg(**kw):
    cfg = H.office_cfg(12, **kw)
    cfg["cam"].update(CAM)
    return cfg


def _poses(cfg):
    """Three poses at the box centre, yawed about the camera's up axis."""
    out = []
    for a in YAWS:
        p = np.eye(4, dtype=np.float32)
        p[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        p[:3, 3] = np.array(cfg["mapping"]["bound"]).mean(1)
        out.append(p)
    return torch.from_numpy(np.stack(out))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, keys, what):
    bad = []
    for k in keys:
        assert got[k].shape == want[k].shape, f"{what}: {k}"
        differ = _bits(got[k]) != _bits(want[k])
        if bool(differ.any()):
            bad.append(f"{k}: {int(differ.sum())} of {differ.numel()} values differ, by {float((got[k] - want[k]).abs().nan_to_num().max()):.3e} at the most")
    assert not bad, f"{what}: " + "; ".join(bad)


def _field(gpu, **cfg_kw):
    from naruto_amd.render import FieldViewRendererHIP
    mlp = cfg_kw.pop("mlp", "fp32")
    cfg = _cfg(**cfg_kw)
    cfg["decoder"]["mlp_precision"] = mlp
    ora = H.make_oracle(cfg, 0.5, 3).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    return cfg, m, FieldViewRendererHIP(m, cfg)


@pytest.fixture(scope="module")
def scene(gpu):
    """The fp32 field, its renderer, the three poses, their rays and the modular twin's renders (n_coarse 64 and 128), made once."""
    cfg, m, r = _field(gpu)
    poses = _poses(cfg).to(gpu)
    rays = r.rays(poses, 0, 3 * NPIX)
    with torch.no_grad():
        coarse = {nc: r._render_fwd(rays[0], rays[1], None, nc, True) for nc in (64, 128)}
    modular = {nc: r.render(poses, n_coarse=nc, fused=False) for nc in (64, 128)}
    return dict(cfg=cfg, model=m, renderer=r, poses=poses, rays=rays, coarse=coarse, modular=modular)


def test_view_rays_equal_rays_to_world_of_camera_rays(gpu, scene):
    from naruto_amd.active_ray_sampler import rays_to_world
    from naruto_amd.slam import camera_rays
    r = scene["renderer"]
    poses = scene["poses"].clone()
    poses[2] = torch.tensor([[0.36, 0.48, -0.8, 0.7], [-0.8, 0.6, 0.0, -1.1], [0.48, 0.64, 0.6, 0.4], [0, 0, 0, 1]], device=gpu)      # not a yaw
    table = camera_rays(**CAM).reshape(-1, 3).to(gpu)
    assert np.array_equal(table.cpu().numpy(), VS.camera_dirs(**CAM).reshape(-1, 3))
    for p0, p1 in ((31, 1000), (0, 3 * NPIX), (NPIX - 7, NPIX + 5), (700, 701)):      # mid-row starts and ends, two and three poses, one pixel
        g = torch.arange(p0, p1, device=gpu)
        want_o, want_d = rays_to_world(table[g % NPIX], g // NPIX, poses)
        got_o, got_d = r.rays(poses, p0, p1)
        assert torch.equal(_bits(got_o), _bits(want_o)) and torch.equal(_bits(got_d), _bits(want_d)), (p0, p1)
        o, d = VS.view_rays(poses.cpu().numpy(), CAM, p0, p1)
        assert np.array_equal(got_o.cpu().numpy().view(np.int32), o.view(np.int32)) and np.array_equal(got_d.cpu().numpy().view(np.int32), d.view(np.int32))


@pytest.mark.parametrize("n_coarse", [64, 128])
def test_crossing_equals_the_twin_on_the_coarse_pass(gpu, scene, n_coarse):
    r, c = scene["renderer"], scene["coarse"][n_coarse]
    raw, z = c["raw"], c["z_vals"]
    assert raw.shape == (3 * NPIX, n_coarse, 5) and z.shape == (3 * NPIX, n_coarse)
    want, k = VS.crossing(raw[..., 3].cpu().numpy(), z.cpu().numpy())
    got = r.crossing(raw, z).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the input populates both branches, and both 64-sample tiles at n_coarse = 128: an input that drifts fails here
    crossed = k >= 0
    print(f"n_coarse {n_coarse}: {crossed.sum()} of {len(k)} rays cross (view 0: {crossed[:NPIX].sum()}), first crossings {k[crossed].min()} .. {k.max()}")
    assert crossed.mean() >= 0.25 and (~crossed).mean() >= 0.05
    for tile in range(n_coarse // 64):
        assert ((k >= 64 * tile) & (k < 64 * (tile + 1))).any(), f"no first crossing in tile {tile}"
    assert np.array_equal(scene["modular"][n_coarse]["surface_z"].reshape(-1).cpu().numpy().view(np.int32), want.view(np.int32))


def _target_depth(gpu):
    rs = np.random.RandomState(11)
    d = (0.4 + 2.5 * rs.rand(3, CAM["H"], CAM["W"])).astype(np.float32)
    d[rs.rand(*d.shape) < 0.1] = 0.0                                 # missing measurements: sampled near .. far
    return torch.from_numpy(d).to(gpu)


def test_depth_guided_render_equals_render_rays(gpu, scene):
    r, m, poses = scene["renderer"], scene["model"], scene["poses"]
    td = _target_depth(gpu)
    with torch.no_grad():
        want = m.render_rays(scene["rays"][0], scene["rays"][1], target_d=td.reshape(-1))
    want = {k: want[k].reshape(3, CAM["H"], CAM["W"], *want[k].shape[1:]) for k in FIELD_OUT}
    modular = r.render(poses, target_depth=td, fused=False)
    _same(modular, want, FIELD_OUT, "modular, depth guided")
    assert torch.equal(modular["surface_z"], td)
    for chunk in (101, 1 << 16):
        _same(r.render(poses, target_depth=td, ray_chunk=chunk), modular, FIELD_OUT + ("surface_z",), f"fused, depth guided, chunk {chunk}")


@pytest.mark.parametrize("n_coarse", [64, 128])
def test_fused_launch_equals_the_modular_twin(gpu, scene, n_coarse):
    """Every output, in every bit; ray chunks of 64 (one wave's lanes), 100 and 101 (the renderer rounds them up to whole groups of 16 rays:
    112), 16 (one workgroup per launch) and the whole batch."""
    from naruto_amd.render import OUTPUTS
    r, poses, want = scene["renderer"], scene["poses"], scene["modular"][n_coarse]
    assert set(want) == set(OUTPUTS) and all(bool(torch.isfinite(want[k]).all()) for k in OUTPUTS)
    assert float(want["uncert_map"].min()) > 0 and bool((want["surface_z"] > 0).any()) and bool((want["surface_z"] == 0).any())
    for chunk in (64, 100, 101, 3 * NPIX) + ((16,) if n_coarse == 128 else ()):
        _same(r.render(poses, n_coarse=n_coarse, ray_chunk=chunk), want, OUTPUTS, f"fused, chunk {chunk}")
    _same(r.render(poses, n_coarse=n_coarse, ray_chunk=100, fused=False), want, OUTPUTS, "modular, chunk 100")
    part = r.render(poses[1:2], n_coarse=n_coarse, outputs=("depth", "uncert_map"))
    assert set(part) == {"depth", "uncert_map"} and torch.equal(_bits(part["depth"][0]), _bits(want["depth"][1]))


def test_fused_launch_equals_the_modular_twin_bf16(gpu):
    from naruto_amd.render import OUTPUTS
    cfg, m, r = _field(gpu, mlp="bf16")
    poses = _poses(cfg).to(gpu)
    want = r.render(poses, fused=False)
    for chunk in (101, 3 * NPIX):
        _same(r.render(poses, ray_chunk=chunk), want, OUTPUTS, f"bf16 fused, chunk {chunk}")
    assert bool((want["surface_z"] > 0).any())


def test_fused_launch_with_a_partly_filled_last_group(gpu, scene):
    """23 x 19 pixels x 2 poses = 874 rays = 54 groups of 16 and one of 10; in chunks of 64 the last launch holds 42 rays."""
    from naruto_amd.render import OUTPUTS, FieldViewRendererHIP
    cam = dict(H=19, W=23, fx=18.0, fy=18.0, cx=11.0, cy=9.0)
    r = FieldViewRendererHIP(scene["model"], scene["cfg"], cam)
    poses = scene["poses"][1:]
    want = r.render(poses, fused=False)
    assert want["rgb"].shape == (2, 19, 23, 3)
    for chunk in (64, 2 * 19 * 23):
        _same(r.render(poses, ray_chunk=chunk), want, OUTPUTS, f"fused, 23 x 19, chunk {chunk}")
    _same(r.render(poses, ray_chunk=64, fused=False), want, OUTPUTS, "modular, 23 x 19, chunk 64")


def test_fused_launch_with_a_fine_pass_of_two_tiles(gpu):
    """75 fine samples: the fine pass walks two 64-sample tiles, with the render's early termination behind the first sign change."""
    from naruto_amd.render import OUTPUTS
    cfg, m, r = _field(gpu, n_samples_d=64)
    poses = _poses(cfg).to(gpu)[:2]
    want = r.render(poses, fused=False)
    _same(r.render(poses, ray_chunk=101), want, OUTPUTS, "fused, 75 fine samples")


def _views(scene, H_, W_, seed):
    """A rendered-looking pair of views: (rgb, depth, gt_rgb, gt_depth) float32 numpy, P = 2."""
    rs = np.random.RandomState(seed)
    gt_rgb = rs.rand(2, H_, W_, 3).astype(np.float32)
    rgb = np.clip(gt_rgb + 0.05 * rs.randn(2, H_, W_, 3), 0, 1).astype(np.float32)
    gt_depth = (0.5 + 3.0 * rs.rand(2, H_, W_)).astype(np.float32)
    gt_depth[rs.rand(2, H_, W_) < 0.2] = 0.0
    depth = (gt_depth + 0.02 * rs.randn(2, H_, W_)).astype(np.float32)
    return rgb, depth, gt_rgb, gt_depth


def _check_metrics(gpu, views, depth_trunc=None):
    from naruto_amd.render import image_metrics
    dev = [torch.from_numpy(v).to(gpu) for v in views]
    got = image_metrics(*dev, depth_trunc=depth_trunc, maps=True)
    again = image_metrics(*dev, depth_trunc=depth_trunc)
    assert torch.equal(got["sums"].view(torch.int64), again["sums"].view(torch.int64)), "the sums of a second run"
    for p in range(len(views[0])):
        want = VS.metrics(*(v[p] for v in views), depth_trunc=depth_trunc)
        for k in ("se_map", "depth_err_map", "ssim_map"):
            g = got[k][p].cpu().numpy()
            assert g.shape == want[k].shape and np.array_equal(g.view(np.int64), want[k].view(np.int64)), (k, p)
        sums = got["sums"][p].cpu().numpy()
        # any summation order over n terms is within n 2^-52 sum |term| of the exact sum (derived, not measured); the counts are exact
        bound = want["n_terms"] * 2.0 ** -52 * want["abs_sums"]
        print("view", p, "sums", sums, "twin", want["sums"], "bound", bound)
        assert (np.abs(sums - want["sums"]) <= bound).all(), (sums, want["sums"], bound)
        assert sums[1] == want["sums"][1] and sums[3] == want["sums"][3] and sums[5] == want["sums"][5]
        for k in ("psnr", "ssim", "depth_l1_cm"):
            a, b = float(got[k][p]), want[k]
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * max(1.0, abs(b)), (k, a, b)
    return got


def test_image_metrics_equal_the_twin(gpu, scene):
    """On the 24 x 20 views (SSIM positions in one 16 x 16 tile, pixels in four) and on 13 x 11 (SSIM windows in a single 3 x 1 strip)."""
    rendered = scene["modular"][128]
    rs = np.random.RandomState(5)
    rgb = rendered["rgb"].cpu().numpy()
    depth = rendered["depth"].cpu().numpy()
    gt_rgb = np.clip(rgb + 0.1 * rs.randn(*rgb.shape), 0, 1).astype(np.float32)
    gt_depth = (depth + 0.05 * rs.randn(*depth.shape)).astype(np.float32)
    gt_depth[rs.rand(*depth.shape) < 0.15] = 0.0
    got = _check_metrics(gpu, (rgb, depth, gt_rgb, gt_depth))
    assert bool(torch.isfinite(got["psnr"]).all()) and bool(((got["ssim"] > 0) & (got["ssim"] < 1)).all()) and bool((got["depth_l1_cm"] > 0).all())
    _check_metrics(gpu, (rgb, depth, gt_rgb, gt_depth), depth_trunc=2.0)
    small = _check_metrics(gpu, _views(scene, 11, 13, 7))
    assert small["ssim_map"].shape == (2, 1, 3, 3)
    _check_metrics(gpu, _views(scene, 37, 50, 8))                      # several tiles each way, partly filled at both edges


def test_image_metrics_edge_views(gpu, scene):
    from naruto_amd.render import image_metrics
    views = _views(scene, 10, 24, 9)
    got = _check_metrics(gpu, views)                                   # H below 11: no SSIM, the other two as the twin has them
    assert bool(torch.isnan(got["ssim"]).all()) and bool(torch.isfinite(got["psnr"]).all()) and bool(torch.isfinite(got["depth_l1_cm"]).all())
    views = _views(scene, 20, 24, 10)
    views = (views[0], views[1], views[2], np.zeros_like(views[3]))
    got = _check_metrics(gpu, views)                                   # no valid depth
    assert bool(torch.isnan(got["depth_l1_cm"]).all()) and bool(torch.isfinite(got["ssim"]).all())
    same = image_metrics(*(torch.from_numpy(v).to(gpu) for v in (views[0], views[1], views[0], views[1])))
    assert bool((same["ssim"] == 1.0).all()) and bool(torch.isinf(same["psnr"]).all())


# --------------------------------------------------------------------------------------------- checkpoints and runs (40 x 30, as test_gpu_slam.py)
WW, HH, FOC = 40, 30, 30.0
ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]


def _run_cfg():
    c = H.office_cfg(12, perturb=1.0)
    cam = CS.camera(WW, HH, FOC)
    c["cam"].update(H=HH, W=WW, fx=FOC, fy=FOC, cx=cam["cx"], cy=cam["cy"], depth_trunc=100.0, near=0, far=5)
    c["mapping"]["bound"] = copy.deepcopy(ROOM)
    c["mapping"]["marching_cubes_bound"] = copy.deepcopy(ROOM)
    c["mapping"].update(sample=128, min_pixels_cur=16, keyframe_every=5, map_every=5, iters=5, first_iters=10, n_pixels=0.5, filter_depth=True)
    c["tracking"] = {"disable": True}
    c["mesh"].update(vis=500, voxel_eval=0.1, voxel_final=0.1)
    return c


def _look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4, dtype=np.float32)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64)).astype(np.float32)
    p[:3, 3] = pos
    return p


def _arc(n):
    return torch.from_numpy(np.stack([_look([1.2 + 0.5 * np.sin(0.08 * k), 1.0 + 0.12 * k, 1.2 + 0.02 * k], CS.ROOM_CENTRE) for k in range(n)]))


def _sim(gpu):
    from naruto_amd.simulator import MeshSimHIP
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    return MeshSimHIP((v, f), CS.camera(WW, HH, FOC), erp_hw=(32, 64), face_w=32, far=100.0, device=gpu)


def test_checkpoint_round_trip(gpu, tmp_path):
    from naruto_amd.render import FieldViewRendererHIP, field_from_checkpoint
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = _run_cfg()
    a = CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=8, seed=3, result_dir=str(tmp_path / "a"), device=gpu)
    poses = _arc(4)
    for i in (0, 2, 5):
        a.est_c2w_data[i] = poses[i % 4]
    a.est_c2w_data_rel[0] = poses[0]
    a.est_c2w_data_rel[2] = poses[3]
    with torch.no_grad():
        a.model.uncert_grid.mul_(0.5)
    want = a.render_view(poses[1:3])
    path = a.save_ckpt(7)
    b = CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=8, seed=4, device=gpu)
    b.est_c2w_data[1] = poses[1]                                     # a pose the checkpoint does not hold: gone after the load
    assert not torch.equal(_bits(b.render_view(poses[1:3])["rgb"]), _bits(want["rgb"])), "the two fields were meant to differ before the load"
    b.load_ckpt(path)
    _same(b.render_view(poses[1:3]), want, tuple(want), "after load_ckpt")
    for x, y in ((a.est_c2w_data, b.est_c2w_data), (a.est_c2w_data_rel, b.est_c2w_data_rel)):
        dx, dy = x.as_dict(), y.as_dict()
        assert sorted(dx) == sorted(dy) and all(torch.equal(dx[k], dy[k]) for k in dx)
    assert sorted(b.est_c2w_data.as_dict()) == [0, 2, 5]
    m = field_from_checkpoint(path, copy.deepcopy(cfg), device=gpu)
    cam = {k: getattr(a, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
    _same(FieldViewRendererHIP(m, cfg, cam).render(poses[1:3]), want, tuple(want), "field_from_checkpoint")
    with pytest.raises(ValueError, match="frame"):
        CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=4, seed=4, device=gpu).load_ckpt(path)


def test_evaluate_views_and_a_run_with_eval_views(gpu, tmp_path):
    from naruto_amd.render import evaluate_views
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg, sim, traj = _run_cfg(), _sim(gpu), _arc(6)
    fresh = CoSLAMNarutoHIP(copy.deepcopy(cfg), num_frames=6, seed=3, device=gpu)
    cam = {k: getattr(fresh, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
    ev = evaluate_views(fresh.model, cfg, sim, traj[::2], cam=cam)               # a field that was never trained
    print("untrained field:", {k: ev[k] for k in ("psnr", "ssim", "depth_l1_cm")})
    assert np.isfinite(ev["psnr"]) and np.isfinite(ev["ssim"]) and len(ev["per_view"]["psnr"]) == 3
    assert ev == evaluate_views(fresh.model, cfg, sim, traj[::2], cam=cam)
    guided = evaluate_views(fresh.model, cfg, sim, traj[::2], cam=cam, depth_guided=True)
    assert np.isfinite(guided["psnr"]) and guided != ev

    def run(tag, **kw):
        slam = CoSLAMNarutoHIP(copy.deepcopy(cfg), voxel_size=0.1, active_ray=False, num_frames=6, seed=3, result_dir=str(tmp_path / tag), device=gpu)
        return slam, run_exploration(slam, sim, None, None, 6, traj=traj, **kw)
    slam_a, plain = run("a")
    slam_b, scored = run("b", eval_views=2)
    assert set(scored) == set(plain) | {"render_eval"}
    assert torch.equal(scored["poses"], plain["poses"]) and scored["fresh"] == plain["fresh"] and scored["states"] == plain["states"]
    assert np.array_equal(np.asarray(scored["mesh"].vertices), np.asarray(plain["mesh"].vertices))
    for (n, p), (_, q) in zip(slam_a.model.named_parameters(), slam_b.model.named_parameters()):
        assert torch.equal(p, q), n
    re = scored["render_eval"]
    print("after 6 frames:", {k: re[k] for k in ("psnr", "ssim", "depth_l1_cm")})
    assert len(re["per_view"]["psnr"]) == 3 and np.isfinite(re["psnr"]) and np.isfinite(re["ssim"])
    assert re == evaluate_views(slam_a.model, cfg, sim, plain["poses"][::2], cam=cam)

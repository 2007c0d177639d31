"""Every launch stays inside the bytes its naruto_*_workspace() function reported.  ``_lib.workspace`` -- the one place the package
turns such a byte count into a tensor -- is replaced by an allocator that serves each request as the front of a larger buffer whose
tail, from the reported byte on, is GUARD bytes of 0xA5.  A write past the reported size lands in that tail, inside the allocation;
every buffer is kept until the scenario ends, then every tail must still read 0xA5.  One scenario per subsystem, at the smallest
shapes of the subsystem's own GPU tests (whose fixtures are reused); values are those tests' business, here a scenario only has to
succeed."""
import numpy as np
import pytest
import torch

import cull_spec as CS
import helpers as H
import sim_spec as SS
from naruto_amd import _lib
from naruto_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture
def guarded(monkeypatch, gpu):
    served = []

    def workspace(n_bytes, device, dtype=torch.float32, zero=False):
        n_bytes = int(n_bytes)
        front = -(-n_bytes // dtype.itemsize) * dtype.itemsize
        raw = torch.zeros(front + GUARD, dtype=torch.uint8, device=device) if zero else torch.empty(front + GUARD, dtype=torch.uint8, device=device)
        raw[n_bytes:] = 0xA5
        served.append((raw, n_bytes))
        return raw[:front].view(dtype)

    monkeypatch.setattr(_lib, "workspace", workspace)
    yield served
    torch.cuda.synchronize()
    assert served, "the scenario allocated no workspace through _lib.workspace"
    for raw, n_bytes in served:
        tail = raw[n_bytes:]
        hit = (tail != 0xA5).nonzero()
        assert hit.numel() == 0, f"a workspace of {n_bytes} reported bytes was written at byte {n_bytes + int(hit[0])} ({hit.numel()} guard bytes changed)"


def _train_iteration(gpu, n_samples_d, smooth):
    from naruto_amd import ops
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=n_samples_d)
    tr, cam = cfg["training"], cfg["cam"]
    m = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.25, 43), gpu)
    N, S = 128, tr["n_samples_d"] + tr["n_range_d"]
    t = {k: torch.from_numpy(v) for k, v in syn.random_rays(N, cfg["mapping"]["bound"], seed=43, zero_depth_frac=0.15).items()}
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.37 if smooth else 0.0, 0.0])
    ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"],
                       far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True, loss_weights=w.to(gpu),
                       smooth=(12, 0.1, 0.05) if smooth else None, device_rng=False)
    if smooth:
        ts.rand[N * S:].copy_(torch.tensor([0.3, 0.6, 0.2, 0.1, 0.7, 0.4]))
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    losses = ts.run(*args, rand=torch.rand(N, S, generator=torch.Generator().manual_seed(7)).to(gpu))
    torch.cuda.synchronize()
    assert S == n_samples_d + 11 and bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(g).all()) for g in ts.grads.values() if g is not None)


def test_training_iteration_with_the_smoothness_term(gpu, guarded):
    _train_iteration(gpu, 32, True)


def test_training_iteration_at_64_samples_per_ray(gpu, guarded):
    _train_iteration(gpu, 53, False)


def test_three_tracking_iterations(gpu, guarded):
    import test_gpu_tracking as TT
    from naruto_amd import tracking as TK
    cfg = H.office_cfg(12, perturb=1.0)
    m = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.25, 43), gpu)
    for p in m.parameters():
        p.requires_grad_(False)
    scene = syn.AnalyticRoom(cfg["mapping"]["bound"])
    fr = scene.rays(1, TT.N_CAM, H=TT.HH, W=TT.WW, f=TT.FOC)
    pos, R = scene.pose(1, TT.N_CAM)
    frame = (torch.tensor((fr["rays_d"].astype(np.float64) @ R).reshape(TT.HH, TT.WW, 3), dtype=torch.float32, device=gpu),
             torch.from_numpy(fr["target_rgb"].reshape(TT.HH, TT.WW, 3)).to(gpu), torch.from_numpy(fr["target_d"].reshape(TT.HH, TT.WW)).to(gpu))
    init = torch.eye(4)
    init[:3, :3], init[:3, 3] = torch.from_numpy(R).float(), torch.from_numpy(pos).float()
    trk = TK.TrackerHIP(m, TT._cfg(cfg, iter=3), TT.HH, TT.WW, rng_seed=16)
    c2w = trk.track(*frame, init)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(c2w)).all())


def test_one_ba_pose_step(gpu, guarded):
    import test_gpu_ba_poses as TBA
    env = TBA._env(gpu, active=True, iters=1, pose_accum_step=1)
    try:
        (poses,), _ = TBA._call(env)
        assert bool(torch.isfinite(poses).all())
    finally:
        TBA._done(env)


def test_mesh_extraction(gpu, guarded):
    from naruto_amd import mesh as M
    x = np.arange(8, dtype=np.float32) - 3.5
    vol = np.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) - 2.6
    v, f = M.marching_cubes(torch.from_numpy(vol.astype(np.float32)).to(gpu), 0.0, 3.0)
    torch.cuda.synchronize()
    assert len(v) > 0 and len(f) > 0 and int(f.max()) < len(v)


def test_reconstruction_metrics(gpu, guarded):
    from naruto_amd import evaluation as E
    out = E.calc_3d_mesh_metric(syn.room_sphere_mesh(0.0, 0.8), syn.room_sphere_mesh(0.02, 0.81), n_samples=20000)
    assert all(np.isfinite(out[k]) for k in ("accuracy_cm", "completion_cm", "completion_ratio_pct")), out


def test_culling_two_poses(gpu, guarded):
    from naruto_amd import culling as CU
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    got = CU.render_depth(v, f, CS.ring_poses(2), CS.camera(16, 12, 12.0), keep_inf=True)
    torch.cuda.synchronize()
    assert got.shape == (2, 12, 16) and bool(torch.isfinite(got).all())          # a closed room: every pixel is covered


def test_simulator_frame_and_panorama(gpu, guarded):
    import test_gpu_sim as TS
    v, f, col, _ = SS.box_scene(missing=TS.MISSING)
    sim = TS._sim((v, f, col), CS.camera(40, 30, 30.0))
    color, depth, erp_color, erp_depth = sim.simulate(TS._box_pose(), return_erp=True, no_print=True)
    torch.cuda.synchronize()
    assert tuple(np.shape(erp_depth)) == (16, 32) and tuple(np.shape(depth))[-2:] == (30, 40)


def test_goal_targets(gpu, guarded):
    from naruto_amd.planner_aggregation import GoalSpaceAggregatorHIP
    ag = GoalSpaceAggregatorHIP([[0.0, 0.3], [0.0, 0.4], [0.0, 0.5]], 0.1, uncert_top_k=8, uncert_top_k_subset=4, gs_z_levels=[1, 3], device=gpu)
    assert (ag.Nx, ag.Ny, ag.Nz) == (4, 5, 6)
    uncert = torch.rand(4, 5, 6, generator=torch.Generator().manual_seed(3)).to(gpu)
    tg = ag.select_targets(uncert)
    torch.cuda.synchronize()
    assert tuple(tg.shape) == (4, 3) and int(tg.min()) >= 0 and bool((tg.cpu() < torch.tensor([4, 5, 6])).all())


def test_rrt_start_grow_and_path(gpu, guarded):
    import test_gpu_rrt as TR
    rec = TR.load("a")
    p = TR.planner(rec)
    flags = TR.replay(rec, p)
    TR.check_tree(rec, p, flags)
    assert p.get_reachable_mask().shape == rec["vol"].shape


def test_active_ray_selection(gpu, guarded):
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    cfg = H.office_cfg(16)
    cfg["mapping"]["sample"], cfg["mapping"]["min_pixels_cur"] = 128, 20
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=40, oversample_mul=4)
    n_cur = 33
    t = {k: torch.from_numpy(v) for k, v in syn.random_rays(smp.oversample_num + n_cur, cfg["mapping"]["bound"], seed=53).items()}
    vol = np.random.RandomState(5).uniform(0, 3, (49, 56, 35)).astype(np.float32)
    got = smp.sample_rays(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")), list(range(n_cur)), vol, cfg["mapping"]["bound"])
    torch.cuda.synchronize()
    assert got[0].shape[0] == smp.n_out(n_cur) and all(bool(torch.isfinite(a).all()) for a in got)

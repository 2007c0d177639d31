"""CoSLAMNarutoHIP and run_exploration on the device: a field trained from the frames the simulator renders.

1. Eleven frames through ``online_recon_step`` against a twin that drives the public pieces by hand in the reference's order
   (``torch.cat``, ``KeyFrameStoreHIP.add_keyframe``, ``FusedBA.global_BA``, ``get_map_volumes``, ``set_volume``): bit for bit.
2. ``tracking.disable: False`` is refused before anything is launched.
3. The closed run: simulator, SLAM and planner for 40 steps on the room mesh.

Run: timeout -k 10 600 python -m pytest tests/test_gpu_slam.py -m gpu -q -s
"""
import copy

import numpy as np
import pytest
import torch

import cull_spec as CS
import helpers as H
import planner_spec as PS

pytestmark = pytest.mark.gpu

WW, HH, FOC = 40, 30, 30.0
ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]


def _cfg(**mapping):
    c = H.office_cfg(12, perturb=1.0)
    cam = CS.camera(WW, HH, FOC)
    c["cam"].update(H=HH, W=WW, fx=FOC, fy=FOC, cx=cam["cx"], cy=cam["cy"], depth_trunc=100.0, near=0, far=5)
    c["mapping"]["bound"] = copy.deepcopy(ROOM)
    c["mapping"]["marching_cubes_bound"] = copy.deepcopy(ROOM)
    c["mapping"].update(sample=128, min_pixels_cur=16, keyframe_every=5, map_every=5, iters=10, first_iters=20, n_pixels=0.5, filter_depth=True)
    c["mapping"].update(mapping)
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
    """A short arc inside the room, looking at the sphere."""
    out = []
    for k in range(n):
        a = 0.08 * k
        out.append(_look([1.2 + 0.5 * np.sin(a), 1.0 + 0.12 * k, 1.2 + 0.02 * k], CS.ROOM_CENTRE))
    return torch.from_numpy(np.stack(out))


def _sim(gpu):
    from naruto_amd.simulator import MeshSimHIP
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    return MeshSimHIP((v, f), CS.camera(WW, HH, FOC), erp_hw=(32, 64), face_w=32, far=100.0, device=gpu)


@pytest.fixture(scope="module")
def frames(gpu):
    """Frames 0 .. 10 of the arc, rendered once: (poses [11,4,4] host, color [11,H,W,3], depth [11,H,W] on the device)."""
    poses = _arc(11)
    color, depth = _sim(gpu).simulate_batch(poses)
    assert bool((depth > 0).any())
    return poses, color, depth


def _params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("active", [False, True])
def test_eleven_frames_equal_the_hand_driven_twin(gpu, frames, active):
    from naruto_amd import trainer
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    from naruto_amd.ba_loop import FusedBA
    from naruto_amd.field import get_map_volumes
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    from naruto_amd.slam import CoSLAMNarutoHIP
    poses, color, depth = frames
    cfg = _cfg()
    slam = CoSLAMNarutoHIP(copy.deepcopy(cfg), voxel_size=0.1, active_ray=active, act_ray_num_uncert_sample=32, act_ray_oversample_mul=4, num_frames=11,
                           seed=7, device=gpu)
    assert slam.num_rays_to_save == 600 and slam.keyframeDatabase.rays.shape[0] == 11 // 5 + 1
    # ---- the twin: the same pieces, driven by hand
    cfg_t = copy.deepcopy(cfg)
    cfg_t["mapping"]["active_ray"] = active
    tr = trainer.MappingTrainer(cfg_t, torch.tensor(ROOM), gpu, uncert_voxel=0.1, fused_adam=True)
    tr.model.load_state_dict(slam.model.state_dict())
    tr.iter_state.copy_(slam.trainer.iter_state)
    store = KeyFrameStoreHIP(cfg_t, HH, WW, num_kf=3, num_rays_to_save=600, device=gpu, seed=7)
    smp = ActiveRaySamplerHIP(config=cfg_t, num_uncert_sample=32, oversample_mul=4) if active else None
    ba = FusedBA(tr, store, smp, max_poses=4, use_graph=False)
    captures, seen_kf, shapes = [], [], []
    cap0, prep0 = slam.trainer.capture, slam.ba.prepare

    def counting_capture(*a, **k):
        captures.append(a[0])
        return cap0(*a, **k)

    def watching_prepare(*a, **k):
        seen_kf.append(len(slam.keyframeDatabase))
        out = prep0(*a, **k)
        shapes.append(out)
        return out
    slam.trainer.capture, slam.ba.prepare = counting_capture, watching_prepare
    est, cached, returned = {}, None, []
    for i in range(11):
        vols = slam.online_recon_step(i, color[i], depth[i], poses[i])
        returned.append(vols is not None)
        # the twin's step, in the reference's order (coslam.py:579-633)
        batch = {"frame_id": torch.tensor([i]), "rgb": color[i][None], "depth": depth[i][None], "direction": slam.rays_d[None]}
        want = None
        if i == 0:
            est[0] = poses[0].to(gpu)
            current = torch.cat([batch["direction"], batch["rgb"], batch["depth"][..., None]], -1).reshape(-1, 7)

            def batches():
                for _ in range(20):
                    yield store.assemble_batch(0, current, est[0][None], 0, rng=tr.iter_state, n_cur=128, n_cur_pop=HH * WW)[:4]
            tr.first_frame_mapping(batches())
            store.add_keyframe(batch, filter_depth=True)
            want = get_map_volumes(tr.model.query_sdf, tr.model.bounding_box, 0.1)
        else:
            est[i] = poses[i].to(gpu)
            if i % 5 == 0:
                p_all = torch.stack([est[k] for k in range(0, i, 5)] + [est[i]])
                current = torch.cat([batch["direction"], batch["rgb"], batch["depth"][..., None]], -1).reshape(-1, 7)
                ba.global_BA(current, p_all, uncert_vol=cached if active else None)
                want = get_map_volumes(tr.model.query_sdf, tr.model.bounding_box, 0.1)
                store.add_keyframe(batch, filter_depth=True)
        if want is not None:
            assert vols is not None and all(v.is_cuda for v in vols)
            for name, got, w in zip(("uncert", "sdf"), vols, want):
                assert np.array_equal(got.cpu().numpy().view(np.int32), w.view(np.int32)), f"frame {i}: {name} volume"
            cached = want[0]
    assert [k for k, r in enumerate(returned) if r] == [0, 5, 10]
    assert slam.keyframeDatabase.frame_ids.tolist() == [0, 5, 10] and store.frame_ids.tolist() == [0, 5, 10]
    assert seen_kf == [1, 2], "the BA of frame i sees the keyframes before i"
    assert torch.equal(slam.keyframeDatabase.rays.view(torch.int32), store.rays.view(torch.int32))
    assert slam.keyframeDatabase.counter == store.counter
    for (n, p), (_, q) in zip(slam.model.named_parameters(), tr.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"
    assert torch.equal(slam.model.uncert_grid.grad, tr.model.uncert_grid.grad)
    assert torch.equal(slam.trainer.iter_state, tr.iter_state)
    # one capture for the first frame, then one per change of (n_cur, n_train)
    assert len(shapes) == 2 and len(captures) <= 1 + len(set(shapes)), (captures, shapes)
    assert torch.equal(slam.est_c2w_data[10].cpu(), poses[10]) and len(slam.est_c2w_data) == 11
    slam.model.check_asserts(block=True)


def test_tracking_is_refused_before_any_launch(gpu, monkeypatch):
    from naruto_amd import _lib
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = _cfg()
    cfg["tracking"] = {"disable": False}
    launched = []

    def no_load():
        launched.append(1)
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(NotImplementedError, match="TrackerHIP"):
        CoSLAMNarutoHIP(cfg, num_frames=11, device=gpu)
    assert not launched


def _closed_run(gpu, tmp_path, tag):
    from naruto_amd.planner import NarutoPlannerHIP
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    cfg = _cfg(sample=512, min_pixels_cur=512, first_iters=100)
    np.random.seed(5)
    slam = CoSLAMNarutoHIP(cfg, voxel_size=0.1, active_ray=False, num_frames=40, seed=3, result_dir=str(tmp_path / tag), device=gpu)
    sim = _sim(gpu)
    p = NarutoPlannerHIP(dataset="NARUTO", device=gpu, gs_z_levels=[12], max_rot_deg=30, rrt_max_iter=2000)
    p.update_sim(sim)
    p.init_data(cfg["mapping"]["bound"])
    p.init_local_planner()
    mins = []
    out = run_exploration(slam, sim, p, _look([2.0, 4.0, 1.2], CS.ROOM_CENTRE), 40,
                          on_step=lambda i, c2w, vols, state: mins.append(float(slam.model.min_uncert_running())) if vols is not None else None)
    return slam, out, mins


def test_closed_run(gpu, tmp_path):
    from naruto_amd import culling
    from naruto_amd.evaluation import ReconEvaluatorHIP, trajectory_length
    slam, out, mins = _closed_run(gpu, tmp_path, "a")
    poses, states = out["poses"], out["states"]
    print("closed run:", "".join("m" if s == "movingToGoal" else s[0] for s in states), "fresh volumes at", out["fresh"],
          "trajectory %.2f m" % trajectory_length(poses), {k: round(v["total_s"], 3) for k, v in out["timing"].items()})
    assert poses.shape == (40, 4, 4) and bool(torch.isfinite(poses).all())
    xyz = poses[:, :3, 3].double().numpy()
    assert (xyz > 0.0).all() and (xyz < np.array([6.0, 5.0, 3.0])).all()
    for a, b in zip(["staying"] + states[:-1], states):
        assert b in PS.ALLOWED[a], (a, b)
    assert out["fresh"] == list(range(0, 40, 5)), "fresh volumes arrive exactly at the mapped frames"
    assert any(not torch.equal(q, poses[0]) for q in poses[1:]), "the camera never moved"
    # geometric and deterministic: the share of room vertices seen from the visited poses against the start pose alone
    v, f = CS.room_mesh()
    cam = CS.camera(WW, HH, FOC)
    seen = []
    for ps in (poses[:1], poses):
        d = culling.render_depth(v, f, ps.numpy(), cam, far=100.0)
        seen.append(float(culling.observed_vertices(v, ps.numpy(), cam, depth=d).float().mean()))
    print("observed vertices: start %.4f, run %.4f" % tuple(seen))
    assert seen[1] > seen[0]
    assert len(mins) == 8 and all(m > 0 for m in mins) and float(slam.model.min_uncert_running()) > 0
    assert len(out["mesh"].vertices) > 0 and len(out["mesh"].faces) > 0
    back = culling.poses_from_checkpoint(out["ckpt_path"])
    assert torch.equal(back, poses), "checkpoint poses: frame id -> [4,4], every frame of the run"
    ev = ReconEvaluatorHIP((v, f), n_samples=20000, device=gpu)
    print("MAD at the end: %.3f cm" % ev.evaluate_field(slam.model, slam.config, slam.bounding_box, 0.1)["mad_cm"])
    # a second run with the same seeds: the same poses and parameters, bit for bit
    want = _params(slam.model)
    slam2, out2, _ = _closed_run(gpu, tmp_path, "b")
    assert torch.equal(out2["poses"], poses) and out2["states"] == states
    for n, q in _params(slam2.model).items():
        assert torch.equal(q, want[n]), f"parameter {n}"

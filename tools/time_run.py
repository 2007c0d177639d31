"""Time a whole exploration run on the device (naruto_amd.run.run_exploration: MeshSimHIP, CoSLAMNarutoHIP, NarutoPlannerHIP) at
office_0 size: 1200 x 680, f = 600, the room-plus-sphere mesh of tools/time_cull.py, active rays on, the shipped mapping schedule
(2 048 rays, 10 iterations per mapped frame, 200 first-frame iterations).  Recorded:

  * a --steps (200) step run: steps per second, and per phase (simulation, SLAM, planning) the total and the median per step, the SLAM
    phase split into mapped frames and the others;
  * for one mapped frame, the device route (naruto_frame_ingest, the 8-byte read-back, naruto_keyframe_row, get_map_volumes onto the
    device) against the expression it replaces (torch.cat, FusedBA.prepare's copy and count, add_keyframe, get_map_volumes to the host
    and both volumes uploaded again) on the same frame, and the ingest launch alone against its traffic bound
    (pixels x 56 bytes at 6.29 TB/s);
  * first-frame mapping on the device (FusedBA.first_frame_mapping, capture included and capture alone) against
    MappingTrainer.first_frame_mapping over batches made with torch indexing as the reference makes them.

    python tools/time_run.py [--out profiles/time_run.json] [--steps 200] [--n-lat 632]

Host timers (time.perf_counter), medians over --repeat where a piece is repeated; the one-frame pieces end in a device synchronise.
Nothing is asserted.  There is NO reference number: the reference's loop needs Habitat-Sim and tiny-cuda-nn, neither of which is on this
stack."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naruto_amd import config as cfgmod  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
from naruto_amd.field import get_map_volumes  # noqa: E402
from naruto_amd.keyframe_store import KeyFrameStoreHIP, frame_ingest  # noqa: E402
from naruto_amd.planner import NarutoPlannerHIP, compute_camera_pose  # noqa: E402
from naruto_amd.run import run_exploration  # noqa: E402
from naruto_amd.simulator import MeshSimHIP  # noqa: E402
from naruto_amd.slam import CoSLAMNarutoHIP  # noqa: E402

ROOM = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
COPY_RATE = 6.29e12            # bytes per second, the device-to-device copy rate the traffic bound is stated against


def config():
    cfg = cfgmod.office0_config(perturb=1.0)
    cfg["mapping"].update(bound=[list(b) for b in ROOM], marching_cubes_bound=[list(b) for b in ROOM])
    cfg["tracking"] = {"disable": True}
    return cfg


def median_ms(fn, repeat, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def start_pose():
    p = np.eye(4, dtype=np.float32)
    pos, at = np.array([2.0, 4.0, 1.2]), np.array([3.0, 2.5, 1.4])
    p[:3, :3], p[:3, 3] = compute_camera_pose(pos, at).astype(np.float32), pos
    return torch.from_numpy(p)


def whole_run(args, dev, mesh):
    cfg = config()
    np.random.seed(args.seed)
    slam = CoSLAMNarutoHIP(cfg, active_ray=True, num_frames=args.steps, seed=args.seed, device=dev)
    sim = MeshSimHIP(mesh, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}, device=dev)
    planner = NarutoPlannerHIP(dataset="NARUTO", device=dev)
    planner.update_sim(sim)
    planner.init_data(cfg["mapping"]["bound"])
    planner.init_local_planner()
    per_step = {"Simulation": [], "SLAM": [], "Planning": []}
    for name, obj, attr in (("Simulation", sim, "simulate"), ("SLAM", slam, "online_recon_step"), ("Planning", planner, "main")):
        def wrap(fn, name=name):
            def call(*a, **k):
                t = time.perf_counter()
                out = fn(*a, **k)
                per_step[name].append(time.perf_counter() - t)
                return out
            return call
        setattr(obj, attr, wrap(getattr(obj, attr)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run_exploration(slam, sim, planner, start_pose(), args.steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    loop = sum(sum(v) for v in per_step.values())
    mapped = set(out["fresh"])
    slam_t = per_step["SLAM"]
    res = {"steps": args.steps, "wall_s_with_final_mesh_and_checkpoint": wall, "loop_s": loop, "steps_per_second": args.steps / loop,
           "phases": {k: {"total_s": sum(v), "median_ms_per_step": statistics.median(v) * 1e3} for k, v in per_step.items()},
           "slam_first_frame_ms": slam_t[0] * 1e3,
           "slam_mapped_frame_median_ms": statistics.median([t for i, t in enumerate(slam_t) if i in mapped and i > 0]) * 1e3,
           "slam_other_frame_median_ms": statistics.median([t for i, t in enumerate(slam_t) if i not in mapped]) * 1e3,
           "mapped_frames": len(mapped), "planner_states": {s: out["states"].count(s) for s in sorted(set(out["states"]))},
           "final_mesh_vertices": int(len(out["mesh"].vertices))}
    return res, slam, sim


def frame_routes(args, slam, sim, dev):
    cfg = slam.config
    color, depth = sim.simulate(start_pose().numpy(), no_print=True)
    trunc, n_pix = float(cfg["cam"]["depth_trunc"]), slam.H * slam.W
    stores = [KeyFrameStoreHIP(cfg, slam.H, slam.W, 4, slam.num_rays_to_save, dev, seed=1) for _ in range(2)]
    cur, word = torch.zeros(n_pix, 7, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    pin = torch.zeros(1, dtype=torch.int64).pin_memory()
    vols = torch.zeros_like(slam._vols)

    def device_route():
        frame_ingest(slam.rays_d, color, depth, trunc, cur, word)
        pin.copy_(word, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        stores[0]._n_ids = 0
        stores[0].add_keyframe_device(cur, 0, True, word, n_valid_host=int(pin[0]))
        return get_map_volumes(slam.model.query_sdf, slam.bounding_box, slam.voxel_size, to_host=False, out=vols)

    def parent_route():
        rays = torch.cat([slam.rays_d[None], color[None], depth[None][..., None]], -1).reshape(-1, 7)
        cur.copy_(rays, non_blocking=True)
        int(((rays[:, -1] > 0.0) & (rays[:, -1] <= trunc)).sum().item())
        stores[1]._n_ids = 0
        stores[1].add_keyframe({"direction": slam.rays_d[None], "rgb": color[None], "depth": depth[None], "frame_id": 0}, filter_depth=True)
        host = get_map_volumes(slam.model.query_sdf, slam.bounding_box, slam.voxel_size)
        return [torch.from_numpy(v).to(dev) for v in host]
    ingest_ms = median_ms(lambda: [frame_ingest(slam.rays_d, color, depth, trunc, cur, word) for _ in range(20)], args.repeat) / 20
    return {"pixels": n_pix, "device_route_ms": median_ms(device_route, args.repeat), "parent_route_ms": median_ms(parent_route, args.repeat),
            "ingest_launch_us_back_to_back": ingest_ms * 1e3, "ingest_traffic_bound_us": n_pix * 56 / COPY_RATE * 1e6}


def first_frame(args, dev, sim):
    from naruto_amd import trainer
    from naruto_amd.ba_loop import FusedBA
    cfg = config()
    bound = torch.tensor(cfg["mapping"]["bound"])
    H, W, n, iters = cfg["cam"]["H"], cfg["cam"]["W"], int(cfg["mapping"]["sample"]), int(cfg["mapping"]["first_iters"])
    color, depth = sim.simulate(start_pose().numpy(), no_print=True)
    from naruto_amd.slam import camera_rays
    rays_d = camera_rays(H, W, 600.0, 600.0, 599.0, 339.0).to(dev)
    pose = start_pose().to(dev)
    out = {}
    tr = trainer.MappingTrainer(cfg, bound, dev, fused_adam=True)
    ba = FusedBA(tr, KeyFrameStoreHIP(cfg, H, W, 2, 16, dev), None, max_poses=4)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    frame_ingest(rays_d, color, depth, float(cfg["cam"]["depth_trunc"]), ba.current, word)
    out["device_ms_with_capture"] = median_ms(lambda: ba.first_frame_mapping(pose, iters), args.repeat)
    out["device_capture_alone_ms"] = median_ms(lambda: ba.first_frame_mapping(pose, 0), args.repeat)
    tr2 = trainer.MappingTrainer(cfg, bound, dev, fused_adam=True)

    def torch_batches():
        # coslam.py:202-211: select_samples, three gathers, the rotation in torch
        for _ in range(iters):
            idx = torch.randperm(H * W, device=dev)[:n]
            ih, iw = idx % H, torch.div(idx, H, rounding_mode="trunc")
            d_cam, rgb, dep = rays_d[ih, iw], color[ih, iw], depth[ih, iw].unsqueeze(-1)
            yield pose[None, :3, -1].repeat(n, 1), torch.sum(d_cam[..., None, :] * pose[:3, :3], -1), rgb, dep
    out["eager_torch_batches_ms"] = median_ms(lambda: tr2.first_frame_mapping(torch_batches()), args.repeat)
    out["iterations"], out["rays"] = iters, n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-lat", type=int, default=632)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    vn, fn = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    res = {"image": [1200, 680], "focal": 600.0, "faces": len(fn), "active_ray": True,
           "reference": "none: the reference's loop needs Habitat-Sim and tiny-cuda-nn, which are not on this stack"}
    res["run"], slam, sim = whole_run(args, dev, (vn, fn))
    print(json.dumps(res["run"], indent=1), flush=True)
    res["mapped_frame_routes"] = frame_routes(args, slam, sim, dev)
    print(json.dumps(res["mapped_frame_routes"], indent=1), flush=True)
    del slam
    res["first_frame_mapping"] = first_frame(args, dev, sim)
    print(json.dumps(res["first_frame_mapping"], indent=1), flush=True)
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_run.py: host timers, medians over --repeat; the one-frame pieces end in a device synchronise; milliseconds unless named otherwise",
               "office_0_size": res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

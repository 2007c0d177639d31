"""Time the view renderer (naruto_amd.render) against its modular twin: the fused launch and the existing launches it replaces, in
alternating runs on the same build, at the office_0 camera size (1200 x 680) for one pose and for eight, and for 64 poses of 40 x 30
(the planner-style batch), both MLP modes; next to them evaluate_views' cost per view and the metrics launches alone.

    python tools/time_view.py [--out profiles/time_view.json] [--repeat 7] [--n-coarse 128]

The field is the tests' closed-form one (helpers.make_oracle(office_cfg(16), 0.5, 3)): how many rays cross, and where, moves the fused
launch's saving, so the crossing statistics are recorded with the times.  Host timers that end in a device synchronise, one warm-up,
medians; ``spread`` is max - min over the repeats.  ``fused_wins`` = the fused median is below the modular one by more than twice the
modular path's own spread: the rule that decides the renderer's default.  Nothing is asserted."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from naruto_amd import render as R  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
from naruto_amd.simulator import MeshSimHIP  # noqa: E402
import helpers as H  # noqa: E402


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternating(fns, repeat):
    """{name: [ms]} with the candidates taking turns inside every repeat."""
    for fn in fns.values():
        fn()
    out = {k: [] for k in fns}
    for _ in range(repeat):
        for k, fn in fns.items():
            out[k].append(once(fn))
    return out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms)}


def yaw_poses(n, centre):
    out = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for k in range(n):
        a = 2.0 * np.pi * k / n
        out[k, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        out[k, :3, 3] = centre
    return torch.from_numpy(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_view.json"))
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--n-coarse", type=int, default=128)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    office = {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}
    small = {"H": 30, "W": 40, "fx": 30.0, "fy": 30.0, "cx": 19.5, "cy": 14.5}
    sizes = [("office0_1_pose", office, 1), ("office0_8_poses", office, 8), ("planner_64x40x30", small, 64)]
    res = {"n_coarse": args.n_coarse, "repeat": args.repeat, "device": torch.cuda.get_device_name(0), "cases": {},
           "context": "the eval render of 8192 rays x 43 samples takes 0.108 - 0.113 ms (README)"}
    for mlp in ("fp32", "bf16"):
        cfg = H.office_cfg(16)
        cfg["decoder"]["mlp_precision"] = mlp
        model = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.5, 3).eval(), dev).eval()
        centre = np.array(cfg["mapping"]["bound"]).mean(1)
        for name, cam, n_poses in sizes:
            r = R.FieldViewRendererHIP(model, cfg, dict(cam, near=cfg["cam"]["near"], far=cfg["cam"]["far"]))
            poses = yaw_poses(n_poses, centre).to(dev)
            ms = alternating({"modular": lambda: r.render(poses, n_coarse=args.n_coarse, fused=False),
                              "fused": lambda: r.render(poses, n_coarse=args.n_coarse, fused=True)}, args.repeat)
            z = r.render(poses, n_coarse=args.n_coarse, outputs=("surface_z",))["surface_z"]
            case = {k: stats(v) for k, v in ms.items()}
            case.update(rays=n_poses * cam["H"] * cam["W"], share_of_rays_that_cross=float((z > 0).float().mean()),
                        mean_crossing_depth_m=float(z[z > 0].mean()) if bool((z > 0).any()) else None)
            case["fused_over_modular"] = case["fused"]["median_ms"] / case["modular"]["median_ms"]
            case["fused_wins"] = case["modular"]["median_ms"] - case["fused"]["median_ms"] > 2.0 * case["modular"]["spread_ms"]
            res["cases"][f"{name}_{mlp}"] = case
            print(name, mlp, json.dumps(case))
    # evaluate_views and the metrics launches alone, at the office_0 size, against the room-plus-sphere mesh
    cfg = H.office_cfg(16)
    cfg["cam"].update(office)
    room = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
    cfg["mapping"]["bound"], cfg["mapping"]["marching_cubes_bound"] = copy.deepcopy(room), copy.deepcopy(room)
    model = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.5, 3).eval(), dev).eval()
    v, f = syn.room_sphere_mesh(n_lat=64, n_lon=128)
    sim = MeshSimHIP((v, f), office, erp_hw=(32, 64), face_w=32, far=100.0, device=dev)
    poses = yaw_poses(8, np.array([2.0, 2.5, 1.2]))
    ev = alternating({"evaluate_views": lambda: R.evaluate_views(model, cfg, sim, poses)}, args.repeat)["evaluate_views"]
    gt_rgb, gt_depth = sim.simulate_batch(poses)[:2]
    views = R.FieldViewRendererHIP(model, cfg).render(poses, outputs=("rgb", "depth"))
    met = alternating({"metrics": lambda: R.image_metrics(views["rgb"], views["depth"], gt_rgb, gt_depth)}, args.repeat)["metrics"]
    res["evaluate_views_8_office0"] = dict(stats(ev), per_view_ms=statistics.median(ev) / 8)
    res["image_metrics_8_office0"] = dict(stats(met), per_view_ms=statistics.median(met) / 8)
    print("evaluate_views", json.dumps(res["evaluate_views_8_office0"]), "metrics", json.dumps(res["image_metrics_8_office0"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

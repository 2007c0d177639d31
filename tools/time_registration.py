"""Time the model alignment on the device (naruto_amd.registration.FieldRegistrationHIP, csrc/naruto_sdfreg.hip) at office_0 size:
1200 x 680, f = 600, frames rendered by MeshSimHIP from the room-plus-sphere mesh of tools/time_tracked_run.py, the field after first-frame
mapping.  Recorded, alternating in ONE loop in one process: the whole ``align_device`` (defaults: levels 2 and 1, 6 iterations each), the
ungated ``rgbd_icp`` estimate (``init_state`` + the level loop) on the same frames, and the stages of one iteration at each level used
(points; query forward; query gradient; accumulate + finish; step).  Host clocks ending in a device synchronise; medians of --repeat (9)
with min .. max.  Nothing is asserted.

    python tools/time_registration.py [--out profiles/time_registration.json] [--n-lat 632]
"""
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
sys.path.insert(1, os.path.join(ROOT, "tools"))

import time_tracked_run as TT  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
from naruto_amd.odometry import RGBDOdometryHIP  # noqa: E402
from naruto_amd.registration import FieldRegistrationHIP  # noqa: E402
from naruto_amd.simulator import MeshSimHIP  # noqa: E402
from naruto_amd.slam import CoSLAMNarutoHIP  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--n-lat", type=int, default=632)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mesh = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    mesh = (mesh[0], mesh[1], TT.smooth_colours(mesh[0]))
    cfg = TT.config(True)
    slam = CoSLAMNarutoHIP(cfg, active_ray=True, num_frames=4, seed=0, device=dev, track=True)
    cam = {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
    sim = MeshSimHIP(mesh, cam, device=dev)
    p0 = TT.TR.start_pose().double().numpy().reshape(4, 4)
    p1 = p0.copy()
    p1[:3, 3] += (0.02, 0.01, 0.01)
    poses = torch.from_numpy(np.stack([p0, p1]).astype(np.float32))
    color, depth = sim.simulate_batch(poses)
    slam.online_recon_step(0, color[0], depth[0], poses[0])
    reg = FieldRegistrationHIP(slam.model, cfg, cam)
    od = RGBDOdometryHIP(cam, device=dev)
    m0, m1 = od.frame_maps(depth[0], color[0]), od.frame_maps(depth[1], color[1])
    est = torch.zeros(2, 4, 4, device=dev)
    pose6 = torch.zeros(6, device=dev)

    def align():
        est[1].copy_(poses[0].to(dev))                                       # the start: the previous frame's pose, 2.4 cm off
        reg.align_device(m1, est, 1, pose6)

    calls = {"align_device": align, "rgbd_icp_ungated_estimate": lambda: od.run_levels(m0, m1, od.init_state())}
    for level in reg.levels:
        calls[f"level_{level}_points"] = lambda level=level: reg.points(m1, level, gated=False)
        calls[f"level_{level}_query_fwd_and_bwd_points"] = lambda level=level: reg.query(level)
        calls[f"level_{level}_accumulate_and_finish"] = lambda level=level: reg.accumulate(level, gated=False)
        calls[f"level_{level}_step"] = lambda level=level: reg.pyramid.step(level, reg.state)
        calls[f"level_{level}_one_iteration"] = lambda level=level: reg._evaluate(m1, level, reg.sums, False)
    times = {k: [] for k in calls}
    for r in range(args.repeat + 2):                                         # two warm-up rounds
        for k, fn in calls.items():
            t = clock(fn)
            if r >= 2:
                times[k].append(t)
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()}
    res["pixels"] = {f"level_{l}": reg.pixels(l) for l in reg.levels}
    res["record_of_the_last_align"] = reg.record.cpu().tolist()
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "what": __doc__.split("\n\n")[0], "repeat": args.repeat, "image": [1200, 680], **res}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

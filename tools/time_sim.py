"""Time the mesh simulator on the device (naruto_amd.simulator) at the reference's sensor sizes: a 1200 x 680 pinhole frame, f = 600, and
a 1024 x 2048 panorama gathered from 512 x 512 cube faces, over synthetic.room_sphere_mesh tessellated to about 1.6 M faces with hashed
RGBA8 vertex colours, from ring poses inside the room.  Recorded: the RGB-D raster per pose next to the culling's depth-only raster of
the same poses in the same run (the yardstick; their ratio), one simulate(return_erp=True), one collision_probe, and the rate of
scattered 8-byte integer atomicMin (the winner raster's access pattern without the rasteriser) next to the 4-byte rate.

    python tools/time_sim.py [--out profiles/r13_time_sim.json] [--raster-poses 64] [--calls 20]

There is NO reference number to compare with: the reference renders with Habitat-Sim, which is not on this stack.  Times are wall clock
including the host side, ending in a device synchronise, warmed up, best of --repeat; nothing is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from naruto_amd import _lib  # noqa: E402
from naruto_amd import culling as CU  # noqa: E402
from naruto_amd import simulator as SIM  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
import cull_spec as CS  # noqa: E402
import sim_spec as SS  # noqa: E402


def timed(fn, repeat, warm=1):
    for _ in range(warm):
        fn()
    best, out = None, None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--raster-poses", type=int, default=64)
    ap.add_argument("--pose-chunk", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20, help="single-pose calls per timed window")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-lat", type=int, default=632)
    ap.add_argument("--face-w", type=int, default=512)
    ap.add_argument("--erp", type=int, nargs=2, default=(1024, 2048))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cam = {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}
    vn, fn = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    v, f = torch.from_numpy(vn).to(dev), torch.from_numpy(fn).to(dev)
    col = torch.from_numpy(SS.hashed_rgba(len(vn))).to(dev)
    poses = CS.ring_poses(args.raster_poses)
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(fn), "vertices": len(vn), "poses": len(poses), "pose_chunk": args.pose_chunk,
           "erp": list(args.erp), "face_w": args.face_w, "large_threshold": CU.DEFAULT_LARGE_THRESHOLD,
           "reference": "none: the reference renders with Habitat-Sim, which is not on this stack"}

    # scattered integer atomics: 4-byte cells (the depth-only raster) and 8-byte cells (the winner raster)
    lib = _lib.load()
    cells, lanes, iters = cam["H"] * cam["W"] * args.pose_chunk, 1 << 20, 16
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.full((cells,), 0x7F800000, dtype=torch.int32, device=dev)
    ms32, _ = timed(lambda: _lib.check(lib.naruto_debug_atomic_min_rate(cells, lanes, iters, buf.data_ptr(), stream)), args.repeat)
    buf = torch.full((cells,), 0x7F800000FFFFFFFF, dtype=torch.int64, device=dev)
    ms64, _ = timed(lambda: _lib.check(lib.naruto_debug_atomic_min64_rate(cells, lanes, iters, buf.data_ptr(), stream)), args.repeat)
    res["scattered_atomic_min"] = {"cells": cells, "atomics": lanes * iters, "ms_4_byte": ms32, "per_second_4_byte": lanes * iters / (ms32 * 1e-3),
                                   "ms_8_byte": ms64, "per_second_8_byte": lanes * iters / (ms64 * 1e-3), "rate_8_over_4_byte": ms32 / ms64}
    del buf

    # pinhole: the depth-only raster (the yardstick) and the RGB-D raster over the same poses, alternating
    sim = SIM.MeshSimHIP((v, f, col), cam, erp_hw=tuple(args.erp), face_w=args.face_w)
    depth_ms, rgbd_ms = [], []
    for _ in range(2):
        ms, d0 = timed(lambda: CU.render_depth(v, f, poses, cam, far=100.0, pose_chunk=args.pose_chunk, keep_inf=True), args.repeat)
        depth_ms.append(ms / len(poses))
        ms, out = timed(lambda: sim.simulate_batch(poses, pose_chunk=args.pose_chunk), args.repeat)
        rgbd_ms.append(ms / len(poses))
    same = bool(torch.equal(torch.where(torch.isinf(d0), torch.zeros_like(d0), d0), out[1]))
    res["pinhole"] = {"depth_only_ms_per_pose": min(depth_ms), "rgbd_ms_per_pose": min(rgbd_ms), "rgbd_over_depth_only": min(rgbd_ms) / min(depth_ms),
                      "both_rounds_depth_only": depth_ms, "both_rounds_rgbd": rgbd_ms, "depth_bits_equal": same,
                      "covered_pixel_share": float((out[1] > 0).float().mean()),
                      "note": "both include the output allocation and the pose upload; depth-only is the culling's 32-bit raster (the yardstick)"}
    del d0, out

    # one pose at a time, as the run loop calls it
    one = poses[0]
    n = args.calls
    ms, _ = timed(lambda: [sim.simulate(one, no_print=True) for _ in range(n)], args.repeat)
    res["simulate_ms"] = ms / n
    ms, out = timed(lambda: [sim.simulate(one, return_erp=True, no_print=True) for _ in range(n)], args.repeat)
    res["simulate_return_erp_ms"] = ms / n
    ms, probe = timed(lambda: [sim.collision_probe(one) for _ in range(n)], args.repeat)
    res["collision_probe_ms"] = ms / n
    erp_d = out[-1][3]
    res["collision_probe"] = {"dist_closest": probe[-1][0], "invalid_region_ratio": probe[-1][1],
                              "equals_erp_depth": bool(probe[-1][0] == float(erp_d.min()) and probe[-1][1] == int((erp_d > 1e6).sum()) / erp_d.numel())}
    print(json.dumps(res, indent=1))
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_sim.py: wall clock including the host side, ending in a device synchronise, warmed up, best of --repeat; milliseconds",
               "sensor_size": res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

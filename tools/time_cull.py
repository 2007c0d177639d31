"""Time mesh culling on the device (naruto_amd.culling) at the evaluation protocol's size: 1200 x 680, f = 600, a room-plus-sphere mesh
tessellated to about 1.6 M faces, 2 000 ring poses inside the room.  Recorded: the depth raster per pose (with the share of candidate
triangles that takes the workgroup route, per threshold of a small sweep, and the pose chunk), the vertex test per pose, the compaction,
the whole cull, and the rate of scattered 4-byte integer atomicMin (the rasteriser's depth minimum without the rasteriser).

    python tools/time_cull.py [--out profiles/r12_time_cull.json] [--poses 2000] [--raster-poses 64]

There is NO reference number to compare with: the reference's cull_mesh.py renders with pyrender (off-screen OpenGL), which is not on
this stack.  The numpy restatement's host time for one small pose (tests/cull_spec.py, 2 221 faces at 80 x 60) is recorded as context
only.  Times are wall clock including the host side, ending in a device synchronise, warmed up, best of --repeat; nothing is asserted."""
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
from naruto_amd import synthetic as syn  # noqa: E402
import cull_spec as CS  # noqa: E402


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


def large_share(v, f, pose, cam, threshold):
    """(candidate triangles, those whose box exceeds the threshold) under one pose, by the contract's box rule in torch on the device."""
    m = torch.from_numpy(pose).to(v.device)
    x = (v - m[:3, 3]) @ m[:3, :3]
    z = -x[:, 2]
    u, w = cam["cx"] + cam["fx"] * (x[:, 0] / z), cam["cy"] - cam["fy"] * (x[:, 1] / z)
    fl = f.long()
    front = (z > 0.01)[fl]
    uu, ww = u[fl], w[fl]
    x0, x1 = (uu.amin(1).ceil() - 1).clamp(min=0), (uu.amax(1).floor() + 1).clamp(max=cam["W"] - 1)
    y0, y1 = (ww.amin(1).ceil() - 1).clamp(min=0), (ww.amax(1).floor() + 1).clamp(max=cam["H"] - 1)
    px = ((x1 - x0 + 1).clamp(min=0) * (y1 - y0 + 1).clamp(min=0))
    px = torch.where(front.all(1), px, torch.where(front.any(1), torch.full_like(px, float(cam["H"] * cam["W"])), torch.zeros_like(px)))
    return int((px > 0).sum()), int((px > threshold).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--raster-poses", type=int, default=64)
    ap.add_argument("--pose-chunk", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--n-lat", type=int, default=632)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cam = {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}
    vn, fn = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    v, f = torch.from_numpy(vn).to(dev), torch.from_numpy(fn).to(dev)
    poses = CS.ring_poses(args.poses)
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(fn), "vertices": len(vn), "poses": args.poses, "pose_chunk": args.pose_chunk,
           "default_large_threshold": CU.DEFAULT_LARGE_THRESHOLD,
           "reference": "none: the reference's cull_mesh.py needs pyrender (off-screen OpenGL), which is not on this stack"}

    # scattered integer atomics
    lib = _lib.load()
    words, lanes, iters = cam["H"] * cam["W"] * args.pose_chunk, 1 << 20, 16
    buf = torch.full((words,), 0x7F800000, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms, _ = timed(lambda: _lib.check(lib.naruto_debug_atomic_min_rate(words, lanes, iters, buf.data_ptr(), stream)), args.repeat)
    res["scattered_atomic_min"] = {"words": words, "atomics": lanes * iters, "ms": ms, "atomics_per_second": lanes * iters / (ms * 1e-3)}
    del buf

    # depth raster, per threshold
    n_r = min(args.raster_poses, args.poses)
    sub = poses[:: max(1, args.poses // n_r)][:n_r]
    res["raster"] = {}
    for threshold in (128, CU.DEFAULT_LARGE_THRESHOLD, 2048, 8192):
        cand, large = zip(*(large_share(v, f, p, cam, threshold) for p in sub[:8]))
        ms, depth = timed(lambda: CU.render_depth(v, f, sub, cam, pose_chunk=args.pose_chunk, plan=CU.RasterPlan(threshold), keep_inf=True), args.repeat)
        res["raster"][str(threshold)] = {"poses": len(sub), "ms_per_pose": ms / len(sub), "candidate_triangles_per_pose": float(np.mean(cand)),
                                         "large_route_share_of_candidates": float(np.sum(large) / max(np.sum(cand), 1)), "pose_chunk": args.pose_chunk}
    res["raster_covered_pixel_share"] = float(torch.isfinite(depth).float().mean())
    del depth

    # vertex test per pose (against one chunk's depth maps), frustum only and with occlusion
    chunk = torch.from_numpy(sub[:args.pose_chunk]).to(dev)
    d = CU.render_depth(v, f, chunk, cam, pose_chunk=args.pose_chunk, keep_inf=True)
    ms, _ = timed(lambda: CU.observed_vertices(v, chunk, cam, depth=d), args.repeat)
    res["vertex_test_ms_per_pose"] = ms / len(chunk)
    ms, _ = timed(lambda: CU.observed_vertices(v, chunk, cam), args.repeat)
    res["vertex_test_frustum_only_ms_per_pose"] = ms / len(chunk)
    del d

    # the whole cull; the compaction alone = a frustum-only cull of one pose minus nothing else of size (its loop is one tiny launch)
    ms, out = timed(lambda: CU.cull_mesh((v, f), poses[:1], cam, remove_occlusion=False), args.repeat)
    res["compaction_with_one_frustum_pose_ms"] = ms
    ms, out = timed(lambda: CU.cull_mesh((v, f), poses, cam, pose_chunk=args.pose_chunk), 1, warm=0)
    res["whole_cull_ms"], res["whole_cull_ms_per_pose"] = ms, ms / args.poses
    res["kept_faces"], res["kept_vertices"] = len(out[1]), len(out[0])
    ms, out = timed(lambda: CU.cull_mesh((v, f), poses, cam, remove_occlusion=False, pose_chunk=args.pose_chunk), 1, warm=0)
    res["whole_cull_frustum_only_ms"] = ms

    # context only: the numpy restatement on one small pose
    sv, sf = CS.room_mesh()
    t = time.perf_counter()
    CS.render_depth(sv, sf, CS.ring_poses(4)[:1], CS.camera())
    res["host_restatement_context"] = {"ms": (time.perf_counter() - t) * 1e3, "faces": len(sf), "image": [80, 60],
                                       "note": "tests/cull_spec.py in numpy on this host, one pose; context only, not the reference"}
    print(json.dumps(res, indent=1))
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_cull.py: wall clock including the host side, ending in a device synchronise, warmed up, best of --repeat; milliseconds",
               "protocol_size": res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

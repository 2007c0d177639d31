"""Time the mesh simulator on the device (naruto_amd.simulator) at the reference's sensor sizes: a 1200 x 680 pinhole frame, f = 600, and
a 1024 x 2048 panorama gathered from 512 x 512 cube faces, over synthetic.room_sphere_mesh tessellated to about 1.6 M faces with hashed
RGBA8 vertex colours, from ring poses inside the room.  Recorded: the RGB-D raster per pose next to the culling's depth-only raster of
the same poses in the same run (the yardstick; their ratio), one simulate(return_erp=True), one collision_probe, and the rate of
scattered 8-byte integer atomicMin (the winner raster's access pattern without the rasteriser) next to the 4-byte rate.

    python tools/time_sim.py [--out profiles/r13_time_sim.json] [--raster-poses 64] [--calls 20]
    python tools/time_sim.py --textured [--out profiles/time_sim_textured.json] [--textures 4] [--texture-side 2048]

--textured: the same mesh with generated uv and a few procedural textures; the textured and the vertex-colour render alternate in one
loop (medians), and the build of the mip chains is timed.

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


def procedural_textures(n, side, seed=0):
    """n uint8 [side,side,4] images: a checker of 32-texel squares under per-texel noise, a tint per image."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    out = []
    for k in range(n):
        base = np.where(((ii >> 5) + (jj >> 5) + k) & 1, 200, 70)[..., None] * np.array([1.0, 0.8 - 0.15 * (k % 3), 0.6 + 0.1 * (k % 4)])
        rgb = np.clip(base + rng.integers(-40, 41, (side, side, 3)), 0, 255).astype(np.uint8)
        out.append(np.concatenate([rgb, np.full((side, side, 1), 255, dtype=np.uint8)], -1))
    return out


def textured(args):
    """--textured: the textured frame next to the vertex-colour frame of the same mesh and poses, alternating in one loop; medians of host
    clocks that end in a device synchronise.  uv are generated from the position (texels_per_metre texels of level 0 per metre), the
    material of a face from the height of its first vertex."""
    from naruto_amd.mesh import Material, TexturedMesh
    dev = torch.device("cuda:0")
    cam = {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}
    vn, fn = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    col = SS.hashed_rgba(len(vn))
    tiles = args.texels_per_metre / args.texture_side
    uv = (np.stack([vn[:, 0] + 0.37 * vn[:, 2], vn[:, 1] + 0.61 * vn[:, 2]], -1) * tiles).astype(np.float32)
    z = vn[fn[:, 0], 2]
    band = np.clip(((z - z.min()) / max(float(z.max() - z.min()), 1e-9) * args.textures).astype(np.int32), 0, args.textures - 1)
    images = procedural_textures(args.textures, args.texture_side)
    mesh = TexturedMesh(vn, fn, col, uv=uv, face_material=band, materials=[Material(k) for k in range(args.textures)], textures=images)
    poses = CS.ring_poses(args.raster_poses)

    def median_ms(fn_, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn_()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts)), ts

    SIM.texture_pyramid(images[:1], dev)                                            # (warm)
    build_ms, build_all = median_ms(lambda: SIM.texture_pyramid(images, dev), args.repeat)
    sim_t = SIM.MeshSimHIP(mesh, cam, erp_hw=tuple(args.erp), face_w=args.face_w, device=dev)
    sim_v = SIM.MeshSimHIP((torch.from_numpy(vn).to(dev), torch.from_numpy(fn).to(dev), torch.from_numpy(col).to(dev)), cam, erp_hw=tuple(args.erp), face_w=args.face_w)
    tex_one, col_one, tex_batch, col_batch = [], [], [], []
    for r in range(args.repeat + 1):                                                # (the first round warms up)
        for k in range(args.calls):
            one = poses[k % len(poses)]
            a = median_ms(lambda: sim_t.simulate(one, no_print=True), 1)[0]
            b = median_ms(lambda: sim_v.simulate(one, no_print=True), 1)[0]
            if r:
                tex_one.append(a)
                col_one.append(b)
        a = median_ms(lambda: sim_t.simulate_batch(poses, pose_chunk=args.pose_chunk), 1)[0] / len(poses)
        b = median_ms(lambda: sim_v.simulate_batch(poses, pose_chunk=args.pose_chunk), 1)[0] / len(poses)
        if r:
            tex_batch.append(a)
            col_batch.append(b)
    ct, dt = sim_t.simulate_batch(poses[:2], pose_chunk=2)[:2]
    cv, dv = sim_v.simulate_batch(poses[:2], pose_chunk=2)[:2]
    erp_t = median_ms(lambda: sim_t.simulate(poses[0], return_erp=True, no_print=True), args.repeat)[0]
    erp_v = median_ms(lambda: sim_v.simulate(poses[0], return_erp=True, no_print=True), args.repeat)[0]
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(fn), "vertices": len(vn), "poses": len(poses), "pose_chunk": args.pose_chunk,
           "textures": args.textures, "texture_side": args.texture_side, "texels_per_metre": args.texels_per_metre,
           "texel_words": int(sim_t.tex.texels.numel()), "pyramid_build_ms": build_ms, "pyramid_build_ms_all": build_all,
           "simulate_ms": {"textured": float(np.median(tex_one)), "vertex_colour": float(np.median(col_one)),
                           "textured_over_vertex_colour": float(np.median(tex_one) / np.median(col_one)), "samples_each": len(tex_one)},
           "batch_ms_per_pose": {"textured": float(np.median(tex_batch)), "vertex_colour": float(np.median(col_batch)),
                                 "textured_over_vertex_colour": float(np.median(tex_batch) / np.median(col_batch)), "samples_each": len(tex_batch)},
           "simulate_return_erp_ms": {"textured": erp_t, "vertex_colour": erp_v},
           "depth_bits_equal": bool(torch.equal(dt.view(torch.int32), dv.view(torch.int32))), "colour_differs": bool((ct != cv).any()),
           "covered_pixel_share": float((dt > 0).float().mean()),
           "reference": "none: the reference renders with Habitat-Sim, which is not on this stack"}
    print(json.dumps({k: v for k, v in res.items() if k != "pyramid_build_ms_all"}, indent=1))
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_sim.py --textured: the textured and the vertex-colour render alternating in one loop; medians of host clocks that end in a "
                       "device synchronise, the first round discarded; milliseconds",
               "sensor_size": res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--textured", action="store_true", help="time the textured render next to the vertex-colour render (and the pyramid build) instead")
    ap.add_argument("--textures", type=int, default=4)
    ap.add_argument("--texture-side", type=int, default=2048)
    ap.add_argument("--texels-per-metre", type=float, default=512.0)
    ap.add_argument("--raster-poses", type=int, default=64)
    ap.add_argument("--pose-chunk", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20, help="single-pose calls per timed window")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-lat", type=int, default=632)
    ap.add_argument("--face-w", type=int, default=512)
    ap.add_argument("--erp", type=int, nargs=2, default=(1024, 2048))
    args = ap.parse_args()
    if args.textured:
        return textured(args)
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

"""Time the depth odometry on the device (naruto_amd.odometry.DepthOdometryHIP, csrc/naruto_odom.hip) at office_0 size: 1200 x 680,
f = 600, frames rendered by MeshSimHIP from the room-plus-sphere mesh of tools/time_tracked_run.py (n_lat = 632: 1 595 181 faces).
Recorded:

  * the frame maps of one frame (one launch);
  * one iteration per level: state init + accumulate (two launches) + step, from the identity, for a 3 cm / 2 degree motion;
  * a whole estimate (the fixed sequence of 1 + 3 x (10 + 5 + 4) launches), and the maps + estimate + pose_predict_relative a tracked frame
    adds, next to the tracked frame's device time recorded in profiles/time_tracked_run.json;
  * the basin at this size: the largest step of a fixed ladder of yaws about the camera's y axis, and of translations along
    (0.6, 0.3, -0.74), that one estimate from the identity recovers to 5 mm / 0.25 degrees.

    python tools/time_odometry.py [--out profiles/time_odometry.json] [--n-lat 632]
    python tools/time_odometry.py --rgbd [--out profiles/time_odometry_rgbd.json]
    python tools/time_odometry.py --gate [--out profiles/time_odometry_gate.json]
    python tools/time_odometry.py --anchor [--out profiles/time_odometry_anchor.json]

With --rgbd only this is recorded: the frame maps and a whole estimate of the depth odometry and of the RGB-D odometry
(naruto_amd.odometry.RGBDOdometryHIP) on the same two frames of the mesh coloured by a smooth function of position, the four calls
alternating in one loop.  With --gate only this: the gated estimate (scored starts and a verdict, ``estimate_gated_device`` from a pose
tensor) and the ungated one (``init_state`` + the level loop, today's path) alternating in one loop, for both odometry classes, and
``score`` alone at K = 1, 2 and 4 at the coarsest level and at level 0; medians with their spread (min, max), the ratio gated / ungated
and whether the difference exceeds twice the ungated call's own spread.  With --anchor only this: the anchored estimate
(``estimate_anchored_device``) on a reference ring of 1 and of 4 slots, every slot holding a frame, and the gated estimate (the baseline)
alternating in one loop for both classes; the candidates and the score over the references alone; the promote launch with the decision
word set (the copy of one maps block) and clear; the same figures and the same rule for claiming a cost.

Host wall clock ending in a device synchronise, every shape warmed up first, the MEDIAN of --repeat.  Nothing is asserted."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naruto_amd import pose_chain as PC  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
from naruto_amd.odometry import DepthOdometryHIP, RGBDOdometryHIP  # noqa: E402
from naruto_amd.planner import compute_camera_pose  # noqa: E402
from naruto_amd.simulator import MeshSimHIP  # noqa: E402

YAWS_DEG = (2.0, 5.0, 10.0, 15.0, 20.0, 30.0, 40.0, 60.0)
STEPS_M = (0.03, 0.1, 0.2, 0.4, 0.8, 1.2)
ALONG = (0.6, 0.3, -0.74)
BOUND_M, BOUND_DEG = 5e-3, 0.25


def timed(fn, repeat, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return statistics.median(times) * 1e3


def rotation(axis, theta):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def motion(axis, deg, dist):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, math.radians(deg))
    T[:3, 3] = dist * np.asarray(ALONG) / np.linalg.norm(ALONG)
    return T


def error(T, ref):
    R = T[:3, :3].T @ ref[:3, :3]
    return float(np.linalg.norm(T[:3, 3] - ref[:3, 3])), math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))))


def rgbd(args, dev, cam):
    """--rgbd: the frame maps and a whole estimate of DepthOdometryHIP and RGBDOdometryHIP on the same two frames (3 cm / 2 degrees), the
    two alternating inside one timing loop so that both see the same machine state; the mesh coloured by a smooth function of position."""
    from time_tracked_run import smooth_colours
    v, f = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)[:2]
    sim = MeshSimHIP((v, f, smooth_colours(v)), cam, device=dev)
    base = np.eye(4)
    pos, at = np.array([2.0, 4.0, 1.2]), np.array([3.0, 2.5, 1.4])
    base[:3, :3], base[:3, 3] = compute_camera_pose(pos, at), pos
    poses = np.stack([base, base @ motion((0, 1, 0), 2.0, 0.03)]).astype(np.float32)
    frames = [sim.simulate(p, no_print=True) for p in poses]
    color, depth = [c.to(dev) for c, _ in frames], [d.to(dev) for _, d in frames]
    rel = np.linalg.inv(poses[0].astype(np.float64)) @ poses[1].astype(np.float64)
    dod, rod = DepthOdometryHIP(cam, device=dev), RGBDOdometryHIP(cam, device=dev)
    dprev, dcur, rprev, rcur = dod.frame_maps(depth[0]), dod.new_maps(), rod.frame_maps(depth[0], color[0]), rod.new_maps()
    calls = {"depth_frame_maps_ms": lambda: dod.frame_maps(depth[1], out=dcur), "rgbd_frame_maps_ms": lambda: rod.frame_maps(depth[1], color[1], out=rcur),
             "depth_estimate_ms": lambda: dod.estimate_device(dprev, dcur), "rgbd_estimate_ms": lambda: rod.estimate_device(rprev, rcur)}
    times = {k: [] for k in calls}
    for k, fn in calls.items():
        fn()
    for _ in range(args.repeat):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(f), "levels": rod.levels, "iters_coarse_to_fine": list(rod.iters),
           "photo_weight": float(rod.photo.weight), "photo_max_diff": float(rod.photo.max_diff), "repeat": args.repeat}
    res.update({k: statistics.median(v) * 1e3 for k, v in times.items()})
    for name, got in (("depth", dod.read_state()), ("rgbd", rod.read_state())):
        dm, dd = error(got.transformation, rel)
        res[name + "_estimate_3cm_2deg"] = {"error_mm": dm * 1e3, "error_deg": dd, "status": got.status, "iterations": got.iterations, "inliers": got.inliers,
                                            "rmse": got.rmse}
    res["rgbd_estimate_3cm_2deg"].update(geometric_rows=rod.read_state().geometric_rows, photometric_rows=rod.read_state().photometric_rows)
    return res


def gate(args, dev, cam):
    """--gate: gated and ungated estimates alternating in one loop, and the score kernel alone (module docstring)."""
    from time_tracked_run import smooth_colours
    v, f = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)[:2]
    sim = MeshSimHIP((v, f, smooth_colours(v)), cam, device=dev)
    base = np.eye(4)
    pos, at = np.array([2.0, 4.0, 1.2]), np.array([3.0, 2.5, 1.4])
    base[:3, :3], base[:3, 3] = compute_camera_pose(pos, at), pos
    step = motion((0, 1, 0), 2.0, 0.03)
    poses = np.stack([base @ np.linalg.inv(step), base, base @ step]).astype(np.float32)        # frames 0, 1, 2 of a steady motion
    frames = [sim.simulate(p, no_print=True) for p in poses[1:]]
    color, depth = [c.to(dev) for c, _ in frames], [d.to(dev) for _, d in frames]
    rel = np.linalg.inv(poses[1].astype(np.float64)) @ poses[2].astype(np.float64)
    est = torch.from_numpy(poses).to(dev)
    ods = {"depth": DepthOdometryHIP(cam, device=dev), "rgbd": RGBDOdometryHIP(cam, device=dev)}
    maps = {"depth": (ods["depth"].frame_maps(depth[0]), ods["depth"].frame_maps(depth[1])),
            "rgbd": (ods["rgbd"].frame_maps(depth[0], color[0]), ods["rgbd"].frame_maps(depth[1], color[1]))}
    calls = {}
    for name, od in ods.items():
        mp, mc = maps[name]
        calls[name + "_ungated_ms"] = lambda od=od, mp=mp, mc=mc: od.run_levels(mp, mc, od.init_state(est=est, i=2, const_speed=True))
        calls[name + "_gated_ms"] = lambda od=od, mp=mp, mc=mc: od.estimate_gated_device(mp, mc, est=est, i=2)
        four = np.stack([np.eye(4), step, motion((0, 1, 0), -2.0, 0.0), motion((0, 1, 0), 4.0, 0.06)])
        for level in (od.levels - 1, 0):
            for K in (1, 2, 4):
                calls[f"{name}_score_level{level}_K{K}_ms"] = lambda od=od, mp=mp, mc=mc, K=K, level=level: od.score(mp, mc, four[:K], level=level)
    times = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    for _ in range(args.repeat):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(f), "repeat": args.repeat}
    for k, vals in times.items():
        res[k] = {"median": statistics.median(vals) * 1e3, "min": min(vals) * 1e3, "max": max(vals) * 1e3}
    for name, od in ods.items():
        un, ga = res[name + "_ungated_ms"], res[name + "_gated_ms"]
        spread = un["max"] - un["min"]
        res[name + "_gated_over_ungated"] = {"ratio": ga["median"] / un["median"], "difference_ms": ga["median"] - un["median"], "ungated_spread_ms": spread,
                                             "exceeds_twice_the_ungated_spread": bool(ga["median"] - un["median"] > 2.0 * spread)}
        od.estimate_gated_device(*maps[name], est=est, i=2)
        rec = od.record.cpu().numpy()
        dm, dd = error(od.read_state().transformation, rel)
        res[name + "_gated_estimate_3cm_2deg"] = {"error_mm": dm * 1e3, "error_deg": dd, "record": [float(x) for x in rec]}
    return res


def anchor(args, dev, cam):
    """--anchor: the anchored estimate (a reference ring of 1 and of 4 slots, every slot holding a frame) and the gated one alternating in
    one loop, for both odometry classes; the score over the references alone and the promote copy (module docstring)."""
    from naruto_amd.odometry import AnchorPolicy
    from time_tracked_run import smooth_colours
    v, f = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)[:2]
    sim = MeshSimHIP((v, f, smooth_colours(v)), cam, device=dev)
    base = np.eye(4)
    pos, at = np.array([2.0, 4.0, 1.2]), np.array([3.0, 2.5, 1.4])
    base[:3, :3], base[:3, 3] = compute_camera_pose(pos, at), pos
    step = motion((0, 1, 0), 2.0, 0.03)
    chain = [base]
    for _ in range(4):                                                      # frames 0 .. 4 of a steady motion; frame 4 is the current one
        chain.append(chain[-1] @ step)
    poses = np.stack(chain).astype(np.float32)
    frames = [sim.simulate(p, no_print=True) for p in poses]
    color, depth = [c.to(dev) for c, _ in frames], [d.to(dev) for _, d in frames]
    est = torch.from_numpy(np.concatenate([poses, poses[-1:]])).to(dev)
    rel = np.linalg.inv(poses[3].astype(np.float64)) @ poses[4].astype(np.float64)
    ods = {"depth": DepthOdometryHIP(cam, device=dev), "rgbd": RGBDOdometryHIP(cam, device=dev)}
    calls, checks = {}, {}
    for name, od in ods.items():
        maps = [od.frame_maps(depth[k], color[k]) if name == "rgbd" else od.frame_maps(depth[k]) for k in range(5)]
        rings = {}
        for slots in (1, 4):
            ring = od.new_anchor(AnchorPolicy(slots=slots))
            for s in range(slots):                                          # slot s holds frame 3 - s: the frame before, then older ones
                ring.ring[s].copy_(maps[3 - s])
            words = [0, 0, 0, 0] + [3 - s for s in range(slots)] + [-1] * (8 - slots)
            rings[slots] = (ring, torch.tensor(words, dtype=torch.int32, device=dev))
        record, arec = torch.zeros(16, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.float64, device=dev)
        calls[name + "_gated_ms"] = lambda od=od, maps=maps: od.estimate_gated_device(maps[3], maps[4], est=est, i=4)

        def anchored(od=od, maps=maps, record=record, arec=arec, ring=None, head=None):
            ring.head.copy_(head)                                           # the same ring every time: a promotion of the last call is undone
            od.estimate_anchored_device(ring, maps[4], est, 4, None, record, arec)
        for slots, (ring, head) in rings.items():
            calls[f"{name}_anchored_slots{slots}_ms"] = lambda fn=anchored, ring=ring, head=head: fn(ring=ring, head=head)

            def refs(od=od, maps=maps, ring=ring, head=head):
                ring.head.copy_(head)
                od.anchor_candidates(ring, est, 4)
                od.score_refs(ring, maps[4])
            calls[f"{name}_score_refs_slots{slots}_ms"] = refs
        # the promote launch alone, on a ring of its own (the copy overwrites a slot): the decision word set, and clear
        spare = od.new_anchor(AnchorPolicy(slots=4))
        taken = torch.tensor([1, 0, 0, 1, 3, 2] + [-1] * 6, dtype=torch.int32, device=dev)
        clear = torch.tensor([1, 0, 0, 0, 3, 2] + [-1] * 6, dtype=torch.int32, device=dev)

        def promote(od=od, maps=maps, spare=spare, words=None):
            spare.head.copy_(words)
            od.anchor_promote(spare, maps[4])
        calls[name + "_promote_copy_ms"] = lambda fn=promote, words=taken: fn(words=words)
        calls[name + "_promote_not_taken_ms"] = lambda fn=promote, words=clear: fn(words=words)
        checks[name] = (od, maps, rings)
    times = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    for _ in range(args.repeat):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(f), "repeat": args.repeat}
    for k, vals in times.items():
        res[k] = {"median": statistics.median(vals) * 1e3, "min": min(vals) * 1e3, "max": max(vals) * 1e3}
    for name, (od, maps, rings) in checks.items():
        ga = res[name + "_gated_ms"]
        spread = ga["max"] - ga["min"]
        res[name + "_maps_block_MB"] = od.maps_bytes / 1e6
        for slots, (ring, head) in rings.items():
            an = res[f"{name}_anchored_slots{slots}_ms"]
            res[f"{name}_anchored_slots{slots}_over_gated"] = {"ratio": an["median"] / ga["median"], "difference_ms": an["median"] - ga["median"], "gated_spread_ms": spread,
                                                               "exceeds_twice_the_gated_spread": bool(an["median"] - ga["median"] > 2.0 * spread)}
            ring.head.copy_(head)
            state = od.estimate_anchored_device(ring, maps[4], est, 4)
            a, rec = ring.record.cpu().numpy(), od.record.cpu().numpy()
            ref = int(a[1])
            want = np.linalg.inv(poses[ref].astype(np.float64)) @ poses[4].astype(np.float64)
            dm, dd = error(state.cpu().numpy()[:16].reshape(4, 4), want)
            res[f"{name}_anchored_slots{slots}_estimate"] = {"reference_frame": ref, "error_mm": dm * 1e3, "error_deg": dd, "anchor_record": [float(x) for x in a],
                                                             "record": [float(x) for x in rec]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--n-lat", type=int, default=632)
    ap.add_argument("--rgbd", action="store_true", help="depth-only and RGB-D odometry alternating in one run (write to profiles/time_odometry_rgbd.json)")
    ap.add_argument("--gate", action="store_true", help="gated and ungated estimates alternating in one run, and the score kernel alone (write to profiles/time_odometry_gate.json)")
    ap.add_argument("--anchor", action="store_true", help="anchored and gated estimates alternating in one run, the score over the references and the promote "
                                                          "copy alone (write to profiles/time_odometry_anchor.json)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_odometry.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    cam = {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}
    if args.anchor:
        res = anchor(args, dev, cam)
        print(json.dumps(res, indent=1))
        if args.out:
            doc = {"device": torch.cuda.get_device_name(0),
                   "what": "tools/time_odometry.py --anchor: host wall clock ending in a device synchronise, warmed up, all calls alternating in one loop, "
                           "median (min, max) of --repeat; milliseconds.  The baseline is estimate_gated_device; every anchored and score_refs call "
                           "includes a 48-byte device copy that puts the ring's head back", "office_0_size": res}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(doc, fh, indent=1)
                fh.write("\n")
        return
    if args.gate:
        res = gate(args, dev, cam)
        print(json.dumps(res, indent=1))
        if args.out:
            doc = {"device": torch.cuda.get_device_name(0),
                   "what": "tools/time_odometry.py --gate: host wall clock ending in a device synchronise, warmed up, all calls alternating in one loop, "
                           "median (min, max) of --repeat; milliseconds.  score_* include the host's copy of the K candidates", "office_0_size": res}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(doc, fh, indent=1)
                fh.write("\n")
        return
    if args.rgbd:
        res = rgbd(args, dev, cam)
        print(json.dumps(res, indent=1))
        if args.out:
            doc = {"device": torch.cuda.get_device_name(0),
                   "what": "tools/time_odometry.py --rgbd: host wall clock ending in a device synchronise, warmed up, the four calls alternating, median of "
                           "--repeat; milliseconds", "office_0_size": res}
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(doc, fh, indent=1)
                fh.write("\n")
        return
    mesh = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    sim = MeshSimHIP(mesh, cam, device=dev)
    base = np.eye(4)
    pos, at = np.array([2.0, 4.0, 1.2]), np.array([3.0, 2.5, 1.4])
    base[:3, :3], base[:3, 3] = compute_camera_pose(pos, at), pos
    rels = [motion((0, 1, 0), 2.0, 0.03)] + [motion((0, 1, 0), a, 0.0) for a in YAWS_DEG] + [motion((0, 1, 0), 0.0, d) for d in STEPS_M]
    poses = torch.from_numpy(np.stack([base] + [base @ r for r in rels]).astype(np.float32))
    depth = torch.stack([sim.simulate(p.numpy(), no_print=True)[1].to(dev) for p in poses])
    # the relative motions as the float32 poses carry them
    gt = poses.double().numpy()
    rels = [np.linalg.inv(gt[0]) @ gt[k] for k in range(1, len(gt))]
    od = DepthOdometryHIP(cam, device=dev)
    res = {"image": [cam["W"], cam["H"]], "focal": cam["fx"], "faces": len(mesh[1]), "levels": od.levels, "iters_coarse_to_fine": list(od.iters),
           "valid_depth_fraction": float((depth[0] > 0).float().mean())}
    maps_prev, maps_cur = od.frame_maps(depth[0]), od.new_maps()
    res["frame_maps_ms"] = timed(lambda: od.frame_maps(depth[1], out=maps_cur), args.repeat)
    for level in range(od.levels):
        def one(level=level):
            od.init_state(None)
            od.accumulate(level, maps_prev, maps_cur)
            od.step(level)
        res[f"level_{level}_init_accumulate_step_ms"] = timed(one, args.repeat)
    res["state_init_ms"] = timed(lambda: od.init_state(None), args.repeat)
    res["estimate_ms"] = timed(lambda: od.estimate_device(maps_prev, maps_cur), args.repeat)
    est = torch.zeros(4, 4, 4, device=dev)
    est[0] = poses[0].to(dev)
    pose6 = torch.zeros(6, device=dev)

    def added():
        od.frame_maps(depth[1], out=maps_cur)
        PC.pose_predict_relative(est, 1, od.estimate_device(maps_prev, maps_cur), pose6)
    res["maps_estimate_predict_ms"] = timed(added, args.repeat)
    got = od.read_state()
    dm, dd = error(got.transformation, rels[0])
    res["estimate_3cm_2deg"] = {"error_mm": dm * 1e3, "error_deg": dd, "status": got.status, "iterations": got.iterations, "inliers": got.inliers, "rmse": got.rmse}
    tracked = os.path.join(ROOT, "profiles", "time_tracked_run.json")
    if os.path.exists(tracked):
        with open(tracked) as fh:
            res["tracked_frame_device_chain_ms_device_from_time_tracked_run"] = json.load(fh)["office_0_size"]["frames"]["tracked_frame_device_chain_ms_device"]
    basin = {"bound": {"mm": BOUND_M * 1e3, "deg": BOUND_DEG}, "yaw_deg": [], "translation_m": []}
    for name, ladder, first in (("yaw_deg", YAWS_DEG, 2), ("translation_m", STEPS_M, 2 + len(YAWS_DEG))):
        largest = None
        for k, s in enumerate(ladder):
            out = od.estimate(depth[0], depth[first + k])
            dm, dd = error(out.transformation, rels[first + k - 1])
            ok = dm <= BOUND_M and dd <= BOUND_DEG
            basin[name].append({"step": s, "error_mm": dm * 1e3, "error_deg": dd, "recovered": ok, "status": out.status})
            if all(e["recovered"] for e in basin[name]):               # the basin ends at the first step that is lost
                largest = s
        basin[name + "_largest_recovered"] = largest
    res["basin"] = basin
    print(json.dumps(res, indent=1))
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_odometry.py: host wall clock ending in a device synchronise, warmed up, median of --repeat; milliseconds", "office_0_size": res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

"""Time camera tracking during a run (CoSLAMNarutoHIP(track=True)) at office_0 size: 1200 x 680, f = 600, the room-plus-sphere mesh and
the mapping schedule of tools/time_run.py, tracking with replica_coslam.yaml's settings (1 024 pixels, 10 iterations).  Recorded:

  * a tracked frame that does not map, end to end: the device pose chain (naruto_pose_predict, TrackerHIP.track_device,
    naruto_pose_commit) against the same frame through the host path that existed before it (tracking.predict_current_pose in torch,
    TrackerHIP.track -- the initial pose goes to the CPU for the fp64 log map --, the relative pose in torch): the time until the host
    has the step behind it (what the run loop pays) and the time until the device has finished;
  * a mapped frame's global_BA with pose refinement, the initial (omega, t) from naruto_pose_log on the device against
    pose_init_on_device=False (matrices_to_pose6 on the host);
  * a --steps (200) step run with simulator, tracker, SLAM and planner: steps per second, the SLAM phase split into mapped frames and
    the others, the trajectory error of the estimate and the motion per step the planner commands (against what one tracking call
    can cover: iter x lr).

    python tools/time_tracked_run.py [--out profiles/time_tracked_run.json] [--steps 200] [--n-lat 632] [--motion-prior depth_icp | rgbd_icp [--prior-gate [--prior-anchor]] [--model-align]]

With --motion-prior only the run is made, with CoSLAMNarutoHIP(motion_prior=...), and it is MERGED into the output file as
office_0_size.run_motion_prior_<name>, beside the run of the default prior (--no-const-speed: tracking.const_speed off, key suffix
_const_speed_off; --prior-gate: _gated; --prior-anchor: the reference ring of naruto_amd.odometry on, _anchored, with its per-frame records; --model-align: the model alignment of naruto_amd.registration on, _aligned, with its per-frame
records).  rgbd_icp needs an image: the tool's mesh has no colours, so its vertices are then coloured by a smooth function of position.

Host timers (time.perf_counter), medians over --repeat.  Nothing is asserted.  There is NO reference number: the reference's loop needs
Habitat-Sim and tiny-cuda-nn, neither of which is on this stack."""
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

import time_run as TR  # noqa: E402  (tools/time_run.py: the scene, the config and the timers)
from naruto_amd import pose_chain as PC  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
from naruto_amd import tracking  # noqa: E402
from naruto_amd.planner import NarutoPlannerHIP, compute_camera_pose  # noqa: E402
from naruto_amd.run import run_exploration  # noqa: E402
from naruto_amd.simulator import MeshSimHIP  # noqa: E402
from naruto_amd.slam import CoSLAMNarutoHIP  # noqa: E402


def smooth_colours(vertices):
    """float32 [V,3] in 0 .. 1: a smooth function of position with structure at the scale of a metre (a mesh without colours renders white)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    c = np.stack([0.5 + 0.25 * np.sin(2.3 * x + 1.1 * y + 0.4) + 0.2 * np.cos(1.7 * z - 0.8 * y),
                  0.5 + 0.25 * np.cos(1.9 * y - 1.3 * z + 0.2) + 0.2 * np.sin(2.9 * x + 0.6 * z),
                  0.5 + 0.25 * np.sin(2.1 * z + 0.9 * x - 0.5) + 0.2 * np.cos(2.6 * y + 1.2 * x)], -1)
    return np.clip(c, 0.0, 1.0).astype(np.float32)


def config(const_speed=True):
    cfg = TR.config()
    cfg["tracking"] = dict(tracking.TRACKING_DEFAULTS, disable=False)
    if not const_speed:
        cfg["tracking"]["const_speed"] = False
    return cfg


def arc(n):
    """A slow arc from tools/time_run.py's start pose: 5 mm per frame, looking at the sphere."""
    out = []
    for k in range(n):
        pos, at = np.array([2.0 + 0.005 * k, 4.0 - 0.002 * k, 1.2]), np.array([3.0, 2.5, 1.4])
        p = np.eye(4, dtype=np.float32)
        p[:3, :3], p[:3, 3] = compute_camera_pose(pos, at).astype(np.float32), pos
        out.append(torch.from_numpy(p))
    return torch.stack(out)


def host_and_device_ms(fn, repeat):
    """Medians of (time until fn returns, time until the device has finished it)."""
    fn()
    host, dev = [], []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t) * 1e3)
        torch.cuda.synchronize()
        dev.append((time.perf_counter() - t) * 1e3)
    return statistics.median(host), statistics.median(dev)


def frames(args, dev, mesh):
    """Frames 0 .. 10 of the arc through a tracked SLAM object; then frame 11 (tracked, not mapped) and frame 10's global_BA, timed."""
    cfg = config()
    slam = CoSLAMNarutoHIP(cfg, active_ray=True, num_frames=16, seed=args.seed, device=dev, track=True)
    sim = MeshSimHIP(mesh, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}, device=dev)
    traj = arc(12)
    for i in range(11):
        color, depth = sim.simulate(traj[i].numpy(), no_print=True)
        slam.online_recon_step(i, color, depth, traj[i])
    color, depth = sim.simulate(traj[11].numpy(), no_print=True)
    est, rel, trk, every = slam.est_c2w_data.tensor, slam.est_c2w_data_rel.tensor, slam.tracker, int(cfg["mapping"]["keyframe_every"])
    const_speed = bool(slam.tracking["const_speed"])

    def device_chain():
        PC.pose_predict(est, 11, const_speed, trk.pose_init)
        PC.pose_commit(est, rel, 11, every, trk.track_device(slam.rays_d, color, depth))

    def host_path():
        init = tracking.predict_current_pose(est[9], est[10], const_speed)
        c2w = trk.track(slam.rays_d, color, depth, init)
        est[11].copy_(c2w)
        rel[11].copy_(c2w @ torch.linalg.inv(est[10]))
    out = {"tracking": {k: slam.tracking[k] for k in ("iter", "sample", "const_speed")}}
    out["tracked_frame_device_chain_ms_host"], out["tracked_frame_device_chain_ms_device"] = host_and_device_ms(device_chain, args.repeat)
    out["tracked_frame_host_path_ms_host"], out["tracked_frame_host_path_ms_device"] = host_and_device_ms(host_path, args.repeat)
    # frame 10's global_BA again: three keyframes stored (0, 5, 10), poses 0, 5, 10 and the current one last
    poses_all = torch.cat([est[0:11:every], est[10:11]], 0)
    n_valid = slam._read_n_valid()
    for on_device in (True, False):
        def call(on_device=on_device):
            slam.ba.global_BA(None, poses_all, uncert_vol=slam.cached_uncert, n_valid=n_valid, optimize_poses=True, pose_init_on_device=on_device)
        key = "global_ba_refining_pose_init_%s_ms" % ("device" if on_device else "host")
        out[key + "_host"], out[key + "_device"] = host_and_device_ms(call, args.repeat)
    out["global_ba_poses"] = int(poses_all.shape[0])
    return out


class OneLine:
    """A list that ``dump_doc`` writes on one line."""

    def __init__(self, values):
        self.values = values


def sig(values, digits=4):
    """Nested lists of numbers at ``digits`` significant digits (integers stay integers): what a per-frame table needs, a fifth of the bytes."""
    if isinstance(values, (list, tuple)):
        return [sig(v, digits) for v in values]
    return int(values) if float(values).is_integer() else float(f"{float(values):.{digits}g}")


def dump_doc(doc, fh):
    """The document with indent 1 as ever; the per-frame tables and frame lists of the ``_aligned`` runs one line each, so that two runs of
    199 frames add some twenty lines to the file and not thirteen thousand."""
    def wrap(v):
        if isinstance(v, dict):
            return {k: wrap(x) for k, x in v.items()}
        return OneLine(v) if isinstance(v, list) else v
    out = dict(doc, office_0_size={k: ({a: wrap(b) if a.endswith("per_frame_from_1") or a.endswith("failed_frames") else b for a, b in run.items()}
                                       if k.endswith("_aligned") else run) for k, run in doc["office_0_size"].items()})
    lines = []

    def token(o):
        lines.append(json.dumps(o.values, separators=(",", ":")))
        return f"@@{len(lines) - 1}@@"
    text = json.dumps(out, indent=1, default=token)
    for n, line in enumerate(lines):
        text = text.replace(f'"@@{n}@@"', line)
    fh.write(text + "\n")


def whole_run(args, dev, mesh):
    cfg = config(not args.no_const_speed)
    np.random.seed(args.seed)
    slam = CoSLAMNarutoHIP(cfg, active_ray=True, num_frames=args.steps, seed=args.seed, device=dev, track=True, motion_prior=args.motion_prior,
                           prior_gate=True if args.prior_gate else None, model_align=True if args.model_align else None,
                           prior_anchor=True if args.prior_anchor else None)
    sim = MeshSimHIP(mesh, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}, device=dev)
    planner = NarutoPlannerHIP(dataset="NARUTO", device=dev)
    planner.update_sim(sim)
    planner.init_data(cfg["mapping"]["bound"])
    planner.init_local_planner()
    slam_t = []
    step0 = slam.online_recon_step

    def timed_step(*a, **k):
        t = time.perf_counter()
        out = step0(*a, **k)
        slam_t.append(time.perf_counter() - t)
        return out
    slam.online_recon_step = timed_step
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prior_poses, tracked_poses = [], []

    def on_step(i, c2w, vols, state):
        """--prior-gate: the pose the prior handed the tracker (est[i-1] @ T, as both stand at the end of the step) and the tracked pose."""
        if i > 0 and args.prior_anchor:                                     # T is relative to the reference the anchor record names
            ref = torch.index_select(slam.est_c2w_data.tensor, 0, slam.anchor_log[i, 1:2].long())[0]
            prior_poses.append(ref.double() @ slam.odometry.state[:16].view(4, 4))
            tracked_poses.append(slam.est_c2w_data.tensor[i].double().clone())
        elif i > 0:
            prior_poses.append(slam.est_c2w_data.tensor[i - 1].double() @ slam.odometry.state[:16].view(4, 4))
            tracked_poses.append(slam.est_c2w_data.tensor[i].double().clone())
    out = run_exploration(slam, sim, planner, TR.start_pose(), args.steps, on_step=on_step if args.prior_gate else None)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    loop = sum(v["total_s"] for v in out["timing"].values())
    mapped = set(out["fresh"])
    err = (out["est_poses"][:, :3, 3].double() - out["poses"][:, :3, 3].double()).norm(dim=1)
    # what the planner asks of the tracker: the commanded motion between consecutive frames (one tracking call covers about
    # iter x lr_trans metres and iter x lr_rot radians)
    gt = out["poses"].double()
    move = (gt[1:, :3, 3] - gt[:-1, :3, 3]).norm(dim=1) * 100.0
    cos = ((gt[1:, :3, :3].transpose(1, 2) @ gt[:-1, :3, :3]).diagonal(dim1=1, dim2=2).sum(1) - 1.0) / 2.0
    turn = torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0)))
    reach = {"translation_cm": slam.tracking["iter"] * slam.tracking["lr_trans"] * 100.0,
             "rotation_deg": float(np.degrees(slam.tracking["iter"] * slam.tracking["lr_rot"]))}
    gated = {}
    if args.prior_gate:
        def errors(poses):
            p = torch.stack(poses).cpu()
            g = gt[1:]
            c = ((p[:, :3, :3].transpose(1, 2) @ g[:, :3, :3]).diagonal(dim1=1, dim2=2).sum(1) - 1.0) / 2.0
            return ((p[:, :3, 3] - g[:, :3, 3]).norm(dim=1) * 100.0).tolist(), torch.rad2deg(torch.acos(c.clamp(-1.0, 1.0))).tolist()
        log = out["prior_log"]
        failed = [int(i) for i in torch.nonzero(log[1:, 0] == 0.0).flatten() + 1]
        pe, te = errors(prior_poses), errors(tracked_poses)
        first = lambda cm: next((i + 1 for i, e in enumerate(cm) if e > 10.0), None)        # noqa: E731  the first frame more than 10 cm off
        gated = {"prior_failed_frames": failed, "first_frame_prior_over_10cm": first(pe[0]), "first_frame_tracked_over_10cm": first(te[0]),
                 "per_frame_from_1": {"prior_error_cm": pe[0], "prior_error_deg": pe[1], "tracked_error_cm": te[0], "tracked_error_deg": te[1],
                                      "record": log[1:].tolist()}}
    if args.prior_anchor:                                                   # the ring's records, frame 1 on; the prior's 16-double records stay with the gated runs
        alog = out["anchor_log"]
        refs = alog[1:, 1].long()
        gated["prior_anchor_promotions"] = int((alog[1:, 3] == 1.0).sum())
        gated["frames_registered_to_an_older_reference"] = [int(i) + 1 for i in torch.nonzero(refs < torch.arange(len(refs))).flatten()]
        gated["per_frame_from_1"] = {k: sig(v) for k, v in gated["per_frame_from_1"].items() if k != "record"}
        gated["anchor_per_frame_from_1"] = {"record": sig(alog[1:].tolist())}
    if args.model_align:                                                    # the alignment's records, frame 1 on, and every frame's tracked error
        log = out["align_log"]
        g = gt[:, :3, 3]
        gated["align_failed_frames"] = [int(i) for i in torch.nonzero(log[1:, 0] == 0.0).flatten() + 1]
        gated["align_per_frame_from_1"] = {"record": sig(log[1:].tolist()), "tracked_error_cm": sig(((out["est_poses"][1:, :3, 3].double() - g[1:]).norm(dim=1) * 100.0).tolist())}
        if "per_frame_from_1" in gated and "record" in gated["per_frame_from_1"]:   # the prior's 16-double records stay with the runs without alignment
            gated["per_frame_from_1"] = {k: sig(v) for k, v in gated["per_frame_from_1"].items() if k != "record"}
    return {**gated, "steps": args.steps, "wall_s_with_final_mesh_and_checkpoint": wall, "loop_s": loop, "steps_per_second": args.steps / loop,
            "phases_total_s": {k: v["total_s"] for k, v in out["timing"].items()},
            "slam_first_frame_ms": slam_t[0] * 1e3,
            "slam_mapped_frame_median_ms": statistics.median([t for i, t in enumerate(slam_t) if i in mapped and i > 0]) * 1e3,
            "slam_tracked_only_frame_median_ms": statistics.median([t for i, t in enumerate(slam_t) if i not in mapped]) * 1e3,
            "commanded_motion_per_step": {"translation_cm_median": float(move.median()), "translation_cm_max": float(move.max()),
                                          "rotation_deg_median": float(turn.median()), "rotation_deg_max": float(turn.max()),
                                          "steps_within_one_call_reach": int(((move <= reach["translation_cm"]) & (turn <= reach["rotation_deg"])).sum()),
                                          "one_call_reach": reach},
            "ate": out["ate"], "mean_translation_error_cm": float(err.mean()) * 100.0, "max_translation_error_cm": float(err.max()) * 100.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-lat", type=int, default=632)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--motion-prior", default=None, choices=["const_speed", "depth_icp", "rgbd_icp"], help="only the run, with this prior, merged into --out")
    ap.add_argument("--no-const-speed", action="store_true", help="with --motion-prior: tracking.const_speed off (depth_icp then starts from the identity)")
    ap.add_argument("--prior-gate", action="store_true", help="with --motion-prior depth_icp / rgbd_icp: the prior's scored starts and verdict on; key suffix _gated; "
                    "per-frame errors of the prior and of the tracked pose against the commanded pose, and the records")
    ap.add_argument("--prior-anchor", action="store_true", help="with --prior-gate: the prior registers every frame to a reference ring kept on the device "
                    "(CoSLAMNarutoHIP(prior_anchor=True)); key suffix _anchored; the ring's per-frame records")
    ap.add_argument("--model-align", action="store_true", help="with --motion-prior: every predicted pose registered to the field's SDF before the tracker "
                    "takes it (CoSLAMNarutoHIP(model_align=True)); key suffix _aligned; the per-frame records and tracked errors")
    ap.add_argument("--small-test", default=None, help="JSON object merged into the document (figures of tests/test_gpu_tracked_run.py)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    mesh = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    if args.motion_prior == "rgbd_icp" and len(mesh) < 3:               # the photometric term needs an image: colour the bare mesh
        mesh = (mesh[0], mesh[1], smooth_colours(mesh[0]))
    res = {"image": [1200, 680], "focal": 600.0, "faces": len(mesh[1]), "active_ray": True,
           "reference": "none: the reference's loop needs Habitat-Sim and tiny-cuda-nn, which are not on this stack"}
    if args.motion_prior is not None:
        run = whole_run(args, dev, mesh)
        print(json.dumps(run, indent=1), flush=True)
        if args.out:
            with open(args.out) as fh:
                doc = json.load(fh)
            doc["office_0_size"]["run_motion_prior_" + args.motion_prior + ("_const_speed_off" if args.no_const_speed else "") + ("_gated" if args.prior_gate else "") +
                                ("_anchored" if args.prior_anchor else "") + ("_aligned" if args.model_align else "")] = run
            with open(args.out, "w") as fh:
                dump_doc(doc, fh)
        return
    res["frames"] = frames(args, dev, mesh)
    print(json.dumps(res["frames"], indent=1), flush=True)
    res["run"] = whole_run(args, dev, mesh)
    print(json.dumps(res["run"], indent=1), flush=True)
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_tracked_run.py: host timers, medians over --repeat; *_ms_host ends when the call returns, *_ms_device after a device "
                       "synchronise; milliseconds unless named otherwise",
               "office_0_size": res}
        if args.small_test:
            doc["tests_test_gpu_tracked_run"] = json.loads(args.small_test)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

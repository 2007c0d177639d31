"""An exploration run with this library alone: the loop of the reference's src/naruto/main.py:90-146 over ``MeshSimHIP`` (in
Habitat's place), ``CoSLAMNarutoHIP`` and ``NarutoPlannerHIP``.

Per step: the modules' step counters, ``sim.simulate(c2w)``, ``slam.online_recon_step(i, color, depth, c2w)``,
``planner.main(uncert_sdf, c2w, is_new_vols)`` (the planner keeps the last volumes it was given; ``is_new_vols`` tells it when they are
fresh).  After the loop: the final mesh at ``mesh.voxel_final`` (``mesh_<num_iter>_final.ply``) and the checkpoint
(``ckpt_<num_iter>_final.pt``).  With a predefined trajectory (the reference's passive mapping, ``enable_active_planning = False``) the
pose of step i is the trajectory's and the planner is skipped.

Command line::

    python -m naruto_amd.run --config <coslam.yaml> --mesh <scene.ply | scene.glb | scene.gltf> [--mesh_frame gltf|mp3d] --num_iter N --result_dir D [--start x y z]
        [--traj traj.txt]
                             [--no_active_ray] [--seed S] [--track] [--eval_views K] [--planner key=value ...]

``--config`` is a Co-SLAM yaml (``naruto_amd.config.load_config``).  The reference's ``.py`` config files are not read: the planner's
settings are ``naruto_amd.planner.DEFAULTS`` (the values of the reference's configs/default.py, restated as data) with ``--planner
key=value`` overrides, and the SLAM keywords (voxel size 0.1, 500 active rays out of a 4x oversampled batch) are ``CoSLAMNarutoHIP``'s
defaults.  ``--traj`` reads a Replica trajectory file: sixteen numbers per line, camera-to-world row-major, columns 1 and 2 of the
rotation negated as the reference's ``load_Replica_pose`` does.  The run's trajectory length goes to ``<result_dir>/results.txt`` as
``traj_len(m),<value>`` (``evaluation.update_results_file``'s format).  ``--track`` estimates the camera poses during the run
(``CoSLAMNarutoHIP(track=True)``) and adds ``ate_rmse(cm)`` / ``ate_mean(cm)``: the estimated trajectory against the poses the frames were
taken at (``evaluation.ate``).  ``--prior_gate`` (with ``--motion_prior depth_icp`` or ``rgbd_icp``) switches on the odometry prior's scored
starts and verdict (``CoSLAMNarutoHIP(prior_gate=True)``) and adds ``prior_failed_frames``, the frames whose prior was refused.
``--prior_anchor [--anchor_slots N]`` (with ``--prior_gate``) registers every frame to one of a ring of reference frames kept on the device
(``CoSLAMNarutoHIP(prior_anchor=...)``) and adds ``prior_anchor_promotions``, the frames that became references.
``--model_align`` (with ``--track``) registers every predicted pose to the field's SDF before the tracker takes it
(``CoSLAMNarutoHIP(model_align=True)``, ``naruto_amd.registration``) and adds ``align_failed_frames``, the frames whose alignment was refused.  ``--eval_views K`` renders every K-th pose of the run from the final map and scores it against the
simulator: ``psnr``, ``ssim`` and ``depth_l1(cm)`` (``naruto_amd.render``).
"""

from __future__ import annotations

import ast
import os
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

PHASES = ("Simulation", "SLAM", "Planning")


def load_replica_traj(path: str) -> torch.Tensor:
    """[N,4,4] float32 camera-to-world poses of a Replica ``traj.txt`` (pose_loader.py:78-91: one pose per line, 16 numbers; columns 1
    and 2 of the upper three rows change sign)."""
    poses = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            if not line.strip():
                continue
            vals = line.split()
            if len(vals) != 16:
                raise ValueError(f"{path}:{n}: expected 16 numbers per pose, got {len(vals)}")
            c2w = np.array(list(map(float, vals))).reshape(4, 4)
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            poses.append(torch.from_numpy(c2w).float())
    if not poses:
        raise ValueError(f"{path}: no pose")
    return torch.stack(poses)


def run_exploration(slam, sim, planner, start_c2w, num_iter: int, on_step: Optional[Callable] = None, traj: Optional[torch.Tensor] = None,
                    eval_views: Optional[int] = None) -> Dict:
    """main.py:90-146.  ``planner`` is set up by the caller (``update_sim``, ``init_data``, ``init_local_planner``) or None with ``traj``
    ([N,4,4], N >= num_iter: the pose of step i is ``traj[i]``).  ``on_step(i, c2w, vols, state)`` is called at the end of every step.
    Returns ``poses`` [num_iter,4,4] (the pose each frame was taken at), ``states`` (the planner's state after each step), ``fresh``
    (the steps that produced new volumes), ``timing`` {phase: {"total_s", "calls", "mean_s"}} from host timers around each phase (the
    SLAM phase ends with whatever the step waited for, not with a device synchronisation), ``mesh`` and ``ckpt_path`` of the final
    save.  When ``slam`` tracks (``CoSLAMNarutoHIP(track=True)``): also ``est_poses`` [num_iter,4,4] (``slam.resolved_poses()``, on the
    host) and ``ate`` (``evaluation.ate(est_poses, poses)``; None below 3 steps).  The planner keeps receiving the COMMANDED pose, the
    one the frame was rendered at, not the estimate -- as the reference's loop does (main.py:135-137).  With ``prior_gate``: also
    ``prior_log`` [num_iter,16] float64 on the host, frame i's record of the odometry prior (``naruto_amd.odometry``; row 0 is zeros).  With ``prior_anchor``: also ``anchor_log`` [num_iter,8] float64 on the host, frame i's anchor record.  With
    ``model_align``: also ``align_log`` [num_iter,8] float64 on the host, frame i's record of the model alignment (``naruto_amd.registration``).  ``eval_views`` = K: after the final
    mesh every K-th pose of the run is rendered from the map and scored against the simulator (``render.evaluate_views``): the result
    gains ``render_eval``.  None: no launch is added."""
    if planner is None and traj is None:
        raise ValueError("run_exploration: a planner or a predefined trajectory")
    if traj is not None and len(traj) < num_iter:
        raise ValueError(f"run_exploration: the trajectory has {len(traj)} poses, the run {num_iter} steps")
    if eval_views is not None and int(eval_views) < 1:
        raise ValueError("run_exploration: eval_views is a positive stride over the run's poses (or None)")
    c2w = torch.as_tensor(start_c2w if traj is None else traj[0]).detach().to("cpu", torch.float32).reshape(4, 4).clone()
    spent = {k: [0.0, 0] for k in PHASES}

    def timed(name, fn, *args):
        t0 = time.perf_counter()
        out = fn(*args)
        spent[name][0] += time.perf_counter() - t0
        spent[name][1] += 1
        return out

    poses, states, fresh = [], [], []
    uncert_sdf = None
    for i in range(int(num_iter)):
        for module in (sim, slam, planner):
            if module is not None and hasattr(module, "update_step"):
                module.update_step(i)
        if traj is not None:
            c2w = traj[i].detach().to("cpu", torch.float32).clone()
        poses.append(c2w.clone())
        color, depth = timed("Simulation", lambda: sim.simulate(c2w.numpy().copy(), no_print=True))
        vols = timed("SLAM", slam.online_recon_step, i, color, depth, c2w)
        if vols is not None:
            uncert_sdf = vols
            fresh.append(i)
        if planner is not None:
            c2w = timed("Planning", planner.main, uncert_sdf, c2w.numpy(), vols is not None)
            c2w = torch.as_tensor(c2w).detach().to("cpu", torch.float32).reshape(4, 4)
            states.append(planner.state)
        if on_step is not None:
            on_step(i, poses[-1], vols, states[-1] if states else None)
    mesh = slam.save_mesh(int(num_iter), voxel_size=slam.config["mesh"]["voxel_final"], suffix="_final")
    ckpt_path = slam.save_ckpt(int(num_iter), suffix="_final") if slam.result_dir is not None else None
    timing = {k: {"total_s": t, "calls": n, "mean_s": t / n if n else 0.0} for k, (t, n) in spent.items()}
    out = {"poses": torch.stack(poses) if poses else torch.zeros(0, 4, 4), "states": states, "fresh": fresh, "timing": timing, "mesh": mesh,
           "ckpt_path": ckpt_path}
    if getattr(slam, "track", False):
        from .evaluation import ate
        out["est_poses"] = slam.resolved_poses().cpu()
        out["ate"] = ate(out["est_poses"], out["poses"]) if len(poses) >= 3 else None
    if getattr(slam, "align_log", None) is not None:                       # the model alignment's records, one row per frame (row 0: zeros)
        out["align_log"] = slam.align_log[:len(poses)].cpu()
    if getattr(slam, "anchor_log", None) is not None:                      # the reference ring's records, one row per frame (row 0: zeros)
        out["anchor_log"] = slam.anchor_log[:len(poses)].cpu()
    if getattr(slam, "prior_log", None) is not None:                       # the gated odometry prior's records, one row per frame (row 0: zeros)
        out["prior_log"] = slam.prior_log[:len(poses)].cpu()
    if eval_views is not None and poses:
        from .render import evaluate_views
        cam = {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
        cam.update(near=slam.config["cam"]["near"], far=slam.config["cam"]["far"])
        out["render_eval"] = evaluate_views(slam.model, slam.config, sim, out["poses"][::int(eval_views)], cam=cam)
    return out


def _planner_overrides(items: List[str]) -> Dict:
    out = {}
    for item in items or []:
        key, sep, val = item.partition("=")
        if not sep or not key:
            raise ValueError(f"--planner {item!r}: expected key=value")
        try:
            out[key] = ast.literal_eval(val)
        except (ValueError, SyntaxError):
            out[key] = val
    return out


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m naruto_amd.run", description="Run an exploration on a mesh: simulate, map, plan.")
    parser.add_argument("--config", type=str, required=True, help="Co-SLAM yaml config (inherit_from chains are followed)")
    parser.add_argument("--mesh", type=str, required=True, help="scene mesh the simulator renders (.ply, or a textured .glb / .gltf)")
    parser.add_argument("--mesh_frame", type=str, default=None, choices=["gltf", "mp3d"],
                        help="a glTF scene's frame: as stored, or MP3D's (x, y, z) -> (x, -z, y); default: mp3d with --dataset MP3D, else gltf")
    parser.add_argument("--num_iter", type=int, required=True, help="number of steps")
    parser.add_argument("--result_dir", type=str, required=True, help="meshes, checkpoints and results.txt go here")
    parser.add_argument("--start", type=float, nargs=3, metavar=("X", "Y", "Z"), help="start position (identity rotation); default: the bound's centre")
    parser.add_argument("--traj", type=str, help="predefined Replica trajectory (passive mapping: the planner is skipped)")
    parser.add_argument("--no_active_ray", action="store_true", help="switch the active ray sampler off")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--track", action="store_true", help="estimate the camera poses during the run (tracking + pose refinement); adds the ATE to results.txt")
    parser.add_argument("--motion_prior", type=str, default=None, choices=["const_speed", "depth_icp", "rgbd_icp"],
                        help="with --track: the tracker's initial pose from constant-speed extrapolation (default), from frame-to-frame depth odometry, "
                             "or from RGB-D odometry (depth plus a photometric term)")
    parser.add_argument("--model_align", action="store_true",
                        help="with --track: register every predicted pose to the field's SDF before the tracker takes it (adds align_failed_frames to results.txt)")
    parser.add_argument("--prior_gate", action="store_true",
                        help="with --motion_prior depth_icp / rgbd_icp: score the prior's two starts and judge its estimate (adds prior_failed_frames to results.txt)")
    parser.add_argument("--prior_anchor", action="store_true",
                        help="with --prior_gate: register every frame to one of a ring of reference frames kept on the device instead of the frame before "
                             "(adds prior_anchor_promotions to results.txt)")
    parser.add_argument("--anchor_slots", type=int, default=None, metavar="N", help="with --prior_anchor: the ring's size, 1 .. 8 (default 4)")
    parser.add_argument("--dataset", type=str, default="NARUTO", choices=["Replica", "MP3D", "NARUTO"], help="the planner's collision rule")
    parser.add_argument("--eval_views", type=int, default=None, metavar="K", help="after the run, render every K-th pose from the map and score it against the simulator (psnr, ssim, depth_l1(cm) in results.txt)")
    parser.add_argument("--planner", type=str, nargs="*", default=[], metavar="KEY=VALUE", help="planner settings over naruto_amd.planner.DEFAULTS")
    args = parser.parse_args(argv)
    if args.num_iter <= 0:
        parser.error("--num_iter must be positive")
    if not args.mesh.lower().endswith((".ply", ".glb", ".gltf")):
        parser.error(f"--mesh {args.mesh}: only .ply, .glb and .gltf meshes are read")
    if args.mesh_frame is None:
        args.mesh_frame = "mp3d" if args.dataset == "MP3D" and args.mesh.lower().endswith((".glb", ".gltf")) else "gltf"
    if args.eval_views is not None and args.eval_views < 1:
        parser.error("--eval_views must be positive")
    if args.anchor_slots is not None and not args.prior_anchor:
        parser.error("--anchor_slots sizes the ring of --prior_anchor")
    if args.traj is not None and args.start is not None:
        parser.error("--start and --traj exclude each other: the trajectory's first pose is the start")
    args.planner = _planner_overrides(args.planner)
    return args


def _anchor_policy(args):
    """``--prior_anchor [--anchor_slots N]`` as ``CoSLAMNarutoHIP``'s ``prior_anchor``."""
    if not args.prior_anchor:
        return None
    from .odometry import AnchorPolicy
    return AnchorPolicy() if args.anchor_slots is None else AnchorPolicy(slots=args.anchor_slots)


def main(argv=None) -> Dict:
    args = parse_args(argv)
    from . import config as cfgmod
    from .evaluation import trajectory_length, update_results_file
    from .planner import DEFAULTS, NarutoPlannerHIP
    from .simulator import MeshSimHIP
    from .slam import CoSLAMNarutoHIP
    unknown = set(args.planner) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"--planner: unknown keys {sorted(unknown)}")
    cfg = cfgmod.load_config(args.config)
    traj = load_replica_traj(args.traj) if args.traj else None
    np.random.seed(args.seed)                      # the planner's RRT draws from numpy's generator
    os.makedirs(args.result_dir, exist_ok=True)
    slam = CoSLAMNarutoHIP(cfg, active_ray=not args.no_active_ray, num_frames=args.num_iter, seed=args.seed, result_dir=args.result_dir, track=args.track,
                           motion_prior=args.motion_prior, prior_gate=True if args.prior_gate else None,
                           model_align=True if args.model_align else None, prior_anchor=_anchor_policy(args))
    sim = MeshSimHIP(args.mesh, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}, device=slam.device, mesh_frame=args.mesh_frame)
    planner = None
    if traj is None:
        planner = NarutoPlannerHIP(dataset=args.dataset, device=slam.device, **args.planner)
        planner.update_sim(sim)
        planner.init_data(cfg["mapping"]["bound"])
        planner.init_local_planner()
    start = torch.eye(4)
    start[:3, 3] = torch.tensor(args.start if args.start is not None else [0.5 * (b[0] + b[1]) for b in cfg["mapping"]["bound"]])
    out = run_exploration(slam, sim, planner, start, args.num_iter, traj=traj, eval_views=args.eval_views)
    length = trajectory_length(out["poses"])
    results = {"traj_len(m)": length}
    if out.get("ate") is not None:
        results.update({"ate_rmse(cm)": out["ate"]["ate_rmse_cm"], "ate_mean(cm)": out["ate"]["ate_mean_cm"]})
    if out.get("align_log") is not None:
        results["align_failed_frames"] = int((out["align_log"][1:, 0] == 0.0).sum())
    if out.get("prior_log") is not None:
        results["prior_failed_frames"] = int((out["prior_log"][1:, 0] == 0.0).sum())
    if out.get("anchor_log") is not None:
        results["prior_anchor_promotions"] = int((out["anchor_log"][1:, 3] == 1.0).sum())
    if out.get("render_eval") is not None:
        from .render import results_rows
        results.update(results_rows(out["render_eval"]))
    update_results_file(results, os.path.join(args.result_dir, "results.txt"))
    torch.cuda.synchronize(slam.device)
    for k, v in out["timing"].items():
        print(f"{k}: {v['total_s']:.3f} s over {v['calls']} calls")
    print(f"trajectory length {length:.2f} m; final mesh {len(out['mesh'].vertices)} vertices; checkpoint {out['ckpt_path']}")
    return out


if __name__ == "__main__":
    main()

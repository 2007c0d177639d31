"""Timing of the pose refinement inside FusedBA (naruto_amd.ba_loop, optimize_poses=True) at the shipped size -- bench.py's office0_ba_iter
scene: 2 148 rays x 43, 40 keyframes, active rays off and on -- one process, the variants alternating, warm, device-event timed; prints
ONE JSON line (ms per 10-iteration call, median of --reps):

  off_graph_call          FusedBA.call_iterations, pose optimisation off: the call graph of today
  on_graph_call           the same with optimize_poses=True: the call graph with the five pose launches per iteration
  on_graph_global_BA      prepare + call_iterations: + the host's matrix -> (omega, t) conversion, its upload and the reset launch
  off_graph_global_BA     prepare + call_iterations with pose optimisation off
  on_eager_call           optimize_poses=True without graphs (prefetch on)
  modular_call            (active rays off only) what a caller had before: the reference's loop body around NarutoFieldHIP
                          (tools/dropin_caller.py, fused optimiser and smoothness) with the poses as torch leaves -- batched Rodrigues,
                          rays from R[ids] / t[ids], autograd to the poses, torch Adam every pose_accum_step iterations

Per-kernel times: run it under rocprofv3 --kernel-trace --stats (--only on_graph_call keeps the trace to the refining call)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import bench  # noqa: E402
from naruto_amd.ba_loop import FusedBA  # noqa: E402
from naruto_amd.tracking import matrices_to_pose6  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _rodrigues(W):
    th2 = (W * W).sum(1)
    th = th2.sqrt().clamp_min(1e-12)
    A, Bc = torch.sin(th) / th, (1 - torch.cos(th)) / th2.clamp_min(1e-24)
    z = torch.zeros_like(th)
    K = torch.stack([z, -W[:, 2], W[:, 1], W[:, 2], z, -W[:, 0], -W[:, 1], W[:, 0], z], 1).reshape(-1, 3, 3)
    return torch.eye(3, device=W.device) + A[:, None, None] * K + Bc[:, None, None] * (K @ K)


def _modular(dev):
    """The caller's own loop: returns a function that runs one 10-iteration call."""
    from dropin_caller import DropInCaller
    cfg, tr, store, _, current, poses, _, (Hh, Ww, n_kf, R) = bench.ba_scene("fp32", False, dev)
    m = tr.model
    m.train()
    caller = DropInCaller(m, cfg, 0.1, optimizer="fused", smoothness="fused")
    mp = cfg["mapping"]
    P = poses.shape[0]
    n_cur = max(mp["sample"] // n_kf, mp["min_pixels_cur"])
    cur = current.to(dev)
    every = mp["keyframe_every"]

    def call():
        p6 = matrices_to_pose6(poses).float().to(dev)
        W, T = p6[:, :3].clone().requires_grad_(True), p6[:, 3:].clone().requires_grad_(True)
        opt = torch.optim.Adam([{"params": [W], "lr": mp["lr_rot"]}, {"params": [T], "lr": mp["lr_trans"]}])
        for i in range(mp["iters"]):
            rays, fids = store.sample_global_rays(mp["sample"])
            idx = torch.randint(0, cur.shape[0], (n_cur,), device=dev)
            rows = torch.cat([rays, cur[idx]], 0)
            ids = torch.cat([torch.div(fids, every, rounding_mode="trunc"), torch.full((n_cur,), P - 1, device=dev, dtype=torch.int64)])
            Rm = _rodrigues(W)
            rays_d = torch.sum(rows[:, None, :3] * Rm[ids], -1)
            caller.ba_iteration(i, T[ids], rays_d, rows[:, 3:6], rows[:, 6:7])
            if (i + 1) % mp["pose_accum_step"] == 0:
                opt.step()
                opt.zero_grad()
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default=None, help="time this variant alone (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"what": "FusedBA pose refinement, 2148 rays x 43, 40 keyframes, 10 iterations per call (pose_accum_step 5)", "unit": "ms per call", "measured": True}
    for active in (False, True):
        variants = {}

        def make(use_graph, on):
            cfg, tr, store, smp, current, poses, vol, _ = bench.ba_scene("fp32", active, dev)
            ba = FusedBA(tr, store, smp, max_poses=256, use_graph=use_graph)
            v = vol if active else None
            ba.prepare(current, poses, v, optimize_poses=on)
            return ba, (lambda: ba.call_iterations()), (lambda: ba.global_BA(current, poses, uncert_vol=v, optimize_poses=on))
        keep = []
        for name, use_graph, on in (("off_graph", True, False), ("on_graph", True, True), ("on_eager", False, True)):
            if args.only and not args.only.startswith(name):
                continue
            ba, call, whole = make(use_graph, on)
            keep.append(ba)
            variants[name + "_call"] = call
            if use_graph:
                variants[name + "_global_BA"] = whole
        if not active and not args.only:
            variants["modular_call"] = _modular(dev)
        if args.only:
            variants = {k: f for k, f in variants.items() if k == args.only}
        for _ in range(args.warmup):
            for f in variants.values():
                f()
        torch.cuda.synchronize()
        ts = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, f in variants.items():               # alternating
                ts[k].append(_timed(f))
        key = "active_ray_on" if active else "active_ray_off"
        out[key] = {k: round(float(np.median(v)), 4) for k, v in ts.items()}
        out[key + "_spread"] = {k: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for k, v in ts.items()}
        del keep, variants
    print(json.dumps(out))


if __name__ == "__main__":
    main()

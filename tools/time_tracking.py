"""Timing of the device tracker (naruto_amd.tracking.TrackerHIP: Co-SLAM tracking_render, 1024 rays x 43, network frozen); prints ONE
JSON line.

  modular_1024x43_iter       the modular route of tools/time_point_grads.py's tracking step: torch pose math around NarutoFieldHIP.forward,
                             mapping loss, backward to the pose, torch Adam -- per iteration (profiles/r07_time_point_grads.json: 1.80 ms)
  tracker_eager_1024x43_iter TrackerHIP.track without a graph: a 10-iteration call (draw, rays, 10 x (forward + naruto_track_backward)) / 10
  tracker_eager_1024x43_call the same call
  tracker_graph_1024x43_call one 10-iteration call replayed as ONE hipGraph (the replay alone)
  tracker_graph_track_call   TrackerHIP.track on a captured tracker: frame copies + the initial pose's axis-angle on the host + the replay

Event-timed on the current stream, median of --reps after --warmup.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import helpers as H  # noqa: E402
from naruto_amd import synthetic as syn, trainer  # noqa: E402
from naruto_amd import tracking as TK  # noqa: E402


def _median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = H.office_cfg(16, perturb=1.0)
    cfg["tracking"] = dict(TK.TRACKING_DEFAULTS)
    iters = cfg["tracking"]["iter"]
    ora = H.make_oracle(cfg, 0.05, 3)
    m = H.make_hip_from_oracle(cfg, ora, dev)
    m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    scene = syn.AnalyticRoom(cfg["mapping"]["bound"])
    Hh, Ww = 120, 160
    fr = scene.rays(1, 12, H=Hh, W=Ww, f=120.0)
    pos, R = scene.pose(1, 12)
    direction = torch.tensor((fr["rays_d"].astype(np.float64) @ R).reshape(Hh, Ww, 3), dtype=torch.float32, device=dev)
    rgb = torch.from_numpy(fr["target_rgb"].reshape(Hh, Ww, 3)).to(dev)
    depth = torch.from_numpy(fr["target_d"].reshape(Hh, Ww)).to(dev)
    init = torch.eye(4)
    init[:3, :3], init[:3, 3] = torch.from_numpy(R).float(), torch.from_numpy(pos).float()
    out = {"what": "device tracking (TrackerHIP), 1024 rays x 43, 10 iterations per call", "unit": "ms", "measured": True}

    # ---- the modular route (tools/time_point_grads.py's tracking step on the same frame's rays)
    trk = TK.TrackerHIP(m, cfg, Hh, Ww, rng_seed=1)
    trk.track(direction, rgb, depth, init)
    d_cam, tgt_rgb, tgt_d = trk.d_cam.clone(), trk.target_rgb.clone(), trk.target_d.clone()[:, None]
    rot = trk.pose_init[:3].clone().requires_grad_(True)
    trans = trk.pose_init[3:].clone().requires_grad_(True)
    opt = torch.optim.Adam([rot, trans], lr=1e-3)

    def modular_step():
        rd = torch.sum(d_cam[..., None, :] * TK.axis_angle_to_matrix(rot)[None], -1)
        ret = m.forward(trans[None].expand(1024, 3), rd, tgt_rgb, tgt_d)
        loss = trainer.get_loss_from_ret(m, cfg, ret)
        opt.zero_grad()
        loss.backward()
        opt.step()
    out["modular_1024x43_iter"] = _median_ms(modular_step, args.warmup, args.reps)
    out["modular_baseline_r07_tracking_1024x43_step"] = 1.80

    # ---- the tracker, eager and as one graph
    out["tracker_eager_1024x43_call"] = _median_ms(lambda: trk._run(), args.warmup, args.reps)
    out["tracker_eager_1024x43_iter"] = out["tracker_eager_1024x43_call"] / iters
    trk.capture()
    out["tracker_graph_1024x43_call"] = _median_ms(lambda: trk._graph.replay(), args.warmup, args.reps)
    out["tracker_graph_track_call"] = _median_ms(lambda: trk.track(direction, rgb, depth, init), args.warmup, args.reps)
    out["speedup_graph_call_vs_10_modular"] = iters * out["modular_1024x43_iter"] / out["tracker_graph_1024x43_call"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()

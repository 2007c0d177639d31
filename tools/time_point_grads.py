"""Timing of the point / ray gradients (naruto_query_bwd_points); prints ONE JSON line.

  tracking      a tracking-shaped step (Co-SLAM tracking_render: network frozen, 1024 rays x 43, pose = axis-angle + translation
                leaves): forward + mapping loss + backward to the pose, per step
  ba_<S>        a global_BA-shaped iteration on the modular route (office0, 2048 rays x S samples): forward + loss + backward with
                the rays requiring grad, against the same iteration with detached rays
  kernel_<S>    naruto_query_bwd_points over all points of 2048 x S ray samples (one launch + the per-ray reduction) next to
                naruto_query_fwd (raw only) on the same points

Event-timed on the current stream, median of --reps after --warmup.  For per-kernel times run it under
rocprofv3 --kernel-trace --stats (profiles/r07_point_grads_*)."""
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
from naruto_amd import ops, synthetic as syn, trainer  # noqa: E402


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


def _skew(w):
    z = w[0] * 0
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"what": "point gradients (naruto_query_bwd_points)", "unit": "ms", "measured": True}

    # ---- (a) tracking step
    cfg = H.office_cfg(16, perturb=1.0)
    ora = H.make_oracle(cfg, 0.05, 3)
    m = H.make_hip_from_oracle(cfg, ora, dev)
    m.train()
    for p in m.parameters():
        p.requires_grad_(False)
    rays = syn.random_rays(1024, cfg["mapping"]["bound"], seed=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in rays.items()}
    R0 = torch.eye(3, device=dev)
    t0 = t["rays_o"][0].clone()
    rot = torch.zeros(3, device=dev, requires_grad=True)
    trans = torch.zeros(3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([rot, trans], lr=1e-3)

    def track_step():
        R = torch.linalg.matrix_exp(_skew(rot)) @ R0
        rd = torch.sum(t["rays_d"][..., None, :] * R[None], -1)
        ro = (t0 + trans)[None].expand(1024, 3)
        ret = m.forward(ro, rd, t["target_rgb"], t["target_d"])
        loss = trainer.get_loss_from_ret(m, cfg, ret)
        opt.zero_grad()
        loss.backward()
        opt.step()
    out["tracking_1024x43_step"] = _median_ms(track_step, args.warmup, args.reps)

    # ---- (b) BA iteration with / without ray gradients; kernel pair on the same points
    for n_d, S in ((32, 43), (117, 128)):
        cfg = H.office_cfg(16, perturb=1.0, n_samples_d=n_d)
        ora = H.make_oracle(cfg, 0.05, 5)
        m = H.make_hip_from_oracle(cfg, ora, dev)
        m.train()
        m.fused_train = False
        rays = syn.random_rays(2048, cfg["mapping"]["bound"], seed=5)
        t = {k: torch.from_numpy(v).to(dev) for k, v in rays.items()}
        for grad in (False, True):
            ro = t["rays_o"].clone().requires_grad_(grad)
            rd = t["rays_d"].clone().requires_grad_(grad)

            def it():
                for p in m.parameters():
                    p.grad = None
                ret = m.forward(ro, rd, t["target_rgb"], t["target_d"])
                trainer.get_loss_from_ret(m, cfg, ret).backward()
            out[f"ba_2048x{S}_{'ray_grads' if grad else 'params_only'}"] = _median_ms(it, args.warmup, args.reps)
        z = m._sample_z(t["rays_o"], t["target_d"], torch.rand(2048, S, device=dev))
        params = {k: v.detach() for k, v in m._params().items()}
        pts, M = ops._points_struct(None, t["rays_o"], t["rays_d"], z)
        raw = torch.empty(M, 5, device=dev)
        d_raw = torch.randn(M, 5, device=dev)
        d_o, d_d = torch.empty_like(t["rays_o"]), torch.empty_like(t["rays_d"])
        lib = ops._lib.load()
        ps = ops._params_struct(params)

        def fwd():
            ops.check(lib.naruto_query_fwd(m._handle().ptr, ops.C.byref(ps), M, ops.C.byref(pts), ops._p(raw), None, None, None, ops._stream()))

        def bwd_pts():
            ops.point_grads(m._handle(), params, pts, M, d_raw, None, d_rays_o=d_o, d_rays_d=d_d)
        out[f"kernel_2048x{S}_query_fwd"] = _median_ms(fwd, args.warmup, args.reps)
        out[f"kernel_2048x{S}_query_bwd_points"] = _median_ms(bwd_pts, args.warmup, args.reps)
        out[f"kernel_2048x{S}_ratio"] = out[f"kernel_2048x{S}_query_bwd_points"] / out[f"kernel_2048x{S}_query_fwd"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()

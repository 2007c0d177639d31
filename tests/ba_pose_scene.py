"""Shared set-up of the pose-refinement tests (test_ba_poses_host.py, test_gpu_ba_poses.py): the naruto_amd.synthetic.AnalyticRoom
scene the tracking and point-gradient tests use, N_KF keyframes + the current frame of a camera ring, a field mapped from the TRUE
poses (tests/golden/ba_pose_field.npz, written by tools/make_ba_pose_fixture.py on the device: hash size 12, uncertainty voxel 0.2),
keyframe poses 1.. and the current pose perturbed, and the contract of naruto_amd/ba_loop.py restated in torch around the CPU oracle
(``OracleBA``: rays from (omega, t) leaves in coslam.py:342-344's form, S.total_loss (+ S.smoothness), torch.optim.Adam).

The schedule of the refinement tests (perturbation, learning rates, pose_accum_step, number of calls, ray count) was found with the
oracle loop alone on the CPU; test_ba_poses_host.py asserts that half, so the device is never the first to see it."""
import os

import numpy as np
import torch

import helpers as H
from naruto_amd import synthetic as syn
from naruto_amd import tracking as TK
from oracle import spec_torch as S

HH, WW, FOC, N_CAM = 60, 80, 60.0, 12
N_KF, R_SAVE = 5, 1500
UNCERT_VOXEL = 0.2
FIELD = "ba_pose_field"
PERTURB_SEED, PERTURB_DEG, PERTURB_M = 3, 1.0, 0.025
# the refinement schedule (test 5): calls of mapping.iters iterations each
REFINE = {"calls": 6, "lr_rot": 2e-3, "lr_trans": 2e-3, "pose_accum_step": 2}


def cfg(**mapping):
    c = H.office_cfg(12, perturb=1.0)
    c["mapping"].update(sample=384, min_pixels_cur=48, keyframe_every=5, iters=10, pose_accum_step=5, filter_depth=True, optim_cur=True)
    c["mapping"].update(mapping)
    return c


def scene(c):
    return syn.AnalyticRoom(c["mapping"]["bound"])


def frame(sc, k, every=5):
    """Camera k's frame as the keyframe store takes it: camera-frame directions, colours, depths."""
    fr = sc.rays(k, N_CAM, H=HH, W=WW, f=FOC)
    _, R = sc.pose(k, N_CAM)
    d_cam = (fr["rays_d"].astype(np.float64) @ R).astype(np.float32)
    return {"direction": torch.from_numpy(d_cam.reshape(1, HH, WW, 3)), "rgb": torch.from_numpy(fr["target_rgb"].reshape(1, HH, WW, 3)),
            "depth": torch.from_numpy(fr["target_d"].reshape(1, HH, WW)), "frame_id": torch.tensor([k * every])}


def current_rays(fr):
    return torch.cat([fr["direction"], fr["rgb"], fr["depth"][..., None]], -1).reshape(-1, 7)


def true_poses(sc, n):
    out = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    for k in range(n):
        pos, R = sc.pose(k, N_CAM)
        out[k, :3, :3], out[k, :3, 3] = torch.from_numpy(R), torch.from_numpy(pos)
    return out


def perturbed(true, seed=PERTURB_SEED, deg=PERTURB_DEG, dist=PERTURB_M):
    """Poses 1.. rotated by ``deg`` about a random axis and moved by ``dist`` in a random direction (pose 0 is the gauge: untouched)."""
    rs = np.random.RandomState(seed)
    out = true.clone()
    for k in range(1, true.shape[0]):
        ax, dr = rs.normal(size=3), rs.normal(size=3)
        w = torch.tensor(ax / np.linalg.norm(ax) * (deg * np.pi / 180.0))
        out[k, :3, :3] = TK.axis_angle_to_matrix(w) @ true[k, :3, :3]
        out[k, :3, 3] += torch.tensor(dr / np.linalg.norm(dr) * dist)
    return out.float()


def errors(c2w, true, rows=None):
    """Mean (degrees, metres) between poses [P,4,4] and the true ones over ``rows`` (default: 1..)."""
    c2w = torch.as_tensor(c2w).detach().double().cpu()
    rows = range(1, c2w.shape[0]) if rows is None else rows
    ang = [float(TK.matrix_to_axis_angle(c2w[k, :3, :3].T @ true[k, :3, :3]).norm()) * 180.0 / np.pi for k in rows]
    dst = [float((c2w[k, :3, 3] - true[k, :3, 3]).norm()) for k in rows]
    return float(np.mean(ang)), float(np.mean(dst))


def pose6_matrices(pose6):
    return torch.stack([TK.pose_matrix(p.double()) for p in pose6])


# ------------------------------------------------------------------------------------------------ the mapped field
def field_path():
    return os.path.join(H.GOLDEN, FIELD + ".npz")


NAMES = ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1", "uncert_grid")


def hip_params(m):
    return {"table": m.embed_fn.params, "sdf_w0": m.decoder.sdf_net.model[0].weight, "sdf_w1": m.decoder.sdf_net.model[2].weight,
            "col_w0": m.decoder.color_net.model[0].weight, "col_w1": m.decoder.color_net.model[2].weight, "uncert_grid": m.uncert_grid}


def load_oracle(c):
    ora = H.make_oracle(c, 0.05, 0, uncert_voxel=UNCERT_VOXEL)
    g = H.load_golden(FIELD)
    with torch.no_grad():
        for n in NAMES:
            getattr(ora, n).copy_(torch.from_numpy(g[n]).reshape(getattr(ora, n).shape))
    return ora


def load_trainer(tr):
    g = H.load_golden(FIELD)
    with torch.no_grad():
        for n, p in hip_params(tr.model).items():
            p.copy_(torch.from_numpy(g[n]).reshape(p.shape).to(p.device))


def sync_oracle(ora, m):
    with torch.no_grad():
        for n, p in hip_params(m).items():
            getattr(ora, n).copy_(p.detach().cpu().reshape(getattr(ora, n).shape))


# ------------------------------------------------------------------------------------------------ the contract in torch
class OracleBA:
    """One ``global_BA`` call with pose optimisation as naruto_amd/ba_loop.py states it.  ``pose6`` [P,6] the initial (omega, t);
    ``step_network``: the oracle steps its own network (reference create_optimizer / init_uncert_grid_optim) -- otherwise the caller
    keeps its parameters in step with the device (sync_oracle) and only the poses evolve here."""

    def __init__(self, ora, c, pose6, step_network=False, net_opts=None):
        mp = c["mapping"]
        self.ora, self.c, self.P = ora, c, pose6.shape[0]
        self.W = pose6[:, :3].clone().float().requires_grad_(True)
        self.T = pose6[:, 3:].clone().float().requires_grad_(True)
        self.mask = torch.zeros(self.P, dtype=torch.bool)
        self.mask[1:self.P - 1] = True
        if self.P >= 2 and mp["optim_cur"]:
            self.mask[self.P - 1] = True
        self.opt = torch.optim.Adam([{"params": [self.W], "lr": mp["lr_rot"]}, {"params": [self.T], "lr": mp["lr_trans"]}], betas=(0.9, 0.999), eps=1e-8)
        self.accum = int(mp["pose_accum_step"])
        self.trace = []                 # per pose step: ((omega, t) before [P,6], accumulated gradient [P,6])
        self.step_network = step_network
        for p in ora.parameters():
            p.requires_grad_(step_network)
        self.net_opts = net_opts
        if step_network and net_opts is None:
            groups, ugrid = ora.param_groups()
            self.net_opts = (torch.optim.Adam(groups, betas=(0.9, 0.99)), torch.optim.Adam(ugrid, lr=1))
            ora.uncert_grid.grad = torch.zeros_like(ora.uncert_grid)

    def pose6(self):
        return torch.cat([self.W, self.T], 1).detach().clone()

    def iteration(self, i, d_cam, pid, rgb, dep, rand, rand6=None):
        ora, tr = self.ora, self.c["training"]
        ora.train()
        R = torch.stack([TK.axis_angle_to_matrix(self.W[p]) for p in range(self.P)])
        rays_d = torch.sum(d_cam[:, None, :] * R[pid], -1)                 # coslam.py:343
        rays_o = self.T[pid]
        ret = ora.forward(rays_o, rays_d, rgb, dep.reshape(-1, 1), rand=rand)
        sm = S.smoothness(ora, tr["smooth_pts"], tr["smooth_vox"], tr["smooth_margin"], rand6[:3], rand6[3:]) if rand6 is not None else None
        loss = S.total_loss(ret, tr, sm)
        if self.step_network:
            self.net_opts[0].zero_grad(set_to_none=True)
        loss.backward()
        if self.step_network:
            self.net_opts[0].step()
            if (i + 1) % 5 == 0:
                self.net_opts[1].step()
                ora.uncert_grid.grad.zero_()
        if (i + 1) % self.accum == 0:
            self.pose_step()
        return float(loss.detach())

    def pose_step(self):
        with torch.no_grad():
            self.W.grad[~self.mask] = 0.0
            self.T.grad[~self.mask] = 0.0
            self.trace.append((self.pose6(), torch.cat([self.W.grad, self.T.grad], 1).clone()))
        self.opt.step()                        # rows with gradient 0 and moments 0 do not move
        self.opt.zero_grad(set_to_none=False)


def trajectory_mask(grad_ref):
    """Components whose reference gradient exceeds 10 x test 1's bound (1e-4 of the block's largest magnitude + 1e-3 relative): Adam's
    first step is a sign, so a component within the bound of zero may flip."""
    keep = torch.zeros_like(grad_ref, dtype=torch.bool)
    for blk in (slice(0, 3), slice(3, 6)):
        g = grad_ref[:, blk].abs().double()
        keep[:, blk] = g > 10.0 * (1e-4 * float(g.max()) + 1e-3 * g)
    return keep


def host_draw(rs, frames, n_global, n_cur):
    """A BA batch drawn on the host (numpy; the device draws its own): (d_cam, pose id, rgb, depth) of n_global keyframe pixels and n_cur
    pixels of the current frame (the last of ``frames``, pose id P-1)."""
    n_kf = len(frames) - 1
    kf = rs.randint(0, n_kf, n_global)
    px = rs.randint(0, HH * WW, n_global)
    pid = np.concatenate([kf, np.full(n_cur, n_kf)])
    px = np.concatenate([px, rs.choice(HH * WW, n_cur, replace=False)])
    d = torch.stack([frames[k]["direction"].reshape(-1, 3)[p] for k, p in zip(pid, px)])
    c = torch.stack([frames[k]["rgb"].reshape(-1, 3)[p] for k, p in zip(pid, px)])
    z = torch.stack([frames[k]["depth"].reshape(-1)[p] for k, p in zip(pid, px)])
    return d, torch.from_numpy(pid).long(), c, z

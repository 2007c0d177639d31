"""The fused camera tracker's contract (naruto_amd/tracking.py, csrc/naruto_track.hip) restated in numpy / torch fp64, importing nothing of the
package but its config defaults.  tests/test_tracking_spec_host.py pins this twin on the CPU (against the kernels' own host build and fp64
autograd); tests/test_gpu_tracking_edges.py holds the device to it, tests/test_gpu_tracking.py uses ``oracle_track`` and ``schedule``.

interior_pixels, unflatten   the set the draw may return and the h-fastest rule, by enumeration (no % or // of the flat index)
rotation                     R(omega) in torch, differentiable: closed form, Taylor series below theta^2 = 1e-4
rays_from_pose               the bits of the device's rays: R(omega) in fp64 rounded once, then ((dx R_i0) + (dy R_i1)) + (dz R_i2) in fp32
pose_gradient                d_t = sum d_rays_o, G = sum d_rays_d (x) d_cam, d_omega by fp64 autograd through R; and sum |terms| per component
schedule                     Co-SLAM's best-pose / wait_iters bookkeeping over recorded losses
adam_step                    torch.optim.Adam on (omega, t) from adam_spec.adam_twin: two learning rates, one step count
oracle_track, oracle_eval    the oracle's loss and autograd for a whole call / at one given pose (teacher forcing)
CASES, case_cfg, case_frame  the edge suite's case matrix: built on the CPU, so that its premises are checked without a GPU
"""
import numpy as np
import torch

import adam_spec
import helpers as H
from oracle import spec_torch as S

SERIES_BELOW = 1e-4                 # theta^2 under which R(omega) is a series (naruto_pose.h: rodrigues_coeffs)
BETAS, EPS = (0.9, 0.999), 1e-8     # torch.optim.Adam's defaults, which Co-SLAM's pose optimiser keeps
# replica_coslam.yaml:29-42 (restated: this module does not import the tracker)
TRACKING_DEFAULTS = {"iter": 10, "sample": 1024, "lr_rot": 1e-3, "lr_trans": 1e-3, "ignore_edge_W": 20, "ignore_edge_H": 20,
                     "iter_point": 0, "wait_iters": 100, "const_speed": True, "best": True}


# ------------------------------------------------------------------------------------------------ the draw
def _interior_order(Hh, Ww, eh, ew):
    """Flat pixels h * W + w of the interior [eh, H - eh) x [ew, W - ew), column after column (h fastest: Co-SLAM's order)."""
    return np.array([h * Ww + w for w in range(ew, Ww - ew) for h in range(eh, Hh - eh)], dtype=np.int64)


def interior_pixels(Hh, Ww, eh, ew):
    return set(_interior_order(Hh, Ww, eh, ew).tolist())


def unflatten(k, Hh, Ww, eh, ew):
    """Flat pixel index of interior index k (an int or an array of them)."""
    return _interior_order(Hh, Ww, eh, ew)[np.asarray(k, dtype=np.int64)]


# ------------------------------------------------------------------------------------------------ R(omega)
def _skew(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def rotation(w):
    """Rodrigues' formula R = I + sin(th)/th K + (1 - cos(th))/th^2 K^2, K = [w]x, for w [3]; differentiable.  Below theta^2 = 1e-4 both
    coefficients are their Taylor series to theta^10 (the next term is below 1e-27 there)."""
    th2 = (w * w).sum()
    K = _skew(w)
    if float(th2.detach()) < SERIES_BELOW:
        A = 1 - th2 / 6 * (1 - th2 / 20 * (1 - th2 / 42 * (1 - th2 / 72 * (1 - th2 / 110))))
        B = 0.5 - th2 / 24 * (1 - th2 / 30 * (1 - th2 / 56 * (1 - th2 / 90 * (1 - th2 / 132))))
    else:
        th = th2.sqrt()
        A, B = torch.sin(th) / th, (1 - torch.cos(th)) / th2
    return torch.eye(3, dtype=w.dtype) + A * K + B * (K @ K)


def rotation_f32(pose6):
    """The fp32 rotation the device forms rays and c2w with: R(omega) in fp64 of the fp32 omega, rounded once."""
    w = torch.from_numpy(np.asarray(pose6, dtype=np.float32)[:3].astype(np.float64))
    return rotation(w).numpy().astype(np.float32)


def rays_from_pose(pose6, d_cam):
    """(rays_o, rays_d) [N,3] float32 as k_track_rays / k_track_step write them: each product and each sum rounded to fp32, no FMA."""
    p = np.asarray(pose6, dtype=np.float32)
    d = np.asarray(d_cam, dtype=np.float32)
    R = rotation_f32(p)
    rays_d = np.empty_like(d)
    for i in range(3):
        rays_d[:, i] = ((d[:, 0] * R[i, 0]) + (d[:, 1] * R[i, 1])) + (d[:, 2] * R[i, 2])
    assert rays_d.dtype == np.float32
    return np.tile(p[3:], (d.shape[0], 1)), rays_d


def c2w_f32(pose6):
    """[4,4] float32 camera-to-world of (omega, t) as the device writes it."""
    p = np.asarray(pose6, dtype=np.float32)
    out = np.eye(4, dtype=np.float32)
    out[:3, :3] = rotation_f32(p)
    out[:3, 3] = p[3:]
    return out


def pose_gradient(pose6, d_cam, d_rays_o, d_rays_d):
    """The gradient of the loss w.r.t. (omega, t) from the rays' gradients, in fp64 -> (grad [6], sum of |terms| [6]).  rays_o = t and
    rays_d[r,i] = sum_j R[i,j] d_cam[r,j], so d_t = sum_r d_rays_o[r], dL/dR = G = sum_r d_rays_d[r] (x) d_cam[r] and
    d_omega[k] = sum_ij G[i,j] dR[i,j]/d omega[k], the Jacobian by autograd through ``rotation``."""
    w = torch.from_numpy(np.asarray(pose6, dtype=np.float64)[:3].copy())
    dc, dro, drd = (np.asarray(a, dtype=np.float64) for a in (d_cam, d_rays_o, d_rays_d))
    J = torch.autograd.functional.jacobian(rotation, w).numpy()            # [3,3,3]: (i, j, k)
    G, G_abs = drd.T @ dc, np.abs(drd).T @ np.abs(dc)
    grad = np.concatenate([np.einsum("ij,ijk->k", G, J), dro.sum(0)])
    terms = np.concatenate([np.einsum("ij,ijk->k", G_abs, np.abs(J)), np.abs(dro).sum(0)])
    return grad, terms


# ------------------------------------------------------------------------------------------------ schedule and Adam
def schedule(losses, poses, wait_iters, best_flag):
    """Co-SLAM's bookkeeping over recorded losses (fp32 values compared as the device compares them)."""
    best, best_pose, thresh = None, None, 0
    for i, L in enumerate(losses):
        if i == 0:
            best, best_pose = L, poses[0]
        if L < best:
            best, best_pose, thresh = L, poses[i], 0
        else:
            thresh += 1
        if thresh > wait_iters:
            return {"stopped": True, "n": i + 1, "best_pose": best_pose, "thresh": thresh, "result": best_pose if best_flag else poses[i]}
    return {"stopped": False, "n": len(losses), "best_pose": best_pose, "thresh": thresh, "result": best_pose if best_flag else poses[-1]}


def adam_step(pose, grads, lr_rot, lr_trans, betas=BETAS, eps=EPS):
    """The pose after Adam step number len(grads), taken from ``pose`` [6] with the moments of ``grads`` [n,6] (the gradients of steps
    1 .. n, moments zero before the first): adam_spec.adam_twin per step -- fp64 arithmetic on moments stored in fp32, as the device
    stores them -- with lr_rot for omega, lr_trans for t and one step count.  -> (pose [6] fp64, adam_twin's bound [6])."""
    grads = np.asarray(grads, dtype=np.float32).reshape(-1, 6)
    lr = np.array([lr_rot] * 3 + [lr_trans] * 3)
    m, v = np.zeros(6, np.float32), np.zeros(6, np.float32)
    p = np.asarray(pose, dtype=np.float32)
    for t, g in enumerate(grads, 1):
        p1, m, v, bound, _, _ = adam_spec.adam_twin(p, g, m, v, lr=lr, betas=betas, eps=eps, wd=0.0, t=t, fp64_bias=True)
    return p1, bound


def ulp32(x):
    """The spacing of fp32 at |x| (fp64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_track(ora, cfg, d_cam, rgb, dep, pose0, rand):
    """The contract in torch: rays from (omega, t), the oracle's training forward and total loss, best-pose bookkeeping, torch Adam."""
    tk = cfg["tracking"]
    w = pose0[:3].clone().requires_grad_(True)
    t = pose0[3:].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [w], "lr": tk["lr_rot"]}, {"params": [t], "lr": tk["lr_trans"]}], betas=BETAS, eps=EPS)
    poses, losses, grads = [], [], []
    best, best_pose, thresh, last = None, None, 0, None
    ora.train()
    for i in range(tk["iter"]):
        opt.zero_grad()
        rays_d = torch.sum(d_cam[..., None, :] * rotation(w)[None], -1)
        rays_o = t[None].expand(d_cam.shape[0], 3)
        ret = ora.forward(rays_o, rays_d, rgb, dep[:, None], rand=rand[i])
        loss = S.total_loss(ret, cfg["training"])
        last = torch.cat([w, t]).detach().clone()
        poses.append(last)
        losses.append(float(loss.detach()))
        if i == 0:
            best, best_pose = losses[-1], last
        if losses[-1] < best:
            best, best_pose, thresh = losses[-1], last, 0
        else:
            thresh += 1
        if thresh > tk["wait_iters"]:
            break
        loss.backward()
        grads.append(torch.cat([w.grad, t.grad]).detach().clone())
        opt.step()
    return {"poses": poses, "losses": losses, "grads": grads, "result": best_pose if tk["best"] else last}


def oracle_eval(ora, cfg, d_cam, rgb, dep, pose6, rand):
    """The oracle at ONE given pose (teacher forcing): (omega, t) are fp64 leaves, the rays R(omega) d_cam and t in fp64 rounded to fp32,
    then the oracle's fp32 training forward and total loss on the pixels' colours and depths with the jitter ``rand`` [N,S].
    -> loss, d_pose [6] (fp64 autograd), d_rays_o / d_rays_d [N,3] (autograd w.r.t. the fp32 rays), z_vals [N,S], and ``active`` [N,S]:
    the samples whose raw output carries a cotangent."""
    tr, cam = cfg["training"], cfg["cam"]
    p = torch.as_tensor(pose6).detach().double().cpu()
    w, t = p[:3].clone().requires_grad_(True), p[3:].clone().requires_grad_(True)
    d64 = d_cam.double()
    rays_d = torch.sum(d64[..., None, :] * rotation(w)[None], -1).float()
    rays_o = t[None].expand(d_cam.shape[0], 3).float()
    rays_d.retain_grad()
    rays_o.retain_grad()
    ora.train()
    rend = ora.render_rays(rays_o, rays_d, target_d=dep[:, None], rand=rand)
    rend["raw"].retain_grad()
    ret = S.render_losses(rend, rgb, dep[:, None], cam["depth_trunc"], tr["rgb_missing"], tr["trunc"], cfg["data"]["sc_factor"])
    loss = S.total_loss(ret, tr)
    loss.backward()
    return {"loss": float(loss.detach()), "d_pose": torch.cat([w.grad, t.grad]).detach(), "d_rays_o": rays_o.grad.detach(), "d_rays_d": rays_d.grad.detach(),
            "rays_o": rays_o.detach(), "rays_d": rays_d.detach(), "z_vals": rend["z_vals"].detach(),
            "active": rend["raw"].grad.detach().abs().sum(-1) > 0}


def kink_rays(ora, cfg, ev):
    """[N] bool: the rays with an active sample within fp32 rounding of a ReLU kink (helpers.relu_kink_distance's 2e-6), where the oracle's
    own gradient is decided by rounding noise.  By bisection over the rays: one call where the batch has none."""
    N = ev["active"].shape[0]
    out = torch.zeros(N, dtype=torch.bool)
    todo = [(0, N)]
    while todo:
        lo, hi = todo.pop()
        only = torch.zeros_like(ev["active"])
        only[lo:hi] = ev["active"][lo:hi]
        if H.relu_kink_distance(ora, cfg, ev["rays_o"], ev["rays_d"], ev["z_vals"], only)[1] == 0:
            continue
        if hi - lo == 1:
            out[lo] = True
        else:
            todo += [(lo, (lo + hi) // 2), ((lo + hi) // 2, hi)]
    return out


def trajectory_kink_distance(ora, cfg, d_cam, rgb, dep, pose0, rand):
    """The smallest ReLU-kink distance over the iterations of the oracle's own run of a call (oracle_track, then oracle_eval at each pose)."""
    out = float("inf")
    for i, p in enumerate(oracle_track(ora, cfg, d_cam, rgb, dep, pose0, rand)["poses"]):
        ev = oracle_eval(ora, cfg, d_cam, rgb, dep, p, rand[i])
        out = min(out, H.relu_kink_distance(ora, cfg, ev["rays_o"], ev["rays_d"], ev["z_vals"], ev["active"])[0])
    return out


# ------------------------------------------------------------------------------------------------ the edge suite's cases
FRAME = (24, 32, 2, 3)              # H, W, ignore_edge_H, ignore_edge_W: a non-square 20 x 26 interior
WALK, SHORT = 1, 3                  # launch_forms.WALK / SHORT


def _case(id, N=5, nd=2, nr=1, frame=FRAME, iters=2, seed=0, pose="near", zero_depth=0.0, one_depth=False, wait_iters=100, best=True,
          form=SHORT, tiles=0, mode="fp32", lr=1e-3, device_pose=False, rng_seed=None):
    return dict(id=id, N=N, nd=nd, nr=nr, frame=frame, iters=iters, seed=seed, pose=pose, zero_depth=zero_depth, one_depth=one_depth,
                wait_iters=wait_iters, best=best, form=form, tiles=tiles, mode=mode, lr=lr, device_pose=device_pose,
                rng_seed=rng_seed if rng_seed is not None else 1000 + seed)


def _cases():
    """The seeds are chosen so that, along the oracle's own trajectory of the case (``trajectory_kink_distance``), no sample with a
    cotangent comes within 4e-6 of a ReLU kink -- twice the 2e-6 at which helpers.relu_kink_distance calls the oracle's gradient
    rounding noise: d_pose sums every ray, so check b needs a batch without such a sample at every iteration it is asserted."""
    out = []
    # ray count at S = 2 + 1: k_track_step's 256-ray stride and tree, the last block of k_track_draw / k_track_rays
    for N, seed in ((1, 10), (3, 11), (255, 1312), (256, 2413), (257, 1814), (513, 15)):
        out.append(_case(f"N{N}", N=N, iters=3 if N <= 257 else 1, seed=seed))
    # samples per ray: the training forward's form under the tracker's workspace
    out.append(_case("S3+2_short", N=5, nd=3, nr=2, iters=3, seed=20))
    out.append(_case("S53+11_short", N=5, nd=53, nr=11, iters=3, seed=21))
    out.append(_case("S54+11_partial_walk", N=5, nd=54, nr=11, iters=3, seed=22, form=WALK, tiles=2))
    out.append(_case("S117+11_exact_walk", N=9, nd=117, nr=11, iters=3, seed=3227, form=WALK, tiles=2))
    # the draw
    out.append(_case("borders0", N=37, frame=(9, 7, 0, 0), seed=30))
    out.append(_case("one_row", N=11, frame=(9, 20, 4, 2), seed=31))               # Hi = 1
    out.append(_case("one_column", N=11, frame=(20, 9, 2, 4), seed=32))            # Wi = 1
    out.append(_case("whole_interior", N=35, frame=(9, 11, 2, 2), seed=33))        # N = n_interior = 5 x 7
    out.append(_case("one_pixel", N=1, frame=(5, 7, 2, 3), seed=34))
    # depth
    out.append(_case("depth_30pct_missing", N=64, iters=3, seed=40, zero_depth=0.3))
    out.append(_case("one_depth", N=17, iters=3, seed=41, one_depth=True))
    # pose
    out.append(_case("omega0", N=33, iters=3, seed=50, pose="zero"))
    out.append(_case("omega9.9e-3", N=33, iters=3, seed=51, pose=9.9e-3, device_pose=True))
    out.append(_case("omega1.01e-2", N=33, iters=3, seed=152, pose=1.01e-2, device_pose=True))
    out.append(_case("omega3.1", N=33, iters=3, seed=53, pose=3.1))
    out.append(_case("omega3.5", N=33, iters=3, seed=54, pose=3.5, device_pose=True))
    out.append(_case("outside_the_box", N=33, iters=3, seed=55, pose="outside"))
    # schedule
    for best in (True, False):
        b = "best" if best else "last"
        out.append(_case(f"iter1_{b}", N=65, iters=1, seed=60, best=best))
        out.append(_case(f"wait0_{b}", N=65, iters=3, seed=61, wait_iters=0, best=best))
        out.append(_case(f"wait1_diverging_{b}", N=65, iters=6, seed=62, wait_iters=1, best=best, lr=0.3))
    # bf16 MLP mode: checks c, d, f
    out.append(_case("bf16_short", N=65, nd=32, nr=11, iters=2, seed=70, mode="bf16"))
    out.append(_case("bf16_walk", N=9, nd=117, nr=11, iters=2, seed=71, mode="bf16", form=WALK, tiles=2))
    return out


CASES = _cases()
ITER1 = [c for c in CASES if c["iters"] == 1]


def case_cfg(c):
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=c["nd"], n_range_d=c["nr"])
    cfg["tracking"] = dict(TRACKING_DEFAULTS, iter=c["iters"], sample=c["N"], ignore_edge_H=c["frame"][2], ignore_edge_W=c["frame"][3],
                           wait_iters=c["wait_iters"], best=c["best"], lr_rot=c["lr"], lr_trans=c["lr"])
    if c["mode"] == "bf16":
        cfg["decoder"]["mlp_precision"] = "bf16"
    return cfg


def case_frame(c, cfg):
    """The synthetic frame (direction [H,W,3] of roughly unit length, colours, depths in (0.3, 4)), the initial pose (omega, t) as fp32
    and the jitter [iter, N, S], all on the CPU."""
    Hh, Ww, eh, ew = c["frame"]
    rs = np.random.RandomState(c["seed"])
    d = rs.normal(size=(Hh, Ww, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rs.uniform(0.9, 1.1, (Hh, Ww, 1))
    rgb = rs.uniform(0, 1, (Hh, Ww, 3))
    dep = rs.uniform(0.3, 4.0, (Hh, Ww))
    if c["zero_depth"] > 0:
        dep[rs.uniform(size=(Hh, Ww)) < c["zero_depth"]] = 0.0
    bb = np.asarray(cfg["mapping"]["bound"], dtype=np.float64)
    centre, half = bb.mean(1), 0.5 * (bb[:, 1] - bb[:, 0])
    axis = rs.normal(size=3)
    axis /= np.linalg.norm(axis)
    t = centre + rs.uniform(-0.3, 0.3, 3) * half
    if c["pose"] == "zero":
        w = np.zeros(3)
    elif c["pose"] == "near":
        w = axis * rs.uniform(0.3, 1.5)
    elif c["pose"] == "outside":
        w = axis * 0.7
        t = bb[:, 1] + 6.0 * half                 # every sample (depths up to far) misses the box
    else:
        w = axis * float(c["pose"])
    pose = np.concatenate([w, t]).astype(np.float32)
    S_tot = c["nd"] + c["nr"]
    rand = torch.rand(c["iters"], c["N"], S_tot, generator=torch.Generator().manual_seed(c["seed"]))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return f32(d), f32(rgb), f32(dep), torch.from_numpy(pose), rand


def host_draw(lib, c, seed, counter):
    """The draw restated: naruto_perm_index (the keyed permutation, pinned by tests/test_tracking_host.py) through ``unflatten``."""
    Hh, Ww, eh, ew = c["frame"]
    n_int = (Hh - 2 * eh) * (Ww - 2 * ew)
    k = [lib.naruto_perm_index(i, n_int, seed % (1 << 64), counter, 4) for i in range(c["N"])]
    return torch.from_numpy(unflatten(k, Hh, Ww, eh, ew))


def keep_one_depth(c, dep, pix):
    """The 'one_depth' frame: every depth 0 except at ONE drawn pixel."""
    keep = int(pix[c["N"] // 2])
    out = torch.zeros_like(dep)
    out.reshape(-1)[keep] = dep.reshape(-1)[keep]
    return out


def gather(direction, rgb, dep, pix):
    return direction.reshape(-1, 3)[pix], rgb.reshape(-1, 3)[pix], dep.reshape(-1)[pix]

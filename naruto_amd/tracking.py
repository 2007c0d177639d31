"""Camera tracking on the device: Co-SLAM's ``tracking_render`` (called at coslam.py:594-602 when ``tracking.disable`` is false).

Co-SLAM's ``tracking_render`` and its helpers (``select_samples``, ``get_pose_param_optim``, ``matrix_from_tensor``,
``predict_current_pose``, Co-SLAM 3bb904e) are not in the reference tree: what follows is the published algorithm as this
project restates it (parity unpinned).  Per call, for one frame, with the network frozen:

1. ``tracking.sample`` distinct pixels of the interior ``[iH, H-iH) x [iW, W-iW)`` are drawn ONCE (flat interior index k ->
   ``h = iH + k % (H-2iH)``, ``w = iW + k // (H-2iH)``: Co-SLAM's h-fastest order) with the keyed Feistel permutation of
   ``naruto_sample_distinct`` instead of ``random.sample`` (the keyframe store's documented deviation).
2. The pose is an absolute axis-angle ``omega`` of the camera-to-world rotation plus the translation ``t``; ``R(omega)`` is
   Rodrigues' formula.  A fresh ``torch.optim.Adam`` (betas 0.9 / 0.999, eps 1e-8) with ``lr_rot`` / ``lr_trans``.
3. Each iteration: ``rays_o = t``, ``rays_d = R d_cam`` (coslam.py:342-344's form), the training forward, ``get_loss_from_ret``'s
   default terms; best-pose bookkeeping (the first loss is the best, then ``loss < best`` resets ``thresh``, else ``thresh += 1``);
   ``thresh > wait_iters`` stops the call, else one Adam step on ``(omega, t)``.
4. The result is the best pose (``tracking.best``) or the pose evaluated last (before the last step), as a [4,4] float32 tensor.

Differences from the reference: parameter gradients are not accumulated (the next ``global_BA`` zeroes them before any step,
coslam.py:284-288); ``ignore_edge_* = 0`` means no margin (the reference's ``[0:-0]`` slices to nothing).

Per iteration the device runs the training forward (naruto_train_forward), then naruto_track_backward: the loss backward and
compaction, the point gradients (k_query_bwd_points, k_ray_point_reduce) and one workgroup that sums the pose gradient, steps
Adam and writes the next iteration's rays.  ``capture()`` records a whole call as one hipGraph.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib, ops
from .capture import preserved, warm_up

# replica_coslam.yaml:29-42
TRACKING_DEFAULTS = {"iter": 10, "sample": 1024, "lr_rot": 1e-3, "lr_trans": 1e-3, "ignore_edge_W": 20, "ignore_edge_H": 20,
                     "iter_point": 0, "wait_iters": 100, "const_speed": True, "best": True}
DRAW_SALT = 4              # the key of the pixel draw: mix(seed, counter, 4) (naruto_perm_index's salt)


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def tracking_settings(config: Dict) -> Dict:
    """``config['tracking']`` over replica_coslam.yaml's values, with the device tracker's refusals."""
    tk = dict(TRACKING_DEFAULTS)
    tk.update(config.get("tracking", {}) or {})
    if int(tk["iter_point"]) > 0:
        raise NotImplementedError("tracking.iter_point > 0 (Co-SLAM tracking_pc) is not implemented by TrackerHIP")
    rot_rep = config.get("training", {}).get("rot_rep", "axis_angle")
    if rot_rep != "axis_angle":
        raise NotImplementedError(f"TrackerHIP optimises an axis-angle pose: training.rot_rep = {rot_rep!r} is not implemented")
    return tk


def check_frame(direction, rgb, depth, H: int, W: int) -> None:
    """ValueError unless the frame is float32 device tensors of [H,W,3] [H,W,3] [H,W]."""
    for a, n, shape in ((direction, "direction", (H, W, 3)), (rgb, "rgb", (H, W, 3)), (depth, "depth", (H, W))):
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32):
            raise ValueError(f"tracking: {n} must be a float32 tensor on the GPU")
        if tuple(a.shape) != shape:
            raise ValueError(f"tracking: {n} must be {list(shape)} for this tracker, got {list(a.shape)}")


def draw_pixels_host(H: int, W: int, edge_h: int, edge_w: int, n: int, seed: int, counter: int) -> torch.Tensor:
    """The pixel draw of naruto_track_draw on the host (naruto_perm_index): flat pixel indices ``h * W + w`` [n] for the random word
    {seed, counter} as the draw reads it."""
    lib = _lib.load()
    Hi, Wi = H - 2 * edge_h, W - 2 * edge_w
    k = torch.tensor([lib.naruto_perm_index(i, Hi * Wi, seed % (1 << 64), counter, DRAW_SALT) for i in range(n)], dtype=torch.int64)
    return (edge_h + k % Hi) * W + (edge_w + k // Hi)


def matrix_to_axis_angle(R: torch.Tensor) -> torch.Tensor:
    """Axis-angle [3] of one rotation matrix [3,3] through the unit quaternion (as pytorch3d's ``matrix_to_axis_angle``), fp64."""
    a = torch.as_tensor(R).double().reshape(3, 3)
    tr = a[0, 0] + a[1, 1] + a[2, 2]
    # the largest of 4w^2, 4x^2, 4y^2, 4z^2 picks the well-conditioned branch
    cand = torch.stack([1 + tr, 1 + a[0, 0] - a[1, 1] - a[2, 2], 1 - a[0, 0] + a[1, 1] - a[2, 2], 1 - a[0, 0] - a[1, 1] + a[2, 2]])
    k = int(cand.argmax())
    s = 2.0 * torch.sqrt(cand[k].clamp_min(1e-300))
    if k == 0:
        q = torch.stack([s / 4, (a[2, 1] - a[1, 2]) / s, (a[0, 2] - a[2, 0]) / s, (a[1, 0] - a[0, 1]) / s])
    elif k == 1:
        q = torch.stack([(a[2, 1] - a[1, 2]) / s, s / 4, (a[0, 1] + a[1, 0]) / s, (a[0, 2] + a[2, 0]) / s])
    elif k == 2:
        q = torch.stack([(a[0, 2] - a[2, 0]) / s, (a[0, 1] + a[1, 0]) / s, s / 4, (a[1, 2] + a[2, 1]) / s])
    else:
        q = torch.stack([(a[1, 0] - a[0, 1]) / s, (a[0, 2] + a[2, 0]) / s, (a[1, 2] + a[2, 1]) / s, s / 4])
    if q[0] < 0:
        q = -q                                   # w >= 0: angle in [0, pi]
    n = q[1:].norm()
    if n < 1e-12:
        return q[1:] * (2.0 / q[0])
    return q[1:] * (2.0 * torch.atan2(n, q[0]) / n)


def matrices_to_pose6(c2w: torch.Tensor) -> torch.Tensor:
    """``(matrix_to_axis_angle(R), t)`` of P camera-to-world matrices [P,4,4] at once -> [P,6] fp64 on the CPU: the same branches
    and formulas as ``matrix_to_axis_angle``, batched (a ``global_BA`` call converts every keyframe pose)."""
    a = torch.as_tensor(c2w).detach().double().cpu().reshape(-1, 4, 4)
    R = a[:, :3, :3]
    d0, d1, d2 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    cand = torch.stack([1 + d0 + d1 + d2, 1 + d0 - d1 - d2, 1 - d0 + d1 - d2, 1 - d0 - d1 + d2], 1)
    k = cand.argmax(1)
    s = 2.0 * torch.sqrt(cand.gather(1, k[:, None])[:, 0].clamp_min(1e-300))
    x, y, z = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
    xy, xz, yz = R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]
    q4 = s / 4
    branches = torch.stack([torch.stack([q4, x / s, y / s, z / s], 1), torch.stack([x / s, q4, xy / s, xz / s], 1),
                            torch.stack([y / s, xy / s, q4, yz / s], 1), torch.stack([z / s, xz / s, yz / s, q4], 1)], 1)      # [P,4 branches,4]
    q = branches[torch.arange(a.shape[0]), k]
    q = torch.where(q[:, :1] < 0, -q, q)                       # w >= 0: angle in [0, pi]
    n = q[:, 1:].norm(dim=1)
    small = n < 1e-12
    scale = torch.where(small, 2.0 / q[:, 0], 2.0 * torch.atan2(n, q[:, 0]) / torch.where(small, torch.ones_like(n), n))
    return torch.cat([q[:, 1:] * scale[:, None], a[:, :3, 3]], 1)


def axis_angle_to_matrix(w: torch.Tensor) -> torch.Tensor:
    """Rodrigues' formula for w [3]: R = I + sin(th)/th K + (1 - cos(th))/th^2 K^2, K = [w]x (the kernels' R(omega)); differentiable."""
    th2 = (w * w).sum()
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    if float(th2.detach()) < 1e-8:
        A, B = 1 - th2 / 6, 0.5 - th2 / 24
    else:
        th = th2.sqrt()
        A, B = torch.sin(th) / th, (1 - torch.cos(th)) / th2
    return torch.eye(3, dtype=w.dtype, device=w.device) + A * K + B * (K @ K)


def pose_matrix(pose6: torch.Tensor) -> torch.Tensor:
    """[4,4] camera-to-world from (omega, t) [6]."""
    pose6 = torch.as_tensor(pose6)
    out = torch.eye(4, dtype=pose6.dtype, device=pose6.device)
    out[:3, :3] = axis_angle_to_matrix(pose6[:3])
    out[:3, 3] = pose6[3:]
    return out


def predict_current_pose(prev2: torch.Tensor, prev: torch.Tensor, const_speed: bool = True) -> torch.Tensor:
    """Co-SLAM's constant-speed initialisation: ``prev @ (inv(prev2) @ prev)`` when ``const_speed`` (the last relative motion
    applied once more), else ``prev``.  Camera-to-world poses [4,4]."""
    if not const_speed:
        return prev.clone()
    return prev @ (torch.linalg.inv(prev2) @ prev)


class TrackerHIP:
    """Co-SLAM ``tracking_render`` on the device for frames of ``H x W`` pixels, with the field ``model`` (a ``NarutoFieldHIP``, e.g.
    ``MappingTrainer.model``) frozen: its handle and parameters are shared, never written, and no gradient is formed for them.  The
    tracker owns its buffers, its ``{seed, counter}`` random word (pixel draw and depth jitter), its training-step buffers and
    workspace: a ``MappingTrainer``'s random state, graphs and batches are left alone.

    ``track(direction, rgb, depth, init_c2w, rand=None)``: the frame's camera-frame ray directions, colours and depths
    (``[H,W,3] [H,W,3] [H,W]`` float32 on the device) and the initial camera-to-world pose [4,4]; returns the tracked pose [4,4].
    ``rand`` [iter, N, S]: each iteration's depth jitter instead of the device's own draw.  ``track`` converts the initial pose on the host
    (one wait per call); ``track_device`` takes it from ``pose_init`` on the device, where the run loop's pose chain puts it
    (``naruto_amd.pose_chain``, ``CoSLAMNarutoHIP(track=True)``)."""

    def __init__(self, model, config: Dict, H: int, W: int, device=None, rng_seed: Optional[int] = None):
        self.tk = tk = tracking_settings(config)
        self.config = config
        self.model = model
        self.H, self.W = int(H), int(W)
        self.iters = int(tk["iter"])
        self.N = N = int(tk["sample"])
        self.edge_h, self.edge_w = int(tk["ignore_edge_H"]), int(tk["ignore_edge_W"])
        if self.edge_h < 0 or self.edge_w < 0 or self.H - 2 * self.edge_h <= 0 or self.W - 2 * self.edge_w <= 0:
            raise ValueError(f"tracking: the edges {self.edge_h} / {self.edge_w} leave no interior of a {self.H} x {self.W} frame")
        self.n_interior = (self.H - 2 * self.edge_h) * (self.W - 2 * self.edge_w)
        if N <= 0 or N > self.n_interior:
            raise ValueError(f"tracking.sample = {N} distinct pixels out of {self.n_interior} interior pixels")
        if self.iters <= 0:
            raise ValueError("tracking.iter must be positive")
        self.device = torch.device(device) if device is not None else model.embed_fn.params.device
        tr, cam, dec = config["training"], config["cam"], config.get("decoder", {})
        self.S = S = int(tr["n_samples_d"]) + int(tr["n_range_d"])
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # get_loss_from_ret's default terms (coslam.py:154-174): rgb, depth, sdf, fs, uncert; no smoothness
        uncert_w = tr["uncert_weight"] if (dec.get("pred_uncert") or dec.get("uncert_grid")) else 0.0
        self.loss_w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, uncert_w, 0.0, 0.0, 0.0, 0.0], **f32)
        if rng_seed is None:
            rng_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.rng = torch.tensor([int(rng_seed), 0], dtype=torch.int64, device=dev)
        self.ts = ops.TrainStep(model._handle(), model._params(), None, N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"],
                                far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                                perturb=tr["perturb"] > 0.0, loss_weights=self.loss_w, rng_state=self.rng, own_grads=False)
        # the frame and the initial pose (omega, t): static, a captured call reads them from here
        self.direction = torch.zeros(self.H, self.W, 3, **f32)
        self.rgb = torch.zeros(self.H, self.W, 3, **f32)
        self.depth = torch.zeros(self.H, self.W, **f32)
        self.pose_init = torch.zeros(6, **f32)
        self.rays_o, self.rays_d = torch.zeros(N, 3, **f32), torch.zeros(N, 3, **f32)
        self.target_rgb, self.target_d = torch.zeros(N, 3, **f32), torch.zeros(N, **f32)
        self.d_cam = torch.zeros(N, 3, **f32)
        self.pix = torch.zeros(N, dtype=torch.int64, device=dev)
        self.d_rays_o, self.d_rays_d = torch.zeros(N, 3, **f32), torch.zeros(N, 3, **f32)
        self.pose, self.exp_avg, self.exp_avg_sq = torch.zeros(6, **f32), torch.zeros(6, **f32), torch.zeros(6, **f32)
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)          # {Adam steps, thresh, stopped, iterations}
        self.best_pose, self.best_loss, self.c2w = torch.zeros(6, **f32), torch.zeros(1, **f32), torch.zeros(4, 4, **f32)
        self.trace_loss = torch.zeros(self.iters, **f32)
        self.trace_pose = torch.zeros(self.iters, 6, **f32)
        self.trace_d_pose = torch.zeros(self.iters, 6, **f32)
        self.ws = _lib.workspace(_lib.load().naruto_track_workspace(model._handle().ptr, N, S), dev, zero=True)
        k = _lib.NarutoTrackStep()
        k.n_rays, k.H, k.W, k.edge_h, k.edge_w = N, self.H, self.W, self.edge_h, self.edge_w
        k.direction, k.rgb, k.depth, k.rng = _p(self.direction), _p(self.rgb), _p(self.depth), _p(self.rng)
        k.d_cam, k.pix = _p(self.d_cam), _p(self.pix)
        k.pose_init, k.pose, k.exp_avg, k.exp_avg_sq, k.state = _p(self.pose_init), _p(self.pose), _p(self.exp_avg), _p(self.exp_avg_sq), _p(self.state)
        k.lr_rot, k.lr_trans, k.beta1, k.beta2, k.eps = float(tk["lr_rot"]), float(tk["lr_trans"]), 0.9, 0.999, 1e-8
        k.wait_iters, k.best = int(tk["wait_iters"]), 1 if tk["best"] else 0
        k.best_pose, k.best_loss, k.c2w = _p(self.best_pose), _p(self.best_loss), _p(self.c2w)
        k.d_rays_o, k.d_rays_d = _p(self.d_rays_o), _p(self.d_rays_d)
        k.trace_loss, k.trace_pose, k.trace_d_pose, k.max_trace = _p(self.trace_loss), _p(self.trace_pose), _p(self.trace_d_pose), self.iters
        k.workspace = _p(self.ws)
        self.k = k
        t = self.ts.t
        t.rays_o, t.rays_d, t.target_rgb, t.target_d = _p(self.rays_o), _p(self.rays_d), _p(self.target_rgb), _p(self.target_d)
        self._graph = None

    def _load(self, direction, rgb, depth, init_c2w):
        check_frame(direction, rgb, depth, self.H, self.W)
        init = torch.as_tensor(init_c2w).detach().double().cpu().reshape(4, 4)
        with torch.no_grad():
            self.direction.copy_(direction)
            self.rgb.copy_(rgb)
            self.depth.copy_(depth)
            self.pose_init.copy_(torch.cat([matrix_to_axis_angle(init[:3, :3]), init[:3, 3]]).float())

    def _launch_prologue(self):
        lib, st = _lib.load(), ops._stream()
        ops.check(lib.naruto_track_draw(C.byref(self.k), C.byref(self.ts.t), st), "naruto_track_draw")
        ops.check(lib.naruto_track_rays(C.byref(self.k), C.byref(self.ts.t), st), "naruto_track_rays")

    def _launch_iteration(self):
        lib, st, ts = _lib.load(), ops._stream(), self.ts
        ops.check(lib.naruto_train_forward(ts.handle.ptr, C.byref(ts.ps), C.byref(ts.t), 1, st), "naruto_train_forward")
        ops.check(lib.naruto_track_backward(ts.handle.ptr, C.byref(ts.ps), C.byref(ts.t), C.byref(self.k), st), "naruto_track_backward")

    def _run(self, rand: Optional[torch.Tensor] = None):
        ts = self.ts
        if rand is not None:
            if tuple(rand.shape) != (self.iters, self.N, self.S):
                raise ValueError(f"tracking: rand must be [{self.iters}, {self.N}, {self.S}], got {list(rand.shape)}")
            ts._set_rng_mode(False)
        try:
            with ops._on_device(self.device):
                self._launch_prologue()
                for i in range(self.iters):
                    if rand is not None:
                        ts.rand[:self.N * self.S].copy_(rand[i].reshape(-1))
                    self._launch_iteration()
        finally:
            if rand is not None:
                ts._set_rng_mode(True)

    def track(self, direction, rgb, depth, init_c2w, rand: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One frame: the tracked camera-to-world pose [4,4] (float32, on the device)."""
        self._load(direction, rgb, depth, init_c2w)
        with torch.no_grad():
            if self._graph is not None and rand is None:
                self._graph.replay()
            else:
                self._run(rand)
        return self.c2w.clone()

    def track_device(self, direction, rgb, depth, rand: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One frame whose initial pose is ALREADY in ``self.pose_init`` as (omega, t) -- ``pose_chain.pose_predict(est, i, const_speed,
        tracker.pose_init)`` wrote it on the device: only the frame is copied, then the captured call is replayed (or run).  Nothing
        goes to the host.  Returns ``self.c2w`` itself, the [4,4] buffer the next call overwrites (``pose_chain.pose_commit`` reads it on
        the same stream).  ``rand``: as in ``track`` (an eager run with the caller's depth jitter)."""
        check_frame(direction, rgb, depth, self.H, self.W)
        with torch.no_grad():
            self.direction.copy_(direction)
            self.rgb.copy_(rgb)
            self.depth.copy_(depth)
            if self._graph is not None and rand is None:
                self._graph.replay()
            else:
                self._run(rand)
        return self.c2w

    def capture(self, warmup: int = 1):
        """Record one call (draw, iteration 0's rays, ``iter`` iterations; no parallel branches) as ONE hipGraph.  Later ``track``
        calls without ``rand`` copy their frame and initial pose into the static buffers and replay it.  The warm-up and the capture
        put the random word back."""
        g = torch.cuda.CUDAGraph()
        with preserved([self.rng]), torch.no_grad():
            warm_up(self.device, lambda _: self._run(), warmup)
            with torch.cuda.graph(g):
                self._launch_prologue()
                for _ in range(self.iters):
                    self._launch_iteration()
            torch.cuda.synchronize(self.device)
        self._graph = g
        return g

    def drawn_pixels(self) -> torch.Tensor:
        """Flat pixel indices ``h * W + w`` [N] (int64) of the last call's rays."""
        return self.pix.clone()

    def last_trace(self) -> Dict:
        """The last call, read when asked: per evaluated iteration ``loss`` [n] (the weighted total), ``pose`` [n,6] (omega, t) and
        ``d_pose`` [n,6] its gradient; ``n_iter`` (iterations evaluated: the one that stopped the call is the last), ``stopped``,
        ``thresh``, ``best_loss``, ``best_pose``."""
        state = self.state.cpu()
        stopped = bool(state[2])
        n = int(state[0]) + 1 if stopped else min(int(state[3]), self.iters)
        return {"loss": self.trace_loss.cpu()[:n].clone(), "pose": self.trace_pose.cpu()[:n].clone(), "d_pose": self.trace_d_pose.cpu()[:n].clone(),
                "n_iter": n, "stopped": stopped, "thresh": int(state[1]), "best_loss": float(self.best_loss.cpu()[0]),
                "best_pose": self.best_pose.cpu().clone()}

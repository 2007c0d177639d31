"""Whole views from the field, and their 2D scores: point a camera at the map and get an image back.

``render_rays`` takes caller-made rays and a measured depth to sample near the surface.  :class:`FieldViewRendererHIP` takes poses: it
makes the rays of every pixel, finds the surface itself and returns RGB, depth, depth variance and uncertainty images, batched over the
poses (P poses x a small image is also what a view-based planner would query).  :func:`image_metrics` scores views against ground
truth (PSNR, SSIM, depth L1) on the device; :func:`evaluate_views` does both against ``MeshSimHIP``.

CONTRACT (PARITY UNPINNED: Co-SLAM's ``render_img`` is not in the reference tree and the surface search is this library's own;
tests/view_spec.py restates the ray rule, the crossing rule and the metrics in numpy, and the kernels equal it in every bit).

Rays.  The pixel at row j, column i of a pose ``c2w`` has the camera-frame direction ((i - cx)/fx, -(j - cy)/fy, -1) in float32, each
operation rounded once (``slam.camera_rays``), taken to the world as ``naruto_rays_to_world`` does it: the result equals
``rays_to_world(camera_rays(...), ids, poses)`` in every bit.

Surface search (no target depth given).  Coarse pass: ``n_coarse`` uniform depths in [cam.near, cam.far] -- the render's
``target_d == NULL`` sampling, no jitter -- through the field query.  Crossing rule: walking the samples from the camera, the first k
with ``sdf[k] > 0`` and ``!(sdf[k+1] > 0)`` (a NaN counts as not positive) gives
``z* = z[k] + (z[k+1] - z[k]) * (sdf[k] / (sdf[k] - sdf[k+1]))``, float32 in exactly that order, no fused multiply-add; a ray without
such a k gets z* = 0, which the sampler treats as "no depth: sample near..far".  Fine pass: the render's depth-guided sampling around z*
with ``training.n_samples_d``, ``n_range_d``, ``range_d``, no jitter, and its compositing.  With ``target_depth`` given the coarse pass
is skipped: Co-SLAM's own evaluation render, guided by the sensor depth.

The fused launch (``naruto_render_view``, one wave per ray) stops the coarse pass after the 64-sample tile that decides the first
crossing; its modular twin (``fused=False``) is ``naruto_view_rays`` -> ``naruto_render_fwd`` (coarse, raw kept) ->
``naruto_view_crossing`` -> ``naruto_render_fwd`` (fine).  Both give the same bits.  A fine pass of at most 64 samples is the render's
packed form (16 rays per workgroup, their samples back to back in 64-sample tiles, OneBlob's form chosen per tile: a sample's bits depend
on the tile it shares), which the fused launch keeps tile for tile; ``ray_chunk`` is rounded up to whole groups of 16 rays and the twin
keeps its launches below the ray count at which ``naruto_render_fwd`` switches to its eight-wave form (another matrix chain, DESIGN.md
7j), so no bit of either depends on ``ray_chunk``.

Metrics: float64 sums per view over float32 images.  PSNR: ``mse = sum (a - b)^2 / (3 H W)``, ``psnr = -10 log10(mse)`` (+inf at 0).
Depth L1: mean ``|d - d_gt|`` over the pixels with ``d_gt > 0`` (and ``d_gt <= depth_trunc`` when given), NaN without any, in cm.
SSIM (Wang et al. 2004): an 11-tap Gaussian window, sigma 1.5, made and normalised in float64 on the host; separable over valid
positions only -- the map is (H-10) x (W-10) per channel -- horizontal pass first, taps ascending, every accumulation from 0.0, no fused
multiply-add; windowed x, y, x^2, y^2, xy; C1 = 0.01^2, C2 = 0.03^2;
``ssim = ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx + sy + C2))``; the score is the mean over channels and positions, NaN when
H or W is below 11.

Command line::

    python -m naruto_amd.render --config <coslam.yaml> --ckpt <ckpt.pt> --mesh <scene.ply | scene.glb | scene.gltf> (--traj traj.txt | --poses)
                                --out_dir D [--every K] [--png] [--result_txt results.txt]

renders every K-th pose of the trajectory file (``--traj``) or of the checkpoint (``--poses``), writes the image stacks as ``.npy`` (with
``--png`` and PIL importable also PNGs; uncertainty through ``mesh.jet_lut``) and the three metrics against the mesh through
``update_results_file``.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from . import culling as CU
from ._lib import check

OUTPUTS = ("rgb", "depth", "depth_var", "uncert_map", "acc_map", "surface_z")
MAX_RAY_SAMPLES = 1024                     # naruto_render_fwd's per-ray LDS limit (kMaxSamples)
SSIM_WINDOW, SSIM_SIGMA = 11, 1.5
_RENDER_FORM_PACKED8 = 2                   # naruto_debug_render_plan's out[0]
RAY_GROUP = 16                             # rays per workgroup of the packed render (kPackRays): launches start at whole groups


def view_camera(config: Dict) -> Dict:
    """``config['cam']`` as ``CoSLAMNarutoHIP`` reads it (divided by ``data.downsample``), with near and far."""
    cam, ds = config["cam"], int(config.get("data", {}).get("downsample", 1))
    out = {"H": cam["H"] // ds, "W": cam["W"] // ds}
    out.update({k: cam[k] // ds if ds != 1 else cam[k] for k in ("fx", "fy", "cx", "cy")})
    out.update({"near": cam["near"], "far": cam["far"]})
    return out


def gaussian_window() -> np.ndarray:
    """The 11 taps of the SSIM window, float64, normalised to sum 1."""
    x = np.arange(SSIM_WINDOW, dtype=np.float64) - (SSIM_WINDOW - 1) / 2.0
    w = np.exp(-(x * x) / (2.0 * SSIM_SIGMA * SSIM_SIGMA))
    return w / w.sum()


class FieldViewRendererHIP:
    """Views of ``model`` (a ``NarutoFieldHIP``) through the pinhole ``cam`` (H, W, fx, fy, cx, cy[, near, far]; default:
    :func:`view_camera` of the config).  Module docstring: the contract."""

    def __init__(self, model, config: Dict, cam: Optional[Dict] = None):
        self.model, self.config = model, config
        base = view_camera(config)
        cam = dict(base if cam is None else cam)
        near, far = float(cam.get("near", base["near"])), float(cam.get("far", base["far"]))
        if not (np.isfinite(near) and np.isfinite(far) and near < far):
            raise ValueError(f"render: need finite near < far (got {near}, {far})")
        self.cam = CU._camera(cam)                                               # (validates the intrinsics; its near > 0 is not asked here: the shipped near is 0)
        self.cam.near_, self.cam.far_ = near, far
        self.H, self.W = self.cam.H, self.cam.W

    def _fine(self):
        tr = self.config["training"]
        return int(tr["n_samples_d"]), int(tr["n_range_d"]), float(tr["range_d"])

    def _check_samples(self, n_coarse: int, searching: bool) -> None:
        nu, nr, _ = self._fine()
        if not 2 <= nu + nr <= MAX_RAY_SAMPLES:
            raise ValueError(f"render: {nu + nr} fine samples per ray (training.n_samples_d + n_range_d): the render takes 2 .. {MAX_RAY_SAMPLES}")
        if searching and not 2 <= int(n_coarse) <= MAX_RAY_SAMPLES:
            raise ValueError(f"render: n_coarse = {n_coarse}: the render takes 2 .. {MAX_RAY_SAMPLES} samples per ray")

    def rays(self, c2ws: torch.Tensor, p0: int, p1: int):
        """(rays_o, rays_d) [p1 - p0, 3] of the flat pixels [p0, p1) of the poses (``naruto_view_rays``)."""
        dev = c2ws.device
        o, d = torch.empty(p1 - p0, 3, dtype=torch.float32, device=dev), torch.empty(p1 - p0, 3, dtype=torch.float32, device=dev)
        with ops._on_device(dev):
            check(_lib.load().naruto_view_rays(C.byref(self.cam), len(c2ws), c2ws.data_ptr(), p0, p1, o.data_ptr(), d.data_ptr(), ops._stream()), "naruto_view_rays")
        return o, d

    def _rows_per_launch(self, n: int, S: int) -> int:
        """Rays per ``naruto_render_fwd`` launch of the modular twin: all ``n``, unless that many would run the eight-wave form."""
        h = self.model._handle()
        out = (C.c_uint32 * 8)()
        check(_lib.load().naruto_debug_render_plan(h.ptr, n, S, int(h.mlp_mode == "bf16"), -1, out), "naruto_debug_render_plan")
        return n if out[0] != _RENDER_FORM_PACKED8 else max(RAY_GROUP, (int(out[3]) - int(out[1])) // RAY_GROUP * RAY_GROUP)

    def _render_fwd(self, rays_o, rays_d, target_d, n_samples: int, want_raw: bool) -> Dict[str, torch.Tensor]:
        nu, nr, range_d = self._fine()
        S = nu + nr if target_d is not None else n_samples
        step = self._rows_per_launch(len(rays_o), S)
        parts = [ops.render_fused(self.model._handle(), self.model._params(), rays_o[a:a + step], rays_d[a:a + step],
                                  None if target_d is None else target_d[a:a + step], near=self.cam.near_, far=self.cam.far_, n_samples_d=nu, n_range_d=nr,
                                  range_d=range_d, n_samples=n_samples, rand=None, want_raw=want_raw) for a in range(0, len(rays_o), step)]
        return parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}

    def crossing(self, raw: torch.Tensor, z_vals: torch.Tensor) -> torch.Tensor:
        """z* [N] of the coarse pass's raw [N,S,5] / z_vals [N,S] (``naruto_view_crossing``)."""
        raw, z_vals = ops._f32c(raw, "raw"), ops._f32c(z_vals, "z_vals")
        out = torch.empty(raw.shape[0], dtype=torch.float32, device=raw.device)
        with ops._on_device(raw.device):
            check(_lib.load().naruto_view_crossing(raw.shape[0], raw.shape[1], raw.data_ptr(), z_vals.data_ptr(), out.data_ptr(), ops._stream()), "naruto_view_crossing")
        return out

    @torch.no_grad()
    def render(self, c2ws, target_depth=None, n_coarse: int = 128, ray_chunk: int = 1 << 16, fused: bool = True, outputs: Sequence[str] = OUTPUTS) -> Dict[str, torch.Tensor]:
        """c2ws [P,4,4] (or [4,4]) -> device tensors ``rgb`` [P,H,W,3] and ``depth``, ``depth_var``, ``uncert_map``, ``acc_map``,
        ``surface_z`` [P,H,W] (those named in ``outputs``).  ``target_depth`` [P,H,W]: the sensor depth guides the sampling and the
        coarse pass is skipped.  The loop over the chunks of ``ray_chunk`` rays has no host synchronisation and no bit of the result
        depends on ``ray_chunk``."""
        unknown = set(outputs) - set(OUTPUTS)
        if unknown or not outputs:
            raise ValueError(f"render: outputs are among {OUTPUTS} (got {sorted(unknown) or 'none'})")
        if int(ray_chunk) < 1:
            raise ValueError("render: ray_chunk >= 1")
        self._check_samples(n_coarse, target_depth is None)
        ray_chunk = -(-int(ray_chunk) // RAY_GROUP) * RAY_GROUP               # whole ray groups: the packed render's tiles then do not move with the chunk
        dev = self.model.embed_fn.params.device
        p = torch.as_tensor(c2ws)
        if p.dim() == 2:
            p = p[None]
        if p.dim() != 3 or p.shape[1:] != (4, 4) or len(p) == 0:
            raise ValueError(f"render: poses must be [P,4,4] with P >= 1, got {tuple(p.shape)}")
        p = p.detach().to(dev, torch.float32).contiguous()
        P, H, W = len(p), self.H, self.W
        N = P * H * W
        if N >= 2 ** 32:
            raise ValueError("render: poses x pixels per call must stay below 2^32")
        td = None
        if target_depth is not None:
            td = ops._f32c(torch.as_tensor(target_depth).to(dev), "target_depth").reshape(-1)
            if td.numel() != N:
                raise ValueError(f"render: target_depth is [P,H,W] = [{P},{H},{W}], got {tuple(torch.as_tensor(target_depth).shape)}")
        out = {k: torch.empty((P, H, W, 3) if k == "rgb" else (P, H, W), dtype=torch.float32, device=dev) for k in OUTPUTS if k in outputs}
        nu, nr, range_d = self._fine()
        if fused:
            r = _lib.NarutoViewRender()
            r.n_poses, r.poses, r.target_d = P, p.data_ptr(), ops._p(td)
            r.n_samples_d, r.n_range_d, r.range_d, r.n_coarse = nu, nr, range_d, int(n_coarse)
            r.rgb, r.depth, r.acc, r.depth_var, r.uncert_map, r.surface_z = (ops._p(out.get(k)) for k in ("rgb", "depth", "acc_map", "depth_var", "uncert_map", "surface_z"))
            ps = ops._params_struct({k: ops._f32c(v.detach(), k) for k, v in self.model._params().items()})
            lib, h = _lib.load(), self.model._handle()
            with ops._on_device(dev):
                for p0 in range(0, N, int(ray_chunk)):
                    r.p0, r.p1 = p0, min(p0 + int(ray_chunk), N)
                    check(lib.naruto_render_view(h.ptr, C.byref(ps), C.byref(self.cam), C.byref(r), ops._stream()), "naruto_render_view")
            return out
        flat = {k: v.reshape(N, 3) if k == "rgb" else v.reshape(N) for k, v in out.items()}
        for p0 in range(0, N, int(ray_chunk)):
            p1 = min(p0 + int(ray_chunk), N)
            rays_o, rays_d = self.rays(p, p0, p1)
            if td is None:
                coarse = self._render_fwd(rays_o, rays_d, None, int(n_coarse), True)
                z_star = self.crossing(coarse["raw"], coarse["z_vals"])
            else:
                z_star = td[p0:p1]
            fine = self._render_fwd(rays_o, rays_d, z_star, 0, False)
            fine["surface_z"] = z_star
            for k, v in flat.items():
                v[p0:p1].copy_(fine[k])
        return out


@torch.no_grad()
def image_metrics(rgb, depth, gt_rgb, gt_depth, depth_trunc: Optional[float] = None, maps: bool = False) -> Dict[str, torch.Tensor]:
    """Views [P,H,W,3] / [P,H,W] (or one view without the leading axis) against ground truth, on the device (module docstring) ->
    float64 device tensors: ``sums`` [P,6] (squared-error sum, pixels, depth-error sum, valid pixels, SSIM sum, SSIM terms) and the
    per-view ``psnr``, ``ssim``, ``depth_l1_cm`` [P]; with ``maps`` also ``se_map`` [P,H,W,3], ``depth_err_map`` [P,H,W] (0 where the
    ground truth is invalid) and ``ssim_map`` [P,H-10,W-10,3].  Bitwise reproducible; nothing comes to the host."""
    rgb = ops._f32c(torch.as_tensor(rgb), "rgb")
    if rgb.dim() == 3:
        rgb = rgb[None]
    if rgb.dim() != 4 or rgb.shape[-1] != 3 or rgb.numel() == 0:
        raise ValueError(f"image_metrics: rgb is [P,H,W,3], got {tuple(rgb.shape)}")
    P, H, W = rgb.shape[:3]
    dev = rgb.device
    depth, gt_depth = (ops._f32c(torch.as_tensor(t).to(dev), n).reshape(-1) for t, n in ((depth, "depth"), (gt_depth, "gt_depth")))
    gt_rgb = ops._f32c(torch.as_tensor(gt_rgb).to(dev), "gt_rgb").reshape(-1)
    if gt_rgb.numel() != rgb.numel() or depth.numel() != P * H * W or gt_depth.numel() != P * H * W:
        raise ValueError("image_metrics: the four image stacks must have the same views and size")
    if depth_trunc is not None and np.isnan(float(depth_trunc)):
        raise ValueError("image_metrics: depth_trunc is not a number")
    lib = _lib.load()
    n_ws = lib.naruto_image_metrics_workspace(P, H, W)
    if n_ws == 0:
        raise ValueError(f"image_metrics: {P} views of {W} x {H} are beyond the supported sizes (65535 views, 2^30 pixels)")
    ws = _lib.workspace(n_ws, dev, torch.float64)
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"sums": torch.empty(P, 6, **f64)}
    if maps:
        out["se_map"], out["depth_err_map"] = torch.empty(P, H, W, 3, **f64), torch.empty(P, H, W, **f64)
        out["ssim_map"] = torch.empty(P, max(H - (SSIM_WINDOW - 1), 0), max(W - (SSIM_WINDOW - 1), 0), 3, **f64)
    win = (C.c_double * SSIM_WINDOW)(*gaussian_window().tolist())
    with ops._on_device(dev):
        check(lib.naruto_image_metrics(P, H, W, rgb.data_ptr(), depth.data_ptr(), gt_rgb.data_ptr(), gt_depth.data_ptr(), int(depth_trunc is not None),
                                       float(depth_trunc or 0.0), win, ws.data_ptr(), out["sums"].data_ptr(), ops._p(out.get("se_map")), ops._p(out.get("depth_err_map")),
                                       ops._p(out.get("ssim_map")) if H >= SSIM_WINDOW and W >= SSIM_WINDOW else None, ops._stream()), "naruto_image_metrics")
    out.update(scores_from_sums(out["sums"]))
    return out


def scores_from_sums(sums) -> Dict:
    """[P,6] float64 sums (torch or numpy) -> per-view ``psnr``, ``ssim``, ``depth_l1_cm``."""
    log10 = torch.log10 if isinstance(sums, torch.Tensor) else np.log10
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = sums[:, 0] / (3.0 * sums[:, 1])
        return {"psnr": -10.0 * log10(mse), "ssim": sums[:, 4] / sums[:, 5], "depth_l1_cm": sums[:, 2] / sums[:, 3] * 100.0}


@torch.no_grad()
def evaluate_views(model, config: Dict, sim, c2ws, depth_guided: bool = False, cam: Optional[Dict] = None, **render_args) -> Dict:
    """Render the poses ``c2ws`` [P,4,4] (the field's frame) and score them against ``sim.simulate_batch`` (a ``MeshSimHIP`` with the
    same camera, in metres: poses and depths go through ``data.sc_factor`` / ``data.translation`` as ``culling.to_metric`` does) ->
    ``psnr``, ``ssim``, ``depth_l1_cm`` (the mean over the views) and ``per_view`` (lists).  ``depth_guided``: the ground-truth depth
    guides the sampling (Co-SLAM's evaluation render).  3 P doubles reach the host."""
    renderer = FieldViewRendererHIP(model, config, cam)
    if (sim.cam.H, sim.cam.W) != (renderer.H, renderer.W):
        raise ValueError(f"evaluate_views: the simulator renders {sim.cam.W} x {sim.cam.H}, the field's camera {renderer.W} x {renderer.H}")
    p = CU._poses(c2ws)
    sc = float(config["data"]["sc_factor"])
    gt_rgb, gt_depth = sim.simulate_batch(CU.to_metric(config, p)[0])[:2]
    views = renderer.render(p, target_depth=(gt_depth if sc == 1.0 else gt_depth * sc) if depth_guided else None, outputs=("rgb", "depth"), **render_args)
    depth = views["depth"] if sc == 1.0 else views["depth"] / sc
    m = image_metrics(views["rgb"], depth, gt_rgb, gt_depth, depth_trunc=None)
    host = torch.stack([m["psnr"], m["ssim"], m["depth_l1_cm"]]).cpu().numpy()
    out = {k: float(np.mean(host[i])) for i, k in enumerate(("psnr", "ssim", "depth_l1_cm"))}
    out["per_view"] = {k: host[i].tolist() for i, k in enumerate(("psnr", "ssim", "depth_l1_cm"))}
    return out


def results_rows(scores: Dict) -> Dict[str, float]:
    """The three lines ``results.txt`` gains."""
    return {"psnr": scores["psnr"], "ssim": scores["ssim"], "depth_l1(cm)": scores["depth_l1_cm"]}


def load_checkpoint(path) -> Dict:
    """``save_ckpt``'s file: {'pose', 'pose_rel', 'model'} (``torch.load(..., weights_only=True)``)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or not isinstance(ckpt.get("model"), dict):
        raise ValueError(f"{path}: no 'model' state dict in the checkpoint")
    return ckpt


def load_field_state(model, state: Dict) -> None:
    """The checkpoint's ``state_dict`` into ``model``: the uncertainty grid takes the checkpoint's shape; the reference's checkpoints
    carry every decoder weight twice (``decoder.sdf_net...`` and the top-level alias ``sdf_net...``), as this module's own do."""
    if "uncert_grid" not in state:
        raise ValueError("checkpoint: no uncert_grid in the model's state dict")
    dev = model.embed_fn.params.device
    model.uncert_grid = torch.nn.parameter.Parameter(torch.as_tensor(state["uncert_grid"]).detach().to(dev, torch.float32).clone())
    model.cache_uncert = np.zeros(tuple(model.uncert_grid.shape), dtype=np.float32)
    model.load_state_dict(state, strict=True)


def field_from_checkpoint(path, config: Dict, device="cuda"):
    """A ``NarutoFieldHIP`` with the checkpoint's weights (the inverse of ``CoSLAMNarutoHIP.save_ckpt`` for the model)."""
    from .field import NarutoFieldHIP
    device = torch.device(device)
    bbox = torch.tensor(config["mapping"]["bound"], dtype=torch.float32, device=device)
    model = NarutoFieldHIP(config, bbox).to(device)
    load_field_state(model, load_checkpoint(path)["model"])
    return model.eval()


def _to_png(path: str, image: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.clip(np.rint(image * 255.0), 0, 255).astype(np.uint8)).save(path)


def write_views(out_dir: str, views: Dict[str, torch.Tensor], png: bool = False) -> None:
    """The image stacks as ``<name>.npy``; with ``png`` (and PIL importable) ``<name>_<view>.png``: depth scaled by its maximum,
    uncertainty through ``mesh.jet_lut`` on its own range."""
    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.cpu().numpy() for k, v in views.items()}
    for k, v in host.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), v)
    if not png:
        return
    try:
        import PIL  # noqa: F401
    except ImportError:
        print("render: PIL is not importable, no PNGs written")
        return
    from .mesh import jet_lut
    lut = jet_lut().numpy()
    for k in ("rgb", "depth", "uncert_map"):
        for i, img in enumerate(host.get(k, ())):
            if k == "depth":
                img = np.repeat((img / max(float(img.max()), 1e-12))[..., None], 3, -1)
            elif k == "uncert_map":
                lo, hi = float(img.min()), float(img.max())
                img = lut[np.clip(np.rint((img - lo) / max(hi - lo, 1e-12) * 255.0), 0, 255).astype(np.int64)]
            _to_png(os.path.join(out_dir, f"{k}_{i:04}.png"), img)


def parse_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m naruto_amd.render", description="Render views of a checkpoint's field and score them against a mesh.")
    parser.add_argument("--config", type=str, required=True, help="Co-SLAM yaml config")
    parser.add_argument("--ckpt", type=str, required=True, help="checkpoint written by save_ckpt")
    parser.add_argument("--mesh", type=str, required=True, help="ground-truth mesh the simulator renders (.ply, or a textured .glb / .gltf)")
    parser.add_argument("--mesh_frame", type=str, default="gltf", choices=["gltf", "mp3d"], help="a glTF scene's frame: as stored, or MP3D's (x, y, z) -> (x, -z, y)")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--traj", type=str, help="Replica trajectory file with the poses to render")
    src.add_argument("--poses", action="store_true", help="render the checkpoint's own poses")
    parser.add_argument("--out_dir", type=str, required=True, help="the image stacks go here")
    parser.add_argument("--every", type=int, default=1, help="render every K-th pose")
    parser.add_argument("--png", action="store_true", help="also write PNGs (needs PIL)")
    parser.add_argument("--result_txt", type=str, help="results file the three metrics are written to")
    parser.add_argument("--depth_guided", action="store_true", help="guide the sampling by the ground-truth depth (Co-SLAM's evaluation render)")
    args = parser.parse_args(argv)
    if args.every < 1:
        parser.error("--every must be positive")
    if not args.mesh.lower().endswith((".ply", ".glb", ".gltf")):
        parser.error(f"--mesh {args.mesh}: only .ply, .glb and .gltf meshes are read")
    return args


def main(argv=None) -> Dict:
    args = parse_args(argv)
    from . import config as cfgmod
    from .evaluation import update_results_file
    from .run import load_replica_traj
    from .simulator import MeshSimHIP
    cfg = cfgmod.load_config(args.config)
    model = field_from_checkpoint(args.ckpt, cfg)
    poses = (load_replica_traj(args.traj) if args.traj else CU.poses_from_checkpoint(args.ckpt))[::args.every]
    cam = view_camera(cfg)
    sim = MeshSimHIP(args.mesh, cam, device=model.embed_fn.params.device, mesh_frame=args.mesh_frame)
    sc = float(cfg["data"]["sc_factor"])
    gt_rgb, gt_depth = sim.simulate_batch(CU.to_metric(cfg, CU._poses(poses))[0])[:2]
    views = FieldViewRendererHIP(model, cfg).render(poses, target_depth=gt_depth * sc if args.depth_guided else None)
    m = image_metrics(views["rgb"], views["depth"] / sc, gt_rgb, gt_depth)
    host = torch.stack([m["psnr"], m["ssim"], m["depth_l1_cm"]]).cpu().numpy()
    scores = {k: float(np.mean(host[i])) for i, k in enumerate(("psnr", "ssim", "depth_l1_cm"))}
    write_views(args.out_dir, views, png=args.png)
    if args.result_txt:
        update_results_file(results_rows(scores), args.result_txt)
    print(f"{len(poses)} views of {cam['W']} x {cam['H']}: psnr {scores['psnr']:.3f} dB, ssim {scores['ssim']:.4f}, depth L1 {scores['depth_l1_cm']:.3f} cm -> {args.out_dir}")
    return scores


if __name__ == "__main__":
    main()

"""Mesh culling on the device: keep the part of a mesh the estimated cameras can have seen.

In the reference's evaluation protocol (scripts/evaluation/eval_replica.sh:55-72) the mesh eval_recon.py scores is not the one save_mesh
wrote but ``mesh_<iter>_final_cull_occlusion.ply``, made by ``third_parties/neural_slam_eval/cull_mesh.py --remove_occlusion`` from the
estimated poses in the checkpoint.  That tool is not part of the reference tree (an empty submodule; it needs ``trimesh`` and off-screen
OpenGL through ``pyrender``), so this is PARITY UNPINNED, as tracking, the BA pose optimiser and the metrics are.  This is the contract,
restated from the published strategy (Co-SLAM / GO-Surf culling), not from that code:

  Inputs: a mesh (vertices, faces, optional vertex colours); poses ``c2w [P,4,4]`` in this repository's camera convention (x right, y up,
  looking along -z; pixel (i, j) has the ray ((i - cx)/fx, -(j - cy)/fy, -1), so pixel centres sit at integer (u, v)); the intrinsics
  H, W, fx, fy, cx, cy of ``config["cam"]``.

  1. Bounds (optional, [3,2]): a vertex is inside iff lo <= p <= hi on all axes; a face survives iff any of its vertices is inside.
  2. One depth map per pose of an occluder mesh, double sided (winding never matters): by default the input mesh's surviving faces,
     or the mesh given as ``occluder=`` (the ground truth, for example).  A pixel nothing covers holds +inf and occludes nothing.
  3. Per vertex and pose: in frustum iff zc > 0 and the vertex rounds to a pixel of the image; observed iff in frustum and, with
     ``remove_occlusion``, zc < D[j,i] + eps (eps = 0.03 m).
  4. A face is kept iff it survived step 1 and any of its three vertices is observed in any pose.  Kept faces stay in their order; the
     vertices no kept face references are dropped, the rest stay in their order; faces are re-indexed, colours carried along.  Nothing
     kept is an empty mesh, not an error.

  Arithmetic: float32 in the operation order written at the top of csrc/naruto_cull.hip (camera space, the homogeneous edge and plane
  values of the rasteriser -- a triangle reaching behind the camera needs no clipping --, the candidate pixel box, the vertex test).
  tests/cull_spec.py restates it in numpy and the kernels equal it in every bit: the depth minimum is an integer atomicMin on the bit
  pattern, so it does not depend on the order of arrival.  Vertices are rounded to float32 for the tests; the culled mesh carries the
  input's own values.

  0. (optional, ``max_edge=``) ``trimesh.remesh.subdivide_to_size`` of the input mesh, restated in naruto_amd/remesh.py (also parity
     unpinned).  To the author's recollection the protocol's tool does this by default at 1.5 cm; that cannot be verified on this stack,
     so here it is off unless asked for.  Without it the granularity is the input mesh's own triangles (<= 3.5 cm edges at
     ``mesh.voxel_final``) and a mesh of large faces is culled by its corners only (the 12 wall triangles of a room seen from inside are
     all culled at 80 x 60).  With it, steps 1, 3 and 4 run on the subdivided mesh and the result is the subdivided, culled mesh.  The
     depth maps of step 2 are still rendered from the INPUT mesh (its faces that survive step 1, or ``occluder=``): the surface is the
     same, so they are the bits they are without ``max_edge``, from up to 16 x fewer triangles.

Left out:
  * the missing-ground-truth-depth rule: this library's frames come from the simulator, there are no stored depth images;
  * virtual cameras.

Command line, with the arguments of the reference's script::

    python -m naruto_amd.culling --config configs/Replica/office0/coslam.yaml --input_mesh M.ply --ckpt_path C.pt [--remove_occlusion]
                                 [--max_edge 0.015 [--max_iter 10]]

writes ``M_cull_occlusion.ply`` (``M_cull_frustum.ply`` without the flag); with ``--max_edge`` the line it prints carries the number of
generations and any faces still longer.  Checkpoint poses and ``mapping.marching_cubes_bound`` live in
the field's frame; the mesh is metric (extract_mesh's last transform), so both go through p / data.sc_factor - data.translation first.
"""

from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import check
from . import mesh as M
from . import remesh as RM

DEFAULT_LARGE_THRESHOLD = 512        # pixels: a triangle whose candidate box is larger is spread over workgroups (k_cull_raster_large)


@dataclass
class RasterPlan:
    """Launch plan of the depth render; the result does not depend on it."""
    large_threshold: int = DEFAULT_LARGE_THRESHOLD


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _camera(cam: Dict, near: float = 0.01, far: float = 10.0) -> _lib.NarutoCullCam:
    try:
        H, W = int(cam["H"]), int(cam["W"])
        fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    except (KeyError, TypeError) as e:
        raise ValueError(f"culling: the camera needs H, W, fx, fy, cx, cy ({e})") from None
    if H < 1 or W < 1:
        raise ValueError(f"culling: image of {W} x {H} pixels")
    if not all(math.isfinite(x) for x in (fx, fy, cx, cy)) or fx == 0.0 or fy == 0.0:
        raise ValueError("culling: intrinsics must be finite with fx, fy != 0")
    if not (0.0 < float(near) < float(far)):
        raise ValueError("culling: need 0 < near < far")
    return _lib.NarutoCullCam(H, W, fx, fy, cx, cy, float(near), float(far))


def _poses(poses) -> torch.Tensor:
    """-> float32 [P,4,4] (host); finite, at least one."""
    p = torch.as_tensor(poses).detach().to(device="cpu", dtype=torch.float32)
    if p.dim() == 2 and p.shape == (4, 4):
        p = p[None]
    if p.dim() != 3 or p.shape[1:] != (4, 4) or len(p) == 0:
        raise ValueError(f"culling: poses must be [P,4,4] with P >= 1, got {tuple(p.shape)}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError("culling: non-finite pose")
    return p.contiguous()


def _as_mesh(mesh):
    """Mesh | (vertices, faces[, colors]) | path -> (vertices, faces, colors or None, kind) with kind 'mesh' or 'tuple'."""
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
        mesh = M.Mesh.load(mesh)
    if isinstance(mesh, M.Mesh):
        return mesh.vertices, mesh.faces, mesh.vertex_colors, "mesh"
    if not isinstance(mesh, (tuple, list)) or len(mesh) not in (2, 3):
        raise ValueError("culling: a mesh is a naruto_amd.mesh.Mesh, a path or (vertices, faces[, colors])")
    return mesh[0], mesh[1], (mesh[2] if len(mesh) == 3 else None), "tuple"


def _geometry(vertices, faces, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (vertices in their own float dtype [V,3], faces int32 [F,3]) contiguous on the device, face indices checked on the host."""
    v, f = torch.as_tensor(vertices), torch.as_tensor(faces)
    if v.is_cuda and device is None:
        device = v.device
    if v.dtype not in (torch.float32, torch.float64):
        v = v.to(torch.float64)
    if v.numel() % 3 or f.numel() % 3:
        raise ValueError("culling: vertices and faces are rows of three")
    n_v, n_f = v.numel() // 3, f.numel() // 3
    if n_f == 0:
        raise ValueError("culling: a mesh without faces")
    lo, hi = (int(x) for x in torch.stack([f.min(), f.max()]).cpu())             # one two-number copy before anything is read through them
    if lo < 0 or hi >= n_v:
        raise ValueError(f"culling: face index out of range ({lo} .. {hi} for {n_v} vertices)")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    v = v.to(device).reshape(-1, 3).contiguous()
    f = f.to(device).reshape(-1, 3).to(torch.int32).contiguous()
    return v, f


def _threshold(plan) -> int:
    t = DEFAULT_LARGE_THRESHOLD if plan is None else int(plan.large_threshold if isinstance(plan, RasterPlan) else plan["large_threshold"])
    if t < 0:
        raise ValueError("culling: the large-route threshold is a pixel count >= 0")
    return min(t, 2 ** 32 - 1)


class _Raster:
    """Workspace and arguments of the depth render of one occluder, reused over the pose chunks."""

    def __init__(self, v32: torch.Tensor, faces: torch.Tensor, cam: _lib.NarutoCullCam, chunk: int, plan, face_mask: Optional[torch.Tensor] = None):
        self.v, self.f, self.cam, self.mask = v32, faces, cam, face_mask
        self.threshold = _threshold(plan)
        # faces x poses per launch stays below 2^28 (the large route's list): a huge mesh gets a smaller chunk
        self.chunk = max(1, min(int(chunk), (2 ** 28 - 1) // max(len(faces), 1), 65535))
        self.ws = _lib.workspace(_lib.load().naruto_render_depth_workspace(len(v32), len(faces), self.chunk), v32.device, torch.int64)
        if self.ws.numel() == 0:
            raise ValueError(f"culling: a mesh of {len(v32)} vertices and {len(faces)} faces is beyond the depth render's sizes")

    def render(self, poses: torch.Tensor, out: torch.Tensor) -> None:
        """poses [B,4,4] float32 on the device, B <= chunk -> out [B,H,W] (+inf where nothing is hit)."""
        check(_lib.load().naruto_render_depth(C.byref(self.cam), len(self.v), self.v.data_ptr(), len(self.f), self.f.data_ptr(),
                                              self.mask.data_ptr() if self.mask is not None else None, len(poses), poses.data_ptr(), self.threshold,
                                              self.ws.data_ptr(), out.data_ptr(), _stream()), "naruto_render_depth")


def render_depth(vertices, faces, poses, cam: Dict, near: float = 0.01, far: float = 10.0, pose_chunk: int = 8, plan=None, keep_inf: bool = False) -> torch.Tensor:
    """Depth maps of a double-sided mesh: float32 [P,H,W] on the device, z along the viewing axis.  Pixels nothing covers inside
    (near, far) come back as 0, the usual depth-image convention (``keep_inf``: +inf, as the cull holds them).  ``plan``: a
    :class:`RasterPlan`; every bit of the result is independent of it and of ``pose_chunk``."""
    c = _camera(cam, near, far)
    p = _poses(poses)
    if int(pose_chunk) < 1:
        raise ValueError("culling: pose_chunk >= 1")
    v, f = _geometry(vertices, faces)
    with torch.cuda.device(v.device):
        r = _Raster(v.to(torch.float32), f, c, pose_chunk, plan)
        pd = p.to(v.device)
        out = torch.empty(len(p), c.H, c.W, dtype=torch.float32, device=v.device)
        for s in range(0, len(p), r.chunk):
            r.render(pd[s:s + r.chunk], out[s:s + r.chunk])
        if not keep_inf:
            out = torch.where(torch.isinf(out), torch.zeros_like(out), out)
    return out


def _observe(v32: torch.Tensor, poses: torch.Tensor, cam: _lib.NarutoCullCam, depth: Optional[torch.Tensor], eps: float, mask: torch.Tensor) -> None:
    check(_lib.load().naruto_observed_vertices(C.byref(cam), len(v32), v32.data_ptr(), len(poses), poses.data_ptr(), depth.data_ptr() if depth is not None else None,
                                               float(eps), mask.data_ptr(), _stream()), "naruto_observed_vertices")


def observed_vertices(vertices, poses, cam: Dict, depth=None, eps: float = 0.03) -> torch.Tensor:
    """bool [V] on the device: the vertex is in the frustum of some pose and, with ``depth`` (float32 [P,H,W]; 0 or +inf = nothing
    there), not behind it: zc < depth + eps."""
    c = _camera(cam)
    p = _poses(poses)
    if math.isnan(float(eps)):
        raise ValueError("culling: eps is not a number")
    v = torch.as_tensor(vertices)
    device = v.device if v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    v32 = v.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    mask = torch.zeros(len(v32), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        d = None
        if depth is not None:
            d = torch.as_tensor(depth).to(device=device, dtype=torch.float32)
            if tuple(d.shape) != (len(p), c.H, c.W):
                raise ValueError(f"culling: depth must be [P,H,W] = {(len(p), c.H, c.W)}, got {tuple(d.shape)}")
            d = torch.where(d == 0, torch.full_like(d, float("inf")), d).contiguous()
        _observe(v32, p.to(device), c, d, eps, mask)
    return mask.bool()


def _face_flags(faces: torch.Tensor, n_vertices: int, observed: Optional[torch.Tensor], inside: Optional[torch.Tensor], want_vertices: bool):
    keep = torch.empty(len(faces), dtype=torch.uint8, device=faces.device)
    used = torch.empty(n_vertices, dtype=torch.uint8, device=faces.device) if want_vertices else None
    check(_lib.load().naruto_cull_faces(len(faces), n_vertices, faces.data_ptr(), observed.data_ptr() if observed is not None else None,
                                        inside.data_ptr() if inside is not None else None, keep.data_ptr(), used.data_ptr() if used is not None else None, _stream()),
          "naruto_cull_faces")
    return keep, used


def cull_mesh(mesh, poses, cam: Dict, bounds=None, remove_occlusion: bool = True, occluder=None, eps: float = 0.03, near: float = 0.01, far: float = 10.0,
              pose_chunk: int = 8, plan=None, max_edge: Optional[float] = None, max_iter: int = RM.DEFAULT_MAX_ITER, max_faces: int = RM.DEFAULT_MAX_FACES):
    """The culled mesh (module docstring); with ``max_edge`` the subdivided, culled one (step 0; ``max_iter``, ``max_faces``:
    :func:`naruto_amd.remesh.subdivide_to_size`), as the protocol's output file is; ``max_edge=None`` launches what it always launched.
    ``mesh``: a :class:`naruto_amd.mesh.Mesh` or the path of a ``.ply`` (or of a ``.glb`` / ``.gltf``: its geometry) -> a Mesh (float64 vertices, int64 faces, colours carried along); a tuple (vertices, faces[, colors RGBA8 [V,4]]) of arrays or device tensors -> the same tuple
    as device tensors (vertices in their own dtype, faces int32), so a caller can stay on the device.  The loop over the pose chunks has
    no host synchronisation; one copy of two numbers at the end reads the kept counts (the subdivision reads two more per generation)."""
    return _cull(mesh, poses, cam, bounds, remove_occlusion, occluder, eps, near, far, pose_chunk, plan, max_edge, max_iter, max_faces)[0]


def _cull(mesh, poses, cam, bounds, remove_occlusion, occluder, eps, near, far, pose_chunk, plan, max_edge, max_iter, max_faces):
    """cull_mesh -> (the culled mesh, the subdivision's SubdivideResult or None)."""
    c = _camera(cam, near, far)
    p = _poses(poses)
    if math.isnan(float(eps)):
        raise ValueError("culling: eps is not a number")
    if int(pose_chunk) < 1:
        raise ValueError("culling: pose_chunk >= 1")
    if max_edge is not None:
        RM.check_arguments(max_edge, max_iter, max_faces)
    vertices, faces, colors, kind = _as_mesh(mesh)
    v, f = _geometry(vertices, faces)
    device = v.device
    col = None
    if colors is not None:
        col = torch.as_tensor(colors).to(device=device, dtype=torch.uint8).reshape(-1, 4).contiguous()
        if len(col) != len(v):
            raise ValueError("culling: one RGBA colour per vertex")
    b = None
    if bounds is not None:
        b = torch.as_tensor(bounds, dtype=torch.float64).reshape(3, 2)
        if not bool(torch.isfinite(b).all()):
            raise ValueError("culling: non-finite bounds")
    occ = None
    if occluder is not None and remove_occlusion:
        ov, of, _, _ = _as_mesh(occluder)
        occ = _geometry(ov, of, device)

    def result(vo, fo, co):
        if kind == "mesh":
            return M.Mesh(vo.to(torch.float64).cpu().numpy(), fo.to(torch.int64).cpu().numpy(), co.cpu().numpy() if co is not None else None)
        return (vo, fo, co) if colors is not None else (vo, fo)

    with torch.cuda.device(device):
        v32 = v.to(torch.float32)
        inside = alive = None
        bd = b.to(device=device, dtype=v.dtype) if b is not None else None
        if bd is not None:
            inside = ((v >= bd[:, 0]) & (v <= bd[:, 1])).all(1).to(torch.uint8).contiguous()
            alive, _ = _face_flags(f, len(v), None, inside, False)
        pd = p.to(device)
        raster = depth = None
        chunk = int(pose_chunk)
        if remove_occlusion:
            raster = _Raster(occ[0].to(torch.float32), occ[1], c, chunk, plan) if occ is not None else _Raster(v32, f, c, chunk, plan, alive)
            chunk = raster.chunk
            depth = torch.empty(chunk, c.H, c.W, dtype=torch.float32, device=device)
        sub = None
        if max_edge is not None:
            # step 0.  The raster above keeps the input mesh: the same surface and the same depth bits as without max_edge, from up to 16 x
            # fewer triangles after two generations.  Bounds, vertex test, keep rule and compaction run on the subdivided mesh.
            v, f, col, sub = RM.subdivide_on_device(v, f, col, float(max_edge), int(max_iter), int(max_faces))
            v32 = v.to(torch.float32)
            if bd is not None:
                inside = ((v >= bd[:, 0]) & (v <= bd[:, 1])).all(1).to(torch.uint8).contiguous()
        observed = torch.zeros(len(v), dtype=torch.uint8, device=device)
        for s in range(0, len(pd), chunk):                                       # (no host synchronisation in here)
            part = pd[s:s + chunk]
            if raster is not None:
                raster.render(part, depth[:len(part)])
            _observe(v32, part, c, depth, eps, observed)
        keep, used = _face_flags(f, len(v), observed, inside, True)
        face_pos = torch.cumsum(keep, 0, dtype=torch.int32)
        vertex_pos = torch.cumsum(used, 0, dtype=torch.int32)
        n_f, n_v = (int(x) for x in torch.stack([face_pos[-1], vertex_pos[-1]]).cpu())        # the one host sync: output sizes
        out_f = torch.empty(n_f, 3, dtype=torch.int32, device=device)
        out_v = torch.empty(n_v, 3, dtype=v.dtype, device=device)
        out_c = torch.empty(n_v, 4, dtype=torch.uint8, device=device) if col is not None else None
        check(_lib.load().naruto_cull_compact(len(f), len(v), f.data_ptr(), keep.data_ptr(), face_pos.data_ptr(), used.data_ptr(), vertex_pos.data_ptr(), v.data_ptr(),
                                              int(v.dtype == torch.float64), col.data_ptr() if col is not None else None, n_f, n_v, out_f.data_ptr(), out_v.data_ptr(),
                                              out_c.data_ptr() if out_c is not None else None, _stream()), "naruto_cull_compact")
    return result(out_v, out_f, out_c), sub


def poses_from_checkpoint(path) -> torch.Tensor:
    """``ckpt["pose"]``, the dict frame id -> [4,4] that save_ckpt writes (coslam.py:514), as float32 [P,4,4] sorted by frame id."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or "pose" not in ckpt or not isinstance(ckpt["pose"], dict) or len(ckpt["pose"]) == 0:
        raise ValueError(f"{path}: no 'pose' dict of frame id -> [4,4] in the checkpoint")
    poses = ckpt["pose"]
    return torch.stack([torch.as_tensor(poses[k]).detach().to(torch.float32).reshape(4, 4) for k in sorted(poses)])


def culled_path(input_mesh: str, remove_occlusion: bool) -> str:
    """M.ply -> M_cull_occlusion.ply (the name eval_replica.sh reads) or M_cull_frustum.ply."""
    stem, ext = os.path.splitext(input_mesh)
    return f"{stem}_cull_{'occlusion' if remove_occlusion else 'frustum'}{ext or '.ply'}"


def to_metric(config: Dict, poses: torch.Tensor, bounds=None):
    """Checkpoint poses and the marching-cubes bound from the field's frame into the mesh's (extract_mesh: p / sc_factor - translation)."""
    sc, tr = float(config["data"]["sc_factor"]), float(config["data"]["translation"])
    p = poses.clone()
    p[:, :3, 3] = p[:, :3, 3] / sc - tr
    if bounds is not None:
        bounds = torch.as_tensor(bounds, dtype=torch.float64).reshape(3, 2) / sc - tr
    return p, bounds


def main(argv=None) -> str:
    import argparse
    from . import config as cfgmod
    parser = argparse.ArgumentParser(prog="python -m naruto_amd.culling", description="Arguments to cull the mesh.")
    parser.add_argument("--config", type=str, required=True, help="path to the config file")
    parser.add_argument("--input_mesh", type=str, required=True, help="path to the mesh to be culled (.ply)")
    parser.add_argument("--ckpt_path", type=str, required=True, help="checkpoint with the estimated poses")
    parser.add_argument("--remove_occlusion", action="store_true", help="also remove the surface hidden behind the mesh itself")
    parser.add_argument("--max_edge", type=float, default=None, help="subdivide to this edge length (metres) before culling; the protocol's tool uses 0.015; off when absent")
    parser.add_argument("--max_iter", type=int, default=RM.DEFAULT_MAX_ITER, help="generations of subdivision at the most")
    args = parser.parse_args(argv)
    if not args.input_mesh.lower().endswith((".ply", ".glb", ".gltf")):
        raise ValueError(f"{args.input_mesh}: only .ply, .glb and .gltf meshes are read")
    cfg = cfgmod.load_config(args.config)
    poses, bounds = to_metric(cfg, poses_from_checkpoint(args.ckpt_path), cfg.get("mapping", {}).get("marching_cubes_bound"))
    mesh, sub = _cull(M.Mesh.load(args.input_mesh), poses, cfg["cam"], bounds, args.remove_occlusion, None, 0.03, 0.01, 10.0, 8, None, args.max_edge, args.max_iter,
                      RM.DEFAULT_MAX_FACES)
    out = culled_path(args.input_mesh, args.remove_occlusion)
    mesh.export(out)
    line = f"{out}: {len(mesh.vertices)} vertices, {len(mesh.faces)} faces"
    if sub is not None:
        line += f"; subdivided to {args.max_edge} m in {sub.generations} generations"
        if sub.remaining_long:
            line += f", {sub.remaining_long} faces still longer"
    print(line)
    return out


if __name__ == "__main__":
    main()

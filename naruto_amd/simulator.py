"""Mesh simulator on the device: a triangle mesh in the place of the reference's HabitatSim.

The reference's run loop (src/naruto/main.py) starts every step with ``sim.simulate(c2w)``: an RGB-D frame from Habitat-Sim at the
planned pose, and -- with ``return_erp`` -- an equirectangular (ERP) colour image and radial-distance map, which the planner's movement
check reads (``NarutoPlanner.detect_collision_v2``, naruto_planner.py:544-547: ``erp_depth.min()`` and the share of pixels above 1e6).
Habitat-Sim is an external renderer that is not on this stack.  :class:`MeshSimHIP` renders a mesh instead -- a ground-truth ``.ply``,
a textured ``.glb`` / ``.gltf`` scene (``naruto_amd.gltf``), the room-plus-sphere of ``naruto_amd.synthetic``, or a mesh this library
extracted -- with the call surface of ``HabitatSim.simulate``.

PARITY UNPINNED against Habitat.  Pinned, by the reference's recorded results (tests/golden/g13_c2e.npz): the cube-to-panorama gather
(``C2E``, src/layers/c2e.py, through :func:`cube_table`) and ``erp_conversions.depth2dist`` (:func:`depth_to_dist`).  Differences from
Habitat:

  * colours are the vertex colours interpolated in float32 or, on faces with a material, its base colour: the factor, times one
    bilinear tap of the base-colour texture at one mip level; a mesh with neither renders white;
  * no lighting, no alpha (blended and masked materials render opaque), no trilinear or anisotropic filtering, no texture
    transform, no physics, no objects;
  * the reference's ``depth2dist`` call uses ``K = face_w / 2``, half a pixel off the grid ``C2E`` samples; the simulator uses the
    consistent ``(face_w - 1) / 2``.  :func:`depth_to_dist` takes any intrinsics;
  * the front half of ``ERPDepth2Dist`` -- six bilinear ``E2P`` resamplings of a Habitat ERP image into cube faces -- is NOT built:
    a mesh renders its cube faces directly.

Contract (float32 in the operation order at the top of csrc/naruto_sim.hip; tests/sim_spec.py restates it in numpy and the kernels equal
it in every bit):

  Camera: this repository's convention -- x right, y up, looking along -z; pixel (i, j) has the ray ((i - cx)/fx, -(j - cy)/fy, -1);
  ``depth`` is z along the viewing axis.  The rasteriser is the culling's (naruto_amd/culling.py): homogeneous, double sided, no
  clipping.  Per pixel the nearest hit inside (near, far) wins; among the faces whose depth equals the minimum in every bit, the lowest
  face index.  Colour: perspective-correct barycentrics from the rasteriser's own edge values.  A pixel nothing covers has depth 0
  (Habitat's invalid value; Co-SLAM masks ``depth > 0``), colour 0 and face id -1.

  Materials (a :class:`naruto_amd.mesh.TexturedMesh`): the rasteriser, depth and face id do not change.  A hit pixel's colour by its
  face's material: -1: the vertex colours, in the untextured render's bits; a material without a texture: factor.rgb; a texture:
  u = (w_a*u_a + w_b*u_b) + w_c*u_c (v likewise); the same expression at the rays of pixels (i+1, j) and (i, j+1) with the same face's
  edge values gives (u_x, v_x) and (u_y, v_y); ax = (u_x - u)*W0, bx = (v_x - v)*H0, rx = ax*ax + bx*bx, ry likewise from (u_y, v_y);
  rho2 = rx, or ry where ry > rx; level = the number of k in 0 .. n_levels-2 with rho2 > 4^k (NaN: level 0; no blend between levels).
  One bilinear tap at the level's size (w, h), uv (0, 0) the corner of the first stored row: x = u*w - 0.5f, y = v*h - 0.5f; unless
  |x| < 2^30 and |y| < 2^30 the texel colour is 0; x0 = floor(x), a = x - x0 (y0, b likewise); x0, x0+1, y0, y0+1 wrapped by the
  axis's mode (REPEAT: mod w; MIRRORED_REPEAT: m = mod 2w, m < w ? m : 2w-1-m; CLAMP_TO_EDGE: clamp); t = byte/255.0f;
  top = t00 + a*(t10 - t00), bot = t01 + a*(t11 - t01), c = top + b*(bot - top); colour = c * factor.  Alpha is stored and ignored.
  The mip chains: :func:`texture_pyramid`.  tests/sim_texture_spec.py restates all of it.

  Cube faces, in the reference's order F R B L U D, each a ``face_w`` x ``face_w`` pinhole image with fx = fy = cx = cy = (face_w-1)/2
  (pixel i at tangent -1 + 2i/(face_w-1), as C2E assumes) and pose ``c2w @ R_face``; right, up and view vectors in the camera frame:
  F identity; R, B, L yawed right by 90, 180, 270 degrees about +y; U right +x, up +z, view +y; D right +x, up -z, view -y.

  Panorama [h, w]: pixel (row, col) reads the cube pixel ``cube_table(face_w, h, w)[row, col]``.  Its centre column looks along the
  camera's -z, u grows toward +x and v toward +y: the direction is (cos v sin u, sin v, -cos v cos u).  ``erp_depth`` is the radial
  distance t * sqrt(dx^2 + dy^2 + 1) along the chosen cube pixel's ray; nothing hit: 1e8 * that norm (the reference sets invalid depth to
  1e8 before its conversion and tests > 1e6).
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from . import culling as CU

FACE_ORDER = "FRBLUD"


def face_rotations() -> np.ndarray:
    """float64 [6,3,3]: R_face with columns (right, up, -view) in the camera frame, order F R B L U D."""
    x, y, z = np.eye(3)
    frames = [(x, y, -z), (z, y, x), (-x, y, z), (-z, y, -x), (x, z, y), (x, -z, -y)]               # (right, up, view)
    return np.stack([np.stack([r, u, -v], 1) for r, u, v in frames])


def cube_grid(face_w: int, h: int, w: int) -> np.ndarray:
    """The normalised sampling grid of the reference's C2E(face_w, h, w), float32 [h,w,3] = (x, y, face) in [-1, 1], restated from its
    mathematics: float32 linspace angles (numpy keeps their trigonometry in float32), the face-type map with its rolled ceiling mask,
    the tangent formulas accumulated in float64 -- clip to +-0.5, (. + 0.5) * (face_w - 1), normalise to [-1, 1] -- cast to float32."""
    face_w, h, w = int(face_w), int(h), int(w)
    if face_w < 2:
        raise ValueError("simulator: face_w >= 2")
    if h < 2 or w < 8 or w % 8:
        raise ValueError(f"simulator: a panorama of {w} x {h}: need h >= 2 and w a multiple of 8")
    u = np.linspace(-np.pi, np.pi, num=w, dtype=np.float32)
    v = np.linspace(np.pi, -np.pi, num=h, dtype=np.float32) / 2
    u, v = np.meshgrid(u, v)
    # face type: four vertical bands F R B L (F centred), then the ceiling and the floor where |v| is beyond the band's upper edge
    q, roll = w // 4, 3 * w // 8
    tp = np.roll(np.repeat(np.arange(4), q)[None].repeat(h, 0), roll, 1)
    edge = h // 2 - np.round(np.arctan(np.cos(np.linspace(-np.pi, np.pi, q) / 4)) * h / np.pi).astype(int)
    ceil = np.roll(np.tile(np.arange(h)[:, None] < edge[None], (1, 4)), roll, 1)
    tp[ceil] = 4
    tp[ceil[::-1]] = 5
    x, y = np.zeros((h, w)), np.zeros((h, w))
    for k in range(4):
        m = tp == k
        yaw = u[m] - np.pi * k / 2
        x[m] = 0.5 * np.tan(yaw)
        y[m] = -0.5 * np.tan(v[m]) / np.cos(yaw)
    for k, sign in ((4, 1.0), (5, -1.0)):
        m = tp == k
        c = 0.5 * np.tan(np.pi / 2 - np.abs(v[m]))
        x[m] = c * np.sin(u[m])
        y[m] = sign * c * np.cos(u[m])
    x = (np.clip(x, -0.5, 0.5) + 0.5) * (face_w - 1)
    y = (np.clip(y, -0.5, 0.5) + 0.5) * (face_w - 1)
    return np.stack([x / (face_w - 1) * 2 - 1, y / (face_w - 1) * 2 - 1, tp.astype(np.float64) / 5 * 2 - 1], -1).astype(np.float32)


def cube_table(face_w: int, h: int, w: int) -> np.ndarray:
    """int32 [h,w]: the word of a cube map [6, face_w, face_w] that panorama pixel (row, col) reads -- C2E.forward(mode='nearest'), i.e.
    grid_sample's own rule on :func:`cube_grid`: ((g + 1)/2) * (size - 1) in float32, rounded half to even."""
    g = cube_grid(face_w, h, w)

    def nearest(c, size):
        return np.rint(((c + np.float32(1)) / np.float32(2)) * np.float32(size - 1)).astype(np.int64)

    return ((nearest(g[..., 2], 6) * face_w + nearest(g[..., 1], face_w)) * face_w + nearest(g[..., 0], face_w)).astype(np.int32)


def _device(device) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _table_on(table, n_cube: int, device) -> torch.Tensor:
    t = torch.as_tensor(table)
    if t.dtype not in (torch.int32, torch.int64) or t.numel() == 0:
        raise ValueError("simulator: the table is a non-empty int32 array of cube indices")
    lo, hi = (int(x) for x in torch.stack([t.min(), t.max()]).cpu())
    if lo < 0 or hi >= n_cube:
        raise ValueError(f"simulator: table entry out of range ({lo} .. {hi} for a cube of {n_cube} words)")
    return t.to(device=device, dtype=torch.int32).contiguous()


def cube_to_erp(cube, table) -> torch.Tensor:
    """Nearest gather of a cube map [C,6,s,s] (any 4-byte dtype) to the panorama [C,h,w] through ``table`` [h,w] (:func:`cube_table`)."""
    c = torch.as_tensor(cube)
    if c.dim() != 4 or c.shape[1] != 6 or c.shape[2] != c.shape[3] or c.element_size() != 4:
        raise ValueError(f"simulator: a cube map is [C,6,s,s] of a 4-byte dtype, got {tuple(c.shape)} {c.dtype}")
    device = c.device if c.is_cuda else _device(None)
    t = torch.as_tensor(table)
    if t.dim() != 2:
        raise ValueError("simulator: the table is [h,w]")
    s = int(c.shape[2])
    td = _table_on(t, 6 * s * s, device)
    c = c.to(device).contiguous()
    out = torch.empty(c.shape[0], *t.shape, dtype=c.dtype, device=device)
    with torch.cuda.device(device):
        check(_lib.load().naruto_cube_to_erp(c.shape[0], s, td.numel(), td.data_ptr(), c.data_ptr(), out.data_ptr(), CU._stream()), "naruto_cube_to_erp")
    return out


def depth_to_dist(depth, fx: float, fy: float, cx: float, cy: float) -> torch.Tensor:
    """Perspective depth [N,H,W] (or [H,W]) to the distance along the pixel ray: depth * sqrt(((i-cx)/fx)^2 + ((j-cy)/fy)^2 + 1)
    (reference erp_conversions.depth2dist with K = [[fx,0,cx],[0,fy,cy],[0,0,1]])."""
    d = torch.as_tensor(depth)
    one = d.dim() == 2
    if one:
        d = d[None]
    if d.dim() != 3 or d.numel() == 0:
        raise ValueError(f"simulator: depth is [N,H,W], got {tuple(d.shape)}")
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    if not all(math.isfinite(x) for x in (fx, fy, cx, cy)) or fx == 0.0 or fy == 0.0:
        raise ValueError("simulator: intrinsics must be finite with fx, fy != 0")
    device = d.device if d.is_cuda else _device(None)
    d = d.to(device=device, dtype=torch.float32).contiguous()
    out = torch.empty_like(d)
    with torch.cuda.device(device):
        check(_lib.load().naruto_depth_to_dist(d.shape[0], d.shape[1], d.shape[2], fx, fy, cx, cy, d.data_ptr(), out.data_ptr(), CU._stream()), "naruto_depth_to_dist")
    return out[0] if one else out


def _colors(colors, n_vertices: int):
    """None | RGBA8 [V,4] | float [V,3] -> (host tensor uint8 [V,4] or float32 [V,3], is_float)."""
    if colors is None:
        return torch.full((n_vertices, 4), 255, dtype=torch.uint8), False
    c = torch.as_tensor(colors)
    if c.dtype == torch.uint8:
        if c.numel() != 4 * n_vertices:
            raise ValueError(f"simulator: one RGBA8 colour per vertex ({c.numel()} bytes for {n_vertices} vertices)")
        return c.reshape(-1, 4), False
    if not c.dtype.is_floating_point:
        raise ValueError("simulator: vertex colours are RGBA8 [V,4] or float [V,3]")
    if c.numel() != 3 * n_vertices:
        raise ValueError(f"simulator: one float RGB colour per vertex ({c.numel()} values for {n_vertices} vertices)")
    if not bool(torch.isfinite(c).all()):
        raise ValueError("simulator: non-finite vertex colour")
    return c.reshape(-1, 3).to(torch.float32), True


WRAP_MODES = (10497, 33648, 33071)                     # glTF's REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE
MAX_TEXTURE_SIDE = 16384
MAX_UV = 1024.0


def _images(images):
    """-> [uint8 [H,W,4] contiguous host arrays], checked."""
    out = []
    for k, im in enumerate(images):
        a = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or not (1 <= a.shape[0] <= MAX_TEXTURE_SIDE and 1 <= a.shape[1] <= MAX_TEXTURE_SIDE):
            raise ValueError(f"simulator: texture {k} is {a.dtype} {a.shape}: uint8 [H,W,4] with sides 1 .. {MAX_TEXTURE_SIDE}")
        out.append(np.ascontiguousarray(a))
    if not out:
        raise ValueError("simulator: no texture")
    return out


def texture_pyramid(images, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Textures (uint8 [H,W,4] each) -> (texels int32 [n_words], desc int32 [n,4]) on the device: every texture's mip chain in one buffer
    of RGBA8 words (R in the lowest byte), level after level, built on the device in integers -- level l+1 is max(1, w >> 1) x
    max(1, h >> 1), each channel (t(xa,ya) + t(xb,ya) + t(xa,yb) + t(xb,yb) + 2) >> 2 over xa = min(2x, w-1), xb = min(2x+1, w-1) and ya,
    yb likewise; desc = word offset of level 0, W, H, n_levels = 1 + floor(log2(max(W, H)))."""
    ims = _images(images)
    device = _device(device)
    lib = _lib.load()
    words = [lib.naruto_tex_bytes(a.shape[1], a.shape[0]) // 4 for a in ims]
    if sum(words) >= 2 ** 32:
        raise ValueError("simulator: the textures' mip chains must hold fewer than 2^32 texels")
    texels = torch.empty(sum(words), dtype=torch.int32, device=device)
    desc = torch.empty(len(ims), 4, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        off = 0
        for k, a in enumerate(ims):
            check(lib.naruto_tex_build(a.shape[1], a.shape[0], off, a.ctypes.data, desc[k].data_ptr(), texels.data_ptr(), CU._stream()), "naruto_tex_build")
            off += words[k]
    return texels, desc


class _Textures:
    """The material side of a :class:`naruto_amd.mesh.TexturedMesh` on the device, validated on the host: ``struct`` is the
    ``NarutoSimTextures`` the render takes (this object keeps its tensors alive)."""

    def __init__(self, mesh, n_vertices: int, n_faces: int, device):
        fm = np.asarray(mesh.face_material)
        if fm.shape != (n_faces,) or fm.dtype.kind not in "iu":
            raise ValueError(f"simulator: face_material is one integer per face ({fm.shape} for {n_faces} faces)")
        n_mat = len(mesh.materials)
        if int(fm.min()) < -1 or int(fm.max()) >= n_mat:
            raise ValueError(f"simulator: face material out of range ({int(fm.min())} .. {int(fm.max())} for {n_mat} materials; -1: none)")
        uv = np.asarray(mesh.uv if mesh.uv is not None else np.zeros((n_vertices, 2)), dtype=np.float32)
        if uv.shape != (n_vertices, 2):
            raise ValueError(f"simulator: uv is [V,2] ({uv.shape} for {n_vertices} vertices)")
        if not np.isfinite(uv).all() or float(np.abs(uv).max(initial=0.0)) > MAX_UV:
            raise ValueError(f"simulator: uv must be finite with |uv| <= {MAX_UV:g}")
        n_tex = len(mesh.textures)
        table = np.zeros((n_mat, 8), dtype=np.uint32)
        for k, m in enumerate(mesh.materials):
            tex, ws, wt, factor = (m.texture, m.wrap_s, m.wrap_t, m.factor) if hasattr(m, "texture") else m
            factor = np.asarray(factor, dtype=np.float32).reshape(-1)
            if int(tex) < -1 or int(tex) >= n_tex:
                raise ValueError(f"simulator: material {k} names texture {tex} of {n_tex} (-1: none)")
            if int(ws) not in WRAP_MODES or int(wt) not in WRAP_MODES:
                raise ValueError(f"simulator: material {k} has wrap modes {ws}, {wt} (10497, 33648 or 33071)")
            if factor.shape != (4,) or not np.isfinite(factor).all():
                raise ValueError(f"simulator: material {k}'s factor is four finite numbers")
            table[k, 0], table[k, 1], table[k, 2] = np.int32(tex).astype(np.uint32), int(ws), int(wt)
            table[k, 4:] = factor.view(np.uint32)
        self.uv = torch.from_numpy(uv.copy()).to(device).contiguous()
        self.face_material = torch.from_numpy(fm.astype(np.int32)).to(device).contiguous()
        self.materials = torch.from_numpy(table.view(np.int32)).to(device).contiguous()
        self.texels, self.desc = texture_pyramid(mesh.textures, device) if n_tex else (None, None)
        ptr = lambda t: t.data_ptr() if t is not None else None                                                   # noqa: E731
        self.struct = _lib.NarutoSimTextures(C.sizeof(_lib.NarutoSimTextures), n_mat, n_tex, 0, self.texels.numel() if n_tex else 0, self.uv.data_ptr(),
                                             self.face_material.data_ptr(), ptr(self.materials) if n_mat else None, ptr(self.desc), ptr(self.texels))


class _RasterRGBD:
    """Workspace and arguments of the RGB-D render of one camera, reused over the calls."""

    def __init__(self, sim: "MeshSimHIP", cam: _lib.NarutoCullCam, chunk: int):
        self.sim, self.cam = sim, cam
        n_v, n_f = len(sim.v), len(sim.f)
        self.chunk = max(1, min(int(chunk), (2 ** 28 - 1) // max(n_f, 1), (2 ** 32 - 1) // (cam.H * cam.W), 65535))
        self.ws = _lib.workspace(_lib.load().naruto_render_rgbd_workspace(n_v, n_f, self.chunk, cam.H, cam.W), sim.device, torch.int64)
        if self.ws.numel() == 0:
            raise ValueError(f"simulator: a mesh of {n_v} vertices and {n_f} faces at {cam.W} x {cam.H} is beyond the render's sizes")

    def render(self, poses: torch.Tensor, depth=None, color=None, face_id=None, keep_inf: bool = False) -> None:
        """poses [B,4,4] float32 on the device, B <= chunk -> depth [B,H,W], color [B,H,W,3], face_id [B,H,W] (each optional)."""
        s = self.sim
        ptr = lambda t: t.data_ptr() if t is not None else None                                                   # noqa: E731
        if s.tex is not None:
            check(_lib.load().naruto_render_rgbd_tex(C.byref(self.cam), len(s.v), s.v.data_ptr(), len(s.f), s.f.data_ptr(), s.col.data_ptr(), int(s.col_f32), len(poses),
                                                     poses.data_ptr(), s.threshold, _lib.SIM_KEEP_INF if keep_inf else 0, self.ws.data_ptr(), ptr(depth), ptr(color),
                                                     ptr(face_id), C.byref(s.tex.struct), CU._stream()), "naruto_render_rgbd_tex")
            return
        check(_lib.load().naruto_render_rgbd(C.byref(self.cam), len(s.v), s.v.data_ptr(), len(s.f), s.f.data_ptr(), s.col.data_ptr(), int(s.col_f32), len(poses),
                                             poses.data_ptr(), s.threshold, _lib.SIM_KEEP_INF if keep_inf else 0, self.ws.data_ptr(), ptr(depth), ptr(color), ptr(face_id),
                                             CU._stream()), "naruto_render_rgbd")

    def render_depth(self, poses: torch.Tensor, depth: torch.Tensor) -> None:
        """The culling's depth-only render (32-bit cells, +inf where nothing is hit) in the same workspace: the same depth bits."""
        s = self.sim
        check(_lib.load().naruto_render_depth(C.byref(self.cam), len(s.v), s.v.data_ptr(), len(s.f), s.f.data_ptr(), None, len(poses), poses.data_ptr(), s.threshold,
                                              self.ws.data_ptr(), depth.data_ptr(), CU._stream()), "naruto_render_depth")


class MeshSimHIP:
    """``HabitatSim`` over a mesh (module docstring).  ``mesh``: a :class:`naruto_amd.mesh.Mesh` or ``TexturedMesh``, the path of a ``.ply``, ``.glb`` or ``.gltf``
    (``mesh_frame``: ``naruto_amd.gltf.load_gltf``'s ``frame``) or a tuple (vertices, faces[, colors]) with colours RGBA8 [V,4] or float [V,3]; uploaded once.  ``cam``: H, W, fx, fy, cx, cy of the pinhole
    sensor (``config["cam"]``).  ``erp_hw``, ``face_w``: the panorama and the cube faces it is gathered from.  ``plan``: a
    :class:`naruto_amd.culling.RasterPlan`; no bit of any result depends on it."""

    def __init__(self, mesh, cam: Dict, erp_hw: Tuple[int, int] = (1024, 2048), face_w: int = 512, near: float = 0.01, far: float = 100.0, device=None, plan=None, mesh_frame: str = "gltf"):
        self.cam_dict = dict(cam)
        self.cam = CU._camera(cam, near, far)
        self.h, self.w = (int(x) for x in erp_hw)
        self.face_w = int(face_w)
        table = cube_table(self.face_w, self.h, self.w)                                     # (validates face_w, h, w)
        k = (self.face_w - 1) / 2.0
        self.cube_cam = CU._camera({"H": self.face_w, "W": self.face_w, "fx": k, "fy": k, "cx": k, "cy": k}, near, far)
        self.threshold = CU._threshold(plan)
        if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
            from .mesh import Mesh
            mesh = Mesh.load(mesh, mesh_frame)
        vertices, faces, colors, _ = CU._as_mesh(mesh)
        col, self.col_f32 = _colors(colors, torch.as_tensor(vertices).numel() // 3)
        v, self.f = CU._geometry(vertices, faces, device)
        if not bool(torch.isfinite(v).all()):
            raise ValueError("simulator: non-finite vertex")
        self.device = v.device
        self.v = v.to(torch.float32)
        self.col = col.to(self.device).contiguous()
        # materials: only a mesh that has a face with one takes the textured shade; any other goes through the launches it always did
        fm = getattr(mesh, "face_material", None)
        self.tex = _Textures(mesh, len(self.v), len(self.f), self.device) if fm is not None and len(fm) and int(np.asarray(fm).max()) >= 0 else None
        self.table = torch.from_numpy(table).to(self.device).reshape(-1).contiguous()
        self.face_rot = torch.from_numpy(face_rotations()).to(torch.float32)                # (host: face poses are made before the upload)
        self._rasters: Dict[Tuple[str, int], _RasterRGBD] = {}

    # ---- plumbing ----------------------------------------------------------------------------------------------------
    def _raster(self, kind: str, chunk: int) -> _RasterRGBD:
        key = (kind, int(chunk))
        if key not in self._rasters:
            self._rasters[key] = _RasterRGBD(self, self.cam if kind == "pinhole" else self.cube_cam, chunk)
        return self._rasters[key]

    def _cube_poses(self, p: torch.Tensor) -> torch.Tensor:
        """host [P,4,4] -> host [P*6,4,4]: c2w @ R_face, the translation kept."""
        out = p[:, None].repeat(1, 6, 1, 1)
        out[:, :, :3, :3] = p[:, None, :3, :3] @ self.face_rot[None]
        return out.reshape(-1, 4, 4).contiguous()

    def _erp(self, p: torch.Tensor, pano_chunk: int, want_images: bool, invalid_thre: float):
        """-> (erp_color [P,h,w,3] or None, erp_dist [P,h,w] or None, stats uint32-as-int32 [P,2]); no host synchronisation."""
        n, s, dev = len(p), self.face_w, self.device
        r = self._raster("cube", 6 * max(1, int(pano_chunk)))
        per = max(1, r.chunk // 6)
        if r.chunk < 6:
            raise ValueError("simulator: the mesh is too large for six cube faces per launch")
        poses = self._cube_poses(p).to(dev)
        stats = torch.empty(n, 2, dtype=torch.int32, device=dev)
        dist = torch.empty(n, self.h, self.w, dtype=torch.float32, device=dev) if want_images else None
        color = torch.empty(n, self.h, self.w, 3, dtype=torch.float32, device=dev) if want_images else None
        cube_d = torch.empty(per * 6, s, s, dtype=torch.float32, device=dev)
        cube_c = torch.empty(per * 6, s, s, 3, dtype=torch.float32, device=dev) if want_images else None
        lib = _lib.load()
        for a in range(0, n, per):                                                          # (no host synchronisation in here)
            b = min(a + per, n)
            part = poses[6 * a:6 * b]
            if want_images:
                r.render(part, depth=cube_d[:len(part)], color=cube_c[:len(part)])
            else:
                r.render_depth(part, cube_d[:len(part)])
            check(lib.naruto_sim_erp(b - a, s, self.h * self.w, self.table.data_ptr(), cube_d.data_ptr(), cube_c.data_ptr() if want_images else None, float(invalid_thre),
                                     dist[a:b].data_ptr() if want_images else None, color[a:b].data_ptr() if want_images else None, stats[a:b].data_ptr(), CU._stream()),
                  "naruto_sim_erp")
        return color, dist, stats

    # ---- the simulator's surface -------------------------------------------------------------------------------------
    def simulate_batch(self, c2ws, return_erp: bool = False, pose_chunk: int = 8, return_face_id: bool = False):
        """(color [P,H,W,3], depth [P,H,W]) float32 on the device [+ (erp_color [P,h,w,3], erp_depth [P,h,w])] [+ face_id int32 [P,H,W]];
        the loop over the pose chunks has no host synchronisation.  No bit depends on ``pose_chunk``."""
        p = CU._poses(c2ws)
        if int(pose_chunk) < 1:
            raise ValueError("simulator: pose_chunk >= 1")
        with torch.cuda.device(self.device):
            r = self._raster("pinhole", pose_chunk)
            pd = p.to(self.device)
            H, W = self.cam.H, self.cam.W
            depth = torch.empty(len(p), H, W, dtype=torch.float32, device=self.device)
            color = torch.empty(len(p), H, W, 3, dtype=torch.float32, device=self.device)
            fid = torch.empty(len(p), H, W, dtype=torch.int32, device=self.device) if return_face_id else None
            for a in range(0, len(p), r.chunk):
                b = a + r.chunk
                r.render(pd[a:b], depth[a:b], color[a:b], fid[a:b] if fid is not None else None)
            out = (color, depth)
            if return_erp:
                ec, ed, _ = self._erp(p, max(1, int(pose_chunk) // 6), True, 1e6)
                out += (ec, ed)
            if return_face_id:
                out += (fid,)
        return out

    def simulate(self, c2w, return_erp: bool = False, no_print: bool = False):
        """``HabitatSim.simulate``: (color [H,W,3] in 0..1, depth [H,W]) or, with ``return_erp``, (color, depth, erp_color [h,w,3],
        erp_depth [h,w] -- the radial distance map), float32 tensors on the device."""
        p = CU._poses(c2w)
        if len(p) != 1:
            raise ValueError("simulator: simulate takes one [4,4] pose (simulate_batch takes [P,4,4])")
        if not no_print:
            print(f"MeshSimHIP: simulating at position [{float(p[0, 0, 3]):.3f}, {float(p[0, 1, 3]):.3f}, {float(p[0, 2, 3]):.3f}]")
        return tuple(x[0] for x in self.simulate_batch(p, return_erp=return_erp, pose_chunk=1))

    def collision_probe(self, c2w, invalid_thre: float = 1e6) -> Tuple[float, float]:
        """(dist_closest, invalid_region_ratio) of detect_collision_v2 (naruto_planner.py:544-547) at the pose: the minimum of the
        ERP distance map and the share of its pixels above ``invalid_thre``, reduced on the device (depth-only cube faces, no images);
        two scalars come to the host."""
        p = CU._poses(c2w)
        if len(p) != 1:
            raise ValueError("simulator: collision_probe takes one [4,4] pose")
        if math.isnan(float(invalid_thre)):
            raise ValueError("simulator: the threshold is not a number")
        with torch.cuda.device(self.device):
            _, _, stats = self._erp(p, 1, False, invalid_thre)
            bits, count = (int(x) for x in stats[0].cpu())
        return float(np.array([bits], dtype=np.int32).view(np.float32)[0]), count / (self.h * self.w)

"""Reconstruction metrics on the device: Accuracy (cm), Completion (cm), Completion ratio (% < 5 cm) and MAD (cm).

The reference's protocol (its README, "Evaluation"; scripts/evaluation/eval_replica.sh:56-83) reports these four through
src/evaluation/eval_recon.py and src/evaluation/eval_mad.py.  The first three come from third-party code that is not part of the
reference tree (``neural_slam_eval``'s ``calc_3d_mesh_metric`` on top of ``trimesh`` and scipy), so they are PARITY UNPINNED here, as
tracking and the BA pose optimiser are.  This is the contract, restated from the published algorithms, not from that code:

  * 200 000 surface samples per mesh, area weighted: a face is drawn with probability area / total area by a left-sided
    ``searchsorted`` of u0 * total in the cumulative face areas; the point is v0 + e1*u1 + e2*u2 with (u1, u2) uniform and replaced by
    (|u1 - 1|, |u2 - 1|) when u1 + u2 > 1 (trimesh.sample.sample_surface's rule).  A zero-area face is never drawn, except as
    searchsorted's boundary case: it LEADS the face list and u0 is exactly 0.
  * nearest neighbour each way (scipy.spatial.cKDTree.query, Euclidean, k = 1);
  * ``accuracy_cm`` = mean distance rec -> gt x 100, ``completion_cm`` = mean distance gt -> rec x 100, ``completion_ratio_pct`` =
    share of the gt -> rec distances below ``threshold`` (0.05 m) x 100.  Coordinates are metres.

What differs from that code: the random stream (trimesh draws from numpy's global generator; here it is the library's keyed
splitmix64 stream: seed for the ground truth, seed + 1 for the reconstruction, so a run is reproducible bit for bit), and where it runs
(csrc/naruto_recon.hip: nothing but a handful of scalars reaches the host).  What IS pinned: the nearest-neighbour distances equal
``cKDTree.query``'s in every bit (tests/test_gpu_recon.py); among equidistant targets the lowest original index is returned.

``mad_cm`` (evaluate_field only) follows eval_mad.py:84-90 through predict_sdf / query_point_sdf (coslam_utils.py:35-56): the mean
|predicted sdf| at ground-truth surface points, normalised into the bounding box as query_point_sdf does.  The network's sdf is in
units of the truncation distance, so the metric value is mean * training.trunc * 100; the reference hard-codes ``* 10`` there, which is
the same number for its trunc of 0.1 m and a quirk for any other (tests/accuracy_study.py uses the same conversion).

Mesh culling, the step the protocol runs before these metrics (cull_mesh.py --remove_occlusion from the estimated poses), is
``naruto_amd.culling``; ``evaluate_field(cull_poses=..., cull_cam=...)`` runs it on the device between extraction and sampling
(``max_edge=...``: with the tool's subdivision before it, ``naruto_amd.remesh``).

Mesh alignment, the protocol's other step before the metrics (eval_recon.py:80-85: ``get_align_transformation(rec_mesh, gt_mesh)``, applied
to the reconstruction), is ``icp`` / ``get_align_transformation`` here and ``align=True`` on the three metric entry points.  A tracked run's
mesh lives in the frame of the ESTIMATED trajectory; without the alignment Accuracy and Completion mix reconstruction error with drift
(the trajectory gets the same treatment before its error is reported: ``ate``).  ``get_align_transformation`` is neural_slam_eval's too,
so this is PARITY UNPINNED as well; the contract follows the published algorithm (Open3D's ``registration_icp``, point-to-point, defaults):

  * source = the reconstructed mesh's VERTICES, target = the ground-truth mesh's VERTICES; the initial transformation is the identity;
  * ``max_correspondence_distance`` 0.1 m; ``max_iteration`` 30; ``relative_fitness`` = ``relative_rmse`` = 1e-6;
  * a source point is an inlier iff its nearest target is at distance <= max_correspondence_distance (the fp64 distance of the query
    above; ties go to the lowest original index); ``fitness`` = inliers / source points, ``inlier_rmse`` = sqrt(mean squared inlier
    distance), 0 without inliers;
  * point-to-point estimation, no scale: Kabsch with the determinant correction, ``ate``'s formula, on the inlier pairs (transformed
    source point, its target);
  * the loop: evaluate the correspondences at T; then up to max_iteration times: dT from the current inlier pairs, T = dT @ T,
    re-evaluate, and stop as ``converged`` when |fitness - previous| < relative_fitness and |rmse - previous| < relative_rmse;
  * it stops early, unconverged, with T unchanged and status ``degenerate``, when there are fewer than 3 inliers or the second singular
    value of the cross-covariance is <= 1e-10 x the first (collinear pairs: the rotation is not determined);
  * every evaluation transforms the ORIGINAL source points by the cumulative fp64 T and rounds once to float32, in the order
    ((r0*x + r1*y) + r2*z) + t with products and sums rounded (no contraction): tests/icp_spec.py makes the same bits in numpy, and
    nothing drifts across iterations.

It runs in csrc/naruto_icp.hip (transform, 17 fp64 sums in a fixed order, a one-thread Kabsch / convergence step) around the query above;
per iteration the host reads eight doubles to learn whether to go on.

Command line, with the arguments of the reference's eval_recon.py::

    python -m naruto_amd.evaluation --rec_mesh A.ply --gt_mesh B.ply --result_txt out.txt [--icp_align]

``--icp_align`` is the reference's ``--align`` step; ``--align`` itself still raises NotImplementedError (its behaviour is pinned).
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from . import mesh as M

DEFAULT_RING_BUDGET = 4          # rings R = 0 .. 3: a nearest neighbour closer than three cell edges closes in the grid
SCAN_BELOW = 4096                # nearest_distances(method="auto"): targets this small are scanned without a grid


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device(device=None) -> torch.device:
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _mesh_tensors(mesh, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Mesh | (vertices, faces) | path -> (vertices float32 or float64 [V,3], faces int32 [F,3]), contiguous on the device."""
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
        mesh = M.Mesh.load(mesh)
    if isinstance(mesh, M.Mesh):
        mesh = (mesh.vertices, mesh.faces)
    v, f = mesh
    if isinstance(v, torch.Tensor) and v.is_cuda and device is None:
        device = v.device
    device = _device(device)
    v = torch.as_tensor(v)
    f = torch.as_tensor(f)
    if v.dtype not in (torch.float32, torch.float64):
        v = v.to(torch.float64)
    v = v.to(device).reshape(-1, 3).contiguous()
    f = f.to(device).reshape(-1, 3).to(torch.int32).contiguous()
    return v, f


def face_areas(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """float64 [F] triangle areas on the device (naruto_surface_areas: the operation order is part of the ABI)."""
    v, f = _mesh_tensors((vertices, faces))
    if len(f) == 0:
        raise ValueError("face_areas: a mesh without faces")
    areas = torch.empty(len(f), dtype=torch.float64, device=v.device)
    with torch.cuda.device(v.device):
        check(_lib.load().naruto_surface_areas(len(f), len(v), v.data_ptr(), int(v.dtype == torch.float64), f.data_ptr(), areas.data_ptr(), _stream()),
              "naruto_surface_areas")
    return areas


def sample_surface(vertices, faces, count: int, seed: int = 0, cumulative: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``count`` area-weighted surface samples -> (points float32 [count,3], face_index int32 [count]) on the device.
    ``cumulative`` (float64 [F], optional) replaces the cumulative face areas the function would form with ``torch.cumsum``."""
    v, f = _mesh_tensors((vertices, faces))
    if len(f) == 0:
        raise ValueError("sample_surface: a mesh without faces has no surface to sample")
    if cumulative is None:
        cumulative = torch.cumsum(face_areas(v, f), 0)
    cum = cumulative.to(device=v.device, dtype=torch.float64).contiguous()
    if cum.shape != (len(f),):
        raise ValueError("sample_surface: one cumulative area per face")
    # face indices live on the device: one three-number copy checks them and the total area before anything is read through them
    lo, hi, total = (float(x) for x in torch.stack([f.min().double(), f.max().double(), cum[-1]]).cpu())
    if lo < 0 or hi >= len(v):
        raise ValueError(f"sample_surface: face index out of range ({int(lo)} .. {int(hi)} for {len(v)} vertices)")
    if not (math.isfinite(total) and total > 0.0):
        raise ValueError(f"sample_surface: total surface area {total}")
    points = torch.empty(count, 3, dtype=torch.float32, device=v.device)
    face_index = torch.empty(count, dtype=torch.int32, device=v.device)
    with torch.cuda.device(v.device):
        check(_lib.load().naruto_surface_sample(len(f), len(v), v.data_ptr(), int(v.dtype == torch.float64), f.data_ptr(), cum.data_ptr(), int(count),
                                                int(seed) & (2 ** 64 - 1), points.data_ptr(), face_index.data_ptr(), _stream()), "naruto_surface_sample")
    return points, face_index


def _cloud(points, device=None) -> torch.Tensor:
    p = torch.as_tensor(points)
    if p.is_cuda and device is None:
        device = p.device
    return p.to(device=_device(device), dtype=torch.float32).reshape(-1, 3).contiguous()


class PointGridHIP:
    """A target cloud binned once into a uniform grid (counting sort by cell), queried any number of times.

    ``cell``: the cell edge; None derives it from the cloud (naruto_nn_grid_plan: 2 * sqrt(bounding-box surface / points)).  ``max_cells``
    caps the grid (default 2^21 cells); a finer request has its cell enlarged.  ``query`` returns (dist float64 [N], index int32 [N])."""

    def __init__(self, points, cell: Optional[float] = None, max_cells: Optional[int] = None, ring_budget: int = DEFAULT_RING_BUDGET, sort_queries: bool = True):
        self.target = _cloud(points)
        n = len(self.target)
        if n == 0:
            raise ValueError("PointGridHIP: an empty target cloud")
        self.device = self.target.device
        self.ring_budget, self.sort_queries = int(ring_budget), bool(sort_queries)
        box = torch.stack([self.target.amin(0), self.target.amax(0)]).cpu().double().numpy()                # six numbers
        if not np.isfinite(box).all():
            raise ValueError("PointGridHIP: non-finite coordinates in the target cloud")
        self.box = box                       # float64 [2,3]: the cloud's lower and upper corner
        lib = _lib.load()
        self.grid = _lib.NarutoNnGrid()
        check(lib.naruto_nn_grid_plan(n, (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]), 0.0 if cell is None else float(cell), int(max_cells or 0),
                                      C.byref(self.grid)), "naruto_nn_grid_plan")
        self.cell, self.dims = float(self.grid.cell), tuple(self.grid.dims)
        self._start, self._sorted = self._bin(self.grid, self.target)
        self.last_fallback = None            # device uint32 [1 + N] of the last grid query: [0] = queries served by the scan

    def _bin(self, grid: "_lib.NarutoNnGrid", cloud: torch.Tensor):
        lib = _lib.load()
        cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
        start = torch.empty(cells + 1, dtype=torch.int32, device=self.device)
        pts = torch.empty(len(cloud), 4, dtype=torch.float32, device=self.device)
        grid.cell_start, grid.points = start.data_ptr(), pts.data_ptr()
        ws = _lib.workspace(lib.naruto_nn_grid_workspace(C.byref(grid)), self.device, torch.int64)
        with torch.cuda.device(self.device):
            check(lib.naruto_nn_grid_build(C.byref(grid), cloud.data_ptr(), ws.data_ptr(), _stream()), "naruto_nn_grid_build")
        return start, pts

    def query(self, q, method: str = "grid", ring_budget: Optional[int] = None, sort_queries: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        if method not in ("grid", "scan"):
            raise ValueError(f"PointGridHIP.query: method {method!r} (grid or scan)")
        q = _cloud(q, self.device)
        n = len(q)
        dist = torch.empty(n, dtype=torch.float64, device=self.device)
        index = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return dist, index
        lib = _lib.load()
        with torch.cuda.device(self.device):
            if method == "scan":
                check(lib.naruto_nn_scan(len(self.target), self.target.data_ptr(), n, q.data_ptr(), dist.data_ptr(), index.data_ptr(), _stream()), "naruto_nn_scan")
                return dist, index
            budget = self.ring_budget if ring_budget is None else int(ring_budget)
            if budget < 1:
                raise ValueError("PointGridHIP.query: the ring budget is at least 1")
            q_sorted = None
            if self.sort_queries if sort_queries is None else sort_queries:
                # the queries in the TARGET grid's cell order (cells clamped for queries outside the box): a wave's 64 queries read the same few cells
                qg = _lib.NarutoNnGrid()
                qg.n_points, qg.dims, qg.lo, qg.cell = n, self.grid.dims, self.grid.lo, self.grid.cell
                _, q_sorted = self._bin(qg, q)
            fallback = torch.empty(1 + n, dtype=torch.int32, device=self.device)
            check(lib.naruto_nn_grid_query(C.byref(self.grid), n, q.data_ptr(), q_sorted.data_ptr() if q_sorted is not None else None, budget,
                                           dist.data_ptr(), index.data_ptr(), fallback.data_ptr(), _stream()), "naruto_nn_grid_query")
            self.last_fallback = fallback
        return dist, index


def nearest_distances(query, target, method: str = "auto", cell: Optional[float] = None, **grid_args) -> Tuple[torch.Tensor, torch.Tensor]:
    """One-shot nearest neighbour: (dist float64 [N], index int32 [N]) of every query point in ``target``.  ``auto`` scans targets of up to
    4096 points and bins larger ones."""
    target = _cloud(target)
    if method == "auto":
        method = "scan" if len(target) <= SCAN_BELOW else "grid"
    if method == "scan":
        if len(target) == 0:
            raise ValueError("nearest_distances: an empty target cloud")
        q = _cloud(query, target.device)
        dist = torch.empty(len(q), dtype=torch.float64, device=target.device)
        index = torch.empty(len(q), dtype=torch.int32, device=target.device)
        if len(q):
            with torch.cuda.device(target.device):
                check(_lib.load().naruto_nn_scan(len(target), target.data_ptr(), len(q), q.data_ptr(), dist.data_ptr(), index.data_ptr(), _stream()), "naruto_nn_scan")
        return dist, index
    return PointGridHIP(target, cell=cell, **grid_args).query(query, method=method)


def reduce_distances(dist: torch.Tensor, threshold: float) -> torch.Tensor:
    """device float64 [2]: mean of ``dist``, number of entries below ``threshold`` -- fixed summation order, bitwise reproducible."""
    d = dist.to(torch.float64).contiguous()
    if len(d) == 0:
        raise ValueError("reduce_distances: no distances")
    lib = _lib.load()
    ws = _lib.workspace(lib.naruto_dist_reduce_workspace(len(d)), d.device, torch.int64)
    out = torch.empty(2, dtype=torch.float64, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.naruto_dist_reduce(len(d), d.data_ptr(), float(threshold), ws.data_ptr(), out.data_ptr(), _stream()), "naruto_dist_reduce")
    return out


@dataclass
class IcpResult:
    """``transformation``: float64 [4,4] taking source coordinates to target coordinates; ``fitness`` / ``inlier_rmse``: of the last
    evaluation (the one at ``transformation``); ``iterations``: updates applied; ``status``: converged | max_iteration | degenerate;
    ``history``: (fitness, inlier_rmse) of every evaluation, the one at the initial transformation first."""
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    iterations: int
    converged: bool
    status: str
    history: List[Tuple[float, float]]


def transform_points(points: torch.Tensor, transformation) -> torch.Tensor:
    """``points`` (device float32 or float64 [N,3]) moved by ``transformation`` ([4,4], or a device float64 tensor of >= 16 elements) in
    fp64, the points' own dtype out (naruto_icp_transform: the operation order is part of the ABI)."""
    if points.dtype not in (torch.float32, torch.float64):
        raise ValueError("transform_points: float32 or float64 points")
    p = points.reshape(-1, 3).contiguous()
    if isinstance(transformation, torch.Tensor) and transformation.is_cuda:
        T = transformation.to(torch.float64).contiguous()
    else:
        T = torch.from_numpy(np.ascontiguousarray(np.asarray(transformation, dtype=np.float64).reshape(16))).to(p.device)
    if T.numel() < 16:
        raise ValueError("transform_points: a [4,4] transformation")
    out = torch.empty_like(p)
    if len(p):
        with torch.cuda.device(p.device):
            check(_lib.load().naruto_icp_transform(len(p), p.data_ptr(), int(p.dtype == torch.float64), T.data_ptr(), out.data_ptr(), _stream()), "naruto_icp_transform")
    return out


def icp(source, target, max_correspondence_distance: float = 0.1, max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
        init=None) -> IcpResult:
    """Point-to-point ICP of the cloud ``source`` ([N,3]) onto ``target`` ([M,3], or a ready ``PointGridHIP``): the module docstring's
    contract.  The target is binned once; per iteration the device runs transform -> nearest neighbour -> 17 sums -> Kabsch and the
    convergence test, and the host reads eight doubles.  ``init``: the initial [4,4] (identity)."""
    grid = target if isinstance(target, PointGridHIP) else PointGridHIP(target)
    src = _cloud(source, grid.device)
    n = len(src)
    if n == 0:
        raise ValueError("icp: an empty source cloud")
    if not (max_correspondence_distance >= 0.0):
        raise ValueError(f"icp: max_correspondence_distance {max_correspondence_distance}")
    if int(max_iteration) < 0 or math.isnan(relative_fitness) or math.isnan(relative_rmse):
        raise ValueError("icp: max_iteration >= 0 and numbers for the convergence criteria")
    host = np.zeros(_lib.ICP_STATE_DOUBLES, dtype=np.float64)
    host[:16] = (np.eye(4) if init is None else np.asarray(init, dtype=np.float64)).reshape(16)
    if not np.isfinite(host).all():
        raise ValueError("icp: a non-finite initial transformation")
    lib = _lib.load()
    dev = grid.device
    state = torch.from_numpy(host).to(dev)
    origin = (C.c_double * 3)(*(0.5 * (grid.box[0] + grid.box[1])))
    moved = torch.empty_like(src)
    sums = torch.empty(_lib.ICP_SUMS, dtype=torch.float64, device=dev)
    ws = _lib.workspace(lib.naruto_icp_accumulate_workspace(n), dev, torch.float64)
    history: List[Tuple[float, float]] = []
    with torch.cuda.device(dev):
        for _ in range(int(max_iteration) + 1):
            check(lib.naruto_icp_transform(n, src.data_ptr(), 0, state.data_ptr(), moved.data_ptr(), _stream()), "naruto_icp_transform")
            dist, index = grid.query(moved)
            check(lib.naruto_icp_accumulate(n, moved.data_ptr(), len(grid.target), grid.target.data_ptr(), index.data_ptr(), dist.data_ptr(),
                                            float(max_correspondence_distance), origin, ws.data_ptr(), sums.data_ptr(), _stream()), "naruto_icp_accumulate")
            check(lib.naruto_icp_step(sums.data_ptr(), n, origin, int(max_iteration), float(relative_fitness), float(relative_rmse), state.data_ptr(), _stream()),
                  "naruto_icp_step")
            row = state[16:24].cpu().numpy()                     # the one read of the iteration: fitness, rmse, previous two, iteration, status, ...
            history.append((float(row[0]), float(row[1])))
            if int(row[5]) != _lib.ICP_RUNNING:
                break
    final = state.cpu().numpy()
    status = int(final[21])
    if status == _lib.ICP_RUNNING:
        raise _lib.NarutoError("icp: the device loop did not stop")
    return IcpResult(final[:16].reshape(4, 4).copy(), float(final[16]), float(final[17]), int(final[20]), status == _lib.ICP_CONVERGED, _lib.ICP_STATUS[status],
                     history)


def _mesh_vertices(mesh):
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
        mesh = M.Mesh.load(mesh)
    return mesh.vertices if isinstance(mesh, M.Mesh) else mesh[0]


def get_align_transformation(rec_mesh, gt_mesh) -> np.ndarray:
    """The reference's name (eval_recon.py:83): the float64 [4,4] that moves ``rec_mesh`` onto ``gt_mesh``, ``icp`` of the vertices with
    the defaults.  Either mesh is a ``.ply`` path, a ``naruto_amd.mesh.Mesh`` or a (vertices, faces) tuple."""
    return icp(_mesh_vertices(rec_mesh), _mesh_vertices(gt_mesh)).transformation


def empty_reconstruction_metrics() -> Dict[str, float]:
    """A reconstruction without faces: nothing to be accurate about, nothing completed."""
    return {"accuracy_cm": float("nan"), "completion_cm": float("inf"), "completion_ratio_pct": 0.0}


def _n_faces(mesh) -> int:
    if isinstance(mesh, M.Mesh):
        return len(mesh.faces)
    if isinstance(mesh, tuple):
        return int(np.prod(tuple(mesh[1].shape))) // 3
    return -1


class ReconEvaluatorHIP:
    """The ground truth sampled and binned ONCE; every ``evaluate_*`` call then costs the reconstruction's side only."""

    def __init__(self, gt_mesh, n_samples: int = 200000, threshold: float = 0.05, seed: int = 0, device=None, **grid_args):
        if isinstance(gt_mesh, (str, bytes)) or hasattr(gt_mesh, "__fspath__"):
            gt_mesh = M.Mesh.load(gt_mesh)
        if _n_faces(gt_mesh) == 0:
            raise ValueError("ReconEvaluatorHIP: the ground-truth mesh has no faces")
        v, f = _mesh_tensors(gt_mesh, device)
        self.n_samples, self.threshold, self.seed = int(n_samples), float(threshold), int(seed)
        self.grid_args = grid_args
        self.device = v.device
        self.gt_points, _ = sample_surface(v, f, self.n_samples, self.seed)
        self.gt_grid = PointGridHIP(self.gt_points, **grid_args)
        self._gt_vertices, self._gt_vertex_grid = v, None       # the alignment target: binned once, at the first align=True

    def align_vertices(self, vertices: torch.Tensor) -> Tuple[torch.Tensor, IcpResult]:
        """The reconstruction's vertices moved onto the ground truth's (``icp`` of vertices onto vertices, the defaults): fp64
        arithmetic, the vertices' own dtype out."""
        if self._gt_vertex_grid is None:
            self._gt_vertex_grid = PointGridHIP(self._gt_vertices, **self.grid_args)
        result = icp(vertices, self._gt_vertex_grid)
        return transform_points(vertices, result.transformation), result

    def _metrics_device(self, vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
        rec_points, _ = sample_surface(vertices, faces, self.n_samples, self.seed + 1)
        d_rec, _ = self.gt_grid.query(rec_points)                                        # rec -> gt
        self.rec_grid = PointGridHIP(rec_points, **self.grid_args)                       # (kept: its last_fallback says what the scan served)
        d_gt, _ = self.rec_grid.query(self.gt_points)                                    # gt -> rec
        acc = reduce_distances(d_rec, self.threshold)
        comp = reduce_distances(d_gt, self.threshold)
        return torch.stack([acc[0] * 100.0, comp[0] * 100.0, comp[1] / float(len(d_gt)) * 100.0])

    def evaluate_mesh(self, vertices, faces=None, align: bool = False) -> Dict[str, float]:
        """``align``: move the reconstruction onto the ground truth first (``icp`` of its vertices onto the ground truth's); the result
        then carries ``align_fitness`` / ``align_inlier_rmse``.  Without it, launches and results are unchanged."""
        mesh = vertices if faces is None else (vertices, faces)
        if _n_faces(mesh) == 0:
            return empty_reconstruction_metrics()
        v, f = _mesh_tensors(mesh, self.device)
        if len(f) == 0:
            return empty_reconstruction_metrics()
        aligned = None
        if align:
            v, aligned = self.align_vertices(v)
        acc, comp, ratio = (float(x) for x in self._metrics_device(v, f).cpu())
        out = {"accuracy_cm": acc, "completion_cm": comp, "completion_ratio_pct": ratio}
        if aligned is not None:
            out["align_fitness"], out["align_inlier_rmse"] = aligned.fitness, aligned.inlier_rmse
        return out

    @torch.no_grad()
    def evaluate_field(self, model, config, bounding_box: torch.Tensor, voxel_size: float, marching_cube_bound=None, cull_poses=None, cull_cam=None,
                       align: bool = False, **cull_args) -> Dict[str, float]:
        """field -> SDF lattice -> marching cubes -> metric vertices (as ``mesh.extract_mesh``) -> samples -> both queries, plus ``mad_cm``;
        no mesh or cloud goes to the host, one copy of four numbers ends the call.  With ``cull_poses`` ([P,4,4], metric frame) and
        ``cull_cam`` (config["cam"]) the extracted mesh is culled on the device first (``culling.cull_mesh``; ``cull_args`` are its keyword
        arguments: ``max_edge=0.015`` subdivides the surface before the cull, as the protocol's tool does; off by default), at the price
        of one more copy of two numbers (two more per generation of subdivision); without them the launches are unchanged.  ``align``: the (culled)
        mesh is moved onto the ground truth by ``icp`` before sampling, as in ``evaluate_mesh``; ``mad_cm`` does not depend on it."""
        vertices, triangles = M.extract_surface(model.query_sdf, config, bounding_box, marching_cube_bound, voxel_size=voxel_size)
        if cull_poses is not None and len(triangles) > 0:
            if cull_cam is None:
                raise ValueError("evaluate_field: cull_poses needs cull_cam (the intrinsics H, W, fx, fy, cx, cy)")
            from . import culling
            vertices, triangles = culling.cull_mesh((vertices, triangles), cull_poses, cull_cam, **cull_args)
        # MAD: the ground-truth samples (metric) into field coordinates (the inverse of extract_mesh's last vertex transform), then into the unit box
        bb = bounding_box.to(self.device)
        pts = (self.gt_points.to(bb.dtype) + config["data"]["translation"]) * config["data"]["sc_factor"]
        pts = (pts - bb[:, 0]) / (bb[:, 1] - bb[:, 0])
        sdf = model.query_sdf(pts[:, None, :]).reshape(-1)
        mad = sdf.to(torch.float64).abs().mean() * (float(config["training"]["trunc"]) * 100.0)
        if len(triangles) == 0:
            out = empty_reconstruction_metrics()
            out["mad_cm"] = float(mad.cpu())
            return out
        aligned = None
        if align:
            v, triangles = _mesh_tensors((vertices, triangles), self.device)
            vertices, aligned = self.align_vertices(v)
        acc, comp, ratio, mad = (float(x) for x in torch.cat([self._metrics_device(vertices, triangles), mad[None]]).cpu())
        out = {"accuracy_cm": acc, "completion_cm": comp, "completion_ratio_pct": ratio, "mad_cm": mad}
        if aligned is not None:
            out["align_fitness"], out["align_inlier_rmse"] = aligned.fitness, aligned.inlier_rmse
        return out


def calc_3d_mesh_metric(mesh_gt, mesh_rec, n_samples: int = 200000, threshold: float = 0.05, seed: int = 0, align: bool = False) -> Dict[str, float]:
    """Accuracy / Completion / Completion ratio of ``mesh_rec`` against ``mesh_gt`` (module docstring).  Either mesh is a
    ``naruto_amd.mesh.Mesh``, a (vertices, faces) tuple of numpy arrays or device tensors, or the path of a ``.ply`` file.  ``align``:
    ``mesh_rec`` is first moved onto ``mesh_gt`` (``ReconEvaluatorHIP.evaluate_mesh``)."""
    load = lambda m: M.Mesh.load(m) if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__") else m      # noqa: E731
    mesh_gt, mesh_rec = load(mesh_gt), load(mesh_rec)
    if _n_faces(mesh_gt) == 0:
        raise ValueError("calc_3d_mesh_metric: the ground-truth mesh has no faces")
    if _n_faces(mesh_rec) == 0:
        return empty_reconstruction_metrics()
    if align:
        return ReconEvaluatorHIP(mesh_gt, n_samples, threshold, seed).evaluate_mesh(mesh_rec, align=True)
    return ReconEvaluatorHIP(mesh_gt, n_samples, threshold, seed).evaluate_mesh(mesh_rec)


def trajectory_length(poses) -> float:
    """The number of the reference's src/evaluation/eval_traj_length.py:64-73 (result key ``traj_len(m)``): the sum over consecutive
    poses of the norm of (P_i^-1 P_{i-1})[:3, 3].  ``poses``: [P,4,4], or the frame id -> [4,4] dict of a checkpoint (visited in
    key order 0, 1, ..., as the reference indexes it).  Evaluated in float64 on the host."""
    if isinstance(poses, dict):
        poses = [poses[k] for k in sorted(poses)]
    if len(poses) == 0:
        return 0.0
    p = torch.stack([torch.as_tensor(q).detach().to("cpu", torch.float64).reshape(4, 4) for q in poses])
    rel = torch.linalg.inv(p[1:]) @ p[:-1]
    return float(torch.linalg.norm(rel[:, :3, 3], dim=-1).sum())


def ate(est, gt) -> Dict[str, float]:
    """Absolute trajectory error of the estimated camera positions against the true ones after the best RIGID alignment (rotation and
    translation, no scale): ``{"ate_rmse_cm", "ate_mean_cm"}``.  ``est`` / ``gt``: [N,4,4] camera-to-world poses (or [N,3] positions),
    N >= 3, in metres.  Parity unpinned -- Co-SLAM's ``pose_evaluation`` is not in the reference tree; the contract: with e_i, g_i the
    positions and their centroids removed, H = sum e_i g_i^T = U S V^T, R = V diag(1, 1, det(V U^T)) U^T (Horn / Kabsch with the
    determinant correction: a rotation, never a reflection), t = mean(g) - R mean(e); the errors are |R e_i + t - g_i|, reported as
    their root mean square and their mean, in centimetres.  fp64 numpy on the host, once per run (as ``trajectory_length``)."""
    def positions(x):
        a = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)
        return a[:, :3, 3] if a.ndim == 3 else a.reshape(-1, 3)
    e, g = positions(est), positions(gt)
    if e.shape != g.shape:
        raise ValueError(f"ate: {e.shape[0]} estimated poses against {g.shape[0]} true ones")
    if e.shape[0] < 3:
        raise ValueError(f"ate: a rigid alignment needs at least 3 poses, got {e.shape[0]}")
    ce, cg = e.mean(0), g.mean(0)
    U, _, Vt = np.linalg.svd((e - ce).T @ (g - cg))
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(Vt.T @ U.T))) or 1.0])
    R = Vt.T @ D @ U.T
    err = np.linalg.norm((e - ce) @ R.T + cg - g, axis=1)
    return {"ate_rmse_cm": float(np.sqrt((err * err).mean()) * 100.0), "ate_mean_cm": float(err.mean() * 100.0)}


def update_results_file(results: Dict[str, float], file_path: str) -> None:
    """``key,value`` lines; keys already in the file are updated in place, new ones appended (general_utils.py:163-188's format)."""
    merged: Dict[str, float] = {}
    try:
        with open(file_path) as fh:
            for line in fh:
                if line.strip():
                    key, value = line.strip().split(",")
                    merged[key] = float(value)
    except FileNotFoundError:
        pass
    merged.update(results)
    with open(file_path, "w") as fh:
        for key, value in merged.items():
            fh.write(f"{key},{value}\n")


def main(argv=None) -> Dict[str, float]:
    import argparse
    parser = argparse.ArgumentParser(prog="python -m naruto_amd.evaluation", description="Arguments to evaluate the reconstruction.")
    parser.add_argument("--rec_mesh", type=str, required=True, help="reconstructed mesh file path (.ply)")
    parser.add_argument("--gt_mesh", type=str, required=True, help="ground truth mesh file path (.ply)")
    parser.add_argument("--align", action="store_true", help="not available: raises NotImplementedError, as it always has here; use --icp_align")
    parser.add_argument("--icp_align", action="store_true",
                        help="align the reconstructed mesh to the ground truth first (point-to-point ICP of the vertices on the device: the reference's --align step)")
    parser.add_argument("--result_txt", type=str, help="result txt")
    args = parser.parse_args(argv)
    if args.align:
        raise NotImplementedError("--align: the reference's get_align_transformation is third-party code outside its tree; --icp_align runs this library's "
                                  "restatement of it (point-to-point ICP of the vertices)")
    for path in (args.rec_mesh, args.gt_mesh):
        if not path.lower().endswith((".ply", ".glb", ".gltf")):
            raise ValueError(f"{path}: only .ply, .glb and .gltf meshes are read (.obj scenes are not)")
    result = calc_3d_mesh_metric(args.gt_mesh, args.rec_mesh, align=True) if args.icp_align else calc_3d_mesh_metric(args.gt_mesh, args.rec_mesh)
    print(result)
    if args.result_txt:
        update_results_file(result, args.result_txt)
    return result


if __name__ == "__main__":
    main()

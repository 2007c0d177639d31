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
``naruto_amd.culling``; ``evaluate_field(cull_poses=..., cull_cam=...)`` runs it on the device between extraction and sampling.  Mesh
alignment stays with the caller.

Command line, with the arguments of the reference's eval_recon.py::

    python -m naruto_amd.evaluation --rec_mesh A.ply --gt_mesh B.ply --result_txt out.txt
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

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
        mesh = M.load_ply(mesh)
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
            gt_mesh = M.load_ply(gt_mesh)
        if _n_faces(gt_mesh) == 0:
            raise ValueError("ReconEvaluatorHIP: the ground-truth mesh has no faces")
        v, f = _mesh_tensors(gt_mesh, device)
        self.n_samples, self.threshold, self.seed = int(n_samples), float(threshold), int(seed)
        self.grid_args = grid_args
        self.device = v.device
        self.gt_points, _ = sample_surface(v, f, self.n_samples, self.seed)
        self.gt_grid = PointGridHIP(self.gt_points, **grid_args)

    def _metrics_device(self, vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
        rec_points, _ = sample_surface(vertices, faces, self.n_samples, self.seed + 1)
        d_rec, _ = self.gt_grid.query(rec_points)                                        # rec -> gt
        self.rec_grid = PointGridHIP(rec_points, **self.grid_args)                       # (kept: its last_fallback says what the scan served)
        d_gt, _ = self.rec_grid.query(self.gt_points)                                    # gt -> rec
        acc = reduce_distances(d_rec, self.threshold)
        comp = reduce_distances(d_gt, self.threshold)
        return torch.stack([acc[0] * 100.0, comp[0] * 100.0, comp[1] / float(len(d_gt)) * 100.0])

    def evaluate_mesh(self, vertices, faces=None) -> Dict[str, float]:
        mesh = vertices if faces is None else (vertices, faces)
        if _n_faces(mesh) == 0:
            return empty_reconstruction_metrics()
        v, f = _mesh_tensors(mesh, self.device)
        if len(f) == 0:
            return empty_reconstruction_metrics()
        acc, comp, ratio = (float(x) for x in self._metrics_device(v, f).cpu())
        return {"accuracy_cm": acc, "completion_cm": comp, "completion_ratio_pct": ratio}

    @torch.no_grad()
    def evaluate_field(self, model, config, bounding_box: torch.Tensor, voxel_size: float, marching_cube_bound=None, cull_poses=None, cull_cam=None,
                       **cull_args) -> Dict[str, float]:
        """field -> SDF lattice -> marching cubes -> metric vertices (as ``mesh.extract_mesh``) -> samples -> both queries, plus ``mad_cm``;
        no mesh or cloud goes to the host, one copy of four numbers ends the call.  With ``cull_poses`` ([P,4,4], metric frame) and
        ``cull_cam`` (config["cam"]) the extracted mesh is culled on the device first (``culling.cull_mesh``; ``cull_args`` are its keyword
        arguments), at the price of one more copy of two numbers; without them the launches are unchanged."""
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
        acc, comp, ratio, mad = (float(x) for x in torch.cat([self._metrics_device(vertices, triangles), mad[None]]).cpu())
        return {"accuracy_cm": acc, "completion_cm": comp, "completion_ratio_pct": ratio, "mad_cm": mad}


def calc_3d_mesh_metric(mesh_gt, mesh_rec, n_samples: int = 200000, threshold: float = 0.05, seed: int = 0) -> Dict[str, float]:
    """Accuracy / Completion / Completion ratio of ``mesh_rec`` against ``mesh_gt`` (module docstring).  Either mesh is a
    ``naruto_amd.mesh.Mesh``, a (vertices, faces) tuple of numpy arrays or device tensors, or the path of a ``.ply`` file."""
    load = lambda m: M.load_ply(m) if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__") else m      # noqa: E731
    mesh_gt, mesh_rec = load(mesh_gt), load(mesh_rec)
    if _n_faces(mesh_gt) == 0:
        raise ValueError("calc_3d_mesh_metric: the ground-truth mesh has no faces")
    if _n_faces(mesh_rec) == 0:
        return empty_reconstruction_metrics()
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
    parser.add_argument("--align", action="store_true", help="Align meshes (not available: raises NotImplementedError)")
    parser.add_argument("--result_txt", type=str, help="result txt")
    args = parser.parse_args(argv)
    if args.align:
        raise NotImplementedError("--align: the reference's get_align_transformation is third-party code outside its tree; align the meshes before calling")
    for path in (args.rec_mesh, args.gt_mesh):
        if not path.lower().endswith(".ply"):
            raise ValueError(f"{path}: only .ply meshes are read (.obj scenes are not)")
    result = calc_3d_mesh_metric(args.gt_mesh, args.rec_mesh)
    print(result)
    if args.result_txt:
        update_results_file(result, args.result_txt)
    return result


if __name__ == "__main__":
    main()

"""The planner's local RRT on the device: a drop-in for the reference's ``RRTNaruto`` (src/planner/rrt_naruto.py, on
src/planner/rrt.py), the ``local_planner_method`` of every shipped config, plus ``is_collision_free`` (rrt.py:77-117), which
the planner also calls on its own (naruto_planner.py:34, :556).

The whole of ``run()`` / ``run_full()`` is one persistent kernel launch (naruto_rrt.hip): the host hears from it only when it is
done, out of random rows or out of room in the tree buffers -- there is no sync per iteration.  The tree lives in device
buffers owned by this object, so a second ``run()`` continues it, as the reference's does.

Random stream: the reference's own.  ``generate_random_point`` (rrt.py:279-297) makes three scalar ``np.random.uniform`` calls
per extension; here the host draws the same numbers as rows ``np.random.uniform(lo3, hi3, size=(n, 3))`` from numpy's global
state, in chunks (small first, growing).  When a chunk is not used up, the saved state is restored and exactly the rows
consumed are drawn again, so after any call ``np.random.get_state()`` is what the reference's loop would have left, and a run
seeded like the reference's makes the reference's tree.  ``points=`` takes an explicit [n,3] array instead.

Differences to the reference:
  * a segment sample outside ``[0, dim-1]`` counts as blocked (the reference raises on ``None > thre``);
  * at a coordinate of exactly ``dim-1`` the upper corner has weight 0 and its index is clamped (the reference indexes out of
    bounds);
  * a direct line of length zero (start within rounding of the goal, where the reference divides by zero) returns "reached"
    with the start as the goal's parent;
  * ``sdf_map`` may be a numpy volume (as the reference passes it) or a device tensor (no host round trip);
  * ``max_iter=None`` with ``maxz=None`` is accepted (no z cap; the reference raises).
Not covered: the plain ``RRT`` class (``local_planner_method == 'RRT'``, off in every shipped config) is not built.
"""

from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _volume(v, device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
    t = t.to(device, torch.float32).contiguous()
    if t.dim() != 3:
        raise ValueError(f"sdf_map must be [X,Y,Z], got shape {tuple(t.shape)}")
    return t


class Node:
    """The reference's Node (rrt.py:120-148) without the per-node device tensor until it is asked for."""

    def __init__(self, x: float, y: float, z: float, device="cpu"):
        self.x, self.y, self.z = x, y, z
        self.parent = None
        self._device = device
        self._xyz_arr = np.asarray([x, y, z])

    def get_xyz(self) -> torch.Tensor:
        return torch.tensor([self.x, self.y, self.z]).reshape(1, 3).to(self._device).float()


def segments_collision_free(pa, pb, sdf_map, step_size: float = 1, collision_thre: float = 0.5, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """``is_collision_free`` for N segments at once: pa, pb [N,3] (numpy or tensors) -> (num_collision_free int32 [N],
    complete_free bool [N]) on the device."""
    lib = _lib.load()
    device = sdf_map.device if isinstance(sdf_map, torch.Tensor) and sdf_map.is_cuda else torch.device(device)
    vol = _volume(sdf_map, device)
    a = torch.as_tensor(np.asarray(pa) if not isinstance(pa, torch.Tensor) else pa).to(device, torch.float64).reshape(-1, 3).contiguous()
    b = torch.as_tensor(np.asarray(pb) if not isinstance(pb, torch.Tensor) else pb).to(device, torch.float64).reshape(-1, 3).contiguous()
    if a.shape != b.shape:
        raise ValueError(f"pa {tuple(a.shape)} and pb {tuple(b.shape)} differ")
    n = a.shape[0]
    cnt = torch.empty(n, dtype=torch.int32, device=device)
    comp = torch.empty(n, dtype=torch.uint8, device=device)
    dims = (C.c_uint32 * 3)(*vol.shape)
    with torch.cuda.device(device):
        check(lib.naruto_segments_free(dims, vol.data_ptr(), n, a.data_ptr(), b.data_ptr(), float(step_size), float(collision_thre),
                                       cnt.data_ptr(), comp.data_ptr(), _stream()), "naruto_segments_free")
    return cnt, comp.bool()


_uploaded = {"key": None, "vol": None, "host": None}


def _cached_volume(sdf_map, device) -> torch.Tensor:
    """The planner calls is_collision_free every step with the numpy volume it holds (naruto_planner.py:556).  The upload is kept and
    reused for as long as the caller passes the SAME array object (same buffer, shape and dtype); the planner gets a fresh array from
    get_map_volumes whenever the map changes.  An array REWRITTEN IN PLACE keeps its identity and would be served from the stale copy:
    pass a device tensor (never cached) or a new array in that case."""
    if not isinstance(sdf_map, np.ndarray):
        return sdf_map
    key = (id(sdf_map), sdf_map.__array_interface__["data"][0], sdf_map.shape, sdf_map.dtype.str, str(device))
    if _uploaded["key"] != key or _uploaded["host"] is not sdf_map:
        _uploaded.update(key=key, vol=_volume(sdf_map, device), host=sdf_map)
    return _uploaded["vol"]


def is_collision_free(pa, pb, sdf_map, step_size: float = 1, collision_thre: float = 0.5) -> Tuple[int, bool]:
    """rrt.py:77-117 -> (num_collision_free, complete_free).  One launch and one read-back per call; a numpy ``sdf_map`` is uploaded
    once per array object (see _cached_volume)."""
    device = sdf_map.device if isinstance(sdf_map, torch.Tensor) and sdf_map.is_cuda else torch.device("cuda")
    cnt, comp = segments_collision_free(np.asarray(pa, dtype=np.float64).reshape(1, 3), np.asarray(pb, dtype=np.float64).reshape(1, 3),
                                        _cached_volume(sdf_map, device), step_size, collision_thre)
    both = torch.stack([cnt[0], comp[0].to(torch.int32)]).cpu().numpy()
    return int(both[0]), bool(both[1])


class RowSource:
    """The rows of one run()/run_full(): chunks of the reference's random stream (numpy's global state), or slices of an explicit
    array.  draw(n) hands out the next n rows; settle(used) says how many of them were consumed: if fewer than drawn, the state
    saved before the draw is restored and exactly `used` rows are drawn again, so numpy's state ends where `taken` calls of
    generate_random_point (three scalar np.random.uniform each, rrt.py:279-297) would have left it."""

    def __init__(self, lo3, hi3, points=None):
        self.lo, self.hi = np.asarray(lo3, dtype=np.float64), np.asarray(hi3, dtype=np.float64)
        self.points = None if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self.taken, self._saved, self._drawn = 0, None, 0

    def draw(self, n: int) -> np.ndarray:
        if self.points is not None:
            rows = self.points[self.taken:self.taken + n]
        else:
            self._saved = np.random.get_state()
            rows = np.random.uniform(self.lo, self.hi, size=(n, 3))
        self._drawn = len(rows)
        return rows

    def settle(self, used: int) -> None:
        if self.points is None and used < self._drawn:
            np.random.set_state(self._saved)
            if used:
                np.random.uniform(self.lo, self.hi, size=(used, 3))
        self.taken += used

    def exhausted(self) -> bool:
        return self.points is not None and self.taken >= len(self.points)


class RRTNarutoHIP:
    chunk_first, chunk_growth, chunk_max = 64, 4, 1 << 16      # rows drawn per launch: small first, growing
    initial_capacity = 4096                                    # nodes; doubled whenever the kernel asks for room

    def __init__(self, bbox: np.ndarray, voxel_size: float, max_iter: int = None, step_size: float = 1., maxz: int = None, z_levels: List = None,
                 step_amplifier: int = 1, collision_thre: float = 0.5, margin: int = 0, device: str = 'cuda', enable_eval: bool = False,
                 enable_direct_line: bool = True, cell_threshold: int = 0):
        """The arguments of RRTNaruto.__init__ (rrt_naruto.py:37-50); ``cell_threshold``: node count from which the nearest-node
        search walks the per-voxel cell lists (0: the library's default; both searches give the same tree)."""
        self.collision_thre, self._device, self.step_amplifier, self.step_size = collision_thre, torch.device(device), step_amplifier, step_size
        self.enable_eval, self.enable_direct_line, self.cell_threshold = enable_eval, enable_direct_line, int(cell_threshold)
        bbox = np.asarray(bbox, dtype=np.float64)
        # Co-SLAM getVoxels: round(extent / voxel_size + 0.0005) + 1 lattice points per axis (rrt.py:230-246)
        vol_shape = tuple(int(round((bbox[a, 1] - bbox[a, 0]) / voxel_size + 0.0005)) + 1 for a in range(3))
        self.vol_shape = vol_shape
        self.max_iter = max_iter if max_iter is not None else int(np.prod(vol_shape))
        self.x_range = [margin, vol_shape[0] - 1 - margin]
        self.y_range = [margin, vol_shape[1] - 1 - margin]
        zmax = vol_shape[2] - 1 - margin
        self.z_range = ([margin, zmax if maxz is None else min(zmax, maxz)]) if z_levels is None else z_levels
        self.full_x_range, self.full_y_range, self.full_z_range = [0, vol_shape[0] - 1], [0, vol_shape[1] - 1], [0, vol_shape[2] - 1]
        self.eval_results = {"time (ms)": [], "node_num": [], "rrt_iter": []}
        self.rrt_iter = 0
        self._plan = None

    # ---- buffers ---------------------------------------------------------------------------------------------------------------
    def _alloc_tree(self, cap: int) -> None:
        dev = self._device
        old = getattr(self, "_tree", None)
        tree = (torch.empty(cap, 3, dtype=torch.float64, device=dev), torch.empty(cap, 3, dtype=torch.float32, device=dev),
                torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev))
        if old is not None:
            n = self._n_nodes
            for new, prev in zip(tree, old):
                new[:n].copy_(prev[:n])
        self._tree, self._cap = tree, cap
        self._path_buf = torch.empty(cap + 1, dtype=torch.int32, device=dev)
        p = self._plan
        p.nodes_xyz, p.nodes_xyz32, p.parent, p.next = (t.data_ptr() for t in tree)
        p.capacity = cap

    def _read_state(self) -> np.ndarray:
        st = self._ws[:_lib.RRT_STATE_INTS].cpu().numpy()           # the one sync per launch
        self._n_nodes = int(st[_lib.RRT_STATE_NODES])
        return st

    def start_new_plan(self, start: np.ndarray, goal: np.ndarray, sdf_map) -> None:
        """rrt.py:248-277.  ``sdf_map``: numpy [X,Y,Z] or a device tensor."""
        lib = _lib.load()
        self.sdf_map = sdf_map
        self._vol = _volume(sdf_map, self._device)
        if tuple(self._vol.shape) != self.vol_shape:
            raise ValueError(f"sdf_map shape {tuple(self._vol.shape)} != planner volume {self.vol_shape}")
        start, goal = np.asarray(start, dtype=np.float64).reshape(3), np.asarray(goal, dtype=np.float64).reshape(3)
        self.start, self.goal = Node(*start, device=self._device), Node(*goal, device=self._device)
        dims = (C.c_uint32 * 3)(*self.vol_shape)
        if self._plan is None:
            p = self._plan = _lib.NarutoRrtPlan()
            p.dims = dims
            for a, (r, f) in enumerate(zip((self.x_range, self.y_range, self.z_range), (self.full_x_range, self.full_y_range, self.full_z_range))):
                p.range[a][0], p.range[a][1] = float(r[0]), float(r[1])
                p.full_range[a][0], p.full_range[a][1] = float(f[0]), float(f[1])
            self._ws = _lib.workspace(lib.naruto_rrt_workspace(dims), self._device, torch.int32)
            p.workspace = self._ws.data_ptr()
            self._n_nodes = 0
            self._alloc_tree(int(self.initial_capacity))
        p = self._plan
        p.step_size, p.step_amplifier, p.collision_thre = float(self.step_size), float(self.step_amplifier), float(self.collision_thre)
        p.enable_direct_line, p.cell_threshold = int(bool(self.enable_direct_line)), self.cell_threshold
        p.sdf_vol = self._vol.data_ptr()
        with torch.cuda.device(self._device):
            check(lib.naruto_rrt_start(C.byref(p), (C.c_double * 3)(*start), (C.c_double * 3)(*goal), _stream()), "naruto_rrt_start")
        self._n_nodes, self.rrt_iter, self._goal_parent = 1, 0, -1

    # ---- growing ---------------------------------------------------------------------------------------------------------------
    def _grow(self, mode: int, points) -> np.ndarray:
        lib = _lib.load()
        full = mode == _lib.RRT_MODE_FULL
        rng = (self.full_x_range, self.full_y_range, self.full_z_range) if full else (self.x_range, self.y_range, self.z_range)
        src = RowSource([r[0] for r in rng], [r[1] for r in rng], points)
        chunk, restart, done_iters = int(self.chunk_first), 1, 0
        while True:
            rows = src.draw(max(1, min(chunk, int(self.chunk_max), self.max_iter - done_iters)))
            rows_dev = torch.from_numpy(rows).to(self._device)
            used = 0
            while True:                                                                   # the same rows again after a stop for room
                with torch.cuda.device(self._device):
                    check(lib.naruto_rrt_grow(C.byref(self._plan), mode, rows_dev[used:].data_ptr() if used < len(rows) else None, len(rows) - used,
                                              int(self.max_iter), restart, _stream()), "naruto_rrt_grow")
                restart = 0
                st = self._read_state()
                used += int(st[_lib.RRT_STATE_ROWS_USED])
                if st[_lib.RRT_STATE_STATUS] != _lib.RRT_NEED_ROOM:
                    break
                self._alloc_tree(2 * self._cap)
            src.settle(used)
            done_iters = int(st[_lib.RRT_STATE_ITER])
            if st[_lib.RRT_STATE_STATUS] == _lib.RRT_DONE:
                return st
            if src.exhausted():
                raise ValueError(f"points ran out after {src.taken} rows ({done_iters} of {self.max_iter} iterations done)")
            chunk = chunk * int(self.chunk_growth)

    def run(self, points=None) -> bool:
        """rrt_naruto.py:189-234 -> target_reachable; sets goal.parent (see find_path)."""
        st = self._grow(_lib.RRT_MODE_RUN, points)
        self.rrt_iter = int(st[_lib.RRT_STATE_RRT_ITER])
        self._goal_parent = int(st[_lib.RRT_STATE_GOAL_PARENT])
        return bool(st[_lib.RRT_STATE_REACHABLE])

    def run_full(self, points=None) -> None:
        """rrt.py:350-355: max_iter random extensions over the full ranges."""
        self._grow(_lib.RRT_MODE_FULL, points)

    # ---- results ---------------------------------------------------------------------------------------------------------------
    def path_indices(self) -> np.ndarray:
        """Node indices goal.parent, ..., start: one launch, one read-back (the walk stops at the tree's node count, so the first
        n_nodes + 1 ints of the path buffer hold the count and every index)."""
        lib = _lib.load()
        with torch.cuda.device(self._device):
            check(lib.naruto_rrt_path(C.byref(self._plan), self._path_buf.data_ptr(), _stream()), "naruto_rrt_path")
        buf = self._path_buf[:self._n_nodes + 1].cpu().numpy()
        return buf[1:1 + int(buf[0])].copy()

    def find_path(self) -> List[Node]:
        """rrt.py:376-387: [goal, ..., start]; only the path is copied back."""
        idx = self.path_indices()
        xyz = self._tree[0][torch.from_numpy(idx).to(self._device).long()].cpu().numpy() if len(idx) else np.zeros((0, 3))
        path = [self.goal]
        self.goal.parent = None
        for row in xyz:
            node = Node(*row, device=self._device)
            path[-1].parent = node
            path.append(node)
        return path

    def get_reachable_mask(self, use_cell_lists: Optional[bool] = None) -> np.ndarray:
        """rrt.py:389-431 -> float32 [X,Y,Z].  ``use_cell_lists``: None = over the cell lists when the plan has them (the start was
        inside the grid), False = node tiles through LDS; both give the same mask."""
        lib = _lib.load()
        mask = torch.empty(self.vol_shape, dtype=torch.float32, device=self._device)
        had = None
        if use_cell_lists is not None:
            had = int(self._ws[_lib.RRT_STATE_USE_CELLS].item())
            if use_cell_lists and not had:
                raise ValueError("this plan has no cell lists: its start lies outside the grid")
            self._ws[_lib.RRT_STATE_USE_CELLS] = int(bool(use_cell_lists))
        with torch.cuda.device(self._device):
            check(lib.naruto_reachable_mask(C.byref(self._plan), mask.data_ptr(), _stream()), "naruto_reachable_mask")
        if had is not None:
            self._ws[_lib.RRT_STATE_USE_CELLS] = had
        return mask.cpu().numpy()

    @property
    def n_nodes(self) -> int:
        return self._n_nodes

    def nodes_xyz(self) -> np.ndarray:
        """float64 [n,3]: every node's _xyz_arr, in the order the reference appends them."""
        return self._tree[0][:self._n_nodes].cpu().numpy()

    def parents(self) -> np.ndarray:
        """int32 [n]: parent index per node, -1 for the start."""
        return self._tree[2][:self._n_nodes].cpu().numpy()

    # ---- evaluation: the bookkeeping the planner's caller drives when enable_eval is set (naruto_planner.py:384-391) ---------------
    def update_eval(self, is_valid_planning: bool, time: float, path: Sequence[Node]) -> None:
        """One more sample of (planning time in ms, tree size, rrt_iter) per SUCCESSFUL planning; ``time`` is in seconds."""
        if is_valid_planning:
            sample = {"time (ms)": 1e3 * time, "node_num": self._n_nodes, "rrt_iter": self.rrt_iter}
            for name, value in sample.items():
                self.eval_results[name].append(value)

    def print_eval_result(self, info_printer) -> None:
        """The mean of every series through the caller's printer: a 20-character label, a colon, two decimals."""
        info_printer("Running RRT Evaluation.")
        means = {name: float(np.mean(series)) if len(series) else float("nan") for name, series in self.eval_results.items()}
        for name, mean in means.items():
            info_printer("%s: %.2f" % (info_printer.adjust_string_length(20, name), mean))

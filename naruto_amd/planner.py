"""The planner: a drop-in for the reference's ``NarutoPlanner`` (src/planner/naruto_planner.py on src/planner/planner.py and
src/planner/rotation_planning.py), the third stage of the step loop (src/naruto/main.py:90-140) after ``MeshSimHIP`` and the mapping.

What runs where:
  * the state machine (``update_state`` :162-229, ``compute_next_state_pose`` :231-294) takes one branch per step and ends in a host
    pose: it is host code, transition for transition the reference's;
  * a planning step (``uncertainty_aware_planning_v2`` :319-401) is device work: the traversability filter is a device multiply, the
    aggregation is ``GoalSpaceAggregatorHIP``, the goal search is ONE launch and one small read-back (``naruto_goal_search``: the
    reference copies the [G] volume to the host, runs ``np.argpartition``, a ``torch.topk``, a gather and a conversion per look-at
    target), the path is ``RRTNarutoHIP``;
  * ``detect_collision_v2`` (:512-594) takes its two scalars from ``sim.collision_probe`` when the simulator has one (``MeshSimHIP``),
    else from ``sim.simulate(..., return_erp=True)`` as written in the reference; the segment test is ``naruto_amd.rrt.is_collision_free``;
  * ``compute_camera_pose`` (planner.py:119-153) and rotation planning (rotation_planning.py:55-192) are fp64 numpy with the quaternion
    arithmetic below -- at most a couple of hundred matrices per plan.  No ``scipy``, no ``mmengine``.

Configuration: keyword arguments or a mapping with the planner keys of configs/default.py:79-123 (``DEFAULTS``), or a whole config
mapping with ``planner`` and ``general.dataset`` entries.

Differences to know about:
  * argmax tie rule: among equal maxima of the aggregated goal volume the LOWEST flat index wins.  The reference's
    ``np.argpartition(a, -1, axis=None)[-1]`` has no rule (which of several equal maxima it returns depends on the array's length);
  * top-k tie rule: equal values in the goal's row are taken in ascending target index (``torch.topk`` leaves the order open);
  * target selection: ``select_targets`` defaults to ``GoalSpaceAggregatorHIP.select_targets`` (the top_k in voxel order, thinned
    evenly) where the reference takes whatever ``np.argpartition`` leaves in the last slots -- see planner_aggregation.py.  Any
    callable ``uncert_volume -> [K,3] voxel indices`` can be given; recorded targets are replayed through it;
  * volumes may be numpy arrays (as the reference passes them) or device tensors, which are used where they are;
    ``traversability_mask`` is a numpy array, as in the reference (``RRTNarutoHIP.get_reachable_mask`` returns one);
  * ``main`` returns the pose as a float32 CPU tensor, as the reference does.
"""

from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check

STATES = ("planning", "rotationPlanningAtStart", "rotatingAtStart", "movingToGoal", "rotationPlanningAtGoal", "rotatingAtGoal", "staying")
DATASETS = ("MP3D", "Replica", "NARUTO")

# configs/default.py:79-123 (rrt_step_size None: step_size / voxel_size, as computed there); collision_thre is the .get() default of
# naruto_planner.py:72
DEFAULTS = dict(
    method="naruto", enable_timing=False, step_size=0.1, voxel_size=0.1,
    uncert_top_k=4000, uncert_top_k_subset=300, gs_sensing_range=(0.5, 2), safe_sdf=0.8, force_uncert_aggre=False, gs_z_levels=None,
    obs_per_goal=10, enable_uncert_filtering=True, up_dir=(0, 0, 1), local_planner_method="RRTNaruto",
    invalid_region_ratio_thre=0.5, collision_dist_thre=0.05, max_rot_deg=10,
    rrt_step_size=None, rrt_step_amplifier=10, rrt_maxz=100, rrt_max_iter=None, rrt_z_levels=None, enable_eval=False, enable_direct_line=True,
    collision_thre=0.05,
)


# ---- rotations: fp64 unit quaternions (x, y, z, w) ----------------------------------------------------------------------------
def quat_from_matrix(m) -> np.ndarray:
    """The matrix need not be exactly orthonormal (poses come back as float32): it is replaced by the nearest orthonormal one, U V^T of
    its singular value decomposition; then Markley's method -- the largest of the diagonal entries and the trace picks the branch --
    and the result is normalised."""
    u, _, vt = np.linalg.svd(np.asarray(m, dtype=np.float64))
    m = u @ vt
    trace = m[0, 0] + m[1, 1] + m[2, 2]
    pick = int(np.argmax([m[0, 0], m[1, 1], m[2, 2], trace]))
    q = np.empty(4)
    if pick == 3:
        q[0], q[1], q[2], q[3] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1.0 + trace
    else:
        i, j, k = pick, (pick + 1) % 3, (pick + 2) % 3
        q[i] = 1.0 - trace + 2.0 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    return q / np.sqrt(q @ q)


def quat_to_matrix(q) -> np.ndarray:
    x, y, z, w = q
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[xx - yy - zz + ww, 2.0 * (xy - zw), 2.0 * (xz + yw)],
                     [2.0 * (xy + zw), -xx + yy - zz + ww, 2.0 * (yz - xw)],
                     [2.0 * (xz - yw), 2.0 * (yz + xw), -xx - yy + zz + ww]])


def quat_mul(p, q) -> np.ndarray:
    """The rotation q followed by p (Hamilton product p q), normalised."""
    r = np.empty(4)
    r[:3] = p[3] * q[:3] + q[3] * p[:3] + np.cross(p[:3], q[:3])
    r[3] = p[3] * q[3] - p[:3] @ q[:3]
    return r / np.sqrt(r @ r)


def quat_inv(q) -> np.ndarray:
    return np.array([-q[0], -q[1], -q[2], q[3]])


def quat_angle(q) -> float:
    """Rotation angle in [0, pi]."""
    return 2.0 * np.arctan2(np.sqrt(q[:3] @ q[:3]), abs(q[3]))


def quat_to_rotvec(q) -> np.ndarray:
    q = -q if q[3] < 0 else q
    angle = 2.0 * np.arctan2(np.sqrt(q[:3] @ q[:3]), q[3])
    if angle <= 1e-3:                                                   # angle / sin(angle / 2), expanded about zero
        scale = 2.0 + angle ** 2 / 12.0 + 7.0 * angle ** 4 / 2880.0
    else:
        scale = angle / np.sin(angle / 2.0)
    return scale * q[:3]


def quat_from_rotvec(v) -> np.ndarray:
    angle = np.sqrt(v @ v)
    if angle <= 1e-3:                                                   # sin(angle / 2) / angle, expanded about zero
        scale = 0.5 - angle ** 2 / 48.0 + angle ** 4 / 3840.0
    else:
        scale = np.sin(angle / 2.0) / angle
    return np.array([scale * v[0], scale * v[1], scale * v[2], np.cos(angle / 2.0)])


def compute_camera_pose(A, B, up_dir=(0, 0, 1)) -> np.ndarray:
    """planner.py:119-153: the RUB rotation [3,3] of a camera at A looking at B; a target straight above or below is nudged by 1e-6
    in x, as there."""
    V = np.asarray(A) - np.asarray(B)                                   # (a new array: the nudge below does not reach the caller's)
    if V[0] == 0 and V[1] == 0:
        V[0] = 1e-6
    R = np.cross(np.asarray(up_dir), V)
    U = np.cross(V, R)
    V = V / np.linalg.norm(V)
    R = R / np.linalg.norm(R)
    U = U / np.linalg.norm(U)
    return np.column_stack((R, U, V))


def order_rotations(start, targets: List[np.ndarray]) -> List[np.ndarray]:
    """rotation_planning.py:74-106: greedy -- from the current rotation always to the nearest remaining one (the first of equals)."""
    ordered, left, cur = [start], list(targets), start
    while left:
        angles = [quat_angle(quat_mul(quat_inv(cur), q)) for q in left]
        cur = left.pop(int(np.argmin(angles)))
        ordered.append(cur)
    return ordered


def interpolate_rotation(q1, q2, step_deg: float) -> List[np.ndarray]:
    """rotation_planning.py:124-157: q1, the slerp at i / n for 0 < i < n = int(total_deg / step_deg), q2."""
    total_deg = quat_angle(quat_mul(quat_inv(q1), q2)) / np.pi * 180
    n = int(total_deg / step_deg)
    rotvec = quat_to_rotvec(quat_mul(quat_inv(q1), q2))
    return [q1] + [quat_mul(q1, quat_from_rotvec(rotvec * (i / n))) for i in range(1, n)] + [q2]


def rotation_planning(R_mat, target_Rs_mat, max_rot_deg: float) -> List[np.ndarray]:
    """rotation_planning.py:160-192 -> the planned rotations [3,3], the current one first, every end point once."""
    ordered = order_rotations(quat_from_matrix(R_mat), [quat_from_matrix(t) for t in target_Rs_mat])
    planned = []
    for i in range(len(ordered) - 1):
        part = interpolate_rotation(ordered[i], ordered[i + 1], max_rot_deg)
        planned += part if i == 0 else part[1:]
    return [quat_to_matrix(q) for q in planned]


# ---- the device goal search ----------------------------------------------------------------------------------------------------
def goal_search(aggregated: torch.Tensor, collections: torch.Tensor, targets: torch.Tensor, goal_idx: torch.Tensor, obs_per_goal: int,
                bbox_min, voxel_size: float, guard: int = 0) -> Dict:
    """``naruto_goal_search`` on device tensors (aggregated fp32 [G], collections fp32 [G,K], targets int32 [K,3], goal_idx int32 [G,3])
    -> {'goal', 'goal_vxl' [3], 'n_lookat', 'lookat_idx' [m], 'lookat_vxl' [m,3], 'lookat_val' [m], 'lookat_loc' fp64 [m,3]} as
    numpy, m = min(obs_per_goal, K), slot r = rank r; the caller keeps the first n_lookat.  One launch, one read-back.
    ``guard``: extra int32 words after the buffer, returned as 'guard' (tests)."""
    lib = _lib.load()
    for name, t, dt in (("aggregated", aggregated, torch.float32), ("collections", collections, torch.float32), ("targets", targets, torch.int32),
                        ("goal_idx", goal_idx, torch.int32)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise ValueError(f"goal_search: {name} must be a contiguous {dt} device tensor")
    G, K = aggregated.numel(), targets.numel() // 3
    if collections.numel() != G * K or goal_idx.numel() != 3 * G:
        raise ValueError(f"goal_search: collections {tuple(collections.shape)} / goal_idx {tuple(goal_idx.shape)} do not fit G = {G}, K = {K}")
    m = max(0, min(int(obs_per_goal), K))
    head = _lib.GOAL_SEARCH_HEAD_INTS
    words = head + 11 * m
    out = torch.full((words + int(guard),), -1, dtype=torch.int32, device=aggregated.device)
    with torch.cuda.device(aggregated.device):
        check(lib.naruto_goal_search(G, K, aggregated.data_ptr(), collections.data_ptr(), targets.data_ptr(), goal_idx.data_ptr(), max(0, int(obs_per_goal)),
                                     (C.c_double * 3)(*(float(b) for b in bbox_min)), float(voxel_size), out.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "naruto_goal_search")
    buf = out.cpu().numpy()                                                                   # the one read-back
    a, b, c = head + 6 * m, head + 7 * m, head + 10 * m
    return {"goal": int(buf[0]), "goal_vxl": buf[1:4].copy(), "n_lookat": int(buf[4]), "lookat_loc": buf[head:a].view(np.float64).reshape(m, 3).copy(),
            "lookat_idx": buf[a:b].copy(), "lookat_vxl": buf[b:c].reshape(m, 3).copy(), "lookat_val": buf[c:words].view(np.float32).copy(),
            "guard": buf[words:].copy()}


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class NarutoPlannerHIP:
    def __init__(self, cfg: Optional[Mapping] = None, info_printer: Optional[Callable] = None, dataset: Optional[str] = None, device="cuda",
                 select_targets: Optional[Callable] = None, **planner_keys):
        """``cfg``: the planner entries (or a whole config with ``planner`` and ``general`` entries); keyword arguments override them.
        ``dataset``: 'Replica', 'MP3D' or 'NARUTO' (``general.dataset``), the rule of detect_collision_v2.  ``select_targets``:
        callable(uncert volume on the device) -> [K,3] voxel indices; None: the aggregator's."""
        cfg = dict(cfg or {})
        if "planner" in cfg:
            if dataset is None and "general" in cfg:
                dataset = cfg["general"]["dataset"]
            cfg = dict(cfg["planner"])
        unknown = set(planner_keys) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"NarutoPlannerHIP: unknown planner keys {sorted(unknown)}")
        self.planner_cfg = _Cfg({**DEFAULTS, **cfg, **planner_keys})
        if self.planner_cfg["rrt_step_size"] is None:
            self.planner_cfg["rrt_step_size"] = self.planner_cfg["step_size"] / self.planner_cfg["voxel_size"]
        self.dataset = "Replica" if dataset is None else dataset
        self.info_printer = info_printer if info_printer is not None else (lambda *a, **k: None)
        self.device = torch.device(device)
        self.select_targets = select_targets
        self.step = 0
        self.state = "staying"
        self.sim = None
        self.path, self.lookat_tgts, self.rots = None, None, []
        self.is_goal_reachable = False
        self.traversability_mask = None
        self.aggregator = self.local_planner = None

    # ---- the base class's surface (planner.py:56-117) ----------------------------------------------------------------------------
    def update_step(self, step: int) -> None:
        self.step = step

    def update_sim(self, sim) -> None:
        self.sim = sim

    def vox2loc(self, vox, bbox=None, voxel_size=None):
        bbox = bbox if bbox is not None else self.bbox
        voxel_size = voxel_size if voxel_size is not None else self.voxel_size
        return vox * voxel_size + bbox[:, 0]

    def loc2vox(self, loc, bbox=None, voxel_size=None):
        bbox = bbox if bbox is not None else self.bbox
        voxel_size = voxel_size if voxel_size is not None else self.voxel_size
        return (loc - bbox[:, 0]) / voxel_size

    def init_data(self, bbox) -> None:
        """naruto_planner.py:91-137; the goal-space lattice is the aggregator's (made on first use of the device)."""
        self.path, self.lookat_tgts = None, None
        self.gs_z_levels = self.planner_cfg.get("gs_z_levels", [5, 11, 17])
        self.voxel_size = self.planner_cfg.voxel_size
        self.bbox = np.asarray(bbox)
        self.Nx, self.Ny, self.Nz = (round((bbox[a][1] - bbox[a][0]) / self.voxel_size + 0.0005) + 1 for a in range(3))
        self.aggregator = None

    def _aggregator(self):
        if self.aggregator is None:
            from .planner_aggregation import GoalSpaceAggregatorHIP
            c = self.planner_cfg
            self.aggregator = GoalSpaceAggregatorHIP(self.bbox, self.voxel_size, c.uncert_top_k, c.uncert_top_k_subset, c.gs_sensing_range, c.safe_sdf,
                                                     self.gs_z_levels, device=self.device)
            for name in ("gs_x_range", "gs_y_range", "gs_z_range", "gs_x", "gs_y", "gs_z", "goal_space_pts"):
                setattr(self, name, getattr(self.aggregator, name))
        return self.aggregator

    def init_local_planner(self) -> None:
        """naruto_planner.py:55-89."""
        c = self.planner_cfg
        if c.local_planner_method != "RRTNaruto":
            raise NotImplementedError(f"local_planner_method {c.local_planner_method!r}: only 'RRTNaruto' is built (see naruto_amd/rrt.py)")
        from .rrt import RRTNarutoHIP
        self.local_planner = RRTNarutoHIP(bbox=self.bbox, voxel_size=self.voxel_size, max_iter=c.get("rrt_max_iter", None), step_size=c.rrt_step_size,
                                          maxz=c.rrt_maxz, z_levels=c.get("rrt_z_levels", None), step_amplifier=c.get("rrt_step_amplifier", 1),
                                          collision_thre=c.get("collision_thre", 0.05) / self.voxel_size, device=str(self.device),
                                          enable_eval=c.get("enable_eval", False), enable_direct_line=c.get("enable_direct_line", True))

    # ---- the state machine (host) -------------------------------------------------------------------------------------------------
    def main(self, uncert_sdf_vols: List, cur_pose: np.ndarray, is_new_vols: bool) -> torch.Tensor:
        """naruto_planner.py:139-160 -> the new camera-to-world pose [4,4], float32."""
        self.update_state(uncert_sdf_vols[1], cur_pose, is_new_vols)
        self.info_printer(f"Current state: {self.state}", self.step, self.__class__.__name__)
        new_pose = self.compute_next_state_pose(cur_pose, uncert_sdf_vols)
        return torch.from_numpy(new_pose).float()

    def update_state(self, sdf_vol, cur_pose: np.ndarray, is_new_vols: bool) -> None:
        """naruto_planner.py:162-229."""
        s = self.state
        if s == "planning":
            self.state = "rotationPlanningAtStart" if self.check_goal_reachable() else "staying"
        elif s == "rotationPlanningAtStart":
            self.state = "rotatingAtStart"
        elif s == "rotatingAtStart":
            self.state = "movingToGoal" if self.check_rotation_done() else "rotatingAtStart"
        elif s == "movingToGoal":
            if self.check_goal_reached():
                self.state = "rotationPlanningAtGoal"
            else:
                next_pt_loc = self.vox2loc(self.path[-1]._xyz_arr)
                collided = self.detect_collision_v2(sdf_vol=sdf_vol, cur_pose=cur_pose, next_pt_loc=next_pt_loc)
                self.state = "staying" if collided else "movingToGoal"
        elif s == "rotationPlanningAtGoal":
            self.state = "rotatingAtGoal"
        elif s == "rotatingAtGoal":
            self.state = "planning" if self.check_rotation_done() else "rotatingAtGoal"
        elif s == "staying":
            self.state = "planning" if self.check_new_map_received(is_new_vols) else "staying"
        # (an unknown state is left as it is, as in the reference; compute_next_state_pose refuses it)

    def compute_next_state_pose(self, cur_pose: np.ndarray, uncert_sdf_vols: List) -> np.ndarray:
        """naruto_planner.py:231-294."""
        s = self.state
        if s == "planning":
            out = self.uncertainty_aware_planning_v2(uncert_sdf_vols, cur_pose)
            self.is_goal_reachable, self.lookat_tgts, self.path = out["is_goal_reachable"], out["lookat_tgts"], out["path"]
            return cur_pose.copy()
        if s == "rotationPlanningAtStart":
            return self.rotation_planning_at_start(cur_pose, self.lookat_tgts[0])
        if s == "rotatingAtStart":
            return self.rotating_at_start(cur_pose)
        if s == "movingToGoal":
            new_pose = self.moving_to_goal(cur_pose, self.lookat_tgts[0], self.path[-1])
            self.path.pop(-1)
            return new_pose
        if s == "rotationPlanningAtGoal":
            return self.rotation_planning_at_goal(cur_pose, self.lookat_tgts)
        if s == "rotatingAtGoal":
            return self.rotating_at_start(cur_pose)                 # (the reference pops through the same routine at the goal)
        if s == "staying":
            return cur_pose.copy()
        raise NotImplementedError(f"planner state {s!r}")

    def check_goal_reachable(self) -> bool:
        return self.is_goal_reachable

    def check_rotation_done(self) -> bool:
        return len(self.rots) == 0

    def check_goal_reached(self) -> bool:
        return len(self.path) == 0

    def check_new_map_received(self, is_new_vols):
        return is_new_vols

    # ---- rotation states (:737-841) -----------------------------------------------------------------------------------------------
    def rotating_at_current_loc(self, cur_pose: np.ndarray) -> np.ndarray:
        new_pose = cur_pose.copy()
        new_pose[:3, :3] = self.rots.pop(0)
        return new_pose

    rotating_at_start = rotating_at_goal = rotating_at_current_loc

    def rotation_planning_at_start(self, cur_pose: np.ndarray, lookat_loc: np.ndarray) -> np.ndarray:
        rot = compute_camera_pose(cur_pose[:3, 3], lookat_loc, up_dir=self.planner_cfg.up_dir)
        self.rots = rotation_planning(cur_pose[:3, :3], [rot], self.planner_cfg.max_rot_deg)
        return cur_pose.copy()

    def rotation_planning_at_goal(self, cur_pose: np.ndarray, lookat_locs) -> np.ndarray:
        rots = [compute_camera_pose(cur_pose[:3, 3], loc, up_dir=self.planner_cfg.up_dir) for loc in lookat_locs]
        self.rots = rotation_planning(cur_pose[:3, :3], rots, self.planner_cfg.max_rot_deg)
        return cur_pose.copy()

    def moving_to_goal(self, cur_pose: np.ndarray, lookat_loc: np.ndarray, next_pt_node) -> np.ndarray:
        next_loc = self.vox2loc(next_pt_node._xyz_arr)
        new_pose = cur_pose.copy()
        new_pose[:3, :3] = compute_camera_pose(next_loc, lookat_loc, up_dir=self.planner_cfg.up_dir)
        new_pose[:3, 3] = next_loc
        return new_pose

    # ---- a planning step (device) -------------------------------------------------------------------------------------------------
    def _on_device(self, v) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        return t.to(self.device, torch.float32).contiguous()

    def _aggregate(self, uncert: torch.Tensor, sdf: torch.Tensor) -> Tuple[bool, Dict]:
        agg = self._aggregator()
        targets = (self.select_targets or agg.select_targets)(uncert)
        return agg.uncertainty_aggregation_v2([uncert, sdf], force_running=self.planner_cfg.force_uncert_aggre, targets=targets)

    def compute_traversability_mask(self, sdf, pose: np.ndarray) -> np.ndarray:
        """naruto_planner.py:296-317."""
        self.local_planner.start_new_plan(start=self.loc2vox(pose[:3, 3]), goal=np.zeros((3)), sdf_map=sdf)
        self.local_planner.run_full()
        return self.local_planner.get_reachable_mask()

    def uncertainty_aware_planning_v2(self, uncert_sdf_vols: List, cur_pose: np.ndarray) -> Dict:
        """naruto_planner.py:319-401 -> {'path', 'is_goal_reachable', 'lookat_tgts'}."""
        c = self.planner_cfg
        uncert_vol, sdf_vol = self._on_device(uncert_sdf_vols[0]), self._on_device(uncert_sdf_vols[1])
        if self.step == 0:
            self.traversability_mask = np.ones(tuple(uncert_vol.shape), dtype=np.float32)
        if c.enable_uncert_filtering:
            uncert_vol = uncert_vol * self._on_device(self.traversability_mask)
        valid, outputs = self._aggregate(uncert_vol, sdf_vol)
        if not valid and c.enable_uncert_filtering:
            # nothing to see from any reachable-looking goal: find what IS reachable, drop the rest, aggregate again
            self.traversability_mask = self.compute_traversability_mask(sdf=sdf_vol, pose=cur_pose)
            uncert_vol = uncert_vol * self._on_device(self.traversability_mask)
            valid, outputs = self._aggregate(uncert_vol, sdf_vol)
        goal_vxl, lookat_tgts = self.goal_search_v2(outputs)
        path, is_goal_reachable, traversability_mask = self.path_planning_v2(sdf_vol=sdf_vol, cur_pose=cur_pose, goal_vxl=goal_vxl)
        if traversability_mask is not None:
            self.traversability_mask = traversability_mask
        return dict(path=path, is_goal_reachable=is_goal_reachable, lookat_tgts=lookat_tgts)

    def goal_search_v2(self, uncert_aggre_outputs: Dict) -> Tuple[np.ndarray, List[np.ndarray]]:
        """naruto_planner.py:462-510 -> (goal_vxl [3], look-at locations in metres), by naruto_goal_search."""
        agg = self._aggregator()
        r = goal_search(uncert_aggre_outputs["gs_aggre_uncerts"].reshape(-1), uncert_aggre_outputs["gs_uncert_collections"],
                        uncert_aggre_outputs["topk_uncert_vxl"].to(torch.int32).contiguous(), agg._goal_idx, self.planner_cfg.obs_per_goal,
                        self.bbox[:, 0], self.voxel_size)
        return r["goal_vxl"].astype(np.int64), [r["lookat_loc"][i] for i in range(r["n_lookat"])]

    def path_planning_v2(self, sdf_vol, cur_pose: np.ndarray, goal_vxl: np.ndarray) -> Tuple:
        """naruto_planner.py:403-460 -> (path [goal, ..., start], is_goal_reachable, traversability mask or None)."""
        if self.step == 0:
            sdf_vol = sdf_vol * 0. + 100.                                   # the first plan is made in an all-free volume
        self.local_planner.start_new_plan(start=self.loc2vox(cur_pose[:3, 3]), goal=goal_vxl, sdf_map=sdf_vol)
        traversability_mask, is_goal_reachable = None, True
        if not self.local_planner.run():
            self.info_printer("Run RRT second time to increase RRT node density.", self.step, self.__class__.__name__)
            is_goal_reachable = self.local_planner.run()
            if not is_goal_reachable:
                self.info_printer("Update observation traversability mask.", self.step, self.__class__.__name__)
                traversability_mask = self.local_planner.get_reachable_mask()
        return self.local_planner.find_path(), is_goal_reachable, traversability_mask

    # ---- collision (:512-594) -----------------------------------------------------------------------------------------------------
    def collision_scalars(self, next_c2w: np.ndarray) -> Tuple[float, float]:
        """(dist_closest, invalid_region_ratio) of the panorama at the pose: reduced on the device when the simulator can."""
        if hasattr(self.sim, "collision_probe"):
            return self.sim.collision_probe(next_c2w)
        _, _, _, erp_depth = self.sim.simulate(next_c2w, return_erp=True, no_print=True)
        return erp_depth.min(), (erp_depth > 1e6).sum() / (erp_depth.shape[0] * erp_depth.shape[1])

    def detect_collision_v2(self, sdf_vol, cur_pose: np.ndarray, next_pt_loc: np.ndarray) -> bool:
        from .rrt import is_collision_free
        c = self.planner_cfg
        if self.dataset not in DATASETS:
            raise NotImplementedError(f"dataset {self.dataset!r}")
        next_c2w = cur_pose.copy()
        next_c2w[:3, 3] = next_pt_loc
        dist_closest, invalid_region_ratio = self.collision_scalars(next_c2w)
        _, sdf_collision_free = is_collision_free(self.loc2vox(next_pt_loc), self.loc2vox(cur_pose[:3, 3]), sdf_vol, step_size=c.rrt_step_size)
        thre = c.get("invalid_region_ratio_thre", 0.2)
        if self.dataset == "Replica":
            collided = not sdf_collision_free
        elif self.dataset == "MP3D":
            collided = invalid_region_ratio > thre or not sdf_collision_free
        else:
            collided = dist_closest < c.collision_dist_thre or invalid_region_ratio > thre or not sdf_collision_free
        collided = bool(collided)
        if collided:
            for line in ("Collision Detected!", f"    Invalid region ratio: {float(invalid_region_ratio):.3f}", f"    SDF collision free: {sdf_collision_free}",
                         f"    Observation distance: {float(dist_closest) * 100:.3f}cm"):
                self.info_printer(line, self.step, self.__class__.__name__)
        return collided

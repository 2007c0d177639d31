"""The planner's host arithmetic restated in numpy: the CPU twin of tests/test_planner_host.py and tests/test_gpu_planner.py.

  * goal_search: what naruto_goal_search computes (reference goal_search_v2, naruto_planner.py:462-510) with the two tie rules the
    device states -- argmax: the lowest flat index among equal maxima; top-k: value descending, then target index ascending.
    Values are ordered by an integer key (NaN above +inf, +0 above -0), so there is nothing to round.
  * camera_pose, plan_rotations: compute_camera_pose (planner.py:119-153) and rotation_planning (rotation_planning.py:55-192) in
    fp64, unit quaternions (x, y, z, w), one rounding per written operation.
  * next_state / replay: the seven-state machine (naruto_planner.py:162-294) driven by recorded planning results and collision flags.
"""
from __future__ import annotations

import numpy as np

STATES = ("planning", "rotationPlanningAtStart", "rotatingAtStart", "movingToGoal", "rotationPlanningAtGoal", "rotatingAtGoal", "staying")

# every transition update_state can take
ALLOWED = {
    "planning": {"rotationPlanningAtStart", "staying"},
    "rotationPlanningAtStart": {"rotatingAtStart"},
    "rotatingAtStart": {"rotatingAtStart", "movingToGoal"},
    "movingToGoal": {"movingToGoal", "rotationPlanningAtGoal", "staying"},
    "rotationPlanningAtGoal": {"rotatingAtGoal"},
    "rotatingAtGoal": {"rotatingAtGoal", "planning"},
    "staying": {"staying", "planning"},
}


# ---- goal search -----------------------------------------------------------------------------------------------------------------
def descending_key(v) -> np.ndarray:
    """uint32 keys whose ASCENDING order is descending value order: float bits made monotone, then complemented."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    mono = np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000))
    return ~mono


def goal_search(aggregated, collections, targets, goal_idx, obs_per_goal, bbox_min, voxel_size):
    """-> dict with the fields of naruto_amd.planner.goal_search: all m = min(obs_per_goal, K) slots, n_lookat of them kept."""
    agg = np.asarray(aggregated, dtype=np.float32).reshape(-1)
    targets, goal_idx = np.asarray(targets).reshape(-1, 3), np.asarray(goal_idx).reshape(-1, 3)
    G, K = len(agg), len(targets)
    assert G > 0 and K > 0 and obs_per_goal > 0
    coll = np.asarray(collections, dtype=np.float32).reshape(G, K)
    key = descending_key(agg)
    goal = int(np.flatnonzero(key == key.min())[0])
    m = min(int(obs_per_goal), K)
    row = coll[goal]
    order = np.lexsort((np.arange(K), descending_key(row)))[:m]              # by key, then by index
    vals = row[order]
    vxl = targets[order].astype(np.int32)
    loc = vxl.astype(np.int64) * float(voxel_size) + np.asarray(bbox_min, dtype=np.float64)
    return {"goal": goal, "goal_vxl": goal_idx[goal].astype(np.int32), "n_lookat": max(int((vals > 0).sum()), 1), "lookat_idx": order.astype(np.int32),
            "lookat_vxl": vxl, "lookat_val": vals, "lookat_loc": loc}


# ---- rotations -------------------------------------------------------------------------------------------------------------------
def _unit(q):
    return q / np.sqrt(q @ q)


def to_quat(m):
    """The nearest orthonormal matrix (U V^T of the SVD) first; then Markley: the largest of m00, m11, m22 and the trace picks which
    component is formed from the diagonal."""
    u, _, vt = np.linalg.svd(np.asarray(m, dtype=np.float64))
    m = u @ vt
    t = m[0, 0] + m[1, 1] + m[2, 2]
    c = int(np.argmax([m[0, 0], m[1, 1], m[2, 2], t]))
    q = np.empty(4)
    if c == 3:
        q[:] = (m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1.0 + t)
    else:
        a, b, d = c, (c + 1) % 3, (c + 2) % 3
        q[a], q[b], q[d], q[3] = 1.0 - t + 2.0 * m[a, a], m[b, a] + m[a, b], m[d, a] + m[a, d], m[d, b] - m[b, d]
    return _unit(q)


def to_matrix(q):
    x, y, z, w = q
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[xx - yy - zz + ww, 2.0 * (xy - zw), 2.0 * (xz + yw)],
                     [2.0 * (xy + zw), -xx + yy - zz + ww, 2.0 * (yz - xw)],
                     [2.0 * (xz - yw), 2.0 * (yz + xw), -xx - yy + zz + ww]])


def compose(p, q):
    r = np.empty(4)
    r[:3] = p[3] * q[:3] + q[3] * p[:3] + np.cross(p[:3], q[:3])
    r[3] = p[3] * q[3] - p[:3] @ q[:3]
    return _unit(r)


def conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def angle_of(q):
    return 2.0 * np.arctan2(np.sqrt(q[:3] @ q[:3]), abs(q[3]))


def between(q1, q2):
    return compose(conj(q1), q2)


def log_map(q):
    q = -q if q[3] < 0 else q
    a = 2.0 * np.arctan2(np.sqrt(q[:3] @ q[:3]), q[3])
    s = 2.0 + a ** 2 / 12.0 + 7.0 * a ** 4 / 2880.0 if a <= 1e-3 else a / np.sin(a / 2.0)
    return s * q[:3]


def exp_map(v):
    a = np.sqrt(v @ v)
    s = 0.5 - a ** 2 / 48.0 + a ** 4 / 3840.0 if a <= 1e-3 else np.sin(a / 2.0) / a
    return np.array([s * v[0], s * v[1], s * v[2], np.cos(a / 2.0)])


def camera_pose(A, B, up=(0, 0, 1)):
    back = np.asarray(A) - np.asarray(B)
    if back[0] == 0 and back[1] == 0:
        back[0] = 1e-6
    right = np.cross(np.asarray(up), back)
    upv = np.cross(back, right)
    return np.column_stack((right / np.linalg.norm(right), upv / np.linalg.norm(upv), back / np.linalg.norm(back)))


def plan_rotations(R, targets, max_deg):
    """-> list of [3,3]: the current rotation, then towards the nearest remaining target each time, in steps of at most max_deg."""
    chain, left = [to_quat(R)], [to_quat(t) for t in targets]
    while left:
        i = int(np.argmin([angle_of(between(chain[-1], q)) for q in left]))
        chain.append(left.pop(i))
    out = [chain[0]]
    for a, b in zip(chain[:-1], chain[1:]):
        n = int(angle_of(between(a, b)) / np.pi * 180 / max_deg)
        v = log_map(between(a, b))
        out += [compose(a, exp_map(v * (i / n))) for i in range(1, n)] + [b]
    return [to_matrix(q) for q in out]


def hop_degrees(R, targets):
    """The angle of every hop of the greedy chain, in degrees (fixture conditions)."""
    chain, left = [to_quat(R)], [to_quat(t) for t in targets]
    hops = []
    while left:
        angles = [angle_of(between(chain[-1], q)) for q in left]
        i = int(np.argmin(angles))
        hops.append(angles[i] / np.pi * 180)
        chain.append(left.pop(i))
    return hops


# ---- the state machine -----------------------------------------------------------------------------------------------------------
def next_state(state, goal_reachable=False, rotations_left=0, path_left=0, collided=None, new_map=False):
    """update_state (:162-229).  ``collided`` is asked for only while moving with path left: pass a callable."""
    if state == "planning":
        return "rotationPlanningAtStart" if goal_reachable else "staying"
    if state == "rotationPlanningAtStart":
        return "rotatingAtStart"
    if state == "rotatingAtStart":
        return "movingToGoal" if rotations_left == 0 else "rotatingAtStart"
    if state == "movingToGoal":
        if path_left == 0:
            return "rotationPlanningAtGoal"
        return "staying" if collided() else "movingToGoal"
    if state == "rotationPlanningAtGoal":
        return "rotatingAtGoal"
    if state == "rotatingAtGoal":
        return "planning" if rotations_left == 0 else "rotatingAtGoal"
    if state == "staying":
        return "planning" if new_map else "staying"
    raise NotImplementedError(state)


def replay(rec):
    """Run the machine over a g14 trajectory with the RECORDED planning results (path, look-at list, reachable flag per planning
    call) and collision flags.  -> (state indices [n], poses float32 [n,4,4])."""
    bbox_min, voxel, up, max_deg = rec["bbox"][:, 0].astype(np.float64), float(rec["voxel_size"]), rec["up_dir"], float(rec["max_rot_deg"])
    plans, cols = iter(range(len(rec["plan_reachable"]))), iter(rec["col_result"])
    path_off, look_off = np.concatenate([[0], np.cumsum(rec["plan_path_len"])]), np.concatenate([[0], np.cumsum(rec["plan_lookat_len"])])
    state, pose = "staying", rec["start_pose"].astype(np.float32)
    reachable, path, looks, rots = False, [], [], []
    states, poses = [], []
    for step in range(len(rec["states"])):
        state = next_state(state, reachable, len(rots), len(path), lambda: bool(next(cols)), bool(rec["is_new_vols"][step]))
        new = pose.copy()
        if state == "planning":
            p = next(plans)
            reachable = bool(rec["plan_reachable"][p])
            path = [x for x in rec["plan_path_xyz"][path_off[p]:path_off[p + 1]]]
            looks = [x for x in rec["plan_lookat_xyz"][look_off[p]:look_off[p + 1]]]
        elif state in ("rotationPlanningAtStart", "rotationPlanningAtGoal"):
            aims = looks[:1] if state == "rotationPlanningAtStart" else looks
            rots = plan_rotations(pose[:3, :3], [camera_pose(pose[:3, 3], a, up) for a in aims], max_deg)
        elif state in ("rotatingAtStart", "rotatingAtGoal"):
            new[:3, :3] = rots.pop(0)
        elif state == "movingToGoal":
            loc = path.pop(-1) * voxel + bbox_min
            new[:3, :3] = camera_pose(loc, looks[0], up)
            new[:3, 3] = loc
        states.append(STATES.index(state))
        poses.append(new)
        pose = new
    return np.array(states), np.stack(poses)

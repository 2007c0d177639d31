"""numpy twin of the frame-to-model alignment (naruto_amd/registration.py restates the contract; csrc/naruto_sdfreg.hip).

* ``points``: q = T p in fp64 in the kernel's order, rounded once to float32; x = (q - bbox_min) / (bbox_max - bbox_min) in float32, operation
  by operation (the kernel forms no fused multiply-add): compared with ``==`` on the bits.
* ``accumulate``: r, g, the rows and the 30 sums in fp64 in the kernel's order -- thread t of workgroup b adds points b*2048 + t + 256 k,
  k = 0..7 in turn; the 256 vectors fold by halves; the finishing workgroup's thread t adds the workgroups t, t + 256, ... and folds the
  same way (odometry_spec.reduce_sums's rule over 30 columns).  Compared on the bits.
* the step is odometry_spec.step on the first 29 sums (compared within the solver's bound, as the odometry's).
* ``verdict`` and ``commit``: plain fp64 / one rounding to float32.
* ``align``: the whole loop with the field as a callable ``field(x float32 [M,3]) -> (sdf float32 [M], d_x float32 [M,3])``.
* ``BoxRoom``: an analytic closed-box room -- exact depth frames and the exact truncated SDF with its gradient.
"""
import math

import numpy as np

import odometry_spec as OS

F32 = np.float32
SUMS, THREADS, PER, RECORD = 30, 256, 8, 8
SDF_GATE, MIN_OVERLAP, MAX_ROT_DEG, ITERS = 0.9, 0.25, 4.0, 6


def gate(max_trans, max_rot_deg=MAX_ROT_DEG, min_overlap=MIN_OVERLAP):
    """The verdict's thresholds as the device takes them: min_trace = 1 + 2 cos(max_rot)."""
    return {"max_trans": float(max_trans), "min_trace": 1.0 + 2.0 * math.cos(math.radians(max_rot_deg)), "min_overlap": float(min_overlap)}


# ---------------------------------------------------------------------------------------------------------------- points (float32)
def points(T, verts, bbox_min, bbox_max):
    """(x float32 [M,3], q float32 [M,3], valid bool [M]) of the vertices [M,3] (float32) under T [4,4] (fp64)."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(verts, F32).reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(bbox_min, F32), np.asarray(bbox_max, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], -1).astype(F32)
        x = ((q - lo[None]) / (hi - lo)[None]).astype(F32)
        valid = (p[:, 2] < 0.0) & ((x >= 0) & (x <= 1)).all(1)
    return np.where(valid[:, None], x, F32(0.5)).astype(F32), q, valid


# ---------------------------------------------------------------------------------------------------------------- rows and sums (fp64)
def terms(sdf, d_x, q, valid, trunc, bbox_min, bbox_max, sdf_gate=SDF_GATE):
    """(flag [M], r [M], terms [M,30]) of one evaluation: fp64 in the kernel's order.  trunc and sdf_gate are the float32 values."""
    trunc, sdf_gate = float(F32(trunc)), float(F32(sdf_gate))
    ext = (np.asarray(bbox_max, F32) - np.asarray(bbox_min, F32)).astype(np.float64)
    sdf = np.asarray(sdf, F32).reshape(-1).astype(np.float64)
    d = np.asarray(d_x, F32).reshape(-1, 3).astype(np.float64)
    q = np.asarray(q, F32).reshape(-1, 3).astype(np.float64)
    valid = np.asarray(valid).reshape(-1) != 0
    n = sdf.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        g = (trunc * d) / ext[None]
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        ok = valid & (np.abs(sdf) < sdf_gate) & (gg > 0.0) & (gg < np.inf)
        r = trunc * sdf
        J = np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2], q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0],
                      g[:, 0], g[:, 1], g[:, 2]], -1)
        cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r, np.ones(n)]
        t = np.where(ok[:, None], np.stack(cols, -1), 0.0)
    t = np.concatenate([t, valid.astype(np.float64)[:, None]], 1)
    return ok.astype(np.float64), np.where(ok, r, 0.0), t


def _fold(a):
    a = a.copy()
    w = THREADS // 2
    while w > 0:
        a[..., :w, :] = a[..., :w, :] + a[..., w:2 * w, :]
        w //= 2
    return a[..., 0, :]


def reduce_sums(t):
    """odometry_spec.reduce_sums over any number of columns."""
    n, c = t.shape
    parts = max(1, -(-n // (THREADS * PER)))
    a = np.zeros((parts * THREADS * PER, c))
    a[:n] = t
    a = a.reshape(parts, PER, THREADS, c)
    acc = np.zeros((parts, THREADS, c))
    for k in range(PER):
        acc = acc + a[:, k]
    part = _fold(acc)
    m = -(-parts // THREADS)
    b = np.zeros((m * THREADS, c))
    b[:parts] = part
    b = b.reshape(m, THREADS, c)
    acc = np.zeros((THREADS, c))
    for k in range(m):
        acc = acc + b[k]
    return _fold(acc)


def accumulate(sdf, d_x, q, valid, trunc, bbox_min, bbox_max, sdf_gate=SDF_GATE):
    """(sums [30], rows [M,2] = (accepted flag, r))."""
    flag, r, t = terms(sdf, d_x, q, valid, trunc, bbox_min, bbox_max, sdf_gate)
    return reduce_sums(t), np.stack([flag, r], -1)


def sum_bounds(sdf, d_x, q, valid, trunc, bbox_min, bbox_max, d_sdf, d_grad, sdf_gate=SDF_GATE):
    """A bound per sum [29] on the change of ``accumulate``'s first 29 sums when every sdf moves by at most ``d_sdf`` and every component of
    d_x by at most ``d_grad``: the budget carried through each term (r and g are linear in them, J is linear in g, every term a product of
    two such factors: |a| db + |b| da + da db), summed over the rows; a row whose acceptance the budget can flip adds its whole term."""
    trunc_, gate_ = float(F32(trunc)), float(F32(sdf_gate))
    ext = (np.asarray(bbox_max, F32) - np.asarray(bbox_min, F32)).astype(np.float64)
    flag, r, t = terms(sdf, d_x, q, valid, trunc, bbox_min, bbox_max, sdf_gate)
    sdf = np.asarray(sdf, F32).reshape(-1).astype(np.float64)
    g = (trunc_ * np.asarray(d_x, F32).reshape(-1, 3).astype(np.float64)) / ext[None]
    q = np.abs(np.asarray(q, F32).reshape(-1, 3).astype(np.float64))
    dg = np.broadcast_to(trunc_ * d_grad / ext, g.shape)
    dr = trunc_ * d_sdf
    J = np.abs(np.stack([q[:, 1] * 0, q[:, 1] * 0, q[:, 1] * 0, g[:, 0], g[:, 1], g[:, 2]], -1))
    ag = np.abs(g)
    J[:, 0], J[:, 1], J[:, 2] = q[:, 1] * ag[:, 2] + q[:, 2] * ag[:, 1], q[:, 2] * ag[:, 0] + q[:, 0] * ag[:, 2], q[:, 0] * ag[:, 1] + q[:, 1] * ag[:, 0]
    dJ = np.stack([q[:, 1] * dg[:, 2] + q[:, 2] * dg[:, 1], q[:, 2] * dg[:, 0] + q[:, 0] * dg[:, 2], q[:, 0] * dg[:, 1] + q[:, 1] * dg[:, 0],
                   dg[:, 0], dg[:, 1], dg[:, 2]], -1)
    ar = np.abs(trunc_ * sdf)
    cols = [J[:, a] * dJ[:, b] + J[:, b] * dJ[:, a] + dJ[:, a] * dJ[:, b] for a in range(6) for b in range(a, 6)]
    cols += [J[:, a] * dr + ar * dJ[:, a] + dJ[:, a] * dr for a in range(6)] + [2.0 * ar * dr + dr * dr, np.zeros(len(sdf))]
    per_row = np.stack(cols, -1)
    whole = np.stack([J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * ar for a in range(6)] + [ar * ar, np.ones(len(sdf))], -1)
    gmax = ag.max(1)
    unsure = (np.asarray(valid).reshape(-1) != 0) & ((np.abs(np.abs(sdf) - gate_) <= d_sdf) | (gmax <= dg.max(1)))   # the gate or g.g > 0 may flip
    sure = (flag != 0) & ~unsure
    return np.where(sure[:, None], per_row, 0.0).sum(0) + np.where(unsure[:, None], whole + per_row, 0.0).sum(0)


def evaluate(T, verts, field, trunc, bbox_min, bbox_max, sdf_gate=SDF_GATE):
    """points -> field -> accumulate: (sums [30], rows [M,2])."""
    x, q, valid = points(T, verts, bbox_min, bbox_max)
    sdf, d_x = field(x)
    return accumulate(sdf, d_x, q, valid, trunc, bbox_min, bbox_max, sdf_gate)


# ---------------------------------------------------------------------------------------------------------------- verdict, commit
def _finite_or(v, other=-1.0):
    return float(v) if math.isfinite(v) else other


def _div(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else float("nan")


def verdict(g, status, sums_start, sums_final, T, T_start):
    """(passed, T, record [8]): k_sdfreg_verdict.  status: the finest level's status word."""
    T, T0 = np.asarray(T, np.float64).reshape(4, 4), np.asarray(T_start, np.float64).reshape(4, 4)
    n_valid, n_rows = float(sums_final[29]), float(sums_final[28])
    mse0, mse1 = _div(sums_start[27], sums_start[28]), _div(sums_final[27], n_rows)
    d = T[:3, 3] - T0[:3, 3]
    t2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    trace = 0.0
    for a in range(3):
        for b in range(3):
            trace = trace + T0[a, b] * T[a, b]
    passed = bool(status != OS.DEGENERATE and n_rows >= g["min_overlap"] * n_valid and n_rows > 0.0 and mse1 <= mse0
                  and t2 <= g["max_trans"] * g["max_trans"] and trace >= g["min_trace"])
    record = np.array([1.0 if passed else 0.0, n_valid, n_rows, _finite_or(_sqrt(mse0)), _finite_or(_sqrt(mse1)), _finite_or(_sqrt(t2)),
                       _finite_or(trace), float(status)])
    return passed, (T if passed else T0).copy(), record


def pose_log(c2w):
    """naruto_pose.h's pose_log of a float32 matrix, branch for branch: (omega, t) float32 [6]."""
    M = np.asarray(c2w, F32).reshape(4, 4).astype(np.float64)
    d0, d1, d2 = M[0, 0], M[1, 1], M[2, 2]
    cand = [1.0 + d0 + d1 + d2, 1.0 + d0 - d1 - d2, 1.0 - d0 + d1 - d2, 1.0 - d0 - d1 + d2]
    br = 0
    for i in range(1, 4):
        if cand[i] > cand[br]:
            br = i
    s = 2.0 * math.sqrt(max(cand[br], 1e-300))
    q4 = s / 4.0
    x, y, z = M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]
    xy, xz, yz = M[0, 1] + M[1, 0], M[0, 2] + M[2, 0], M[1, 2] + M[2, 1]
    q = [[q4, x / s, y / s, z / s], [x / s, q4, xy / s, xz / s], [y / s, xy / s, q4, yz / s], [z / s, xz / s, yz / s, q4]][br]
    if q[0] < 0.0:
        q = [-v for v in q]
    n = math.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    scale = 2.0 / q[0] if n < 1e-12 else 2.0 * math.atan2(n, q[0]) / n
    return np.array([q[1] * scale, q[2] * scale, q[3] * scale, M[0, 3], M[1, 3], M[2, 3]]).astype(F32)


def commit(T):
    """(est [4,4] float32 = T rounded once, pose6 [6] float32 = the log of the stored matrix)."""
    est = np.asarray(T, np.float64).reshape(4, 4).astype(F32)
    return est, pose_log(est)


# ---------------------------------------------------------------------------------------------------------------- the whole estimate
def align(verts, T_start, field, trunc, bbox_min, bbox_max, levels, iters, g, sdf_gate=SDF_GATE, trace=None):
    """``verts``: {level: float32 [M,3]}; ``levels`` from the coarsest to the finest with the caps ``iters``; T_start float32 [4,4] (est[i]).
    -> dict(T, passed, record, status {level}, iterations {level}, inliers {level}, rmse {level}).  ``trace`` (a list) receives T after
    every step."""
    T0 = np.asarray(T_start, F32).reshape(4, 4).astype(np.float64)
    T = T0.copy()
    finest = levels[-1]
    args = (field, trunc, bbox_min, bbox_max, sdf_gate)
    sums_start, _ = evaluate(T, verts[finest], *args)
    status, its, inl, rmse = {}, {}, {}, {}
    for l, cap in zip(levels, iters):
        done, upd, status[l], inl[l], rmse[l] = False, 0, OS.RUNNING, 0.0, 0.0
        for _ in range(cap):
            if done:
                break
            sums, _ = evaluate(T, verts[l], *args)
            T, done, status[l], upd, inl[l], rmse[l] = OS.step(sums[:29], T, upd, cap)
            if trace is not None:
                trace.append(T.copy())
        its[l] = upd
    sums_final, _ = evaluate(T, verts[finest], *args)
    passed, T, record = verdict(g, status[finest], sums_start, sums_final, T, T0)
    return {"T": T, "passed": passed, "record": record, "status": status, "iterations": its, "inliers": inl, "rmse": rmse}


# ---------------------------------------------------------------------------------------------------------------- the analytic room
class BoxRoom:
    """A closed box [0,size]: depth frames from inside and sdf = clip(distance to the nearest wall / trunc, -1, 1) (positive inside), with
    the gradient +-1/trunc on that wall's axis, 0 where saturated.  The field's bounding box is the room grown by ``margin``."""

    def __init__(self, size=(4.0, 3.0, 2.5), trunc=0.1, margin=0.5):
        self.size, self.trunc = np.asarray(size, np.float64), float(trunc)
        self.bbox_min, self.bbox_max = (np.zeros(3) - margin).astype(F32), (self.size + margin).astype(F32)

    def depth(self, c2w, cam):
        """The exact depth along -z of every pixel's ray, float32 [H,W]."""
        c2w = np.asarray(c2w, np.float64).reshape(4, 4)
        h, w = int(cam["H"]), int(cam["W"])
        u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        d = np.stack([(u - cam["cx"]) / cam["fx"], -(v - cam["cy"]) / cam["fy"], -np.ones_like(u)], -1) @ c2w[:3, :3].T
        o = c2w[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(d > 0, (self.size - o) / d, np.where(d < 0, (0.0 - o) / d, np.inf))
        return s.min(-1).astype(F32)

    def world(self, x):
        return self.bbox_min.astype(np.float64) + np.asarray(x, np.float64) * (self.bbox_max - self.bbox_min).astype(np.float64)

    def field(self, x):
        """(sdf float32 [M], d sdf / d x float32 [M,3]) at the normalised points x."""
        p = self.world(x)
        both = np.concatenate([p, self.size[None] - p], 1)                  # distances to the six walls, positive inside
        k = both.argmin(1)
        s = both[np.arange(len(p)), k] / self.trunc
        grad = np.zeros_like(p)
        grad[np.arange(len(p)), k % 3] = np.where(k < 3, 1.0, -1.0) / self.trunc
        grad = np.where((np.abs(s) < 1.0)[:, None], grad, 0.0) * (self.bbox_max - self.bbox_min).astype(np.float64)[None]
        return np.clip(s, -1.0, 1.0).astype(F32), grad.astype(F32)


def perturb(c2w, metres, along, deg, axis):
    """The pose moved by ``metres`` along ``along`` (field frame) and turned by ``deg`` about ``axis`` (camera frame)."""
    out = np.array(c2w, np.float64).reshape(4, 4).copy()
    if deg:
        out[:3, :3] = out[:3, :3] @ OS.rotation(axis, math.radians(deg))
    if metres:
        out[:3, 3] += metres * np.asarray(along, np.float64) / np.linalg.norm(along)
    return out


def pose_error(T, ref):
    """(metres, degrees) between two poses.  The angle comes from the antisymmetric part of R^T R_ref (atan2 of its length and the trace's
    cosine): acos of a trace alone turns the 1e-7 by which a float32-rounded rotation misses orthonormality into 0.02 degrees."""
    T, ref = np.asarray(T, np.float64).reshape(4, 4), np.asarray(ref, np.float64).reshape(4, 4)
    R = T[:3, :3].T @ ref[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.linalg.norm(T[:3, 3] - ref[:3, 3])), math.degrees(math.atan2(float(np.linalg.norm(v)), (np.trace(R) - 1.0) / 2.0))


# the prototype's five starts: (metres, degrees); the rotation of the third about three axes in turn
STARTS = ((0.03, 1.5), (0.05, 0.0), (0.0, 3.0), (0.08, 3.0), (0.12, 0.0))
START_ALONG, START_AXIS = (0.6, 0.3, -0.74), (0.3, -0.8, 0.5)

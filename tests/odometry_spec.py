"""numpy twin of the depth odometry (naruto_amd/odometry.py restates the contract; csrc/naruto_odom.hip, csrc/naruto_odom.h).

* The maps are float32, operation by operation in the kernel's order, so they are compared with ``==`` on the bits.  Fused multiply-add:
  the kernel switches contraction off and forms none (every product and every sum is rounded on its own), so there is nothing to emulate
  here -- unlike ``helpers.fma32`` for the ray points -- and plain float32 numpy operations make the same bits.  Division and square root
  are correctly rounded on both sides.
* The association, the rows and the 29 sums are fp64 in the kernel's order: thread t of workgroup b adds pixels b*2048 + t + 256 k,
  k = 0..7 in turn; the 256 vectors fold by halves; the finishing workgroup's thread t adds the workgroups t, t + 256, ... in turn and folds
  the same way.  A rejected pixel adds nothing, which +0.0 restates exactly.  Compared on the bits.
* The step (Cholesky, the se(3) exponential, T <- exp(xi) T) is fp64 operation by operation in Python floats; sin / cos / the compiler's
  own fused multiply-adds in that scalar code may differ in the last bits, so it is compared within tests/test_odometry_host.py's bound.
"""
import math

import numpy as np

F32 = np.float32
SUMS, THREADS, PER = 29, 256, 8
RUNNING, CONVERGED, DEGENERATE, MAX_ITERATION = 0, 1, 2, 3
STATUS = ("running", "converged", "degenerate", "max_iteration")


# ---------------------------------------------------------------------------------------------------------------- maps (float32)
def level_intrinsics(cam, levels):
    """[(h, w, fx, fy, cx, cy)] per level, intrinsics float32 level by level."""
    h, w = int(cam["H"]), int(cam["W"])
    fx, fy, cx, cy = (F32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    out = []
    for _ in range(levels):
        out.append((h, w, fx, fy, cx, cy))
        h, w = h // 2, w // 2
        fx, fy = fx / F32(2), fy / F32(2)
        cx, cy = (cx + F32(0.5)) / F32(2) - F32(0.5), (cy + F32(0.5)) / F32(2) - F32(0.5)
    return out


def clean_depth(depth):
    d = np.asarray(depth, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where((d > 0) & (d < np.inf), d, F32(0)).astype(F32)


def half_depth(d, band):
    h, w = d.shape[0] // 2, d.shape[1] // 2
    c = [d[dv:2 * h:2, du:2 * w:2] for dv, du in ((0, 0), (0, 1), (1, 0), (1, 1))]
    lo = np.full((h, w), np.inf, dtype=F32)
    for k in c:
        lo = np.where((k > 0) & (k < lo), k, lo)
    s, n = np.zeros((h, w), F32), np.zeros((h, w), F32)
    for k in c:
        with np.errstate(invalid="ignore"):
            inc = (k > 0) & ((k - lo) <= F32(band))
        s = np.where(inc, s + k, s)
        n = np.where(inc, n + F32(1), n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / n, F32(0)).astype(F32)


def vertex_map(d, fx, fy, cx, cy):
    h, w = d.shape
    dx = (np.arange(w, dtype=F32) - cx) / fx
    dy = -((np.arange(h, dtype=F32) - cy) / fy)
    return np.stack([d * dx[None, :], d * dy[:, None], -d], -1).astype(F32)


def normal_map(d, V, jump):
    h, w = d.shape
    N = np.zeros((h, w, 3), F32)
    if h < 2 or w < 2:
        return N
    a, b = V[:-1, 1:] - V[:-1, :-1], V[1:, :-1] - V[:-1, :-1]
    c = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    length = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
    ok = (d[:-1, :-1] > 0) & (d[:-1, 1:] > 0) & (d[1:, :-1] > 0) & (np.abs(a[..., 2]) < F32(jump)) & (np.abs(b[..., 2]) < F32(jump)) & (length > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        N[:-1, :-1] = np.where(ok[..., None], c / length[..., None], F32(0))
    return N


def frame_maps(depth, cam, levels=3, jump=0.15, band=0.1):
    """[(depth [h,w], vertex [h,w,3], normal [h,w,3])] per level, float32."""
    out, d = [], clean_depth(depth)
    for l, (h, w, fx, fy, cx, cy) in enumerate(level_intrinsics(cam, levels)):
        if l > 0:
            d = half_depth(d, band)
        assert d.shape == (h, w)
        V = vertex_map(d, fx, fy, cx, cy)
        out.append((d, V, normal_map(d, V, jump)))
    return out


def pack_maps(maps):
    """The maps block as the device lays it out: per level depth | vertex | normal."""
    return np.concatenate([a.reshape(-1) for level in maps for a in level]).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- rows and sums (fp64)
def rows(T, level_cam, prev, cur, max_dist=0.25):
    """(index int64 [n] (-1 = rejected), residual [n], terms [n,29]) of one evaluation at a level: fp64 in the kernel's order."""
    h, w, fx, fy, cx, cy = level_cam
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    T = np.asarray(T, np.float64).reshape(4, 4)
    n = h * w
    p = cur[1].reshape(n, 3).astype(np.float64)
    pv, pn = prev[1].reshape(n, 3).astype(np.float64), prev[2].reshape(n, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    q = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], -1)
    ok = z < 0.0
    zc = -q[:, 2]
    ok &= zc > 1e-6
    zs = np.where(ok, zc, 1.0)
    u = np.floor(((fx * q[:, 0]) / zs + cx) + 0.5)
    v = np.floor(((-(fy * q[:, 1])) / zs + cy) + 0.5)
    ok &= (u >= 0.0) & (u < float(w)) & (v >= 0.0) & (v < float(h))
    j = np.where(ok, v * w + u, 0).astype(np.int64)
    nn = pn[j]
    ok &= (nn != 0.0).any(1)
    d = q - pv[j]
    md = float(F32(max_dist))
    ok &= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= md * md
    r = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
    J = np.stack([q[:, 1] * nn[:, 2] - q[:, 2] * nn[:, 1], q[:, 2] * nn[:, 0] - q[:, 0] * nn[:, 2], q[:, 0] * nn[:, 1] - q[:, 1] * nn[:, 0],
                  nn[:, 0], nn[:, 1], nn[:, 2]], -1)
    cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r, np.ones(n)]
    terms = np.where(ok[:, None], np.stack(cols, -1), 0.0)
    return np.where(ok, j, -1), np.where(ok, r, 0.0), terms


def _fold(a):
    """[.., 256, 29] -> [.., 29]: the halving tree."""
    a = a.copy()
    w = THREADS // 2
    while w > 0:
        a[..., :w, :] = a[..., :w, :] + a[..., w:2 * w, :]
        w //= 2
    return a[..., 0, :]


def reduce_sums(terms):
    n = terms.shape[0]
    parts = max(1, -(-n // (THREADS * PER)))
    t = np.zeros((parts * THREADS * PER, SUMS))
    t[:n] = terms
    t = t.reshape(parts, PER, THREADS, SUMS)
    acc = np.zeros((parts, THREADS, SUMS))
    for k in range(PER):
        acc = acc + t[:, k]
    part = _fold(acc)                                       # [parts, 29]
    m = -(-parts // THREADS)
    t2 = np.zeros((m * THREADS, SUMS))
    t2[:parts] = part
    t2 = t2.reshape(m, THREADS, SUMS)
    acc = np.zeros((THREADS, SUMS))
    for k in range(m):
        acc = acc + t2[k]
    return _fold(acc)


# ---------------------------------------------------------------------------------------------------------------- the step (fp64)
def solve(sums):
    """(status, xi [6]): naruto_odom.h's odom_solve."""
    xi = [0.0] * 6
    if not sums[28] >= 6.0:
        return DEGENERATE, xi
    L = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            L[i][j] = L[j][i] = float(sums[k])
            k += 1
    top = max(0.0, *[L[i][i] for i in range(6)])
    if not top > 0.0:
        return DEGENERATE, xi
    for j in range(6):
        d = L[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        if not d > 1e-12 * top:
            return DEGENERATE, xi
        p = math.sqrt(d)
        L[j][j] = p
        for i in range(j + 1, 6):
            s = L[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s / p
    y = [0.0] * 6
    for i in range(6):
        s = -float(sums[21 + i])
        for k in range(i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k][i] * xi[k]
        xi[i] = s / L[i][i]
    return RUNNING, xi


def se3_exp(xi):
    w = [float(v) for v in xi[:3]]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < 1e-4:
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0))
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0))
        Cc = 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0 * (1.0 - th2 / 72.0))
    else:
        th = math.sqrt(th2)
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
        Cc = (1.0 - A) / th2
    K = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    E = np.eye(4)
    for i in range(3):
        tv = 0.0
        for j in range(3):
            k2 = 0.0
            for m in range(3):
                k2 += K[i][m] * K[m][j]
            e = 1.0 if i == j else 0.0
            E[i, j] = e + A * K[i][j] + B * k2
            tv += (e + B * K[i][j] + Cc * k2) * float(xi[3 + j])
        E[i, 3] = tv
    return E


def step(sums, T, updates, cap):
    """One k_odom_step: -> (T, done, status, updates, inliers, rmse)."""
    count = float(sums[28])
    rmse = math.sqrt(float(sums[27]) / count) if count > 0.0 else 0.0
    status, xi = solve(sums)
    if status != RUNNING:
        return np.array(T, np.float64).reshape(4, 4), True, DEGENERATE, updates, count, rmse
    E = se3_exp(xi)
    T0 = np.asarray(T, np.float64).reshape(4, 4)
    Tn = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += E[i, k] * T0[k, j]
            Tn[i, j] = s
    updates += 1
    small = math.sqrt(xi[0] ** 2 + xi[1] ** 2 + xi[2] ** 2) < 1e-6 and math.sqrt(xi[3] ** 2 + xi[4] ** 2 + xi[5] ** 2) < 1e-6
    if small:
        return Tn, True, CONVERGED, updates, count, rmse
    if updates >= cap:
        return Tn, True, MAX_ITERATION, updates, count, rmse
    return Tn, False, RUNNING, updates, count, rmse


def estimate(maps_prev, maps_cur, cam, levels=3, iters=(10, 5, 4), max_dist=0.25, init=None):
    """The whole estimate on the twin: (T [4,4], status per level, iterations per level)."""
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    cams = level_intrinsics(cam, levels)
    status, its = [RUNNING] * levels, [0] * levels
    for k, cap in enumerate(iters):
        l = levels - 1 - k
        done, upd = False, 0
        for _ in range(cap):
            if done:
                break
            _, _, terms = rows(T, cams[l], maps_prev[l], maps_cur[l], max_dist)
            T, done, status[l], upd, _, _ = step(reduce_sums(terms), T, upd, cap)
        its[l] = upd
    return T, status, its


# ---------------------------------------------------------------------------------------------------------------- scenes and scores
def rotation(axis, theta):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def relative_motion(axis, deg, along, dist):
    T = np.eye(4)
    T[:3, :3] = rotation(axis, math.radians(deg))
    T[:3, 3] = dist * np.asarray(along, np.float64) / np.linalg.norm(along)
    return T


# the prototype's six cases: (metres, degrees) about two axes, along one direction (camera coordinates of the previous frame)
CASE_STEPS = ((0.03, 2.0), (0.10, 10.0), (0.10, 20.0))
CASE_AXES = ((0.0, 1.0, 0.0), (0.3, -0.8, 0.5))
CASE_ALONG = (0.6, 0.3, -0.74)
CASES = [relative_motion(ax, deg, CASE_ALONG, dist) for dist, deg in CASE_STEPS for ax in CASE_AXES]
CASE_POSITION = (1.4, 1.2, 1.2)
BOUND_M, BOUND_DEG = 5e-3, 0.25


def motion_error(T, ref):
    """(metres, degrees) between two rigid transforms."""
    T, ref = np.asarray(T, np.float64).reshape(4, 4), np.asarray(ref, np.float64).reshape(4, 4)
    R = T[:3, :3].T @ ref[:3, :3]
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    return float(np.linalg.norm(T[:3, 3] - ref[:3, 3])), math.degrees(math.acos(c))

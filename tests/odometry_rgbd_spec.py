"""numpy twin of the RGB-D odometry (naruto_amd/odometry.py restates the contract; csrc/naruto_odom.hip): tests/odometry_spec.py's depth
odometry plus the intensity maps, the photometric row and the 32 sums.

* The intensity maps are float32, operation by operation in the kernel's order (contraction off), compared on the bits.  A NaN's sign
  and payload are not part of the contract: compare through ``canonical`` (every NaN becomes one pattern).
* Both rows of a pixel and the 32 sums are fp64 in the kernel's order: ``rows_rgbd`` gives terms [n,2,32] (the geometric row's, then the
  photometric row's); ``reduce_sums`` adds, per pixel, the geometric terms first and then the photometric ones, pixels / threads / the
  fold / the finishing launch as ``odometry_spec.reduce_sums``.  A rejected row adds +0.0, which changes no bit.
* The photometric row's order of operations, with w = float32 ``photo_weight`` as a double, A = gx*fx, B = gy*fy:
  g = (w*(A/zc), w*(-(B/zc)), w*((A*q.x - B*q.y)/(zc*zc))), r = w*r_I, J = [q x g, g] exactly as the geometric row forms [q x n, n].
* The step is ``odometry_spec.step`` on the first 29 sums.
"""
import math

import numpy as np

import odometry_spec as OS

F32 = np.float32
SUMS = 32
PHOTO_WEIGHT, PHOTO_MAX_DIFF = 0.1, 0.3


# ---------------------------------------------------------------------------------------------------------------- maps (float32)
def intensity(color):
    c = np.asarray(color, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((F32(0.299) * c[..., 0] + F32(0.587) * c[..., 1]) + F32(0.114) * c[..., 2]).astype(F32)


def half_intensity(I):
    h, w = I.shape[0] // 2, I.shape[1] // 2
    a, b, c, d = (I[dv:2 * h:2, du:2 * w:2] for dv, du in ((0, 0), (0, 1), (1, 0), (1, 1)))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((((a + b) + c) + d) * F32(0.25)).astype(F32)


def gradients(I):
    h, w = I.shape
    gx, gy = np.zeros((h, w), F32), np.zeros((h, w), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if w >= 3:
            gx[:, 1:-1] = (I[:, 2:] - I[:, :-2]) * F32(0.5)
        if h >= 3:
            gy[1:-1, :] = (I[2:, :] - I[:-2, :]) * F32(0.5)
    return gx, gy


def intensity_maps(color, levels=3):
    """[(I [h,w], gx [h,w], gy [h,w])] per level, float32."""
    out, I = [], intensity(color)
    for l in range(levels):
        if l > 0:
            I = half_intensity(I)
        out.append((I,) + gradients(I))
    return out


def frame_maps(depth, color, cam, levels=3, jump=0.15, band=0.1):
    """(the depth twin's maps, the intensity maps)."""
    return OS.frame_maps(depth, cam, levels, jump, band), intensity_maps(color, levels)


def pack_maps(maps):
    """The RGB-D maps block: the depth maps block, then per level I | gx | gy."""
    dmaps, imaps = maps
    return np.concatenate([OS.pack_maps(dmaps)] + [a.reshape(-1) for level in imaps for a in level]).astype(F32)


def canonical(a):
    """float32 bits with every NaN as one pattern."""
    a = np.ascontiguousarray(a, dtype=F32)
    return np.where(np.isnan(a), F32(np.nan), a).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- rows and sums (fp64)
def _bilinear(m, u0, v0, a, b):
    s00, s10, s01, s11 = m[v0, u0], m[v0, u0 + 1], m[v0 + 1, u0], m[v0 + 1, u0 + 1]
    top = s00 + a * (s10 - s00)
    bot = s01 + a * (s11 - s01)
    return top + b * (bot - top)


def _terms(q, g, r, ok, extra):
    """[n,32]: the row J = [q x g, g] with residual r into [0..28], ``extra`` = {index: column} beside them; zeros where not ok."""
    n = len(r)
    with np.errstate(invalid="ignore", over="ignore"):
        return _terms_unmasked(n, q, g, r, ok, extra)


def _terms_unmasked(n, q, g, r, ok, extra):
    J = np.stack([q[:, 1] * g[:, 2] - q[:, 2] * g[:, 1], q[:, 2] * g[:, 0] - q[:, 0] * g[:, 2], q[:, 0] * g[:, 1] - q[:, 1] * g[:, 0],
                  g[:, 0], g[:, 1], g[:, 2]], -1)
    cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)] + [r * r, np.ones(n)]
    cols += [extra.get(k, np.zeros(n)) for k in (29, 30, 31)]
    return np.where(ok[:, None], np.stack(cols, -1), 0.0)


def photo_rows(T, level_cam, prev, cur, iprev, icur, max_dist=0.25, photo_weight=PHOTO_WEIGHT, photo_max_diff=PHOTO_MAX_DIFF):
    """The photometric rows of one evaluation: (ok [n], j [n], r_I [n], q [n,3], g [n,3]); r_I and g are 0 where not ok."""
    h, w, fx, fy, cx, cy = level_cam
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    T = np.asarray(T, np.float64).reshape(4, 4)
    n = h * w
    lam, md, mdiff = float(F32(photo_weight)), float(F32(max_dist)), float(F32(photo_max_diff))
    p = cur[1].reshape(n, 3).astype(np.float64)
    pv = prev[1].reshape(n, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    q = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], -1)
    ok = z < 0.0
    zc = -q[:, 2]
    ok &= zc > 1e-6
    zs = np.where(ok, zc, 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        uc = (fx * q[:, 0]) / zs + cx
        vc = (-(fy * q[:, 1])) / zs + cy
        u0, v0 = np.floor(uc), np.floor(vc)
        ok &= (u0 >= 1.0) & (u0 + 1.0 <= float(w) - 2.0) & (v0 >= 1.0) & (v0 + 1.0 <= float(h) - 2.0)
        ok &= lam > 0.0
        u, v = np.floor(uc + 0.5), np.floor(vc + 0.5)
    j = np.where(ok, v * w + u, 0).astype(np.int64)
    d = q - pv[j]
    ok &= pv[j, 2] < 0.0
    ok &= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= md * md
    iu, iv = np.where(ok, u0, 1).astype(np.int64), np.where(ok, v0, 1).astype(np.int64)
    if h < 4 or w < 4:                                      # no pixel has four interior neighbours
        assert not ok.any()
        return ok, j, np.zeros(n), q, np.zeros((n, 3))
    a, b = np.where(ok, uc - u0, 0.0), np.where(ok, vc - v0, 0.0)
    Ip, gxp, gyp = (m.astype(np.float64) for m in iprev)
    with np.errstate(invalid="ignore", over="ignore"):
        rI = _bilinear(Ip, iu, iv, a, b) - icur[0].reshape(n).astype(np.float64)
        gx, gy = _bilinear(gxp, iu, iv, a, b), _bilinear(gyp, iu, iv, a, b)
        ok &= (np.abs(rI) <= mdiff) & (np.abs(gx) < np.inf) & (np.abs(gy) < np.inf)
        rI, gx, gy = np.where(ok, rI, 0.0), np.where(ok, gx, 0.0), np.where(ok, gy, 0.0)
        A, B = gx * fx, gy * fy
        g = np.stack([lam * (A / zs), lam * (-(B / zs)), lam * ((A * q[:, 0] - B * q[:, 1]) / (zs * zs))], -1)
    return ok, j, rI, q, g


def rows_rgbd(T, level_cam, prev, cur, iprev, icur, max_dist=0.25, photo_weight=PHOTO_WEIGHT, photo_max_diff=PHOTO_MAX_DIFF):
    """One evaluation at a level: (geometric index [n] (-1 = rejected), r [n], photometric index [n], r_I [n], terms [n,2,32]).
    prev / cur: a level of the depth twin's maps; iprev / icur: the same level of ``intensity_maps``."""
    n = level_cam[0] * level_cam[1]
    gi, gr, gterms = OS.rows(T, level_cam, prev, cur, max_dist)
    geo = np.concatenate([gterms, np.where(gi >= 0, 1.0, 0.0)[:, None], np.zeros((n, 2))], 1)
    ok, j, rI, q, g = photo_rows(T, level_cam, prev, cur, iprev, icur, max_dist, photo_weight, photo_max_diff)
    photo = _terms(q, g, float(F32(photo_weight)) * rI, ok, {30: np.ones(n), 31: rI * rI})
    return gi, gr, np.where(ok, j, -1), rI, np.stack([geo, photo], 1)


def _fold(a):
    a = a.copy()
    w = OS.THREADS // 2
    while w > 0:
        a[..., :w, :] = a[..., :w, :] + a[..., w:2 * w, :]
        w //= 2
    return a[..., 0, :]


def reduce_sums(terms):
    """terms [n,2,32] -> sums [32] in the kernel's order."""
    n = terms.shape[0]
    per = OS.THREADS * OS.PER
    parts = max(1, -(-n // per))
    t = np.zeros((parts * per, 2, SUMS))
    t[:n] = terms
    t = t.reshape(parts, OS.PER, OS.THREADS, 2, SUMS)
    acc = np.zeros((parts, OS.THREADS, SUMS))
    for k in range(OS.PER):
        acc = (acc + t[:, k, :, 0]) + t[:, k, :, 1]
    part = _fold(acc)
    m = -(-parts // OS.THREADS)
    t2 = np.zeros((m * OS.THREADS, SUMS))
    t2[:parts] = part
    t2 = t2.reshape(m, OS.THREADS, SUMS)
    acc = np.zeros((OS.THREADS, SUMS))
    for k in range(m):
        acc = acc + t2[k]
    return _fold(acc)


def estimate(maps_prev, maps_cur, cam, levels=3, iters=(10, 5, 4), max_dist=0.25, init=None, photo_weight=PHOTO_WEIGHT, photo_max_diff=PHOTO_MAX_DIFF):
    """The whole estimate on the twin: (T [4,4], status per level, iterations per level).  maps_*: ``frame_maps`` results."""
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    cams = OS.level_intrinsics(cam, levels)
    status, its = [OS.RUNNING] * levels, [0] * levels
    for k, cap in enumerate(iters):
        l = levels - 1 - k
        done, upd = False, 0
        for _ in range(cap):
            if done:
                break
            terms = rows_rgbd(T, cams[l], maps_prev[0][l], maps_cur[0][l], maps_prev[1][l], maps_cur[1][l], max_dist, photo_weight, photo_max_diff)[4]
            T, done, status[l], upd, _, _ = OS.step(reduce_sums(terms)[:OS.SUMS], T, upd, cap)
        its[l] = upd
    return T, status, its


# ---------------------------------------------------------------------------------------------------------------- scenes
def smooth_colours(vertices):
    """float32 [V,3] in 0 .. 1: a smooth function of position with structure at the scale of a metre."""
    v = np.asarray(vertices, np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    c = np.stack([0.5 + 0.25 * np.sin(2.3 * x + 1.1 * y + 0.4) + 0.2 * np.cos(1.7 * z - 0.8 * y),
                  0.5 + 0.25 * np.cos(1.9 * y - 1.3 * z + 0.2) + 0.2 * np.sin(2.9 * x + 0.6 * z),
                  0.5 + 0.25 * np.sin(2.1 * z + 0.9 * x - 0.5) + 0.2 * np.cos(2.6 * y + 1.2 * x)], -1)
    return np.clip(c, 0.0, 1.0).astype(F32)


def drawn_pair(Hh, W, seed):
    """(depth_prev, depth_cur [H,W], colour_prev, colour_cur [H,W,3]) float32: two smooth depth frames around 2 m that differ by a centimetre
    or so (tests/test_gpu_odometry.py's _drawn_pair) and two smooth colour frames that differ by a few hundredths: many rows of both
    kinds under any small T."""
    rs = np.random.RandomState(seed)
    v, u = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    prev = 2.0 + 0.2 * np.sin(0.31 * u + 0.5) * np.cos(0.23 * v) + 0.003 * rs.standard_normal((Hh, W))
    cur = prev + 0.01 * np.cos(0.4 * u - 0.3 * v)
    cp = np.stack([0.5 + 0.3 * np.sin(0.37 * u + 0.2 * k) * np.cos(0.29 * v - 0.4 * k) for k in range(3)], -1)
    cc = cp + 0.02 * np.cos(0.2 * u + 0.3 * v)[..., None]
    return prev.astype(F32), cur.astype(F32), cp.astype(F32), cc.astype(F32)


def wall_in_room():
    """The wall mesh standing in the plane x = 0 of a room: (x, y, 0) -> (0, 2.5 + x, 1.5 + y), coloured by its position there."""
    v, f, _ = wall_mesh()
    r = np.stack([np.zeros(len(v)), 2.5 + v[:, 0], 1.5 + v[:, 1]], -1).astype(F32)
    return r, f, smooth_colours(r)


WALL_CELLS, WALL_SIZE, WALL_DISTANCE =(24, 18), (6.0, 4.5), 1.5


def wall_mesh(cells=WALL_CELLS, size=WALL_SIZE):
    """(vertices float32 [V,3], faces int32 [F,3], colours float32 [V,3]): the plane z = 0, centred on the origin, cells[0] x cells[1] cells."""
    nx, ny = cells
    xs, ys = np.linspace(-size[0] / 2, size[0] / 2, nx + 1), np.linspace(-size[1] / 2, size[1] / 2, ny + 1)
    X, Y = np.meshgrid(xs, ys)
    v = np.stack([X.reshape(-1), Y.reshape(-1), np.zeros(X.size)], -1).astype(F32)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(ny + 1, nx + 1)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, 1:].reshape(-1), idx[1:, :-1].reshape(-1)
    f = np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)]).astype(np.int32)
    return v, f, smooth_colours(v)


def wall_pose(distance=WALL_DISTANCE):
    """The camera at (0, 0, distance) looking along -z, straight at the wall (camera axes = world axes)."""
    p = np.eye(4)
    p[2, 3] = distance
    return p


# the three motions of the wall scene: in-plane; in-plane with a turn about the normal; a general one
WALL_MOTIONS = [OS.relative_motion((0, 0, 1), 0.0, (1.0, 0.4, 0.0), 0.03),
                OS.relative_motion((0, 0, 1), 3.0, (0.7, -0.7, 0.0), 0.05),
                OS.relative_motion((0.3, -0.8, 0.5), 4.0, OS.CASE_ALONG, 0.08)]

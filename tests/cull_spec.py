"""numpy float32 restatement of the mesh-culling contract (naruto_amd/culling.py, csrc/naruto_cull.hip): camera space, the homogeneous
rasteriser, the vertex test, the keep rule and the compaction.  Every operation is a float32 numpy operation in the order the contract
writes it, so the device results are compared with ``==`` on the bits.  A plain loop over the triangles: keep scenes small."""
import numpy as np

F32 = np.float32


def _cam(cam):
    return int(cam["H"]), int(cam["W"]), F32(cam["fx"]), F32(cam["fy"]), F32(cam["cx"]), F32(cam["cy"])


def camera_space(vertices, c2w):
    """q = p - t; x_k = (q0*R0k + q1*R1k) + q2*R2k -> float32 [V,3]; zc = -x[:, 2]."""
    p = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    m = np.asarray(c2w, dtype=F32).reshape(4, 4)
    q = [p[:, k] - m[k, 3] for k in range(3)]
    return np.stack([(q[0] * m[0, k] + q[1] * m[1, k]) + q[2] * m[2, k] for k in range(3)], -1)


def _cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def pixel_box(a, b, c, cam, near):
    """Candidate pixels of a camera-space triangle: (x0, y0, x1, y1) inclusive, or None."""
    H, W, fx, fy, cx, cy = _cam(cam)
    z = [-a[2], -b[2], -c[2]]
    front = [zz > F32(near) for zz in z]
    if not any(front):
        return None
    if not all(front):
        return 0, 0, W - 1, H - 1
    u = [cx + fx * (p[0] / zz) for p, zz in zip((a, b, c), z)]
    v = [cy - fy * (p[1] / zz) for p, zz in zip((a, b, c), z)]
    x0, x1 = max(np.ceil(min(u)) - F32(1), F32(0)), min(np.floor(max(u)) + F32(1), F32(W - 1))
    y0, y1 = max(np.ceil(min(v)) - F32(1), F32(0)), min(np.floor(max(v)) + F32(1), F32(H - 1))
    if not (x0 <= x1 and y0 <= y1):
        return None
    return int(x0), int(y0), int(x1), int(y1)


def triangle_depth(a, b, c, dx, dy, near, far):
    """Depth of the triangle at the rays (dx, dy, -1) (arrays), +inf where it is not hit."""
    e = []
    for p, q in ((a, b), (b, c), (c, a)):
        n = _cross(p, q)
        e.append((dx * n[0] + dy * n[1]) - n[2])
    covered = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
    covered &= ~((e[0] == 0) & (e[1] == 0) & (e[2] == 0))
    n = _cross(b - a, c - a)
    den = (dx * n[0] + dy * n[1]) - n[2]
    num = (a[0] * n[0] + a[1] * n[1]) + a[2] * n[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = num / den
    hit = covered & (den != 0) & (t > F32(near)) & (t < F32(far))
    return np.where(hit, t, F32(np.inf)).astype(F32)


def render_depth(vertices, faces, poses, cam, near=0.01, far=10.0, face_mask=None, use_box=True):
    """float32 [P,H,W], +inf where nothing is hit.  ``use_box=False`` tests every pixel against every triangle."""
    H, W, fx, fy, cx, cy = _cam(cam)
    faces = np.asarray(faces).reshape(-1, 3)
    poses = np.asarray(poses, dtype=F32).reshape(-1, 4, 4)
    dx_all = (np.arange(W, dtype=F32) - cx) / fx
    dy_all = -((np.arange(H, dtype=F32) - cy) / fy)
    out = np.full((len(poses), H, W), np.inf, dtype=F32)
    for k, c2w in enumerate(poses):
        x = camera_space(vertices, c2w)
        for f, (i0, i1, i2) in enumerate(faces):
            if face_mask is not None and not face_mask[f]:
                continue
            a, b, c = x[i0], x[i1], x[i2]
            box = pixel_box(a, b, c, cam, near)
            if box is None:
                continue
            x0, y0, x1, y1 = box if use_box else (0, 0, W - 1, H - 1)
            dx, dy = np.meshgrid(dx_all[x0:x1 + 1], dy_all[y0:y1 + 1])
            t = triangle_depth(a, b, c, dx, dy, near, far)
            out[k, y0:y1 + 1, x0:x1 + 1] = np.minimum(out[k, y0:y1 + 1, x0:x1 + 1], t)
    return out


def vertex_tests(vertices, poses, cam, depth=None, eps=0.03):
    """(in_frustum, observed) bool [P,V]; ``depth`` float32 [P,H,W] with +inf where nothing occludes, or None (observed = in frustum)."""
    H, W, fx, fy, cx, cy = _cam(cam)
    poses = np.asarray(poses, dtype=F32).reshape(-1, 4, 4)
    fr, ob = [], []
    for k, c2w in enumerate(poses):
        x = camera_space(vertices, c2w)
        zc = -x[:, 2]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = (fx * x[:, 0]) / zc + cx
            v = cy - (fy * x[:, 1]) / zc
            i, j = np.floor(u + F32(0.5)), np.floor(v + F32(0.5))
        inside = (zc > 0) & (i >= 0) & (i < W) & (j >= 0) & (j < H)
        seen = inside.copy()
        if depth is not None:
            ii, jj = np.where(inside, i, 0).astype(np.int64), np.where(inside, j, 0).astype(np.int64)
            seen &= zc < depth[k][jj, ii] + F32(eps)
        fr.append(inside)
        ob.append(seen)
    return np.stack(fr), np.stack(ob)


def inside_bounds(vertices, bounds):
    b = np.asarray(bounds, dtype=np.float64).reshape(3, 2)
    v = np.asarray(vertices).reshape(-1, 3)
    return ((v >= b[:, 0]) & (v <= b[:, 1])).all(1)


def compact(vertices, faces, keep, colors=None):
    """Kept faces in their order, the vertices they reference in their order, faces re-indexed, colours carried along."""
    faces = np.asarray(faces).reshape(-1, 3)
    kept = faces[keep]
    used = np.zeros(len(vertices), dtype=bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return np.asarray(vertices)[used], new[kept].reshape(-1, 3), (None if colors is None else np.asarray(colors)[used])


def cull_mesh(vertices, faces, poses, cam, colors=None, bounds=None, remove_occlusion=True, occluder=None, eps=0.03, near=0.01, far=10.0):
    """-> (vertices, faces, colours) of the culled mesh; the tests run on float32(vertices), the output carries the input's own values."""
    faces = np.asarray(faces).reshape(-1, 3)
    alive = np.ones(len(faces), dtype=bool)
    if bounds is not None:
        alive = inside_bounds(vertices, bounds)[faces].any(1)
    depth = None
    if remove_occlusion:
        if occluder is not None:
            depth = render_depth(occluder[0], occluder[1], poses, cam, near, far)
        else:
            depth = render_depth(vertices, faces, poses, cam, near, far, face_mask=alive)
    _, seen = vertex_tests(vertices, poses, cam, depth, eps)
    observed = seen.any(0)
    keep = alive & observed[faces].any(1)
    return compact(vertices, faces, keep, colors)


# ---- scenes shared by tests/test_cull_host.py and tests/test_gpu_cull.py ---------------------------------------------------------------
ROOM_LO, ROOM_HI, ROOM_CENTRE, ROOM_RADIUS = (0.0, 0.0, 0.0), (6.0, 5.0, 3.0), (3.0, 2.5, 1.4), 0.8


def camera(W=80, H=60, f=60.0, cx=None, cy=None):
    return {"H": H, "W": W, "fx": f, "fy": f, "cx": (W - 1) / 2.0 if cx is None else cx, "cy": (H - 1) / 2.0 if cy is None else cy}


def analytic_room():
    """synthetic.AnalyticRoom with the walls and the sphere of synthetic.room_sphere_mesh()."""
    from naruto_amd import synthetic as syn
    room = syn.AnalyticRoom(np.stack([np.array(ROOM_LO) - 0.45, np.array(ROOM_HI) + 0.45], 1), wall_margin=0.45, sphere_radius=ROOM_RADIUS)
    room.centre = np.array(ROOM_CENTRE)
    return room


def ring_poses(n):
    """float32 [n,4,4]: AnalyticRoom's ring cameras inside the room, looking at the sphere."""
    room = analytic_room()
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        pos, R = room.pose(k, n)
        out[k, :3, :3], out[k, :3, 3] = R, pos
    return out.astype(F32)


def room_mesh(n_lat=24, n_lon=48, **kw):
    from naruto_amd import synthetic as syn
    return syn.room_sphere_mesh(n_lat=n_lat, n_lon=n_lon, **kw)


def shadow_scene(flip=False):
    """A 101 x 101-vertex plane [-2.5, 2.5]^2 at depth 3 and a 0.6 x 0.6 two-triangle occluder at depth 1.5, seen by the identity pose:
    (vertices float32 [10205,3], faces int32 [20002,3]); the occluder's four vertices and two faces come last."""
    n = 101
    ax = np.linspace(-2.5, 2.5, n)
    x, y = np.meshgrid(ax, ax)
    plane = np.stack([x.reshape(-1), y.reshape(-1), np.full(n * n, -3.0)], 1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, 1:].reshape(-1), idx[1:, :-1].reshape(-1)
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    occ = np.array([[-0.3, -0.3, -1.5], [0.3, -0.3, -1.5], [0.3, 0.3, -1.5], [-0.3, 0.3, -1.5]])
    of = np.array([[0, 1, 2], [0, 2, 3]]) + n * n
    if flip:
        of = of[:, ::-1]
    return np.concatenate([plane, occ]).astype(F32), np.concatenate([faces, of]).astype(np.int32)

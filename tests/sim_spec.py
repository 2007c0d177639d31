"""numpy float32 restatement of the mesh simulator's contract (naruto_amd/simulator.py, csrc/naruto_sim.hip): the winner raster (the
culling's rasteriser of tests/cull_spec.py plus the face that won), the shade, the cube faces, the panorama gather with its distance
and its two scalars.  Every operation is a float32 numpy operation in the order the contract writes it, so the device results are
compared with ``==`` on the bits.  A plain loop over the triangles: keep scenes small."""
import numpy as np

import cull_spec as CS

F32 = np.float32


def vertex_colours(colors):
    """RGBA8 [V,4] -> byte / 255.0f; float [V,3] -> float32."""
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c.reshape(-1, 4)[:, :3].astype(F32) / F32(255.0)
    return c.reshape(-1, 3).astype(F32)


def render_winner(vertices, faces, poses, cam, near=0.01, far=100.0):
    """(t float32 [P,H,W] with +inf where nothing is hit, face id int32 [P,H,W] with -1 there): the nearest hit; among the faces whose
    depth equals the minimum in every bit, the lowest index (faces are visited in ascending order and only a smaller depth replaces)."""
    H, W, fx, fy, cx, cy = CS._cam(cam)
    faces = np.asarray(faces).reshape(-1, 3)
    poses = np.asarray(poses, dtype=F32).reshape(-1, 4, 4)
    dx_all = (np.arange(W, dtype=F32) - cx) / fx
    dy_all = -((np.arange(H, dtype=F32) - cy) / fy)
    best = np.full((len(poses), H, W), np.inf, dtype=F32)
    fid = np.full((len(poses), H, W), -1, dtype=np.int32)
    for k, c2w in enumerate(poses):
        x = CS.camera_space(vertices, c2w)
        for f, (i0, i1, i2) in enumerate(faces):
            a, b, c = x[i0], x[i1], x[i2]
            box = CS.pixel_box(a, b, c, cam, near)
            if box is None:
                continue
            x0, y0, x1, y1 = box
            dx, dy = np.meshgrid(dx_all[x0:x1 + 1], dy_all[y0:y1 + 1])
            t = CS.triangle_depth(a, b, c, dx, dy, near, far)
            sub_t, sub_f = best[k, y0:y1 + 1, x0:x1 + 1], fid[k, y0:y1 + 1, x0:x1 + 1]
            closer = t < sub_t
            sub_t[closer] = t[closer]
            sub_f[closer] = f
    return best, fid


def shade(vertices, faces, colors, poses, cam, t, fid, keep_inf=False):
    """(depth [P,H,W], colour [P,H,W,3]) from the winner raster: s = (e_ab + e_bc) + e_ca; w_a = e_bc/s, w_b = e_ca/s, w_c = e_ab/s;
    colour_k = (w_a*ca_k + w_b*cb_k) + w_c*cc_k.  Nothing hit: depth 0 (+inf with keep_inf), colour 0."""
    H, W, fx, fy, cx, cy = CS._cam(cam)
    faces = np.asarray(faces).reshape(-1, 3)
    poses = np.asarray(poses, dtype=F32).reshape(-1, 4, 4)
    col = vertex_colours(colors)
    dx, dy = np.meshgrid((np.arange(W, dtype=F32) - cx) / fx, -((np.arange(H, dtype=F32) - cy) / fy))
    depth = np.where(fid >= 0, t, F32(np.inf) if keep_inf else F32(0)).astype(F32)
    out = np.zeros(fid.shape + (3,), dtype=F32)
    for k, c2w in enumerate(poses):
        x = CS.camera_space(vertices, c2w)
        hit = fid[k] >= 0
        tri = faces[np.where(hit, fid[k], 0)]                                   # [H,W,3]
        a, b, c = (tuple(x[tri[..., n], m] for m in range(3)) for n in range(3))
        e = []
        for p, q in ((a, b), (b, c), (c, a)):
            n = CS._cross(p, q)
            e.append((dx * n[0] + dy * n[1]) - n[2])
        s = (e[0] + e[1]) + e[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            wa, wb, wc = e[1] / s, e[2] / s, e[0] / s
        for ch in range(3):
            ca, cb, cc = col[tri[..., 0], ch], col[tri[..., 1], ch], col[tri[..., 2], ch]
            out[k, ..., ch] = np.where(hit, (wa * ca + wb * cb) + wc * cc, F32(0))
    return depth, out


def render_rgbd(vertices, faces, colors, poses, cam, near=0.01, far=100.0, keep_inf=False):
    """-> (depth, colour, face id)."""
    t, fid = render_winner(vertices, faces, poses, cam, near, far)
    depth, colour = shade(vertices, faces, colors, poses, cam, t, fid, keep_inf)
    return depth, colour, fid


def face_rotations():
    """[6,3,3] F R B L U D, columns (right, up, -view) in the camera frame."""
    x, y, z = np.eye(3)
    frames = [(x, y, -z), (z, y, x), (-x, y, z), (-z, y, -x), (x, z, y), (x, -z, -y)]
    return np.stack([np.stack([r, u, -v], 1) for r, u, v in frames])


def cube_poses(c2w):
    """float32 [6,4,4]: c2w @ R_face (the entries of R_face are 0 and +-1: exact)."""
    c2w = np.asarray(c2w, dtype=F32).reshape(4, 4)
    out = np.tile(c2w, (6, 1, 1))
    out[:, :3, :3] = c2w[:3, :3] @ face_rotations().astype(F32)
    return out


def cube_camera(face_w):
    k = (face_w - 1) / 2.0
    return {"H": face_w, "W": face_w, "fx": k, "fy": k, "cx": k, "cy": k}


def ray_norm(dx, dy):
    return np.sqrt((dx * dx + dy * dy) + F32(1))


def erp(vertices, faces, colors, c2w, face_w, table, near=0.01, far=100.0):
    """(erp colour [h,w,3], erp distance [h,w]) through ``table`` [h,w]: dist = t * r, r = sqrt((dx*dx + dy*dy) + 1) at the chosen cube
    pixel; nothing hit: 1e8f * r."""
    cam = cube_camera(face_w)
    depth, colour, fid = render_rgbd(vertices, faces, colors, cube_poses(c2w), cam, near, far)
    src = np.asarray(table).astype(np.int64)
    rem = src % (face_w * face_w)
    cj, ci = rem // face_w, rem % face_w
    c = F32(face_w - 1) / F32(2)
    dx = (ci.astype(F32) - c) / c
    dy = -((cj.astype(F32) - c) / c)
    r = ray_norm(dx, dy)
    t = depth.reshape(-1)[src]
    miss = fid.reshape(-1)[src] < 0
    dist = np.where(miss, F32(1e8) * r, t * r).astype(F32)
    return colour.reshape(-1, 3)[src], dist


def depth_to_dist(depth, fx, fy, cx, cy):
    d = np.asarray(depth, dtype=F32)
    H, W = d.shape[-2:]
    dx, dy = np.meshgrid((np.arange(W, dtype=F32) - F32(cx)) / F32(fx), (np.arange(H, dtype=F32) - F32(cy)) / F32(fy))
    return (d * ray_norm(dx, dy)).astype(F32)


# ---- scenes shared by tests/test_sim_host.py and tests/test_gpu_sim.py ------------------------------------------------------------------
def hashed_rgba(n):
    """uint8 [n,4]: a fixed integer hash per vertex and channel, alpha 255."""
    k = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(4) + np.arange(4, dtype=np.uint64)[None]
    h = (k * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(2 ** 32)
    out = ((h >> np.uint64(13)) % np.uint64(256)).astype(np.uint8)
    out[:, 3] = 255
    return out


BOX_LO, BOX_HI = np.array([-2.0, -1.5, -3.0]), np.array([3.0, 1.0, 2.5])
# one colour per wall, in the order -x, +x, -y, +y, -z, +z
BOX_COLOURS = np.array([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9], [0.9, 0.9, 0.1], [0.1, 0.9, 0.9], [0.9, 0.1, 0.9]], dtype=F32)


def box_scene(missing=None):
    """An axis-aligned box of 12 triangles, every wall with its own four vertices and colour (float colours [V,3]); ``missing``: a wall
    (0..5 = -x, +x, -y, +y, -z, +z) that is left out.  -> (vertices float32 [24,3], faces int32 [F,3], colours float32 [24,3], wall [F])."""
    verts, faces, cols, wall = [], [], [], []
    for axis in range(3):
        o1, o2 = (axis + 1) % 3, (axis + 2) % 3
        for side, bound in enumerate((BOX_LO, BOX_HI)):
            w = 2 * axis + side
            base = len(verts)
            for s1, s2 in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = np.zeros(3)
                p[axis] = bound[axis]
                p[o1] = (BOX_LO, BOX_HI)[s1][o1]
                p[o2] = (BOX_LO, BOX_HI)[s2][o2]
                verts.append(p)
                cols.append(BOX_COLOURS[w])
            if w != missing:
                faces += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
                wall += [w, w]
    return np.array(verts, dtype=F32), np.array(faces, dtype=np.int32), np.array(cols, dtype=F32), np.array(wall)


def box_ray_distance(o, d, missing=None):
    """float64 distance along unit rays o + t d (o inside the box) to the box, and the wall hit; +inf through the missing wall."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ax = np.where(d > 0, (BOX_HI - o) / d, np.where(d < 0, (BOX_LO - o) / d, np.inf))
    axis = np.argmin(t_ax, axis=-1)
    t = np.take_along_axis(t_ax, axis[..., None], -1)[..., 0]
    wall = 2 * axis + (np.take_along_axis(d, axis[..., None], -1)[..., 0] > 0)
    return np.where(wall == missing, np.inf, t), wall


def rotation_yx(yaw, pitch):
    """Rotation about +y by ``yaw`` then about the new x by ``pitch`` (camera-to-world, float64)."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return ry @ rx

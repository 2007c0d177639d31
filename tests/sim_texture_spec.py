"""numpy restatement of the mesh simulator's textures (naruto_amd/simulator.py, csrc/naruto_sim.hip: k_tex_down, k_sim_shade_tex): the
mip chain in integers, the level choice, the three wrap modes, the bilinear tap and the shade with materials, built on sim_spec's winner
raster and -- for faces without a material -- on sim_spec.shade.  Every float operation is a float32 numpy operation in the order the
contract writes it, so the device results are compared with ``==`` on the bits."""
import numpy as np

import cull_spec as CS
import sim_spec as SS

F32 = np.float32
REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = 10497, 33648, 33071
WRAPS = (REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE)


# ---- the mip chain ---------------------------------------------------------------------------------------------------------------------
def n_levels(w, h):
    return 1 + int(np.floor(np.log2(max(w, h))))                 # (exact for integers up to 2^14)


def pyramid(image):
    """uint8 [H,W,4] -> [level 0, level 1, ...]: level l+1 is max(1, w >> 1) x max(1, h >> 1); per channel
    (t(xa,ya) + t(xb,ya) + t(xa,yb) + t(xb,yb) + 2) >> 2 with xa = min(2x, w-1), xb = min(2x+1, w-1), ya and yb likewise."""
    cur = np.asarray(image, dtype=np.uint8)
    assert cur.ndim == 3 and cur.shape[2] == 4
    out = [cur]
    for _ in range(n_levels(cur.shape[1], cur.shape[0]) - 1):
        h, w = cur.shape[:2]
        x, y = np.arange(max(1, w >> 1)), np.arange(max(1, h >> 1))
        xa, xb = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
        ya, yb = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1)
        t = cur.astype(np.uint32)
        cur = ((t[ya][:, xa] + t[ya][:, xb] + t[yb][:, xa] + t[yb][:, xb] + 2) >> 2).astype(np.uint8)
        out.append(cur)
    assert out[-1].shape[:2] == (1, 1)
    return out


def pyramid_buffer(images):
    """-> (bytes uint8 [n_words * 4] of the one buffer of RGBA8 words, desc int32 [n,4] = word offset of level 0, W, H, n_levels)."""
    parts, desc, off = [], [], 0
    for im in images:
        levels = pyramid(im)
        desc.append([off, im.shape[1], im.shape[0], len(levels)])
        for lv in levels:
            parts.append(lv.reshape(-1))
            off += lv.shape[0] * lv.shape[1]
    return np.concatenate(parts), np.array(desc, dtype=np.int32)


# ---- level, wrap, tap ------------------------------------------------------------------------------------------------------------------
def level(rho2, levels):
    """The number of k in 0 .. levels-2 with rho2 > 4^k (float32 comparisons: NaN gives 0, +inf the last level)."""
    rho2 = np.asarray(rho2, dtype=F32)
    out = np.zeros(rho2.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(levels - 1):
            out += rho2 > F32(4.0) ** k
    return out


def wrap(i, n, mode):
    i = np.asarray(i, dtype=np.int64)
    if mode == REPEAT:
        return i % n                                             # (numpy's % takes the divisor's sign: into [0, n))
    if mode == MIRRORED_REPEAT:
        m = i % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if mode == CLAMP_TO_EDGE:
        return np.clip(i, 0, n - 1)
    raise ValueError(mode)


def tap(lv, u, v, wrap_s, wrap_t, seen=None):
    """One bilinear tap of the level ``lv`` uint8 [h,w,4] at float32 uv arrays -> float32 [...,3] (glTF: uv (0, 0) is the corner of the
    first stored row).  ``seen``: a set that receives every wrap mode that met a negative index."""
    h, w = lv.shape[:2]
    u, v = np.asarray(u, dtype=F32), np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = u * F32(w) - F32(0.5), v * F32(h) - F32(0.5)
        ok = (np.abs(x) < F32(2.0 ** 30)) & (np.abs(y) < F32(2.0 ** 30))
        xs, ys = np.where(ok, x, F32(0)), np.where(ok, y, F32(0))
        fx0, fy0 = np.floor(xs), np.floor(ys)
        a, b = (xs - fx0)[..., None], (ys - fy0)[..., None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    if seen is not None and ok.any():
        if (x0[ok] < 0).any():
            seen.add(("s", wrap_s))
        if (y0[ok] < 0).any():
            seen.add(("t", wrap_t))
    xa, xb, ya, yb = wrap(x0, w, wrap_s), wrap(x0 + 1, w, wrap_s), wrap(y0, h, wrap_t), wrap(y0 + 1, h, wrap_t)
    for idx, n in ((xa, w), (xb, w), (ya, h), (yb, h)):
        assert idx.min(initial=0) >= 0 and idx.max(initial=0) < n
    t = lv[..., :3].astype(F32) / F32(255.0)
    t00, t10, t01, t11 = t[ya, xa], t[ya, xb], t[yb, xa], t[yb, xb]
    top = t00 + a * (t10 - t00)
    bot = t01 + a * (t11 - t01)
    c = top + b * (bot - top)
    return np.where(ok[..., None], c, F32(0)).astype(F32)


# ---- the shade ---------------------------------------------------------------------------------------------------------------------------
def _material(m):
    if hasattr(m, "texture"):
        m = (m.texture, m.wrap_s, m.wrap_t, m.factor)
    return int(m[0]), int(m[1]), int(m[2]), np.asarray(m[3], dtype=F32)


def shade_tex(vertices, faces, colors, uv, face_material, materials, textures, poses, cam, t, fid, keep_inf=False, info=None):
    """(depth [P,H,W], colour [P,H,W,3]) from the winner raster.  A face with material -1 (or out of range, or whose material names a
    texture out of range): sim_spec.shade.  A material without a texture: factor.rgb.  A texture: the contract's textured path.
    ``info`` (a dict) receives ``levels``: {(texture, level)} over the hit pixels, and ``negative``: {(axis, wrap mode)} that met a
    negative index."""
    H, W, fx, fy, cx, cy = CS._cam(cam)
    faces = np.asarray(faces).reshape(-1, 3)
    poses = np.asarray(poses, dtype=F32).reshape(-1, 4, 4)
    uv = np.asarray(uv, dtype=F32).reshape(-1, 2)
    face_material = np.asarray(face_material).reshape(-1)
    depth, out = SS.shade(vertices, faces, colors, poses, cam, t, fid, keep_inf)
    out = out.copy()
    chains = [pyramid(im) for im in textures]
    levels_seen, negative = set(), set()
    ii, jj = np.arange(W, dtype=F32), np.arange(H, dtype=F32)
    dx0, dy0 = np.meshgrid((ii - cx) / fx, -((jj - cy) / fy))
    dx1, _ = np.meshgrid(((ii + F32(1)) - cx) / fx, jj)
    _, dy1 = np.meshgrid(ii, -(((jj + F32(1)) - cy) / fy))
    for k, c2w in enumerate(poses):
        x = CS.camera_space(vertices, c2w)
        hit = fid[k] >= 0
        face = np.where(hit, fid[k], 0)
        tri = faces[face]
        mat = np.where(hit, face_material[face], -1)
        a, b, c = (tuple(x[tri[..., n], m] for m in range(3)) for n in range(3))
        normals = [CS._cross(p, q) for p, q in ((a, b), (b, c), (c, a))]

        def bary(dx, dy):
            e = [(dx * n[0] + dy * n[1]) - n[2] for n in normals]
            s = (e[0] + e[1]) + e[2]
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                return e[1] / s, e[2] / s, e[0] / s

        def interpolate(w, ch):
            with np.errstate(invalid="ignore", over="ignore"):
                return (w[0] * uv[tri[..., 0], ch] + w[1] * uv[tri[..., 1], ch]) + w[2] * uv[tri[..., 2], ch]

        w0, wx, wy = bary(dx0, dy0), bary(dx1, dy0), bary(dx0, dy1)
        u, v = interpolate(w0, 0), interpolate(w0, 1)
        u_x, v_x, u_y, v_y = interpolate(wx, 0), interpolate(wx, 1), interpolate(wy, 0), interpolate(wy, 1)
        for mi in np.unique(mat[(mat >= 0) & (mat < len(materials))]):
            tex, wrap_s, wrap_t, factor = _material(materials[mi])
            here = mat == mi
            if tex < 0:
                out[k][here] = factor[:3]
                continue
            if tex >= len(chains):
                continue
            chain = chains[tex]
            H0, W0 = chain[0].shape[:2]
            with np.errstate(invalid="ignore", over="ignore"):
                ax, bx = (u_x - u) * F32(W0), (v_x - v) * F32(H0)
                ay, by = (u_y - u) * F32(W0), (v_y - v) * F32(H0)
                rx, ry = ax * ax + bx * bx, ay * ay + by * by
                rho2 = np.where(ry > rx, ry, rx)
            lvl = level(rho2, len(chain))
            for l in np.unique(lvl[here]):
                sel = here & (lvl == l)
                levels_seen.add((tex, int(l)))
                with np.errstate(invalid="ignore", over="ignore"):
                    out[k][sel] = tap(chain[l], u[sel], v[sel], wrap_s, wrap_t, negative) * factor[:3]
    if info is not None:
        info["levels"], info["negative"] = levels_seen, negative
    return depth, out


def render_rgbd_tex(mesh, poses, cam, near=0.01, far=100.0, keep_inf=False, info=None):
    """``mesh``: anything with vertices, faces, vertex_colors, uv, face_material, materials, textures -> (depth, colour, face id)."""
    t, fid = SS.render_winner(mesh.vertices, mesh.faces, poses, cam, near, far)
    colors = mesh.vertex_colors if mesh.vertex_colors is not None else np.full((len(mesh.vertices), 4), 255, dtype=np.uint8)
    depth, colour = shade_tex(mesh.vertices, mesh.faces, colors, mesh.uv, mesh.face_material, mesh.materials, mesh.textures, poses, cam, t, fid, keep_inf, info)
    return depth, colour, fid


def erp_tex(mesh, c2w, face_w, table, near=0.01, far=100.0):
    """sim_spec.erp with the textured shade on the six cube faces: (erp colour [h,w,3], erp distance [h,w])."""
    cam = SS.cube_camera(face_w)
    depth, colour, fid = render_rgbd_tex(mesh, SS.cube_poses(c2w), cam, near, far)
    src = np.asarray(table).astype(np.int64)
    rem = src % (face_w * face_w)
    cj, ci = rem // face_w, rem % face_w
    c = F32(face_w - 1) / F32(2)
    dx = (ci.astype(F32) - c) / c
    dy = -((cj.astype(F32) - c) / c)
    r = SS.ray_norm(dx, dy)
    miss = fid.reshape(-1)[src] < 0
    dist = np.where(miss, F32(1e8) * r, depth.reshape(-1)[src] * r).astype(F32)
    return colour.reshape(-1, 3)[src], dist


# ---- the scene shared by the tests ---------------------------------------------------------------------------------------------------------
def hashed_image(h, w, seed):
    """uint8 [h,w,4]: a fixed integer hash per texel and channel."""
    k = (np.arange(h * w * 4, dtype=np.uint64) + np.uint64(seed) * np.uint64(1000003)) * np.uint64(2654435761) + np.uint64(97)
    return (((k % np.uint64(2 ** 32)) >> np.uint64(11)) % np.uint64(256)).astype(np.uint8).reshape(h, w, 4)


class Scene:
    """The fields of naruto_amd.mesh.TexturedMesh, for the restatement alone."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# uv = (corner - 0.5) * scale per wall (-x, +x, -y, +y, -z, +z): below 0 on every textured wall, the scales a factor of 8 apart
BOX_UV_SCALE = (0.125, 1.0, 8.0, 1.0, 1.0, 64.0)
BOX_WALL_MATERIAL = (0, 1, 2, 3, -1, 4)
CAMERA = {"H": 30, "W": 40, "fx": 30.0, "fy": 30.0, "cx": 19.5, "cy": 14.5}


def textured_box():
    """sim_spec.box_scene() seen from inside: three hashed textures (16 x 16, 8 x 4, 5 x 3) on four walls with every wrap mode on each
    axis, a factor-only wall, and a wall without a material over hashed RGBA8 vertex colours."""
    v, f, _, wall = SS.box_scene()
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64)
    uv = np.concatenate([(corner - 0.5) * BOX_UV_SCALE[w] for w in range(6)]).astype(F32)
    materials = [(0, REPEAT, MIRRORED_REPEAT, (1.0, 1.0, 1.0, 1.0)), (1, MIRRORED_REPEAT, CLAMP_TO_EDGE, (0.5, 1.0, 0.75, 1.0)),
                 (2, CLAMP_TO_EDGE, REPEAT, (1.0, 0.25, 1.0, 0.5)), (-1, REPEAT, REPEAT, (0.2, 0.4, 0.6, 1.0)), (0, CLAMP_TO_EDGE, MIRRORED_REPEAT, (0.9, 0.8, 0.7, 1.0))]
    return Scene(vertices=v, faces=f, vertex_colors=SS.hashed_rgba(len(v)), uv=uv, face_material=np.array([BOX_WALL_MATERIAL[w] for w in wall], dtype=np.int32),
                 materials=materials, textures=[hashed_image(16, 16, 1), hashed_image(4, 8, 2), hashed_image(3, 5, 3)], wall=wall)


def box_poses():
    """float32 [3,4,4] inside the box: two views across it and one that grazes the +z wall from 5 cm."""
    out = np.tile(np.eye(4), (3, 1, 1))
    for k, (pos, yaw, pitch) in enumerate((([0.0, 0.0, 0.0], 0.4, -0.2), ([1.0, -0.5, -1.0], -1.3, 0.3), ([0.0, -0.2, 2.45], 1.45, 0.1))):
        out[k, :3, :3], out[k, :3, 3] = SS.rotation_yx(yaw, pitch), pos
    return out.astype(F32)

"""GPU tests of the mesh simulator (naruto_amd/simulator.py -> C ABI -> csrc/naruto_sim.hip and the rasteriser of csrc/naruto_cull.hip)
against the numpy float32 restatement (tests/sim_spec.py): depth, face id, colour and the panorama's distance equal it in every bit,
whatever the launch plan; the gather and the distance conversion equal the reference's recorded results (tests/golden/g13_c2e.npz)."""
import numpy as np
import pytest
import torch

import cull_spec as CS
import sim_spec as SS
from test_sim_host import GOLDEN, SHAPES, affine_colour, oblique_triangle, screen_space_affine

pytestmark = pytest.mark.gpu

FAR = 100.0


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(got, want, what=""):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = a != b
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def room(gpu):
    """room_mesh(8, 16) -- 12 wall triangles, a 224-face sphere and the zero-area face -- with hashed RGBA8 vertex colours from three ring
    poses inside the room at 80 x 60, and the restatement's frames of it (computed once, never written to)."""
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    col = SS.hashed_rgba(len(v))
    poses, cam = CS.ring_poses(3), CS.camera()
    depth, colour, fid = SS.render_rgbd(v, f, col, poses, cam, far=FAR)
    for a in (depth, colour, fid):
        a.setflags(write=False)
    return {"v": v, "f": f, "col": col, "poses": poses, "cam": cam, "depth": depth, "colour": colour, "fid": fid}


def _sim(scene, cam, **kw):
    from naruto_amd import simulator as SIM
    kw.setdefault("erp_hw", (16, 32))
    kw.setdefault("face_w", 16)
    return SIM.MeshSimHIP(scene, cam, far=FAR, **kw)


@pytest.mark.parametrize("threshold", [0, 512, 2 ** 32], ids=["all-large", "default", "all-small"])
@pytest.mark.parametrize("pose_chunk", [1, 3])
def test_frames_equal_the_restatement_in_every_bit(gpu, room, threshold, pose_chunk):
    """Depth, face id and colour, at every route of the rasteriser: the wall triangles reach behind the camera (whole-image candidate
    boxes: the large route at the default threshold), the sphere's triangles take the one-lane route."""
    from naruto_amd import culling as CU
    v, f, poses, cam = room["v"], room["f"], room["poses"], room["cam"]
    px = []
    x = CS.camera_space(v, poses[0])
    for a, b, c in f:
        box = CS.pixel_box(x[a], x[b], x[c], cam, 0.01)
        px.append(0 if box is None else (box[2] - box[0] + 1) * (box[3] - box[1] + 1))
    px = np.array(px)
    assert (px == 80 * 60).sum() >= 6 and ((px > 0) & (px <= 512)).sum() > 50
    sim = _sim((v, f, room["col"]), cam, plan=CU.RasterPlan(threshold))
    color, depth, fid = sim.simulate_batch(poses, pose_chunk=pose_chunk, return_face_id=True)
    assert depth.is_cuda and color.is_cuda and fid.is_cuda
    _same_bits(depth, room["depth"], "depth")
    _same_bits(fid, room["fid"], "face id")
    _same_bits(color, room["colour"], "colour")
    assert (room["fid"] >= 12).sum() > 200 and (room["fid"] < 12).sum() > 200 and (room["fid"] >= 0).all()


def test_culling_depth_render_is_the_same_depth(gpu, room):
    """The 64-bit winner cells and the culling's 32-bit depth cells hold the same minimum."""
    from naruto_amd import culling as CU
    got = CU.render_depth(room["v"], room["f"], room["poses"], room["cam"], far=FAR)
    _same_bits(got, room["depth"], "depth-only render")


def test_tie_rule_lowest_face_index_wins(gpu):
    """The same triangle twice, as faces 0 and 1 with different colours: every covered pixel has id 0 and face 0's colour; with the
    colours and the vertex order swapped: still id 0.  The rule speaks of depths that are equal in every bit, so the oblique triangle
    has coordinates that are multiples of 1/8: its normal and plane constant are exact in float32 in any vertex order (reversing the
    order negates numerator and denominator exactly), and the test asserts that the two faces alone give the same depth bits -- with
    arbitrary coordinates a reordered face lands an ulp nearer on some pixels and wins them by depth, not by the tie rule."""
    v = np.array([[-0.5, -0.5, -2.0], [0.75, -0.5, -2.5], [0.0, 0.625, -1.5]], dtype=np.float32)
    cam = CS.camera(32, 24, 24.0)
    pose = np.eye(4, dtype=np.float32)
    red, green = [255, 0, 0, 255], [0, 255, 0, 255]
    for faces, cols in (([[0, 1, 2], [3, 4, 5]], [red] * 3 + [green] * 3), ([[0, 1, 2], [3, 4, 5]], [green] * 3 + [red] * 3),
                        ([[2, 1, 0], [3, 4, 5]], [green] * 3 + [red] * 3), ([[0, 1, 2], [5, 4, 3]], [green] * 3 + [red] * 3),
                        ([[3, 4, 5], [0, 1, 2]], [red] * 3 + [green] * 3)):
        v2, f2, col = np.concatenate([v, v]), np.array(faces, dtype=np.int32), np.array(cols, dtype=np.uint8)
        want_d, want_c, want_f = SS.render_rgbd(v2, f2, col, pose[None], cam, far=FAR)
        alone = [SS.render_winner(v2, f2[k:k + 1], pose[None], cam, far=FAR)[0] for k in range(2)]
        assert np.array_equal(alone[0].view(np.uint32), alone[1].view(np.uint32))            # a tie in every bit, on every pixel
        color, depth, fid = _sim((v2, f2, col), cam).simulate_batch(pose[None], return_face_id=True)
        fid = _np(fid)
        covered = fid >= 0
        assert covered.sum() > 40 and np.all(fid[covered] == 0), np.unique(fid)
        _same_bits(fid, want_f)
        _same_bits(depth, want_d)
        _same_bits(color, want_c)
        first = np.array(cols[faces[0][0]][:3], dtype=np.float32) / 255
        assert np.abs(_np(color)[covered] - first).max() <= 4e-7


def test_misses_and_a_degenerate_triangle(gpu):
    """One small triangle in a 16 x 12 image: uncovered pixels have depth 0, colour 0 and id -1 (+inf in the depth with the flag set); a
    degenerate triangle writes nothing."""
    v = np.array([[0.0, 0.0, -2.0], [0.5, 0.0, -2.0], [0.0, 0.5, -2.0], [-0.3, -0.3, -1.0], [0.3, 0.3, -1.0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [3, 3, 4], [3, 4, 4]], dtype=np.int32)
    col = SS.hashed_rgba(len(v))
    cam = CS.camera(16, 12, 12.0)
    pose = np.eye(4, dtype=np.float32)[None]
    want_d, want_c, want_f = SS.render_rgbd(v, f, col, pose, cam, far=FAR)
    sim = _sim((v, f, col), cam)
    color, depth, fid = (_np(t) for t in sim.simulate_batch(pose, return_face_id=True))
    miss = fid[0] < 0
    assert 0 < (~miss).sum() < 20 and set(np.unique(fid)) == {-1, 0}
    assert np.all(depth[0][miss] == 0) and np.all(color[0][miss] == 0)
    _same_bits(depth, want_d)
    _same_bits(color, want_c)
    _same_bits(fid, want_f)
    # the flag: +inf where nothing is hit, everything else unchanged
    r = sim._raster("pinhole", 1)
    d_inf = torch.empty(1, 12, 16, dtype=torch.float32, device=gpu)
    r.render(torch.from_numpy(pose).to(gpu), depth=d_inf, keep_inf=True)
    d_inf = _np(d_inf)
    assert np.isinf(d_inf[0][miss]).all() and (d_inf[0][miss] > 0).all()
    _same_bits(d_inf[0][~miss], want_d[0][~miss])
    # only the degenerate faces: nothing at all
    color, depth, fid = (_np(t) for t in _sim((v, f[1:], col), cam).simulate_batch(pose, return_face_id=True))
    assert np.all(fid == -1) and np.all(depth == 0) and np.all(color == 0)


def test_colours_are_perspective_correct(gpu):
    """One oblique triangle, depths 1 m to 4 m, float vertex colours affine in position: every covered pixel's colour equals that function
    at t*d within 1e-4 absolute (a dozen fp32 operations on values in [0,1] with metre-scale coordinates).  Screen-space-affine
    interpolation of the same triangle is off by more than 1e-2 somewhere, so the test can tell the two apart."""
    v, f, col = oblique_triangle()
    cam = CS.camera(80, 60, 40.0)
    pose = np.eye(4, dtype=np.float32)[None]
    color, depth, fid = (_np(t)[0] for t in _sim((v, f, col), cam).simulate_batch(pose, return_face_id=True))
    hit = fid >= 0
    assert hit.sum() > 300 and depth[hit].min() < 1.5 and depth[hit].max() > 3.2
    i, j = np.meshgrid(np.arange(80, dtype=np.float64), np.arange(60, dtype=np.float64))
    d = np.stack([(i - cam["cx"]) / cam["fx"], -(j - cam["cy"]) / cam["fy"], -np.ones_like(i)], -1)
    want = affine_colour(depth.astype(np.float64)[..., None] * d)
    err = np.abs(color - want)[hit].max()
    off = np.abs(screen_space_affine(v, col, cam) - want)[hit].max()
    print("perspective-correct error", err, "; screen-space-affine error", off)
    assert off > 1e-2
    assert err <= 1e-4
    want_d, want_c, _ = SS.render_rgbd(v, f, col, pose, cam, far=FAR)
    _same_bits(color, want_c[0])
    _same_bits(depth, want_d[0])


@pytest.mark.parametrize("face_w,h,w", SHAPES)
def test_cube_to_erp_equals_the_reference(gpu, golden, face_w, h, w):
    """A pure gather: every bit of the reference's C2E.forward(mode='nearest') on the recorded random cube, and on the index cube."""
    from naruto_amd import simulator as SIM
    table = SIM.cube_table(face_w, h, w)
    got = SIM.cube_to_erp(torch.from_numpy(golden[f"cube_{face_w}"]), table)
    assert got.is_cuda
    _same_bits(got, golden[f"pano_{face_w}"])
    ids = torch.arange(6 * face_w * face_w, dtype=torch.int32).reshape(1, 6, face_w, face_w)
    _same_bits(SIM.cube_to_erp(ids.to(gpu), torch.from_numpy(table).to(gpu))[0], golden[f"index_{face_w}"])


def test_depth_to_dist_equals_the_reference(gpu, golden):
    """depth2dist with K = 4 on the recorded depths, rtol 1e-6: seven roundings of 2^-24 each, counted on both sides (measured on the host
    against d*sqrt(dx^2+dy^2+1): 1.2e-7); and the restatement in every bit."""
    from naruto_amd import simulator as SIM
    depth, want = golden["depth_8"], golden["dist_8"]
    got = _np(SIM.depth_to_dist(torch.from_numpy(depth), 4.0, 4.0, 4.0, 4.0))
    rel = np.abs(got.astype(np.float64) - want) / want
    print("depth_to_dist vs the reference: worst relative error", rel.max())
    assert rel.max() <= 1e-6
    _same_bits(got, SS.depth_to_dist(depth, 4.0, 4.0, 4.0, 4.0))
    _same_bits(SIM.depth_to_dist(torch.from_numpy(depth[0, :5]).to(gpu), 3.0, 5.0, 1.25, -2.0), SS.depth_to_dist(depth[0, :5], 3.0, 5.0, 1.25, -2.0))


MISSING = 5                                                                      # the +z wall: behind the camera below


def _box_pose():
    c2w = np.eye(4)
    c2w[:3, :3] = SS.rotation_yx(0.4, 0.25)
    c2w[:3, 3] = [0.7, -0.3, 0.4]
    return c2w.astype(np.float32)


@pytest.fixture(scope="module")
def box(gpu):
    """The box with its +z wall removed, an off-centre camera rotated about two axes, face_w = 16, ERP 16 x 32: the simulator's panorama
    and the restatement's (computed once)."""
    from naruto_amd import simulator as SIM
    v, f, col, _ = SS.box_scene(missing=MISSING)
    c2w = _box_pose()
    table = SIM.cube_table(16, 16, 32)
    want_c, want_d = SS.erp(v, f, col, c2w, 16, table, far=FAR)
    sim = _sim((v, f, col), CS.camera(40, 30, 30.0))
    color, depth, erp_color, erp_depth = sim.simulate(c2w, return_erp=True, no_print=True)
    return {"sim": sim, "c2w": c2w, "table": table, "want_c": want_c, "want_d": want_d, "color": color, "depth": depth, "erp_color": erp_color, "erp_depth": erp_depth,
            "scene": (v, f, col)}


def test_panorama_of_a_known_room(gpu, box):
    """erp_depth equals the restatement in every bit; valid pixels equal the box's analytic distance along the chosen cube pixel's world
    ray within 1e-5 m; pixels through the missing wall are >= 1e8; the centre, u = +-pi/2 and the top and bottom rows carry the front,
    right, left, up and down walls' colours -- the orientation contract."""
    from naruto_amd import simulator as SIM
    erp_d, erp_c = _np(box["erp_depth"]), _np(box["erp_color"])
    assert erp_d.shape == (16, 32) and erp_c.shape == (16, 32, 3)
    _same_bits(erp_d, box["want_d"], "erp distance")
    _same_bits(erp_c, box["want_c"], "erp colour")
    # analytic distance along the chosen cube pixel's ray
    c2w = box["c2w"].astype(np.float64)
    table = box["table"].astype(np.int64)
    face, rem = table // 256, table % 256
    d_face = np.stack([(rem % 16 - 7.5) / 7.5, -((rem // 16) - 7.5) / 7.5, -np.ones((16, 32))], -1)
    d_world = np.einsum("ij,hwj->hwi", c2w[:3, :3], np.einsum("hwij,hwj->hwi", SIM.face_rotations()[face], d_face))
    d_world /= np.linalg.norm(d_world, axis=-1, keepdims=True)
    t, wall = SS.box_ray_distance(c2w[:3, 3], d_world, missing=MISSING)
    valid = np.isfinite(t)
    assert 0 < valid.sum() < valid.size
    err = np.abs(erp_d[valid] - t[valid]).max()
    print("panorama distance vs the analytic box: worst", err)
    assert err <= 1e-5
    assert (erp_d[~valid] >= 1e8).all() and (erp_d[valid] < 10).all()
    assert np.abs(erp_c[valid] - SS.BOX_COLOURS[wall[valid]]).max() <= 1e-6 and np.all(erp_c[~valid] == 0)
    # orientation: the camera's -z, +x, -x, +y, -y look at the -z, +x, -x, +y, -y walls (walls 4, 1, 0, 3, 2) under this modest rotation
    for (row, col), cam_dir, w in (((8, 16), [0, 0, -1], 4), ((8, 23), [1, 0, 0], 1), ((8, 8), [-1, 0, 0], 0), ((0, 5), [0, 1, 0], 3), ((0, 27), [0, 1, 0], 3),
                                   ((15, 5), [0, -1, 0], 2), ((15, 27), [0, -1, 0], 2)):
        _, hit = SS.box_ray_distance(c2w[:3, 3], (c2w[:3, :3] @ np.array(cam_dir, dtype=np.float64))[None])
        assert hit[0] == w, (cam_dir, hit)
        assert np.abs(erp_c[row, col] - SS.BOX_COLOURS[w]).max() <= 1e-6, (row, col, erp_c[row, col], w)


def test_collision_probe_equals_the_panorama_scalars(gpu, box):
    """dist_closest and invalid_region_ratio of detect_collision_v2, reduced on the device, equal erp_depth.min() and
    (erp_depth > 1e6).sum() / (h*w) of the same pose exactly; with a wall missing the ratio is strictly between 0 and 1."""
    dist, ratio = box["sim"].collision_probe(box["c2w"])
    erp_d = box["erp_depth"]
    assert isinstance(dist, float) and isinstance(ratio, float)
    assert dist == float(erp_d.min())
    assert ratio == int((erp_d > 1e6).sum()) / (16 * 32)
    assert 0.0 < ratio < 1.0 and 0.5 < dist < 3.0
    d2, r2 = box["sim"].collision_probe(box["c2w"], invalid_thre=dist)         # another threshold: everything above the minimum
    assert d2 == dist and r2 == int((erp_d > dist).sum()) / (16 * 32) and r2 > ratio
    # the closed box: nothing invalid
    v, f, col, _ = SS.box_scene()
    d3, r3 = _sim((v, f, col), CS.camera(40, 30, 30.0)).collision_probe(box["c2w"])
    assert r3 == 0.0 and d3 == dist


def test_simulate_shapes_batches_and_repeatability(gpu, box):
    """Shapes, dtypes and device as documented, for return_erp False and True; simulate_batch equals per-pose calls in every bit; two
    runs are bitwise equal."""
    sim = box["sim"]
    out = sim.simulate(box["c2w"], no_print=True)
    assert len(out) == 2
    for t, shape in zip(out, ((30, 40, 3), (30, 40))):
        assert t.shape == shape and t.dtype == torch.float32 and t.device == gpu and t.is_contiguous()
    for t, shape in zip((box["color"], box["depth"], box["erp_color"], box["erp_depth"]), ((30, 40, 3), (30, 40), (16, 32, 3), (16, 32))):
        assert t.shape == shape and t.dtype == torch.float32 and t.device == gpu
    assert torch.equal(out[0], box["color"]) and torch.equal(out[1], box["depth"])
    poses = np.tile(box["c2w"], (4, 1, 1))
    poses[1, :3, 3] += [0.5, 0.2, -0.7]
    poses[2, :3, :3] = SS.rotation_yx(-2.0, -0.6).astype(np.float32)
    poses[3, :3, :3] = SS.rotation_yx(3.0, 1.2).astype(np.float32)
    batch = sim.simulate_batch(poses, return_erp=True, pose_chunk=3)
    again = sim.simulate_batch(poses, return_erp=True, pose_chunk=12)
    assert [tuple(t.shape) for t in batch] == [(4, 30, 40, 3), (4, 30, 40), (4, 16, 32, 3), (4, 16, 32)]
    for a, b in zip(batch, again):
        _same_bits(a, _np(b))
    for k in range(4):
        single = sim.simulate(poses[k], return_erp=True, no_print=True)
        for a, b in zip(single, batch):
            _same_bits(a, _np(b[k]), f"pose {k}")
    assert float((batch[1] == 0).float().mean()) > 0.01                           # some frames look out through the missing wall


def test_sensor_convention_and_downstream_frames(gpu, room):
    """Back-projecting the pinhole depth along this repository's pixel rays ((i-cx)/fx, -(j-cy)/fy, -1) through c2w lands on the winning
    triangle's plane within 1e-5 m (wall pixels: on the room's wall), so the frame is in the convention keyframe_store / tracking
    consume: float32 [H,W,3] in 0..1 and [H,W] with depth > 0 where something was hit."""
    v, f, poses, cam = room["v"].astype(np.float64), room["f"], room["poses"], room["cam"]
    sim = _sim((room["v"], room["f"], room["col"]), cam)
    i, j = np.meshgrid(np.arange(80, dtype=np.float64), np.arange(60, dtype=np.float64))
    d_cam = np.stack([(i - cam["cx"]) / cam["fx"], -(j - cam["cy"]) / cam["fy"], -np.ones_like(i)], -1)
    worst = 0.0
    for k in range(len(poses)):
        color, depth = sim.simulate(poses[k], no_print=True)
        assert color.shape == (60, 80, 3) and depth.shape == (60, 80) and color.dtype == depth.dtype == torch.float32
        color, depth = _np(color), _np(depth).astype(np.float64)
        assert (depth > 0).all() and color.min() >= 0 and color.max() <= 1 + 1e-6
        c2w = poses[k].astype(np.float64)
        p = (depth[..., None] * d_cam) @ c2w[:3, :3].T + c2w[:3, 3]
        tri = v[f[room["fid"][k]]]                                                  # [H,W,3,3]
        n = np.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        worst = max(worst, np.abs(((p - tri[..., 0, :]) * n).sum(-1)).max())
        walls = room["fid"][k] < 12
        on_wall = np.minimum(np.abs(p - np.array(CS.ROOM_LO)), np.abs(p - np.array(CS.ROOM_HI))).min(-1)
        worst = max(worst, on_wall[walls].max())
    print("back-projected depth vs the surface: worst", worst)
    assert worst <= 1e-5
    # downstream: a keyframe store takes the last frame as it is, and the rays it keeps are pixels of that frame
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    color_t, depth_t = sim.simulate(poses[-1], no_print=True)
    store = KeyFrameStoreHIP({"cam": dict(cam, depth_trunc=100.0)}, 60, 80, num_kf=2, num_rays_to_save=64, device=gpu, seed=3)
    direction = torch.from_numpy(d_cam.astype(np.float32)).to(gpu)
    store.add_keyframe({"direction": direction[None], "rgb": color_t[None], "depth": depth_t[None], "frame_id": 0}, filter_depth=True)
    kept = _np(store.rays[0])
    frame = np.concatenate([d_cam.astype(np.float32), _np(color_t), _np(depth_t)[..., None]], -1).reshape(-1, 7)
    assert len(store) == 1 and kept.shape == (64, 7) and (kept[:, 6] > 0).all()
    assert all((frame == row).all(1).any() for row in kept)

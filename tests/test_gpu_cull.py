"""GPU tests of the mesh-culling path (naruto_amd/culling.py -> C ABI -> csrc/naruto_cull.hip) against the numpy float32 restatement
(tests/cull_spec.py): depth maps, observed masks and culled meshes equal it in every bit and element, whatever the launch plan."""
import numpy as np
import pytest
import torch

import cull_spec as CS
import helpers as H

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_depth(got, want):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float32
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _boxes(v, f, pose, cam):
    """Candidate pixel count of every face under one pose (0: no candidates)."""
    x = CS.camera_space(v, pose)
    out = []
    for a, b, c in f:
        box = CS.pixel_box(x[a], x[b], x[c], cam, 0.01)
        out.append(0 if box is None else (box[2] - box[0] + 1) * (box[3] - box[1] + 1))
    return np.array(out)


@pytest.fixture(scope="module")
def room(gpu):
    """room_sphere_mesh(24, 48) -- 2 221 faces, the zero-area face included -- from four ring poses inside the room at 80 x 60, f = 60, and
    the restatement's depth maps of it (computed once, never written to)."""
    v, f = CS.room_mesh()
    poses, cam = CS.ring_poses(4), CS.camera()
    depth = CS.render_depth(v, f, poses, cam)
    depth.setflags(write=False)
    return {"v": v, "f": f, "poses": poses, "cam": cam, "depth": depth}


def test_depth_maps_equal_the_restatement(gpu, room):
    """Every bit of the four depth maps; 6 - 8 wall triangles per pose reach behind the camera and take the whole-image route, the sphere's
    take the one-lane route.  The public result holds 0 where nothing is hit, the cull's own (keep_inf) +inf."""
    from naruto_amd import culling as CU
    v, f, poses, cam = room["v"], room["f"], room["poses"], room["cam"]
    assert len(f) == 2221
    for k in range(len(poses)):
        px = _boxes(v, f, poses[k], cam)
        whole = int((px == cam["H"] * cam["W"]).sum())
        assert 6 <= whole <= 8 and ((px > 0) & (px <= CU.DEFAULT_LARGE_THRESHOLD)).sum() > 100, (k, whole)
    got = CU.render_depth(v, f, poses, cam, keep_inf=True)
    assert got.is_cuda and got.shape == (4, 60, 80)
    _same_depth(got, room["depth"])
    assert np.isfinite(room["depth"]).all()                                  # a closed room: every pixel is covered
    # far = 2.5 m cuts the far walls away: uncovered pixels come back as 0 / +inf
    want = CS.render_depth(v, f, poses[:1], cam, far=2.5)
    assert np.isinf(want).sum() > 100 and np.isfinite(want).sum() > 100
    _same_depth(CU.render_depth(v, f, poses[:1], cam, far=2.5, keep_inf=True), want)
    _same_depth(CU.render_depth(v, f, poses[:1], cam, far=2.5), np.where(np.isinf(want), np.float32(0), want))


@pytest.mark.parametrize("W,H,f,cx,cy", [(1, 1, 60.0, None, None), (67, 3, 40.0, None, None), (128, 96, 100.0, None, None), (80, 60, 60.0, -20.5, 100.25)],
                         ids=["1x1", "67x3", "128x96", "principal-point-outside"])
def test_depth_maps_at_other_image_shapes(gpu, room, W, H, f, cx, cy):
    from naruto_amd import culling as CU
    cam = CS.camera(W, H, f, cx, cy)
    poses = room["poses"][:2]
    want = CS.render_depth(room["v"], room["f"], poses, cam)
    assert np.isfinite(want).any()
    _same_depth(CU.render_depth(room["v"], room["f"], poses, cam, keep_inf=True), want)


def test_pose_chunks_do_not_matter(gpu, room):
    """P = 5 with pose_chunk = 2 (chunks of 2, 2 and 1), chunk 1 and chunk 8: the same bits, the restatement's."""
    from naruto_amd import culling as CU
    v, f, cam = room["v"], room["f"], room["cam"]
    poses = CS.ring_poses(5)
    want = CS.render_depth(v, f, poses, cam)
    for chunk in (2, 1, 8):
        _same_depth(CU.render_depth(v, f, poses, cam, pose_chunk=chunk, keep_inf=True), want)


def test_the_plan_does_not_matter(gpu, room):
    """Threshold 0 (every triangle through the workgroup route), a threshold above the image (every triangle walked by one lane) and the
    default give the same bits; so do thresholds that put a triangle's box exactly at the threshold and one pixel either side of it."""
    from naruto_amd import culling as CU
    v, f, poses, cam = room["v"], room["f"], room["poses"], room["cam"]
    for plan in (CU.RasterPlan(0), CU.RasterPlan(10 ** 9), None, {"large_threshold": 1}):
        _same_depth(CU.render_depth(v, f, poses, cam, plan=plan, keep_inf=True), room["depth"])
    px = _boxes(v, f, poses[0], cam)
    sizes = np.unique(px[(px > 4) & (px < cam["H"] * cam["W"])])
    n = int(sizes[len(sizes) // 2])                                          # a box size some sphere triangles have under pose 0
    assert (px == n).any()
    for threshold in (n - 1, n, n + 1):
        _same_depth(CU.render_depth(v, f, poses[:1], cam, plan=CU.RasterPlan(threshold), keep_inf=True), room["depth"][:1])
    with pytest.raises(ValueError):
        CU.render_depth(v, f, poses, cam, plan=CU.RasterPlan(-1))


def test_degenerate_triangles_write_nothing(gpu):
    """A triangle wholly behind the camera, one edge-on to it (its plane contains the eye: den = 0 on the pixel column it projects to),
    one beyond far and a zero-area face: none writes a pixel, and the two ordinary triangles between them are drawn as if alone."""
    from naruto_amd import culling as CU
    cam = CS.camera(80, 60, 60.0, cx=40.0, cy=30.0)                          # an integer principal point: column 40 has dx = 0 exactly
    pose = np.eye(4, dtype=np.float32)[None]
    v = np.array([[-0.5, -0.4, -2.0], [0.6, -0.3, -2.5], [0.1, 0.5, -1.5],                       # 0-2   ordinary
                  [-0.9, 0.2, -3.0], [-0.2, 0.4, -3.5], [-0.6, -0.5, -2.2],                      # 3-5   ordinary
                  [-0.5, -0.4, 2.0], [0.6, -0.3, 2.5], [0.1, 0.5, 1.5],                          # 6-8   behind the camera
                  [0.0, -0.5, -2.0], [0.0, 0.5, -2.0], [0.0, 0.0, -3.0],                         # 9-11  in the plane x = 0
                  [-0.5, -0.4, -12.0], [0.6, -0.3, -12.5], [0.1, 0.5, -11.5]], dtype=np.float32)  # 12-14 beyond far = 10
    good = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    full = np.array([[6, 7, 8], [0, 1, 2], [9, 10, 11], [12, 13, 14], [3, 4, 5], [0, 0, 1], [2, 2, 2]], dtype=np.int32)
    want = CS.render_depth(v, good, pose, cam)
    assert 100 < np.isfinite(want).sum() < 2000
    _same_depth(CS.render_depth(v, full, pose, cam), want)                   # the restatement agrees with itself first
    for plan in (None, CU.RasterPlan(0), CU.RasterPlan(10 ** 9)):
        _same_depth(CU.render_depth(v, full, pose, cam, plan=plan, keep_inf=True), want)
        _same_depth(CU.render_depth(v, good, pose, cam, plan=plan, keep_inf=True), want)
        for lone in ([6, 7, 8], [9, 10, 11], [12, 13, 14], [0, 0, 1]):
            alone = CU.render_depth(v, np.array([lone], dtype=np.int32), pose, cam, plan=plan)
            assert not bool(alone.any()), lone


@pytest.mark.parametrize("eps", [0.0, 0.03])
def test_observed_mask_equals_the_restatement(gpu, room, eps):
    """Every element, with and without the occlusion test, all poses at once and pose by pose; the room's vertices (from inside, some are
    behind a camera) plus vertices placed behind the camera and on the rounding boundary: u = -0.5 is pixel 0 (in), u = W - 0.5 is
    pixel W (out)."""
    from naruto_amd import culling as CU
    v, poses, cam, depth = room["v"], room["poses"], room["cam"], room["depth"].copy()
    fr, ob = CS.vertex_tests(v, poses, cam, depth, eps)
    assert 0 < ob.sum() < fr.sum() < fr.size
    assert (CS.camera_space(v, poses[0])[:, 2] > 0).any()                    # behind the first camera
    assert np.array_equal(_np(CU.observed_vertices(v, poses, cam)), fr.any(0))
    assert np.array_equal(_np(CU.observed_vertices(v, poses, cam, depth=depth, eps=eps)), ob.any(0))
    zero_empty = np.where(np.isinf(depth), np.float32(0), depth)             # the public depth convention reads the same
    assert np.array_equal(_np(CU.observed_vertices(torch.from_numpy(v).to(gpu), poses, cam, depth=torch.from_numpy(zero_empty).to(gpu), eps=eps)), ob.any(0))
    for k in range(len(poses)):
        assert np.array_equal(_np(CU.observed_vertices(v, poses[k:k + 1], cam, depth=depth[k:k + 1], eps=eps)), ob[k]), k
    # the boundary, identity pose, fx = 60, cx = 39.5: x = -+2 at depth 3 is u = -0.5 / 79.5 exactly; y likewise with cy = 29.5
    edge = np.array([[-2.0, 0.0, -3.0], [2.0, 0.0, -3.0], [0.0, 1.5, -3.0], [0.0, -1.5, -3.0], [0.0, 0.0, 3.0], [0.0, 0.0, 0.0], [-2.0, 0.0, 3.0],
                     [-2.01, 0.0, -3.0], [1.99, 0.0, -3.0]], dtype=np.float32)
    eye = np.eye(4, dtype=np.float32)[None]
    want, _ = CS.vertex_tests(edge, eye, cam)
    assert want[0].tolist() == [True, False, True, False, False, False, False, False, True]
    assert np.array_equal(_np(CU.observed_vertices(edge, eye, cam)), want[0])


def test_analytic_shadow(gpu):
    """A 101 x 101-vertex plane at depth 3 behind a 0.6 x 0.6 occluder at depth 1.5, identity pose, 128 x 96, f = 100: the occluder's
    shadow on the plane is |x|, |y| < 0.6 and the frustum there |x| < 1.92, |y| < 1.44.  Plane vertices inside 0.55 are not observed,
    those outside 0.65 and inside the frustum less 0.05 all are, those beyond the frustum plus 0.05 are not in the frustum, the
    occluder's own vertices are observed, and the occluder's winding changes nothing."""
    from naruto_amd import culling as CU
    cam, eye = CS.camera(128, 96, 100.0), np.eye(4, dtype=np.float32)[None]
    v, f = CS.shadow_scene()
    ax = np.linspace(-2.5, 2.5, 101)
    x, y = (a.reshape(-1) for a in np.meshgrid(ax, ax))
    m = np.maximum(np.abs(x), np.abs(y))
    shadow = m < 0.55
    lit = (m > 0.65) & (np.abs(x) < 1.92 - 0.05) & (np.abs(y) < 1.44 - 0.05)
    outside = (np.abs(x) > 1.92 + 0.05) | (np.abs(y) > 1.44 + 0.05)
    print("shadow", shadow.sum(), "lit", lit.sum(), "outside", outside.sum())
    assert shadow.sum() == 484 and lit.sum() == 3449 and outside.sum() == 5540
    depth = CU.render_depth(v, f, eye, cam)
    observed = _np(CU.observed_vertices(v, eye, cam, depth=depth))
    frustum = _np(CU.observed_vertices(v, eye, cam))
    plane, occ = slice(0, 101 * 101), slice(101 * 101, None)
    assert not observed[plane][shadow].any()
    assert observed[plane][lit].all()
    assert not frustum[plane][outside].any() and frustum[plane][shadow | lit].all()
    assert observed[occ].all()
    vo, fo = CU.cull_mesh((v, f), eye, cam)
    print("kept", len(fo), "of", len(f), "faces,", len(vo), "vertices")
    assert len(fo) == 8036                                                    # (the restatement's count on the CPU)
    v2, f2 = CS.shadow_scene(flip=True)
    vo2, fo2 = CU.cull_mesh((v2, f2), eye, cam)
    assert torch.equal(vo, vo2) and len(fo) == len(fo2) and torch.equal(fo[:-2], fo2[:-2]) and torch.equal(fo[-2:], fo2[-2:].flip(1))
    assert np.array_equal(_np(CU.render_depth(v2, f2, eye, cam)).view(np.uint32), _np(depth).view(np.uint32))


def _colors(n):
    return (np.arange(n * 4, dtype=np.int64) * 7919 % 256).astype(np.uint8).reshape(n, 4)


def _same_mesh(got, want, colors=True):
    gv, gf = _np(got[0]), _np(got[1])
    assert gv.dtype == want[0].dtype and np.array_equal(gv.view(np.uint8), np.ascontiguousarray(want[0]).view(np.uint8))       # the input's own values, bit for bit
    assert gf.shape == want[1].shape and np.array_equal(gf, want[1])
    if colors:
        assert np.array_equal(_np(got[2]), want[2])


def test_cull_mesh_end_to_end(gpu, room):
    """cull_mesh equals the restatement: faces, vertices, colours, order -- with occlusion and without, with bounds, with an occluder that
    is not the input, from an input nothing observes (an empty mesh), from float64 vertices in a Mesh; and two runs give the same bits."""
    from naruto_amd import culling as CU
    from naruto_amd import mesh as M
    v, f, poses, cam = room["v"], room["f"], room["poses"], room["cam"]
    col = _colors(len(v))
    want = CS.cull_mesh(v, f, poses, cam, colors=col)
    assert 100 < len(want[1]) < len(f) - 100
    got = CU.cull_mesh((v, f, col), poses, cam)
    assert all(t.is_cuda for t in got) and got[1].dtype == torch.int32
    _same_mesh(got, want)
    again = CU.cull_mesh((torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), torch.from_numpy(col).to(gpu)), poses, cam, pose_chunk=3, plan=CU.RasterPlan(0))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    _same_mesh(CU.cull_mesh((v, f), poses, cam, remove_occlusion=False), CS.cull_mesh(v, f, poses, cam, remove_occlusion=False), colors=False)
    _same_mesh(CU.cull_mesh((v, f, col), poses, cam, eps=0.0), CS.cull_mesh(v, f, poses, cam, colors=col, eps=0.0))
    # bounds: half of the sphere and the walls behind it survive step 1; the default occluder is what survived
    bounds = [[2.9, 7.0], [-1.0, 6.0], [-1.0, 4.0]]
    wb = CS.cull_mesh(v, f, poses, cam, colors=col, bounds=bounds)
    assert 50 < len(wb[1]) < len(f) and len(wb[1]) != len(want[1])               # (fewer occluders survive, so more of the rest is seen)
    _same_mesh(CU.cull_mesh((v, f, col), poses, cam, bounds=bounds), wb)
    _same_mesh(CU.cull_mesh((v, f, col), poses, cam, bounds=torch.tensor(bounds), remove_occlusion=False),
               CS.cull_mesh(v, f, poses, cam, colors=col, bounds=bounds, remove_occlusion=False))
    # an occluder that is not the input: a coarser sphere alone, moved by 0.3 m (it hides another part of the input's sphere)
    ov, of = CS.room_mesh(n_lat=12, n_lon=24, centre=(3.3, 2.5, 1.4))
    of = of[12:-1]
    wo = CS.cull_mesh(v, f, poses, cam, colors=col, occluder=(ov, of))
    assert 50 < len(wo[1]) and len(wo[1]) != len(want[1])
    _same_mesh(CU.cull_mesh((v, f, col), poses, cam, occluder=(ov, of)), wo)
    _same_mesh(CU.cull_mesh((v, f, col), poses, cam, occluder=M.Mesh(ov.astype(np.float64), of.astype(np.int64))), wo)
    # nothing observed: the mesh moved behind every camera's back... far outside the room
    away = v + np.float32(100.0)
    ev, ef, ec = CU.cull_mesh((away, f, col), poses, cam)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec.shape == (0, 4) and len(CS.cull_mesh(away, f, poses, cam)[1]) == 0
    # a Mesh in, a Mesh out: float64 vertices that float32 cannot hold come back as they went in
    v64 = v.astype(np.float64) + 1e-9
    out = CU.cull_mesh(M.Mesh(v64, f.astype(np.int64), col), poses, cam)
    w64 = CS.cull_mesh(v64, f, poses, cam, colors=col)
    assert isinstance(out, M.Mesh) and out.vertices.dtype == np.float64 and out.faces.dtype == np.int64
    assert np.array_equal(out.vertices, w64[0]) and np.array_equal(out.faces, w64[1]) and np.array_equal(out.vertex_colors, w64[2])
    empty = CU.cull_mesh(M.Mesh(v64 + 100.0, f.astype(np.int64)), poses, cam)
    assert isinstance(empty, M.Mesh) and empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.vertex_colors is None


def test_command_line(gpu, room, tmp_path):
    """A .ply, a checkpoint and a yaml give the named output file, which python -m naruto_amd.evaluation then scores."""
    import yaml
    from naruto_amd import culling as CU
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    v, f, poses, cam = room["v"], room["f"], room["poses"], room["cam"]
    col = _colors(len(v))
    sc, tr = 2.0, 0.25                                                       # the field's frame is not the mesh's: x_field = (x + tr) * sc
    mesh_path, ckpt, cfg_path = tmp_path / "mesh_final.ply", tmp_path / "ckpt.pt", tmp_path / "scene.yaml"
    M.Mesh(v.astype(np.float64), f.astype(np.int64), col).export(str(mesh_path))
    field_poses = torch.from_numpy(poses).clone()
    field_poses[:, :3, 3] = (field_poses[:, :3, 3] + tr) * sc
    torch.save({"pose": {5 * k: field_poses[k] for k in range(len(poses))}}, ckpt)
    bound = [[(lo + tr) * sc, (hi + tr) * sc] for lo, hi in ([2.9, 7.0], [-1.0, 6.0], [-1.0, 4.0])]
    cfg_path.write_text(yaml.safe_dump({"cam": cam, "data": {"sc_factor": sc, "translation": tr}, "mapping": {"marching_cubes_bound": bound}}))
    metric_poses, metric_bound = CU.to_metric({"data": {"sc_factor": sc, "translation": tr}}, field_poses, bound)
    for flag in (True, False):
        out = CU.main(["--config", str(cfg_path), "--input_mesh", str(mesh_path), "--ckpt_path", str(ckpt)] + (["--remove_occlusion"] if flag else []))
        assert out == str(tmp_path / ("mesh_final_cull_occlusion.ply" if flag else "mesh_final_cull_frustum.ply"))
        got = M.load_ply(out)
        want = CS.cull_mesh(v, f, metric_poses.numpy(), cam, colors=col, bounds=metric_bound.numpy(), remove_occlusion=flag)
        assert len(want[1]) > 50
        assert np.array_equal(got.vertices.astype(np.float32), want[0]) and np.array_equal(got.faces, want[1]) and np.array_equal(got.vertex_colors, want[2])
    gt_path = tmp_path / "gt.ply"
    M.Mesh(v.astype(np.float64), f[12:-1].astype(np.int64)).export(str(gt_path))                  # the sphere alone
    res = E.main(["--rec_mesh", str(tmp_path / "mesh_final_cull_occlusion.ply"), "--gt_mesh", str(gt_path), "--result_txt", str(tmp_path / "res.txt")])
    assert res["accuracy_cm"] < 1.0 and 1.0 < res["completion_ratio_pct"] < 99.0                  # a part of the sphere, on it: sample spacing only
    assert (tmp_path / "res.txt").read_text().count("\n") == 3


def test_evaluator_hook(gpu):
    """evaluate_field(cull_poses=...) equals evaluate_mesh on cull_mesh of the extracted surface, bit for bit; without poses it equals
    evaluate_mesh on the extracted surface, as before."""
    from naruto_amd import culling as CU
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    g = H.load_golden("g10_extract_mesh")
    cfg = H.office_cfg(int(g["hash_size"]))
    cfg["data"]["sc_factor"], cfg["data"]["translation"] = float(g["sc_factor"]), float(g["translation"])
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights={k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")}).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    mcb, voxel = torch.from_numpy(g["mcb"]), float(g["voxel"])
    ev = E.ReconEvaluatorHIP((g["color_vertices"], g["faces"]), n_samples=50000, device=gpu)
    with torch.no_grad():
        vertices, triangles = M.extract_surface(m.query_sdf, cfg, m.bounding_box, mcb, voxel_size=voxel)
    # two cameras at the surface's centroid looking along -+x: each sees a part of the surface from inside it
    c = _np(vertices.mean(0))
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    poses[:, :3, 3] = c
    poses[0, :3, :3] = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.float32)             # columns: right = +y, up = +z, back = +x
    poses[1, :3, :3] = np.array([[0, 0, -1], [-1, 0, 0], [0, 1, 0]], dtype=np.float32)
    cam = CS.camera(80, 60, 60.0)
    cv, cf = CU.cull_mesh((vertices, triangles), poses, cam)
    print("evaluator hook: kept", len(cf), "of", len(triangles), "faces")
    assert 0 < len(cf) < len(triangles)
    want = ev.evaluate_mesh(cv, cf)
    got = ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb, cull_poses=poses, cull_cam=cam)
    plain = ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb)
    unculled = ev.evaluate_mesh(vertices, triangles)
    assert set(got) == set(plain) == {"accuracy_cm", "completion_cm", "completion_ratio_pct", "mad_cm"} and got["mad_cm"] == plain["mad_cm"]
    for k in want:
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (k, got[k], want[k])
        assert np.float64(plain[k]).view(np.uint64) == np.float64(unculled[k]).view(np.uint64), (k, plain[k], unculled[k])
    with pytest.raises(ValueError):
        ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb, cull_poses=poses)

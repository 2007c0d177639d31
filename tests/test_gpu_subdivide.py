"""GPU tests of the subdivision path (naruto_amd/remesh.py -> C ABI -> csrc/naruto_subdiv.hip) and of culling with it
(naruto_amd/culling.py, max_edge=) against the numpy restatements tests/subdivide_spec.py and tests/cull_spec.py: vertices, faces and
colours equal them in every bit, whatever the launch plan; the scenes are the culling tests' own."""
import numpy as np
import pytest
import torch

import cull_spec as CS
import helpers as H
import subdivide_spec as SD

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _colors(n):
    return (np.arange(n * 4, dtype=np.int64) * 7919 % 256).astype(np.uint8).reshape(n, 4)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_mesh(got, want, colors=True):
    gv, gf = _np(got[0]), _np(got[1])
    assert gv.dtype == want[0].dtype and gv.shape == want[0].shape and np.array_equal(_raw(gv), _raw(want[0]))      # NaN included: the bits
    assert gf.dtype == np.int32 and gf.shape == want[1].shape and np.array_equal(gf, want[1])
    if colors:
        assert np.array_equal(_np(got[2]), want[2])


def small_scenes():
    """(name, vertices float64, faces, max_edge): the single triangle, the shared-edge pair, the long/short pair (a T-junction), a pair
    with a NaN vertex, and a face with a repeated vertex."""
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    square = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    pair = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 3.0, 0.0], [0.25, -0.4, 0.0]])
    nan = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [np.nan, 5.0, 0.0], [0.0, 2.0, 0.0]])
    return [("triangle", tri, np.array([[0, 1, 2]]), 0.3),
            ("triangle-exact", np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]]), 1.25),
            ("shared-edge", square, np.array([[0, 1, 2], [0, 2, 3]]), 0.8),
            ("long-short", pair, np.array([[1, 0, 3], [0, 1, 2]]), 0.6),
            ("nan", nan, np.array([[0, 1, 2], [0, 1, 3]]), 0.8),
            ("repeated-vertex", tri, np.array([[0, 0, 1], [2, 1, 0]]), 0.4)]


@pytest.mark.parametrize("colors", [False, True], ids=["plain", "colours"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_subdivision_equals_the_restatement(gpu, dtype, colors):
    """Vertices, faces, colours, generations and remainder, bit for bit: the small scenes (also cut short by max_iter = 1), and the room at
    0.25 (the sphere untouched), 0.1 and 0.12 (split and unsplit sphere faces side by side: T-junctions)."""
    from naruto_amd import remesh as RM
    rv, rf = CS.room_mesh()
    scenes = small_scenes() + [("room-0.25", rv, rf, 0.25), ("room-0.1", rv, rf, 0.1), ("room-0.12", rv, rf, 0.12)]
    for name, v, f, max_edge in scenes:
        v, f = v.astype(dtype), f.astype(np.int32)
        col = _colors(len(v)) if colors else None
        for max_iter in ((1, 10) if len(f) < 10 else (10,)):                  # (the full run last: `want` below is its result)
            want = SD.subdivide_to_size(v, f, max_edge, col, max_iter=max_iter)
            got, res = RM.subdivide_to_size((v, f, col) if colors else (v, f), max_edge, max_iter=max_iter)
            assert len(got) == (3 if colors else 2) and all(t.is_cuda for t in got), name
            print(name, dtype.__name__, "max_iter", max_iter, "->", res, len(want[1]), "faces", len(want[0]), "vertices")
            assert (res.generations, res.remaining_long) == (want[3], want[4]), name
            _same_mesh(got, want, colors)
            assert np.array_equal(_raw(_np(got[0])[:len(v)]), _raw(v)), name                     # the input's vertices are a prefix
        if name == "room-0.25":
            assert (want[3], want[4], len(want[1]), len(want[0])) == (5, 0, 14497, 7252)
            assert np.array_equal(want[1][:len(rf) - 12], rf[12:])
        if name == "room-0.1":
            assert (want[3], want[4], len(want[1]), len(want[0])) == (7, 0, 156292, 78405)
        if name == "room-0.12":
            first = SD.long_faces(v, f, max_edge)[12:-1]
            assert first.any() and not first.all()
        if name == "shared-edge":
            assert (want[3], want[4], len(want[1]), len(want[0])) == (1, 0, 8, 9)                # the shared midpoint exists once
        if name == "long-short":
            assert np.array_equal(want[1][0], f[0]) and want[4] == 0                             # the short face's row: untouched
        if name == "nan":
            assert np.array_equal(want[1][0], f[0]) and np.isnan(want[0][2, 0])
        if name == "triangle-exact":
            assert want[3] == 0 and len(want[1]) == 1


def test_reproducible_and_independent_of_the_plan(gpu):
    """Two runs give the same bits; so does every size of the edge table, from exactly half full to 50 cells per slot; a Mesh in gives a
    Mesh out with the same numbers; max_faces is refused with the predicted count."""
    from naruto_amd import mesh as M
    from naruto_amd import remesh as RM
    v, f = CS.room_mesh()
    col = _colors(len(v))
    dev = tuple(torch.from_numpy(a).to(gpu) for a in (v, f, col))
    first, res = RM.subdivide_to_size(dev, 0.12)
    assert res.remaining_long == 0 and res.generations >= 5
    for plan in (None, RM.SubdividePlan(2.0), RM.SubdividePlan(2.5), {"table_factor": 50}):
        again, res2 = RM.subdivide_to_size((v, f, col), 0.12, plan=plan)
        assert res2 == res and all(torch.equal(a, b) for a, b in zip(first, again)), plan
    assert torch.equal(dev[0], torch.from_numpy(v).to(gpu)) and torch.equal(dev[1], torch.from_numpy(f).to(gpu))     # the input is left alone
    out, res3 = RM.subdivide_to_size(M.Mesh(v.astype(np.float64), f.astype(np.int64), col), 0.12)
    assert isinstance(out, M.Mesh) and res3 == res and out.vertices.dtype == np.float64 and out.faces.dtype == np.int64
    want = SD.subdivide_to_size(v.astype(np.float64), f, 0.12, col)
    assert np.array_equal(out.vertices, want[0]) and np.array_equal(out.faces, want[1]) and np.array_equal(out.vertex_colors, want[2])
    with pytest.raises(ValueError, match=f"{len(f) + 36} faces"):
        RM.subdivide_to_size((v, f), 0.25, max_faces=len(f) + 35)
    part, res4 = RM.subdivide_to_size((v, f), 0.25, max_iter=2)
    assert res4.generations == 2 and res4.remaining_long == 12 * 16 and len(part[1]) == len(f) - 12 + 12 * 16


def _wall_faces(v, f):
    """Faces whose three vertices lie on the room's box (midpoints of wall edges stay on it exactly)."""
    v = np.asarray(v, dtype=np.float64)
    on_box = ((v == np.array(CS.ROOM_LO)) | (v == np.array(CS.ROOM_HI))).any(1)
    return on_box[f].all(1)


@pytest.fixture(scope="module")
def room_cull(gpu):
    """The room from four ring poses at 80 x 60 and the restatement's depth maps of the INPUT mesh, without bounds and with the bounds'
    face mask (computed once, never written to)."""
    v, f = CS.room_mesh()
    poses, cam = CS.ring_poses(4), CS.camera()
    bounds = [[2.9, 7.0], [-1.0, 6.0], [-1.0, 4.0]]
    depth = CS.render_depth(v, f, poses, cam)
    depth_b = CS.render_depth(v, f, poses, cam, face_mask=CS.inside_bounds(v, bounds)[f].any(1))
    depth.setflags(write=False)
    depth_b.setflags(write=False)
    sub = SD.subdivide_to_size(v, f, 0.25, _colors(len(v)))
    return {"v": v, "f": f, "poses": poses, "cam": cam, "bounds": bounds, "depth": depth, "depth_b": depth_b, "sub": sub}


def _restated_cull(room, bounds, remove_occlusion):
    """subdivide_spec -> render_depth of the ORIGINAL mesh -> vertex_tests on the subdivided vertices -> keep rule -> compact."""
    sv, sf, sc, _, _ = room["sub"]
    depth = (room["depth_b"] if bounds is not None else room["depth"]) if remove_occlusion else None
    alive = np.ones(len(sf), dtype=bool) if bounds is None else CS.inside_bounds(sv, bounds)[sf].any(1)
    _, seen = CS.vertex_tests(sv, room["poses"], room["cam"], depth, 0.03)
    return CS.compact(sv, sf, alive & seen.any(0)[sf].any(1), sc)


@pytest.mark.parametrize("remove_occlusion", [True, False], ids=["occlusion", "frustum"])
@pytest.mark.parametrize("with_bounds", [False, True], ids=["unbounded", "bounds"])
def test_cull_with_subdivision_equals_its_restatement(gpu, room_cull, monkeypatch, with_bounds, remove_occlusion):
    """Every bit of the subdivided, culled mesh; the depth maps it used are render_depth of the input mesh, bit for bit; without
    max_edge no wall face survives the occlusion test (1 632 do at 0.25 without bounds), and more than the 12 walls stay in every mode."""
    from naruto_amd import culling as CU
    r = room_cull
    v, f, poses, cam = r["v"], r["f"], r["poses"], r["cam"]
    col = _colors(len(v))
    bounds = r["bounds"] if with_bounds else None
    used = []
    render = CU._Raster.render

    def spy(self, part, out):
        render(self, part, out)
        used.append(out.clone())

    monkeypatch.setattr(CU._Raster, "render", spy)
    got = CU.cull_mesh((v, f, col), poses, cam, bounds=bounds, remove_occlusion=remove_occlusion, max_edge=0.25)
    want = _restated_cull(r, bounds, remove_occlusion)
    print("kept", len(want[1]), "of", len(r["sub"][1]), "faces; wall faces kept", int(_wall_faces(want[0], want[1]).sum()))
    assert 100 < len(want[1]) < len(r["sub"][1])
    _same_mesh(got, want)
    if remove_occlusion:
        depth = _np(torch.cat(used))
        ref = r["depth_b"] if with_bounds else r["depth"]
        assert depth.shape == ref.shape and np.array_equal(depth.view(np.uint32), ref.view(np.uint32))
    else:
        assert not used
    plain = CU.cull_mesh((v, f, col), poses, cam, bounds=bounds, remove_occlusion=remove_occlusion)
    if remove_occlusion:                                                      # (by the frustum alone some wall corners are seen: 12 and 10 walls stay)
        assert _wall_faces(_np(plain[0]), _np(plain[1])).sum() == 0
    assert _wall_faces(_np(got[0]), _np(got[1])).sum() > 12
    if not remove_occlusion:                                                  # (no depth render: cheap) the restatement in one call says the same
        whole, _, gens, rem = SD.cull_subdivided(v, f, poses, cam, 0.25, col, bounds, False)
        assert (gens, rem) == (5, 0) and all(np.array_equal(a, b) for a, b in zip(whole, want))


def plane_scene():
    """Two triangles for [-2.5, 2.5]^2 at depth 3 and the 0.6 x 0.6 two-triangle occluder at depth 1.5 (cull_spec.shadow_scene's, with a
    plane of large faces)."""
    plane = np.array([[-2.5, -2.5, -3.0], [2.5, -2.5, -3.0], [2.5, 2.5, -3.0], [-2.5, 2.5, -3.0]])
    occ = np.array([[-0.3, -0.3, -1.5], [0.3, -0.3, -1.5], [0.3, 0.3, -1.5], [-0.3, 0.3, -1.5]])
    return np.concatenate([plane, occ]).astype(np.float32), np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)


def plane_classes(sv, sf):
    """Of the subdivided plane scene: (plane faces wholly inside the shadow less a pixel, plane faces with a lit vertex inside the frustum
    less a pixel, plane faces wholly outside the frustum plus a pixel, occluder faces).  The shadow's edge is |x|, |y| = 0.6 and the
    frustum's |x| = 2, |y| = 1.5 (80 x 60, f = 60, depth 3); a pixel's footprint at depth 3 is 3 / 60 = 0.05."""
    x, y, z = np.abs(sv[:, 0].astype(np.float64)), np.abs(sv[:, 1].astype(np.float64)), sv[:, 2]
    plane, occ = (z == -3.0)[sf].all(1), (z == -1.5)[sf].all(1)
    shadow = plane & ((x < 0.55) & (y < 0.55))[sf].all(1)
    lit = plane & (((x > 0.65) | (y > 0.65)) & (x < 1.9) & (y < 1.4))[sf].any(1)
    outside = plane & ((x > 2.05) | (y > 1.55))[sf].all(1)
    return shadow, lit, outside, occ


def test_analytic_shadow_on_a_coarse_plane(gpu):
    """A plane of two triangles cannot be culled by its corners (all four are outside the frustum: nothing of it survives); subdivided
    to 0.1 its culled border follows the occluder's shadow and the frustum to within one pixel's footprint."""
    from naruto_amd import culling as CU
    from naruto_amd import remesh as RM
    v, f = plane_scene()
    cam, eye = CS.camera(), np.eye(4, dtype=np.float32)[None]
    coarse = CU.cull_mesh((v, f), eye, cam)
    assert len(coarse[1]) == 2 and float(coarse[0][:, 2].max()) == -1.5       # the occluder alone: the plane is gone
    (sv, sf), res = RM.subdivide_to_size((v, f), 0.1)
    assert (res.generations, res.remaining_long, len(sf), len(sv)) == (7, 0, 33280, 16930)
    sv, sf = _np(sv), _np(sf)
    shadow, lit, outside, occ = plane_classes(sv, sf)
    print("shadow", shadow.sum(), "lit", lit.sum(), "outside", outside.sum(), "occluder", occ.sum())
    assert (shadow.sum(), lit.sum(), outside.sum(), occ.sum()) == (1568, 12062, 15810, 512)
    cv, cf = (_np(t) for t in CU.cull_mesh((v, f), eye, cam, max_edge=0.1))
    kept_shadow, kept_lit, kept_outside, kept_occ = plane_classes(cv, cf)
    print("kept: shadow", kept_shadow.sum(), "lit", kept_lit.sum(), "outside", kept_outside.sum(), "occluder", kept_occ.sum(), "of", len(cf))
    assert kept_shadow.sum() == 0 and kept_outside.sum() == 0
    assert kept_lit.sum() == 12062 and kept_occ.sum() == 512


def test_command_line_and_evaluator(gpu, room_cull, tmp_path, capsys):
    """--max_edge writes the file cull_mesh(max_edge=) returns and prints the generations; evaluate_field forwards max_edge."""
    import yaml
    from naruto_amd import culling as CU
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    r = room_cull
    v, f, poses, cam = r["v"], r["f"], r["poses"], r["cam"]
    col = _colors(len(v))
    mesh_path, ckpt, cfg_path = tmp_path / "mesh_final.ply", tmp_path / "ckpt.pt", tmp_path / "scene.yaml"
    M.Mesh(v.astype(np.float64), f.astype(np.int64), col).export(str(mesh_path))
    torch.save({"pose": {5 * k: torch.from_numpy(poses[k]) for k in range(len(poses))}}, ckpt)
    cfg_path.write_text(yaml.safe_dump({"cam": cam, "data": {"sc_factor": 1.0, "translation": 0.0}}))
    args = ["--config", str(cfg_path), "--input_mesh", str(mesh_path), "--ckpt_path", str(ckpt), "--remove_occlusion"]
    out = CU.main(args + ["--max_edge", "0.25"])
    line = capsys.readouterr().out
    assert out == str(tmp_path / "mesh_final_cull_occlusion.ply") and "5 generations" in line and "still longer" not in line
    got = M.load_ply(out)
    want = CU.cull_mesh(M.Mesh(v.astype(np.float64), f.astype(np.int64), col), poses, cam, max_edge=0.25)
    spec = _restated_cull(r, None, True)
    assert np.array_equal(got.vertices, want.vertices) and np.array_equal(got.faces, want.faces) and np.array_equal(got.vertex_colors, want.vertex_colors)
    assert np.array_equal(got.vertices.astype(np.float32), spec[0]) and np.array_equal(got.faces, spec[1]) and np.array_equal(got.vertex_colors, spec[2])
    CU.main(args + ["--max_edge", "0.25", "--max_iter", "2"])
    line = capsys.readouterr().out
    assert "2 generations" in line and "192 faces still longer" in line
    CU.main(args)
    assert "generations" not in capsys.readouterr().out
    # the evaluator: the extracted surface culled with and without the subdivision
    g = H.load_golden("g10_extract_mesh")
    cfg = H.office_cfg(int(g["hash_size"]))
    cfg["data"]["sc_factor"], cfg["data"]["translation"] = float(g["sc_factor"]), float(g["translation"])
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights={k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")}).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    mcb, voxel = torch.from_numpy(g["mcb"]), float(g["voxel"])
    ev = E.ReconEvaluatorHIP((g["color_vertices"], g["faces"]), n_samples=50000, device=gpu)
    with torch.no_grad():
        vertices, triangles = M.extract_surface(m.query_sdf, cfg, m.bounding_box, mcb, voxel_size=voxel)
    c = _np(vertices.mean(0))
    eposes = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    eposes[:, :3, 3] = c
    eposes[0, :3, :3] = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    eposes[1, :3, :3] = np.array([[0, 0, -1], [-1, 0, 0], [0, 1, 0]], dtype=np.float32)
    edge = (vertices[triangles[:, 1].long()] - vertices[triangles[:, 0].long()]).norm(dim=1)
    max_edge = float(edge.median()) * 0.5                                     # half a typical edge of the extracted surface: most faces are split
    plain = ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb, cull_poses=eposes, cull_cam=cam)
    fine = ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb, cull_poses=eposes, cull_cam=cam, max_edge=max_edge)
    cv, cf = CU.cull_mesh((vertices, triangles), eposes, cam, max_edge=max_edge)
    want = ev.evaluate_mesh(cv, cf)
    print("evaluator:", plain, fine)
    assert set(fine) == set(plain) and any(fine[k] != plain[k] for k in ("accuracy_cm", "completion_cm", "completion_ratio_pct"))
    for k in want:
        assert np.float64(fine[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (k, fine[k], want[k])

"""CPU tests of the reconstruction-metric path: the numpy restatement against scipy's cKDTree, the PLY reader, the C ABI's argument
validation, the command line and the degenerate-mesh definitions.  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import recon_spec as RS


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_restatement_equals_ckdtree_on_uniform_points():
    """20 000 x 20 000 seeded float32 points, uniform in a 4 m box: the fp64 formula d2 = (dx*dx + dy*dy) + dz*dz, minimum, sqrt gives
    cKDTree.query's distances in every bit and, there being no ties, its indices."""
    from scipy.spatial import cKDTree
    rs = np.random.RandomState(11)
    t = rs.uniform(0.0, 4.0, (20000, 3)).astype(np.float32)
    q = rs.uniform(0.0, 4.0, (20000, 3)).astype(np.float32)
    d, i = RS.nearest(q, t)
    dk, ik = cKDTree(t).query(q)
    assert np.array_equal(_bits(d), _bits(dk))
    assert np.array_equal(i, ik)


def lattice_clouds():
    rs = np.random.RandomState(12)
    t = (rs.randint(0, 33, (20000, 3)) / 8.0).astype(np.float32)
    q = (rs.randint(0, 33, (20000, 3)) / 8.0).astype(np.float32)
    return q, t


def test_restatement_equals_ckdtree_on_a_lattice_full_of_ties():
    """Points on a 1/8 m lattice (duplicates and equidistant neighbours everywhere): distances still equal cKDTree's in every bit; the
    restatement's index is the LOWEST among the targets at that distance, whatever cKDTree picked."""
    from scipy.spatial import cKDTree
    q, t = lattice_clouds()
    d, i = RS.nearest(q, t)
    dk, ik = cKDTree(t).query(q)
    assert np.array_equal(_bits(d), _bits(dk))
    assert (i != ik).mean() > 0.05                     # the input does tie
    # lowest index: no target with a smaller index is as close
    t64, q64 = t.astype(np.float64), q.astype(np.float64)
    for n in np.random.RandomState(0).choice(len(q), 300, replace=False):
        diff = q64[n] - t64
        d2 = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        assert i[n] == np.flatnonzero(d2 == d2.min())[0]
    same = np.sqrt(((q64 - t64[ik]) ** 2).sum(-1))
    assert np.array_equal(same, d)                     # cKDTree's pick is at the same distance (exact on this lattice)


def test_sampler_restatement_basics():
    from naruto_amd import synthetic as syn
    v, f = syn.room_sphere_mesh()
    areas = RS.face_areas(v, f)
    assert areas[-1] == 0.0 and (areas[:-1] > 0).all()
    assert abs(areas[:12].sum() - 2 * (6 * 5 + 5 * 3 + 6 * 3)) < 1e-9
    u = RS.uniforms(5, 1000)
    assert u.shape == (1000, 3) and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == 3000
    import helpers as H
    key = H._splitmix64(5)
    assert u[7, 2] == (H._splitmix64((key + 3 * 7 + 2) & H._M64) >> 11) * 2.0 ** -53        # python-int splitmix64, exact
    p, face = RS.sample_surface(v, f, np.cumsum(areas), 20000, 0)
    assert p.dtype == np.float32 and (face != len(f) - 1).all()
    # every sample lies on its face's plane and inside the mesh's box
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    off = np.abs(((p - a) * n).sum(-1)) / np.linalg.norm(n, axis=1)
    assert off.max() < 1e-6
    m = RS.metrics(np.array([0.01, 0.03]), np.array([0.04, 0.06, 0.02, 0.05]))
    assert m == {"accuracy_cm": 2.0, "completion_cm": 4.25, "completion_ratio_pct": 50.0}


def test_ply_round_trip_is_exact(tmp_path):
    from naruto_amd import mesh as M
    rs = np.random.RandomState(3)
    v = rs.normal(size=(50, 3)).astype(np.float32).astype(np.float64)
    f = rs.randint(0, 50, (80, 3)).astype(np.int64)
    col = rs.randint(0, 256, (50, 4)).astype(np.uint8)
    for colors in (None, col):
        path = str(tmp_path / "m.ply")
        M.Mesh(v, f, colors).export(path)
        back = M.Mesh.load(path)
        assert back.vertices.dtype == np.float64 and back.faces.dtype == np.int64
        assert np.array_equal(back.vertices, v) and np.array_equal(back.faces, f)
        assert (back.vertex_colors is None) if colors is None else np.array_equal(back.vertex_colors, col)
        again = str(tmp_path / "again.ply")
        back.export(again)
        assert open(again, "rb").read() == open(path, "rb").read()
    empty = str(tmp_path / "empty.ply")
    M.Mesh(v, np.zeros((0, 3), np.int64)).export(empty)
    assert M.load_ply(empty).faces.shape == (0, 3)


def test_ply_reader_quads_ascii_and_extra_properties(tmp_path):
    from naruto_amd import mesh as M
    ascii_ply = "\n".join([
        "ply", "format ascii 1.0", "comment made by hand", "element vertex 5",
        "property float x", "property float y", "property float z", "property float nx", "property uchar red", "property uchar green", "property uchar blue",
        "element face 3", "property list uchar int vertex_indices", "end_header",
        "0 0 0 0.5 10 20 30", "1 0 0 0.5 11 21 31", "1 1 0 0.5 12 22 32", "0 1 0 0.5 13 23 33", "0.5 0.5 1 0.5 14 24 34",
        "4 0 1 2 3", "3 0 1 4", "3 1 2 4", ""])
    path = tmp_path / "a.ply"
    path.write_text(ascii_ply)
    m = M.load_ply(str(path))
    assert np.array_equal(m.vertices[:, 0], [0, 1, 1, 0, 0.5]) and np.array_equal(m.vertices[4], [0.5, 0.5, 1.0])
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4]]              # the quad split 0-1-2 / 0-2-3
    assert np.array_equal(m.vertex_colors[:, 0], [10, 11, 12, 13, 14]) and (m.vertex_colors[:, 3] == 255).all()
    # binary: double coordinates, a property in front of x, an extra property behind the index list, mixed triangle / quad lists
    head = "\n".join(["ply", "format binary_little_endian 1.0", "element vertex 4", "property short tag", "property double x", "property double y",
                      "property double z", "element face 2", "property list uchar uint vertex_indices", "property uchar flag", "end_header", ""]).encode()
    vert = np.zeros(4, dtype=[("tag", "<i2"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8")])
    vert["x"], vert["y"], vert["z"], vert["tag"] = [0, 1, 1, 0], [0, 0, 1, 1], [0.25, 0.25, 0.25, 1e-3], 7
    body = vert.tobytes() + bytes([3]) + np.array([0, 1, 2], "<u4").tobytes() + bytes([9]) + bytes([4]) + np.array([0, 1, 2, 3], "<u4").tobytes() + bytes([9])
    pathb = tmp_path / "b.ply"
    pathb.write_bytes(head + body)
    mb = M.load_ply(str(pathb))
    assert np.array_equal(mb.vertices[:, 2], [0.25, 0.25, 0.25, 1e-3]) and mb.vertex_colors is None
    assert mb.faces.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3]]
    # uniform quads in binary
    bodyq = vert.tobytes() + (bytes([4]) + np.array([0, 1, 2, 3], "<u4").tobytes() + bytes([1])) * 2
    pathq = tmp_path / "q.ply"
    pathq.write_bytes(head + bodyq)
    assert M.load_ply(str(pathq)).faces.tolist() == [[0, 1, 2], [0, 2, 3]] * 2
    bad = tmp_path / "bad.ply"
    bad.write_bytes(head.replace(b"binary_little_endian", b"binary_big_endian") + body)
    with pytest.raises(ValueError):
        M.load_ply(str(bad))
    with pytest.raises(ValueError):
        (tmp_path / "no.ply").write_text("solid\n")
        M.load_ply(str(tmp_path / "no.ply"))


def test_recon_entry_points_validate_arguments(built_lib):
    """Error codes, never a launch: nothing here touches a device."""
    from naruto_amd import _lib
    lib = built_lib
    big = 2 ** 31
    # sampler: zero faces, zero vertices, counts beyond int32, NULL
    assert lib.naruto_surface_areas(0, 8, None, 0, None, None, None) < 0 and b"faces" in lib.naruto_last_error()
    assert lib.naruto_surface_areas(4, 0, None, 0, None, None, None) < 0
    assert lib.naruto_surface_areas(big, 8, None, 0, None, None, None) < 0 and b"int32" in lib.naruto_last_error()
    assert lib.naruto_surface_areas(4, 8, None, 0, None, None, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_surface_sample(0, 8, None, 0, None, None, 10, 0, None, None, None) < 0
    assert lib.naruto_surface_sample(4, 8, None, 0, None, None, 10, 0, None, None, None) < 0
    # grid plan (host only): the rule, the cap, the refusals
    g = _lib.NarutoNnGrid()
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(4, 2, 1)
    assert lib.naruto_nn_grid_plan(0, lo, hi, 0.0, 0, C.byref(g)) < 0 and b"zero points" in lib.naruto_last_error()
    assert lib.naruto_nn_grid_plan(big, lo, hi, 0.0, 0, C.byref(g)) < 0 and b"int32" in lib.naruto_last_error()
    for cell in (float("nan"), float("inf"), -1.0):
        assert lib.naruto_nn_grid_plan(100, lo, hi, cell, 0, C.byref(g)) < 0 and b"cell" in lib.naruto_last_error()
    assert lib.naruto_nn_grid_plan(100, lo, (C.c_double * 3)(4, float("inf"), 1), 0.0, 0, C.byref(g)) < 0
    assert lib.naruto_nn_grid_plan(100, hi, lo, 0.0, 0, C.byref(g)) < 0
    assert lib.naruto_nn_grid_plan(100, None, hi, 0.0, 0, C.byref(g)) < 0
    assert lib.naruto_nn_grid_plan(28000, lo, hi, 0.0, 0, C.byref(g)) == 0
    assert g.n_points == 28000 and g.cell == 2.0 * np.sqrt(28.0 / 28000) and tuple(g.dims) == tuple(int(e // g.cell) + 1 for e in (4, 2, 1))
    assert lib.naruto_nn_grid_plan(100, lo, hi, 0.5, 0, C.byref(g)) == 0 and g.cell == 0.5 and tuple(g.dims) == (9, 5, 3)
    assert lib.naruto_nn_grid_plan(100, lo, hi, 1e-4, 0, C.byref(g)) == 0
    assert g.cell > 1e-4 and g.dims[0] * g.dims[1] * g.dims[2] <= 2 ** 21                  # the cap enlarged the cell
    assert lib.naruto_nn_grid_plan(100, lo, hi, 1e-4, 1000, C.byref(g)) == 0 and g.dims[0] * g.dims[1] * g.dims[2] <= 1000
    assert lib.naruto_nn_grid_plan(7, lo, lo, 0.0, 0, C.byref(g)) == 0 and tuple(g.dims) == (1, 1, 1) and g.cell == 1.0      # one position
    assert lib.naruto_nn_grid_plan(8, lo, (C.c_double * 3)(4, 0, 0), 0.0, 0, C.byref(g)) == 0 and g.cell == 2.0 and tuple(g.dims) == (3, 1, 1)
    # build / query: NULL buffers, broken grids
    assert lib.naruto_nn_grid_plan(100, lo, hi, 0.5, 0, C.byref(g)) == 0
    assert lib.naruto_nn_grid_workspace(C.byref(g)) >= 100 * 4 + 135 * 4
    assert lib.naruto_nn_grid_build(C.byref(g), None, None, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_nn_grid_query(C.byref(g), 10, None, None, 4, None, None, None, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_nn_grid_query(C.byref(g), big, None, None, 4, None, None, None, None) < 0 and b"int32" in lib.naruto_last_error()
    g.cell = float("nan")
    assert lib.naruto_nn_grid_workspace(C.byref(g)) == 0 and lib.naruto_nn_grid_build(C.byref(g), None, None, None) < 0
    assert b"cell" in lib.naruto_last_error()
    g.cell, g.n_points = 0.5, 0
    assert lib.naruto_nn_grid_query(C.byref(g), 10, None, None, 4, None, None, None, None) < 0
    assert lib.naruto_nn_grid_workspace(None) == 0
    # scan and reduce
    assert lib.naruto_nn_scan(0, None, 10, None, None, None, None) < 0 and b"zero points" in lib.naruto_last_error()
    assert lib.naruto_nn_scan(big, None, 10, None, None, None, None) < 0 and lib.naruto_nn_scan(10, None, big, None, None, None, None) < 0
    assert lib.naruto_nn_scan(10, None, 10, None, None, None, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_dist_reduce_workspace(0) == 0 and lib.naruto_dist_reduce_workspace(big) == 0
    assert lib.naruto_dist_reduce_workspace(200000) >= 98 * 16
    assert lib.naruto_dist_reduce(0, None, 0.05, None, None, None) < 0
    assert lib.naruto_dist_reduce(10, None, float("nan"), None, None, None) < 0
    assert lib.naruto_dist_reduce(10, None, 0.05, None, None, None) < 0 and b"NULL" in lib.naruto_last_error()


def test_recon_kernels_are_in_the_code_object_without_scratch(built_lib):
    from naruto_amd import _lib
    res = _lib.kernel_resources()
    for k in ("k_face_areas<true>", "k_face_areas<false>", "k_surface_sample<true>", "k_surface_sample<false>", "k_grid_count", "k_grid_scan_local",
              "k_grid_scan_totals", "k_grid_scan_add", "k_grid_fill", "k_nn_grid", "k_nn_scan", "k_dist_partial", "k_dist_finish"):
        assert k in res, k
        assert res[k].get("vgpr_spill_count", 0) == 0 and res[k].get("private_segment_fixed_size", 0) == 0, (k, res[k])
        assert res[k]["vgpr_count"] <= 128, (k, res[k])                # four waves per SIMD at the least
    assert res["k_nn_scan"]["group_segment_fixed_size"] == 1024 * 16


def test_degenerate_meshes_are_defined_without_a_device():
    """No faces in the reconstruction: accuracy nan, completion inf, ratio 0 -- decided before anything is launched (this test has no
    GPU to launch on).  No faces in the ground truth: ValueError."""
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    v = np.zeros((3, 3))
    tri = np.array([[0, 1, 2]])
    none = np.zeros((0, 3), dtype=np.int64)
    for rec in ((v, none), M.Mesh(v, none)):
        out = E.calc_3d_mesh_metric((v, tri), rec)
        assert np.isnan(out["accuracy_cm"]) and out["completion_cm"] == float("inf") and out["completion_ratio_pct"] == 0.0
        assert set(out) == {"accuracy_cm", "completion_cm", "completion_ratio_pct"}
    with pytest.raises(ValueError):
        E.calc_3d_mesh_metric((v, none), (v, tri))
    with pytest.raises(ValueError):
        E.ReconEvaluatorHIP(M.Mesh(v, none))


def test_command_line(tmp_path, monkeypatch):
    from naruto_amd import evaluation as E
    with pytest.raises(NotImplementedError):
        E.main(["--rec_mesh", "a.ply", "--gt_mesh", "b.ply", "--align"])
    with pytest.raises(SystemExit):
        E.main(["--rec_mesh", "a.ply"])                                  # --gt_mesh is required
    with pytest.raises(ValueError, match="obj"):
        E.main(["--rec_mesh", "a.ply", "--gt_mesh", "scene.obj"])
    seen = {}

    def fake(gt, rec):
        seen["args"] = (gt, rec)
        return {"accuracy_cm": 1.5, "completion_cm": 2.5, "completion_ratio_pct": 99.0}
    monkeypatch.setattr(E, "calc_3d_mesh_metric", fake)
    out = tmp_path / "res.txt"
    out.write_text("mad,0.75\naccuracy_cm,9.0\n")
    got = E.main(["--rec_mesh", "rec.ply", "--gt_mesh", "gt.ply", "--result_txt", str(out)])
    assert seen["args"] == ("gt.ply", "rec.ply") and got["accuracy_cm"] == 1.5
    assert out.read_text() == "mad,0.75\naccuracy_cm,1.5\ncompletion_cm,2.5\ncompletion_ratio_pct,99.0\n"
    import naruto_amd
    assert naruto_amd.evaluation is E and naruto_amd.ReconEvaluatorHIP is E.ReconEvaluatorHIP

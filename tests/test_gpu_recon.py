"""GPU tests of the reconstruction-metric path (naruto_amd/evaluation.py -> C ABI -> csrc/naruto_recon.hip): the sampler against the numpy
restatement (tests/recon_spec.py) bit for bit, the nearest-neighbour kernels against scipy's cKDTree bit for bit, the metrics, and
evaluate_field end to end."""
import contextlib
import time

import numpy as np
import pytest
import torch

import helpers as H
import recon_spec as RS

pytestmark = pytest.mark.gpu

N_FULL = 200000
EDGE_SECONDS = 30.0          # an edge cloud's query is milliseconds of device work; this much wall clock means the bound on the ring search failed


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _np(t):
    return t.detach().cpu().numpy()


def _room(gpu, which):
    from naruto_amd import synthetic as syn
    return syn.room_sphere_mesh(0.0, 0.8) if which == "gt" else syn.room_sphere_mesh(0.02, 0.81)


def _g10_mesh():
    g = H.load_golden("g10_extract_mesh")
    return g["color_vertices"], g["faces"].astype(np.int32)


@pytest.fixture(scope="module")
def room_pair(gpu):
    """200 000 samples of the room-plus-sphere ground truth (seed 0) and of the reconstruction (walls moved by 2 cm, sphere radius + 1 cm;
    seed 1), on the device and on the host."""
    from naruto_amd import evaluation as E
    out = {}
    for which, seed in (("gt", 0), ("rec", 1)):
        v, f = _room(gpu, which)
        p, _ = E.sample_surface(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), N_FULL, seed)
        out[which] = p
        out[which + "_np"] = _np(p)
    return out


@pytest.mark.parametrize("which", ["room", "g10"])
def test_face_areas_and_cumulative(gpu, which):
    """Areas: the operation order is fixed (cross product by components, products rounded, (cx^2 + cy^2) + cz^2, sqrt, half), so they equal the
    restatement's in every bit.  Cumulative array (torch.cumsum on the device, any summation order): nondecreasing, and every prefix --
    the total is the last -- within n * 2^-53 relative of the exact prefix sum (the fp64 reordering bound; 'exact' = 80-bit accumulation)."""
    from naruto_amd import evaluation as E
    v, f = _room(gpu, "gt") if which == "room" else _g10_mesh()
    areas = E.face_areas(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu))
    want = RS.face_areas(v, f)
    assert np.array_equal(_bits(_np(areas)), _bits(want))
    if which == "room":
        assert want[-1] == 0.0
    cum = _np(torch.cumsum(areas, 0))
    assert (np.diff(cum) >= 0).all()
    exact = np.cumsum(want.astype(np.longdouble))
    err = np.abs(cum.astype(np.longdouble) - exact)
    print("cumulative: worst relative prefix error", float((err / exact.clip(1e-300)).max()), "bound", len(f) * 2.0 ** -53)
    assert (err <= len(f) * 2.0 ** -53 * exact).all()


@pytest.mark.parametrize("which", ["room", "g10"])
def test_sampler_matches_restatement_bit_for_bit(gpu, which):
    """Given the device's own cumulative array read back, face index and float32 points equal the restatement's in every bit: 200 000
    samples of the room-plus-sphere mesh (float32 vertices, 12 wall triangles, a UV sphere, one zero-area face) and of the
    g10_extract_mesh fixture's mesh (float64 vertices)."""
    from naruto_amd import evaluation as E
    v, f = _room(gpu, "gt") if which == "room" else _g10_mesh()
    vd, fd = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    cum = torch.cumsum(E.face_areas(vd, fd), 0)
    for seed in (0, 12345678901234567):
        p, face = E.sample_surface(vd, fd, N_FULL, seed, cumulative=cum)
        wp, wf = RS.sample_surface(v, f, _np(cum), N_FULL, seed)
        assert p.dtype == torch.float32 and p.shape == (N_FULL, 3) and face.dtype == torch.int32
        assert np.array_equal(_np(face), wf)
        assert np.array_equal(_np(p).view(np.uint32), wp.view(np.uint32))
    p2, face2 = E.sample_surface(vd, fd, N_FULL, 0)                      # the cumulative array formed inside: the same torch.cumsum
    wp, wf = RS.sample_surface(v, f, _np(cum), N_FULL, 0)
    assert np.array_equal(_np(face2), wf) and np.array_equal(_np(p2).view(np.uint32), wp.view(np.uint32))
    if which == "room":
        assert (wf != len(f) - 1).all()                                  # the zero-area face is never drawn
    with pytest.raises(ValueError):
        E.sample_surface(vd, torch.full((2, 3), len(v), dtype=torch.int32, device=gpu), 10)          # face index out of range
    with pytest.raises(ValueError):
        E.sample_surface(vd, fd[:0], 10)


def test_sampler_coverage_of_the_walls(gpu):
    """Per-face counts on the 12 wall triangles within 5 sigma of n * area / total (binomial).  Seed 0 is fixed, so this is deterministic;
    the restatement gives a worst |z| of 1.89 for it on the CPU."""
    from naruto_amd import evaluation as E
    v, f = _room(gpu, "gt")
    _, face = E.sample_surface(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu), N_FULL, 0)
    areas = RS.face_areas(v, f)
    p = areas[:12] / areas.sum()
    cnt = np.bincount(_np(face), minlength=len(f))[:12]
    z = (cnt - N_FULL * p) / np.sqrt(N_FULL * p * (1 - p))
    print("wall coverage: worst |z|", np.abs(z).max())
    assert np.abs(z).max() <= 5.0


@pytest.mark.parametrize("method", ["grid", "scan"])
def test_nearest_neighbour_equals_ckdtree_at_full_size(gpu, room_pair, method):
    """200 000 x 200 000 on the sampled room pair (reconstruction samples against ground-truth samples): every distance equals
    cKDTree.query's in every bit; indices are compared wherever the oracle's two nearest distances (k = 2) differ.  Share of queries
    skipped for ties: at most 0.1 % (measured on the CPU with the restatement's samples of this pair: 0.0 % in either direction)."""
    from scipy.spatial import cKDTree
    from naruto_amd import evaluation as E
    grid = E.PointGridHIP(room_pair["gt"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d, i = grid.query(room_pair["rec"], method=method)
    torch.cuda.synchronize()
    print(f"{method}: {N_FULL} x {N_FULL} in {time.perf_counter() - t0:.4f} s; cell {grid.cell:.4f} dims {grid.dims}")
    dk, ik = cKDTree(room_pair["gt_np"]).query(room_pair["rec_np"], k=2)
    assert d.dtype == torch.float64 and i.dtype == torch.int32
    assert np.array_equal(_bits(_np(d)), _bits(dk[:, 0]))
    distinct = dk[:, 0] != dk[:, 1]
    print("tie share", 1.0 - distinct.mean())
    assert 1.0 - distinct.mean() <= 1e-3
    assert np.array_equal(_np(i)[distinct], ik[distinct, 0])
    if method == "grid":
        share = int(grid.last_fallback[0]) / N_FULL
        print("fallback share", share)
        assert share < 0.5


def _lattice(seed=12, n=20000):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 33, (n, 3)) / 8.0).astype(np.float32), (rs.randint(0, 33, (n, 3)) / 8.0).astype(np.float32)


def test_nearest_neighbour_ties_take_the_lowest_index(gpu):
    """The 1/8 m lattice cloud (a third of cKDTree's indices differ from the lowest-index rule there): distance AND index equal the
    restatement's for every query, 20 000 x 20 000, through the grid (with and without cell-ordered queries) and the scan."""
    from naruto_amd import evaluation as E
    q, t = _lattice()
    wd, wi = RS.nearest(q, t)
    grid = E.PointGridHIP(torch.from_numpy(t).to(gpu))
    for kw in (dict(method="grid"), dict(method="grid", sort_queries=False), dict(method="scan")):
        d, i = grid.query(torch.from_numpy(q).to(gpu), **kw)
        assert np.array_equal(_bits(_np(d)), _bits(wd)), kw
        assert np.array_equal(_np(i), wi), kw


def test_nearest_neighbour_does_not_depend_on_the_plan(gpu, room_pair):
    """The same bits, distance and index, whatever the search plan: the default cell, one cell for the whole cloud, a cell so fine that the cap
    enlarges it, a small cap, a ring budget of 1 (everything falls back to the scan), other budgets, cell-ordered queries on and off."""
    from naruto_amd import evaluation as E
    t, q = room_pair["gt"][:50000].contiguous(), room_pair["rec"][:50000].contiguous()
    ref_d, ref_i = E.nearest_distances(q, t, method="scan")
    plans = [dict(), dict(cell=1e9), dict(cell=1e-4), dict(max_cells=500), dict(ring_budget=1), dict(ring_budget=2), dict(ring_budget=9),
             dict(sort_queries=False), dict(cell=0.5, sort_queries=False, ring_budget=2)]
    for kw in plans:
        grid = E.PointGridHIP(t, **kw)
        d, i = grid.query(q)
        assert torch.equal(d.view(torch.int64), ref_d.view(torch.int64)), kw
        assert torch.equal(i, ref_i), kw
        cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
        fallen = int(grid.last_fallback[0])
        print(kw, "cell", grid.cell, "dims", grid.dims, "fallback", fallen)
        if kw.get("cell") == 1e9:
            assert cells == 1 and fallen == 0
        if kw.get("cell") == 1e-4:
            assert grid.cell > 1e-4 and cells <= 2 ** 21
        if kw.get("max_cells"):
            assert cells <= 500
        if kw.get("ring_budget") == 1:
            assert fallen == len(q)
    d, i = E.nearest_distances(q, t)                                     # the one-shot form, method chosen by size
    assert torch.equal(d.view(torch.int64), ref_d.view(torch.int64)) and torch.equal(i, ref_i)


def _edge_clouds():
    rs = np.random.RandomState(21)
    unit = rs.uniform(0.0, 1.0, (5000, 3)).astype(np.float32)
    out = {}
    # queries far outside the target's box; the default cell of 5000 points in a unit box is 2 * sqrt(6 / 5000) = 0.069: 1000 edges = 69 m
    far = np.array([[1.0 + 1000 * 0.0693, 0.5, 0.5], [-8.0, 0.5, 0.5], [0.5, 12.0, -3.0], [-5.0, -5.0, -5.0], [3.0, 3.0, 3.0], [0.5, 0.5, 100.0]], np.float32)
    out["far_queries"] = (np.concatenate([far, rs.uniform(-0.5, 1.5, (500, 3)).astype(np.float32)]), unit)
    cluster = (np.array([500.0, 500.0, 500.0]) + rs.uniform(-0.01, 0.01, (50, 3))).astype(np.float32)
    out["outlier_cluster"] = (np.concatenate([rs.uniform(0, 1, (400, 3)), rs.uniform(499, 501, (200, 3)), rs.uniform(0, 500, (200, 3))]).astype(np.float32),
                              np.concatenate([unit, cluster]))
    out["one_point_target"] = (rs.uniform(-1, 1, (1000, 3)).astype(np.float32), np.array([[0.25, -0.5, 0.75]], np.float32))
    out["query_is_target"] = (unit, unit)
    dup = np.concatenate([unit[:1500]] * 3)[rs.permutation(4500)]
    out["duplicates"] = (np.concatenate([unit[:700], rs.uniform(0, 1, (300, 3)).astype(np.float32)]), dup)
    for n, m in ((1, 1), (63, 65), (65, 4097), (4097, 63), (1, 4097), (4097, 1)):
        out[f"sizes_{n}x{m}"] = (rs.uniform(0, 2, (n, 3)).astype(np.float32), rs.uniform(0, 2, (m, 3)).astype(np.float32))
    out["kilometre_coordinates"] = (rs.uniform(1000.0, 1004.0, (3000, 3)).astype(np.float32), rs.uniform(1000.0, 1004.0, (3000, 3)).astype(np.float32))
    return out


@pytest.mark.parametrize("case", sorted(_edge_clouds()))
def test_nearest_neighbour_edge_clouds(gpu, case):
    """Each edge cloud through the grid and the scan against the restatement (distance bits and index), inside a wall-clock limit: a query 1000
    cell edges from every point costs a scan, not a walk over a million empty cells."""
    from naruto_amd import evaluation as E
    q, t = _edge_clouds()[case]
    wd, wi = RS.nearest(q, t)
    for method in ("grid", "scan"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid = E.PointGridHIP(torch.from_numpy(t).to(gpu))
        d, i = grid.query(torch.from_numpy(q).to(gpu), method=method)
        torch.cuda.synchronize()
        took = time.perf_counter() - t0
        assert took < EDGE_SECONDS, (case, method, took)
        assert np.array_equal(_bits(_np(d)), _bits(wd)), (case, method)
        assert np.array_equal(_np(i), wi), (case, method)
    if case == "query_is_target":
        assert (wd == 0).all() and (wi <= np.arange(len(q))).all()
    if case == "far_queries":
        assert abs(grid.cell - 0.0693) < 1e-3 and wd[0] > 999 * grid.cell


def _room_evaluator_inputs(gpu):
    vg, fg = _room(gpu, "gt")
    vr, fr = _room(gpu, "rec")
    return (vg, fg), (vr, fr)


def test_metrics_against_the_oracle_and_reproducible(gpu):
    """calc_3d_mesh_metric on the room pair: two runs give identical bits; the means equal numpy's means of cKDTree's distances (on the same
    samples) within 2 * n * 2^-53 relative (the fp64 reordering bound at n = 200 000: 4.4e-11), the ratio's count is exact."""
    from scipy.spatial import cKDTree
    from naruto_amd import evaluation as E
    gt, rec = _room_evaluator_inputs(gpu)
    a = E.calc_3d_mesh_metric(gt, rec)
    b = E.calc_3d_mesh_metric(gt, rec)
    assert set(a) == {"accuracy_cm", "completion_cm", "completion_ratio_pct"}
    assert all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) for k in a), (a, b)
    pg, _ = E.sample_surface(torch.from_numpy(gt[0]).to(gpu), torch.from_numpy(gt[1]).to(gpu), N_FULL, 0)
    pr, _ = E.sample_surface(torch.from_numpy(rec[0]).to(gpu), torch.from_numpy(rec[1]).to(gpu), N_FULL, 1)
    pg, pr = _np(pg), _np(pr)
    d_rec = cKDTree(pg).query(pr)[0]
    d_gt = cKDTree(pr).query(pg)[0]
    want = RS.metrics(d_rec, d_gt, 0.05)
    print("metrics", a, "oracle", want)
    tol = 2 * N_FULL * 2.0 ** -53
    assert abs(a["accuracy_cm"] - want["accuracy_cm"]) <= tol * want["accuracy_cm"]
    assert abs(a["completion_cm"] - want["completion_cm"]) <= tol * want["completion_cm"]
    assert round(a["completion_ratio_pct"] * N_FULL / 100.0) == np.count_nonzero(d_gt < 0.05)
    assert abs(a["completion_ratio_pct"] - want["completion_ratio_pct"]) <= 1e-12
    # a threshold that splits the distances, through the evaluator and through a mesh object / a file
    ev = E.ReconEvaluatorHIP(gt, threshold=0.024)
    c = ev.evaluate_mesh(torch.from_numpy(rec[0]).to(gpu), torch.from_numpy(rec[1]).to(gpu))
    assert round(c["completion_ratio_pct"] * N_FULL / 100.0) == np.count_nonzero(d_gt < 0.024) and 5.0 < c["completion_ratio_pct"] < 95.0
    assert c["accuracy_cm"] == a["accuracy_cm"] and c["completion_cm"] == a["completion_cm"]
    empty = ev.evaluate_mesh(torch.zeros(0, 3, device=gpu), torch.zeros(0, 3, dtype=torch.int32, device=gpu))
    assert np.isnan(empty["accuracy_cm"]) and empty["completion_cm"] == float("inf") and empty["completion_ratio_pct"] == 0.0


def test_metrics_from_ply_files_and_command_line(gpu, tmp_path):
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    gt, rec = _room_evaluator_inputs(gpu)
    paths = []
    for name, (v, f) in (("gt", gt), ("rec", rec)):
        paths.append(str(tmp_path / f"{name}.ply"))
        M.Mesh(v.astype(np.float64), f.astype(np.int64)).export(paths[-1])
    direct = E.calc_3d_mesh_metric(gt, rec, n_samples=50000)
    assert E.calc_3d_mesh_metric(paths[0], paths[1], n_samples=50000) == direct          # float32 vertices survive the file exactly
    out = tmp_path / "res.txt"
    got = E.main(["--rec_mesh", paths[1], "--gt_mesh", paths[0], "--result_txt", str(out)])
    lines = dict(line.split(",") for line in out.read_text().split())
    assert set(lines) == set(got) and all(float(lines[k]) == got[k] for k in got)
    assert 2.0 < got["accuracy_cm"] < 3.0 and got["completion_ratio_pct"] > 99.0


def _g10_field(gpu):
    g = H.load_golden("g10_extract_mesh")
    cfg = H.office_cfg(int(g["hash_size"]))
    cfg["data"]["sc_factor"], cfg["data"]["translation"] = float(g["sc_factor"]), float(g["translation"])
    w = {k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")}
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights=w).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    return g, cfg, ora, m


@contextlib.contextmanager
def _host_copies():
    """Every device -> host copy made through the tensor methods that make one, with its element count."""
    seen = []
    saved = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "numpy", "to")}

    def wrap(name):
        fn = saved[name]

        def inner(self, *a, **k):
            out = fn(self, *a, **k)
            if self.is_cuda and not (isinstance(out, torch.Tensor) and out.is_cuda):
                seen.append((name, self.numel()))
            return out
        return inner
    for name in saved:
        setattr(torch.Tensor, name, wrap(name))
    try:
        yield seen
    finally:
        for name, fn in saved.items():
            setattr(torch.Tensor, name, fn)


def test_evaluate_field_end_to_end(gpu):
    """ReconEvaluatorHIP.evaluate_field on the g10 field: the three mesh metrics equal calc_3d_mesh_metric on the mesh extract_mesh returns for
    the same field, bit for bit; mad_cm equals the mean |sdf| of the CPU oracle's query_sdf at the same samples within the 1e-4 the parity
    tests assert for query_sdf; and no device-to-host copy in the call is larger than a few scalars."""
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    g, cfg, ora, m = _g10_field(gpu)
    gt = (g["color_vertices"], g["faces"])
    mcb = torch.from_numpy(g["mcb"])
    voxel = float(g["voxel"])
    ev = E.ReconEvaluatorHIP(gt, device=gpu)
    with torch.no_grad():
        ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb)           # warm: workspaces, lazy loads
        with _host_copies() as copies:
            got = ev.evaluate_field(m, cfg, m.bounding_box, voxel, marching_cube_bound=mcb)
    print("evaluate_field", got, "host copies", copies)
    assert copies and max(n for _, n in copies) <= 16, copies
    assert set(got) == {"accuracy_cm", "completion_cm", "completion_ratio_pct", "mad_cm"}
    mesh = M.extract_mesh(m.query_sdf, cfg, m.bounding_box, marching_cube_bound=mcb, color_func=None, voxel_size=voxel, render_uncert=False)
    assert len(mesh.faces) > 1000
    want = E.calc_3d_mesh_metric(gt, mesh)
    for k in want:
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (k, got[k], want[k])
    assert got["accuracy_cm"] < 100 * voxel and got["completion_ratio_pct"] > 50.0
    # MAD against the oracle on the CPU, at the evaluator's own samples, normalised as query_point_sdf normalises
    pts = (ev.gt_points.cpu() + cfg["data"]["translation"]) * cfg["data"]["sc_factor"]
    bb = ora.bounding_box
    pts = (pts - bb[:, 0]) / (bb[:, 1] - bb[:, 0])
    with torch.no_grad():
        sdf = torch.cat([ora.query_sdf(pts[s:s + 65536, None, :]).reshape(-1) for s in range(0, len(pts), 65536)])
    unit = cfg["training"]["trunc"] * 100.0
    print("mad_cm", got["mad_cm"], "oracle", float(sdf.double().abs().mean()) * unit)
    assert abs(got["mad_cm"] / unit - float(sdf.double().abs().mean())) <= 1e-4

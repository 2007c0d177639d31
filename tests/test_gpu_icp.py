"""GPU tests of the rigid-alignment path (naruto_amd.evaluation.icp -> C ABI -> csrc/naruto_icp.hip) against the numpy + cKDTree twin
(tests/icp_spec.py): the transform bit for bit, the 17 sums within the fp64 reordering bound, one update, whole runs on the table of
known displacements, the degenerate cases, and the aligned metrics end to end against the EXISTING evaluator on the undisplaced mesh."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_spec as IS

pytestmark = pytest.mark.gpu

# target samples, source points, rotation (degrees), t (metres); the twin's record: iterations, fitness at the start
TABLE = [(20000, 4099, 2.0, 0.03), (4099, 4099, 1.0, 0.02), (20000, 4099, 4.0, 0.06)]


def _np(t):
    return t.detach().cpu().numpy()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def clouds(gpu):
    """Per table row: (source float32 [ns,3], target float32 [nt,3], T_known).  Target = surface samples of the room-plus-sphere mesh
    (seed 0), source = its first ns points displaced by the known rigid map (fp64, rounded once).  Left unchanged by every test."""
    from naruto_amd import evaluation as E
    from naruto_amd import synthetic as syn
    v, f = syn.room_sphere_mesh(0.0, 0.8)
    vd, fd = torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu)
    samples = {n: _np(E.sample_surface(vd, fd, n, 0)[0]) for n in sorted({row[0] for row in TABLE})}
    out = []
    for nt, ns, angle, t in TABLE:
        target = samples[nt]
        known = IS.rigid(angle, t, target.astype(np.float64).mean(0))
        out.append((IS.transform(target[:ns], known), target, known))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_transform_equals_the_twin_bit_for_bit(gpu, n):
    from naruto_amd import evaluation as E
    rs = np.random.RandomState(n)
    p = (rs.uniform(-1.0, 1.0, (n, 3)) * np.array([6.0, 5.0, 3.0])).astype(np.float32)
    T = IS.rigid(33.0, 0.4, [3.0, 2.5, 1.4])
    got = E.transform_points(torch.from_numpy(p).to(gpu), T)
    assert got.dtype == torch.float32 and np.array_equal(_np(got).view(np.uint32), IS.transform(p, T).view(np.uint32))
    # float64 vertices stay float64: the same arithmetic without the final rounding
    p64 = p.astype(np.float64) + 1e-9
    got64 = _np(E.transform_points(torch.from_numpy(p64).to(gpu), T))
    want64 = np.stack([((T[a, 0] * p64[:, 0] + T[a, 1] * p64[:, 1]) + T[a, 2] * p64[:, 2]) + T[a, 3] for a in range(3)], 1)
    assert got64.dtype == np.float64 and np.array_equal(got64.view(np.uint64), want64.view(np.uint64))


def _accumulate(gpu, p, tgt, idx, dist, thr, origin):
    from naruto_amd import _lib
    lib = _lib.load()
    n = len(p)
    pd, td = torch.from_numpy(p).to(gpu), torch.from_numpy(tgt).to(gpu)
    idd, dd = torch.from_numpy(idx).to(gpu), torch.from_numpy(dist).to(gpu)
    ws = _lib.workspace(lib.naruto_icp_accumulate_workspace(n), gpu, torch.float64)
    sums = torch.full((17,), float("nan"), dtype=torch.float64, device=gpu)
    _lib.check(lib.naruto_icp_accumulate(n, pd.data_ptr(), len(tgt), td.data_ptr(), idd.data_ptr(), dd.data_ptr(), thr, (C.c_double * 3)(*origin), ws.data_ptr(),
                                         sums.data_ptr(), _stream()), "naruto_icp_accumulate")
    return _np(sums)


@pytest.mark.parametrize("n", [3, 257, 4099, 70001])
@pytest.mark.parametrize("inliers", ["none", "all", "mixed"])
def test_accumulate_within_the_reordering_bound_and_reproducible(gpu, n, inliers):
    """One workgroup, a ragged tail, several partials (70 001 points = 35 workgroups).  Count exact; every other sum within
    n * 2^-53 * sum |term| of the 80-bit sum of the same fp64 terms; a distance EQUAL to the threshold is an inlier, a NaN distance and an
    index outside the target are not; two runs give equal bits."""
    rs = np.random.RandomState(7 * n)
    m, thr = 513, 0.1
    origin = np.array([3.0, 2.5, 1.5])
    p = (rs.uniform(0.0, 1.0, (n, 3)) * np.array([6.0, 5.0, 3.0])).astype(np.float32)
    tgt = (rs.uniform(0.0, 1.0, (m, 3)) * np.array([6.0, 5.0, 3.0])).astype(np.float32)
    idx = rs.randint(0, m, n).astype(np.int32)
    if inliers == "none":
        dist = rs.uniform(np.nextafter(thr, 1.0), 0.3, n)
    elif inliers == "all":
        dist = rs.uniform(0.0, thr, n)
    else:
        dist = rs.uniform(0.0, 2.0 * thr, n)
        dist[::5] = thr                                        # exactly the threshold: inliers
        dist[1::5] = np.nextafter(thr, 1.0)                    # one ulp above: not
        dist[2::11] = np.nan
        idx[3::13] = -1
        idx[4::17] = m
    inl = (dist <= thr) & (idx >= 0) & (idx < m)
    got = _accumulate(gpu, p, tgt, idx, dist, thr, origin)
    again = _accumulate(gpu, p, tgt, idx, dist, thr, origin)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    assert got[0] == float(inl.sum())
    if inliers == "none":
        assert inl.sum() == 0 and np.array_equal(got, np.zeros(17))
        return
    assert inl.sum() == n if inliers == "all" else 0 < inl.sum() < n
    pp, qq, dd = p[inl].astype(np.float64) - origin, tgt[idx[inl]].astype(np.float64) - origin, dist[inl]
    terms = np.concatenate([(dd * dd)[:, None], pp, qq, (pp[:, :, None] * qq[:, None, :]).reshape(-1, 9)], 1)        # fp64 terms, as the kernel forms them
    exact = terms.astype(np.longdouble).sum(0)
    bound = n * 2.0 ** -53 * np.abs(terms).astype(np.longdouble).sum(0)
    err = np.abs(got[1:].astype(np.longdouble) - exact)
    print(f"n={n} {inliers}: inliers {int(inl.sum())}, worst error / bound {float((err / bound).max()):.3e}")
    assert (err <= bound).all()


def test_one_update_equals_the_twins_kabsch_on_the_same_pairs(gpu, clouds):
    from naruto_amd import evaluation as E
    source, target, _ = clouds[0]
    grid = E.PointGridHIP(torch.from_numpy(target).to(gpu))
    out = E.icp(torch.from_numpy(source).to(gpu), grid, max_iteration=1)
    assert out.iterations == 1 and len(out.history) == 2 and out.status in ("max_iteration", "converged")
    dist, index = (_np(x) for x in grid.query(torch.from_numpy(source).to(gpu)))             # the device's own correspondences at T = identity
    inl = dist <= 0.1
    assert out.history[0][0] == inl.sum() / len(source)
    want = IS.kabsch(source[inl], target[index[inl]])
    err = np.abs(out.transformation - want).max()
    print("one update: |dT - twin|", err)
    assert err <= 1e-10


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_whole_icp_recovers_the_known_displacement(gpu, clouds, row):
    from naruto_amd import evaluation as E
    source, target, known = clouds[row]
    twin = IS.icp(source, target)
    out = E.icp(torch.from_numpy(source).to(gpu), torch.from_numpy(target).to(gpu))
    res = out.transformation @ known - np.eye(4)
    print(f"row {row}: device {out.iterations} iterations, twin {twin['iterations']}; fitness {out.history[0][0]:.4f} -> {out.fitness}; "
          f"|T T_known - I| {np.abs(res).max():.3e} (twin {np.abs(twin['transformation'] @ known - np.eye(4)).max():.3e}); rmse {out.inlier_rmse:.3e}")
    assert out.converged and out.status == "converged" and out.iterations <= 30 and len(out.history) == out.iterations + 1
    assert out.fitness == 1.0
    assert np.abs(res).max() <= 1e-6                              # one float32 ulp at 6 m is 4.8e-7; the twin reaches 1e-9
    assert out.history[0][0] == twin["history"][0][0]             # the queries are the input bits there
    assert out.transformation.dtype == np.float64 and out.transformation.shape == (4, 4) and np.array_equal(out.transformation[3], [0.0, 0.0, 0.0, 1.0])
    again = E.icp(torch.from_numpy(source).to(gpu), torch.from_numpy(target).to(gpu))
    assert np.array_equal(again.transformation.view(np.uint64), out.transformation.view(np.uint64))
    assert again.history == out.history and again.iterations == out.iterations and again.inlier_rmse == out.inlier_rmse


def test_degenerate_and_empty_sources(gpu):
    from naruto_amd import evaluation as E
    target = torch.from_numpy(np.random.RandomState(0).uniform(0.0, 1.0, (5000, 3)).astype(np.float32)).to(gpu)
    out = E.icp(target[:300] + 2.0, target)                      # every source point is at least 1 m from every target
    assert out.status == "degenerate" and not out.converged and out.iterations == 0
    assert out.fitness == 0.0 and out.inlier_rmse == 0.0 and out.history == [(0.0, 0.0)]
    assert np.array_equal(out.transformation, np.eye(4))
    init = IS.rigid(5.0, 0.0, [0.5, 0.5, 0.5])
    init[:3, 3] += 2.0
    out = E.icp(target[:300], target, init=init)                 # the same through an initial transformation: returned unchanged
    assert out.status == "degenerate" and np.array_equal(out.transformation, init)
    two = E.icp(target[:2], target)                              # two inliers: a rotation is not determined
    assert two.status == "degenerate" and two.fitness == 1.0 and np.array_equal(two.transformation, np.eye(4))
    with pytest.raises(ValueError):
        E.icp(target[:0], target)
    with pytest.raises(ValueError):
        E.icp(target, target[:0])


@pytest.fixture(scope="module")
def meshes(gpu):
    """The ground truth, the reconstruction (walls moved by 2 cm, sphere radius + 1 cm), and the reconstruction displaced by 2 degrees about
    the table's axis around the ground truth's vertex mean and 3 cm -- not 3 degrees / 5 cm: the twin falls into a local minimum of the
    symmetric sphere there."""
    from naruto_amd import synthetic as syn
    gt = syn.room_sphere_mesh(0.0, 0.8)
    rec_v, rec_f = syn.room_sphere_mesh(0.02, 0.81)
    known = IS.rigid(2.0, 0.03, gt[0].astype(np.float64).mean(0))
    moved = (rec_v.astype(np.float64) @ known[:3, :3].T + known[:3, 3]).astype(np.float32)
    return gt, (rec_v, rec_f), (moved, rec_f)


@pytest.fixture(scope="module")
def evaluated(gpu, meshes):
    from naruto_amd import evaluation as E
    gt, rec, moved = meshes
    ev = E.ReconEvaluatorHIP(gt, n_samples=50000)
    return ev, ev.evaluate_mesh(rec), ev.evaluate_mesh(moved), ev.evaluate_mesh(moved, align=True)


def test_aligned_metrics_equal_the_undisplaced_ones(gpu, meshes, evaluated):
    """The yardstick is the EXISTING evaluate_mesh on the undisplaced reconstruction.  The twin's figures: aligned vertices within 7.4e-5 m
    after 12 iterations (the 5e-4 m margin covers a stop one iteration apart at the 1e-6 criteria), metrics within 0.002 cm, the
    unaligned mesh at 5.28 cm against 3.34 cm."""
    from naruto_amd import evaluation as E
    gt, rec, moved = meshes
    ev, plain, unaligned, aligned = evaluated
    back, result = ev.align_vertices(torch.from_numpy(moved[0]).to(gpu))
    worst = float(np.abs(_np(back).astype(np.float64) - rec[0].astype(np.float64)).max())
    dist = float(np.linalg.norm(_np(back).astype(np.float64) - rec[0].astype(np.float64), axis=1).max())
    print(f"aligned: {result.iterations} iterations ({result.status}), fitness {result.fitness}, rmse {result.inlier_rmse:.5f}; vertices within {dist:.3e} m "
          f"(worst coordinate {worst:.3e}); plain {plain}; unaligned {unaligned}; aligned {aligned}")
    assert back.dtype == torch.float32 and result.converged
    assert dist <= 5e-4
    assert set(aligned) == {"accuracy_cm", "completion_cm", "completion_ratio_pct", "align_fitness", "align_inlier_rmse"}
    assert aligned["align_fitness"] == result.fitness and aligned["align_inlier_rmse"] == result.inlier_rmse
    for key in ("accuracy_cm", "completion_cm"):
        assert abs(aligned[key] - plain[key]) <= 0.05, key
        assert unaligned[key] > plain[key] + 1.0, key
    assert np.array_equal(E.get_align_transformation(moved, gt), result.transformation)


def test_align_false_is_unchanged_and_the_command_line_aligns(gpu, meshes, evaluated, tmp_path):
    from naruto_amd import evaluation as E
    from naruto_amd import mesh as M
    gt, rec, moved = meshes
    ev, plain, unaligned, aligned = evaluated
    assert ev.evaluate_mesh(moved, align=False) == unaligned and set(unaligned) == {"accuracy_cm", "completion_cm", "completion_ratio_pct"}
    assert ev.evaluate_mesh(rec, align=False) == plain
    gt_path, rec_path = str(tmp_path / "gt.ply"), str(tmp_path / "rec.ply")
    M.Mesh(gt[0], gt[1]).export(gt_path)
    M.Mesh(moved[0], moved[1]).export(rec_path)
    assert E.calc_3d_mesh_metric(gt_path, rec_path, align=False) == E.calc_3d_mesh_metric(gt_path, rec_path)
    out = tmp_path / "res.txt"
    got = E.main(["--rec_mesh", rec_path, "--gt_mesh", gt_path, "--icp_align", "--result_txt", str(out)])
    want = E.calc_3d_mesh_metric(gt_path, rec_path, align=True)
    assert got == want and "align_fitness" in got and "align_fitness," in out.read_text()
    full = E.calc_3d_mesh_metric(gt_path, (rec[0], rec[1]))      # 200 000 samples, the undisplaced reconstruction
    for key in ("accuracy_cm", "completion_cm"):
        assert abs(got[key] - full[key]) <= 0.05, key
    with pytest.raises(NotImplementedError):
        E.main(["--rec_mesh", rec_path, "--gt_mesh", gt_path, "--align"])

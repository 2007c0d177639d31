"""CPU tests of the mesh-culling path's host side (naruto_amd/culling.py) and of its numpy restatement (tests/cull_spec.py): the
restatement's depth maps against the analytic room, argument validation that never reaches a kernel, the output file name, the checkpoint
reader, the C ABI's argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from naruto_amd import culling as CU

import cull_spec as CS


@pytest.fixture(scope="module")
def room_depth():
    v, f = CS.room_mesh()
    poses, cam = CS.ring_poses(4), CS.camera()
    return v, f, poses, cam, CS.render_depth(v, f, poses, cam)


def test_spec_depth_matches_the_analytic_room_on_wall_pixels(room_depth):
    """The restated rasteriser sees the room from inside -- 6 to 8 of the 12 wall triangles reach behind each camera and are rasterised
    without clipping -- and its depth on the pixels whose ray hits a wall equals AnalyticRoom.cast's (distance along the ray turned into
    depth along the viewing axis).  Bound: coordinates up to 7 m, about ten float32 roundings (2^-24 relative each) from vertex to depth:
    7 * 10 * 6e-8 = 4e-6 m."""
    v, f, poses, cam, depth = room_depth
    room = CS.analytic_room()
    H, W = cam["H"], cam["W"]
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(i - cam["cx"]) / cam["fx"], -(j - cam["cy"]) / cam["fy"], -np.ones_like(i)], -1).reshape(-1, 3)
    worst = 0.0
    for k, c2w in enumerate(poses.astype(np.float64)):
        x = CS.camera_space(v, poses[k])
        whole = sum(CS.pixel_box(x[a], x[b], x[c], cam, 0.01) == (0, 0, W - 1, H - 1) for a, b, c in f[:12])
        assert 6 <= whole <= 8, whole
        dw = dc @ c2w[:3, :3].T
        norm = np.linalg.norm(dw, axis=1)
        t, _, kind = room.cast(np.broadcast_to(c2w[:3, 3], dw.shape), dw / norm[:, None])
        wall = (kind < 6).reshape(H, W)
        assert wall.sum() > 500 and np.isfinite(depth[k]).all()
        worst = max(worst, np.abs(depth[k] - (t / norm).reshape(H, W))[wall].max())
    print("spec depth vs analytic room, wall pixels: worst", worst)
    assert worst <= 4e-6


def test_spec_candidate_box_is_conservative(room_depth):
    """Only coverage decides a pixel: testing every pixel of the image against every triangle gives the same bits as the candidate boxes."""
    v, f, poses, cam, depth = room_depth
    full = CS.render_depth(v, f, poses[:2], cam, use_box=False)
    assert np.array_equal(full.view(np.uint32), depth[:2].view(np.uint32))


def test_spec_keep_rule_and_compaction(room_depth):
    """Kept faces and vertices keep their order, faces are re-indexed, colours follow; the 12 wall triangles (corners outside every
    frustum) are all culled at 80 x 60, as the module docstring says of large faces."""
    v, f, poses, cam, depth = room_depth
    col = (np.arange(len(v) * 4) % 251).astype(np.uint8).reshape(-1, 4)
    vo, fo, co = CS.cull_mesh(v, f, poses, cam, colors=col)
    _, seen = CS.vertex_tests(v, poses, cam, depth, 0.03)
    keep = seen.any(0)[f].any(1)
    assert not keep[:12].any() and 0 < keep.sum() < len(f) and len(fo) == keep.sum()
    assert np.array_equal(vo[fo], v[f[keep]])                      # same triangles, same order, same corner order
    used = np.zeros(len(v), dtype=bool)
    used[f[keep]] = True
    assert np.array_equal(vo, v[used]) and np.array_equal(co, col[used])
    # bounds: a face survives iff one of its vertices is inside
    bounds = [[2.0, 3.0], [0.0, 5.0], [0.0, 3.0]]
    _, fb, _ = CS.cull_mesh(v, f, poses, cam, bounds=bounds, remove_occlusion=False)
    inside = CS.inside_bounds(v, bounds)
    fr, _ = CS.vertex_tests(v, poses, cam)
    assert len(fb) == (inside[f].any(1) & fr.any(0)[f].any(1)).sum() and 0 < len(fb) < len(f)


def test_arguments_are_validated_before_any_launch():
    v, f = CS.room_mesh()
    poses, cam = CS.ring_poses(2), CS.camera()
    bad_f = f.copy()
    bad_f[5, 1] = len(v)
    neg_f = f.copy()
    neg_f[0, 0] = -1
    nan_pose = poses.copy()
    nan_pose[1, 0, 3] = np.nan
    inf_pose = poses.copy()
    inf_pose[0, 1, 1] = np.inf
    for fn in (lambda **k: CU.cull_mesh((k["v"], k["f"]), k["p"], k["cam"]), lambda **k: CU.render_depth(k["v"], k["f"], k["p"], k["cam"])):
        for kw in (dict(f=bad_f), dict(f=neg_f), dict(f=f[:0]), dict(p=nan_pose), dict(p=inf_pose), dict(p=poses[:0]), dict(p=poses[:, :3]),
                   dict(cam={**cam, "H": 0}), dict(cam={**cam, "W": 0}), dict(cam={**cam, "fx": 0.0}), dict(cam={**cam, "cy": float("nan")}),
                   dict(cam={k: cam[k] for k in cam if k != "fy"})):
            with pytest.raises(ValueError):
                fn(**{**dict(v=v, f=f, p=poses, cam=cam), **kw})
    with pytest.raises(ValueError):
        CU.render_depth(v, f, poses, cam, near=1.0, far=1.0)
    with pytest.raises(ValueError):
        CU.render_depth(v, f, poses, cam, near=0.0)
    with pytest.raises(ValueError):
        CU.render_depth(v, f, poses, cam, pose_chunk=0)
    with pytest.raises(ValueError):
        CU.cull_mesh((v, f), poses, cam, eps=float("nan"))
    with pytest.raises(ValueError):
        CU.observed_vertices(v, nan_pose, cam)
    with pytest.raises(ValueError):
        CU.observed_vertices(v, poses, {**cam, "W": -3})
    with pytest.raises(ValueError):
        CU.cull_mesh(5, poses, cam)


def test_output_file_name():
    assert CU.culled_path("out/mesh_1999_final.ply", True) == "out/mesh_1999_final_cull_occlusion.ply"       # the name eval_replica.sh reads
    assert CU.culled_path("out/mesh_1999_final.ply", False) == "out/mesh_1999_final_cull_frustum.ply"
    assert CU.culled_path("a.b/m.PLY", True) == "a.b/m_cull_occlusion.PLY"


def test_poses_from_checkpoint_and_frames(tmp_path):
    poses = torch.from_numpy(CS.ring_poses(5))
    ids = [20, 0, 15, 5, 10]
    path = tmp_path / "ckpt.pt"
    torch.save({"pose": {i: poses[k].double() for k, i in enumerate(ids)}, "frame_id": 20}, path)
    got = CU.poses_from_checkpoint(str(path))
    assert got.dtype == torch.float32 and got.shape == (5, 4, 4)
    assert torch.equal(got, poses[[1, 3, 4, 2, 0]])                                 # sorted by frame id
    torch.save({"model": {}}, path)
    with pytest.raises(ValueError):
        CU.poses_from_checkpoint(str(path))
    # field frame -> metric frame: extract_mesh's last vertex transform, on the camera centres and the bound
    cfg = {"data": {"sc_factor": 2.0, "translation": 0.5}}
    p, b = CU.to_metric(cfg, poses, [[-2.0, 2.0], [0.0, 4.0], [1.0, 3.0]])
    assert torch.equal(p[:, :3, :3], poses[:, :3, :3]) and torch.equal(p[:, :3, 3], poses[:, :3, 3] / 2.0 - 0.5)
    assert b.tolist() == [[-1.5, 0.5], [-0.5, 1.5], [0.0, 1.0]]


def test_entry_points_validate_arguments(built_lib):
    from naruto_amd import _lib
    lib = built_lib
    cam = _lib.NarutoCullCam(60, 80, 60.0, 60.0, 39.5, 29.5, 0.01, 10.0)
    assert lib.naruto_render_depth_workspace(100, 200, 8) >= 100 * 8 * 16 + 200 * 8 * 12
    assert lib.naruto_render_depth_workspace(0, 200, 8) == 0 and lib.naruto_render_depth_workspace(100, 200, 0) == 0
    assert lib.naruto_render_depth_workspace(100, 1 << 27, 2) == 0                  # faces x poses per call stays below 2^28
    assert lib.naruto_render_depth(C.byref(cam), 100, None, 200, None, None, 8, None, 512, None, None, None) < 0
    assert b"NULL" in lib.naruto_last_error()
    assert lib.naruto_render_depth(None, 100, None, 200, None, None, 8, None, 512, None, None, None) < 0
    for field, val in (("H", 0), ("W", 0), ("fx", 0.0), ("near_", 0.0), ("far_", 0.005), ("cx", float("nan"))):
        bad = _lib.NarutoCullCam(60, 80, 60.0, 60.0, 39.5, 29.5, 0.01, 10.0)
        setattr(bad, field, val)
        assert lib.naruto_render_depth(C.byref(bad), 100, None, 200, None, None, 8, None, 512, None, None, None) < 0, field
    assert lib.naruto_observed_vertices(C.byref(cam), 100, None, 2, None, None, 0.03, None, None) < 0
    assert lib.naruto_observed_vertices(C.byref(cam), 100, None, 2, None, None, float("nan"), None, None) < 0
    assert lib.naruto_cull_faces(10, 10, None, None, None, None, None, None) < 0
    assert lib.naruto_cull_compact(10, 10, None, None, None, None, None, None, 0, None, 11, 1, None, None, None, None) < 0
    assert lib.naruto_cull_compact(10, 10, None, None, None, None, None, None, 0, None, 3, 3, None, None, None, None) < 0
    assert lib.naruto_cull_compact(10, 10, None, None, None, None, None, None, 0, None, 0, 0, None, None, None, None) == 0      # an empty result: nothing to do

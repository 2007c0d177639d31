"""Host side of the stand-alone run (no GPU): the step schedule of ``online_recon_step``, the trajectory length, trajectory-file
parsing, the command line's argument handling, and the frame entry points of the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from naruto_amd import run as R
from naruto_amd.evaluation import trajectory_length, update_results_file
from naruto_amd.slam import camera_rays, step_schedule


@pytest.mark.parametrize("map_every,keyframe_every", [(5, 5), (3, 4)])
def test_step_schedule_is_the_reference_conditions(map_every, keyframe_every):
    """coslam.py:571 (mesh), :579 (first frame, which is always a keyframe and returns volumes), :607 (global_BA + volumes, frames
    other than 0), :622 (keyframe), restated."""
    cfg = {"mapping": {"map_every": map_every, "keyframe_every": keyframe_every}, "mesh": {"vis": 10}}
    for i in range(21):
        mesh = i % 10 == 0
        if i == 0:
            first, mapped, keyframe = True, False, True
        else:
            first, mapped, keyframe = False, i % map_every == 0, i % keyframe_every == 0
        want = {"mesh": mesh, "first": first, "map": mapped, "keyframe": keyframe, "volumes": first or mapped}
        assert step_schedule(i, cfg) == want, i
    mapped = [i for i in range(21) if step_schedule(i, cfg)["volumes"]]
    assert mapped == ([0, 5, 10, 15, 20] if map_every == 5 else [0, 3, 6, 9, 12, 15, 18])


def _poses(n, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        p = np.eye(4)
        p[:3, :3], p[:3, 3] = q, rs.uniform(-2, 2, 3)
        out.append(p)
    return out


def test_trajectory_length_is_the_reference_formula():
    """eval_traj_length.py:64-73 in fp64: sum of |(P_i^-1 P_{i-1})[:3, 3]| (for rigid poses: the path length of the positions)."""
    poses = _poses(7)
    want = 0.0
    for i in range(1, len(poses)):
        rel = np.linalg.inv(poses[i]) @ poses[i - 1]
        want += float(np.linalg.norm(rel[:3, 3]))
    got = trajectory_length(torch.from_numpy(np.stack(poses)))
    assert abs(got - want) <= 1e-12 * want
    path = sum(float(np.linalg.norm(poses[i][:3, 3] - poses[i - 1][:3, 3])) for i in range(1, len(poses)))
    assert abs(got - path) <= 1e-9 * path
    assert trajectory_length({k: torch.from_numpy(p) for k, p in enumerate(poses)}) == got, "a checkpoint's frame id -> pose dict"
    assert trajectory_length(poses[:1]) == 0.0 and trajectory_length([]) == 0.0
    line = np.eye(4)[None].repeat(3, 0)
    line[1, 0, 3], line[2, 0, 3] = 1.5, 1.0
    assert trajectory_length(line) == 2.0


def test_results_file_carries_the_trajectory_length(tmp_path):
    path = tmp_path / "results.txt"
    update_results_file({"accuracy_cm": 1.5}, str(path))
    update_results_file({"traj_len(m)": 12.25}, str(path))
    assert path.read_text() == "accuracy_cm,1.5\ntraj_len(m),12.25\n"


def test_replica_trajectory_parsing(tmp_path):
    poses = _poses(3, seed=4)
    path = tmp_path / "traj.txt"
    path.write_text("\n".join(" ".join(repr(float(x)) for x in p.reshape(-1)) for p in poses) + "\n\n")
    got = R.load_replica_traj(str(path))
    assert got.shape == (3, 4, 4) and got.dtype == torch.float32
    for g, p in zip(got, poses):
        want = p.copy()
        want[:3, 1] *= -1
        want[:3, 2] *= -1
        assert np.array_equal(g.numpy(), want.astype(np.float32))
        assert np.array_equal(g.numpy()[:, 0], p[:, 0].astype(np.float32)) and np.array_equal(g.numpy()[:, 3], p[:, 3].astype(np.float32))
    bad = tmp_path / "bad.txt"
    bad.write_text("1 2 3\n")
    with pytest.raises(ValueError, match="16 numbers"):
        R.load_replica_traj(str(bad))
    empty = tmp_path / "empty.txt"
    empty.write_text("\n")
    with pytest.raises(ValueError, match="no pose"):
        R.load_replica_traj(str(empty))


def test_command_line_arguments():
    base = ["--config", "c.yaml", "--mesh", "scene.ply", "--num_iter", "200", "--result_dir", "out"]
    a = R.parse_args(base)
    assert (a.config, a.mesh, a.num_iter, a.result_dir) == ("c.yaml", "scene.ply", 200, "out")
    assert a.start is None and a.traj is None and not a.no_active_ray and a.seed == 0 and a.planner == {} and a.dataset == "NARUTO"
    a = R.parse_args(base + ["--start", "1", "2.5", "-0.5", "--no_active_ray", "--seed", "9", "--planner", "max_rot_deg=30", "gs_z_levels=[12]",
                             "local_planner_method=RRTNaruto"])
    assert a.start == [1.0, 2.5, -0.5] and a.no_active_ray and a.seed == 9
    assert a.planner == {"max_rot_deg": 30, "gs_z_levels": [12], "local_planner_method": "RRTNaruto"}
    assert R.parse_args(base + ["--traj", "traj.txt"]).traj == "traj.txt"
    for bad in (base[:-2], base[:4] + ["--num_iter", "0", "--result_dir", "out"], base + ["--traj", "t.txt", "--start", "0", "0", "0"],
                ["--config", "c.yaml", "--mesh", "scene.obj", "--num_iter", "3", "--result_dir", "out"]):
        with pytest.raises(SystemExit):
            R.parse_args(bad)
    with pytest.raises(ValueError, match="key=value"):
        R.parse_args(base + ["--planner", "max_rot_deg"])
    # every planner key the command line can set is one the planner knows
    from naruto_amd.planner import DEFAULTS
    assert {"max_rot_deg", "gs_z_levels", "rrt_max_iter", "voxel_size", "step_size"} <= set(DEFAULTS)


def test_run_refuses_a_missing_source_of_poses():
    with pytest.raises(ValueError, match="planner or a predefined trajectory"):
        R.run_exploration(None, None, None, torch.eye(4), 3)
    with pytest.raises(ValueError, match="2 poses"):
        R.run_exploration(None, None, None, None, 3, traj=torch.eye(4)[None].repeat(2, 1, 1))


def test_camera_rays_table():
    """((i - cx)/fx, -(j - cy)/fy, -1) for column i, row j: x right, y up, looking along -z."""
    d = camera_rays(3, 4, 2.0, 4.0, 1.0, 0.5)
    assert d.shape == (3, 4, 3) and d.dtype == torch.float32 and d.is_contiguous()
    assert d[2, 3].tolist() == [1.0, -0.375, -1.0] and d[0, 0].tolist() == [-0.5, 0.125, -1.0]


def test_frame_entry_points_of_the_abi(built_lib):
    """The two new symbols are exported with the declared signatures and validate their arguments before touching the device."""
    from naruto_amd import _lib
    for name, n_args in (("naruto_frame_ingest", 8), ("naruto_keyframe_row", 8)):
        assert hasattr(built_lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
    # uint64 pixel counts, uint64 seed / counter, float depth_trunc, uint32 rays_per_kf: the widths the header declares
    assert _lib.SIGNATURES["naruto_frame_ingest"][1][0] is C.c_uint64 and _lib.SIGNATURES["naruto_frame_ingest"][1][4] is C.c_float
    assert [C.sizeof(t) for t in _lib.SIGNATURES["naruto_keyframe_row"][1]] == [8, 8, 8, 4, 8, 8, 8, 8]
    assert built_lib.naruto_frame_ingest(16, None, None, None, 1.0, None, None, None) != 0
    assert b"NULL" in built_lib.naruto_last_error()
    one = C.c_void_p(16)                                # never dereferenced: the size checks come first
    assert built_lib.naruto_frame_ingest(0, one, one, one, 1.0, one, one, None) != 0
    assert built_lib.naruto_keyframe_row(None, 16, None, 4, 0, 0, None, None) != 0
    assert built_lib.naruto_keyframe_row(one, 16, None, 0, 0, 0, one, None) != 0
    assert b"out of range" in built_lib.naruto_last_error()
    header = open(_lib.HEADER).read()
    assert "naruto_frame_ingest(" in header and "naruto_keyframe_row(" in header
    assert "naruto_frame.hip" in _lib.SOURCES

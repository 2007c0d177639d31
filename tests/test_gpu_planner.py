"""GPU tests of the planner on the device: naruto_goal_search (csrc/naruto_planner.hip) against the numpy restatement
tests/planner_spec.py in every bit, the recorded goal searches and main() trajectories of the reference's own NarutoPlanner
(tests/golden/g14_planner_traj_*.npz) through NarutoPlannerHIP, and one closed loop with MeshSimHIP without recordings."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import planner_spec as PS
from test_planner_host import BOUND, TRAJECTORIES, load

pytestmark = pytest.mark.gpu

GUARD = 16


def _search(gpu, agg, coll, tgt, gidx, obs, bbox_min, voxel):
    from naruto_amd import planner as P
    return P.goal_search(torch.from_numpy(agg).to(gpu), torch.from_numpy(coll).to(gpu), torch.from_numpy(tgt).to(gpu), torch.from_numpy(gidx).to(gpu), obs,
                         bbox_min, voxel, guard=GUARD)


def _same(got, want, what=""):
    """Every integer output, the values and the look-at locations equal in every bit; the guard tail intact."""
    assert got["goal"] == want["goal"], (what, got["goal"], want["goal"])
    assert np.array_equal(got["goal_vxl"], want["goal_vxl"]), what
    assert got["n_lookat"] == want["n_lookat"], (what, got["n_lookat"], want["n_lookat"])
    for k in ("lookat_idx", "lookat_vxl"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert np.array_equal(got["lookat_val"].view(np.uint32), want["lookat_val"].view(np.uint32)), (what, got["lookat_val"], want["lookat_val"])
    assert got["lookat_loc"].dtype == np.float64 and np.array_equal(got["lookat_loc"].view(np.uint64), want["lookat_loc"].view(np.uint64)), what
    assert len(got["guard"]) == GUARD and (got["guard"] == -1).all(), (what, got["guard"])


def _problem(G, K, seed, levels=6):
    """Few distinct values (ties everywhere: in the aggregated volume and inside every row), many exact zeros."""
    rs = np.random.RandomState(seed)
    coll = (rs.randint(0, levels, size=(G, K)) * (rs.uniform(size=(G, K)) < 0.4) / 4.0).astype(np.float32)
    agg = coll.sum(1).astype(np.float32)
    tgt = rs.randint(0, 200, size=(K, 3)).astype(np.int32)
    gidx = rs.randint(0, 200, size=(G, 3)).astype(np.int32)
    return agg, coll, tgt, gidx


BBOX_MIN, VOXEL = np.array([-1.2, 0.3, -0.45]), 0.1


@pytest.mark.parametrize("G", [30, 2100, 5000])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 300])
def test_goal_search_equals_the_spec_in_every_bit(gpu, G, K):
    """G below one wave, the office_0 size and above one workgroup's stride; K around the wave size; obs_per_goal 1, 10 and >= K."""
    agg, coll, tgt, gidx = _problem(G, K, 100 * K + G)
    for obs in (1, 10, K + 7):
        got, want = _search(gpu, agg, coll, tgt, gidx, obs, BBOX_MIN, VOXEL), PS.goal_search(agg, coll, tgt, gidx, obs, BBOX_MIN, VOXEL)
        assert len(got["lookat_idx"]) == min(obs, K)
        _same(got, want, (G, K, obs))


def test_goal_search_ties_zero_rows_and_the_last_partial_wave(gpu):
    G, K = 2100, 65                                            # 2100 = 32 waves and 52 lanes of the 33rd
    _, coll, tgt, gidx = _problem(G, K, 7)
    base = np.zeros(G, dtype=np.float32)
    # tied maxima at the first, the middle and the last goal; a unique maximum in the last partial wave; one at the very end
    for where, goal in (((0, 1050, 2099), 0), ((1050, 2099), 1050), ((2099,), 2099), ((2048 + 5,), 2053), ((1023, 1024), 1023), ((2047, 2048, 2099), 2047)):
        agg = base.copy()
        agg[list(where)] = 3.5
        got = _search(gpu, agg, coll, tgt, gidx, 10, BBOX_MIN, VOXEL)
        assert got["goal"] == goal, (where, got["goal"])
        _same(got, PS.goal_search(agg, coll, tgt, gidx, 10, BBOX_MIN, VOXEL), where)
    # everything zero: goal 0; a winning row that is all zero keeps ONE look-at target, the first
    got = _search(gpu, base, coll * 0, tgt, gidx, 10, BBOX_MIN, VOXEL)
    assert got["goal"] == 0 and got["n_lookat"] == 1 and list(got["lookat_idx"]) == list(range(10))
    _same(got, PS.goal_search(base, coll * 0, tgt, gidx, 10, BBOX_MIN, VOXEL), "zeros")
    # fewer positives than obs_per_goal, tied values inside the row (index ascending among equals)
    agg = base.copy()
    agg[77] = 1.0
    c2 = coll.copy()
    c2[77] = 0.0
    c2[77, [64, 3, 40, 9]] = [2.0, 1.0, 2.0, 1.0]
    got = _search(gpu, agg, c2, tgt, gidx, 10, BBOX_MIN, VOXEL)
    assert got["goal"] == 77 and got["n_lookat"] == 4 and list(got["lookat_idx"][:6]) == [40, 64, 3, 9, 0, 1]
    _same(got, PS.goal_search(agg, c2, tgt, gidx, 10, BBOX_MIN, VOXEL), "few positives")
    # the key's order: NaN above +inf, -0 below +0, negative values below zero
    agg = base.copy() - 1.0
    agg[[5, 9]] = [-0.0, 0.0]
    assert _search(gpu, agg, coll, tgt, gidx, 3, BBOX_MIN, VOXEL)["goal"] == 9
    agg[[2000, 2098]] = [np.inf, np.nan]
    got = _search(gpu, agg, coll, tgt, gidx, 3, BBOX_MIN, VOXEL)
    assert got["goal"] == 2098
    _same(got, PS.goal_search(agg, coll, tgt, gidx, 3, BBOX_MIN, VOXEL), "nan")


def test_goal_search_refuses_empty_problems(gpu, built_lib):
    from naruto_amd import _lib, planner as P
    agg, coll, tgt, gidx = (torch.from_numpy(a).to(gpu) for a in _problem(30, 5, 1))
    out = torch.full((8 + 11 * 5 + GUARD,), -1, dtype=torch.int32, device=gpu)
    box = (C.c_double * 3)(0.0, 0.0, 0.0)
    call = lambda G, K, obs: built_lib.naruto_goal_search(G, K, agg.data_ptr(), coll.data_ptr(), tgt.data_ptr(), gidx.data_ptr(), obs, box, 0.1, out.data_ptr(), None)  # noqa: E731
    for G, K, obs in ((0, 5, 3), (30, 0, 3), (30, 5, 0), (30, _lib.GOAL_SEARCH_MAX_TARGETS + 1, 3)):
        assert call(G, K, obs) == -22, (G, K, obs)
        assert b"goal_search" in built_lib.naruto_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()                         # a refused call writes nothing
    with pytest.raises(_lib.NarutoError):
        P.goal_search(agg, coll, tgt, gidx, 0, [0, 0, 0], 0.1)
    with pytest.raises(ValueError):
        P.goal_search(agg.double(), coll, tgt, gidx, 3, [0, 0, 0], 0.1)
    assert call(30, 5, 3) == 0


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_recorded_goal_searches_through_the_kernel(gpu, name):
    """g14 (b): goal_vxl and the look-at locations equal the reference's."""
    rec = load("traj_" + name)
    cfg = json.loads(str(rec["planner"]))
    off = np.concatenate([[0], np.cumsum(rec["gs_lookat_len"])])
    for i in range(len(rec["gs_agg"])):
        got = _search(gpu, rec["gs_agg"][i], rec["gs_coll"][i], rec["gs_targets"][i].astype(np.int32), rec["goal_idx"], cfg["obs_per_goal"], rec["bbox"][:, 0],
                      float(rec["voxel_size"]))
        want = rec["gs_lookat_xyz"][off[i]:off[i + 1]]
        assert np.array_equal(got["goal_vxl"], rec["gs_goal_vxl"][i]) and got["n_lookat"] == len(want)
        assert np.array_equal(got["lookat_loc"][:len(want)].view(np.uint64), want.view(np.uint64))


# ---- g14 (c): the recorded trajectories through NarutoPlannerHIP -------------------------------------------------------------------
class StubSim:
    """The recording's simulator: a 4 x 8 distance map with the scripted minimum and number of invalid pixels."""

    def __init__(self, dist, invalid):
        self.dist, self.invalid, self.calls = dist, invalid, 0

    def simulate(self, c2w, return_erp=False, no_print=False):
        i = min(self.calls, len(self.dist) - 1)
        self.calls += 1
        erp = np.full(32, 1.5, dtype=np.float32)
        erp[0] = self.dist[i]
        erp[1:1 + int(self.invalid[i])] = 1e8
        return None, None, None, erp.reshape(4, 8)


def _run_recorded(rec, gpu, on_device):
    from naruto_amd.planner import NarutoPlannerHIP
    targets = iter(rec["agg_targets"])
    p = NarutoPlannerHIP(json.loads(str(rec["planner"])), dataset=str(rec["dataset"]), device=gpu, select_targets=lambda uncert: next(targets))
    p.update_sim(StubSim(rec["sim_dist"], rec["sim_invalid"]))
    p.init_data(rec["bbox"].tolist())
    p.init_local_planner()
    vol = (lambda a: torch.from_numpy(a).to(gpu)) if on_device else (lambda a: a)
    sdf, versions = vol(rec["sdf"]), [vol(u) for u in rec["uncert_versions"]]
    np.random.seed(int(rec["seed"]))
    pose = rec["start_pose"].copy()
    states, poses, paths = [], [], []
    for step in range(len(rec["states"])):
        p.update_step(step)
        pose = p.main([versions[int(rec["vol_id"][step])], sdf], pose, bool(rec["is_new_vols"][step])).numpy()
        states.append(p.state)
        poses.append(pose)
        paths.append(np.array([n._xyz_arr for n in (p.path or [])], dtype=np.float64).reshape(-1, 3))
    assert next(targets, None) is None                             # as many aggregations as the reference made
    return states, np.stack(poses), paths, p


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_recorded_trajectories_through_the_planner(gpu, name):
    """Recorded targets, the stub simulator, the recorded numpy seed: every step's state equals the recording, every path node for node
    (coordinates to 1e-12, as for the RRT's own fixtures), every pose within the bound; a second run -- volumes as device tensors --
    gives the same bits."""
    rec = load("traj_" + name)
    states, poses, paths, p = _run_recorded(rec, gpu, on_device=False)
    want = [PS.STATES[s] for s in rec["states"]]
    first = next((i for i, (a, b) in enumerate(zip(states, want)) if a != b), None)
    assert first is None, (first, states[first], want[first])
    off = np.concatenate([[0], np.cumsum(rec["path_len"])])
    for step, path in enumerate(paths):
        ref = rec["path_xyz"][off[step]:off[step + 1]]
        assert path.shape == ref.shape, (step, path.shape, ref.shape)
        assert path.size == 0 or float(np.abs(path - ref).max()) <= 1e-12, step
    diff = float(np.abs(poses.astype(np.float64) - rec["poses"].astype(np.float64)).max())
    print(name, "planner vs recorded poses: max abs diff", diff)
    assert poses.dtype == np.float32 and diff <= BOUND
    if name == "mask":
        assert isinstance(p.traversability_mask, np.ndarray) and 0 < p.traversability_mask.sum() < p.traversability_mask.size
    states2, poses2, paths2, _ = _run_recorded(rec, gpu, on_device=True)
    assert states2 == states and np.array_equal(poses2.view(np.uint32), poses.view(np.uint32))
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(paths, paths2))


# ---- one closed loop without recordings ----------------------------------------------------------------------------------------------
WALL_X, WALL_Y0 = 3.53, 3.7                                         # a thin wall x = 3.53, y >= 3.7, floor to ceiling


def _room_with_wall():
    import cull_spec as CS
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    w = np.array([[WALL_X, WALL_Y0, 0.0], [WALL_X, 5.0, 0.0], [WALL_X, 5.0, 3.0], [WALL_X, WALL_Y0, 3.0]], dtype=v.dtype)
    wf = np.array([[0, 1, 2], [0, 2, 3], [0, 2, 1], [0, 3, 2]], dtype=f.dtype) + len(v)            # both windings
    return np.concatenate([v, w]), np.concatenate([f, wf])


def _room_sdf(with_wall):
    """The room's signed distance in voxels (0.1 m) on the 61 x 51 x 31 lattice, quantised to 2^-6: six walls and the sphere, and, when
    asked, the thin wall."""
    import cull_spec as CS
    x, y, z = np.meshgrid(*(np.arange(n) * 0.1 for n in (61, 51, 31)), indexing="ij")
    c, hi = CS.ROOM_CENTRE, CS.ROOM_HI
    d = np.minimum.reduce([x, hi[0] - x, y, hi[1] - y, z, hi[2] - z, np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - CS.ROOM_RADIUS])
    if with_wall:
        d = np.minimum(d, np.sqrt((x - WALL_X) ** 2 + np.maximum(WALL_Y0 - y, 0.0) ** 2))
    return (np.round(d / 0.1 * 64.0) / 64.0).astype(np.float32)


def test_closed_loop_with_the_mesh_simulator(gpu):
    """NarutoPlannerHIP (dataset NARUTO) with MeshSimHIP on the simulator tests' room mesh plus a thin wall the first SDF volume does not
    know about; a static quantised SDF volume and an uncertainty blob on the far wall; 40 steps.  Every pose stays inside the room,
    every transition is one the state machine allows, the planner enters `staying` at the wall (the simulator sees it 3 cm ahead) and
    never passes it; after fresh volumes that contain the wall it plans around it or reports the goal unreachable.

    Run: timeout -k 10 120 python -m pytest "tests/test_gpu_planner.py::test_closed_loop_with_the_mesh_simulator" -m gpu -q
    """
    import cull_spec as CS
    from naruto_amd.planner import NarutoPlannerHIP
    from naruto_amd.simulator import MeshSimHIP
    sim = MeshSimHIP(_room_with_wall(), CS.camera(40, 30, 30.0), erp_hw=(32, 64), face_w=32, far=100.0)
    p = NarutoPlannerHIP(dataset="NARUTO", device=gpu, gs_z_levels=[12], max_rot_deg=30, rrt_max_iter=2000)
    p.update_sim(sim)
    p.init_data([[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]])
    p.init_local_planner()
    assert (p.Nx, p.Ny, p.Nz) == (61, 51, 31)
    uncert = np.zeros((61, 51, 31), dtype=np.float32)
    uncert[59, 36:47, 8:19] = (1 + np.arange(121).reshape(11, 11) % 37) / 8.0                  # on the far wall, in the corner behind the thin wall
    uncert = torch.from_numpy(uncert).to(gpu)
    blind, aware = torch.from_numpy(_room_sdf(False)).to(gpu), torch.from_numpy(_room_sdf(True)).to(gpu)
    np.random.seed(5)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = [2.0, 4.0, 1.2]
    states, poses, fresh_at = [], [pose], None
    for step in range(40):
        p.update_step(step)
        fresh = step == 0 or (fresh_at is None and len(states) >= 3 and states[-3:] == ["staying"] * 3)
        if fresh and step > 0:
            fresh_at = step
        sdf = blind if fresh_at is None else aware
        pose = p.main([uncert, sdf], pose, fresh).numpy()
        states.append(p.state)
        poses.append(pose)
    print("closed loop:", "".join("m" if s == "movingToGoal" else s[0] for s in states), "fresh volumes at", fresh_at)
    xyz = np.stack(poses)[:, :3, 3].astype(np.float64)
    assert np.isfinite(np.stack(poses)).all()
    assert (xyz > 0.05).all() and (xyz < np.array([6.0, 5.0, 3.0]) - 0.05).all()
    for a, b in zip(["staying"] + states[:-1], states):
        assert b in PS.ALLOWED[a], (a, b)
    # it set out towards the far wall, and stopped in front of the thin one
    assert states[0] == "planning" and "movingToGoal" in states and fresh_at is not None
    stopped = states.index("staying")
    assert states[stopped - 1] == "movingToGoal" and WALL_X - 0.2 < xyz[stopped + 1, 0] < WALL_X and xyz[stopped + 1, 1] > WALL_Y0
    for a, b in zip(xyz[:-1], xyz[1:]):                                 # no step crosses the wall's rectangle
        if (a[0] - WALL_X) * (b[0] - WALL_X) < 0:
            t = (WALL_X - a[0]) / (b[0] - a[0])
            assert a[1] + t * (b[1] - a[1]) < WALL_Y0, (a, b)
    # after the fresh volumes: a new plan, and either a way round (rotating towards it next) or "unreachable" (staying)
    assert fresh_at + 1 < len(states) and states[fresh_at] == "planning"
    assert states[fresh_at + 1] in ("rotationPlanningAtStart", "staying")

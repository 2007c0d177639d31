"""CPU tests of the planner's host side (naruto_amd/planner.py) against the recordings of the reference's own NarutoPlanner,
rotation_planning and compute_camera_pose (tests/golden/g14_planner_*.npz, made by tools/make_planner_golden.py) and against the
numpy restatement tests/planner_spec.py.

Bound: poses and rotation matrices within 1e-12 absolute -- fp64 quaternion arithmetic of a few dozen operations on entries of
magnitude <= 1, against scipy's; the measured maximum is stored in each fixture as ``max_abs_diff``."""
import json
import os

import numpy as np
import pytest

import planner_spec as PS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAJECTORIES = ["direct", "mask", "collision"]
BOUND = 1e-12


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"g14_planner_{name}.npz")))


@pytest.fixture(scope="module")
def rotations():
    return load("rotations")


def rotation_cases(rec):
    off = np.concatenate([[0], np.cumsum(rec["planned_len"])])
    for i in range(len(rec["A"])):
        n = int(rec["n_targets"][i])
        yield rec["A"][i], rec["B"][i, :n], rec["R0"][i], float(rec["max_rot_deg"][i]), rec["cam"][i, :n], rec["planned"][off[i]:off[i + 1]]


def test_fixture_covers_the_cases_it_should(rotations):
    """One and several targets, a hop below max_rot_deg, a hop that is no multiple of it, the vertical look-at edge, no hop within a
    degree of 180; the trajectories: a direct one, one with the second run() and the mask, one that stays after a collision."""
    hops_all, vertical = [], 0
    for A, B, R0, deg, cam, planned in rotation_cases(rotations):
        hops = PS.hop_degrees(R0, cam)
        hops_all += [(h, deg) for h in hops]
        vertical += int(((B - A)[:, :2] == 0).all(axis=1).any())
    assert {1} <= set(rotations["n_targets"]) and max(rotations["n_targets"]) >= 5
    assert any(h < d for h, d in hops_all) and any(h > d and abs(h / d - round(h / d)) > 0.05 for h, d in hops_all)
    assert vertical >= 2 and max(h for h, _ in hops_all) < 179.0
    assert float(rotations["max_abs_diff"]) <= BOUND
    direct, mask, col = (load("traj_" + n) for n in TRAJECTORIES)
    assert direct["plan_reachable"].all() and not direct["col_result"].any() and PS.STATES.index("rotatingAtGoal") in direct["states"]
    assert (mask["plan_second_run"] & ~mask["plan_reachable"]).any() and mask["plan_reachable"][-1]
    assert col["col_result"].sum() == 1 and (col["states"] == PS.STATES.index("staying")).sum() > 2
    for rec in (direct, mask, col):
        assert 40 <= len(rec["states"]) <= 80 and rec["sdf"].shape == (24, 28, 17)
        u = rec["uncert_versions"]
        assert np.array_equal(u * 64, np.round(u * 64)) and u.max() < 8


def test_spec_equals_the_recorded_rotations(rotations):
    worst = 0.0
    for A, B, R0, deg, cam, planned in rotation_cases(rotations):
        mine_c = [PS.camera_pose(A.copy(), b.copy()) for b in B]
        mine = PS.plan_rotations(R0, mine_c, deg)
        assert len(mine) == len(planned)
        worst = max([worst] + [float(np.abs(a - b).max()) for a, b in zip(mine_c + mine, list(cam) + list(planned))])
    print("spec vs recorded rotations: max abs diff", worst)
    assert worst <= BOUND


def test_package_rotations_equal_the_spec_bit_for_bit_and_the_recordings(rotations):
    from naruto_amd import planner as P
    worst = 0.0
    for A, B, R0, deg, cam, planned in rotation_cases(rotations):
        got_c = [P.compute_camera_pose(A.copy(), b.copy()) for b in B]
        want_c = [PS.camera_pose(A.copy(), b.copy()) for b in B]
        got, want = P.rotation_planning(R0, got_c, deg), PS.plan_rotations(R0, want_c, deg)
        assert len(got) == len(want) == len(planned)
        for a, b in zip(got_c + got, want_c + want):
            assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        worst = max([worst] + [float(np.abs(a - b).max()) for a, b in zip(got_c + got, list(cam) + list(planned))])
    print("package vs recorded rotations: max abs diff", worst)
    assert worst <= BOUND
    A = np.array([0.5, 0.5, 0.5])
    P.compute_camera_pose(A, np.array([0.5, 0.5, 1.0]))
    assert np.array_equal(A, [0.5, 0.5, 0.5])                      # the nudge of the vertical edge stays inside


def test_package_needs_neither_scipy_nor_mmengine():
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "naruto_amd", "planner.py")).read()
    assert "import scipy" not in src and "from scipy" not in src and "import mmengine" not in src


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_spec_equals_the_recorded_trajectories(name):
    rec = load("traj_" + name)
    states, poses = PS.replay(rec)
    assert np.array_equal(states, rec["states"])
    assert poses.dtype == rec["poses"].dtype == np.float32
    diff = float(np.abs(poses.astype(np.float64) - rec["poses"].astype(np.float64)).max())
    print(name, "spec vs recorded poses: max abs diff", diff)
    assert diff <= BOUND
    for a, b in zip(rec["states"][:-1], rec["states"][1:]):
        assert PS.STATES[b] in PS.ALLOWED[PS.STATES[a]]


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_spec_goal_search_equals_the_recorded_goal_searches(name):
    rec = load("traj_" + name)
    cfg = json.loads(str(rec["planner"]))
    off = np.concatenate([[0], np.cumsum(rec["gs_lookat_len"])])
    for i in range(len(rec["gs_agg"])):
        r = PS.goal_search(rec["gs_agg"][i], rec["gs_coll"][i], rec["gs_targets"][i], rec["goal_idx"], cfg["obs_per_goal"], rec["bbox"][:, 0], float(rec["voxel_size"]))
        want = rec["gs_lookat_xyz"][off[i]:off[i + 1]]
        assert np.array_equal(r["goal_vxl"], rec["gs_goal_vxl"][i]) and r["n_lookat"] == len(want)
        assert np.array_equal(r["lookat_loc"][:r["n_lookat"]].view(np.uint64), want.view(np.uint64))


def test_spec_goal_search_tie_rules():
    agg = np.array([1, 5, 5, 2, 5], dtype=np.float32)
    coll = np.zeros((5, 6), dtype=np.float32)
    coll[1] = [2, 3, 3, 0, 2, 3]
    tgt = np.arange(18).reshape(6, 3)
    r = PS.goal_search(agg, coll, tgt, np.arange(15).reshape(5, 3), 4, np.zeros(3), 0.1)
    assert r["goal"] == 1 and list(r["lookat_idx"]) == [1, 2, 5, 0] and r["n_lookat"] == 4
    r = PS.goal_search(np.zeros(5, np.float32), coll * 0, tgt, np.arange(15).reshape(5, 3), 4, np.zeros(3), 0.1)
    assert r["goal"] == 0 and list(r["lookat_idx"]) == [0, 1, 2, 3] and r["n_lookat"] == 1
    assert PS.goal_search(np.array([0.0, -0.0, np.nan, np.inf], np.float32), np.ones((4, 1), np.float32), tgt[:1], np.zeros((4, 3)), 1, np.zeros(3), 1.0)["goal"] == 2


# ---- the state machine of NarutoPlannerHIP with stubbed planning, collision and simulator pieces ----------------------------------
class _Node:
    def __init__(self, xyz):
        self._xyz_arr = np.asarray(xyz, dtype=np.float64)


def _stubbed(rec):
    from naruto_amd.planner import NarutoPlannerHIP
    cfg = json.loads(str(rec["planner"]))
    p = NarutoPlannerHIP(cfg, dataset=str(rec["dataset"]), device="cpu")
    p.init_data(rec["bbox"].tolist())
    plans, cols = iter(range(len(rec["plan_reachable"]))), iter(rec["col_result"])
    p_off, l_off = np.concatenate([[0], np.cumsum(rec["plan_path_len"])]), np.concatenate([[0], np.cumsum(rec["plan_lookat_len"])])

    def planning(vols, cur_pose):
        i = next(plans)
        assert p.step == int(rec["plan_step"][i])
        return dict(path=[_Node(x) for x in rec["plan_path_xyz"][p_off[i]:p_off[i + 1]]], is_goal_reachable=bool(rec["plan_reachable"][i]),
                    lookat_tgts=[x for x in rec["plan_lookat_xyz"][l_off[i]:l_off[i + 1]]])

    def collision(sdf_vol, cur_pose, next_pt_loc):
        return bool(next(cols))
    p.uncertainty_aware_planning_v2, p.detect_collision_v2 = planning, collision
    return p


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_state_machine_follows_the_recorded_trajectories(name):
    """States equal, the path and the look-at list after every step equal, poses within the bound; main returns float32 [4,4]."""
    rec = load("traj_" + name)
    p = _stubbed(rec)
    assert p.state == "staying"
    pose = rec["start_pose"].copy()
    p_off, l_off = np.concatenate([[0], np.cumsum(rec["path_len"])]), np.concatenate([[0], np.cumsum(rec["lookat_len"])])
    worst = 0.0
    for step in range(len(rec["states"])):
        p.update_step(step)
        new = p.main([None, None], pose, bool(rec["is_new_vols"][step]))
        assert tuple(new.shape) == (4, 4) and str(new.dtype) == "torch.float32"
        new = new.numpy()
        assert p.state == PS.STATES[rec["states"][step]], (step, p.state)
        worst = max(worst, float(np.abs(new.astype(np.float64) - rec["poses"][step].astype(np.float64)).max()))
        path = np.array([n._xyz_arr for n in (p.path or [])]).reshape(-1, 3)
        assert np.array_equal(path, rec["path_xyz"][p_off[step]:p_off[step + 1]])
        assert np.array_equal(np.array(p.lookat_tgts or []).reshape(-1, 3), rec["lookat_xyz"][l_off[step]:l_off[step + 1]])
        pose = new
    print(name, "state machine vs recorded poses: max abs diff", worst)
    assert worst <= BOUND


def test_unknown_state_and_dataset_are_refused():
    from naruto_amd.planner import NarutoPlannerHIP
    p = NarutoPlannerHIP(device="cpu")
    p.init_data([[0, 1], [0, 1], [0, 1]])
    p.state = "dancing"
    with pytest.raises(NotImplementedError):
        p.main([None, None], np.eye(4, dtype=np.float32), False)
    q = NarutoPlannerHIP(dataset="ScanNet", device="cpu")
    q.init_data([[0, 1], [0, 1], [0, 1]])
    with pytest.raises(NotImplementedError):
        q.detect_collision_v2(None, np.eye(4, dtype=np.float32), np.zeros(3))
    with pytest.raises(NotImplementedError):
        NarutoPlannerHIP(local_planner_method="RRT", device="cpu").init_local_planner()
    with pytest.raises(TypeError):
        NarutoPlannerHIP(no_such_key=1)


def test_config_defaults_equal_the_recorded_defaults(rotations):
    from naruto_amd.planner import DEFAULTS, NarutoPlannerHIP
    want = json.loads(str(rotations["default_planner"]))
    assert len(want) >= 20
    cfg = NarutoPlannerHIP(device="cpu").planner_cfg
    for key, value in want.items():
        got = cfg[key]
        got = list(got) if isinstance(got, tuple) else got
        assert got == value and type(got) is type(value), (key, got, value)
    assert set(DEFAULTS) - set(want) == {"collision_thre"}            # the one .get() default of the reference's class
    # a whole config: planner + general.dataset; keyword arguments win
    p = NarutoPlannerHIP({"planner": {"obs_per_goal": 3, "max_rot_deg": 5}, "general": {"dataset": "MP3D"}}, max_rot_deg=7, device="cpu")
    assert (p.planner_cfg.obs_per_goal, p.planner_cfg.max_rot_deg, p.dataset, p.planner_cfg.uncert_top_k) == (3, 7, "MP3D", 4000)


def test_vox_loc_round_trip_is_the_reference_expression():
    from naruto_amd.planner import NarutoPlannerHIP
    p = NarutoPlannerHIP(device="cpu")
    p.init_data([[-1.2, 1.2], [-1.4, 1.4], [-0.4, 1.3]])
    assert (p.Nx, p.Ny, p.Nz) == (25, 29, 18)
    v = np.array([3, 7, 11])
    assert np.array_equal(p.vox2loc(v), v * 0.1 + np.array([-1.2, -1.4, -0.4]))
    assert np.array_equal(p.loc2vox(p.vox2loc(v)), (v * 0.1 + np.array([-1.2, -1.4, -0.4]) - np.array([-1.2, -1.4, -0.4])) / 0.1)

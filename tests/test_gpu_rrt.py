"""GPU tests of the planner's RRT on the device (naruto_amd.rrt, naruto_rrt.hip) against the fixtures recorded from the reference's
own RRTNaruto (tests/golden/g12_rrt_*.npz) and against the numpy restatement tests/rrt_spec.py.  "The same tree" means: node count,
parents, rrt_iter, reachable flags and path EXACTLY, float64 coordinates to 1e-12."""
import os

import numpy as np
import pytest
import torch

import rrt_spec as RS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["a", "b", "c", "d", "e"]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"g12_rrt_{name}.npz")))


def planner(rec, **kw):
    from naruto_amd.rrt import RRTNarutoHIP
    args = dict(bbox=rec["bbox"], voxel_size=float(rec["voxel_size"]), max_iter=int(rec["max_iter"]), step_size=float(rec["step_size"]), maxz=int(rec["maxz"]),
                step_amplifier=float(rec["step_amplifier"]), collision_thre=float(rec["collision_thre"]), enable_direct_line=bool(rec["direct"]))
    args.update(kw)
    return RRTNarutoHIP(**args)


def replay(rec, p, vol=None, seeded=False):
    """Drive the device planner through the fixture's calls.  seeded: numpy's global stream from the fixture's seed, as the reference ran;
    else the recorded rows, call by call.  -> reachable flags."""
    if seeded:
        np.random.seed(int(rec["seed"]))
    p.start_new_plan(rec["start"], rec["goal"], rec["vol"] if vol is None else vol)
    used, flags = 0, []
    for c, upto in zip(rec["calls"], rec["rows_after_call"]):
        pts = None if seeded else rec["rows"][used:int(upto)]
        if c == 0:
            flags.append(p.run(points=pts))
        else:
            p.run_full(points=pts)
        used = int(upto)
    return flags


def check_tree(rec, p, flags):
    RS.same_tree(rec, p.n_nodes, p.parents(), p.nodes_xyz(), p.rrt_iter, flags, p.path_indices() if "path" in rec else None)


_D64 = {}


def check_mask(rec, p):
    m = p.get_reachable_mask()
    assert m.dtype == np.float32 and m.shape == rec["mask"].shape and set(np.unique(m)) <= {0.0, 1.0}
    key = int(rec["seed"]), len(rec["parents"])
    if key not in _D64:                                     # the fixture's nodes' float64 distance to every voxel, once per fixture
        _D64[key] = RS.replay_fixture(rec)[0].reachable_mask()[1]
    d64 = _D64[key]
    band = np.abs(d64 - float(rec["step_size"])) <= 1e-4
    print(f"mask: {int(band.sum())} of {band.size} voxels in the band, {int((m != rec['mask']).sum())} differ in all, {int((m != rec['mask'])[~band].sum())} outside it")
    assert band.mean() <= 0.005, int(band.sum())
    assert np.array_equal(m[~band], rec["mask"][~band])


@pytest.mark.parametrize("name", SCENES)
def test_device_builds_the_reference_tree_from_the_recorded_rows(gpu, name):
    rec = load(name)
    p = planner(rec)
    flags = replay(rec, p)
    check_tree(rec, p, flags)
    if "path" in rec:
        path = p.find_path()
        assert path[0] is p.goal and len(path) == len(rec["path"]) + 1
        assert np.array_equal(np.stack([n._xyz_arr for n in path[1:]]), p.nodes_xyz()[rec["path"]])
        assert path[-1].parent is None and all(a.parent is b for a, b in zip(path[:-1], path[1:]))
        assert np.array_equal(path[-1]._xyz_arr, rec["start"]) and path[1].get_xyz().dtype == torch.float32 and path[1].x == path[1]._xyz_arr[0]
    if "mask" in rec:
        check_mask(rec, p)


@pytest.mark.parametrize("name", SCENES)
def test_device_seeded_like_the_reference_makes_its_tree_and_leaves_its_random_state(gpu, name):
    rec = load(name)
    p = planner(rec)
    flags = replay(rec, p, seeded=True)
    check_tree(rec, p, flags)
    after = np.random.uniform(size=3)
    np.random.seed(int(rec["seed"]))                       # the reference's loop: three scalar draws per extension
    lo = [rec["x_range"][0], rec["y_range"][0], rec["z_range"][0]] if rec["calls"][0] == 0 else [0, 0, 0]
    hi = [rec["x_range"][1], rec["y_range"][1], rec["z_range"][1]] if rec["calls"][0] == 0 else [48, 55, 34]
    rows = np.array([[np.random.uniform(lo[a], hi[a]) for a in range(3)] for _ in range(len(rec["rows"]))]).reshape(-1, 3)
    assert np.array_equal(rows, rec["rows"])
    assert np.array_equal(after, np.random.uniform(size=3))


def test_segments_equal_the_reference(gpu):
    from naruto_amd.rrt import segments_collision_free, is_collision_free
    seg = load("segments")
    cnt, comp = segments_collision_free(seg["pa"], seg["pb"], seg["vol"], float(seg["step_size"]), float(seg["collision_thre"]))
    assert cnt.dtype == torch.int32 and comp.dtype == torch.bool
    assert np.array_equal(cnt.cpu().numpy(), seg["num_collision_free"]) and np.array_equal(comp.cpu().numpy(), seg["complete_free"])
    for i in (0, 1, 2, int(np.argmin(seg["num_collision_free"])), int(np.argmax(seg["num_collision_free"]))):       # the planner's own signature
        assert is_collision_free(seg["pa"][i], seg["pb"][i], seg["vol"], step_size=float(seg["step_size"]), collision_thre=float(seg["collision_thre"])) == \
            (int(seg["num_collision_free"][i]), bool(seg["complete_free"][i]))
    # a numpy volume is uploaded once per array object, a new array replaces it
    from naruto_amd import rrt
    kept = rrt._uploaded["vol"]
    assert rrt._uploaded["host"] is seg["vol"] and kept is not None
    is_collision_free(seg["pa"][3], seg["pb"][3], seg["vol"])
    assert rrt._uploaded["vol"] is kept
    other = seg["vol"] * 0 + 100
    assert is_collision_free(seg["pa"][3], seg["pb"][3], other)[1] is True and rrt._uploaded["host"] is other
    # other step sizes and thresholds against the spec (long segments: several passes of the wave)
    rng = np.random.RandomState(5)
    pa, pb = rng.uniform(2, 30, size=(300, 3)), rng.uniform(2, 30, size=(300, 3))
    for step, thre in ((0.25, 0.5), (2.0, 1.5), (1.0, -1.0)):
        cnt, comp = segments_collision_free(pa, pb, seg["vol"], step, thre)
        want = [RS.collision_free(a, b, seg["vol"], step, thre) for a, b in zip(pa, pb)]
        assert cnt.cpu().tolist() == [w[0] for w in want] and comp.cpu().tolist() == [w[1] for w in want]


def test_second_run_continues_the_tree(gpu):
    rec = load("c")
    p = planner(rec)
    p.start_new_plan(rec["start"], rec["goal"], rec["vol"])
    k = int(rec["rows_after_call"][0])
    assert p.run(points=rec["rows"][:k]) is False
    n1 = p.n_nodes
    assert n1 == int(rec["nodes_after_call"][0]) and p.rrt_iter == 300
    first = p.nodes_xyz().copy()
    assert p.run(points=rec["rows"][k:]) is False
    assert p.n_nodes == int(rec["nodes_after_call"][1]) > n1 and p.rrt_iter == 600
    assert np.array_equal(p.nodes_xyz()[:n1], first)
    p.start_new_plan(rec["start"], rec["goal"], rec["vol"])                 # a new plan starts over
    assert p.n_nodes == 1 and p.rrt_iter == 0 and np.array_equal(p.nodes_xyz()[0], rec["start"]) and p.parents().tolist() == [-1]


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_capacity_stop_does_not_change_the_tree(gpu, name):
    rec = load(name)
    p = planner(rec)
    p.initial_capacity = 2                                  # the first append already asks for room; doubled again and again
    flags = replay(rec, p)
    check_tree(rec, p, flags)
    assert p._cap >= p.n_nodes and p._cap < 4 * p.n_nodes
    if "mask" in rec:
        check_mask(rec, p)


def test_chunk_boundary_at_every_position(gpu):
    rec = load("b")
    p = planner(rec)
    p.chunk_first, p.chunk_growth = 1, 1                    # one row per launch: a stop for rows before every extension
    check_tree(rec, p, replay(rec, p))
    for first in range(1, len(rec["rows"]) + 2):            # one boundary, at every position in turn (and one past the end)
        p.chunk_first, p.chunk_growth = first, 1000
        check_tree(rec, p, replay(rec, p))
    p = planner(rec)
    p.chunk_first, p.chunk_growth = 1, 1                    # the same with numpy's stream: state restored and re-drawn at every stop
    check_tree(rec, p, replay(rec, p, seeded=True))
    rec = load("c")                                         # two run() calls of 300 rows, boundaries every 7 rows
    p = planner(rec)
    p.chunk_first, p.chunk_growth = 7, 1
    check_tree(rec, p, replay(rec, p))


def test_cell_lists_and_plain_scan_grow_the_same_tree(gpu):
    """A run_full long enough to cross the cell-list threshold several times over: the spec (a plain scan) against the device with the default
    threshold, with the cell lists from the first node on, and with the plain scan throughout."""
    from naruto_amd import _lib
    rec = load("d")
    n_iter = 4000
    np.random.seed(99)
    rows = RS.draw_rows(n_iter, [0, 0, 0], [48, 55, 34])
    s = RS.SpecRRT(rec["vol"], 1.0, 10, 0.5, True)
    s.start_new_plan(rec["start"], rec["goal"])
    s.run_full(rows, n_iter)
    assert s.n > 2 * _lib.RRT_CELL_THRESHOLD, s.n
    print(f"spec: {s.n} nodes, smallest margin {s.marg.smallest:.3g} {s.marg.by_kind}")
    masks = []
    for thr in (0, 1, 1 << 30):
        p = planner(rec, max_iter=n_iter, cell_threshold=thr)
        p.start_new_plan(rec["start"], rec["goal"], rec["vol"])
        p.run_full(points=rows)
        assert p.n_nodes == s.n and np.array_equal(p.parents(), np.array(s.parent, dtype=np.int32)), thr
        err = float(np.abs(p.nodes_xyz() - s.nodes_xyz()).max())
        print(f"cell_threshold {thr}: largest coordinate difference to the spec {err:.3g}")
        assert err <= 1e-12, thr
        assert p.rrt_iter == 0
        masks.append(p.get_reachable_mask())
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], masks[2]) and 0 < masks[0].sum() < masks[0].size


@pytest.mark.parametrize("name", ["a", "b", "c", "e"])
def test_run_over_the_cell_lists_builds_the_reference_tree(gpu, name):
    """run() with the nearest-node search over the cell lists from the second node on: the random extension between direct lines, the early
    exit and the search for goal.parent after the loop all go through the cells, against the fixtures recorded from the reference."""
    rec = load(name)
    p = planner(rec, cell_threshold=1)
    check_tree(rec, p, replay(rec, p))
    if "mask" in rec:
        check_mask(rec, p)
    q = planner(rec, cell_threshold=1 << 30)                # and never: the plain scan throughout
    check_tree(rec, q, replay(rec, q))
    assert np.array_equal(p.nodes_xyz(), q.nodes_xyz())


def test_off_grid_behaviours(gpu):
    from naruto_amd.rrt import segments_collision_free
    rec = load("e")
    vol = rec["vol"]                                        # free everywhere: only the grid's edge blocks
    hi = np.array(vol.shape, dtype=np.float64) - 1.0
    # 1. a sample outside [0, dim-1] counts as blocked
    pa = np.array([[10.0, 10.0, 10.0], [10.0, 10.0, 10.0], [-0.5, 10.0, 10.0], [10.0, 10.0, 10.0]])
    pb = np.array([[10.0, 10.0, 37.0], [10.0, 58.2, 10.0], [5.0, 10.0, 10.0], [np.nan, 10.0, 10.0]])
    cnt, comp = segments_collision_free(pa, pb, vol)
    want = [RS.collision_free(a, b, vol) for a, b in zip(pa, pb)]
    got = cnt.cpu().tolist()
    assert got == [w[0] for w in want] and 20 <= got[0] <= 24 and 40 <= got[1] <= 45 and got[2:] == [-1, -1] and not comp.any()
    # 2. at exactly dim-1 the upper corner has weight 0 and its index is clamped: free, and complete up to the very corner
    pa = np.array([[40.0, 50.0, 30.0], hi - 3.0, [48.0, 0.0, 0.0]])
    pb = np.array([[48.0, 50.0, 30.0], hi, [48.0, 55.0, 34.0]])
    cnt, comp = segments_collision_free(pa, pb, vol)
    want = [RS.collision_free(a, b, vol) for a, b in zip(pa, pb)]
    assert cnt.cpu().tolist() == [w[0] for w in want] and comp.all() and all(w[1] for w in want)
    # the grower: a goal outside the grid is never reached and nothing leaves the grid
    p = planner(rec, max_iter=40)
    p.start_new_plan([20.5, 30.25, 10.0], [20.5, 30.25, 40.0], vol)
    np.random.seed(1)
    assert p.run() is False and p.rrt_iter == 40
    x = p.nodes_xyz()
    assert p.n_nodes > 40 and (x >= 0).all() and (x <= hi).all()
    # a start outside the grid, no direct line: every segment from it is blocked at its first sample, the tree stays the start node
    p = planner(rec, max_iter=25, enable_direct_line=False)
    p.start_new_plan([-2.0, 30.25, 10.0], [20.5, 30.25, 10.0], vol)
    assert p.run() is False and p.n_nodes == 1 and p.rrt_iter == 25 and p.path_indices().tolist() == [0]
    assert p.get_reachable_mask().sum() == 0
    # with the direct line (counted from the goal's end, so nodes ARE laid from the off-grid start): the spec's tree, by the plain scan
    np.random.seed(2)
    rows = RS.draw_rows(60, [0, 0, 0], [48, 55, 28])
    s = RS.SpecRRT(vol, 1.0, 10, 0.5, True)
    s.start_new_plan([-2.0, 30.25, 10.0], [20.5, 41.5, 13.0])
    ok, used = s.run(rows, 60)
    p = planner(rec, max_iter=60)
    p.start_new_plan([-2.0, 30.25, 10.0], [20.5, 41.5, 13.0], vol)
    assert p.run(points=rows[:used]) == ok and p.n_nodes == s.n and p.rrt_iter == s.rrt_iter
    assert np.array_equal(p.parents(), np.array(s.parent, dtype=np.int32)) and np.abs(p.nodes_xyz() - s.nodes_xyz()).max() <= 1e-12
    assert p.path_indices().tolist() == s.path() and (p.nodes_xyz()[:, 0] < 0).any()
    # 3. a start within rounding of the goal: reached at once, the start is the goal's parent
    p = planner(rec)
    p.start_new_plan([20.5, 30.25, 10.0], [20.5, 30.25, 10.0], vol)
    assert p.run() is True and p.n_nodes == 1 and p.rrt_iter == 1 and p.path_indices().tolist() == [0]
    path = p.find_path()
    assert len(path) == 2 and path[0] is p.goal and path[0].parent is path[1] and np.array_equal(path[1]._xyz_arr, [20.5, 30.25, 10.0])


def test_lds_tile_mask_equals_the_cell_list_mask(gpu):
    """The mask kernel's two routes on the same nodes: over the cell lists, and (after the plan's cell lists are switched off) node tiles."""
    from naruto_amd import _lib
    rec = load("c")
    p = planner(rec)
    replay(rec, p)
    a = p.get_reachable_mask()
    assert int(p._ws[_lib.RRT_STATE_USE_CELLS].item()) == 1
    b = p.get_reachable_mask(use_cell_lists=False)
    assert int(p._ws[_lib.RRT_STATE_USE_CELLS].item()) == 1          # the plan's own state is put back
    assert np.array_equal(a, b) and np.array_equal(a, p.get_reachable_mask(use_cell_lists=True)) and 0 < a.sum() < a.size


def test_device_tensor_volume_equals_numpy_volume(gpu):
    rec = load("b")
    p = planner(rec)
    check_tree(rec, p, replay(rec, p, vol=torch.from_numpy(rec["vol"]).to(gpu)))
    q = planner(rec)
    check_tree(rec, q, replay(rec, q, vol=torch.from_numpy(rec["vol"]).to(gpu).double()))       # any float dtype: converted on the device
    assert np.array_equal(p.nodes_xyz(), q.nodes_xyz())
    from naruto_amd.rrt import segments_collision_free
    seg = load("segments")
    a = segments_collision_free(seg["pa"], seg["pb"], torch.from_numpy(seg["vol"]).to(gpu))
    b = segments_collision_free(torch.from_numpy(seg["pa"]).to(gpu), torch.from_numpy(seg["pb"]).to(gpu), seg["vol"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[0].cpu().numpy(), seg["num_collision_free"])


def test_eval_bookkeeping(gpu):
    rec = load("a")
    p = planner(rec, enable_eval=True)
    flags = replay(rec, p)
    path = p.find_path()
    p.update_eval(False, 0.5, path)
    assert p.eval_results["rrt_iter"] == []
    p.update_eval(flags[0], 0.25, path)
    assert p.eval_results == {"time (ms)": [250.0], "node_num": [p.n_nodes], "rrt_iter": [1]}

    class Printer:
        lines = []

        def __call__(self, s):
            self.lines.append(s)

        def adjust_string_length(self, n, s):
            return s.ljust(n)
    p.print_eval_result(Printer())
    assert len(Printer.lines) == 4 and "250.00" in Printer.lines[1]

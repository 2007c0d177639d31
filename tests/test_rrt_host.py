"""CPU tests of the planner's RRT: the numpy restatement (tests/rrt_spec.py) against every fixture recorded from the reference's
own RRTNaruto (tests/golden/g12_rrt_*.npz, tools/make_rrt_golden.py), the host's draw of the reference's random stream, and the
argument validation of the C entry points."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import rrt_spec as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["a", "b", "c", "d", "e"]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"g12_rrt_{name}.npz")))


def test_no_fixture_is_left_out():
    have = sorted(os.path.basename(p)[len("g12_rrt_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "g12_rrt_*.npz")))
    assert have == sorted(SCENES + ["segments"])
    for p in glob.glob(os.path.join(GOLDEN, "g12_rrt_*.npz")):
        assert os.path.getsize(p) < 1_000_000, p


@pytest.mark.parametrize("name", SCENES)
def test_spec_builds_the_reference_tree(name):
    rec = load(name)
    s, flags = RS.replay_fixture(rec)
    RS.same_tree(rec, s.n, s.parent, s.nodes_xyz(), s.rrt_iter, flags, s.path())
    # what makes the demand fair: no decision of this run hangs on the last bits (see the docstring of rrt_spec)
    assert s.marg.smallest >= RS.NEED and float(rec["min_margin"]) >= RS.NEED, s.marg.by_kind
    if "mask" in rec:
        m, d64 = s.reachable_mask()
        band = np.abs(d64 - float(rec["step_size"])) <= 1e-4
        assert band.mean() <= 0.005, int(band.sum())
        assert np.array_equal(m[~band], rec["mask"][~band])


def test_scenes_are_what_they_claim():
    a, b, c, d, e = (load(n) for n in SCENES)
    for r in (a, b, c, d, e):
        assert r["vol"].shape == (49, 56, 35) and r["vol"].dtype == np.float32
    assert a["reachable"].tolist() == [True] and int(a["rrt_iter"]) == 1 and len(a["rows"]) == 0                   # the direct line alone
    assert b["reachable"].tolist() == [True] and len(b["rows"]) > 20                                               # random extensions were needed
    assert c["reachable"].tolist() == [False, False] and int(c["rrt_iter"]) == 600 and len(c["nodes_after_call"]) == 2
    assert c["nodes_after_call"][1] > c["nodes_after_call"][0]                                                    # the second run() continued the tree
    assert d["calls"].tolist() == [1] and int(d["rrt_iter"]) == 0 and len(d["rows"]) == 1500 and len(d["parents"]) > 2048
    assert np.all(e["vol"] == 100.0) and e["reachable"].tolist() == [True]
    assert e["start"][2] == e["goal"][2]                                                                          # numpy's zero-step form of linspace


def test_spec_segments_match_the_reference():
    seg = load("segments")
    assert len(seg["pa"]) == 2000
    for a, b, n, c in zip(seg["pa"], seg["pb"], seg["num_collision_free"], seg["complete_free"]):
        assert RS.collision_free(a, b, seg["vol"], float(seg["step_size"]), float(seg["collision_thre"])) == (int(n), bool(c))
    assert seg["num_collision_free"].min() == -1 and seg["complete_free"].any() and not seg["complete_free"].all()


def test_chunked_draw_leaves_numpys_state_where_a_scalar_loop_does():
    from naruto_amd.rrt import RowSource
    lo, hi = [1, 2, 0], [47, 53.5, 28]

    def scalar_loop(n):                                  # generate_random_point, n times
        return np.array([[np.random.uniform(lo[a], hi[a]) for a in range(3)] for _ in range(n)]).reshape(-1, 3)

    for consumed in ([64, 100], [0], [64, 256, 0], [5], [64, 256, 1024, 1]):
        np.random.seed(7)
        src, got, chunk = RowSource(lo, hi), [], 64
        for used in consumed:
            rows = src.draw(chunk)
            assert rows.shape == (chunk, 3)
            got.append(rows[:used])
            src.settle(used)
            chunk *= 4
        state = np.random.get_state()
        after = np.random.uniform(size=4)
        np.random.seed(7)
        want = scalar_loop(sum(consumed))
        ref_state = np.random.get_state()
        assert np.array_equal(np.concatenate(got), want)
        assert state[0] == ref_state[0] and np.array_equal(state[1], ref_state[1]) and state[2:] == ref_state[2:]
        assert np.array_equal(after, np.random.uniform(size=4))
        assert src.taken == sum(consumed)
    # the spec's own draw (what the GPU tests feed both sides) is the same stream as the host's chunks
    np.random.seed(11)
    want = RS.draw_rows(9, lo, hi)
    np.random.seed(11)
    src = RowSource(lo, hi)
    first = src.draw(5).copy()
    src.settle(5)
    assert np.array_equal(np.concatenate([first, src.draw(4)]), want)
    # an explicit array is handed out in slices and touches no random state
    pts = np.arange(30, dtype=np.float64).reshape(10, 3)
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    src = RowSource(lo, hi, pts)
    assert np.array_equal(src.draw(4), pts[:4])
    src.settle(3)
    assert np.array_equal(src.draw(100), pts[3:]) and not src.exhausted()
    src.settle(7)
    assert src.exhausted() and np.array_equal(np.random.get_state()[1], before)


def test_rrt_entry_points_validate_arguments(built_lib):
    from naruto_amd import _lib
    lib = built_lib
    assert lib.naruto_rrt_workspace((C.c_uint32 * 3)(0, 4, 4)) == 0
    assert lib.naruto_rrt_workspace((C.c_uint32 * 3)(2048, 2048, 2048)) == 0
    assert lib.naruto_rrt_workspace((C.c_uint32 * 3)(4, 5, 6)) >= 4 * 120 + 64
    start, goal = (C.c_double * 3)(1, 1, 1), (C.c_double * 3)(2, 2, 2)
    assert lib.naruto_rrt_start(None, start, goal, None) == -22 and b"NULL plan" in lib.naruto_last_error()
    p = _lib.NarutoRrtPlan()
    p.dims = (C.c_uint32 * 3)(4, 5, 6)
    p.step_size, p.step_amplifier, p.collision_thre = 1.0, 10.0, 0.5
    p.capacity = 16
    for a in range(3):
        p.range[a][1] = p.full_range[a][1] = 3.0
    assert lib.naruto_rrt_start(C.byref(p), start, goal, None) == -22 and b"NULL buffer" in lib.naruto_last_error()
    fake = 4096                                            # validation comes before anything is dereferenced or launched
    p.sdf_vol = p.workspace = p.nodes_xyz = p.nodes_xyz32 = p.parent = p.next = fake
    assert lib.naruto_rrt_start(C.byref(p), None, goal, None) == -22 and b"NULL start" in lib.naruto_last_error()
    assert lib.naruto_rrt_start(C.byref(p), (C.c_double * 3)(1, float("nan"), 1), goal, None) == -22
    assert lib.naruto_rrt_grow(C.byref(p), 7, None, 0, 10, 1, None) == -22 and b"mode" in lib.naruto_last_error()
    assert lib.naruto_rrt_grow(C.byref(p), _lib.RRT_MODE_RUN, None, 5, 10, 1, None) == -22 and b"NULL rows" in lib.naruto_last_error()
    assert lib.naruto_rrt_path(C.byref(p), None, None) == -22
    assert lib.naruto_reachable_mask(C.byref(p), None, None) == -22 and b"NULL mask" in lib.naruto_last_error()
    p.capacity = 0
    assert lib.naruto_rrt_grow(C.byref(p), _lib.RRT_MODE_RUN, None, 0, 10, 1, None) == -22 and b"capacity" in lib.naruto_last_error()
    p.capacity = 16
    p.step_size = 0.0
    assert lib.naruto_rrt_grow(C.byref(p), _lib.RRT_MODE_FULL, None, 0, 10, 1, None) == -22 and b"step_size" in lib.naruto_last_error()
    p.step_size = 1.0
    p.range[2][0] = 9.0
    assert lib.naruto_rrt_grow(C.byref(p), _lib.RRT_MODE_FULL, None, 0, 10, 1, None) == -22 and b"range" in lib.naruto_last_error()
    dims = (C.c_uint32 * 3)(4, 5, 6)
    assert lib.naruto_segments_free(dims, None, 1, None, None, 1.0, 0.5, None, None, None) == -22 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_segments_free(dims, fake, 1, fake, fake, -1.0, 0.5, fake, fake, None) == -22 and b"step_size" in lib.naruto_last_error()
    assert lib.naruto_segments_free((C.c_uint32 * 3)(0, 5, 6), fake, 1, fake, fake, 1.0, 0.5, fake, fake, None) == -22
    assert lib.naruto_segments_free(dims, fake, 0, fake, fake, 1.0, 0.5, fake, fake, None) == 0          # nothing to do, nothing launched


def test_planner_class_mirrors_the_reference_attributes():
    from naruto_amd.rrt import RRTNarutoHIP
    import naruto_amd
    assert naruto_amd.RRTNarutoHIP is RRTNarutoHIP and naruto_amd.rrt.is_collision_free
    p = RRTNarutoHIP(bbox=np.array([[0.0, 4.8], [0.0, 5.5], [0.0, 3.4]]), voxel_size=0.1, step_size=1.0, maxz=28, step_amplifier=10, margin=2, device="cpu")
    assert p.vol_shape == (49, 56, 35) and p.max_iter == 96040
    assert (p.x_range, p.y_range, p.z_range) == ([2, 46], [2, 53], [2, 28])
    assert (p.full_x_range, p.full_y_range, p.full_z_range) == ([0, 48], [0, 55], [0, 34])
    assert p.rrt_iter == 0 and set(p.eval_results) == {"time (ms)", "node_num", "rrt_iter"}
    assert RRTNarutoHIP(bbox=np.array([[0.0, 4.8], [0.0, 5.5], [0.0, 3.4]]), voxel_size=0.1, maxz=28, z_levels=[5, 11], max_iter=7, device="cpu").z_range == [5, 11]

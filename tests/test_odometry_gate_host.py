"""The odometry prior's scored starts and verdict without a GPU: the numpy twin (tests/odometry_gate_spec.py) over the study the design
rests on (DESIGN 7m prints these tables), and the C ABI's argument checks (nothing is launched).

The study.  Scene A: 160 x 120 from OS.CASE_POSITION looking at the room's centre; scene B: 80 x 60 at (0.5, 1.0, 1.5) looking at
(3.0, 1.0, 0.2).  True motions: yaw +18 / -18 degrees about y, 0.1 m along OS.CASE_ALONG, both together, none, 5 degrees about
(0.3, -0.8, 0.5) with 0.03 m (the six), yaw 40 (the choice), yaw 10 and 0.05 m (the verdict).  Starts: the identity, yaw +18, yaw -18, the
0.1 m translation, yaw +36.  An estimate CONVERGED when it is within OS.BOUND_M / OS.BOUND_DEG of the true motion, else it is LOST.

Run: python -m pytest tests/test_odometry_gate_host.py -q -s
"""
import ctypes as C
import math

import numpy as np
import pytest

import cull_spec as CS
import odometry_gate_spec as GS
import odometry_rgbd_spec as RS
import odometry_spec as OS
import sim_spec as SS

Y = (0.0, 1.0, 0.0)
SCENES = {"A": (CS.camera(160, 120, 120.0), OS.CASE_POSITION, CS.ROOM_CENTRE), "B": (CS.camera(80, 60, 60.0), (0.5, 1.0, 1.5), (3.0, 1.0, 0.2))}
SIX = {"yaw +18": OS.relative_motion(Y, 18.0, OS.CASE_ALONG, 0.0), "yaw -18": OS.relative_motion(Y, -18.0, OS.CASE_ALONG, 0.0),
       "0.1 m": OS.relative_motion(Y, 0.0, OS.CASE_ALONG, 0.1), "yaw +18, 0.1 m": OS.relative_motion(Y, 18.0, OS.CASE_ALONG, 0.1),
       "none": np.eye(4), "5 deg, 0.03 m": OS.relative_motion((0.3, -0.8, 0.5), 5.0, OS.CASE_ALONG, 0.03)}
CHOICE_TRUTHS = dict(SIX, **{"yaw +40": OS.relative_motion(Y, 40.0, OS.CASE_ALONG, 0.0)})
VERDICT_TRUTHS = dict(SIX, **{"yaw +10": OS.relative_motion(Y, 10.0, OS.CASE_ALONG, 0.0), "0.05 m": OS.relative_motion(Y, 0.0, OS.CASE_ALONG, 0.05)})
TRUTHS = dict(CHOICE_TRUTHS, **VERDICT_TRUTHS)
STARTS = {"identity": np.eye(4), "yaw +18": SIX["yaw +18"], "yaw -18": SIX["yaw -18"], "0.1 m": SIX["0.1 m"],
          "yaw +36": OS.relative_motion(Y, 36.0, OS.CASE_ALONG, 0.0)}


def _look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64))
    p[:3, 3] = pos
    return p


class Study:
    """Maps and estimates of the study, each made once and shared by the tests (never changed)."""

    def __init__(self):
        self.mesh = CS.room_mesh(n_lat=8, n_lon=16)
        self._maps, self._est = {}, {}

    def maps(self, scene, rel, key=None):
        key = (scene, key if key is not None else np.asarray(rel).tobytes())
        if key not in self._maps:
            cam, pos, at = SCENES[scene]
            pose = (_look(pos, at) @ rel).astype(np.float32)
            self._maps[key] = OS.frame_maps(CS.render_depth(self.mesh[0], self.mesh[1], pose[None], cam, near=0.01, far=100.0)[0], cam)
        return self._maps[key]

    def estimate(self, scene, truth, start):
        """The estimate of TRUTHS[truth] in ``scene`` from STARTS[start] with its level-0 verdict figures (a K = 1 gated estimate)."""
        key = (scene, truth, start)
        if key not in self._est:
            cam = SCENES[scene][0]
            out = GS.estimate_gated(self.maps(scene, np.eye(4)), self.maps(scene, TRUTHS[truth]), cam, STARTS[start][None])
            out.error = OS.motion_error(out.estimate, TRUTHS[truth])
            out.converged = out.error[0] <= OS.BOUND_M and out.error[1] <= OS.BOUND_DEG
            self._est[key] = out
        return self._est[key]

    def start_costs(self, scene, truth, trunc=GS.SCORE_TRUNC):
        """The cost of each of the five starts at the coarsest level (five K = 1 scores: the sums of a candidate do not depend on the others)."""
        cam = SCENES[scene][0]
        prev, cur = self.maps(scene, np.eye(4)), self.maps(scene, TRUTHS[truth])
        return {s: GS.costs(GS.score(T[None], cam, 2, prev, cur, trunc), 1, trunc)[0] for s, T in STARTS.items()}


@pytest.fixture(scope="module")
def study():
    return Study()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- cross-checks
def test_score_equals_the_accumulate_twins_in_every_bit(study):
    cam = SCENES["B"][0]
    prev, cur = study.maps("B", np.eye(4)), study.maps("B", SIX["5 deg, 0.03 m"])
    cams = OS.level_intrinsics(cam, 3)
    md = float(np.float32(0.25))
    for level in (0, 1, 2):
        for T in (np.eye(4), SIX["5 deg, 0.03 m"], SIX["yaw -18"]):
            _, _, terms = OS.rows(T, cams[level], prev[level], cur[level])
            want = OS.reduce_sums(terms)
            got = GS.score(T[None], cam, level, prev, cur, md)
            assert want[28] > 0 and got[0] >= got[1]
            assert np.array_equal(_bits(got[1:3]), _bits(want[[28, 27]])), (level, got, want[27:])
            assert not got[3:].any()
    # RGB-D blocks: [1], [3], [4] are the RGB-D accumulate's [29], [30], [31]
    Hh, W = 40, 56
    dp, dc, cp, cc = RS.drawn_pair(Hh, W, 3)
    camd = CS.camera(W, Hh, float(W))
    mp, mc = RS.frame_maps(dp, cp, camd), RS.frame_maps(dc, cc, camd)
    T = OS.relative_motion((0.3, -0.8, 0.5), 1.0, OS.CASE_ALONG, 0.02)
    for level in (0, 1):
        lc = OS.level_intrinsics(camd, 3)[level]
        want = RS.reduce_sums(RS.rows_rgbd(T, lc, mp[0][level], mc[0][level], mp[1][level], mc[1][level])[4])
        got = GS.score(T[None], camd, level, mp, mc, md, photo_weight=RS.PHOTO_WEIGHT)
        assert want[29] > 0 and want[30] > 0
        assert np.array_equal(_bits(got[[1, 3, 4]]), _bits(want[[29, 30, 31]])), (level, got, want[29:])
        off = GS.score(T[None], camd, level, mp, mc, md, photo_weight=0.0)
        assert np.array_equal(_bits(off[1:3]), _bits(got[1:3])) and not off[3:].any()


def test_trunc_below_a_residual_truncates(study):
    cam = SCENES["B"][0]
    prev, cur = study.maps("B", np.eye(4)), study.maps("B", SIX["0.1 m"])
    lc = OS.level_intrinsics(cam, 3)[2]
    gi, gr, _ = OS.rows(np.eye(4), lc, prev[2], cur[2])
    r = np.abs(gr[gi >= 0])
    assert len(r) > 50
    edge = float(np.sort(r)[len(r) // 2])                  # a residual of the frame itself as trunc: r^2 = trunc^2 exactly for that row
    terms = GS.score_terms(np.eye(4)[None], lc, prev[2], cur[2], edge)
    rr = gr * gr
    want = np.where(gi >= 0, np.minimum(rr, edge * edge), 0.0)
    assert np.array_equal(_bits(terms[:, 2]), _bits(want))
    assert (rr[gi >= 0] > edge * edge).sum() > 0 and (rr[gi >= 0] == edge * edge).sum() >= 1 and (rr[gi >= 0] < edge * edge).sum() > 0
    full = GS.score(np.eye(4)[None], cam, 2, prev, cur, float(np.float32(0.25)))
    cut = GS.score(np.eye(4)[None], cam, 2, prev, cur, edge)
    assert cut[1] == full[1] and cut[2] < full[2] and cut[2] <= edge * edge * cut[1]


# ---------------------------------------------------------------------------------------------------------------- the choice
def test_the_lowest_cost_start_converges_in_every_case(study):
    wrong = []
    for scene in SCENES:
        for truth in CHOICE_TRUTHS:
            cost = study.start_costs(scene, truth)
            cost01 = study.start_costs(scene, truth, 0.1)
            pick = min(cost, key=cost.get)                                  # dicts keep the order: ties go to the first
            conv = {s: study.estimate(scene, truth, s).converged for s in STARTS}
            print(f"scene {scene} truth {truth:15s}: " + "  ".join(f"{s} {cost[s]:.3f}{'+' if conv[s] else '-'}" for s in STARTS) +
                  f"  -> {pick}; tau 0.1 -> {min(cost01, key=cost01.get)}")
            assert any(conv.values()), (scene, truth, "no start converges")
            if not conv[pick]:
                wrong.append((scene, truth, pick))
    assert not wrong, wrong


def test_neither_fixed_policy_is_safe_and_the_scored_start_recovers(study):
    """Finding 1: scene A, truth yaw -18, after a +18 turn: "always last motion" is lost; scene B, truth yaw -18: "always identity" is lost."""
    for scene, truth, losing, last in (("A", "yaw -18", "yaw +18", "yaw +18"), ("B", "yaw -18", "identity", "yaw -18")):
        lost = study.estimate(scene, truth, losing)
        print(f"scene {scene} truth {truth} from {losing}: {lost.error[0] * 1e3:.3f} mm {lost.error[1]:.4f} deg")
        assert not lost.converged
        cam = SCENES[scene][0]
        out = GS.estimate_gated(study.maps(scene, np.eye(4)), study.maps(scene, TRUTHS[truth]), cam, np.stack([np.eye(4), STARTS[last]]))
        dm, dd = OS.motion_error(out.T, TRUTHS[truth])
        print(f"  scored start {out.chosen} (costs {out.costs}): {dm * 1e3:.3f} mm {dd:.4f} deg, passed {out.passed}")
        assert out.passed and dm <= OS.BOUND_M and dd <= OS.BOUND_DEG


def test_on_the_wall_every_start_converges_so_the_choice_is_harmless():
    """The RGB-D twin on the textured wall seen head on (tests/test_odometry_rgbd_host.py's scene, 160 x 120): the depth rows are
    degenerate there, the photometric cost still ranks the starts, and whichever start is taken the estimate converges and passes."""
    cam = SCENES["A"][0]
    v, f, c = RS.wall_mesh()
    base = RS.wall_pose()
    poses = np.stack([base] + [base @ rel for rel in RS.WALL_MOTIONS]).astype(np.float32)
    depth, colour, _ = SS.render_rgbd(v, f, c, poses, cam)
    gt = poses.astype(np.float64)
    prev = RS.frame_maps(depth[0], colour[0], cam)
    for k in range(3):
        rel = np.linalg.inv(gt[0]) @ gt[1 + k]
        cur = RS.frame_maps(depth[1 + k], colour[1 + k], cam)
        for cands in (np.stack([np.eye(4), rel]), np.stack([RS.WALL_MOTIONS[(k + 1) % 3], np.eye(4)])):
            out = GS.estimate_gated(prev, cur, cam, cands, photo_weight=RS.PHOTO_WEIGHT)
            dm, dd = OS.motion_error(out.T, rel)
            print(f"wall motion {k}: start {out.chosen} costs {[round(x, 3) for x in out.costs]} -> {dm * 1e3:.4f} mm {dd:.5f} deg, passed {out.passed}, "
                  f"photometric rows {int(out.record[12])}, rmse {out.record[13]:.5f}")
            assert out.passed and dm <= OS.BOUND_M and dd <= OS.BOUND_DEG and out.record[12] > 0
            assert 0.0 <= min(out.costs) and max(out.costs) <= 2.0, "two terms, each at most 1"
        other = GS.estimate_gated(prev, cur, cam, np.stack([np.eye(4), rel])[::-1].copy(), photo_weight=RS.PHOTO_WEIGHT)
        assert other.passed and OS.motion_error(other.T, rel)[0] <= OS.BOUND_M


# ---------------------------------------------------------------------------------------------------------------- the verdict
def test_verdict_confusion_table(study):
    table = {(c, p): 0 for c in (True, False) for p in (True, False)}
    for scene in SCENES:
        for truth in VERDICT_TRUTHS:
            for start in STARTS:
                e = study.estimate(scene, truth, start)
                table[(e.converged, e.passed)] += 1
                r = e.record
                print(f"scene {scene} {truth:15s} from {start:9s}: {'converged' if e.converged else 'LOST     '} {'PASS' if e.passed else 'FAIL'}  "
                      f"overlap {e.overlap:.3f} rmse {r[8] * 1e3:.3f} mm |t| {r[9]:.3f} trace {r[10]:.3f} status {OS.STATUS[int(r[11])]}")
    print(f"converged: {table[(True, True)]} passed, {table[(True, False)]} refused; lost: {table[(False, True)]} passed, {table[(False, False)]} refused")
    assert sum(table.values()) == 80
    assert table[(False, True)] == 0 and table[(True, False)] == 0


def test_forced_failures(study):
    cam = SCENES["B"][0]
    prev = study.maps("B", np.eye(4))
    for deg in (60.0, 90.0):
        rel = OS.relative_motion(Y, deg, OS.CASE_ALONG, 0.0)
        cur = study.maps("B", rel)
        for start in (np.eye(4), STARTS["yaw +36"]):
            out = GS.estimate_gated(prev, cur, cam, start[None])
            assert not out.passed and np.isfinite(out.record).all() and np.array_equal(out.T, start), (deg, out.record)
    zero = OS.frame_maps(np.zeros((cam["H"], cam["W"]), np.float32), cam)
    cands = np.stack([np.eye(4), SIX["yaw +18"]])
    for name, (p, c) in {"current missing": (prev, zero), "previous missing": (zero, prev)}.items():
        out = GS.estimate_gated(p, c, cam, cands)
        assert not out.passed and np.isfinite(out.record).all() and np.array_equal(out.T, cands[out.chosen]), name
        assert out.chosen == 0, "equal costs: the lowest index"
    nan = np.full((4, 4), np.nan)
    cur = study.maps("B", SIX["5 deg, 0.03 m"])
    out = GS.estimate_gated(prev, cur, cam, np.stack([nan, np.eye(4)]))
    assert out.chosen == 1 and out.costs[0] == 1.0 and out.passed, "a NaN candidate has no rows; the good one beside it is taken"
    alone = GS.score(np.eye(4)[None], cam, 2, prev, cur, GS.SCORE_TRUNC)
    assert np.array_equal(_bits(out.coarse[[0, 5, 6]]), _bits(alone[[0, 1, 2]])), "the good candidate's sums are unchanged"
    out = GS.estimate_gated(prev, cur, cam, nan[None])
    assert not out.passed and out.chosen == 0 and np.isfinite(out.record).all() and np.isnan(out.T).all()


def test_a_prior_only_chain_flags_the_jump_alone(study):
    """Ten frames at 80 x 60 from scene A's position: +4 degrees of yaw and 2 cm per frame, a 60-degree jump at frame 5, no motion at frame
    6, then on as before.  est[i] = est[i-1] @ T with the starts {identity, last motion}: the jump is the only FAIL."""
    cam = SCENES["B"][0]
    step, jump = OS.relative_motion(Y, 4.0, OS.CASE_ALONG, 0.02), OS.relative_motion(Y, 60.0, OS.CASE_ALONG, 0.0)
    rels = [step, step, step, step, jump, np.eye(4), step, step, step]
    gt = [_look(OS.CASE_POSITION, CS.ROOM_CENTRE)]
    for r in rels:
        gt.append(gt[-1] @ r)
    mesh = study.mesh
    maps = [OS.frame_maps(CS.render_depth(mesh[0], mesh[1], p.astype(np.float32)[None], cam, near=0.01, far=100.0)[0], cam) for p in gt]
    est, verdicts = [gt[0]], []
    for i in range(1, 10):
        out = GS.estimate_gated(maps[i - 1], maps[i], cam, GS.candidates(est, i))
        dm, dd = OS.motion_error(out.T, rels[i - 1])
        print(f"frame {i}: {'PASS' if out.passed else 'FAIL'} start {out.chosen} costs {[round(c, 3) for c in out.costs]} {dm * 1e3:.3f} mm {dd:.4f} deg")
        verdicts.append(out.passed)
        est.append(est[-1] @ out.T)
        if i == 6:
            assert out.chosen == 0
        if i != 5:
            assert dm <= OS.BOUND_M and dd <= OS.BOUND_DEG, i
    assert verdicts == [i != 5 for i in range(1, 10)]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_arguments_are_refused_before_anything_is_launched():
    from naruto_amd import _lib
    lib = _lib.load()
    assert _lib.ODOM_GATE_WORDS == GS.GATE_WORDS and _lib.ODOM_MAX_CANDS == GS.MAX_CANDS
    desc = _lib.NarutoOdomDesc(H=60, W=80, levels=3, iters=(C.c_uint32 * 4)(10, 5, 4, 0), fx=60.0, fy=60.0, cx=39.5, cy=29.5, max_dist=0.25, jump=0.15, band=0.1)
    d, p = C.byref(desc), 4096                             # p: any non-NULL address; a refused call reads and launches nothing
    assert lib.naruto_odom_score_workspace_bytes(d, 4) == 17 * 8 * 3 and lib.naruto_odom_score_workspace_bytes(d, 1) == 5 * 8 * 3
    for K in (0, 5):
        assert lib.naruto_odom_score_workspace_bytes(d, K) == 0
        assert lib.naruto_odom_score(d, None, 2, p, p, p, K, 0.05, p, p, None) != 0
        assert lib.naruto_odom_choose(K, p, p, 0, 0.05, 0.0, p, p, None) != 0
    assert b"candidates" in lib.naruto_last_error()
    assert lib.naruto_odom_score(d, None, 3, p, p, p, 2, 0.05, p, p, None) != 0 and b"level" in lib.naruto_last_error()
    assert lib.naruto_odom_score(None, None, 0, p, p, p, 2, 0.05, p, p, None) != 0
    for trunc in (0.0, -0.05, math.inf, math.nan):
        assert lib.naruto_odom_score(d, None, 0, p, p, p, 2, trunc, p, p, None) != 0 and b"trunc" in lib.naruto_last_error()
        assert lib.naruto_odom_choose(2, p, p, 0, trunc, 0.0, p, p, None) != 0
    for k in range(5):                                      # maps_prev, maps_cur, cands, sums, workspace
        a = [p] * 5
        a[k] = None
        assert lib.naruto_odom_score(d, None, 0, a[0], a[1], a[2], 2, 0.05, a[3], a[4], None) != 0 and b"NULL" in lib.naruto_last_error()
    bad = _lib.NarutoOdomPhoto(weight=float("nan"), max_diff=0.3)
    assert lib.naruto_odom_score(d, C.byref(bad), 0, p, p, p, 2, 0.05, p, p, None) != 0
    for k in range(4):                                      # sums, cands, state, record
        a = [p] * 4
        a[k] = None
        assert lib.naruto_odom_choose(2, a[0], a[1], 0, 0.05, 0.0, a[2], a[3], None) != 0
        g = _lib.NarutoOdomGate(max_trans=0.3, min_trace=2.7, min_overlap=0.25, max_rmse=0.006)
        assert lib.naruto_odom_verdict(d, C.byref(g), a[0], a[1], a[2], a[3], None) != 0
    assert lib.naruto_odom_choose(2, p, p, 1, 0.05, 0.0, p, p, None) != 0, "a photometric cost needs its tau"
    assert lib.naruto_odom_verdict(d, None, p, p, p, p, None) != 0
    for field, value in (("max_trans", math.nan), ("min_trace", 3.5), ("min_overlap", -0.1), ("max_rmse", math.inf)):
        g = _lib.NarutoOdomGate(max_trans=0.3, min_trace=2.7, min_overlap=0.25, max_rmse=0.006)
        setattr(g, field, value)
        assert lib.naruto_odom_verdict(d, C.byref(g), p, p, p, p, None) != 0 and b"gate" in lib.naruto_last_error()
    assert lib.naruto_odom_candidates(None, 4, 2, p, None) != 0 and lib.naruto_odom_candidates(p, 4, 2, None, None) != 0
    assert lib.naruto_odom_candidates(p, 4, 4, p, None) != 0 and b"frame 4 of 4" in lib.naruto_last_error()


def test_the_python_gate():
    from naruto_amd.odometry import OdometryGate
    g = OdometryGate()
    assert (g.max_trans, g.max_rot_deg, g.min_overlap, g.max_rmse, g.score_trunc) == (GS.MAX_TRANS, GS.MAX_ROT_DEG, GS.MIN_OVERLAP, GS.MAX_RMSE, GS.SCORE_TRUNC)
    assert g.abi().min_trace == GS.gate().min_trace and OdometryGate.of(True) == g and OdometryGate.of(None) == g
    for kw in ({"score_trunc": 0.0}, {"max_rot_deg": 200.0}, {"min_overlap": 1.5}, {"max_rmse": float("nan")}):
        with pytest.raises(ValueError):
            OdometryGate(**kw)
    with pytest.raises(ValueError):
        OdometryGate.of(0.3)

"""The odometry prior's reference ring without a GPU: the numpy twin (tests/odometry_anchor_spec.py) over its rules and over the two
trajectories the design rests on (DESIGN 7o prints these tables), and the argument checks of the Python interface.

Trajectories (80 x 60, f = 60, noise-free depth of cull_spec.room_mesh(8, 16) from OS.CASE_POSITION looking at the room's centre; pose k =
base @ relative_motion(y, A sin(2 pi k / p), CASE_ALONG, B sin(2 pi k / q))): A = 25 frames, 9 degrees, p = 12, 0.04 m, q = 8 (it never
leaves frame 0's view and ends in frame 0's pose); B = 97 frames, 40 degrees, p = 96, 0.25 m, q = 64.

Run: python -m pytest tests/test_odometry_anchor_host.py -q -s
"""
import math

import numpy as np
import pytest

import cull_spec as CS
import odometry_anchor_spec as AS
import odometry_gate_spec as GS
import odometry_spec as OS

CAM = CS.camera(80, 60, 60.0)
# the final twin's ratios anchored / frame-to-frame of (final, mean) translation error with the default policy; the tests
# here and on the GPU bound the ratio by twice these, and never by more than 1
TWIN_RATIOS = {"A": (0.140, 0.172), "B": (0.242, 0.201)}


def ratio_bounds(name):
    return tuple(min(1.0, 2.0 * r) for r in TWIN_RATIOS[name])


def look(pos, at):
    from naruto_amd.planner import compute_camera_pose
    p = np.eye(4)
    p[:3, :3] = compute_camera_pose(np.asarray(pos, np.float64), np.asarray(at, np.float64))
    p[:3, 3] = pos
    return p


class Study:
    """Frames, maps and the twin's two chains per trajectory, each made once and shared (never changed); tests/test_gpu_odometry_anchor.py
    reads the same object."""

    def __init__(self):
        self.mesh = CS.room_mesh(n_lat=8, n_lon=16)
        self.base = look(OS.CASE_POSITION, CS.ROOM_CENTRE)
        self._frames, self._chains = {}, {}

    def frames(self, name):
        """(true poses float32 [n,4,4], depth frames float32 [n,60,80], the twin's maps per frame)."""
        if name not in self._frames:
            truth = AS.trajectory(self.base, *AS.TRAJECTORIES[name])
            depth = CS.render_depth(self.mesh[0], self.mesh[1], truth, CAM, near=0.01, far=100.0).astype(np.float32)
            self._frames[name] = (truth, depth, [OS.frame_maps(d, CAM) for d in depth])
        return self._frames[name]

    def chains(self, name):
        """(gated frame-to-frame chain, anchored chain with the default policy) on the twin."""
        if name not in self._chains:
            truth, _, maps = self.frames(name)
            self._chains[name] = (AS.chain(maps, CAM, truth[0]), AS.chain(maps, CAM, truth[0], pol=AS.policy()))
        return self._chains[name]


_STUDY = None


def shared_study():
    global _STUDY
    if _STUDY is None:
        _STUDY = Study()
    return _STUDY


@pytest.fixture(scope="module")
def study():
    return shared_study()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _poses(n, seed=0):
    rng = np.random.default_rng(seed)
    est = np.zeros((n, 4, 4), np.float32)
    for k in range(n):
        ax = rng.normal(size=3)
        est[k] = OS.relative_motion(ax / np.linalg.norm(ax), 4.0 * k, OS.CASE_ALONG, 0.05 * k)
    return est


# ---------------------------------------------------------------------------------------------------------------- the rules
def test_candidates_of_the_previous_frame_are_the_gates():
    est = _poses(6)
    for i in (1, 2, 5):
        head = AS.new_head(0)
        head[5], head[6] = i - 1, -1                                        # slot 1 holds frame i-1, slot 2 is empty
        c = AS.candidates(est, i, head, 3)
        want = GS.candidates(est, i)
        assert np.array_equal(c[1, 0], np.eye(4)) and np.array_equal(c[2, 0], np.eye(4))
        assert np.array_equal(_bits(c[1, 1]), _bits(c[2, 1])) and np.array_equal(_bits(c[1, 1]), _bits(AS.last_motion(est, i)))
        assert np.abs(c[1] - want).max() < 1e-12                            # GS.candidates inverts with numpy: equal to rounding
        if i > 1:                                                           # slot 0 holds frame 0: inv(est[0]) @ est[i-1], and that times the last motion
            R = np.linalg.inv(est[0].astype(np.float64)) @ est[i - 1].astype(np.float64)
            assert np.abs(c[0, 0] - R).max() < 1e-12 and np.abs(c[0, 1] - R @ want[1]).max() < 1e-12
    assert np.abs(AS.inverse(est[3]) @ est[3].astype(np.float64) - np.eye(4)).max() < 1e-12


def _sums(costs):
    """[slots,9] sums whose K = 2 costs at trunc = 0.05 are about ``costs`` [slots][2]: 100 valid pixels, 100 rows, so cost = s / (100 t2);
    a cost that is not finite is put into s as it is."""
    t2 = 0.05 * 0.05
    out = np.zeros((len(costs), 9))
    for s, pair in enumerate(costs):
        out[s, 0] = 100.0
        for k, c in enumerate(pair):
            out[s, 1 + 4 * k], out[s, 2 + 4 * k] = 100.0, (c * 100.0 * t2 if math.isfinite(c) else c)
    return out


def test_choose_ties_empty_slots_and_infinite_costs():
    cands = np.arange(4 * 2 * 16, dtype=np.float64).reshape(4, 2, 4, 4)
    head = np.array([2, 0, 0, 0, 7, 3, 9, -1] + [-1] * 4, np.int32)         # slots 0, 1, 2 hold frames 7, 3, 9; slot 3 is empty; slot 2 was written last
    # the lowest cost wins; an empty slot's (zero) sums are never looked at
    sums = _sums([(0.5, 0.4), (0.3, 0.6), (0.7, 0.8), (0.0, 0.0)])
    ch = AS.choose(sums, cands, head, 0.05)
    assert (ch.slot, ch.start) == (1, 0) and ch.head[2] == 1 and list(ch.anchor[:3]) == [1.0, 3.0, 3.0]
    assert np.array_equal(ch.cands, cands[1]) and np.array_equal(ch.T, cands[1, 0])
    assert np.array_equal(_bits(ch.record[2:6]), _bits(GS.costs(sums[1], 2, 0.05) + [-1.0, -1.0])) and ch.record[1] == 0.0
    assert ch.anchor[6] == GS.costs(sums[1], 2, 0.05)[0] and ch.anchor[7] == GS.costs(sums[0], 2, 0.05)[1]
    # a tie goes to the larger frame id, whatever the slot order; inside a slot to the lower start
    sums = _sums([(0.25, 0.9), (0.25, 0.9), (0.25, 0.25), (0.0, 0.0)])
    ch = AS.choose(sums, cands, head, 0.05)
    assert (ch.slot, ch.start) == (2, 0) and ch.anchor[1] == 9.0 and ch.anchor[6] == ch.anchor[7]
    head2 = head.copy()
    head2[4], head2[6] = 9, 7
    assert AS.choose(sums, cands, head2, 0.05).slot == 0
    # a cost that is not finite is +inf and loses; all +inf, or no slot with a frame: the slot written last, start 0
    sums = _sums([(math.nan, math.inf), (0.9, math.nan), (math.inf, math.inf), (0.0, 0.0)])
    ch = AS.choose(sums, cands, head, 0.05)
    assert (ch.slot, ch.start) == (1, 0) and ch.anchor[7] == -1.0
    sums = _sums([(math.nan, math.inf)] * 3 + [(0.0, 0.0)])
    ch = AS.choose(sums, cands, head, 0.05)
    assert (ch.slot, ch.start) == (2, 0) and ch.anchor[6] == -1.0 and ch.anchor[7] == -1.0 and ch.anchor[1] == 9.0
    empty = AS.new_head()
    empty[0] = 3
    ch = AS.choose(_sums([(0.1, 0.2)] * 4), cands, empty, 0.05)
    assert (ch.slot, ch.start) == (3, 0) and list(ch.anchor[:3]) == [3.0, -1.0, 0.0]
    empty[0] = 77                                                           # a word that is not a slot reads the last slot
    assert AS.choose(_sums([(0.1, 0.2)] * 4), cands, empty, 0.05).slot == 3


def record(passed, overlap=0.9, t=0.02, rot_deg=2.0):
    r = np.zeros(GS.GATE_WORDS)
    r[0], r[6], r[7], r[9], r[10] = float(passed), 1000.0, 1000.0 * overlap, t, 1.0 + 2.0 * math.cos(math.radians(rot_deg))
    return r


# (record, promoted, the slot written, the streak after): a pass inside the limits; each limit crossed alone; two refusals in a row;
# then, with two slots, three promotions wrap around and overwrite the oldest
SCRIPT = [(record(1), 0, -1, 0), (record(1, overlap=0.69), 1, 1, 0), (record(1, t=0.11), 1, 0, 0), (record(1, rot_deg=10.5), 1, 1, 0),
          (record(0), 0, -1, 1), (record(1), 0, -1, 0), (record(0), 0, -1, 1), (record(0), 1, 0, 0), (record(0), 0, -1, 1), (record(1, t=0.2), 1, 1, 0)]


def run_script(slots=2):
    """The twin over SCRIPT from a ring that holds frame 0 in slot 0; frame i = 1 + the script's index.  -> [(head, anchor, ring)]."""
    pol, head, ring, out = AS.policy(slots=slots), AS.new_head(0), ["maps 0"] + [None] * (slots - 1), []
    for k, (rec, *_) in enumerate(SCRIPT):
        head, anchor = AS.update(pol, 1 + k, rec, head, np.zeros(AS.ANCHOR_WORDS))
        ring = AS.promote(head, ring, f"maps {1 + k}")
        out.append((head, anchor, ring))
    return out


def test_update_and_promote_over_the_script():
    out = run_script(2)
    for k, ((_, promoted, written, streak), (head, anchor, ring)) in enumerate(zip(SCRIPT, out)):
        assert (anchor[3], anchor[4], anchor[5]) == (promoted, written, streak), (k, anchor)
        assert head[3] == promoted and head[1] == streak
        if promoted:
            assert head[0] == written and head[4 + written] == 1 + k and ring[written] == f"maps {1 + k}"
    # slots = 2: frames 2, 3, 4 were promoted in turn into slots 1, 0, 1: frame 0 went first, then frame 2 (the oldest each time)
    assert [list(h[4:6]) for h, _, _ in out[1:4]] == [[0, 2], [3, 2], [3, 4]]
    assert out[-1][0][4:6].tolist() == [8, 10] and out[-1][2] == ["maps 8", "maps 10"] and (out[-1][0][6:] == -1).all()
    # one slot: every promotion lands in slot 0; a refail of 1 promotes every refused frame
    pol = AS.policy(slots=1, refail=1)
    head, anchor = AS.update(pol, 5, record(0), AS.new_head(0), np.zeros(8))
    assert head[:5].tolist() == [0, 0, 0, 1, 5] and anchor[3:6].tolist() == [1.0, 0.0, 0.0]


def test_predict_reads_the_reference_from_the_record():
    est = _poses(5)
    T = OS.relative_motion((0.0, 1.0, 0.0), 3.0, OS.CASE_ALONG, 0.02)
    a = np.zeros(8)
    a[1] = 1.0
    assert np.array_equal(AS.predict(est, 4, a, T), AS.mul(est[1].astype(np.float64), T).astype(np.float32))
    for bad in (-1.0, 4.0, 9.0):                                            # anything outside 0 .. i-1 reads frame i-1
        a[1] = bad
        assert np.array_equal(AS.predict(est, 4, a, T), AS.mul(est[3].astype(np.float64), T).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the trajectories
def report(name, truth, ff, an):
    ef, ea = AS.translation_errors(ff.poses, truth), AS.translation_errors(an.poses, truth)
    print(f"\ntrajectory {name}: {len(truth)} frames")
    print("  chain            final mm   mean mm    max mm  refused  promoted   margin")
    print(f"  frame to frame   {1e3 * ef[0]:8.2f}  {1e3 * ef[1]:8.2f}  {1e3 * ef[2]:8.2f}  {int((ff.prior_log[1:, 0] == 0).sum()):7d}         -  {ff.margin:.2e}")
    print(f"  anchored         {1e3 * ea[0]:8.2f}  {1e3 * ea[1]:8.2f}  {1e3 * ea[2]:8.2f}  {int((an.prior_log[1:, 0] == 0).sum()):7d}  {int(an.anchor_log[:, 3].sum()):8d}  {an.margin:.2e}")
    print(f"  ratio            {ea[0] / ef[0]:8.3f}  {ea[1] / ef[1]:8.3f}")
    print("  frame: reference frame / start / verdict / promoted, where the reference is not the frame before:")
    print("   " + " ".join(f"{i}:{int(an.anchor_log[i, 1])}/{int(an.prior_log[i, 1])}/{int(an.prior_log[i, 0])}/{int(an.anchor_log[i, 3])}"
                          for i in range(1, len(truth)) if int(an.anchor_log[i, 1]) != i - 1))
    return ef, ea


@pytest.mark.parametrize("name", ["A", "B"])
def test_trajectory_on_the_twin(study, name):
    truth, _, _ = study.frames(name)
    ff, an = study.chains(name)
    ef, ea = report(name, truth, ff, an)
    final_bound, mean_bound = ratio_bounds(name)
    assert ea[0] < final_bound * ef[0] and ea[1] < mean_bound * ef[1], (ea, ef)
    # no threshold comparison of either chain is closer than 1e-6 (relative) to its threshold: the device cannot decide otherwise
    assert ff.margin >= 1e-6 and an.margin >= 1e-6, (ff.margin, an.margin)
    refs = an.anchor_log[1:, 1].astype(int)
    assert (refs >= 0).all() and (refs < np.arange(1, len(truth))).all()
    if name == "B":                                                         # the local revisit: an older slot is taken while newer ones exist
        newest = np.array([an.anchor_log[1:i + 1, 3].nonzero()[0].max(initial=-1) + 1 for i in range(len(truth) - 1)])
        assert (refs[1:] < newest[:-1]).any()


# ---------------------------------------------------------------------------------------------------------------- the interface
def test_anchor_policy_arguments(built_lib):
    from naruto_amd.odometry import AnchorPolicy, OdometryGate
    p = AnchorPolicy()
    assert (p.slots, p.min_overlap, p.max_trans, p.max_rot_deg, p.refail) == (AS.SLOTS, AS.MIN_OVERLAP, AS.MAX_TRANS, AS.MAX_ROT_DEG, AS.REFAIL)
    a, t = p.abi(), AS.policy()
    assert (a.slots, a.refail, a.min_overlap, a.max_trans, a.min_trace) == (t.slots, t.refail, t.min_overlap, t.max_trans, t.min_trace)
    assert AnchorPolicy.of(None).slots == 4 and AnchorPolicy.of(True).slots == 4 and AnchorPolicy.of(p) is p
    for bad in (dict(slots=0), dict(slots=9), dict(slots=2.0), dict(refail=0), dict(min_overlap=1.5), dict(max_trans=-1.0), dict(max_rot_deg=float("nan")),
                dict(min_overlap=0.25), dict(max_trans=0.3), dict(max_rot_deg=30.0), dict(min_overlap=0.1), dict(max_trans=0.5)):
        with pytest.raises(ValueError):
            AnchorPolicy(**bad)
    tight = OdometryGate(max_trans=0.05)
    with pytest.raises(ValueError):
        p.within(tight)
    with pytest.raises(ValueError):
        AnchorPolicy(gate=tight)
    assert AnchorPolicy(max_trans=0.04, gate=tight).within(tight).max_trans == 0.04
    with pytest.raises(ValueError):
        AnchorPolicy.of("yes")


def test_slam_argument_errors(built_lib):
    from naruto_amd.slam import CoSLAMNarutoHIP
    for kw in (dict(track=True, motion_prior="depth_icp"), dict(track=True, motion_prior="const_speed", prior_gate=None), dict(track=True),
               dict(track=True, motion_prior="rgbd_icp", prior_gate=False)):
        with pytest.raises(ValueError, match="prior_anchor"):
            CoSLAMNarutoHIP({}, prior_anchor=True, **kw)


def test_command_line_flags():
    from naruto_amd import run
    base = ["--config", "c.yaml", "--mesh", "m.ply", "--result_dir", "out", "--num_iter", "5"]
    args = run.parse_args(base + ["--track", "--motion_prior", "depth_icp", "--prior_gate", "--prior_anchor", "--anchor_slots", "2"])
    assert args.prior_anchor and args.anchor_slots == 2 and run._anchor_policy(args).slots == 2
    assert run._anchor_policy(run.parse_args(base)) is None
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--anchor_slots", "2"])

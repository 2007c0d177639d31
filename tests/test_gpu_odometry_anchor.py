"""The odometry prior's reference ring on the device (naruto_amd/odometry.py, csrc/naruto_odom_anchor.hip) against the numpy twin
(tests/odometry_anchor_spec.py) and against the existing calls it shares its kernel bodies with, and the tracked run with prior_anchor=True.

1. score over the references  2. the anchored accumulate and K = 1 score  3. the one-thread kernels and the ring over a script
4. one slot, promoted every frame = the gated chain  5. trajectories A and B  6. the tracked run  7. the command line

Run: timeout -k 10 900 python -m pytest tests/test_gpu_odometry_anchor.py -m gpu -q -s
"""
import math

import numpy as np
import pytest
import torch
import yaml

import cull_spec as CS
import odometry_anchor_spec as AS
import odometry_gate_spec as GS
import odometry_rgbd_spec as RS
import odometry_spec as OS
import test_gpu_odometry_gate as TG
import test_odometry_anchor_host as TH

pytestmark = pytest.mark.gpu

Y = (0.0, 1.0, 0.0)
SMALL_T = OS.relative_motion((0.3, -0.8, 0.5), 1.0, OS.CASE_ALONG, 0.02)
NAN_T = np.full((4, 4), np.nan)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _set_head(anchor, words):
    anchor.head.copy_(torch.tensor([int(w) for w in words], dtype=torch.int32))


def _ring_of(gpu, Hh, W, slots, rgbd, levels=1):
    """An odometry, a current frame and ``slots`` different reference frames at Hh x W: (od, anchor, device maps, the twin's maps, camera)."""
    from naruto_amd.odometry import AnchorPolicy, DepthOdometryHIP, RGBDOdometryHIP
    cam = CS.camera(W, Hh, float(max(W, Hh)))
    dp, dc, cp, cc = RS.drawn_pair(Hh, W, seed=Hh * 1000 + W)
    if Hh >= 3 and W >= 8:
        dc[Hh // 2, W // 3:W // 3 + 3] = 0.0                               # a hole
        dp[Hh // 3, W // 2] = np.nan                                       # a NaN depth in every reference
    iters = (1,) * levels
    od = RGBDOdometryHIP(cam, levels=levels, iters=iters, device=gpu) if rgbd else DepthOdometryHIP(cam, levels=levels, iters=iters, device=gpu)
    anchor = od.new_anchor(AnchorPolicy(slots=slots))
    refs = [(dp + np.float32(0.002 * s)).astype(np.float32) for s in range(slots)]       # slot s: the previous frame, 2 s mm farther
    frames = [(r, cp) for r in refs] + [(dc, cc)]
    dev = [od.frame_maps(*_dev(gpu, d, c)) if rgbd else od.frame_maps(*_dev(gpu, d)) for d, c in frames]
    twin = [RS.frame_maps(d, c, cam, levels) if rgbd else OS.frame_maps(d, cam, levels) for d, c in frames]
    for s in range(slots):
        anchor.ring[s].copy_(dev[s])
    return od, anchor, dev, twin, cam


# --------------------------------------------------------------------------------------------- 1. score over the references
# pixel counts 1, 255 (below one round of threads), 2049 (two workgroups), 19200 (ten workgroups); slots 1, 3, 8
@pytest.mark.parametrize("rgbd", [False, True], ids=["depth", "rgbd"])
@pytest.mark.parametrize("slots", [1, 3, 8])
@pytest.mark.parametrize("Hh,W", [(1, 1), (15, 17), (3, 683), (120, 160)])
def test_score_refs_equals_score_per_slot_and_the_twin_in_every_bit(gpu, Hh, W, slots, rgbd):
    od, anchor, dev, twin, cam = _ring_of(gpu, Hh, W, slots, rgbd)
    cur, tcur = dev[-1], twin[-1]
    T = OS.relative_motion(Y, math.degrees(2.0 / max(W, Hh)), (0.6, 0.0, -0.74), 0.004)
    frames = list(range(slots))
    if slots >= 3:
        frames[1] = -1                                                      # an empty slot in the middle
    _set_head(anchor, [0, 0, 0, 0] + frames + [-1] * (8 - slots))
    trunc = 0.004
    if slots == 8:                                                          # the candidates from est, one of the slots' poses NaN
        est = np.stack([OS.relative_motion(Y, 0.3 * k, OS.CASE_ALONG, 0.002 * k) for k in range(10)]).astype(np.float32)
        est[2] = np.nan
        cands = od.anchor_candidates(anchor, torch.from_numpy(est).to(gpu), 9).cpu().numpy()
        assert np.isnan(cands[2, :, :12]).all() and np.isfinite(np.delete(cands, 2, 0)).all()     # the affine inverse's last row is 0 0 0 1
    else:
        cands = np.stack([np.stack([T, SMALL_T]) if s % 2 == 0 else np.stack([np.eye(4), T]) for s in range(slots)]).reshape(slots, 2, 16)
        anchor.cands.copy_(torch.from_numpy(cands))
    anchor.sums.fill_(7.0)
    got = od.score_refs(anchor, cur, level=0, trunc=trunc).cpu().numpy().copy()
    w = RS.PHOTO_WEIGHT if rgbd else 0.0
    rows = 0
    for s in range(slots):
        if frames[s] < 0:
            assert not got[s].any(), (s, got[s])
            continue
        one = od.score(anchor.ring[s], cur, anchor.cands[s].reshape(2, 16), level=0, trunc=trunc).cpu().numpy()
        assert np.array_equal(_bits64(got[s]), _bits64(one)), (s, got[s], one)
        want = GS.score(cands[s].reshape(2, 4, 4), cam, 0, twin[s], tcur, trunc, levels=1, photo_weight=w)
        assert np.array_equal(_bits64(got[s]), _bits64(want)), (s, got[s], want)
        if np.isnan(cands[s]).any():
            assert not got[s, 1:].any()
        rows += got[s, 1] + got[s, 5]
    if Hh >= 15:
        assert rows > 0 and (not rgbd or got[0, 3] > 0)
    again = od.score_refs(anchor, cur, level=0, trunc=trunc).cpu().numpy()
    assert np.array_equal(_bits64(again), _bits64(got))


# --------------------------------------------------------------------------------------------- 2. the anchored accumulate and K = 1 score
@pytest.mark.parametrize("rgbd", [False, True], ids=["depth", "rgbd"])
@pytest.mark.parametrize("Hh,W", [(23, 89), (120, 160)])
def test_anchored_accumulate_and_score_equal_the_existing_calls_in_every_bit(gpu, Hh, W, rgbd):
    slots = 3
    od, anchor, dev, _, _ = _ring_of(gpu, Hh, W, slots, rgbd, levels=2)
    cur = dev[-1]
    # the chosen slot 0 and slots - 1; a word that is not a slot (written by the host) reads the last slot
    for word, s in ((0, 0), (slots - 1, slots - 1), (slots, slots - 1), (77, slots - 1), (-1, slots - 1)):
        _set_head(anchor, [0, 0, word, 0, 0, 1, 2] + [-1] * 5)
        for level in (0, 1):
            state = od.init_state(SMALL_T)
            want = od.accumulate(level, anchor.ring[s], cur, state).cpu().numpy().copy()
            od.sums.fill_(7.0)
            got = od.accumulate_anchored(level, anchor, cur, state).cpu().numpy().copy()
            assert want[28] > 0 and np.array_equal(_bits64(got), _bits64(want)), (word, level, got, want)
            want = od.score(anchor.ring[s], cur, state[:16], level=level, trunc=float(od.desc.max_dist)).cpu().numpy().copy()
            od.score_sums.fill_(7.0)
            got = od.score_anchored(anchor, cur, state[:16], level=level).cpu().numpy().copy()
            assert np.array_equal(_bits64(got), _bits64(want)), (word, level, got, want)
    first = od.accumulate(0, anchor.ring[0], cur, od.init_state(SMALL_T)).cpu().numpy().copy()
    last = od.accumulate(0, anchor.ring[2], cur, od.init_state(SMALL_T)).cpu().numpy().copy()
    assert not np.array_equal(first, last), "the slots' blocks differ, so a wrong slot would show"


# --------------------------------------------------------------------------------------------- 3. the one-thread kernels and the ring
def test_choose_rules_equal_the_twin(gpu):
    from naruto_amd.odometry import AnchorPolicy, DepthOdometryHIP
    od = DepthOdometryHIP(CS.camera(16, 12, 12.0), device=gpu)
    anchor = od.new_anchor(AnchorPolicy(slots=4))
    cands = np.arange(4 * 2 * 16, dtype=np.float64).reshape(4, 2, 16)
    anchor.cands.copy_(torch.from_numpy(cands))
    head = [2, 0, 0, 0, 7, 3, 9, -1, -1, -1, -1, -1]
    inf, nan = math.inf, math.nan
    cases = [(head, [(0.5, 0.4), (0.3, 0.6), (0.7, 0.8), (0.0, 0.0)]), (head, [(0.25, 0.9), (0.25, 0.9), (0.25, 0.25), (0.0, 0.0)]),
             ([2, 0, 0, 0, 9, 3, 7, -1] + [-1] * 4, [(0.25, 0.9), (0.25, 0.9), (0.25, 0.25), (0.0, 0.0)]),
             (head, [(nan, inf), (0.9, nan), (inf, inf), (0.0, 0.0)]), (head, [(nan, inf)] * 3 + [(0.0, 0.0)]),
             ([3, 0, 0, 0] + [-1] * 8, [(0.1, 0.2)] * 4), ([77, 0, 0, 0] + [-1] * 8, [(0.1, 0.2)] * 4)]
    for words, costs in cases:
        sums = TH._sums(costs)
        anchor.sums.copy_(torch.from_numpy(sums))
        _set_head(anchor, words)
        state = torch.full((48,), 7.0, dtype=torch.float64, device=gpu)
        record = torch.full((16,), 7.0, dtype=torch.float64, device=gpu)
        arec = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)
        od.anchor_choose(anchor, 0.05, state, record, arec)
        want = AS.choose(sums, cands.reshape(4, 2, 4, 4), np.array(words, np.int32), 0.05)
        assert anchor.head.cpu().tolist() == want.head.tolist(), (words, costs)
        assert np.array_equal(_bits64(record.cpu().numpy()), _bits64(want.record)) and np.array_equal(_bits64(arec.cpu().numpy()), _bits64(want.anchor))
        assert np.array_equal(od.cands[:32].cpu().numpy(), want.cands.reshape(32))
        assert np.array_equal(state.cpu().numpy()[:16], want.T.reshape(16)) and not state.cpu().numpy()[16:].any()


def test_candidates_update_promote_and_the_ring_equal_the_twin_over_the_script(gpu):
    from naruto_amd.odometry import AnchorPolicy, DepthOdometryHIP
    Hh, W, slots = 15, 17, 2
    cam = CS.camera(W, Hh, float(W))
    od = DepthOdometryHIP(cam, levels=1, iters=(1,), device=gpu)
    anchor = od.new_anchor(AnchorPolicy(slots=slots))
    assert anchor.head.cpu().tolist() == AS.new_head().tolist() and anchor.ring.shape == (slots, od.maps_bytes // 4)
    n = 1 + len(TH.SCRIPT)
    rs = np.random.RandomState(5)
    depth = [(2.0 + 0.01 * k + 0.2 * rs.rand(Hh, W)).astype(np.float32) for k in range(n)]
    maps = [od.frame_maps(*_dev(gpu, d)) for d in depth]
    tmaps = [OS.frame_maps(d, cam, 1) for d in depth]
    est_np = TH._poses(n, seed=2)
    est = torch.from_numpy(est_np).to(gpu)
    od.anchor_reset(anchor, maps[0], 0)
    pol, head, ring = AS.policy(slots=slots), AS.new_head(0), [0] + [None] * (slots - 1)      # the twin's ring holds frame numbers
    assert anchor.head.cpu().tolist() == head.tolist() and torch.equal(anchor.ring[0], maps[0]) and not anchor.ring[1].any()
    state, record, arec = (torch.zeros(k, dtype=torch.float64, device=gpu) for k in (48, 16, 8))
    for k, (rec, *_) in enumerate(TH.SCRIPT):
        i = 1 + k
        # candidates: the twin's to rounding (its products are not fused); the pair of a slot that holds frame i-1 is candidates' own bits
        got = od.anchor_candidates(anchor, est, i).cpu().numpy().copy()
        want = AS.candidates(est_np, i, head, slots)
        assert np.abs(got.reshape(slots, 2, 4, 4) - want).max() <= 1e-12, (i, got, want)
        own = od.candidates(est, i).cpu().numpy()
        for s in range(slots):
            if head[4 + s] < 0 or head[4 + s] == i - 1:
                assert np.array_equal(_bits64(got[s]), _bits64(own)), (i, s)
        # score and choose: the twin on the device's own candidates and sums
        sums = od.score_refs(anchor, maps[i], level=0, trunc=0.05).cpu().numpy().copy()
        tsums = AS.score_refs(got.reshape(slots, 2, 4, 4), cam, 0, [None if f is None else tmaps[f] for f in ring], head, tmaps[i], 0.05, levels=1)
        assert np.array_equal(_bits64(sums), _bits64(tsums)), (i, sums, tsums)
        od.anchor_choose(anchor, 0.05, state, record, arec)
        ch = AS.choose(sums, got.reshape(slots, 2, 4, 4), head, 0.05)
        assert anchor.head.cpu().tolist() == ch.head.tolist() and np.array_equal(_bits64(arec.cpu().numpy()), _bits64(ch.anchor)), (i, ch.anchor)
        assert np.array_equal(_bits64(record.cpu().numpy()), _bits64(ch.record)) and np.array_equal(_bits64(state.cpu().numpy()[:16]), _bits64(ch.T.reshape(16)))
        # update and promote on the script's verdict record (written by the host)
        record.copy_(torch.from_numpy(rec))
        od.anchor_update(anchor, i, record, arec)
        head, tan = AS.update(pol, i, rec, ch.head, ch.anchor)
        assert anchor.head.cpu().tolist() == head.tolist(), (i, anchor.head.cpu().tolist(), head.tolist())
        assert np.array_equal(_bits64(arec.cpu().numpy()), _bits64(tan)), (i, arec.cpu().numpy(), tan)
        od.anchor_promote(anchor, maps[i])
        ring = AS.promote(head, ring, i)
        for s in range(slots):                                              # the whole ring, byte for byte
            want_block = torch.zeros_like(maps[0]) if ring[s] is None else maps[ring[s]]
            assert torch.equal(anchor.ring[s].view(torch.int32), want_block.view(torch.int32)), (i, s, ring)
    assert ring == [8, 10]


def test_predict_anchored_reads_the_reference_from_the_record(gpu):
    from naruto_amd.pose_chain import pose_predict_anchored, pose_predict_relative
    est_np = TH._poses(6, seed=3)
    T = torch.from_numpy(np.concatenate([SMALL_T.reshape(16), np.zeros(32)])).to(gpu)
    for f, ref in ((1.0, 1), (4.0, 4), (-1.0, 4), (5.0, 4), (9.0, 4)):
        est, pose6 = torch.from_numpy(est_np.copy()).to(gpu), torch.zeros(6, device=gpu)
        arec = torch.tensor([0.0, f, 1.0, 0, 0, 0, 0, 0], dtype=torch.float64, device=gpu)
        pose_predict_anchored(est, 5, arec, T, pose6)
        assert np.array_equal(est[5].cpu().numpy(), AS.predict(est_np, 5, arec.cpu().numpy(), SMALL_T)), f
        if ref == 4:                                                        # the frame before: pose_predict_relative's bits, pose6 too
            est2, pose62 = torch.from_numpy(est_np.copy()).to(gpu), torch.zeros(6, device=gpu)
            pose_predict_relative(est2, 5, T, pose62)
            assert torch.equal(est.view(torch.int32), est2.view(torch.int32)) and torch.equal(pose6.view(torch.int32), pose62.view(torch.int32))


# --------------------------------------------------------------------------------------------- 4. one slot, promoted every frame
def test_one_slot_promoted_every_frame_is_the_gated_chain_bit_for_bit(gpu):
    from naruto_amd.odometry import AnchorPolicy, DepthOdometryHIP
    truth, depth, _ = TH.shared_study().frames("B")
    frames = _dev(gpu, *[depth[2 * k] for k in range(6)])                   # every second frame: five degrees and five centimetres a step
    od = DepthOdometryHIP(TH.CAM, device=gpu)
    every = AnchorPolicy(slots=1, min_overlap=1.0, max_trans=0.0, refail=1)
    a = od.chain(frames, anchor=every, first=truth[0])
    b = od.chain(frames, first=truth[0])
    assert a.anchor_log[1:, 3].tolist() == [1.0] * 5 and a.anchor_log[1:, 1].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and b.anchor_log is None
    assert np.array_equal(a.poses.view(np.int32), b.poses.view(np.int32)), np.abs(a.poses - b.poses).max()
    assert np.array_equal(_bits64(a.prior_log), _bits64(b.prior_log))
    print("verdicts", a.prior_log[1:, 0], "starts", a.prior_log[1:, 1])
    assert (a.prior_log[1:, 6] > 0).all() and np.isfinite(a.prior_log).all()


# --------------------------------------------------------------------------------------------- 5. trajectories A and B
@pytest.mark.parametrize("name", ["A", "B"])
def test_trajectory_chains_equal_the_twin_and_the_ring_cuts_the_drift(gpu, name):
    from naruto_amd.odometry import AnchorPolicy, DepthOdometryHIP
    study = TH.shared_study()
    truth, depth, _ = study.frames(name)
    tff, tan = study.chains(name)
    od = DepthOdometryHIP(TH.CAM, device=gpu)
    frames = _dev(gpu, *depth)
    ff = od.chain(frames, first=truth[0])
    an = od.chain(frames, anchor=AnchorPolicy(), first=truth[0])
    again = od.chain(frames, anchor=True, first=truth[0])
    assert np.array_equal(an.poses.view(np.int32), again.poses.view(np.int32)) and np.array_equal(_bits64(an.prior_log), _bits64(again.prior_log))
    assert np.array_equal(_bits64(an.anchor_log), _bits64(again.anchor_log))
    # the decisions are the twin's: chosen slot and frame, valid slots, promoted, slot written, streak; start, verdict
    assert np.array_equal(an.anchor_log[:, :6], tan.anchor_log[:, :6]), np.argwhere(an.anchor_log[:, :6] != tan.anchor_log[:, :6])
    assert np.array_equal(an.prior_log[:, :2], tan.prior_log[:, :2]) and np.array_equal(ff.prior_log[:, :2], tff.prior_log[:, :2])
    for got, want in ((ff, tff), (an, tan)):                                # the poses: within the solver's bound of the twin's
        dt = np.linalg.norm(got.poses[:, :3, 3].astype(np.float64) - want.poses[:, :3, 3], axis=1).max()
        # the angle between two rotations from the chord |Rg - Rw|_F = 2 sqrt(2) sin(angle / 2): float32 matrices are orthonormal to 1e-7
        # only, which the arc cosine of a trace near 3 turns into hundredths of a degree
        chord = np.linalg.norm(got.poses[:, :3, :3].astype(np.float64) - want.poses[:, :3, :3], axis=(1, 2)).max()
        dr = math.degrees(2.0 * math.asin(min(1.0, chord / (2.0 * math.sqrt(2.0)))))
        print(f"trajectory {name}: device against twin {dt * 1e3:.6f} mm, {dr:.6f} deg")
        assert dt <= OS.BOUND_M and dr <= OS.BOUND_DEG
    ef, ea = AS.translation_errors(ff.poses, truth), AS.translation_errors(an.poses, truth)
    print(f"trajectory {name}: frame to frame final {ef[0] * 1e3:.2f} mm mean {ef[1] * 1e3:.2f} mm; anchored final {ea[0] * 1e3:.2f} mm mean {ea[1] * 1e3:.2f} mm; "
          f"ratios {ea[0] / ef[0]:.3f} {ea[1] / ef[1]:.3f}; refused {int((an.prior_log[1:, 0] == 0).sum())}, promoted {int(an.anchor_log[:, 3].sum())}")
    final_bound, mean_bound = TH.ratio_bounds(name)
    assert ea[0] < final_bound * ef[0] and ea[1] < mean_bound * ef[1], (ea, ef)


# --------------------------------------------------------------------------------------------- 6. the tracked run
N_RUN = 12


def _trajectory():
    """Two degrees of yaw and 2 cm per frame, out for six frames and back: the ring's limits are crossed on the way (10 degrees after five)."""
    out, back = OS.relative_motion(Y, 2.0, OS.CASE_ALONG, 0.02), OS.relative_motion(Y, -2.0, OS.CASE_ALONG, -0.02)
    poses = [TG._look(OS.CASE_POSITION, CS.ROOM_CENTRE)]
    for i in range(1, N_RUN):
        poses.append(poses[-1] @ (out if i <= 6 else back))
    return torch.from_numpy(np.stack(poses).astype(np.float32))


def _tracked_run(gpu, guard):
    from naruto_amd import tracking
    from naruto_amd.run import run_exploration
    from naruto_amd.slam import CoSLAMNarutoHIP
    slam = CoSLAMNarutoHIP(TG._cfg(), voxel_size=0.1, active_ray=False, num_frames=N_RUN, seed=3, device=gpu, track=True, motion_prior="depth_icp", prior_gate=True,
                           prior_anchor=True)
    assert slam.anchor_log.shape == (N_RUN, 8) and slam.anchor_log.dtype == torch.float64 and slam.prior_anchor.slots == 4
    sim = TG._sim(gpu, {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")})
    saved = (tracking.matrices_to_pose6, tracking.matrix_to_axis_angle)

    def boom(*a, **k):
        raise AssertionError("the host's log map was called during a tracked step")

    def on_step(i, c2w, vols, state):
        if i == 0 and guard:                        # from the first tracked frame on, the host's pose conversion is out of reach
            tracking.matrices_to_pose6, tracking.matrix_to_axis_angle = boom, boom
    try:
        out = run_exploration(slam, sim, None, None, N_RUN, traj=_trajectory(), on_step=on_step)
    finally:
        tracking.matrices_to_pose6, tracking.matrix_to_axis_angle = saved
    assert torch.equal(slam.anchor_log.cpu(), out["anchor_log"])
    return out


def test_a_tracked_run_fills_the_anchor_log_never_waits_for_the_host_and_repeats(gpu):
    from naruto_amd.slam import CoSLAMNarutoHIP
    with pytest.raises(ValueError, match="prior_anchor"):
        CoSLAMNarutoHIP(TG._cfg(), num_frames=4, device=gpu, track=True, motion_prior="depth_icp", prior_anchor=True)
    out = _tracked_run(gpu, guard=True)
    log, plog = out["anchor_log"].numpy(), out["prior_log"].numpy()
    for i in range(1, N_RUN):
        print(f"frame {i}: slot {int(log[i, 0])} frame {int(log[i, 1])} of {int(log[i, 2])}, promoted {int(log[i, 3])} into {int(log[i, 4])}, streak {int(log[i, 5])}, "
              f"costs {log[i, 6]:.4f} {log[i, 7]:.4f}; verdict {plog[i, 0]}, |t| {plog[i, 9]:.4f}, trace {plog[i, 10]:.4f}")
    assert log.shape == (N_RUN, 8) and not log[0].any() and np.isfinite(log).all() and np.isfinite(plog).all()
    refs = log[1:, 1].astype(int)
    assert (log[1:, 2] >= 1).all() and (refs >= 0).all() and (refs < np.arange(1, N_RUN)).all() and (log[1:, 6] >= 0).all()
    assert log[1:, 3].sum() >= 1 and (refs < np.arange(N_RUN - 1)).any(), "a frame was promoted and a frame was registered to an older reference"
    assert bool(torch.isfinite(out["est_poses"]).all())
    again = _tracked_run(gpu, guard=False)
    assert torch.equal(out["est_poses"].view(torch.int32), again["est_poses"].view(torch.int32))
    assert np.array_equal(_bits64(log), _bits64(again["anchor_log"].numpy())) and np.array_equal(_bits64(plog), _bits64(again["prior_log"].numpy()))


# --------------------------------------------------------------------------------------------- 7. the command line
def test_prior_anchor_through_the_command_line(gpu, tmp_path):
    from naruto_amd.mesh import Mesh
    from naruto_amd.run import main
    v, f = CS.room_mesh(n_lat=8, n_lon=16)
    Mesh(np.asarray(v, np.float64), np.asarray(f, np.int64)).export(str(tmp_path / "room.ply"))
    with open(tmp_path / "cfg.yaml", "w") as fh:
        yaml.safe_dump(TG._cfg(), fh)
    argv = ["--config", str(tmp_path / "cfg.yaml"), "--mesh", str(tmp_path / "room.ply"), "--num_iter", "12", "--result_dir", str(tmp_path / "out"),
            "--start", "2.0", "4.0", "1.2", "--no_active_ray", "--seed", "5", "--track", "--motion_prior", "rgbd_icp", "--prior_gate", "--prior_anchor",
            "--anchor_slots", "2", "--planner", "gs_z_levels=[12]", "max_rot_deg=30", "rrt_max_iter=2000"]
    out = main(argv)
    log = out["anchor_log"].numpy()
    assert log.shape == (12, 8) and np.isfinite(log).all() and not log[0].any() and (log[1:, 2] >= 1).all() and (log[1:, 0] < 2).all()
    rows = dict(line.strip().split(",") for line in open(tmp_path / "out" / "results.txt"))
    assert set(rows) == {"traj_len(m)", "ate_rmse(cm)", "ate_mean(cm)", "prior_failed_frames", "prior_anchor_promotions"}
    assert int(rows["prior_anchor_promotions"]) == int((log[1:, 3] == 1.0).sum())
    with pytest.raises(ValueError, match="prior_anchor"):
        main(argv[:argv.index("--prior_gate")] + argv[argv.index("--prior_anchor"):])

"""numpy twin of the odometry prior's reference ring (naruto_amd/odometry.py restates the contract; csrc/naruto_odom_anchor.hip), built on
tests/odometry_gate_spec.py, tests/odometry_spec.py and tests/odometry_rgbd_spec.py.

* ``inverse`` and ``mul`` are the pose chain's ``pose_affine_inverse`` and ``pose_mul`` operation by operation in fp64, every product and
  sum rounded.  The device functions are compiled where the compiler may fuse a product into the following sum, so the device's
  candidates agree with ``candidates`` to a few units in the last place, not on the bits -- except the pair of a slot that holds frame
  i-1, which is exact on both sides (the identity; the last motion is compared as ``naruto_odom_candidates``' own).
* ``score_refs`` is ``odometry_gate_spec.score`` at K = 2 per slot: bit for bit the device's sums when both are given the same candidates.
* ``choose``, ``update``, ``promote`` and ``predict`` are Python floats and ints in the kernels' order: compared on the bits.
* ``chain`` is the prior-only chain of ``DepthOdometryHIP.chain`` over maps made by the twins, with or without the ring; it also returns,
  per frame, how far (relatively) every threshold comparison was from its threshold.
"""
import math
from types import SimpleNamespace

import numpy as np

import odometry_gate_spec as GS
import odometry_rgbd_spec as RS
import odometry_spec as OS

F32 = np.float32
MAX_REFS, HEAD_WORDS, ANCHOR_WORDS, REF_SUMS = 8, 12, 8, 9
SLOTS, MIN_OVERLAP, MAX_TRANS, MAX_ROT_DEG, REFAIL = 4, 0.7, 0.10, 10.0, 2


def policy(slots=SLOTS, min_overlap=MIN_OVERLAP, max_trans=MAX_TRANS, max_rot_deg=MAX_ROT_DEG, refail=REFAIL):
    """The promote policy as the host hands it to the kernel: min_trace = 1 + 2 cos(max_rot)."""
    return SimpleNamespace(slots=int(slots), min_overlap=float(min_overlap), max_trans=float(max_trans), max_rot_deg=float(max_rot_deg),
                           min_trace=1.0 + 2.0 * math.cos(math.radians(max_rot_deg)), refail=int(refail))


def new_head(frame=None):
    """int32 [12]: all slots empty, or frame ``frame`` in slot 0 (``anchor_reset``)."""
    h = np.array([0, 0, 0, 0] + [-1] * MAX_REFS, np.int32)
    if frame is not None:
        h[4] = frame
    return h


def slot_of(word, slots):
    """A slot word as the kernels read it: as uint32, anything not below ``slots`` is the last slot."""
    w = int(word) & 0xFFFFFFFF
    return w if w < slots else slots - 1


# ---------------------------------------------------------------------------------------------------------------- the pose chain's arithmetic
def mul(A, B):
    A, B = np.asarray(A, np.float64).reshape(4, 4), np.asarray(B, np.float64).reshape(4, 4)
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s = s + float(A[i, k]) * float(B[k, j])
            C[i, j] = s
    return C


def inverse(M):
    M = np.asarray(M, np.float64).reshape(4, 4)
    a, b, c, d, e, f, g, h, k = (float(v) for v in M[:3, :3].reshape(9))
    c00, c01, c02 = e * k - f * h, c * h - b * k, b * f - c * e
    c10, c11, c12 = f * g - d * k, a * k - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    with np.errstate(all="ignore"):
        r = float(np.float64(1.0) / np.float64(a * c00 + b * c10 + c * c20))
    A = [c00 * r, c01 * r, c02 * r, c10 * r, c11 * r, c12 * r, c20 * r, c21 * r, c22 * r]
    t = [float(M[0, 3]), float(M[1, 3]), float(M[2, 3])]
    out = np.eye(4)
    for i in range(3):
        out[i, :3] = A[3 * i:3 * i + 3]
        out[i, 3] = -(A[3 * i] * t[0] + A[3 * i + 1] * t[1] + A[3 * i + 2] * t[2])
    return out


def last_motion(est, i):
    """inv(est[i-2]) @ est[i-1] for i > 1, else the identity (``naruto_odom_candidates``' second matrix, to the last few bits)."""
    return mul(inverse(est[i - 2]), est[i - 1]) if i > 1 else np.eye(4)


def candidates(est, i, head, slots, M=None):
    """[slots,2,4,4]: slot s's starts inv(est[f]) @ est[i-1] and that times M (default ``last_motion``); the identity and M for f = i-1
    and for an empty slot."""
    M = last_motion(est, i) if M is None else np.asarray(M, np.float64).reshape(4, 4)
    out = np.zeros((slots, 2, 4, 4))
    for s in range(slots):
        f = int(head[4 + s])
        if f < 0 or f >= i - 1:
            out[s, 0], out[s, 1] = np.eye(4), M
        else:
            R = mul(inverse(est[f]), est[i - 1])
            out[s, 0], out[s, 1] = R, mul(R, M)
    return out


# ---------------------------------------------------------------------------------------------------------------- score, choose, update, promote
def score_refs(cands_all, cam, level, ring, head, maps_cur, trunc, levels=3, max_dist=0.25, photo_weight=0.0, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """[slots,9]: ``odometry_gate_spec.score`` at K = 2 of slot s's pair against ring[s]; zeros for an empty slot."""
    slots = len(ring)
    out = np.zeros((slots, REF_SUMS))
    for s in range(slots):
        if int(head[4 + s]) >= 0:
            out[s] = GS.score(cands_all[s], cam, level, ring[s], maps_cur, trunc, levels, max_dist, photo_weight, photo_max_diff)
    return out


def _finite_or(v, other):
    return v if abs(v) < math.inf else other


def choose(sums, cands_all, head, trunc, photo_on=False, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """-> namespace slot, start, head (a copy with [2] written), cands [2,4,4], T, record [16], anchor [8]."""
    cands_all = np.asarray(cands_all, np.float64)
    slots = cands_all.shape[0]
    best, second, bs, bf, bk, valid = math.inf, math.inf, -1, -1, 0, 0
    for s in range(slots):
        f = int(head[4 + s])
        if f < 0:
            continue
        valid += 1
        for k, c in enumerate(GS.costs(sums[s], 2, trunc, photo_on, photo_max_diff)):
            if c < best or (c == best and c < math.inf and f > bf):
                second, best, bs, bf, bk = best, c, s, f, k
            elif c < second:
                second = c
    slot = bs if bs >= 0 else slot_of(head[0], slots)
    record = np.zeros(GS.GATE_WORDS)
    record[1] = float(bk)
    record[2:6] = GS.costs(sums[slot], 2, trunc, photo_on, photo_max_diff) + [-1.0, -1.0]
    head = np.array(head, np.int32)
    head[2] = slot
    anchor = np.zeros(ANCHOR_WORDS)
    anchor[0], anchor[1], anchor[2] = float(slot), float(head[4 + slot]), float(valid)
    anchor[6], anchor[7] = _finite_or(best, -1.0), _finite_or(second, -1.0)
    return SimpleNamespace(slot=slot, start=bk, head=head, cands=cands_all[slot].copy(), T=cands_all[slot, bk].copy(), record=record, anchor=anchor)


def update(pol, i, record, head, anchor):
    """-> (head, anchor) after k_odom_anchor_update on the verdict's ``record``."""
    head, anchor = np.array(head, np.int32), np.array(anchor, np.float64)
    ok = float(record[0]) == 1.0
    valid, rows, t, trace = (float(record[k]) for k in (6, 7, 9, 10))
    streak = int(head[1])
    if ok:
        promote = rows < pol.min_overlap * valid or t > pol.max_trans or trace < pol.min_trace
        streak = 0
    else:
        streak = 1 if streak < 0 else (streak + 1 if streak < pol.refail else pol.refail)
        promote = streak >= pol.refail
        if promote:
            streak = 0
    written = -1
    if promote:
        written = (slot_of(head[0], pol.slots) + 1) % pol.slots
        head[0], head[4 + written] = written, i
    head[1], head[3] = streak, 1 if promote else 0
    anchor[3], anchor[4], anchor[5] = float(promote), float(written), float(streak)
    return head, anchor


def promote(head, ring, maps_cur):
    """ring (a list of maps, one per slot) after k_odom_anchor_promote: the current maps in slot head[0] when head[3] is set."""
    ring = list(ring)
    if int(head[3]) != 0:
        ring[slot_of(head[0], len(ring))] = maps_cur
    return ring


def predict(est, i, anchor, T):
    """est[i] (float32 [4,4]) = est[f] @ T, f = anchor[1] (outside 0 .. i-1: i-1), rounded once."""
    f = float(anchor[1])
    ref = int(f) if 0.0 <= f < float(i) else i - 1
    return mul(np.asarray(est[ref], np.float64), T).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- margins
def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0.0 else (math.inf if a != b else 0.0)


def margins(g, record, pol=None):
    """The relative distance of every threshold comparison of one frame from its threshold: the verdict's four, then the update's three
    (after a PASS only: a refused frame's update compares integers)."""
    valid, rows, rmse, t, trace = (float(record[k]) for k in (6, 7, 8, 9, 10))
    out = [_rel(rows, g.min_overlap * valid), _rel(rmse, g.max_rmse) if rows > 0 else math.inf, _rel(t, g.max_trans), _rel(trace, g.min_trace)]
    if pol is not None and float(record[0]) == 1.0:
        out += [_rel(rows, pol.min_overlap * valid), _rel(t, pol.max_trans), _rel(trace, pol.min_trace)]
    return out


# ---------------------------------------------------------------------------------------------------------------- the chains
def estimate_anchored(ring, head, maps_cur, est, i, cam, g, pol, levels=3, iters=(10, 5, 4), max_dist=0.25, photo_weight=0.0,
                      photo_max_diff=RS.PHOTO_MAX_DIFF):
    """One anchored estimate on the twin.  -> namespace T (relative to the reference ``anchor[1]`` names), record, anchor, head, ring."""
    rgbd = isinstance(maps_cur, tuple)
    photo_on = rgbd and float(F32(photo_weight)) > 0.0
    pw = photo_weight if rgbd else 0.0
    cands_all = candidates(est, i, head, pol.slots)
    sums = score_refs(cands_all, cam, levels - 1, ring, head, maps_cur, g.score_trunc, levels, max_dist, pw, photo_max_diff)
    ch = choose(sums, cands_all, head, g.score_trunc, photo_on, photo_max_diff)
    prev = ring[ch.slot]
    if rgbd:
        T, status, _ = RS.estimate(prev, maps_cur, cam, levels, iters, max_dist, ch.T, photo_weight, photo_max_diff)
    else:
        T, status, _ = OS.estimate(prev, maps_cur, cam, levels, iters, max_dist, ch.T)
    fine = GS.score(T[None], cam, 0, prev, maps_cur, float(F32(max_dist)), levels, max_dist, pw, photo_max_diff)
    Tv, record = GS.verdict(g, fine, T, status[0], ch.cands, ch.record)
    head, anchor = update(pol, i, record, ch.head, ch.anchor)
    return SimpleNamespace(T=Tv, record=record, anchor=anchor, head=head, ring=promote(head, ring, maps_cur), cands=cands_all, sums=sums)


def chain(maps, cam, first=None, g=None, pol=None, levels=3, iters=(10, 5, 4), max_dist=0.25, photo_weight=0.0, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """The prior-only chain over the frames' maps (``odometry_spec.frame_maps`` results, or the RGB-D twin's pairs).  pol None: gated frame to
    frame (the two starts of ``candidates`` for a slot that holds frame i-1).  -> namespace poses float32 [n,4,4], prior_log [n,16],
    anchor_log [n,8] or None, margin (the smallest of ``margins`` over the chain)."""
    g = g or GS.gate()
    n = len(maps)
    est = np.zeros((n, 4, 4), F32)
    est[0] = np.eye(4) if first is None else np.asarray(first, F32)
    prior_log, anchor_log, margin = np.zeros((n, GS.GATE_WORDS)), None if pol is None else np.zeros((n, ANCHOR_WORDS)), math.inf
    if pol is not None:
        ring, head = [maps[0]] + [None] * (pol.slots - 1), new_head(0)
    for i in range(1, n):
        if pol is None:
            out = GS.estimate_gated(maps[i - 1], maps[i], cam, np.stack([np.eye(4), last_motion(est, i)]), g, levels, iters, max_dist, photo_weight,
                                    photo_max_diff)
            est[i] = mul(np.asarray(est[i - 1], np.float64), out.T).astype(F32)
        else:
            out = estimate_anchored(ring, head, maps[i], est, i, cam, g, pol, levels, iters, max_dist, photo_weight, photo_max_diff)
            ring, head, anchor_log[i] = out.ring, out.head, out.anchor
            est[i] = predict(est, i, out.anchor, out.T)
        prior_log[i] = out.record
        margin = min([margin] + margins(g, out.record, pol))
    return SimpleNamespace(poses=est, prior_log=prior_log, anchor_log=anchor_log, margin=margin)


# ---------------------------------------------------------------------------------------------------------------- the study's trajectories
def trajectory(base, n, amp_deg, p, amp_m, q):
    """[n,4,4] float32: pose k = base @ relative_motion(y, amp_deg sin(2 pi k / p), CASE_ALONG, amp_m sin(2 pi k / q))."""
    return np.stack([(np.asarray(base, np.float64) @ OS.relative_motion((0.0, 1.0, 0.0), amp_deg * math.sin(2.0 * math.pi * k / p), OS.CASE_ALONG,
                                                                        amp_m * math.sin(2.0 * math.pi * k / q))).astype(F32) for k in range(n)])


TRAJECTORIES = {"A": (25, 9.0, 12, 0.04, 8), "B": (97, 40.0, 96, 0.25, 64)}


def translation_errors(poses, truth):
    """(final, mean over frames 1 .., max) of |t - t_true| in metres."""
    e = np.linalg.norm(np.asarray(poses, np.float64)[:, :3, 3] - np.asarray(truth, np.float64)[:, :3, 3], axis=1)
    return float(e[-1]), float(e[1:].mean()), float(e.max())

"""numpy twin of the odometry prior's scored starts and verdict (naruto_amd/odometry.py restates the contract; csrc/naruto_odom.hip:
k_odom_score, k_odom_candidates, k_odom_choose, k_odom_verdict), built on tests/odometry_spec.py and tests/odometry_rgbd_spec.py.

* ``score``: per candidate the geometric rows are ``odometry_spec.rows`` and the photometric rows ``odometry_rgbd_spec.photo_rows`` -- the
  twins of the device function both accumulate kernels and k_odom_score call -- so the sums are compared on the bits.  Every slot of the
  1 + 4 K sums gets one addition per pixel, in ``odometry_spec.reduce_sums``'s order (pixels, threads, the fold, the finishing launch).
* ``costs``, ``choose`` and ``verdict`` are fp64 operation by operation in Python floats, in the kernels' order; the kernels switch
  contraction off and use no transcendental function (sqrt and division are correctly rounded), so the records are compared on the bits.
* ``estimate_gated`` is the fixed sequence: score K starts at the coarsest level, choose, the level loop of the twin it is built on, a
  K = 1 score at level 0 with trunc = max_dist, the verdict.
"""
import math
from types import SimpleNamespace

import numpy as np

import odometry_rgbd_spec as RS
import odometry_spec as OS

F32 = np.float32
MAX_CANDS, GATE_WORDS = 4, 16
PASS, FAIL = 1.0, 0.0
# the defaults (chosen from the confusion table of tests/test_odometry_gate_host.py)
MAX_TRANS, MAX_ROT_DEG, MIN_OVERLAP, MAX_RMSE, SCORE_TRUNC = 0.3, 30.0, 0.25, 0.006, 0.05


def gate(max_trans=MAX_TRANS, max_rot_deg=MAX_ROT_DEG, min_overlap=MIN_OVERLAP, max_rmse=MAX_RMSE, score_trunc=SCORE_TRUNC):
    """The verdict's thresholds as the host hands them to the kernel: min_trace = 1 + 2 cos(max_rot)."""
    return SimpleNamespace(max_trans=float(max_trans), min_trace=1.0 + 2.0 * math.cos(math.radians(max_rot_deg)), min_overlap=float(min_overlap),
                           max_rmse=float(max_rmse), score_trunc=float(score_trunc), max_rot_deg=float(max_rot_deg))


def _split(maps):
    """(depth maps, intensity maps or None) of ``odometry_spec.frame_maps`` / ``odometry_rgbd_spec.frame_maps`` results."""
    return (maps[0], maps[1]) if isinstance(maps, tuple) else (maps, None)


# ---------------------------------------------------------------------------------------------------------------- the score
def score_terms(cands, level_cam, prev, cur, trunc, max_dist=0.25, iprev=None, icur=None, photo_weight=0.0, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """terms [n, 1 + 4 K] of one score at a level: [0] p.z < 0, then per candidate (row, min(r^2, trunc^2), photometric row, r_I^2)."""
    cands = np.asarray(cands, np.float64).reshape(-1, 4, 4)
    n = level_cam[0] * level_cam[1]
    t2 = float(trunc) * float(trunc)
    cols = [np.where(cur[1].reshape(n, 3)[:, 2].astype(np.float64) < 0.0, 1.0, 0.0)]
    for T in cands:
        with np.errstate(all="ignore"):
            gi, gr, _ = OS.rows(T, level_cam, prev, cur, max_dist)
            rr = gr * gr
            cols += [np.where(gi >= 0, 1.0, 0.0), np.where(gi >= 0, np.where(rr < t2, rr, t2), 0.0)]
            if float(F32(photo_weight)) > 0.0 and iprev is not None:
                ok, _, rI, _, _ = RS.photo_rows(T, level_cam, prev, cur, iprev, icur, max_dist, photo_weight, photo_max_diff)
                cols += [np.where(ok, 1.0, 0.0), np.where(ok, rI * rI, 0.0)]
            else:
                cols += [np.zeros(n), np.zeros(n)]
    return np.stack(cols, -1)


def _fold(a):
    a = a.copy()
    w = OS.THREADS // 2
    while w > 0:
        a[..., :w, :] = a[..., :w, :] + a[..., w:2 * w, :]
        w //= 2
    return a[..., 0, :]


def reduce_sums(terms):
    """terms [n, N] -> sums [N]: ``odometry_spec.reduce_sums`` over N columns."""
    n, N = terms.shape
    per = OS.THREADS * OS.PER
    parts = max(1, -(-n // per))
    t = np.zeros((parts * per, N))
    t[:n] = terms
    t = t.reshape(parts, OS.PER, OS.THREADS, N)
    acc = np.zeros((parts, OS.THREADS, N))
    for k in range(OS.PER):
        acc = acc + t[:, k]
    part = _fold(acc)
    m = -(-parts // OS.THREADS)
    t2 = np.zeros((m * OS.THREADS, N))
    t2[:parts] = part
    t2 = t2.reshape(m, OS.THREADS, N)
    acc = np.zeros((OS.THREADS, N))
    for k in range(m):
        acc = acc + t2[k]
    return _fold(acc)


def score(cands, cam, level, maps_prev, maps_cur, trunc, levels=3, max_dist=0.25, photo_weight=0.0, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """sums [1 + 4 K] of K candidates at ``level``; maps_*: the depth twin's maps, or the RGB-D twin's (depth maps, intensity maps)."""
    (dp, ip), (dc, ic) = _split(maps_prev), _split(maps_cur)
    lc = OS.level_intrinsics(cam, levels)[level]
    return reduce_sums(score_terms(cands, lc, dp[level], dc[level], trunc, max_dist, None if ip is None else ip[level], None if ic is None else ic[level],
                                   photo_weight, photo_max_diff))


# ---------------------------------------------------------------------------------------------------------------- the one-thread kernels
def _term(n_valid, n, s, tau):
    if n_valid == 0.0:
        return 1.0
    t2 = tau * tau
    d = n_valid * t2
    num = s + (n_valid - n) * t2
    c = num / d if d != 0.0 else (math.nan if num == 0.0 or num != num else math.copysign(math.inf, num))
    return c if abs(c) < math.inf else math.inf


def costs(sums, K, trunc, photo_on=False, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """[K] costs (k_odom_choose's)."""
    s = [float(v) for v in sums]
    out = []
    for k in range(K):
        c = _term(s[0], s[1 + 4 * k], s[2 + 4 * k], float(trunc))
        if photo_on:
            c = c + _term(s[0], s[3 + 4 * k], s[4 + 4 * k], float(photo_max_diff))
        out.append(c if abs(c) < math.inf else math.inf)
    return out


def choose(sums, cands, trunc, photo_on=False, photo_max_diff=RS.PHOTO_MAX_DIFF):
    """(chosen index, T [4,4], record [16] with [1] and [2..5] set)."""
    cands = np.asarray(cands, np.float64).reshape(-1, 4, 4)
    K = len(cands)
    c = costs(sums, K, trunc, photo_on, photo_max_diff)
    best, chosen = math.inf, 0
    for k in range(K):
        if c[k] < best:
            best, chosen = c[k], k
    record = np.zeros(GATE_WORDS)
    record[1] = float(chosen)
    record[2:6] = c + [-1.0] * (MAX_CANDS - K)
    return chosen, cands[chosen].copy(), record


def _finite_or(v, other):
    return v if abs(v) < math.inf else other


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan


def verdict(g, sums, T, status0, cands, record):
    """(T [4,4], record [16]): k_odom_verdict on a K = 1 score ``sums`` of the estimate T; status0 = level 0's status word."""
    T = np.array(T, np.float64).reshape(4, 4)
    record = np.array(record, np.float64)
    n_valid, n_geo, s_geo, n_photo, s_photo = (float(v) for v in sums[:5])
    t2 = (T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3]) + T[2, 3] * T[2, 3]
    trace = (T[0, 0] + T[1, 1]) + T[2, 2]
    ok = (float(status0) >= 0.0 and float(status0) != float(OS.DEGENERATE) and n_geo >= g.min_overlap * n_valid and n_geo > 0.0 and
          s_geo <= (g.max_rmse * g.max_rmse) * n_geo and t2 <= g.max_trans * g.max_trans and trace >= g.min_trace)
    record[0] = PASS if ok else FAIL
    record[6], record[7] = n_valid, n_geo
    record[8] = _finite_or(_sqrt(s_geo / n_geo), -1.0) if n_geo > 0.0 else 0.0
    record[9] = _finite_or(_sqrt(float(t2)), -1.0)
    record[10] = _finite_or(float(trace), -1.0)
    record[11] = float(status0)
    record[12] = n_photo
    record[13] = _finite_or(_sqrt(s_photo / n_photo), -1.0) if n_photo > 0.0 else 0.0
    record[14] = record[15] = 0.0
    if not ok:
        c = record[1]
        T = np.asarray(cands, np.float64).reshape(-1, 4, 4)[int(c) if 0.0 <= c < MAX_CANDS else 0].copy()
    return T, record


def candidates(est, i):
    """[2,4,4]: the identity and the last motion inv(est[i-2]) @ est[i-1] (i > 1; not bit-exact: numpy's inverse), else the identity."""
    out = np.stack([np.eye(4), np.eye(4)])
    if i > 1:
        out[1] = np.linalg.inv(np.asarray(est[i - 2], np.float64)) @ np.asarray(est[i - 1], np.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------- the gated estimate
def estimate_gated(maps_prev, maps_cur, cam, cands=None, g=None, levels=3, iters=(10, 5, 4), max_dist=0.25, photo_weight=0.0,
                   photo_max_diff=RS.PHOTO_MAX_DIFF):
    """The gated estimate on the twin.  maps_*: the depth twin's maps (depth odometry) or the RGB-D twin's pair (then ``photo_weight`` is
    the RGB-D odometry's).  -> namespace T, passed, chosen, costs, overlap, rmse, status, record, estimate (T before the verdict)."""
    g = g or gate()
    cands = np.eye(4)[None] if cands is None else np.asarray(cands, np.float64).reshape(-1, 4, 4)
    rgbd = isinstance(maps_prev, tuple)
    photo_on = rgbd and float(F32(photo_weight)) > 0.0
    pw = photo_weight if rgbd else 0.0
    coarse = score(cands, cam, levels - 1, maps_prev, maps_cur, g.score_trunc, levels, max_dist, pw, photo_max_diff)
    chosen, T0, record = choose(coarse, cands, g.score_trunc, photo_on, photo_max_diff)
    if rgbd:
        T, status, _ = RS.estimate(maps_prev, maps_cur, cam, levels, iters, max_dist, T0, photo_weight, photo_max_diff)
    else:
        T, status, _ = OS.estimate(maps_prev, maps_cur, cam, levels, iters, max_dist, T0)
    md = float(F32(max_dist))
    fine = score(T[None], cam, 0, maps_prev, maps_cur, md, levels, max_dist, pw, photo_max_diff)
    Tv, record = verdict(g, fine, T, status[0], cands, record)
    return SimpleNamespace(T=Tv, passed=bool(record[0] == PASS), chosen=chosen, costs=[float(c) for c in record[2:2 + len(cands)]],
                           overlap=(record[7] / record[6] if record[6] > 0 else 0.0), rmse=float(record[8]), status=list(status), record=record,
                           estimate=np.array(T, np.float64), sums=fine, coarse=coarse)

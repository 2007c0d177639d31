"""The local planner's RRT (RRTNaruto: run, run_full, is_collision_free, get_reachable_mask) restated in numpy, with the
precision choices of naruto_amd/csrc/naruto_rrt.hip, as the CPU side of tests/test_rrt_host.py and tests/test_gpu_rrt.py.

Arithmetic.  Everything that decides something is float64, one rounding per operation, in this order:
  * |v| = sqrt((x*x + y*y) + z*z)
  * the samples of a segment are np.linspace's: start + i * (delta / div), the last one the end point itself; when a
    component of delta / div is zero numpy switches to (i / div) * delta + start for all three
  * the trilinear sum has eight terms ((wx * wy) * wz) * c, added left to right, the volume values promoted from float32
  * a new node is base + (delta / |delta|) * min(step * (i + 1), |delta|); its float32 copy is that value rounded
  * the nearest node minimises |q - float32 node| in float64, the lowest index among equal distances
The two goal tests of run() and the reachable mask are float32, sqrtf((x*x + y*y) + z*z) of float32 differences.

Off the grid: a sample outside [0, dim-1] counts as blocked, at exactly dim-1 the upper corner (weight 0) is clamped, and a
direct line of length zero ends the run as reached.

Margins.  The reference's own sums cannot be read off (np.linalg.norm goes through BLAS ddot, torch.norm through a vectorised
reduction), so "the same tree" is a fair demand only where no decision hangs on the last bits.  Every decision taken notes
how far its two sides are apart, in rounding units of the arithmetic that decides it (2^-52 or 2^-24 relative to the larger
side; coordinates against the grid bounds relative to the bound):
  dist      a float64 distance against a threshold (steer, reachable)
  sdf       an interpolated value against collision_thre
  bounds    a sample coordinate against 0 and dim-1
  nearest   best against second-best nearest distance (nodes with identical float32 coordinates excepted)
  goal32    the float32 goal tests
  round32   a new coordinate against the float32 rounding boundary nearest to it (its float32 copy feeds `nearest`)
  ceil      the argument of ceil against the nearest integer -- with one qualification.  A steered extension has length
            step*amplifier up to a few rounding units, so its argument |d| / (step / 5) sits ON an integer (50 for step 1,
            amplifier 10) in nearly every iteration, above or below it by the last bit of the norm: no seed at all would pass
            a plain bound.  Within 1000 units of an integer the spec therefore evaluates the segment with BOTH sample counts;
            if they give the same (count, complete) the choice decides nothing (the new nodes do not depend on the sample
            count) and only the sdf / bounds margins of both sets of samples are noted; if they differ, the true (tiny)
            margin is noted and the seed is refused.
`Margins.smallest` is the minimum over all of them; tools/make_rrt_golden.py keeps a seed only if it is >= 1000.
"""
from __future__ import annotations

import math

import numpy as np

EPS64 = 2.0 ** -52
EPS32 = 2.0 ** -24
NEED = 1000.0


class Margins:
    def __init__(self):
        self.by_kind = {}

    def note(self, kind: str, a: float, b: float, eps: float = EPS64, scale: float = None) -> None:
        s = max(abs(a), abs(b)) if scale is None else scale
        u = abs(a - b) / (eps * s) if s > 0 else math.inf
        if u < self.by_kind.get(kind, math.inf):
            self.by_kind[kind] = u

    @property
    def smallest(self) -> float:
        return min(self.by_kind.values(), default=math.inf)


def norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def _interp(vol: np.ndarray, pts: np.ndarray, marg: Margins = None):
    """-> (values float64 [n], inside bool [n]); values of outside samples are 0."""
    X, Y, Z = vol.shape
    hi = np.array([X - 1, Y - 1, Z - 1], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.all((pts >= 0.0) & (pts <= hi), axis=1)
    if marg is not None and len(pts):
        fin = np.isfinite(pts).all(axis=1)
        if fin.any():
            for a in range(3):
                c = pts[fin, a]
                if hi[a] > 0:
                    marg.note("bounds", float(np.min(np.abs(c))), 0.0, scale=hi[a])
                    marg.note("bounds", float(np.min(np.abs(c - hi[a]))), 0.0, scale=hi[a])
    p = np.where(inside[:, None], pts, 0.0)
    i0 = p.astype(np.int64)
    i1 = np.minimum(i0 + 1, np.array([X - 1, Y - 1, Z - 1]))
    d = p - i0
    u = 1.0 - d
    v = vol.astype(np.float64)
    x0, y0, z0 = i0.T
    x1, y1, z1 = i1.T
    dx, dy, dz = d.T
    ux, uy, uz = u.T
    s = ((ux * uy) * uz) * v[x0, y0, z0]
    s = s + ((ux * uy) * dz) * v[x0, y0, z1]
    s = s + ((ux * dy) * uz) * v[x0, y1, z0]
    s = s + ((ux * dy) * dz) * v[x0, y1, z1]
    s = s + ((dx * uy) * uz) * v[x1, y0, z0]
    s = s + ((dx * uy) * dz) * v[x1, y0, z1]
    s = s + ((dx * dy) * uz) * v[x1, y1, z0]
    s = s + ((dx * dy) * dz) * v[x1, y1, z1]
    return np.where(inside, s, 0.0), inside


def _samples(pa: np.ndarray, pb: np.ndarray, num: int) -> np.ndarray:
    if num == 1:
        return pa[None, :].copy()
    div = float(num - 1)
    delta = pb - pa
    st = delta / div
    i = np.arange(num, dtype=np.float64)[:, None]
    pts = (i / div) * delta + pa if np.any(st == 0.0) else i * st + pa
    pts[-1] = pb
    return pts


def _count(vol, pa, pb, num, thre, marg):
    pts = _samples(pa, pb, num)
    val, inside = _interp(vol, pts, marg)
    if marg is not None and inside.any():
        v = val[inside]
        scale = np.maximum(np.abs(v), abs(thre))
        k = int(np.argmin(np.where(scale > 0, np.abs(v - thre) / np.where(scale > 0, scale, 1.0), np.inf)))
        marg.note("sdf", float(v[k]), thre)
    free = inside & (val > thre)
    if free.all():
        return max((num - 1) // 5, 1), True
    fb = int(np.argmin(free))
    return (fb - 1) // 5, False


def collision_free(pa, pb, vol, step_size=1.0, collision_thre=0.5, marg: Margins = None):
    """is_collision_free -> (num_collision_free, complete_free)."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    e = pb - pa
    arg = norm3(e[0], e[1], e[2]) / (step_size / 5.0)
    if not arg < 1.0e9:
        return -1, False
    c = int(math.ceil(arg))
    r = round(float(arg))
    res = _count(vol, pa, pb, c + 1, collision_thre, marg)
    if marg is not None and arg > 0.0 and abs(arg - r) < NEED * EPS64 * arg:
        other = r + 1 if c == r else r                    # ceil of a value a hair on the other side of r
        if _count(vol, pa, pb, other + 1, collision_thre, marg) != res:
            marg.note("ceil", float(arg), float(r))
    elif marg is not None and arg > 0.0:
        marg.note("ceil", float(arg), float(r))
    return res


class SpecRRT:
    """The tree of RRTNaruto for explicit random rows.  Nodes are rows of xyz64 / xyz32, parents are indices (-1: the start)."""

    def __init__(self, vol, step_size=1.0, step_amplifier=10, collision_thre=0.5, enable_direct_line=True):
        self.vol = np.ascontiguousarray(vol, dtype=np.float32)
        self.step, self.amp, self.thre, self.direct = float(step_size), float(step_amplifier), float(collision_thre), bool(enable_direct_line)
        self.marg = Margins()

    def start_new_plan(self, start, goal):
        self.goal = np.asarray(goal, dtype=np.float64).copy()
        self.goal32 = self.goal.astype(np.float32)
        self.xyz64 = [np.asarray(start, dtype=np.float64).copy()]
        self.xyz32 = np.zeros((1024, 3), dtype=np.float32)
        self.xyz32[0] = self.xyz64[0].astype(np.float32)
        self.parent = [-1]
        self.rrt_iter = 0
        self.goal_parent = -1

    @property
    def n(self):
        return len(self.parent)

    def nodes_xyz(self):
        return np.array(self.xyz64)

    def nearest(self, q) -> int:
        n32 = self.xyz32[:self.n].astype(np.float64)
        e = q[None, :] - n32
        d = norm3(e[:, 0], e[:, 1], e[:, 2])
        i = int(np.argmin(d))
        if self.n > 1:
            same = np.all(self.xyz32[:self.n] == self.xyz32[i], axis=1)
            if not same.all():
                self.marg.note("nearest", float(d[i]), float(np.min(d[~same])))
        return i

    def _append(self, base_idx, base, e, dist, cnt):
        first = self.n
        for i in range(cnt):
            p = base + (e / dist) * min(self.step * (i + 1), dist)
            if self.n == len(self.xyz32):
                self.xyz32 = np.concatenate([self.xyz32, np.zeros_like(self.xyz32)])
            p32 = p.astype(np.float32)
            for a in range(3):                  # distance to the nearer float32 rounding boundary, in float64 units
                lo, hi = np.nextafter(p32[a], np.float32(-np.inf)), np.nextafter(p32[a], np.float32(np.inf))
                edge = min(abs(p[a] - (float(lo) + float(p32[a])) / 2), abs(p[a] - (float(hi) + float(p32[a])) / 2))
                self.marg.note("round32", edge, 0.0, scale=max(abs(p[a]), 1e-300))
            self.xyz32[self.n] = p32
            self.xyz64.append(p)
            self.parent.append(base_idx if i == 0 else self.n - 1)
        return first

    def _near_goal32(self, rows) -> bool:
        e = self.xyz32[rows] - self.goal32[None, :]
        d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        for v in d:
            self.marg.note("goal32", float(v), self.step, eps=EPS32)
        return bool(np.min(d) < np.float32(self.step))

    def _straight(self) -> bool:
        last = self.n - 1
        pl = self.xyz64[last]
        cnt, _ = collision_free(self.goal, pl, self.vol, self.step, 0.5, self.marg)
        if cnt <= 0:
            return False
        e = self.goal - pl
        dist = norm3(e[0], e[1], e[2])
        if dist == 0.0:
            return True
        self._append(last, pl, e, dist, cnt)
        return self._near_goal32([self.n - 1])

    def _extend(self, rp) -> int:
        near = self.nearest(rp)
        pn = self.xyz64[near]
        e = rp - pn
        dist = norm3(e[0], e[1], e[2])
        reach = self.step * self.amp
        self.marg.note("dist", float(dist), reach)
        pnew = pn + e / dist * min(reach, dist) if dist > reach else rp
        cnt, _ = collision_free(pn, pnew, self.vol, self.step, self.thre, self.marg)
        e = pnew - pn
        dist = norm3(e[0], e[1], e[2])
        if not dist > 0.0:
            cnt = 0
        if cnt > 0:
            self._append(near, pn, e, dist, cnt)
        return max(cnt, 0)

    def run(self, rows, max_iter) -> tuple:
        """-> (target_reachable, rows used)."""
        used = 0
        for _ in range(max_iter):
            self.rrt_iter += 1
            if self.direct and self._straight():
                break
            cnt = self._extend(np.asarray(rows[used], dtype=np.float64))
            used += 1
            if cnt > 0 and self._near_goal32(np.arange(self.n - cnt, self.n)):
                break
        last = self.nearest(self.goal)
        e = self.xyz64[last] - self.goal
        d = norm3(e[0], e[1], e[2])
        self.marg.note("dist", float(d), self.step)
        self.goal_parent = last
        return bool(d <= self.step), used

    def run_full(self, rows, max_iter) -> int:
        for i in range(max_iter):
            self._extend(np.asarray(rows[i], dtype=np.float64))
        return max_iter

    def path(self):
        """Node indices goal.parent, ..., start (find_path without the goal itself)."""
        out, j = [], self.goal_parent
        while j >= 0:
            out.append(j)
            j = self.parent[j]
        return out

    def reachable_mask(self, chunk=1024):
        """-> (mask float32 [X,Y,Z], float64 nearest-node distance [X,Y,Z])."""
        X, Y, Z = self.vol.shape
        g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3)
        n32 = self.xyz32[:self.n]
        n64 = n32.astype(np.float64)
        m = np.empty(len(g), dtype=np.float32)
        dmin = np.empty(len(g), dtype=np.float64)
        for b in range(0, len(g), chunk):
            p = g[b:b + chunk]
            e = p[:, None, :].astype(np.float32) - n32[None, :, :]
            d32 = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
            m[b:b + chunk] = ~(d32.min(axis=1) > np.float32(self.step))
            e = p[:, None, :].astype(np.float64) - n64[None, :, :]
            dmin[b:b + chunk] = norm3(e[..., 0], e[..., 1], e[..., 2]).min(axis=1)
        return m.reshape(X, Y, Z), dmin.reshape(X, Y, Z)


def draw_rows(n, lo3, hi3):
    """n rows of the reference's random stream: what n calls of generate_random_point leave behind (rrt.py:279-297)."""
    return np.random.uniform(np.asarray(lo3, dtype=np.float64), np.asarray(hi3, dtype=np.float64), size=(n, 3))


def replay_fixture(rec):
    """Run the spec on a g12 fixture's volume, start, goal and rows, call by call.  -> (SpecRRT, reachable flags of the run() calls)."""
    s = SpecRRT(rec["vol"], float(rec["step_size"]), float(rec["step_amplifier"]), float(rec["collision_thre"]), bool(rec["direct"]))
    s.start_new_plan(rec["start"], rec["goal"])
    used, flags = 0, []
    for c, upto in zip(rec["calls"], rec["rows_after_call"]):
        rows = rec["rows"][used:upto]
        if c == 0:
            ok, k = s.run(rows, int(rec["max_iter"]))
            assert k == len(rows), f"the spec used {k} rows, the reference {len(rows)}"
            flags.append(ok)
        else:
            s.run_full(rows, int(rec["max_iter"]))
        used = int(upto)
    return s, flags


def same_tree(rec, n, parents, xyz, rrt_iter, flags, path=None) -> None:
    """The criteria of every fixture comparison: node count, parents, rrt_iter, flags and path EXACTLY, coordinates to 1e-12."""
    assert n == len(rec["parents"]), (n, len(rec["parents"]))
    assert np.array_equal(np.asarray(parents, dtype=np.int32), rec["parents"])
    assert int(rrt_iter) == int(rec["rrt_iter"]), (rrt_iter, int(rec["rrt_iter"]))
    assert [bool(f) for f in flags] == [bool(f) for f in rec["reachable"]], (flags, rec["reachable"])
    err = float(np.abs(np.asarray(xyz, dtype=np.float64) - rec["nodes"]).max())
    assert err <= 1e-12, err
    if "path" in rec:
        assert np.array_equal(np.asarray(path, dtype=np.int32), rec["path"])

"""Depth sampling (stage A1, naruto_render.hip: linspace_at, sample_z_input, sample_z_merge, sample_z_jitter) restated in float32 --
numpy, no GPU.  Every operation below is one float32 operation, rounded once, in the order the kernel states them:

  linspace    steps == 1: start.  Otherwise step = (end - start) / (steps - 1); element i is fma(step, i, start) for i < steps // 2
              and fma(-step, steps - i - 1, end) from there on (torch.linspace's two-sided formula)
  inputs      the uniform samples linspace(near, far, nu); the near-surface samples linspace(-range_d, range_d, nr) + d where d > 0,
              linspace(near, far, nr) otherwise (d <= 0, -0.0 and NaN all land there)
  merged row  np.sort of the two lists side by side.  The kernel ranks instead of sorting and keeps the uniform element first among
              equal values; equal float32 values here have equal bits (+0 and -0 never meet: a near-surface sample exists only where
              d > 0), so that order cannot be observed and is not modelled
  no depth    linspace(near, far, n_samples)
  jitter      lo = z[0] for the first sample, else 0.5 * (z[s] + z[s - 1]); up = z[S - 1] for the last one, else
              0.5 * (z[s + 1] + z[s]); v = fma(up - lo, r, lo), r from rand[n, s] or from the device generator at index n * S + s

The three multiply-adds are ONE operation each, a fused multiply-add, because that is what the kernel computes: it wrote them with
__fmul_rn / __fadd_rn, which the clang HIP headers define as the plain operators, and hipcc contracts those (naruto_common.h says the
same of load_point); the kernel now writes fmaf.  ``fused=False`` gives the other reading -- product and sum rounded separately, what
np.float32 arithmetic does unaided -- which the stand-alone kernel missed at 98 of the 200 settings of the first (near, far) (at a
tie of step * k the two differ by an ulp of the sum, e.g. 0x1p-28 against 0x1p-27 for the middle element of linspace(-0.1, 0.1, 11));
the host test measures both readings against the torch oracle.

So the expectation is bit for bit wherever it is not NaN (the payload and sign of inf - inf differ between hosts and the device: NaN
positions are compared, NaN bits are not).  boundary_depths / special_depths are the depths at which a rank can go wrong; rank_merge
replays the kernel's rank rule on the host to show that they are.
"""
import numpy as np

f32 = np.float32
f64 = np.float64


def fma(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly (helpers.fma32 in numpy): a b is exact in float64; the float64 sum s and its TwoSum
    error e give the exact a b + c rounded to odd, and rounding that to float32 once is the correctly rounded result."""
    a, b, c = (np.asarray(t, dtype=f32).astype(f64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bv = s - p
        e = (p - (s - bv)) + (c - bv)
        odd = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
        return np.where(odd, toward, s).astype(f32)


def _muladd(a, b, c, fused):
    if fused:
        return fma(a, b, c)
    with np.errstate(all="ignore"):
        return (np.asarray(c, dtype=f32) + (np.asarray(a, dtype=f32) * np.asarray(b, dtype=f32)).astype(f32)).astype(f32)


BOUNDARY_CAP = 4096                 # depths per setting
SHIPPED = [(0.0, 5.0, 32, 11, 0.1), (0.0, 5.0, 117, 11, 0.1), (0.0, 5.0, 53, 11, 0.1)]      # (near, far, n_samples_d, n_range_d, range_d)


def linspace_at(start, end, steps, i, fused=True):
    """Element(s) i of linspace(start, end, steps): float32, the shape of i."""
    start, end = f32(start), f32(end)
    i = np.asarray(i, dtype=np.int64)
    if steps == 1:
        return np.full(i.shape, start, dtype=f32)
    with np.errstate(all="ignore"):
        step = f32(f32(end - start) / f32(steps - 1))
    low = _muladd(step, i.astype(f32), start, fused)
    high = _muladd(-step, (steps - i - 1).astype(f32), end, fused)
    return np.where(i < steps // 2, low, high).astype(f32)


def linspace(start, end, steps, fused=True):
    return linspace_at(start, end, steps, np.arange(steps), fused)


def ray_inputs(target_d, near, far, nu, nr, range_d, fused=True):
    """[n, nu + nr] float32: the uniform list, then the near-surface list of every ray."""
    d = np.asarray(target_d, dtype=f32).reshape(-1)
    out = np.empty((d.shape[0], nu + nr), dtype=f32)
    out[:, :nu] = linspace(near, far, nu, fused)
    if nr:
        with np.errstate(all="ignore"):
            around = linspace(-f32(range_d), f32(range_d), nr, fused)[None, :] + d[:, None]
        out[:, nu:] = np.where((d > 0)[:, None], around, linspace(near, far, nr, fused)[None, :])
    return out


def jitter_bounds(z):
    """lo, up [n, S] float32: the stratum of every sample."""
    z = np.asarray(z, dtype=f32)
    with np.errstate(all="ignore"):
        mids = f32(0.5) * (z[:, 1:] + z[:, :-1])
    return np.concatenate([z[:, :1], mids], 1), np.concatenate([mids, z[:, -1:]], 1)


def jitter(z, r, fused=True):
    lo, up = jitter_bounds(z)
    with np.errstate(all="ignore"):
        width = (up - lo).astype(f32)
    return _muladd(width, r, lo, fused)


def device_rand(seed, counter, n_rays, S):
    """The numbers the kernels draw for iteration ``counter``: rand[n, s] = rng_uniform(key, n * S + s)."""
    import helpers as H
    return H.device_rng_uniform(seed, counter, range(n_rays * S)).reshape(n_rays, S)


def sample_z(n_rays, target_d, near, far, n_samples_d, n_range_d, range_d, rand=None, n_samples=0, rng=None, fused=True):
    """z_vals [n_rays, S] float32.  ``rand`` [n_rays, S]: the explicit jitter; ``rng`` = (seed, counter): the device generator's;
    neither: no jitter.  ``target_d`` None: linspace(near, far, n_samples) in every row."""
    if target_d is None:
        z = np.tile(linspace(near, far, n_samples, fused), (n_rays, 1))
    else:
        z = np.sort(ray_inputs(target_d, near, far, n_samples_d, n_range_d, range_d, fused), axis=1)
        assert z.shape[0] == n_rays
    if rand is None and rng is not None:
        rand = device_rand(rng[0], rng[1], n_rays, z.shape[1])
    return z if rand is None else jitter(z, rand, fused)


# ---- the depths at which a rank can go wrong ----
def boundary_depths(near, far, nu, nr, range_d, cap=BOUNDARY_CAP):
    """The depths at which near-surface sample k meets uniform sample i exactly -- float32(u_i - r_k) -- and one ulp either side of
    that, for the pairs (i, k); only depths > 0; (value, up, down) per pair, pair after pair.  At most ``cap`` depths: where there
    are more than cap // 3 pairs, m = cap // 3 of them are taken at a fixed stride, pair j = (j * nu // m, j mod nr) -- m >= nu and
    m >= nr (asserted), so every i and every k still appears."""
    if nu == 0 or nr == 0:
        return np.zeros(0, dtype=f32)
    u, r = linspace(near, far, nu), linspace(-f32(range_d), f32(range_d), nr)
    m = cap // 3
    if nu * nr <= m:
        i, k = np.divmod(np.arange(nu * nr), nr)
    else:
        assert m >= nu and m >= nr, f"cap {cap} cannot hold every one of {nu} + {nr} samples"
        j = np.arange(m)
        i, k = j * nu // m, j % nr
        assert len(set(i.tolist())) == nu and len(set(k.tolist())) == nr
    v = (u[i] - r[k]).astype(f32)
    d = np.stack([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))], 1).reshape(-1)
    return d[d > 0]


def special_depths(near, far, range_d=0.1):
    return np.array([0.0, -0.0, -1.0, np.nan, np.inf, 2.0 ** -126, near, far, f32(far) + f32(range_d), 250.0, 2.0 ** 24], dtype=f32)


def pick(depths, n):
    """At most n of the depths, spread over the whole list (a fractional stride: value, up and down of a pair all stay represented)."""
    depths = np.asarray(depths, dtype=f32)
    return depths if len(depths) <= n else depths[np.arange(n) * len(depths) // n]


# ---- the parameter grid of the stand-alone kernel ----
NEAR_FAR = [(0.0, 5.0), (0.0, 4.0), (0.01, 7.3)]
GRID_ND = [0, 1, 2, 21, 32, 33, 53, 117, 1013]
GRID_NR = [0, 1, 2, 5, 11, 32]
GRID_RANGE = [0.0, 0.1, 0.25, 3.0]
MAX_SAMPLES = 1024                  # kMaxSamples
ALMOST_ONE = f32(1.0 - 2.0 ** -24)  # the largest float32 below 1, the largest draw


def grid(near, far):
    """Every (near, far, n_samples_d, n_range_d, range_d) of the grid with 2 <= S <= 1 024."""
    return [(near, far, nd, nr, rd) for nd in GRID_ND for nr in GRID_NR for rd in GRID_RANGE if 2 <= nd + nr <= MAX_SAMPLES]


def setting_inputs(setting):
    """A setting's depths (special, boundary, 256 random ones in (0, 1.3 far)) and its explicit jitter: row 0 all 0, row 1 all
    1 - 2^-24 (both ends of every stratum), the rest multiples of 2^-24 in [0, 1) as the device generator draws them."""
    near, far, nd, nr, rd = setting
    rs = np.random.RandomState(1000 * nd + 10 * nr + int(10 * rd) + int(far))
    d = np.concatenate([special_depths(near, far, rd), boundary_depths(near, far, nd, nr, rd),
                        rs.uniform(0.0, 1.3 * far, 256).astype(f32)]).astype(f32)
    rand = (rs.randint(0, 1 << 24, (len(d), nd + nr)) * 2.0 ** -24).astype(f32)
    rand[0], rand[1] = 0.0, ALMOST_ONE
    return d, rand


# ---- the launch forms that sample: training forward and eval render ----
FORM_SPLITS = [(32, 11), (53, 11), (64, 11), (117, 11)]      # S = 43, 64 (Short), 75 (the partial walk), 128 (the exact walk)


def form_depths(near, far, nd, nr, range_d, n_boundary=1200):
    """The depths of a launch-form case: at most n_boundary of the setting's boundary depths, then 0, -1, NaN and far.  (inf, 250 and
    2^24 stay with the stand-alone kernel: they put sample points far outside anything the field kernels are tested at.)"""
    return np.concatenate([pick(boundary_depths(near, far, nd, nr, range_d), n_boundary), np.array([0.0, -1.0, np.nan, far], dtype=f32)]).astype(f32)


def form_rand(n_rays, S, seed):
    rand = (np.random.RandomState(seed).randint(0, 1 << 24, (n_rays, S)) * 2.0 ** -24).astype(f32)
    rand[0], rand[1] = 0.0, ALMOST_ONE
    return rand


# ---- comparison ----
def mismatch(got, want, depths, what):
    """None, or the message of the first ray whose row differs: bitwise on the non-NaN elements, NaN positions must coincide."""
    got, want = np.ascontiguousarray(got, dtype=f32), np.ascontiguousarray(want, dtype=f32)
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, the twin's {want.shape}"
    bad = np.isnan(got) != np.isnan(want)
    bad |= (got.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(want)
    if not bad.any():
        return None
    n = int(np.argmax(bad.any(1)))
    s = np.flatnonzero(bad[n])
    d = "none" if depths is None else float(np.asarray(depths, dtype=f32).reshape(-1)[n]).hex()
    return (f"{what}: {int(bad.any(1).sum())} of {got.shape[0]} rows differ; first: ray {n}, depth {d}, samples {s[:8].tolist()}: got "
            f"{[float(x).hex() for x in got[n, s[:4]]]}, the twin {[float(x).hex() for x in want[n, s[:4]]]}")


# ---- the kernel's rank rule, replayed ----
def rank_merge(us, nu, nr, walk_up=True, walk_down=True):
    """sample_z_merge for every element of one ray in plain Python: ``us`` = the uniform list [0, nu), then the near-surface list
    [nu, nu + nr).  The estimate's arithmetic is np.float32, operation by operation; ``walk_up`` / ``walk_down`` = False drop one of
    the two correction walks.  Returns the merged row (a slot nothing was written to holds NaN) and the number of writes per slot."""
    us = [f32(x) for x in np.asarray(us, dtype=f32).reshape(-1)]
    S = nu + nr
    zs, writes = np.full(S, np.nan, dtype=f32), np.zeros(S, dtype=np.int64)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        u0 = us[0] if nu else zero
        u_step = (us[nu - 1] - us[0]) / f32(nu - 1) if nu > 1 else zero
        r0 = us[nu] if nr else zero
        r_step = (us[nu + nr - 1] - us[nu]) / f32(nr - 1) if nr > 1 else zero
        for s in range(S):
            v = us[s]
            if u_step < zero or r_step < zero:                  # descending input (no shipped config): the plain scans
                if s < nu:
                    rank = s + sum(1 for k in range(nr) if us[nu + k] < v)
                else:
                    lo, hi = 0, nu
                    while lo < hi:
                        mid = (lo + hi) >> 1
                        if us[mid] <= v:
                            lo = mid + 1
                        else:
                            hi = mid
                    rank = (s - nu) + lo
            elif s < nu:                                        # uniform element: rank = i + #{R < U[i]}
                e = (v - r0) / r_step
                c = 0 if not e > zero else (nr if e >= f32(nr) else int(e))
                while walk_up and c < nr and us[nu + c] < v:
                    c += 1
                while walk_down and c > 0 and not us[nu + c - 1] < v:
                    c -= 1
                rank = s + c
            else:                                               # near-surface element: rank = k + #{U <= R[k]}
                e = (v - u0) / u_step + f32(1.0)
                c = 0 if not e > zero else (nu if e >= f32(nu) else int(e))
                while walk_up and c < nu and us[c] <= v:
                    c += 1
                while walk_down and c > 0 and not us[c - 1] <= v:
                    c -= 1
                rank = (s - nu) + c
            zs[rank] = v
            writes[rank] += 1
    return zs, writes

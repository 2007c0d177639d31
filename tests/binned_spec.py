"""The binned table scatter (naruto_binned.hip: k_bin_count .. k_bin_apply) restated in exact integer arithmetic -- numpy, no GPU.

What a level of more than 2^17 entries must receive from a list of points x [M,3] with cotangents c [M,32]:

  positions   pos = float32(float64(scale) * x + 0.5): the kernel's fmaf (helpers.hash_encode_cells says why one rounding of the
              fp64 position is the fused multiply-add); cell = floor(pos), (uint32)(int) of it, corner indices from
              oracle.spec_torch.hash_grid_index
  weights     w = pos - cell in fp32; ux = fl32(1 - wx); wyz[q] = fl32((q & 1 ? wy : 1 - wy) * (q & 2 ? wz : 1 - wz)), q = dy + 2 dz
  items       per feature f: a_f = fl32(wyz[q] * g_f); the pair's x0 corner receives a_f * ux, its x1 corner a_f * wx
  lattice     |a_f| < 2047: the exact product of the two fp32 numbers (48 bits: exact in fp64), rounded to nearest-even onto the
              2^-40 lattice -- the fma with kFixMagic (fix40_prod).  Otherwise to_fix40 (naruto_field.hip): v = fl32(a_f * w),
              t = v * 2^8, H = rint(t), r = t - H exact, L = trunc(r * 2^32) saturated to int32 (r = +1/2 gives 2^31 - 1),
              contribution = H * 2^32 + L
  range       a feature with !(|g_f| < 2^22) -- NaN, Inf, too large -- contributes nothing at any corner (the
              tiled scatter's per-point, per-feature test); a point whose two components are zero or dropped makes no item
  sum         integers per entry, modulo 2^64 in two's complement like the kernel's LDS accumulator (numpy int64 addition wraps the
              same way; no float64 accumulation anywhere), then float32(float64(sum) * 2^-40)

Every step is one determinate rounding and the sum is an integer: on binned levels the expectation is bit for bit.  Only the
entries the points touch are formed (sorted entry numbers + values): no table is allocated.
"""
import numpy as np
import torch

from oracle import spec_torch as S

BIN_LOG2 = 13                       # kBinLog2: 8 192 entries per bin
BIN_ENTRIES = 1 << BIN_LOG2
TILED_MAX = 1 << 17                 # levels of up to 2^17 entries stay with the LDS-tiled scatter
MAGIC_RANGE = np.float32(2047.0)    # kFixMagicRange
G_RANGE = np.float32(4194304.0)     # 2^22: the fixed point's range, the contract's bound on a cotangent

_f32, _f64, _i64 = np.float32, np.float64, np.int64


def meta_for(log2_T, desired_resolution=1024):
    """Level tables of config.unit_cube_config(desired_resolution, log2_T) without the field or its table."""
    return S.HashGridMeta.from_desired_resolution(desired_resolution, log2_hashmap_size=log2_T)


def binned_levels(meta):
    return [l for l in range(meta.n_levels) if int(meta.size[l]) > TILED_MAX]


def is_hashed(meta, lvl):
    return int(meta.size[lvl]) < int(meta.resolution[lvl]) ** 3


def n_bins(meta, lvl):
    return (int(meta.size[lvl]) + BIN_ENTRIES - 1) // BIN_ENTRIES


def level_geometry(meta, lvl, x):
    """x [M,3] float32 -> idx [M,8] int64 (corner c = dx + 2 dy + 4 dz, within the level), wx, ux [M] and wyz [M,4], all fp32."""
    x = np.ascontiguousarray(x, dtype=_f32)
    pos = (x.astype(_f64) * _f64(meta.scale[lvl]) + 0.5).astype(_f32)
    cell = np.floor(pos)
    w = (pos - cell).astype(_f32)
    u = (_f32(1.0) - w).astype(_f32)
    gi = torch.from_numpy(cell.astype(_i64) & S.U32)
    idx = np.empty((x.shape[0], 8), _i64)
    for c in range(8):
        cc = [(gi[:, d] + ((c >> d) & 1)) & S.U32 for d in range(3)]
        idx[:, c] = S.hash_grid_index(meta, lvl, cc[0], cc[1], cc[2]).numpy()
    wyz = np.stack([((w[:, 1] if q & 1 else u[:, 1]) * (w[:, 2] if q & 2 else u[:, 2])).astype(_f32) for q in range(4)], axis=1)
    return idx, w[:, 0].copy(), u[:, 0].copy(), wyz


def fix40_magic(a, w):
    """fma((double)a, (double)w, kFixMagic) read back as an integer: the exact product on the 2^-40 lattice, ties to even."""
    return np.rint(a.astype(_f64) * w.astype(_f64) * 2.0 ** 40).astype(_i64)


def fix40_split(a, w):
    """to_fix40(a * w) as written in naruto_field.hip."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = (a.astype(_f32) * w.astype(_f32)).astype(_f32)
        t = (v * _f32(256.0)).astype(_f32)
        t = np.where(np.abs(t) < _f32(1073741824.0), t, _f32(0.0)).astype(_f32)          # NaN compares false
    hf = np.rint(t).astype(_f32)
    r = (t - hf).astype(_f32)                                                           # exact, in [-1/2, 1/2]
    lo = np.minimum(np.trunc(r.astype(_f64) * 4294967296.0), 2147483647.0).astype(_i64)  # v_cvt_i32_f32 saturates
    return hf.astype(_i64) * (1 << 32) + lo


def fix40_prod(a, w):
    """fix40_prod of naruto_binned.hip, elementwise; a, w float32 arrays of one shape."""
    a, w = np.asarray(a, _f32), np.asarray(w, _f32)
    magic = np.abs(a) < MAGIC_RANGE
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(magic, fix40_magic(np.where(magic, a, _f32(0.0)), w), fix40_split(np.where(magic, _f32(0.0), a), w))
    return out.astype(_i64)


def in_range(g):
    """The range contract, per feature component: only |g| < 2^22 contributes."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(g, _f32)) < G_RANGE


def fix_to_float(s):
    """k_bin_apply's output: (float)((double)(long long)sum * 2^-40)."""
    return (np.asarray(s, _i64).astype(_f64) * 2.0 ** -40).astype(_f32)


class LevelTwin:
    """One binned level's expectation.  entries: sorted entry numbers within the whole table (level offset included); fixed [n,2]:
    the integer sums; values [n,2]: the fp32 gradient; counts [n]: corner visits per entry; straddles: x-pairs whose two corners lie
    in different bins; bins: the level-local bins that receive an item."""

    def __init__(self, entries, fixed, counts, straddles, bins):
        self.entries, self.fixed, self.counts, self.straddles, self.bins = entries, fixed, counts, straddles, bins
        self.values = fix_to_float(fixed)


def twin_level(meta, lvl, x, g):
    """x [M,3] float32, g [M,2] float32 (the level's two cotangent components) -> LevelTwin."""
    g = np.array(g, dtype=_f32, copy=True)
    g[~in_range(g)] = 0.0
    live = ~((g[:, 0] == 0.0) & (g[:, 1] == 0.0))
    x, g = np.asarray(x, _f32)[live], g[live]
    idx, wx, ux, wyz = level_geometry(meta, lvl, x)
    keys, vals = [], []
    straddles = 0
    for q in range(4):
        a = (wyz[:, q:q + 1] * g).astype(_f32)                        # [m,2]: a_f = fl32(wyz * g_f)
        i0, i1 = idx[:, 2 * q], idx[:, 2 * q + 1]
        straddles += int(np.count_nonzero((i0 >> BIN_LOG2) != (i1 >> BIN_LOG2)))
        keys += [i0, i1]
        vals += [fix40_prod(a, np.broadcast_to(ux[:, None], a.shape)), fix40_prod(a, np.broadcast_to(wx[:, None], a.shape))]
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    if keys.size == 0:
        z = np.zeros(0, _i64)
        return LevelTwin(z, np.zeros((0, 2), _i64), z, 0, z)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    fixed = np.add.reduceat(vals, first, axis=0)                      # int64: exact, wraps modulo 2^64 like the accumulator
    counts = np.diff(np.concatenate([first, [keys.size]]))
    entries = keys[first]
    return LevelTwin(entries + int(meta.offset[lvl]), fixed, counts, straddles, np.unique(entries >> BIN_LOG2))


def twin(meta, x, c, levels=None):
    """x [M,3], c [M,32] -> {level: LevelTwin} for the binned levels (or the given ones)."""
    c = np.asarray(c, _f32)
    return {l: twin_level(meta, l, x, c[:, 2 * l:2 * l + 2]) for l in (binned_levels(meta) if levels is None else levels)}


# ------------------------------------------------------------------------------------------------ constructed inputs
def straddle_points(meta, lvl, how, n, rs):
    """n points whose x-pairs on level ``lvl`` straddle two bins.
    "dense":  a dense level; cells whose x0 corner's index is 8191 mod 8192 (the x1 corner opens the next bin)
    "minus1": a hashed level; gx = -1, so the x1 corner's gx wraps to 0 and every low bit of the index flips
    "carry":  a hashed level; gx = 8191 mod 8192, i.e. x near 8191.3 / scale, far outside the box"""
    scale = float(meta.scale[lvl])
    res = int(meta.resolution[lvl])
    frac = rs.uniform(0.15, 0.85, (n, 3))
    if how == "dense":
        assert not is_hashed(meta, lvl)
        g = np.arange(res - 1, dtype=_i64)
        gz, gy, gx = np.meshgrid(g, g, g, indexing="ij")
        lin = (gx + gy * res + gz * res * res).reshape(-1)
        hit = np.flatnonzero(lin % BIN_ENTRIES == BIN_ENTRIES - 1)
        assert hit.size > 0
        pick = hit[rs.randint(0, hit.size, n)]
        cell = np.stack([gx.reshape(-1)[pick], gy.reshape(-1)[pick], gz.reshape(-1)[pick]], axis=1).astype(_f64)
    else:
        assert is_hashed(meta, lvl)
        cell = rs.randint(0, res - 1, (n, 3)).astype(_f64)
        cell[:, 0] = -1.0 if how == "minus1" else 8191.0
    return ((cell + frac - 0.5) / scale).astype(_f32)


def mixed_points(rs, n=3000):
    """The twin case's list: uniform points, 300 in one cell (offsets <= 1e-5), 200 exact repeats, points in [-0.6, 1.6], the corners
    0, 1 and the centre; 20 % zero cotangents and one point with g.x = 0, g.y != 0 on every level."""
    n_uni = n - 300 - 200 - 400 - 3
    uni = rs.uniform(0, 1, (n_uni, 3))
    same = np.array([[0.4137, 0.2871, 0.6312]]) + rs.uniform(0, 1e-5, (300, 3))
    x = np.concatenate([uni, same, uni[:200], rs.uniform(-0.6, 1.6, (400, 3)), np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5]])]).astype(_f32)
    c = rs.normal(size=(n, 32)).astype(_f32)
    c[rs.uniform(size=n) < 0.2] = 0.0
    c[7, 0::2] = 0.0
    c[7, 1::2] = 0.75
    return x, c


def bad_cotangents(c, every=97):
    """Range-contract case: every 97th point bad, in rotation NaN, Inf, 1e9, 5e6, and feature 0 NaN beside a finite feature 1.
    Returns the cotangents with the bad components in place and with exactly those components zeroed."""
    c_bad, c_zero = c.copy(), c.copy()
    bad = np.arange(0, c.shape[0], every)
    for k, val in enumerate((np.nan, np.inf, 1e9, 5e6)):
        c_bad[bad[k::5]] = val
        c_zero[bad[k::5]] = 0.0
    rows = bad[4::5]
    c_bad[rows, 0::2] = np.nan
    c_zero[rows, 0::2] = 0.0
    return c_bad, c_zero

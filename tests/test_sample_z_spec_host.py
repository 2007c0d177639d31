"""Depth sampling's float32 twin (sample_z_spec.py) checked on the CPU: against the torch oracle, on its own properties, and -- with
a host replay of the kernel's rank rule -- that the boundary depths reach the ranks random depths miss.  Plus the argument checks
of naruto_sample_z, which need no device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import spec_torch as S

import sample_z_spec as Z

f32 = np.float32

# Twin against oracle, measured on this grid over every (near, far), keyed by (fused, jittered); the assertions allow twice these.
# (fused, no jitter) measured 0 -- the twin IS torch's CPU linspace, bit for bit; one ulp of the row's magnitude is allowed there, for
# a torch build whose linspace does not fuse, and the element figure (then pure cancellation) is not asserted.
ROW_ULPS = {(True, False): 0.5, (True, True): 2.0, (False, False): 2.0, (False, True): 2.0}       # in ulps of the row's largest finite magnitude
ELEMENT_ULPS = {(True, False): np.inf, (True, True): 30975.0, (False, False): 16777215.0, (False, True): 131072.0}   # in ulps of max(|a|, |b|) of the element


def _ulps(a, b, scale):
    with np.errstate(all="ignore"):
        return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(scale, f32(2.0 ** -126))).astype(np.float64)


@pytest.mark.parametrize("near,far", Z.NEAR_FAR)
def test_twin_against_the_torch_oracle(near, far):
    """The twin and oracle.spec_torch.sample_z over the grid of the GPU test (sample_z_spec.grid: special, boundary and random depths
    per setting; 231 M elements per jitter setting), without jitter and with the explicit rand, in both readings of the multiply-adds.

    Measured here, over the finite elements (NaN and inf positions are equal in every case):
      * fused (the kernel's arithmetic, the twin's default): without jitter NOT ONE element differs from the oracle -- torch's CPU
        linspace fuses its multiply-add too; with jitter 0.4 % differ (torch's eager `lower + (upper - lower) * rand` rounds twice), by
        at most 2 ulps of the row's largest finite magnitude, 30 975 ulps of the element itself;
      * unfused (product and sum rounded separately): 8 - 11 % differ, with and without jitter, by at most 2 ulps of the row's
        magnitude (4.8e-7); of the element itself 16 777 215 ulps without jitter ((0, 4), 21 + 11, range_d 3: 2^-23 where the oracle
        has 0) and 131 072 with it.
    The element figures are cancellation, not disagreement: at a boundary depth d = u_i - r_k a near-surface sample r_k + d lands
    within an ulp of r_k of a uniform one -- or of zero -- and one ulp of r_k is then millions of ulps of the result; a jittered value
    can land anywhere near zero.  They are asserted as measured and bound next to nothing; the row figures are the check.  The bounds
    are twice the measurement: one more rounding in the jitter's multiply-add.  They hold against the oracle, never against the
    kernel (which is compared with the twin bit for bit).

    A NaN depth is left out: the oracle's `target_d <= 0` is false for it and its rows turn NaN, while the kernel's contract
    (`!(d > 0)`, stated by the twin) samples such a ray like one without a depth."""
    worst_row, worst_el = {k: 0.0 for k in ROW_ULPS}, {k: 0.0 for k in ROW_ULPS}
    differ, total = {k: 0 for k in ROW_ULPS}, {k: 0 for k in ROW_ULPS}
    for setting in Z.grid(near, far):
        _, _, nd, nr, rd = setting
        d, rand = Z.setting_inputs(setting)
        keep = ~np.isnan(d)
        d, rand = d[keep], rand[keep]
        n = len(d)
        oracle = {j: S.sample_z(n, torch.from_numpy(d)[:, None], near, far, nd, nr, rd, 1.0 if j else 0.0,
                                rand=torch.from_numpy(rand) if j else None).numpy() for j in (False, True)}
        for key in ROW_ULPS:
            fused, j = key
            a, b = Z.sample_z(n, d, near, far, nd, nr, rd, rand=rand if j else None, fused=fused), oracle[j]
            what = f"{setting} {'fused' if fused else 'unfused'} {'rand' if j else 'no jitter'}"
            assert a.shape == b.shape == (n, nd + nr), what
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)), f"{what}: NaN / inf positions"
            assert not np.isneginf(a).any() and not np.isneginf(b).any(), what
            fin = np.isfinite(a)
            a0, b0 = np.where(fin, a, f32(0)), np.where(fin, b, f32(0))
            mag = np.maximum(np.abs(a0), np.abs(b0))
            row = _ulps(a0, b0, mag.max(1, keepdims=True))
            el = _ulps(a0, b0, mag)
            worst_row[key], worst_el[key] = max(worst_row[key], float(row.max())), max(worst_el[key], float(el.max()))
            differ[key] += int((row > 0).sum())
            total[key] += int(fin.sum())
            assert row.max() <= 2 * ROW_ULPS[key], f"{what}: {row.max()} ulps of the row's magnitude, ray depth {float(d[int(row.max(1).argmax())]).hex()}"
            assert el.max() <= 2 * ELEMENT_ULPS[key], f"{what}: {el.max()} ulps of the element, ray depth {float(d[int(el.max(1).argmax())]).hex()}"
    print(f"twin vs oracle ({near}, {far}), (fused, jittered): differing {differ} of {total}")
    print(f"twin vs oracle ({near}, {far}): row ulps {worst_row}, element ulps {worst_el}")


@pytest.mark.parametrize("setting", Z.SHIPPED + [(0.0, 4.0, 33, 5, 0.25), (0.01, 7.3, 2, 32, 3.0), (0.0, 5.0, 0, 11, 0.1), (0.0, 5.0, 21, 0, 0.0)])
def test_twin_properties(setting):
    """Unjittered rows are non-decreasing; each row is a permutation of its two input lists; jittered values lie in [lo, up] (rows
    that hold an inf: wherever lo and up are both finite)."""
    near, far, nd, nr, rd = setting
    d, rand = Z.setting_inputs(setting)
    n = len(d)
    z = Z.sample_z(n, d, near, far, nd, nr, rd)
    assert not np.isnan(z).any()
    assert (z[:, 1:] >= z[:, :-1]).all()
    ins = Z.ray_inputs(d, near, far, nd, nr, rd)
    assert np.array_equal(np.sort(ins, 1).view(np.uint32), z.view(np.uint32))
    assert np.array_equal(ins[:, :nd], np.tile(Z.linspace(near, far, nd), (n, 1)))
    no_depth = ~(d > 0)
    assert no_depth[:4].all() and np.array_equal(ins[no_depth, nd:], np.tile(Z.linspace(near, far, nr), (int(no_depth.sum()), 1)))
    lo, up = Z.jitter_bounds(z)
    v = Z.sample_z(n, d, near, far, nd, nr, rd, rand=rand)
    ok = np.isfinite(lo) & np.isfinite(up)
    assert ok[np.isfinite(d)].all() and (lo[ok] <= up[ok]).all()
    assert (v[ok] >= lo[ok]).all() and (v[ok] <= up[ok]).all()
    assert np.array_equal(v[0][ok[0]], lo[0][ok[0]])                  # r = 0: the lower end, exactly
    # the device generator's path is the same arithmetic on its own numbers
    assert np.array_equal(Z.sample_z(3, d[:3], near, far, nd, nr, rd, rng=(7, 1)),
                          Z.sample_z(3, d[:3], near, far, nd, nr, rd, rand=Z.device_rand(7, 1, 3, nd + nr)))
    # no depth at all: the uniform list of n_samples
    assert np.array_equal(Z.sample_z(2, None, near, far, 0, 0, 0.0, n_samples=nd + nr), np.tile(Z.linspace(near, far, nd + nr), (2, 1)))


def test_linspace_at_by_hand():
    assert Z.linspace(2.0, 9.0, 1).tolist() == [2.0]
    assert Z.linspace(0.0, 4.0, 33).tolist() == [k / 8 for k in range(33)]
    step = f32(f32(5.0) / f32(31.0))
    exact = Fraction(5) - Fraction(float(step)) * 15                                    # one rounding of the exact value: the fma
    assert Z.linspace_at(0.0, 5.0, 32, 15) == f32(step * f32(15.0)) and Z.linspace_at(0.0, 5.0, 32, 16) == f32(float(exact))
    assert Z.linspace_at(0.0, 5.0, 32, 16, fused=False) == f32(f32(5.0) - f32(step * f32(15.0)))
    # a tie of step * k: the two readings differ (the kernel's is the fused one)
    assert float(Z.linspace(-0.1, 0.1, 11)[5]) == 2.0 ** -28 and float(Z.linspace(-0.1, 0.1, 11, fused=False)[5]) == 2.0 ** -27
    a, b, c = f32(1.0 + 2.0 ** -13), f32(1.0 - 2.0 ** -13), f32(-1.0)
    assert float(Z.fma(a, b, c)) == -2.0 ** -26 and float(f32(a * b) + c) == 0.0
    assert np.isnan(Z.fma(f32(np.inf), 0.0, 1.0)) and Z.fma(f32(np.inf), 1.0, 1.0) == np.inf and Z.fma(1.0, 1.0, f32(-np.inf)) == -np.inf
    assert Z.linspace(0.0, 5.0, 0).shape == (0,)


def test_boundary_depths_cover_every_sample():
    """Under the cap every pair is there; over it every i and every k still is (the stride), and the cap holds."""
    for near, far in Z.NEAR_FAR:
        for setting in Z.grid(near, far):
            _, _, nd, nr, rd = setting
            b = Z.boundary_depths(near, far, nd, nr, rd)
            assert len(b) <= Z.BOUNDARY_CAP and (b > 0).all() and b.dtype == f32
            if nd and nr:
                assert len(b) > 0
    u, r = Z.linspace(0.0, 5.0, 1013), Z.linspace(-0.1, 0.1, 11)
    b = set(Z.boundary_depths(0.0, 5.0, 1013, 11, 0.1).tolist())
    deep = [i for i in range(1013) if u[i] > 0.1]            # (nearer ones lose the pairs whose depth is not > 0)
    assert all(any(float(f32(u[i] - r[k])) in b for k in range(11)) for i in deep)
    assert all(any(float(f32(u[i] - r[k])) in b for i in deep) for k in range(11))
    # under the cap: every pair, three depths each, less the ones that are not > 0 (u_0 = 0 against r_k >= 0)
    v = (Z.linspace(0.0, 5.0, 32)[:, None] - r[None, :]).astype(f32).reshape(-1)
    triples = np.stack([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))], 1).reshape(-1)
    assert np.array_equal(Z.boundary_depths(0.0, 5.0, 32, 11, 0.1), triples[triples > 0])


def _wrong_rows(setting, depths, **walks):
    near, far, nd, nr, rd = setting
    ins = Z.ray_inputs(depths, near, far, nd, nr, rd)
    want = np.sort(ins, 1)
    wrong = []
    for n in range(len(depths)):
        zs, writes = Z.rank_merge(ins[n], nd, nr, **walks)
        if not (np.array_equal(zs.view(np.uint32), want[n].view(np.uint32)) and (writes == 1).all()):
            wrong.append(n)
    return wrong


@pytest.mark.parametrize("setting", Z.SHIPPED)
def test_rank_rule_as_written_sorts_the_boundary_depths(setting):
    """sample_z_merge's estimate and its two walks, replayed on the host, give the sorted row and write every slot exactly once at
    every boundary and special depth of the shipped settings."""
    near, far, nd, nr, rd = setting
    depths = np.concatenate([Z.special_depths(near, far, rd), Z.boundary_depths(near, far, nd, nr, rd)])
    wrong = _wrong_rows(setting, depths)
    assert not wrong, f"{setting}: {len(wrong)} rows wrong, first at depth {float(depths[wrong[0]]).hex()}"


def test_boundary_depths_catch_what_random_depths_miss():
    """A statement about the test data, not about the kernel: with the downward walk removed (an estimate that overshoots is then
    kept) the replay goes wrong on boundary rows of the shipped 32 + 11 sampling -- two elements in one slot, another never written
    -- while 20 000 random depths in (0, 1.3 far) are all still right.  Measured here: 80 of the 1 038 boundary rows."""
    setting = Z.SHIPPED[0]
    near, far, nd, nr, rd = setting
    boundary = Z.boundary_depths(near, far, nd, nr, rd)
    wrong = _wrong_rows(setting, boundary, walk_down=False)
    print(f"walk_down=False: {len(wrong)} of {len(boundary)} boundary rows wrong")
    assert len(wrong) >= 1
    rnd = np.random.RandomState(20).uniform(0.0, 1.3 * far, 20000).astype(f32)
    rnd = rnd[rnd > 0]
    assert not _wrong_rows(setting, rnd, walk_down=False)
    # (and the upward walk is the one every depth needs: without it random rows go wrong too)
    assert _wrong_rows(setting, rnd[:200], walk_up=False)


def test_sample_z_argument_checks(built_lib):
    """naruto_sample_z refuses a NULL output, S < 2 and S > 1 024 with NARUTO_ERR_INVALID, and an empty batch is NARUTO_OK: each
    call returns from the argument checks (no pointer below is ever dereferenced, nothing is launched)."""
    lib = built_lib
    fake = C.c_void_p(0x10000)
    INVALID, OK = -22, 0

    def call(n_rays=4, target_d=fake, nd=32, nr=11, n_samples=0, z=fake):
        return lib.naruto_sample_z(n_rays, target_d, 0.0, 5.0, nd, nr, 0.1, n_samples, None, z, None)
    assert call(z=None) == INVALID
    assert call(n_rays=0, z=None) == INVALID
    assert call(nd=1, nr=0) == INVALID and call(nd=0, nr=1) == INVALID and call(nd=0, nr=0) == INVALID
    assert call(nd=1013, nr=12) == INVALID and call(nd=1024, nr=1) == INVALID
    assert call(target_d=None, n_samples=1) == INVALID and call(target_d=None, n_samples=1025) == INVALID
    assert call(target_d=None, nd=32, nr=11, n_samples=0) == INVALID           # without a depth only n_samples counts
    assert call(n_rays=0) == OK and call(n_rays=0, nd=0, nr=0) == OK and call(n_rays=0, target_d=None) == OK
    assert b"sample_z" in lib.naruto_last_error()

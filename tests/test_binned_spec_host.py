"""The binned scatter's fixed-point twin (binned_spec.py) checked on the CPU: against oracle autograd, on constructed straddles
and on hand-computed values of both conversion branches and of the range contract."""
import numpy as np
import pytest
import torch

from oracle import spec_torch as S

import binned_spec as B
import helpers as H

f32 = np.float32


@pytest.mark.parametrize("log2_T", [18, 20])
def test_twin_against_oracle_autograd(log2_T):
    """2 000 random points, cotangents ~N(0,1): on every binned level the twin agrees with the backward of S.hash_encode to fp32
    accumulation distance (grad_close's bound), and the oracle's gradient is zero wherever the twin has no entry."""
    meta = B.meta_for(log2_T)
    levels = B.binned_levels(meta)
    assert levels == list(range(5, 16))
    assert [l for l in levels if not B.is_hashed(meta, l)] == ([5, 6] if log2_T == 20 else [])
    rs = np.random.RandomState(log2_T)
    x = rs.uniform(0, 1, (2000, 3)).astype(f32)
    c = rs.normal(size=(2000, 32)).astype(f32)
    table = torch.zeros(meta.n_params, requires_grad=True)
    (S.hash_encode(torch.from_numpy(x), table, meta) * torch.from_numpy(c)).sum().backward()
    want = table.grad.reshape(-1, 2)
    tw = B.twin(meta, x, c)
    for l in levels:
        t = tw[l]
        lo, hi = int(meta.offset[l]), int(meta.offset[l]) + int(meta.size[l])
        assert t.entries.min() >= lo and t.entries.max() < hi
        assert int(t.counts.sum()) == 8 * 2000
        H.grad_close(torch.from_numpy(t.values), want[t.entries], f"T{log2_T}.level{l}")
        rest = want[lo:hi].clone()
        rest[t.entries - lo] = 0.0
        assert int(torch.count_nonzero(rest)) == 0, f"level {l}: the oracle touches entries the twin does not"


def test_partial_last_bins_of_the_dense_levels():
    meta = B.meta_for(20)
    assert [int(meta.size[l]) for l in (5, 6)] == [274632, 614128]
    assert [int(meta.size[l]) % B.BIN_ENTRIES for l in (5, 6)] == [4296, 7920]
    assert B.n_bins(B.meta_for(24), 15) == 2048 and B.n_bins(B.meta_for(22), 15) == 512


@pytest.mark.parametrize("how,log2_T,lvl", [("dense", 20, 5), ("dense", 20, 6), ("minus1", 18, 5), ("minus1", 20, 15),
                                            ("carry", 18, 9), ("carry", 20, 15)])
def test_straddle_constructor(how, log2_T, lvl):
    """Every constructed point has at least one x-pair whose corners fall into two bins on the target level (all four on a hashed
    one); uniform points in the box have none on a hashed level."""
    meta = B.meta_for(log2_T)
    rs = np.random.RandomState(7)
    x = B.straddle_points(meta, lvl, how, 64, rs)
    if how == "carry":
        assert abs(float(x[0, 0]) * float(meta.scale[lvl]) - 8191.3) < 1.0
    idx = B.level_geometry(meta, lvl, x)[0]
    per_point = sum(((idx[:, 2 * q] >> B.BIN_LOG2) != (idx[:, 2 * q + 1] >> B.BIN_LOG2)).astype(int) for q in range(4))
    assert (per_point >= 1).all() if how == "dense" else (per_point == 4).all()
    if how == "dense":
        assert (idx[:, 0] % B.BIN_ENTRIES == B.BIN_ENTRIES - 1).all() and (idx[:, 1] == idx[:, 0] + 1).all()
    g = np.ones((64, 2), f32)
    t = B.twin_level(meta, lvl, x, g)
    assert t.straddles == int(per_point.sum()) >= 64
    if how != "dense":
        inside = rs.uniform(0, 1, (2000, 3)).astype(f32)
        assert B.twin_level(meta, lvl, inside, np.ones((2000, 2), f32)).straddles == 0


def test_fix40_branches_by_hand():
    one = 1 << 40

    def fx(a, w):
        return int(B.fix40_prod(np.array([a], f32), np.array([w], f32))[0])

    # |a| < 2047: the exact product, ties to even on the 2^-40 lattice
    assert fx(1.0, 0.5) == one // 2
    assert fx(2.0 ** -40, 0.5) == 0 and fx(3 * 2.0 ** -40, 0.5) == 2 and fx(5 * 2.0 ** -40, 0.5) == 2
    assert fx(-(2.0 ** -40), 0.5) == 0 and fx(-3 * 2.0 ** -40, 0.5) == -2
    assert fx(1.0, 1 - 2.0 ** -24) == one - (1 << 16)
    a = float(f32(2046.9999))                                                       # the last floats below the switch: 24 x 24 bits, exact
    assert fx(a, 1 - 2.0 ** -24) == int(round(a * 2 ** 13)) * ((1 << 24) - 1) * (1 << 3)
    # |a| >= 2047: fp32 product first.  2047 (1 - 2^-24) rounds to 2047 - 2^-13 in fp32; the exact product is 2047 - 2047 2^-24
    assert fx(2047.0, 1 - 2.0 ** -24) == 2047 * one - (1 << 27) != 2047 * one - 2047 * (1 << 16)
    assert fx(4096.0, 0.5) == 2048 * one and fx(-8000.0, 0.25) == -2000 * one
    # the split's low word: r = +1/2 saturates one unit short, r = -1/2 is exact
    assert fx(2048.0, 2.0 ** -20) == (1 << 31) - 1
    assert fx(2048.0, 3 * 2.0 ** -20) == 3 * (1 << 31)
    assert fx(-2048.0, 2.0 ** -20) == -(1 << 31)
    # a small negative contribution of a large a keeps its low bits (the floor / fract split would not)
    assert fx(-4096.0, 2.0 ** -23 + 2.0 ** -40) == -((1 << 29) + (1 << 12))
    assert fx(float("nan"), 0.5) == 0 and fx(float("inf"), 0.5) == 0
    assert float(B.fix_to_float(np.array([3 * one // 2]))[0]) == 1.5


def test_range_contract_by_hand():
    """One point at a cell's centre on level 15 of T = 2^18: the eight corners each receive g / 8, a component outside (-2^22, 2^22)
    nothing, its in-range neighbour all the same."""
    meta = B.meta_for(18)
    lvl = 15
    x = ((np.array([[100.0, 200.0, 300.0]]) + 0.5 - 0.5) / float(meta.scale[lvl])).astype(f32)
    idx, wx, ux, wyz = B.level_geometry(meta, lvl, x)
    ok = B.twin_level(meta, lvl, x, np.array([[1.0, -3.0]], f32))
    assert ok.entries.size == 8 and (ok.counts == 1).all()
    want = np.array([[1.0, -3.0]]) * np.concatenate([wyz[0, q] * np.array([ux[0], wx[0]], np.float64) for q in range(4)])[:, None]
    got = ok.values[np.argsort(np.argsort(idx[0]))]                                      # back into corner order
    assert np.abs(got - want).max() <= 2.0 ** -40 + 2.0 ** -25 * 3
    for bad in (np.nan, np.inf, -np.inf, 1e9, 5e6, 4194304.0, -4194304.0):
        t = B.twin_level(meta, lvl, x, np.array([[bad, -3.0]], f32))
        assert np.array_equal(t.entries, ok.entries) and (t.fixed[:, 0] == 0).all() and np.array_equal(t.fixed[:, 1], ok.fixed[:, 1]), bad
        assert B.twin_level(meta, lvl, x, np.array([[bad, bad]], f32)).entries.size == 0
        assert B.twin_level(meta, lvl, x, np.array([[bad, 0.0]], f32)).entries.size == 0
    # the largest float below 2^22 is in range and takes the fp32 split on every corner (|a| ~ 2^19)
    g = float(np.nextafter(f32(4194304.0), f32(0.0)))
    t = B.twin_level(meta, lvl, x, np.array([[g, 0.0]], f32))
    assert (np.abs(t.fixed[:, 0]) >= 2047 << 40).all()
    assert abs(float(t.values[:, 0].astype(np.float64).sum()) - g) <= 8 * 2.0 ** -4 * 2          # eight corners, four roundings of half an ulp(2^19) each
    c = np.zeros((485, 32), f32) + f32(1e-3)
    c_bad, c_zero = B.bad_cotangents(c)
    assert np.isnan(c_bad[0]).all() and np.isinf(c_bad[97]).all() and (c_bad[194] == f32(1e9)).all() and (c_bad[291] == f32(5e6)).all()
    assert np.isnan(c_bad[388, 0::2]).all() and (c_bad[388, 1::2] == f32(1e-3)).all() and (c_zero[388, 1::2] == f32(1e-3)).all()
    assert np.array_equal(~B.in_range(c_bad), c_zero != c) and int((c_zero != c).sum()) == 4 * 32 + 16

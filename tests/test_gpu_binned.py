"""The binned table scatter (naruto_binned.hip: k_bin_count, k_bin_colscan, k_bin_start, k_bin_fill<1024|512>, k_bin_apply) against its
fixed-point twin (tests/binned_spec.py), bit for bit, at its edges: collisions in one bin, pairs that straddle two bins, dense binned
levels with a partly filled last bin, both branches of fix40_prod, the range contract per feature component, list lengths around the
1 024-point row, 512-point rounds (forced, and natural at T = 2^24 with 2 048 bins per level) and bins gone empty between two written
backwards.

Route: ops.hash_encode(handle, x, table) backward unless a test says otherwise.  The handle is built directly and the table is a zero
tensor on the device (its values do not enter its own gradient); no CPU copy of a table exists anywhere.  Levels of up to 2^17 entries
belong to the LDS-tiled scatter and are compared with oracle autograd by grad_close where they are compared; every other assertion is on
the binned levels and exact.  No tolerance in this file is taken from the code under test: binned_spec.py's header derives the bits."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from oracle import spec_torch as S

import binned_spec as B
import helpers as H
import launch_forms as LF

pytestmark = pytest.mark.gpu

f32 = np.float32


def _handle(log2_T):
    """What NarutoFieldHIP._make_handle builds for config.unit_cube_config(1024, log2_T), without the module or its parameters."""
    from naruto_amd import config as C, ops
    cfg = C.unit_cube_config(1024, log2_T)
    dec, tr = cfg["decoder"], cfg["training"]
    h = ops.FieldHandle(log2_hashmap_size=log2_T, per_level_scale=float(np.exp2(np.log2(1024 / 16) / 15)), n_bins=cfg["pos"]["n_bins"],
                        hidden_dim=dec["hidden_dim"], geo_feat_dim=dec["geo_feat_dim"], hidden_dim_color=dec["hidden_dim_color"],
                        uncert_dims=(8, 8, 8), bbox_min=[0.0, 0.0, 0.0], bbox_max=[1.0, 1.0, 1.0], trunc=tr["trunc"],
                        sc_factor=cfg["data"]["sc_factor"], white_bkgd=tr["white_bkgd"])
    meta = B.meta_for(log2_T)
    scale, res, size, off = h.levels()
    assert np.array_equal(np.asarray(scale, f32), np.asarray(meta.scale, f32)), "the twin's level scales are not the kernel's"
    assert np.array_equal(np.asarray(size), meta.size) and np.array_equal(np.asarray(off), meta.offset) and np.array_equal(np.asarray(res), meta.resolution)
    assert h.n_params == meta.n_params
    return h, meta


@functools.lru_cache(maxsize=None)
def _field(log2_T):
    """(handle, meta, zero table on the device) of T = 2^18 / 2^20, shared by the tests of this module."""
    h, meta = _handle(log2_T)
    return h, meta, torch.zeros(h.n_params, device="cuda:0", requires_grad=True)


def _backward(h, table, x, c):
    """d table of sum(hash_encode(x) * c): x [M,3], c [M,32] numpy or device tensors."""
    from naruto_amd import ops
    dev = table.device
    xt = torch.as_tensor(x).to(dev)
    ct = torch.as_tensor(c).to(dev)
    table.grad = None
    ops.hash_encode(h, xt, table).backward(ct)
    g = table.grad
    table.grad = None
    return g.detach()


def _where(meta, i):
    """Flat gradient index -> (level, entry within the level, feature)."""
    e = int(i) // 2
    lvl = int(np.searchsorted(np.asarray(meta.offset), e, side="right")) - 1
    return lvl, e - int(meta.offset[lvl]), int(i) % 2


def _assert_twin(got, tw, meta, what):
    """The gradient's binned levels equal the twin bit for bit at every entry the twin holds and are zero everywhere else."""
    g2 = got.reshape(-1, 2)
    for lvl, t in tw.items():
        lo, hi = int(meta.offset[lvl]), int(meta.offset[lvl]) + int(meta.size[lvl])
        have = g2[torch.from_numpy(t.entries).to(got.device)].cpu().numpy() if t.entries.size else np.zeros((0, 2), f32)
        diff = np.flatnonzero((have.view(np.int32) != t.values.view(np.int32)).reshape(-1))
        nz = int(torch.count_nonzero(g2[lo:hi]))
        print(f"{what}: level {lvl} ({'hashed' if B.is_hashed(meta, lvl) else 'dense'}, {B.n_bins(meta, lvl)} bins, {t.bins.size} with items) "
              f"{t.entries.size} entries, up to {int(t.counts.max()) if t.counts.size else 0} visits each, {t.straddles} straddling pairs, "
              f"{diff.size} values differ, {nz} nonzero on the device")
        if diff.size:
            k = int(diff[0])
            e = int(t.entries[k // 2]) - lo
            raise AssertionError(f"{what}: level {lvl} entry {e} (bin {e >> B.BIN_LOG2}) feature {k % 2}: device {have.reshape(-1)[k]!r}, twin "
                                 f"{t.values.reshape(-1)[k]!r} (fixed {int(t.fixed.reshape(-1)[k])}, {int(t.counts[k // 2])} visits); "
                                 f"{diff.size} of {have.size} values differ on this level")
        assert nz == int(np.count_nonzero(t.values)), f"{what}: level {lvl}: {nz} nonzero values on the device, {int(np.count_nonzero(t.values))} in the twin"


def _assert_tiled_close(got, meta, x, c, what):
    """The LDS-tiled levels (up to 2^17 entries) against oracle autograd, as in test_hash_encode_backward_large_tables."""
    n_tiled = 2 * int(meta.offset[B.binned_levels(meta)[0]])
    table = torch.zeros(meta.n_params, requires_grad=True)
    (S.hash_encode(torch.from_numpy(x), table, meta) * torch.from_numpy(c)).sum().backward()
    H.grad_close(got[:n_tiled], table.grad[:n_tiled], what)


@functools.lru_cache(maxsize=None)
def _mixed_case(log2_T):
    """The twin case's inputs, its twin and the device's gradient in sparse form (flat indices of the nonzero values, their bits), once."""
    h, meta, table = _field(log2_T)
    x, c = B.mixed_points(np.random.RandomState(100 + log2_T))
    if log2_T == 20:                                   # T = 2^20: some of the list sits on the dense levels' bin boundaries
        rs = np.random.RandomState(5)
        x[500:564] = B.straddle_points(meta, 5, "dense", 64, rs)         # (a fifth of the list has no cotangent)
        x[564:628] = B.straddle_points(meta, 6, "dense", 64, rs)
    got = _backward(h, table, x, c)
    first = 2 * int(meta.offset[B.binned_levels(meta)[0]])
    nz = torch.nonzero(got[first:]).reshape(-1)
    return x, c, B.twin(meta, x, c), got, nz.cpu().numpy(), got[first:][nz].cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------ the twin, bit for bit
@pytest.mark.parametrize("log2_T", [18, 20])
def test_binned_levels_equal_the_twin(gpu, log2_T):
    """T = 2^18: eleven hashed binned levels.  T = 2^20: levels 5 and 6 are dense and binned, with last bins of 4 296 and 7 920 entries.
    3 000 points: uniform ones, 300 in one cell (one bin takes the collisions), 200 exact repeats, points in [-0.6, 1.6] (negative cells:
    gx = -1 straddles on the hashed levels), the corners 0, 1 and the centre; a fifth of the cotangents zero, one point with g.x = 0,
    g.y != 0.  Nothing is written outside the twin's entries."""
    h, meta, table = _field(log2_T)
    x, c, tw, got, _, _ = _mixed_case(log2_T)
    assert sorted(tw) == list(range(5, 16))
    dense = [l for l in tw if not B.is_hashed(meta, l)]
    assert dense == ([5, 6] if log2_T == 20 else [])
    for l in dense:
        assert int(meta.size[l]) % B.BIN_ENTRIES != 0 and tw[l].bins.max() == B.n_bins(meta, l) - 1, "the partly filled last bin takes no item"
        assert tw[l].straddles >= 32
    assert max(int(t.counts.max()) for t in tw.values()) >= 200, "the 300 points of one cell (a fifth without a cotangent) collide"
    _assert_twin(got, tw, meta, f"T{log2_T}.mixed")
    _assert_tiled_close(got, meta, x, c, f"T{log2_T}.mixed.tiled levels")
    perm = np.random.RandomState(1).permutation(x.shape[0])
    assert torch.equal(_backward(h, table, x[perm], c[perm])[2 * int(meta.offset[5]):], got[2 * int(meta.offset[5]):])


# ------------------------------------------------------------------------------------------------ straddles
@pytest.mark.parametrize("how,log2_T,lvl", [("dense", 20, 5), ("dense", 20, 6), ("minus1", 18, 5), ("minus1", 18, 15), ("carry", 18, 9), ("carry", 18, 15)])
def test_pairs_that_straddle_two_bins(gpu, how, log2_T, lvl):
    """An x-pair whose corners lie in two bins becomes two single-corner items.  Constructed from the level tables: a dense level's cells
    whose x0 corner's index is 8191 mod 8192; a hashed level with gx = -1 (gx + 1 wraps to 0); a hashed level with gx = 8191 mod 8192
    (x near 8, far outside the box, at the finest level).  96 such points among 160 ordinary ones."""
    h, meta, table = _field(log2_T)
    rs = np.random.RandomState(31 + lvl)
    x = np.concatenate([B.straddle_points(meta, lvl, how, 96, rs), rs.uniform(0, 1, (160, 3)).astype(f32)])
    x = x[rs.permutation(x.shape[0])]
    c = rs.normal(size=(x.shape[0], 32)).astype(f32)
    tw = B.twin(meta, x, c)
    assert tw[lvl].straddles >= 32 and B.is_hashed(meta, lvl) == (how != "dense")
    _assert_twin(_backward(h, table, x, c), tw, meta, f"T{log2_T}.straddle.{how}.level{lvl}")


# ------------------------------------------------------------------------------------------------ both branches of fix40_prod
@pytest.mark.parametrize("size", ["tiny", "large"])
def test_small_and_large_cotangents_on_binned_levels(gpu, size):
    """test_scatter_small_contributions_are_exact's inputs on a field whose fine levels are binned.  "tiny": 1e-7 .. 1e-5 of both signs,
    the fp64 fma onto the lattice.  "large": 10 .. 8 000 of both signs: a = wyz g lies on both sides of 2047 within every bin, so
    k_bin_apply mixes the fma with the fp32 split of to_fix40 (restated bit for bit in binned_spec.fix40_split)."""
    h, meta, table = _field(18)
    lo_exp, hi_exp = (-7.0, -5.0) if size == "tiny" else (1.0, 3.9)
    rs = np.random.RandomState(53)
    x = rs.uniform(0, 1, (20000, 3)).astype(f32)
    c = (rs.choice([-1.0, 1.0], size=(20000, 32)) * 10.0 ** rs.uniform(lo_exp, hi_exp, size=(20000, 32))).astype(f32)
    if size == "large":
        for l in B.binned_levels(meta):
            a = np.abs(B.level_geometry(meta, l, x)[3][:, :1] * c[:, 2 * l:2 * l + 1])
            assert 0.01 < float((a >= 2047.0).mean()) < 0.5, "both branches are meant to be busy"
    _assert_twin(_backward(h, table, x, c), B.twin(meta, x, c), meta, f"T18.{size} cotangents")


# ------------------------------------------------------------------------------------------------ the range contract
@pytest.mark.parametrize("log2_T", [18, 20])
def test_binned_levels_drop_out_of_range_cotangents(gpu, log2_T):
    """test_scatter_drops_nan_cotangents on the binned levels and per feature component: every 97th point is bad, in
    rotation NaN, Inf, 1e9, 5e6, and one feature NaN beside a finite one.  The gradient must be that of the same batch with the offending
    components zeroed, bit for bit on every level.  (Before bin_cotangent, naruto_binned.hip tested only the products: a 1e9 or 5e6
    cotangent kept its corners of small weight.)"""
    h, meta, table = _field(log2_T)
    rs = np.random.RandomState(59)
    x = rs.uniform(0, 1, (30000, 3)).astype(f32)
    c_bad, c_zero = B.bad_cotangents((rs.standard_normal((30000, 32)) * 1e-3).astype(f32))
    g_bad, g_zero = _backward(h, table, x, c_bad), _backward(h, table, x, c_zero)
    diff = torch.nonzero(g_bad.view(torch.int32) != g_zero.view(torch.int32)).reshape(-1)
    print(f"T{log2_T}.range: {int(diff.numel())} of {g_bad.numel()} values differ, finite: {bool(torch.isfinite(g_bad).all())}")
    if diff.numel():
        per_level = np.bincount([_where(meta, i)[0] for i in diff[:: max(1, diff.numel() // 2000)].tolist()], minlength=16)
        worst = diff[torch.argmax((g_bad[diff] - g_zero[diff]).abs())]
        lvl, e, f = _where(meta, int(diff[0]))
        wl, we, wf = _where(meta, int(worst))
        raise AssertionError(f"T{log2_T}: {int(diff.numel())} values keep a share of an out-of-range cotangent (sampled per level: {per_level.tolist()}); "
                             f"first: level {lvl} entry {e} feature {f}: {float(g_bad[diff[0]])!r} instead of {float(g_zero[diff[0]])!r}; "
                             f"largest: level {wl} entry {we} feature {wf}: {float(g_bad[worst])!r} instead of {float(g_zero[worst])!r}")
    assert bool(torch.isfinite(g_bad).all())
    _assert_twin(g_bad, B.twin(meta, x, c_bad), meta, f"T{log2_T}.range")


# ------------------------------------------------------------------------------------------------ list lengths
@pytest.mark.parametrize("M", [1, 1023, 1024, 1025, 2049])
def test_list_lengths_around_the_row_boundary(gpu, M):
    """One row of the count matrix per 1 024 points: a single point, one short of a row, exactly one, one more, two rows and a point."""
    h, meta, table = _field(18)
    rs = np.random.RandomState(77)
    x = rs.uniform(0, 1, (2049, 3)).astype(f32)[:M]
    c = rs.normal(size=(2049, 32)).astype(f32)[:M]
    _assert_twin(_backward(h, table, x, c), B.twin(meta, x, c), meta, f"T18.M{M}")


def test_empty_list(gpu):
    """M = 0: a written gradient is all zero, an accumulated one keeps its bits -- through autograd and at the C boundary, where an empty
    batch comes with NULL point pointers."""
    from naruto_amd import _lib, ops
    h, meta, table = _field(18)
    x, c = torch.zeros(0, 3, device=gpu), torch.zeros(0, 32, device=gpu)
    assert ops.hash_encode(h, x, table).shape == (0, 32)
    g = _backward(h, table, x, c)
    assert g.shape == table.shape and int(torch.count_nonzero(g)) == 0
    rs = np.random.RandomState(3)
    x1, c1 = rs.uniform(0, 1, (500, 3)).astype(f32), rs.normal(size=(500, 32)).astype(f32)
    acc = _backward(h, table, x1, c1).clone()
    keep = acc.clone()
    ws = _lib.workspace(_lib.load().naruto_scatter_workspace(h.ptr, 0), gpu)
    _lib.check(_lib.load().naruto_hash_encode_bwd(h.ptr, 0, None, None, None, acc.data_ptr(), ws.data_ptr(), None), "naruto_hash_encode_bwd")
    torch.cuda.synchronize()
    assert torch.equal(acc.view(torch.int32), keep.view(torch.int32)) and int(torch.count_nonzero(acc)) > 0
    table.grad = keep.clone()
    ops.hash_encode(h, x, table).backward(c)
    assert torch.equal(table.grad.view(torch.int32), keep.view(torch.int32))
    table.grad = None


def test_multi_round_rows(gpu):
    """M = 263 169 = 257 x 1 024 + 1: past the 256-row cap of the count matrix, so a row takes two 1 024-point rounds -- 128 full rows, one
    of 1 025 points whose second round holds a single point, and 127 rows without a point.  The twin is formed for the first, a middle
    and the last binned level."""
    h, meta, table = _field(18)
    M = 263169
    rs = np.random.RandomState(11)
    x = rs.uniform(0, 1, (M, 3)).astype(f32)
    c = rs.normal(size=(M, 32)).astype(f32)
    c[rs.uniform(size=M) < 0.1] = 0.0
    got = _backward(h, table, x, c)
    _assert_twin(got, B.twin(meta, x, c, levels=(5, 10, 15)), meta, "T18.M263169")


# ------------------------------------------------------------------------------------------------ 512-point rounds
_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_binned as T
out = {}
for log2_T in (18, 20):
    nz, bits = T._mixed_case(log2_T)[4:6]
    out[f"nz{log2_T}"], out[f"bits{log2_T}"] = nz, bits
np.savez(sys.argv[2], **out)
"""


def test_512_point_rounds_give_the_same_bits(gpu, tmp_path):
    """NARUTO_DEBUG_BIN_ROUND=512 (read once per process: a child interpreter) sends the twin case through k_bin_fill<512> at T = 2^18 and
    T = 2^20: the same nonzero entries with the same bits as the 1 024-point rounds of this process, which equal the twin."""
    assert os.environ.get("NARUTO_DEBUG_BIN_ROUND") is None
    script = tmp_path / "rounds512.py"
    script.write_text(_CHILD)
    out = tmp_path / "rounds512.npz"
    LF.run_child(script, [out], {"NARUTO_DEBUG_BIN_ROUND": "512"}, 600)
    r = dict(np.load(out))
    for log2_T in (18, 20):
        nz, bits = _mixed_case(log2_T)[4:6]
        assert nz.size > 0 and np.array_equal(r[f"nz{log2_T}"], nz), f"T{log2_T}: 512-point rounds touch other entries"
        assert np.array_equal(r[f"bits{log2_T}"], bits), f"T{log2_T}: 512-point rounds change bits"


# ------------------------------------------------------------------------------------------------ T = 2^24
def test_T24_takes_512_point_rounds_over_2048_bins(gpu):
    """create accepts log2_hashmap_size up to 24, and only there does a level have more than 1 024 bins: k_bin_fill<512> by itself, 2 048
    bins per hashed level, four bins per thread in the round's prefix scan.  3 000 points (the twin case's list with dense-level straddles)
    against the sparse twin; the twin's items reach both halves of every level's bin range.
    On MI355X: 227.6 M parameters (0.85 GiB table + as much gradient), 13 871 bins; forward + backward 1.2 ms, peak device memory
    1.92 GiB, the whole test 0.04 s beside the CPU twin -- so the list stays at 3 000 points."""
    h, meta = _handle(24)
    assert B.n_bins(meta, 15) == 2048
    dense = [l for l in B.binned_levels(meta) if not B.is_hashed(meta, l)]
    x, c = B.mixed_points(np.random.RandomState(124))
    rs = np.random.RandomState(6)
    for k, l in enumerate(dense[:3]):
        x[500 + 64 * k:564 + 64 * k] = B.straddle_points(meta, l, "dense", 64, rs)       # (a fifth of the list has no cotangent)
    tw = B.twin(meta, x, c)
    for l, t in tw.items():
        nb = B.n_bins(meta, l)
        assert t.bins.min() < nb // 2 <= t.bins.max(), f"level {l}: the items stay in one half of the bin range"
    assert all(tw[l].straddles >= 32 for l in dense[:3])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    table = torch.zeros(h.n_params, device=gpu, requires_grad=True)
    t0 = time.perf_counter()
    got = _backward(h, table, x, c)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"T24: {h.n_params} parameters, {sum(B.n_bins(meta, l) for l in tw)} bins; forward + backward of 3 000 points {dt * 1e3:.1f} ms, "
          f"peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    _assert_twin(got, tw, meta, "T24.mixed")
    del got, table
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ stale bins
def test_a_bin_gone_empty_is_written_as_zero(gpu):
    """Written (overwrite) gradients of ops.TrainStep at T = 2^18: batch A's rays stay in one octant of the cube, batch B's in the
    opposite one.  After A then B, the binned levels of ts.grads["table"] are those of a fresh TrainStep that only saw B -- a bin that
    took items from A and none from B is written as zeros, not left as it was."""
    from naruto_amd import config as C, ops
    cfg = C.unit_cube_config(1024, 18, perturb=1.0)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.05, 29)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    assert ops.handle_supports_overwrite(m._handle())
    off = m._handle().levels()[3]
    N, S_tot = 6, tr["n_samples_d"] + tr["n_range_d"]
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.0, 0.0])
    rs = np.random.RandomState(8)

    def batch(lo, sign):
        o = rs.uniform(lo, lo + 0.004, (N, 3))
        d = sign * rs.uniform(0.002, 0.01, (N, 3))                       # every sample within 0.01 of its origin (far = 1): a few cells of the
                                                                         # coarsest binned levels, so most of their 32 bins take no item
        return [torch.from_numpy(a.astype(f32)).to(gpu).contiguous() for a in (o, d, rs.uniform(0, 1, (N, 3)))] + \
               [torch.from_numpy(rs.uniform(0.3, 0.8, N).astype(f32)).to(gpu)]

    A, Bb = batch(0.1, 1.0), batch(0.85, -1.0)
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(3)).to(gpu)

    def step():
        return ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                             near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                             perturb=True, loss_weights=w.to(gpu), smooth=None, device_rng=False)

    first = 2 * off[5]
    ts = step()
    ts.run(*A, rand=rand)
    torch.cuda.synchronize()
    g_a = ts.grads["table"].reshape(-1)[first:].clone()
    ts.run(*Bb, rand=rand)
    torch.cuda.synchronize()
    g_ab = ts.grads["table"].reshape(-1)[first:].clone()
    fresh = step()
    fresh.run(*Bb, rand=rand)
    torch.cuda.synchronize()
    g_b = fresh.grads["table"].reshape(-1)[first:].clone()
    assert int(torch.count_nonzero(g_a)) > 0 and int(torch.count_nonzero(g_b)) > 0
    # bins are 8 192 entries = 16 384 floats; every binned level of T = 2^18 is a whole number of them
    assert g_a.numel() % (2 * B.BIN_ENTRIES) == 0
    bins_a = (g_a.reshape(-1, 2 * B.BIN_ENTRIES) != 0).any(1)
    bins_b = (g_b.reshape(-1, 2 * B.BIN_ENTRIES) != 0).any(1)
    stale = int((bins_a & ~bins_b).sum())
    print(f"stale bins: {int(bins_a.sum())} bins with items from A, {int(bins_b.sum())} from B, {stale} from A only, of {bins_a.numel()}")
    assert stale >= 1, "no bin goes from items to none between the two batches"
    assert torch.equal(g_ab.view(torch.int32), g_b.view(torch.int32))

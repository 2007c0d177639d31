"""OneBlob in the fp32 MLP backward (k_query_bwd).  When every point of a 32-point tile is inside the closed form's range the kernel writes the tile's
OneBlob stage columns as zeros plus three bins per coordinate stored by address (each of a point's two lanes keeps the bins of its parity, the others
go to a dump word) and reads an active K pair's operand back from the stage; otherwise it builds the dense form in registers as before.  Against
oracle autograd with the harness and the tolerance of test_gpu_bwd_tiles (H.office_cfg(12), grad_close: 1e-4 of the tensor's largest gradient
magnitude + 1e-3 relative) at 1, 33 and 65 points through query_color_sdf, on point sets built for what the placement can get wrong: every centre
bin per coordinate with both wraps, coordinates on the bin edges, a tile sent to the dense form by one point, tiles with all pairs / one bin active.

The bitwise test needs no second build: K pairs that no point of a tile touches are skipped, so adding a point with an all-zero cotangent that
switches further pairs on makes the kernel process, for the other points, pairs of exact zeros that it skipped before -- the same sums."""
import numpy as np
import pytest
import torch

from oracle import spec_torch as S

import helpers as H
from test_gpu_bwd_tiles import WEIGHTS, _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def field(gpu):
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 21)
    return ora, H.make_hip_from_oracle(cfg, ora, gpu)


def _leaves(ora, m):
    return ([ora.sdf_w0, ora.sdf_w1, ora.col_w0, ora.col_w1, ora.uncert_grid, ora.table],
            [m.decoder.sdf_net.model[0].weight, m.decoder.sdf_net.model[2].weight, m.decoder.color_net.model[0].weight,
             m.decoder.color_net.model[2].weight, m.uncert_grid, m.embed_fn.params])


def _hip_grads(field, gpu, x, c_raw):
    ora, m = field
    for t in _leaves(ora, m)[1]:
        t.grad = None
    raw = m.query_color_sdf(torch.from_numpy(x).to(gpu))
    (raw * torch.from_numpy(c_raw).to(gpu)).sum().backward()
    torch.cuda.synchronize()
    return {k: (None if v is None else v.detach().clone()) for k, v in H.hip_grads(m).items()}


def _ora_grads(field, x, c_raw):
    ora, m = field
    for t in _leaves(ora, m)[0]:
        t.grad = None
    (ora.query_color_sdf(torch.from_numpy(x)) * torch.from_numpy(c_raw)).sum().backward()
    return {k: (None if v is None else v.detach().clone()) for k, v in H.ora_grads(ora).items()}


def _check(field, gpu, x, what):
    x = np.ascontiguousarray(x, dtype=np.float32)
    c_raw = np.random.RandomState(3).normal(size=(x.shape[0], 5)).astype(np.float32)
    _compare(_hip_grads(field, gpu, x, c_raw), _ora_grads(field, x, c_raw), what)


def _centre_bins(x):
    """b0 of the closed form: floor(16 x) mod 16, per point and coordinate."""
    return np.floor(x.astype(np.float64) * 16.0).astype(np.int64) % 16


def _bin_walk(n, start):
    """Point i's coordinate d sits in bin (i + start + 5 d) mod 16, away from the edges."""
    rs = np.random.RandomState(11)
    i = np.arange(n)[:, None]
    b = (i + start + 5 * np.arange(3)[None, :]) % 16
    return ((b + rs.uniform(0.05, 0.95, size=(n, 3))) / 16.0).astype(np.float32), b


# one point: the six starts put b0 = 0 and b0 = 15 (the wraps: lower neighbour bin 15, upper neighbour bin 0) on each coordinate in turn;
# 33 and 65 points walk every coordinate through all sixteen centre bins (both parities of the three bins)
@pytest.mark.parametrize("n_pts,start", [(1, 0), (1, 15), (1, 11), (1, 10), (1, 6), (1, 5), (33, 0), (65, 0)])
def test_every_centre_bin(field, gpu, n_pts, start):
    x, b = _bin_walk(n_pts, start)
    assert np.array_equal(_centre_bins(x), b)
    if n_pts == 1:
        assert 0 in b or 15 in b
    else:
        for d in range(3):
            assert set(b[:32, d]) == set(range(16)), d            # ... within the first tile already
    _check(field, gpu, x, f"centre bins, {n_pts} points from {start}")


@pytest.mark.parametrize("n_pts,start", [(1, 0), (1, 16), (33, 0), (65, 0)])
def test_bin_edges(field, gpu, n_pts, start):
    """Every coordinate exactly on a bin edge k/16, k = 0..16 (0 and 1 among them): the closed form's fraction is 0, its upper bin an exact zero."""
    i = np.arange(n_pts)[:, None]
    k = (i + start + 6 * np.arange(3)[None, :]) % 17
    x = (k / 16.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 16.0, k)
    if n_pts > 1:
        for d in range(3):
            assert set(k[:, d]) == set(range(17)), d
    _check(field, gpu, x, f"bin edges, {n_pts} points from {start}")


@pytest.mark.parametrize("n_pts,far", [(1, -0.95), (1, 1.95), (33, -0.95), (65, -0.95)])
def test_dense_tile(field, gpu, n_pts, far):
    """One point of a tile outside the closed form's range (-0.93, 1.93) sends the whole tile to the dense form: the first point at -0.95 and,
    with more than one tile, the last point (alone in its tile) at 1.95; at 65 points the tile between them keeps the closed form."""
    x = np.random.RandomState(12).uniform(0.05, 0.95, size=(n_pts, 3)).astype(np.float32)
    x[0, 0] = far
    if n_pts > 1:
        x[-1, 2] = 1.95
    _check(field, gpu, x, f"dense tile, {n_pts} points")


def _all_pairs_tile(rs, n):
    """Up to 32 points whose centre bins run through all sixteen bins of every coordinate: all eight pairs of each active."""
    k = np.arange(n)[:, None]
    b = (k + 3 * np.arange(3)[None, :]) % 16
    return (b + rs.uniform(0.05, 0.95, size=(n, 3))) / 16.0


def _one_bin_tile(rs, n):
    """Up to 32 points that share one centre bin per coordinate (3, 8 and the wrapping 15): two pairs of each active, six skipped."""
    b = np.array([3, 8, 15])[None, :]
    return (b + rs.uniform(0.05, 0.95, size=(n, 3))) / 16.0


@pytest.mark.parametrize("n_pts,first", [(1, "all"), (33, "all"), (33, "one"), (65, "all"), (65, "one")])
def test_all_pairs_and_one_bin_tiles(field, gpu, n_pts, first):
    rs = np.random.RandomState(13)
    kinds = [_all_pairs_tile, _one_bin_tile] if first == "all" else [_one_bin_tile, _all_pairs_tile]
    tiles = [kinds[t % 2](rs, min(32, n_pts - 32 * t)) for t in range((n_pts + 31) // 32)]
    x = np.concatenate(tiles).astype(np.float32)
    if n_pts > 1:
        full = x[:32] if first == "all" else x[32:64] if n_pts >= 64 else None
        if full is not None:
            assert all(set(_centre_bins(full)[:, d]) == set(range(16)) for d in range(3))
        one = x[:32] if first == "one" else x[32:64]
        assert all(len(set(_centre_bins(one)[:, d])) == 1 for d in range(3))
    _check(field, gpu, x, f"{first} first, {n_pts} points")


def _active_pairs(x):
    """[3][8] booleans from the oracle's encoding: pair Q of coordinate d has a non-zero bin at some point."""
    e = S.oneblob_encode(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), 16).reshape(-1, 3, 8, 2)
    return (e != 0).any(dim=3).any(dim=0).numpy()


# One point inside the closed form's range touches three adjacent bins, at most two pairs per coordinate, and a point outside it moves the tile to
# the dense form, whose non-zero bins are not the closed form's bits: so "one more point, further pairs on" is a far-away point that switches on
# two pairs per coordinate which the others left off, and "EVERY pair on" takes four such points (centre bins 1, 5, 9, 13: pairs {0,1} .. {6,7}).
@pytest.mark.parametrize("n_base,extra_bins", [(31, [[12, 13, 14]]), (28, [[1, 1, 1], [5, 5, 5], [9, 9, 9], [13, 13, 13]])])
def test_skipped_pairs_are_pairs_of_zeros_bitwise(field, gpu, n_base, extra_bins):
    rs = np.random.RandomState(14)
    # the points with cotangents: centre bins 2 .. 5 of every coordinate (bins 1 .. 6: pairs 0 .. 3)
    base = ((rs.randint(2, 6, size=(n_base, 3)) + rs.uniform(0.05, 0.95, size=(n_base, 3))) / 16.0).astype(np.float32)
    extra = ((np.array(extra_bins) + 0.5) / 16.0).astype(np.float32)
    n_extra = len(extra_bins)
    c_base = rs.normal(size=(n_base, 5)).astype(np.float32)
    c_zero = np.zeros((n_extra, 5), dtype=np.float32)
    if n_extra > 1:
        # several added points: the first run gets as many points WITHOUT a cotangent among the others' bins, so that both lists are 32 long (the
        # table scatter sums consecutive points of a cell in float before its fixed point, and where it cuts the list depends on the list's
        # length: four entries more moved 8 table entries by an ulp, whatever the MLP backward did with them)
        near = ((np.full((n_extra, 3), 3) + 0.5) / 16.0).astype(np.float32)
        base, c_base = np.concatenate([base, near]), np.concatenate([c_base, c_zero])
        both = np.concatenate([base[:n_base], extra])
    else:
        both = np.concatenate([base, extra])
    assert both.shape[0] == 32                                       # one tile either way
    # on the CPU first: the base points leave pairs of every coordinate off, the added points switch some of those on
    on_base, on_both = _active_pairs(base), _active_pairs(both)
    assert all((~on_base[d]).any() for d in range(3)), on_base
    assert all((on_both[d] & ~on_base[d]).any() for d in range(3)), (on_base, on_both)
    if n_extra == 4:
        assert on_both.all(), on_both
    c_both = np.concatenate([c_base[:n_base], c_zero])
    a = _hip_grads(field, gpu, base, c_base)
    b = _hip_grads(field, gpu, both, c_both)
    for k in WEIGHTS + ("table",):
        assert float(a[k].abs().max()) > 0.0, k
        assert torch.equal(a[k], b[k]), f"gradient {k}: {int((a[k] != b[k]).sum())} entries differ when pairs of exact zeros are processed instead of skipped"

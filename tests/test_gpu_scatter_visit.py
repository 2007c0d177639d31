"""The hashed units' LIST visit of k_hash_scatter_lds (hash_corner_addr8 + fix_add_corners8: the training layout, four points per lane, the
LDS address formed from the corner's byte offset) against the GENERIC visit of the same library (hash_corner_index + fix_add_corners, one point
per thread) on the same points and cotangents: the same table gradient, bit for bit, per level.

Both routes add the same fixed-point contributions into the same entries -- sums of integers, whatever the order -- and run the same plan over the
same count, hence the same split bounds and the same float sum over the splits in k_scatter_reduce: nothing here is a tolerance.

Routes: naruto_debug_scatter_list (x_soa [3][cap], d_feat [16][cap][2], the count on the device) and naruto_hash_encode_bwd (x [M,3],
d_feat [M,32]).  Fields: the office_0 box with 2^15, 2^16, 2^17 entries per hashed level (2, 4, 8 chunks of 16 384 entries; 2^17 is the
largest LDS-tiled size) and 2^14 (one chunk: every in-chunk test is true)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

f32 = np.float32
CHUNK = 16384                                         # kChunk: entries per LDS image
LENGTHS = (1, 3, 4, 4095, 4096, 4097, 2 * 4096 + 5)   # prefetch clamp, last partial vector, more than one loop trip (256 lanes x 4 points each)
N_POOL = LENGTHS[-1]
P1LOW, P2LOW = 2654435761 & 0xFFFFFF, 805459861 & 0xFFFFFF


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _field(log2_T):
    from naruto_amd.field import NarutoFieldHIP
    cfg = H.office_cfg(log2_T)
    m = NarutoFieldHIP(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32))
    h = m._make_handle((8, 8, 8))
    scale, res, size, off = h.levels()
    hashed = [l for l in range(h.n_levels) if size[l] == (1 << log2_T) and (res[l] + 1) ** 3 > size[l]]
    assert hashed, f"T = 2^{log2_T}: no hashed level (sizes {size})"
    return h, np.asarray(scale, f32), np.asarray(size), np.asarray(off), hashed


def _points(scale_fine, rs):
    """Normalised positions [N_POOL, 3]: the box is [0, 1]^3; p = scale x + 1/2, so a coordinate in (-1.4, -0.6) / scale has cell index -1 on the
    finest level, one in 1 + (0.6, 2.4) / scale a cell index at and past the last."""
    n = N_POOL
    x = rs.uniform(0.0, 1.0, (n, 3))
    cell = 1.0 / float(scale_fine)

    def face(rows, k):
        u = rs.uniform(0.0, 1.0, len(rows))
        x[rows, k // 2] = -(0.6 + 0.8 * u) * cell if k % 2 == 0 else 1.0 + (0.6 + 1.8 * u) * cell

    # [0, 1024): every second point just outside one of the six faces, in turn -- lanes at cell index -1 / res beside in-box lanes in every wave
    odd = np.arange(1, 1024, 2)
    for k in range(6):
        face(odd[(odd // 2) % 6 == k], k)
    # [1024, 1792) and [1792, 2560): 768 consecutive points just outside the low / the high x face -- whole waves of them wherever a split starts
    face(np.arange(1024, 1792), 0)
    face(np.arange(1792, 2560), 1)
    # [2560, 2816): far outside, both sides, every axis
    far = np.arange(2560, 2816)
    x[far] = np.where(rs.uniform(size=(256, 3)) < 0.5, rs.uniform(-6.0, -2.0, (256, 3)), rs.uniform(2.0, 7.0, (256, 3)))
    return x.astype(f32)


def _cotangents(rs):
    """[N_POOL, 16, 2]: mostly order 1; zero, 1e-12, around 2047 (the magic-number conversion up to it, the fp32 split beyond), 4e6 (near the
    fixed point's range), NaN and Inf (add nothing) mixed in per (point, level, feature) -- so one feature is often zero and the other not."""
    kinds = np.array([0.0, 1e-12, np.nextafter(f32(2047.0), f32(0.0)), 2047.0, np.nextafter(f32(2047.0), f32(4096.0)), 4.0e6, np.nan, np.inf], dtype=f32)
    p = np.array([0.12, 0.04, 0.03, 0.02, 0.03, 0.02, 0.02, 0.02])
    pick = rs.choice(len(kinds) + 1, size=(N_POOL, 16, 2), p=np.concatenate([p, [1.0 - p.sum()]]))
    c = np.where(pick == len(kinds), rs.uniform(0.25, 1.75, pick.shape), kinds[np.minimum(pick, len(kinds) - 1)]).astype(f32)
    c *= np.where(rs.uniform(size=pick.shape) < 0.5, f32(-1.0), f32(1.0))
    c[0, :, :] = 0.75                                  # the list of one point is a plain order-1 visit
    c[2, :, 0] = 0.0                                   # feature 0 zero, feature 1 not, on every level
    c[2, :, 1] = -1.25
    return c


@functools.lru_cache(maxsize=None)
def _inputs(log2_T):
    h, scale, size, off, hashed = _field(log2_T)
    rs = np.random.RandomState(700 + log2_T)
    return _points(scale[-1], rs), _cotangents(rs)


def _generic(h, x, c, dev):
    from naruto_amd import _lib
    lib = _lib.load()
    n = x.shape[0]
    xt, ct = torch.from_numpy(x).to(dev).contiguous(), torch.from_numpy(c.reshape(n, 32)).to(dev).contiguous()
    g = torch.zeros(h.n_params, device=dev)
    ws = _lib.workspace(lib.naruto_scatter_workspace(h.ptr, n), dev)
    _lib.check(lib.naruto_hash_encode_bwd(h.ptr, n, xt.data_ptr(), ct.data_ptr(), None, g.data_ptr(), ws.data_ptr(), _stream()), "naruto_hash_encode_bwd")
    torch.cuda.synchronize()
    return g


def _list(h, x, c, dev):
    from naruto_amd import _lib
    lib = _lib.load()
    n = x.shape[0]
    cap = (n + 3) & ~3
    # what lies between the count and the capacity is stale in training: a position and a cotangent that would show if they were visited
    xs = np.full((3, cap), 0.5, f32)
    xs[:, :n] = x.T
    cs = np.full((16, cap, 2), 1.0, f32)
    cs[:, :n, :] = c.transpose(1, 0, 2)
    xt, ct = torch.from_numpy(xs).to(dev).contiguous(), torch.from_numpy(cs).to(dev).contiguous()
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
    g = torch.zeros(h.n_params, device=dev)
    ws = _lib.workspace(lib.naruto_scatter_workspace(h.ptr, cap), dev)
    _lib.check(lib.naruto_debug_scatter_list(h.ptr, cap, n_dev.data_ptr(), xt.data_ptr(), ct.data_ptr(), g.data_ptr(), ws.data_ptr(), _stream()),
               "naruto_debug_scatter_list")
    torch.cuda.synchronize()
    return g


def _corner_chunks(x, scale, size):
    """Chunk number of the eight hashed corners of every point on one level (hash_corner_index's arithmetic): [n, 8]."""
    g = np.floor(f32(scale) * x + f32(0.5)).astype(np.int64)
    out = np.empty((x.shape[0], 8), np.int64)
    for c in range(8):
        cx, cy, cz = g[:, 0] + (c & 1), g[:, 1] + ((c >> 1) & 1), g[:, 2] + (c >> 2)
        out[:, c] = ((cx ^ (cy * P1LOW) ^ (cz * P2LOW)) & (int(size) - 1)) >> 14
    return out


@pytest.mark.parametrize("log2_T", [15, 16, 17, 14])
def test_list_visit_equals_generic_visit(gpu, log2_T):
    h, scale, size, off, hashed = _field(log2_T)
    x, c = _inputs(log2_T)
    n_chunks = (1 << log2_T) // CHUNK
    # the list as given reaches cell index -1 and a cell index past the grid on the finest level, in whole waves and beside in-box lanes
    gfine = np.floor(scale[-1] * x + f32(0.5)).astype(np.int64)
    assert (gfine[1024:1792, 0] == -1).all() and (gfine[1792:2560, 0] >= int(scale[-1])).all()
    assert {-1}.issubset(set(gfine[1:1024:2].min(axis=1).tolist())) and (gfine[0:1024:2].min() >= 0)
    for n in LENGTHS:
        want, got = _generic(h, x[:n], c[:n], gpu), _list(h, x[:n], c[:n], gpu)
        assert torch.isfinite(want).all(), f"T = 2^{log2_T}, {n} points: the generic route's gradient is not finite"
        for l in range(h.n_levels):
            a, b = got[2 * int(off[l]):2 * int(off[l + 1])], want[2 * int(off[l]):2 * int(off[l + 1])]
            if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
                k = int(torch.nonzero(a.view(torch.int32) != b.view(torch.int32))[0])
                raise AssertionError(f"T = 2^{log2_T}, {n} points, level {l} ({'hashed' if l in hashed else 'dense'}): entry {k // 2} (chunk {k // 2 // CHUNK}) feature "
                                     f"{k % 2}: list route {float(a[k])!r}, generic route {float(b[k])!r}; {int((a != b).sum())} values differ")
        nz = {l: int(torch.count_nonzero(want[2 * int(off[l]):2 * int(off[l + 1])])) for l in hashed}
        print(f"T = 2^{log2_T}, {n} points: {h.n_levels} levels equal bit for bit; nonzero values on the hashed levels {nz}")
        assert all(v > 0 for v in nz.values())
        if n == LENGTHS[-1]:
            # no chunk's path goes unvisited: every chunk of every hashed level takes a share of the corners of the points that add something,
            # and the list route's gradient is nonzero in every chunk
            for l in hashed:
                for f in range(2):
                    adds = np.isfinite(c[:, l, f]) & (c[:, l, f] != 0.0) & (np.abs(c[:, l, f]) < 4194304.0)
                    frac = np.bincount(_corner_chunks(x[adds], scale[l], size[l]).reshape(-1), minlength=n_chunks) / (8.0 * adds.sum())
                    assert frac.shape == (n_chunks,) and (frac > 0).all(), (log2_T, l, f, frac)
                lvl = got[2 * int(off[l]):2 * int(off[l + 1])].reshape(n_chunks, CHUNK, 2)
                assert (torch.count_nonzero(lvl, dim=(1, 2)) > 0).all(), (log2_T, l)
            print(f"T = 2^{log2_T}: share of the hashed corners per chunk on level {hashed[-1]}: {np.round(frac, 3).tolist()}")

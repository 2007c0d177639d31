"""Point gradients (naruto_query_bwd_points) without a GPU: the semantics the GPU tests compare against (the oracle's autograd and
the fp64 reference that takes the kernel's hash cell, tests/helpers.py), the entry point's argument validation, and the sub-modules
that refuse a point gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
from oracle import spec_torch as S


def test_oracle_point_gradient_matches_central_differences():
    """torch autograd of the oracle's query_color_sdf / query_sdf w.r.t. x (what the HIP point gradient is compared with) equals fp64
    central differences of the same forward, on points away from the piecewise kinks (hash and uncertainty cell faces, ReLU zeros).
    Points outside [0,1]^3 are included: the uncertainty grid's zero padding and OneBlob's periodic images apply there."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 5).double()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(400, 3, generator=g, dtype=torch.float64) * 1.2 - 0.1
    x = x[H._away_from_kinks(ora, x, 1e-3)][:96]
    assert x.shape[0] >= 64
    w_raw = torch.randn(x.shape[0], 5, generator=g, dtype=torch.float64)
    w_geo = torch.randn(x.shape[0], 15, generator=g, dtype=torch.float64)

    def f_color(p):                     # per-point values: the points are independent, so one perturbation per axis serves all
        return (ora.query_color_sdf(p) * w_raw).sum(1)

    def f_sdf(p):
        su, geo = ora.query_sdf(p, return_geo=True, return_uncert=True)
        return (su * w_raw[:, 3:5]).sum(1) + (geo * w_geo).sum(1)

    for fn in (f_color, f_sdf):
        xa = x.clone().requires_grad_(True)
        fn(xa).sum().backward()
        h = 1e-7
        num = torch.zeros_like(x)
        with torch.no_grad():
            for d in range(3):
                e = torch.zeros_like(x)
                e[:, d] = h
                num[:, d] = (fn(x + e) - fn(x - e)) / (2 * h)
        scale = float(num.abs().max())
        H.assert_close(xa.grad, num, 1e-6 * scale, f"oracle autograd vs central differences ({fn.__name__})", rel=1e-5)


def test_query_bwd_points_validates_arguments(built_lib):
    """Every malformed call returns NARUTO_ERR_INVALID with a message before anything is launched (no pointer below is ever
    dereferenced: each call is rejected by the argument checks)."""
    from naruto_amd import _lib, ops
    lib = built_lib
    h = ops.FieldHandle(log2_hashmap_size=12, per_level_scale=1.4, uncert_dims=(4, 5, 6), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1),
                        trunc=0.1, sc_factor=1.0)
    fake = 0x10000                                           # a non-NULL address for arguments the checks only test for presence
    ps = _lib.NarutoParams(*([fake] * 6))
    px = _lib.NarutoPoints(fake, None, None, None, 0)
    pr = _lib.NarutoPoints(None, fake, fake, fake, 43)
    M = 2048 * 43
    ws = fake
    acc = _lib.BWD_POINTS_ACCUMULATE

    def call(pts, m=M, d_raw=fake, active=None, n_active=None, d_x=None, d_o=None, d_d=None, flags=0, w=ws, params=ps):
        return lib.naruto_query_bwd_points(h.ptr, C.byref(params), m, C.byref(pts), d_raw, None, active, n_active, d_x, d_o, d_d, flags,
                                           w, None)

    cases = {
        "NULL d_raw": dict(pts=px, d_raw=None, d_x=fake),
        "d_rays_o with x points": dict(pts=px, d_x=fake, d_o=fake),
        "d_rays_d with x points": dict(pts=px, d_x=fake, d_d=fake),
        "no output (x points)": dict(pts=px),
        "no output (ray points)": dict(pts=pr),
        "d_x with ray points": dict(pts=pr, d_x=fake, d_o=fake),
        "M out of range": dict(pts=px, m=(1 << 29) + 1, d_x=fake),
        "M not whole rays": dict(pts=pr, m=M + 1, d_o=fake),
        "S out of range": dict(pts=_lib.NarutoPoints(None, fake, fake, fake, 1025), m=1025 * 4, d_o=fake),
        "no samples": dict(pts=_lib.NarutoPoints(None, fake, fake, fake, 0), d_o=fake),
        "active_idx without n_active": dict(pts=px, d_x=fake, active=fake),
        "n_active without active_idx": dict(pts=pr, d_o=fake, n_active=fake),
        "unknown flags": dict(pts=px, d_x=fake, flags=acc | 8),
        "ray points without workspace": dict(pts=pr, d_o=fake, w=None),
        "NULL parameter": dict(pts=px, d_x=fake, params=_lib.NarutoParams(fake, None, fake, fake, fake, fake)),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == -22, f"{what}: returned {rc}"
        assert lib.naruto_last_error(), what
    assert lib.naruto_query_bwd_points(None, C.byref(ps), M, C.byref(px), fake, None, None, None, fake, None, None, 0, None, None) == -22
    assert lib.naruto_query_bwd_points_workspace(h.ptr, M) >= 12 * M


def test_cell_reference_equals_the_oracle_away_from_faces():
    """hash_encode_cells / cell_field equal S.hash_encode / the oracle's field in fp64 (values and autograd) on points away from every
    kink, for a dense and a hashed table, inside and outside [0,1]^3."""
    for hs in (12, 18):
        cfg = H.office_cfg(hs)
        ora = H.make_oracle(cfg, 0.25, 9).double()
        x = torch.from_numpy(np.random.RandomState(hs).uniform(-0.2, 1.2, (600, 3)).astype(np.float32)).double()
        x = x[H._away_from_kinks(ora, x, 1e-4)]
        assert x.shape[0] >= 100
        H.assert_close(H.hash_encode_cells(x, ora.table, ora.meta), S.hash_encode(x, ora.table, ora.meta), 1e-15, f"T=2^{hs}: features")
        w = torch.randn(x.shape[0], 5, generator=torch.Generator().manual_seed(hs), dtype=torch.float64)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        raw, geo, _, _, amb, _, _ = H.cell_field(ora, xa)
        assert not amb.any()
        want = ora.query_color_sdf(xb)
        H.assert_close(raw, want, 1e-13, f"T=2^{hs}: raw")
        (raw * w).sum().backward()
        (want * w).sum().backward()
        H.assert_close(xa.grad, xb.grad, 1e-12, f"T=2^{hs}: d x", rel=1e-12)
        H.assert_close(H.ref_point_grad(ora, x, w), xb.grad, 1e-12, f"T=2^{hs}: ref_point_grad", rel=1e-12)


def test_cell_reference_is_one_sided_at_faces():
    """On a hash face (fp32 points whose fmaf(scale, x, 0.5f) is an integer, and their 1-ulp neighbours) the reference's autograd
    equals the derivative of the interpolant of the cell the kernel picks (floorf of the fp32 pos).  That derivative is formed
    from the plain fp64 oracle S.hash_encode at points strictly inside the cell: along the face's axis the interpolant is linear,
    so a difference across the cell is exact; along the other axes the derivative is linear in the face axis' coordinate, so
    central differences at two positions inside the cell are extrapolated to the point.  The fp64 oracle's own floor picks the
    other cell at some of these points: asserted, so that the test is not vacuous."""
    cfg = H.office_cfg(14)
    ora = H.make_oracle(cfg, 0.25, 13).double()
    meta = ora.meta
    rs = np.random.RandomState(2)
    differs = 0
    for lvl in (0, 5, 11, 15):
        scale = float(np.float32(meta.scale[lvl]))
        k = rs.randint(1, int(meta.resolution[lvl]), 40)
        face = ((k - 0.5) / scale).astype(np.float32)
        xs = np.concatenate([face, np.nextafter(face, np.float32(-np.inf)), np.nextafter(face, np.float32(np.inf))])
        x = rs.uniform(0.05, 0.95, (xs.shape[0], 3)).astype(np.float32)
        axis = lvl % 3
        x[:, axis] = xs
        x = torch.from_numpy(x).double()
        w = torch.randn(x.shape[0], 2, generator=torch.Generator().manual_seed(lvl), dtype=torch.float64)

        def plain(p):                          # the fp64 oracle's level-lvl features, contracted with w
            return (S.hash_encode(p, ora.table, meta)[:, 2 * lvl:2 * lvl + 2] * w).sum(1)

        xa = x.clone().requires_grad_(True)
        (H.hash_encode_cells(xa, ora.table, meta, levels=(lvl,))[:, 2 * lvl:2 * lvl + 2] * w).sum().backward()
        pos64 = x[:, axis] * scale + 0.5
        cell = torch.floor(pos64.float().double())
        differs += int((torch.floor(pos64) != cell).sum())

        def at(t):                             # the points moved along the face axis to pos = cell + t
            q = x.clone()
            q[:, axis] = (cell + t - 0.5) / scale
            return q

        want = torch.zeros_like(x)
        with torch.no_grad():
            want[:, axis] = (plain(at(0.75)) - plain(at(0.25))) / (0.5 / scale)
            for d in range(3):
                if d == axis:
                    continue
                hd = 1e-6 / scale
                e = torch.zeros_like(x)
                e[:, d] = hd
                der = [(plain(at(t) + e) - plain(at(t) - e)) / (2 * hd) for t in (0.25, 0.75)]
                t = pos64 - cell
                want[:, d] = der[0] + (der[1] - der[0]) * (t - 0.25) / 0.5
        scl = float(want.abs().max())
        H.assert_close(xa.grad, want, 1e-6 * scl, f"level {lvl}: one-sided derivative into the kernel's cell", rel=1e-6)
    assert differs > 0, "no point where the fp64 floor and the kernel's fp32 floor disagree: the faces were not hit"


def test_kink_detector_flags_relu_zeros_and_ambiguous_voxels():
    """point_kinks flags a point placed on a ReLU zero of the first layer and leaves generic points alone; its hash-face flag finds
    points built on a face."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 4).double()
    x = torch.from_numpy(np.random.RandomState(3).uniform(0.1, 0.9, (64, 3)).astype(np.float32)).double()
    k = H.point_kinks(ora, x)
    assert int(k["kink"].sum()) <= 2
    # move unit 0's pre-activation of point 0 to (nearly) zero by bisection along x
    with torch.no_grad():
        def h0(p):
            return H.cell_field(ora, p)[2][:, 0]
        a, b = x[:1].clone(), x[:1].clone()
        b[0, 0] += 0.05
        while float(h0(a)) * float(h0(b)) > 0 and float(b[0, 0]) < 1.5:
            b[0, 0] += 0.05
        assert float(h0(a)) * float(h0(b)) <= 0, "no sign change of unit 0 found"
        for _ in range(60):
            m = (a + b) / 2
            if float(h0(a)) * float(h0(m)) <= 0:
                b = m
            else:
                a = m
        p = a.float().double()
    assert bool(H.point_kinks(ora, p)["relu"][0])
    scale = np.float32(ora.meta.scale[7])
    xf = x.clone()
    xf[:8, 1] = torch.from_numpy(((np.arange(3, 11) - 0.5) / np.float64(scale)).astype(np.float32)).double()
    assert bool(H.point_kinks(ora, xf)["hash_faces"][:8].all())


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    """helpers.fma32 (how the tests form ray points: fmaf(d, z, o)) against exact rational arithmetic rounded to the nearest fp32
    (ties to even), including |o| far larger and far smaller than |d z|, where an fp64 sum is itself rounded."""
    from fractions import Fraction
    rs = np.random.RandomState(11)
    n = 400
    a = (rs.normal(size=n) * 10.0 ** rs.uniform(-3, 3, n)).astype(np.float32)
    b = (rs.uniform(0.02, 3.0, n) * 10.0 ** rs.uniform(-4, 2, n)).astype(np.float32)
    c = (rs.normal(size=n) * 10.0 ** rs.uniform(-6, 6, n)).astype(np.float32)
    # ties of fp32 on purpose: c + a b exactly halfway between two fp32 numbers (a b = half an ulp of c)
    c[:40] = np.float32(1.0) + np.arange(40, dtype=np.float32) * np.float32(2.0 ** -20)
    a[:40], b[:40] = np.float32(2.0 ** -24), np.float32(1.0)
    got = H.fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c)).numpy()

    def rn32(q):
        f = np.float32(float(q))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - q), int(np.array(v).view(np.int32)) & 1))
        return best

    want = np.array([rn32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.flatnonzero(got != want)[:10]


def test_embed_fn_refuses_a_point_gradient(built_lib):
    """ops.hash_encode (embed_fn, query_sdf(embed=True), calc_embedding) raises NotImplementedError when grad is enabled and x
    requires grad -- before anything is launched (x here is on the CPU: a launch would fail with another error).  With x not
    requiring grad or under no_grad it passes the check (and reaches the device check)."""
    from naruto_amd import ops
    h = ops.FieldHandle(log2_hashmap_size=12, per_level_scale=1.4, uncert_dims=(4, 5, 6), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1),
                        trunc=0.1, sc_factor=1.0)
    table = torch.zeros(64, requires_grad=True)
    x = torch.rand(8, 3, requires_grad=True)
    with pytest.raises(NotImplementedError, match="table only"):
        ops.hash_encode(h, x, table)
    for xx, ctx in ((x.detach(), torch.enable_grad()), (x, torch.no_grad())):
        with ctx, pytest.raises(RuntimeError, match="expected a tensor on the GPU"):
            ops.hash_encode(h, xx, table)

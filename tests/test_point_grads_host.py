"""Point gradients (naruto_query_bwd_points) without a GPU: the semantics the GPU tests compare against, and the entry point's
argument validation."""
import ctypes as C

import torch

import helpers as H
from oracle import spec_torch as S


def _away_from_kinks(ora, x, margin):
    """Points whose every hash level, uncertainty voxel and ReLU unit is at least ``margin`` away from a kink (fp64)."""
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    for lvl in range(ora.meta.n_levels):
        f = torch.frac(x * float(ora.meta.scale[lvl]) + 0.5)
        ok &= ((f > margin) & (f < 1 - margin)).all(1)
    D, Hh, W = ora.uncert_grid.shape
    f = torch.frac(x * torch.tensor([W, Hh, D], dtype=x.dtype) - 0.5)
    ok &= ((f > margin) & (f < 1 - margin)).all(1)
    with torch.no_grad():
        feats, pos = S.hash_encode(x, ora.table, ora.meta), S.oneblob_encode(x, 16)
        h = torch.cat([feats, pos], -1) @ ora.sdf_w0.T
        c = torch.cat([pos, (torch.relu(h) @ ora.sdf_w1.T)[:, 1:]], -1) @ ora.col_w0.T
    ok &= (h.abs() > margin).all(1) & (c.abs() > margin).all(1)
    return ok


def test_oracle_point_gradient_matches_central_differences():
    """torch autograd of the oracle's query_color_sdf / query_sdf w.r.t. x (what the HIP point gradient is compared with) equals fp64
    central differences of the same forward, on points away from the piecewise kinks (hash and uncertainty cell faces, ReLU zeros).
    Points outside [0,1]^3 are included: the uncertainty grid's zero padding and OneBlob's periodic images apply there."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 5).double()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(400, 3, generator=g, dtype=torch.float64) * 1.2 - 0.1
    x = x[_away_from_kinks(ora, x, 1e-3)][:96]
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

"""naruto_query_bwd_points at the places a rewrite of k_query_bwd_points / k_ray_point_reduce goes wrong: each term on its own (one
hash level's Jacobian, OneBlob, the uncertainty sample, each MLP branch and the wave-uniform colour skip), table sizes 2^10 .. 2^22 and
drawn boxes, partial blocks and guard rows around every output, the active list and accumulation, and the Python routes that return
point or ray gradients.  The reference is autograd of the oracle's field in fp64 with the kernel's hash cell (helpers.cell_field);
every point that is not a kink is compared element by element (helpers.check_point_grads)."""
import numpy as np
import pytest
import torch

import helpers as H
from naruto_amd import config as C
from naruto_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -7.25          # guard rows around every output
G = 5                     # guard rows before and after


def _cfg(kind):
    if kind == "office12":
        return H.office_cfg(12)
    if kind == "office16":
        return H.office_cfg(16)
    if kind == "t20":
        return H.office_cfg(20)
    if kind == "unit1024":
        return C.unit_cube_config(1024, 16)
    if kind == "t22":
        return C.unit_cube_config(1024, 22)
    if kind == "mp3d":
        return C.mp3d_large_config()
    if kind.startswith("drawn"):
        return H.drawn_field_config(int(kind[5:]))[0]
    raise KeyError(kind)


def _setup(kind, seed):
    cfg = _cfg(kind)
    ora = H.make_oracle(cfg, 0.25, seed)
    return cfg, ora, H.make_hip_from_oracle(cfg, ora, torch.device("cuda:0"))


def _set(ora, m, **kw):
    """The same parameter values in the oracle and the HIP module."""
    dst = {"table": m.embed_fn.params, "uncert_grid": m.uncert_grid, "sdf_w0": m.decoder.sdf_net.model[0].weight,
           "sdf_w1": m.decoder.sdf_net.model[2].weight, "col_w0": m.decoder.color_net.model[0].weight,
           "col_w1": m.decoder.color_net.model[2].weight}
    with torch.no_grad():
        for k, v in kw.items():
            getattr(ora, k).copy_(v)
            dst[k].copy_(v)


def _params(m):
    return {k: v.detach() for k, v in m._params().items()}


def _hip_dx(m, x, d_raw, d_geo=None):
    """d x through the C ABI (x route, all points)."""
    dev = m.bounding_box.device
    xg = x.float().to(dev).contiguous()
    pts, M = ops._points_struct(xg, None, None, None)
    d_x = torch.full((M, 3), float("nan"), device=dev)
    dg = None if d_geo is None else d_geo.float().to(dev).contiguous()
    ops.point_grads(m._handle(), _params(m), pts, M, d_raw.float().to(dev).contiguous(), dg, d_x=d_x)
    torch.cuda.synchronize()
    return d_x.cpu()


def _check(m, ora, x, d_raw, what, d_geo=None, levels=None, budget=0.01):
    got = _hip_dx(m, x, d_raw, d_geo)
    ref = H.ref_point_grad(ora, x, d_raw, d_geo, levels=levels)
    o32 = H.o32_point_grad(ora, x, d_raw, d_geo)
    kinks = H.point_kinks(ora, x, d_raw, levels=levels)
    assert float(ref.abs().max()) > 0, f"{what}: the reference is 0: nothing is tested"
    H.check_point_grads(got, ref, o32, kinks, what, budget)
    return got, ref


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


# --------------------------------------------------------------------------------------------- 2. each term on its own
LEVEL_CONFIGS = ["office12", "office16", "unit1024", "mp3d", "t22", "drawn3", "drawn7"]


def _level_points(rs, scale, res, n_rand=256, n_face=48):
    """Random points in and around [0,1]^3, points on the level's cell faces (fmaf(scale, x, 0.5f) ~ integer) along each axis, and
    their 1-ulp neighbours."""
    pts = [rs.uniform(-0.3, 1.3, (n_rand, 3)).astype(np.float32)]
    for axis in range(3):
        k = rs.randint(0, int(res) + 1, n_face)
        face = ((k - 0.5) / np.float64(scale)).astype(np.float32)
        for v in (face, np.nextafter(face, np.float32(-np.inf)), np.nextafter(face, np.float32(np.inf))):
            p = rs.uniform(-0.1, 1.1, (n_face, 3)).astype(np.float32)
            p[:, axis] = v
            pts.append(p)
    return _f32(np.concatenate(pts))


@pytest.mark.parametrize("kind", LEVEL_CONFIGS)
def test_single_level_jacobians(gpu, kind):
    """One hash level at a time: the table zero outside level l, the OneBlob columns of sdf_w0 and col_w0 zero, no uncertainty
    cotangent -- d x is then level l's Jacobian contracted with the MLP backward.  All 16 levels, with points on l's cell faces,
    their 1-ulp neighbours and points outside [0,1]^3."""
    cfg, ora, m = _setup(kind, 71)
    sc, res, size, off = m._handle().levels()
    assert [int(v) for v in off] == [int(v) for v in ora.meta.offset]
    table0 = ora.table.detach().clone()
    W0, C0 = ora.sdf_w0.detach().clone(), ora.col_w0.detach().clone()
    W0[:, 32:] = 0
    C0[:, :48] = 0
    _set(ora, m, sdf_w0=W0, col_w0=C0)
    rs = np.random.RandomState(72)
    for lvl in range(16):
        t = torch.zeros_like(table0)
        a, b = 2 * int(off[lvl]), 2 * int(off[lvl + 1])
        t[a:b] = table0[a:b]
        _set(ora, m, table=t)
        x = _level_points(rs, sc[lvl], res[lvl])
        d_raw = torch.from_numpy(rs.normal(size=(x.shape[0], 5)).astype(np.float32))
        d_raw[:, 4] = 0
        _check(m, ora, x, d_raw, f"{kind} level {lvl}", levels=(lvl,))


ONEBLOB_SWEEP = np.unique(np.concatenate([
    np.linspace(-1.2, 2.2, 1201), np.arange(-19, 36) / 16.0, [-0.93, 1.93, -0.9375, 1.9375, 0.0, 1.0, -0.5, 0.5, 1.5],
    1.0 - 2.0 ** -np.arange(1, 24), 2.0 ** -np.arange(1, 24)])).astype(np.float32)


@pytest.mark.parametrize("kind", LEVEL_CONFIGS)
def test_oneblob_alone(gpu, kind):
    """A zero table and no uncertainty cotangent: d x is OneBlob's derivative and the MLP backward.  Each axis swept over
    [-1.2, 2.2] with the bin edges k/16 (where |u| = 1 for the neighbouring bins and the rounding r switches at +-0.5), their
    1-ulp neighbours (both sides of bin 15's wrap), 0, 1 and the values of test_query_boundary_sweeps."""
    cfg, ora, m = _setup(kind, 81)
    _set(ora, m, table=torch.zeros_like(ora.table))
    rs = np.random.RandomState(82)
    edges = (np.arange(-19, 36) / 16.0).astype(np.float32)
    sweep = np.unique(np.concatenate([ONEBLOB_SWEEP, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))]))
    pts = []
    for axis in range(3):
        p = rs.uniform(0.05, 0.95, (len(sweep), 3)).astype(np.float32)
        p[:, axis] = sweep
        pts.append(p)
    x = _f32(np.concatenate(pts))
    d_raw = torch.from_numpy(rs.normal(size=(x.shape[0], 5)).astype(np.float32))
    d_raw[:, 4] = 0
    _check(m, ora, x, d_raw, f"{kind} OneBlob")


UNCERT_CONFIGS = ["office16", "mp3d", "drawn3", "drawn7"]     # LEVEL_CONFIGS with D != H != W (the unit cubes' grids are 11^3,
                                                              # where an axis swap cannot show; the table does not enter this term)


@pytest.mark.parametrize("kind", UNCERT_CONFIGS)
def test_uncertainty_alone(gpu, kind):
    """Cotangent (0, 0, 0, 0, g), no d_geo: d x is the uncertainty sample's gradient only.  A random grid (the closed-form one is
    smooth enough to hide an axis swap) of D != H != W; points inside, within half a voxel of each face (4 of 8 corners in the zero
    padding), fully outside (exactly 0) and on voxel centres (where the interpolation cell changes: one-sided).  Up to 5 % of the
    points may be left out: 60 of the ~1380 sit on voxel centres, where the two fp32 roundings of the voxel index may disagree."""
    cfg, ora, m = _setup(kind, 91)
    D, Hh, W = ora.uncert_grid.shape
    assert len({D, Hh, W}) == 3
    rs = np.random.RandomState(92)
    _set(ora, m, uncert_grid=torch.from_numpy(rs.uniform(-2.0, 5.0, (D, Hh, W)).astype(np.float32)))
    n_ax = np.array([W, Hh, D], dtype=np.float64)             # coordinate 0 walks W (the x <-> z quirk)
    pts = [rs.uniform(0.0, 1.0, (600, 3))]
    for axis in range(3):
        for lo, hi in ((-1.0, 0.5), (n_ax[axis] - 1.5, n_ax[axis])):          # ix = x N - 0.5 within half a voxel of the first / last centre
            p = rs.uniform(0.0, 1.0, (60, 3))
            p[:, axis] = (rs.uniform(lo, hi, 60) + 0.5) / n_ax[axis]
            pts.append(p)
    centres = (rs.randint(0, np.array([W, Hh, D]), (60, 3)) + 0.5) / n_ax
    pts.append(centres)
    outside = rs.uniform(0.0, 1.0, (60, 3))
    outside[:30, 0] = -rs.uniform(0.6, 3.0, 30) / W
    outside[30:, 2] = 1.0 + rs.uniform(0.6, 3.0, 30) / D
    pts.append(outside)
    x = _f32(np.concatenate(pts))
    d_raw = torch.zeros(x.shape[0], 5)
    d_raw[:, 4] = torch.from_numpy(rs.normal(size=x.shape[0]).astype(np.float32))
    got, ref = _check(m, ora, x, d_raw, f"{kind} uncertainty", budget=0.05)
    assert torch.equal(got[-60:], torch.zeros(60, 3)), "points fully outside the grid must get an exact 0"
    assert float(ref[:600].abs().max()) > 0


@pytest.mark.parametrize("kind", LEVEL_CONFIGS)
def test_mlp_branches_and_the_wave_uniform_colour_skip(gpu, kind):
    """Cotangents on rgb only, sdf only, geo only, uncertainty only; then rgb cotangents on some lanes of a wave only (alternating
    lanes, one lane per wave, whole zero waves next to non-zero ones), every lane with an sdf cotangent: the kernel runs the colour
    net for a wave if ANY lane wants it, and the lanes without an rgb cotangent must come out as if it had not run."""
    cfg, ora, m = _setup(kind, 101)
    rs = np.random.RandomState(102)
    N = 64 * 40
    x = _f32(rs.uniform(-0.1, 1.1, (N, 3)))
    r = torch.from_numpy(rs.normal(size=(N, 5)).astype(np.float32))
    geo = torch.from_numpy(rs.normal(size=(N, 15)).astype(np.float32))
    zero = torch.zeros(N, 5)
    for name, keep in (("rgb", [0, 1, 2]), ("sdf", [3]), ("uncert", [4])):
        d = zero.clone()
        d[:, keep] = r[:, keep]
        _check(m, ora, x, d, f"{kind} {name} only")
    _check(m, ora, x, zero.clone(), f"{kind} geo only", d_geo=geo)
    lane = torch.arange(N)
    for name, mask in (("alternating lanes", lane % 2 == 0), ("one lane per wave", lane % 64 == 17),
                       ("alternating waves", (lane // 64) % 2 == 0)):
        d = r.clone()
        d[~mask, :3] = 0
        d[:, 4] = 0
        _check(m, ora, x, d, f"{kind} {name}")


# --------------------------------------------------------------------------------------------- 3. config sweep, both routes
SWEEP = [f"drawn{k}" for k in range(10)] + ["mp3d", "unit1024", "t20", "t22"]


@pytest.mark.parametrize("kind", SWEEP)
def test_config_sweep_both_routes(gpu, kind):
    """x route (query_color_sdf; query_sdf with geo and uncertainty) and ray route (render_rays under autograd, rays requiring grad)
    on drawn boxes and on mp3d, unit1024, T = 2^20 and 2^22.  Each against the fp64 reference: the relative l2 within _bound of the
    oracle's own fp32 error, and every non-kink point element by element."""
    cfg, ora, m = _setup(kind, 111)
    rs = np.random.RandomState(112)
    n = 1500
    x = _f32(rs.uniform(-0.3, 1.3, (n, 3)))
    d_raw = torch.from_numpy(rs.normal(size=(n, 5)).astype(np.float32))
    d_geo = torch.from_numpy(rs.normal(size=(n, 15)).astype(np.float32))
    d_sdf = d_raw.clone()
    d_sdf[:, :3] = 0
    for name, fn, d, dg in (("query_color_sdf", lambda p: (m.query_color_sdf(p) * d_raw.to(gpu)).sum(), d_raw, None),
                            ("query_sdf", lambda p: _sdf_loss(m.query_sdf(p, return_geo=True, return_uncert=True), d_raw, d_geo), d_sdf, d_geo)):
        xa = x.to(gpu).requires_grad_(True)
        fn(xa).backward()
        got = xa.grad.cpu()
        ref = H.ref_point_grad(ora, x, d, dg)
        o32 = H.o32_point_grad(ora, x, d, dg)
        assert H.rel(got, ref) <= H.bound(o32, ref), f"{kind} {name}: rel l2 {H.rel(got, ref):.3e}"
        H.check_point_grads(got, ref, o32, H.point_kinks(ora, x, d), f"{kind} {name}")
    # ray route
    n_rays = 96
    bb = np.asarray(cfg["mapping"]["bound"], dtype=np.float64)
    ro = _f32(rs.uniform(bb[:, 0], bb[:, 1], (n_rays, 3)))
    rd = _f32(rs.normal(size=(n_rays, 3)))
    td = _f32(rs.uniform(0.3, 2.0, (n_rays, 1)))
    cfg["training"]["perturb"] = 1.0
    S_tot = cfg["training"]["n_samples_d"] + cfg["training"]["n_range_d"]
    rand = torch.from_numpy(rs.uniform(size=(n_rays, S_tot)).astype(np.float32))
    roa, rda = ro.to(gpu).requires_grad_(True), rd.to(gpu).requires_grad_(True)
    ret = m.render_rays(roa, rda, target_d=td.to(gpu), rand=rand.to(gpu))
    w = torch.from_numpy(rs.normal(size=tuple(ret["raw"].shape)).astype(np.float32))
    (ret["raw"] * w.to(gpu)).sum().backward()
    H.check_ray_grads(ora, cfg["mapping"]["bound"], ro, rd, ret["z_vals"].detach().cpu(), w, roa.grad.cpu(), rda.grad.cpu(), kind)


def _sdf_loss(out, d_raw, d_geo):
    su, geo = out
    dev = su.device
    return (su * d_raw[:, 3:5].to(dev)).sum() + (geo * d_geo.to(dev)).sum()


# --------------------------------------------------------------------------------------------- 4. launch edges through the C ABI
def _guarded(rows, fill, dev, width=3):
    """A [rows, width] view into a buffer with G sentinel rows before and after it."""
    buf = torch.full((rows + 2 * G, width), SENTINEL, dtype=torch.float32, device=dev)
    v = buf[G:G + rows]
    if rows:
        v.fill_(fill)
    return buf, v


def _guards_intact(buf, what):
    torch.cuda.synchronize()
    b = buf.cpu()
    assert torch.equal(b[:G], torch.full_like(b[:G], SENTINEL)) and torch.equal(b[-G:], torch.full_like(b[-G:], SENTINEL)), \
        f"{what}: a guard row was written"


@pytest.fixture(scope="module")
def edge_field():
    cfg, ora, m = _setup("office12", 121)
    return cfg, ora, m


def _x_call(m, x, d_raw, out, active=None, n_active=None, accumulate=False, M=None):
    pts, _ = ops._points_struct(x, None, None, None)
    ops.point_grads(m._handle(), _params(m), pts, x.shape[0] if M is None else M, d_raw, None, d_x=out, active=active, n_active=n_active, accumulate=accumulate)
    torch.cuda.synchronize()


def test_x_route_sizes_and_guards(gpu, edge_field):
    """M in {0, 1, 63, 64, 127, 129, 4097} (partial blocks of 128): outputs as views between sentinel rows, NaN-filled: every row
    written, no guard touched, each row the same bits as in the 4097-point call, which itself matches the reference.  M = 0 is OK
    and writes nothing."""
    cfg, ora, m = edge_field
    rs = np.random.RandomState(122)
    X = _f32(rs.uniform(-0.2, 1.2, (4097, 3)))
    R = torch.from_numpy(rs.normal(size=(4097, 5)).astype(np.float32))
    full = None
    xb, x = _guarded(1, 0.0, gpu)                 # M = 0: valid pointers (an empty tensor has none), nothing read or written
    rb, d = _guarded(1, 0.0, gpu, 5)
    ob, out = _guarded(1, SENTINEL, gpu)
    _x_call(m, x, d, out, M=0)
    assert torch.equal(ob.cpu(), torch.full_like(ob.cpu(), SENTINEL)), "M=0 wrote"
    for M in (4097, 1, 63, 64, 127, 129):
        xb, x = _guarded(M, 0.0, gpu)
        rb, d = _guarded(M, 0.0, gpu, 5)
        if M:
            x.copy_(X[:M])
            d.copy_(R[:M])
        ob, out = _guarded(M, float("nan"), gpu)
        _x_call(m, x, d, out)
        _guards_intact(ob, f"M={M}")
        got = out.cpu()
        assert not torch.isnan(got).any(), f"M={M}: a row was not written"
        if M == 4097:
            full = got
            ref = H.ref_point_grad(ora, X, R)
            H.check_point_grads(got, ref, H.o32_point_grad(ora, X, R), H.point_kinks(ora, X, R), "M=4097")
        else:
            assert torch.equal(got, full[:M]), f"M={M}: rows differ from the 4097-point call"


RAY_SHAPES = [(1, 1), (3, 2), (5, 63), (7, 64), (9, 65), (33, 129), (4097, 43), (2, 1024)]


def _rays(rs, n, S, cfg, dev):
    bb = np.asarray(cfg["mapping"]["bound"], dtype=np.float64)
    ro = _f32(rs.uniform(bb[:, 0], bb[:, 1], (n, 3)))
    rd = _f32(rs.normal(size=(n, 3)))
    z = torch.from_numpy(np.sort(rs.uniform(0.05, 3.0, (n, S)), 1).astype(np.float32))
    d = torch.from_numpy(rs.normal(size=(n * S, 5)).astype(np.float32))
    return ro, rd, z, d


def _ray_call(m, ro, rd, z, d_raw, d_o, d_d, active=None, n_active=None, accumulate=False):
    pts, M = ops._points_struct(None, ro, rd, z)
    ops.point_grads(m._handle(), _params(m), pts, M, d_raw, None, d_rays_o=d_o, d_rays_d=d_d, active=active, n_active=n_active,
                    accumulate=accumulate)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", RAY_SHAPES, ids=[f"{n}x{s}" for n, s in RAY_SHAPES])
def test_ray_route_against_x_route(gpu, edge_field, shape):
    """The ray route on (n_rays, S) that leave the reduction's last 4-ray block and the per-lane strides partly filled: guard rows
    untouched, every row written; d_rays_o[n] = sum_s fl(d_x[n,s] / ext) and d_rays_d[n] = sum_s z fl(d_x[n,s] / ext), with d_x from
    the x route on the same points formed as load_point forms them (the same bits per point), summed in fp64.  Bound: the kernel's
    sum is ceil(S/64) strided adds, a 6-level tree and one fma per term -- (ceil(S/64) + 7) 2^-24 of the sum of |terms|.
    Then d_rays_o alone and d_rays_d alone: the same bits as with both, nothing else written."""
    cfg, ora, m = edge_field
    n, S = shape
    rs = np.random.RandomState(131 + n)
    ro, rd, z, d = _rays(rs, n, S, cfg, gpu)
    rob, rog = _guarded(n, 0.0, gpu)
    rdb, rdg = _guarded(n, 0.0, gpu)
    rog.copy_(ro)
    rdg.copy_(rd)
    zg, dg = z.to(gpu).contiguous(), d.to(gpu).contiguous()
    ob, d_o = _guarded(n, float("nan"), gpu)
    db, d_d = _guarded(n, float("nan"), gpu)
    _ray_call(m, rog, rdg, zg, dg, d_o, d_d)
    for buf, v, what in ((ob, d_o, "d_rays_o"), (db, d_d, "d_rays_d")):
        _guards_intact(buf, f"{shape} {what}")
        assert not torch.isnan(v.cpu()).any(), f"{shape} {what}: a ray was not written"
    xr, ext = H.ray_points(cfg["mapping"]["bound"], ro, rd, z)
    dx = _hip_dx(m, xr, d)
    g = (dx / ext).double().reshape(n, S, 3)
    zz = z.double()[..., None]
    k = (S + 63) // 64 + 7
    for what, got, terms in (("d_rays_o", d_o, g), ("d_rays_d", d_d, g * zz)):
        want = terms.sum(1)
        tol = k * 2.0 ** -24 * terms.abs().sum(1)
        err = (got.cpu().double() - want).abs()
        assert bool((err <= tol).all()), f"{shape} {what}: max err {float(err.max()):.3e}, over by {float((err - tol).max()):.3e}"
    both = (d_o.cpu().clone(), d_d.cpu().clone())
    for which in (0, 1):
        ob2, o2 = _guarded(n, float("nan"), gpu)
        _ray_call(m, rog, rdg, zg, dg, o2 if which == 0 else None, o2 if which == 1 else None)
        _guards_intact(ob2, f"{shape} only output {which}")
        assert torch.equal(o2.cpu(), both[which]), f"{shape}: only {('d_rays_o', 'd_rays_d')[which]} differs from the both-outputs call"
    _guards_intact(rob, "rays_o")
    _guards_intact(rdb, "rays_d")


def test_lists_and_accumulation(gpu, edge_field):
    """The active list on the x route (non-accumulating: rows off the list are 0; accumulating: they keep their prior bits and listed
    rows are fl(prior + fresh)), an empty list on both routes, a list in non-monotone order (the same bits as the all-points call with
    d_raw zeroed off the list), and the ray route accumulating onto a random non-zero prior (fl(prior + fresh), bit for bit)."""
    cfg, ora, m = edge_field
    rs = np.random.RandomState(141)
    M = 4097
    x = _f32(rs.uniform(-0.2, 1.2, (M, 3))).to(gpu)
    d = torch.from_numpy(rs.normal(size=(M, 5)).astype(np.float32)).to(gpu)
    fresh = torch.full((M, 3), float("nan"), device=gpu)
    _x_call(m, x, d, fresh)
    lst = torch.from_numpy(rs.permutation(M)[:1500].astype(np.int32)).to(gpu)     # non-monotone
    on = torch.zeros(M, dtype=torch.bool, device=gpu)
    on[lst.long()] = True
    n_act = torch.tensor([lst.numel()], dtype=torch.int32, device=gpu)
    # non-accumulating
    ob, out = _guarded(M, float("nan"), gpu)
    _x_call(m, x, d, out, lst, n_act)
    _guards_intact(ob, "list")
    assert torch.equal(out[on], fresh[on]) and bool((out[~on] == 0).all()), "list: listed rows must be the all-points bits, others 0"
    dz = torch.where(on[:, None], d, torch.zeros_like(d))
    ref_z = torch.full((M, 3), float("nan"), device=gpu)
    _x_call(m, x, dz, ref_z)
    assert torch.equal(out, ref_z), "list: not the bits of the all-points call with d_raw zeroed off the list"
    # accumulating
    prior = torch.from_numpy(rs.normal(size=(M, 3)).astype(np.float32)).to(gpu)
    ob, out = _guarded(M, 0.0, gpu)
    out.copy_(prior)
    _x_call(m, x, d, out, lst, n_act, accumulate=True)
    _guards_intact(ob, "list, accumulate")
    assert torch.equal(out[~on], prior[~on]), "list, accumulate: a row off the list changed"
    assert torch.equal(out[on], (prior + fresh)[on]), "list, accumulate: listed rows are not fl(prior + fresh)"
    # empty list
    zero = torch.zeros(1, dtype=torch.int32, device=gpu)
    ob, out = _guarded(M, float("nan"), gpu)
    _x_call(m, x, d, out, lst, zero)
    _guards_intact(ob, "empty list")
    assert bool((out == 0).all()), "empty list, non-accumulating: every row must be 0"
    out.copy_(prior)
    _x_call(m, x, d, out, lst, zero, accumulate=True)
    assert torch.equal(out, prior), "empty list, accumulating: a row changed"
    # ray route
    n, S = 257, 43
    ro, rd, z, dr = _rays(rs, n, S, cfg, gpu)
    ro, rd, z, dr = (t.to(gpu).contiguous() for t in (ro, rd, z, dr))
    fo, fd = torch.full((n, 3), float("nan"), device=gpu), torch.full((n, 3), float("nan"), device=gpu)
    _ray_call(m, ro, rd, z, dr, fo, fd)
    po = torch.from_numpy(rs.normal(size=(n, 3)).astype(np.float32)).to(gpu)
    pd = torch.from_numpy(rs.normal(size=(n, 3)).astype(np.float32)).to(gpu)
    ao, ad = po.clone(), pd.clone()
    _ray_call(m, ro, rd, z, dr, ao, ad, accumulate=True)
    assert torch.equal(ao, po + fo) and torch.equal(ad, pd + fd), "ray route, accumulate: not fl(prior + fresh)"
    rl = torch.from_numpy(rs.permutation(n * S)[:3000].astype(np.int32)).to(gpu)
    ob, eo = _guarded(n, float("nan"), gpu)
    _ray_call(m, ro, rd, z, dr, eo, None, rl, zero)
    _guards_intact(ob, "ray route, empty list")
    assert bool((eo == 0).all()), "ray route, empty list: every ray must be 0"
    onr = torch.zeros(n * S, dtype=torch.bool, device=gpu)
    onr[rl.long()] = True
    drz = torch.where(onr[:, None], dr, torch.zeros_like(dr))
    lo, ld = torch.full_like(fo, float("nan")), torch.full_like(fd, float("nan"))
    _ray_call(m, ro, rd, z, dr, lo, ld, rl, torch.tensor([rl.numel()], dtype=torch.int32, device=gpu))
    zo, zd = torch.full_like(fo, float("nan")), torch.full_like(fd, float("nan"))
    _ray_call(m, ro, rd, z, drz, zo, zd)
    assert torch.equal(lo, zo) and torch.equal(ld, zd), "ray route, non-monotone list: not the bits of the zeroed all-points call"


# --------------------------------------------------------------------------------------------- 5. full size (configs[4]'s shard)
_FULL_SCRIPT = r"""
import sys
import numpy as np
import torch
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, root + "/tests")
import helpers as H
from naruto_amd import config as C, ops

dev = torch.device("cuda:0")
cfg = C.unit_cube_config(1024, 22)
ora = H.make_oracle(cfg, 0.25, 161)
m = H.make_hip_from_oracle(cfg, ora, dev)
del ora
N, S = 131072, 43
M = N * S
g = torch.Generator(device=dev).manual_seed(162)
ro = torch.rand(N, 3, generator=g, device=dev) * 1.2 - 0.1
rd = torch.randn(N, 3, generator=g, device=dev)
z = torch.sort(torch.rand(N, S, generator=g, device=dev) * 1.5 + 0.02, 1).values.contiguous()
d_raw = torch.randn(M, 5, generator=g, device=dev)
x = (torch.rand(M, 3, generator=g, device=dev) * 1.4 - 0.2).contiguous()
params = {k: v.detach() for k, v in m._params().items()}
rays, _ = ops._points_struct(None, ro, rd, z)
pts, _ = ops._points_struct(x, None, None, None)
res = []
for rep in range(2):
    d_o = torch.full((N, 3), float("nan"), device=dev)
    d_d = torch.full((N, 3), float("nan"), device=dev)
    d_x = torch.full((M, 3), float("nan"), device=dev)
    ops.point_grads(m._handle(), params, rays, M, d_raw, None, d_rays_o=d_o, d_rays_d=d_d)
    ops.point_grads(m._handle(), params, pts, M, d_raw, None, d_x=d_x)
    torch.cuda.synchronize()
    res.append((d_o.cpu(), d_d.cpu(), d_x.cpu()))
same = all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
nan = any(bool(torch.isnan(t).any()) for t in res[0])
rs = np.random.RandomState(163)
# samples whose index, or element offset in the [M,3] point / output and [M,5] cotangent arrays, crosses 2^22, 2^23 or 2^24
cross = sorted({-(-(1 << k) // w) + d for k in (22, 23, 24) for w in (1, 3, 5) for d in (-1, 0)} & set(range(M)))
edge_rays = [0, N - 1] + [c // S for c in cross]
ray_ids = np.unique(np.concatenate([rs.choice(N, 2040, replace=False), edge_rays]))
edge_rows = [0, M - 1] + cross
row_ids = np.unique(np.concatenate([rs.choice(M, 4090, replace=False), edge_rows]))
ri, xi = torch.from_numpy(ray_ids), torch.from_numpy(row_ids)
samp = (ri[:, None] * S + torch.arange(S)[None, :]).reshape(-1)
dr = d_raw.cpu()
np.savez(out, same=np.array([same]), nan=np.array([nan]), ray_ids=ray_ids, row_ids=row_ids,
         ro=ro.cpu()[ri].numpy(), rd=rd.cpu()[ri].numpy(), z=z.cpu()[ri].numpy(), ray_draw=dr[samp].reshape(len(ray_ids), S, 5).numpy(),
         d_o=res[0][0][ri].numpy(), d_d=res[0][1][ri].numpy(),
         x=x.cpu()[xi].numpy(), row_draw=dr[xi].numpy(), d_x=res[0][2][xi].numpy())
"""


def test_full_size_shard(gpu, tmp_path):
    """BASELINE configs[4]'s shard at full size: 131 072 rays x 43 samples (5.6 M points, sample indices past 2^22 and 2^23), T = 2^22,
    random d_raw, both routes, in a child process with a time limit.  Two calls give the same bits and write every row; ~2 048
    sampled rays and ~4 096 sampled x rows against the fp64 reference, among them the first and last ray / row and the samples on
    both sides of index 2^22 and of the element offsets 2^22, 2^23, 2^24 in the [M,3] and [M,5] arrays (M = 5 636 096 < 2^23, so
    no sample index reaches 2^23 itself), evaluated on those points only (check_ray_grads,
    check_point_grads; the reference gathers only the table entries they touch)."""
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "full_points.py"
    script.write_text(_FULL_SCRIPT)
    out = tmp_path / "full_points.npz"
    subprocess.run([sys.executable, str(script), root, str(out)], check=True, timeout=600)
    r = dict(np.load(out))
    assert bool(r["same"][0]), "two full-size calls differ"
    assert not bool(r["nan"][0]), "a ray or row was not written"
    N, S = 131072, 43
    assert {N - 1, (1 << 22) // S, -(-(1 << 24) // 3) // S} <= set(r["ray_ids"].tolist())
    assert {N * S - 1, 1 << 22, -(-(1 << 24) // 3)} <= set(r["row_ids"].tolist())
    cfg = C.unit_cube_config(1024, 22)
    ora = H.make_oracle(cfg, 0.25, 161)
    H.check_ray_grads(ora, cfg["mapping"]["bound"], torch.from_numpy(r["ro"]), torch.from_numpy(r["rd"]), torch.from_numpy(r["z"]),
                      torch.from_numpy(r["ray_draw"]), torch.from_numpy(r["d_o"]), torch.from_numpy(r["d_d"]), "full size")
    x, dr = torch.from_numpy(r["x"]), torch.from_numpy(r["row_draw"])
    H.check_point_grads(r["d_x"], H.ref_point_grad(ora, x, dr), H.o32_point_grad(ora, x, dr), H.point_kinks(ora, x, dr), "full size x rows")


# --------------------------------------------------------------------------------------------- 6. Python routes against oracle autograd
def test_python_routes_against_oracle(gpu):
    """run_network on world points [a, b, 3]; render_rays under autograd with rays requiring grad, with target_d and on the n_samples
    path; render_surface_color under autograd (rays_o and normal); query_color; query_sdf without geo, and without geo and
    uncertainty.  Each gradient within _bound of the oracle's own fp32-vs-fp64 error (floor 1e-4 where a ray sums samples)."""
    cfg = H.office_cfg(16, perturb=1.0)
    cfg["training"]["n_samples"] = 48
    o32, o64 = H.oracle_pair(H.make_oracle(cfg, 0.25, 151))
    m = H.make_hip_from_oracle(cfg, o32, gpu)
    rs = np.random.RandomState(152)
    bb = np.asarray(cfg["mapping"]["bound"], dtype=np.float64)
    wp = torch.from_numpy(rs.uniform(bb[:, 0] - 0.3, bb[:, 1] + 0.3, (12, 40, 3)))
    ro = torch.from_numpy(rs.uniform(bb[:, 0] * 0.8, bb[:, 1] * 0.8, (256, 3)))
    rd = torch.from_numpy(rs.normal(size=(256, 3)))
    td = torch.from_numpy(rs.uniform(0.3, 2.5, (256, 1)))
    x = torch.from_numpy(rs.uniform(-0.1, 1.1, (2048, 3)))
    S_tot = cfg["training"]["n_samples_d"] + cfg["training"]["n_range_d"]
    rand = torch.from_numpy(rs.uniform(size=(256, S_tot)))
    rand_n = torch.from_numpy(rs.uniform(size=(256, 48)))
    w5 = torch.from_numpy(rs.normal(size=(12, 40, 5)))
    w3 = torch.from_numpy(rs.normal(size=(256, 3)))
    wx = torch.from_numpy(rs.normal(size=(2048, 3)))
    w2 = torch.from_numpy(rs.normal(size=(2048, 2)))
    w1 = torch.from_numpy(rs.normal(size=2048))

    def rr(mod, a, b, target, rnd, dev, dt):
        ret = mod.render_rays(a, b, target_d=None if target is None else target.to(dev, dt), rand=rnd.to(dev, dt))
        return (ret["rgb"] * w3.to(dev, dt)).sum() + (ret["depth"] * w3[:, 0].to(dev, dt)).sum()

    cases = {
        "run_network": ((wp,), lambda mod, dev, dt, p: (mod.run_network(p) * w5.to(dev, dt)).sum(), 2e-5),
        "render_rays target_d": ((ro, rd), lambda mod, dev, dt, a, b: rr(mod, a, b, td, rand, dev, dt), 1e-4),
        "render_rays n_samples": ((ro, rd), lambda mod, dev, dt, a, b: rr(mod, a, b, None, rand_n, dev, dt), 1e-4),
        "render_surface_color": ((ro, rd / rd.norm(dim=1, keepdim=True)),
                                 lambda mod, dev, dt, a, b: (mod.render_surface_color(a, b) * w3.to(dev, dt)).sum(), 1e-4),
        "query_color": ((x,), lambda mod, dev, dt, p: (mod.query_color(p) * wx.to(dev, dt)).sum(), 2e-5),
        "query_sdf uncert": ((x,), lambda mod, dev, dt, p: (mod.query_sdf(p, return_uncert=True) * w2.to(dev, dt)).sum(), 2e-5),
        "query_sdf": ((x,), lambda mod, dev, dt, p: (mod.query_sdf(p) * w1.to(dev, dt)).sum(), 2e-5),
    }
    for name, (inputs, fn, floor) in cases.items():
        res = {}
        for tag, mod, dev, dt in (("hip", m, gpu, torch.float32), ("o32", o32, "cpu", torch.float32), ("o64", o64, "cpu", torch.float64)):
            mod.eval()
            leaves = [t.detach().clone().to(dev, dt).requires_grad_(True) for t in inputs]
            fn(mod, dev, dt, *leaves).backward()
            assert all(t.grad is not None for t in leaves), f"{name}: {tag} gave no gradient"
            res[tag] = [t.grad.detach().double().cpu() for t in leaves]
        for i in range(len(inputs)):
            got, a, b = res["hip"][i], res["o32"][i], res["o64"][i]
            assert float(got.abs().sum()) > 0, f"{name}: input {i} has a zero gradient"
            bnd = H.bound(a, b, floor=floor)
            assert H.rel(got, b) <= bnd, f"{name} input {i}: rel l2 {H.rel(got, b):.3e} > {bnd:.3e}"

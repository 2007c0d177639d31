"""Shared helpers for the parity tests: identical parameters in the oracle (CPU) and the HIP module."""
import os

import numpy as np
import torch

from naruto_amd import config as C
from naruto_amd import synthetic as syn
from oracle import spec_torch as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def office_cfg(hash_size=16, perturb=0.0, n_samples_d=32, **kw):
    cfg = C.office0_config(perturb=perturb, n_samples_d=n_samples_d, **kw)
    cfg["grid"]["hash_size"] = hash_size
    return cfg


def drawn_field_config(case):
    """test_random_field_configs' drawn config: an anisotropic box (1 .. 25 m per axis), a finest voxel and a table size
    2^10 .. 2^18.  Returns the config and the generator, positioned after the config's draws."""
    rs = np.random.RandomState(500 + case)
    ext = rs.uniform(1.0, 25.0, 3)
    lo = rs.uniform(-10.0, 5.0, 3)
    cfg = C.office0_config()
    cfg["mapping"]["bound"] = [[float(lo[i]), float(lo[i] + ext[i])] for i in range(3)]
    cfg["mapping"]["marching_cubes_bound"] = cfg["mapping"]["bound"]
    cfg["grid"]["voxel_sdf"] = float(rs.choice([0.02, 0.04, 0.1]))
    cfg["grid"]["hash_size"] = int(rs.choice([10, 12, 14, 16, 17, 18]))
    return cfg, rs


def make_oracle(cfg, table_amp, seed, weights=None, uncert_voxel=0.1):
    bbox = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32)
    ora = S.OracleField(cfg, bbox, uncert_voxel)
    w = weights if weights is not None else syn.mlp_weights(seed)
    dims = S.uncert_grid_dims(bbox, uncert_voxel)
    with torch.no_grad():
        ora.table.copy_(torch.from_numpy(syn.closed_form_table(ora.meta.n_params, table_amp)))
        ora.sdf_w0.copy_(torch.from_numpy(w["sdf_w0"]))
        ora.sdf_w1.copy_(torch.from_numpy(w["sdf_w1"]))
        ora.col_w0.copy_(torch.from_numpy(w["col_w0"]))
        ora.col_w1.copy_(torch.from_numpy(w["col_w1"]))
        ora.uncert_grid.copy_(torch.from_numpy(syn.closed_form_uncert_grid(dims)))
    return ora


def make_hip_from_oracle(cfg, ora, device, uncert_voxel=0.1):
    from naruto_amd.field import NarutoFieldHIP
    bbox = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32, device=device)
    m = NarutoFieldHIP(cfg, bbox).to(device)
    m.get_uncert_grid(uncert_voxel)
    with torch.no_grad():
        assert m.embed_fn.params.numel() == ora.table.numel()
        m.embed_fn.params.copy_(ora.table)
        m.decoder.sdf_net.model[0].weight.copy_(ora.sdf_w0)
        m.decoder.sdf_net.model[2].weight.copy_(ora.sdf_w1)
        m.decoder.color_net.model[0].weight.copy_(ora.col_w0)
        m.decoder.color_net.model[2].weight.copy_(ora.col_w1)
        assert tuple(m.uncert_grid.shape) == tuple(ora.uncert_grid.shape)
        m.uncert_grid.copy_(ora.uncert_grid)
    return m


def hip_grads(m):
    return {"sdf_w0": m.decoder.sdf_net.model[0].weight.grad, "sdf_w1": m.decoder.sdf_net.model[2].weight.grad,
            "col_w0": m.decoder.color_net.model[0].weight.grad, "col_w1": m.decoder.color_net.model[2].weight.grad,
            "uncert_grid": m.uncert_grid.grad, "table": m.embed_fn.params.grad}


def ora_grads(o):
    return {"sdf_w0": o.sdf_w0.grad, "sdf_w1": o.sdf_w1.grad, "col_w0": o.col_w0.grad, "col_w1": o.col_w1.grad,
            "uncert_grid": o.uncert_grid.grad, "table": o.table.grad}


def assert_close(a, b, tol, what, rel=0.0):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN pattern differs"
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
    err = (a - b).abs()
    bound = tol + rel * b.abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: max abs err {err.max().item():.3e} (tol {tol:g}, rel {rel:g}) at "
                           f"{int(bad.sum())}/{bad.numel()} elements; worst idx {int(err.argmax())}, "
                           f"got {a.reshape(-1)[int(err.argmax())].item():.6g} want {b.reshape(-1)[int(err.argmax())].item():.6g}")


# ---- the kernels' own uniform numbers (naruto_common.h: splitmix64 keyed by seed, iteration counter, index) ----
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def device_rng_uniform(seed: int, counter: int, idx):
    """float32 array of the values rng_uniform(rng_key({seed, counter}), i) for i in idx (python ints: exact)."""
    key = _splitmix64((seed & _M64) ^ _splitmix64(counter & _M64))
    return np.array([(_splitmix64((key + int(i)) & _M64) >> 40) * 2.0 ** -24 for i in idx], dtype=np.float32)


def grad_close(got, want, what, frac=1e-4):
    """Gradients: frac of the largest magnitude of the wanted tensor + 1e-3 relative."""
    want = torch.as_tensor(want).detach().double().cpu()
    scale = max(want.abs().max().item(), 1e-12)
    assert_close(got, want, frac * scale, what, rel=1e-3)


def relu_kink_distance(ora, cfg, rays_o, rays_d, z_vals, active):
    """Smallest |pre-activation| of either hidden layer over the samples that carry a cotangent (fp64, oracle weights).  A unit
    within fp32 rounding of 0 has its ReLU mask decided by rounding noise: the reference itself would flip it."""
    bb = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32)
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z_vals[..., None]).reshape(-1, 3)
    xn = ((pts - bb[:, 0]) / (bb[:, 1] - bb[:, 0]))[active.reshape(-1)]
    if xn.shape[0] == 0:
        return float("inf"), 0
    with torch.no_grad():
        feats, pos = S.hash_encode(xn, ora.table, ora.meta).double(), S.oneblob_encode(xn, 16).double()
        h = torch.cat([feats, pos], -1) @ ora.sdf_w0.double().T
        out = torch.relu(h) @ ora.sdf_w1.double().T
        c = torch.cat([pos, out[:, 1:]], -1) @ ora.col_w0.double().T
    near = (h.abs() < 2e-6).any(1) | (c.abs() < 2e-6).any(1)
    return min(float(h.abs().min()), float(c.abs().min())), int(near.sum())


# ---- point gradients (naruto_query_bwd_points): the fp64 reference and its tolerances ----
def rel(a, b):
    """Relative l2 distance of a from b (fp64)."""
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def oracle_pair(ora):
    """The oracle in fp32 and an fp64 copy of it (same parameters)."""
    o64 = make_oracle(ora.config, 0.25, 0)
    o64.load_state_dict(ora.state_dict())
    return ora, o64.double()


def bound(o32, o64, factor=4.0, floor=2e-5):
    """Tolerance of a relative l2 comparison: a multiple of the oracle's own fp32 rounding (its fp32 result against its fp64 one),
    with a floor for the cases where the oracle happens to be closer than the summation orders allow."""
    return max(factor * rel(o32, o64), floor)


bound_l2 = bound


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


def hash_encode_cells(x, table, meta, levels=None):
    """S.hash_encode in fp64 with the KERNEL's cell.  x [M,3] fp64 holding fp32 values.  The cell is floorf(fmaf(scale, x, 0.5f)):
    the product of two fp32 numbers is exact in fp64, and so is the sum wherever the cell can change (|scale x| >= 1/2 there),
    so rounding the fp64 pos to fp32 once is the fused multiply-add.  The weights are pos64 - cell, so autograd gives the
    derivative one-sided into that cell at a face (where the fp64 oracle's own floor may pick the other one).  ``levels``: only
    these levels are gathered (the others come out 0, as with a table that is zero outside them).  Only the entries the points touch
    are read, and converted to fp64 after the gather: no fp64 copy of a large table."""
    M = x.shape[0]
    Fd = meta.n_features
    tab = table.detach().reshape(-1, Fd)
    outs = []
    for lvl in range(meta.n_levels):
        if levels is not None and lvl not in levels:
            outs.append(torch.zeros(M, Fd, dtype=x.dtype))
            continue
        pos = x * float(meta.scale[lvl]) + 0.5
        cell = torch.floor(pos.detach().float().double())
        w = pos - cell
        gi = cell.to(torch.int64) & S.U32
        off = int(meta.offset[lvl])
        res = torch.zeros(M, Fd, dtype=x.dtype)
        for corner in range(8):
            wgt = torch.ones(M, dtype=x.dtype)
            c = []
            for dim in range(3):
                if (corner >> dim) & 1:
                    wgt = wgt * w[:, dim]
                    c.append((gi[:, dim] + 1) & S.U32)
                else:
                    wgt = wgt * (1 - w[:, dim])
                    c.append(gi[:, dim])
            idx = S.hash_grid_index(meta, lvl, c[0], c[1], c[2]) + off
            res = res + wgt[:, None] * tab[idx].to(x.dtype)
        outs.append(res)
    return torch.cat(outs, dim=-1)


def _uncert_cells(x, dims):
    """The kernel's uncertainty voxel per axis (uncert_base: gx = 2x - 1, ix = ((gx + 1) N - 1) / 2 in fp32, N = W, H, D for
    coordinates 0, 1, 2).  The compiler may contract (gx + 1) N - 1 into one fma, so both roundings are formed; ``ambiguous`` marks
    the points where they pick different voxels."""
    x32 = x.detach().float()
    n = torch.tensor(dims, dtype=torch.float32)
    g1 = (x32 * 2.0 - 1.0) + 1.0
    split = torch.floor((g1 * n - 1.0) * 0.5)
    fused = torch.floor(((g1.double() * n.double() - 1.0).float()) * 0.5)
    return split.double(), (split != fused).any(1)


def uncert_sample_cells(grid, x):
    """S.sample_uncert_grid_manual in fp64 with the kernel's voxel (see _uncert_cells): grid [D,H,W], x [M,3] fp64 -> [M], ambiguous [M]."""
    D, Hh, W = grid.shape
    cell, amb = _uncert_cells(x, (W, Hh, D))
    i64 = x * torch.tensor([W, Hh, D], dtype=x.dtype) - 0.5
    f = i64 - cell
    c0 = cell.to(torch.int64)
    flat = grid.detach().reshape(-1).double()
    out = torch.zeros(x.shape[0], dtype=x.dtype)
    for corner in range(8):
        d = [(corner >> k) & 1 for k in range(3)]
        wgt = torch.ones(x.shape[0], dtype=x.dtype)
        for k in range(3):
            wgt = wgt * (f[:, k] if d[k] else 1 - f[:, k])
        xi, yi, zi = c0[:, 0] + d[0], c0[:, 1] + d[1], c0[:, 2] + d[2]
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < Hh) & (zi >= 0) & (zi < D)
        idx = (zi.clamp(0, D - 1) * Hh + yi.clamp(0, Hh - 1)) * W + xi.clamp(0, W - 1)
        out = out + torch.where(ok, flat[idx] * wgt, torch.zeros_like(wgt))
    return out, amb


def cell_field(ora, x, table=None, levels=None):
    """The oracle's field at fp32 points x (fp64 tensor) in fp64 with the kernel's hash cells and uncertainty voxels.
    Returns raw [M,5] (rgb, sdf, uncert), geo [M,15], the pre-activations h [M,32] and c [M,32], the ambiguous-voxel mask, and the
    MLP inputs (hash features [M,32], OneBlob [M,48])."""
    W0, W1, C0, C1 = (getattr(ora, k).detach().double() for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1"))
    feats = hash_encode_cells(x, ora.table if table is None else table, ora.meta, levels)
    pos = S.oneblob_encode(x, 16)
    u, amb = uncert_sample_cells(ora.uncert_grid, x)
    h = torch.cat([feats, pos], -1) @ W0.T
    out = torch.relu(h) @ W1.T
    c = torch.cat([pos, out[:, 1:]], -1) @ C0.T
    rgb = torch.relu(c) @ C1.T
    return torch.cat([rgb, out[:, :1], u[:, None]], -1), out[:, 1:], h, c, amb, feats, pos


def point_kinks(ora, x, d_raw=None, table=None, levels=None, d_geo=None):
    """x-space kink detector: points whose gradient a correct fp32 evaluation may legitimately take from another piece.
    (i) A ReLU unit within rounding of 0: a dot product of n <= 80 fp32 terms is off by at most n 2^-24 sum |w_k in_k| (4.8e-6 of it),
    its inputs by a few ulp more: units with |pre-activation| <= 2e-5 sum |w_k in_k| are flagged -- sdf-net units only where a
    cotangent reaches the MLP (rgb, sdf or geo), colour units only where the point has an rgb cotangent.  (ii) An uncertainty voxel
    the two possible fp32 roundings disagree on (only where the uncertainty cotangent is non-zero).  (iii) hash_faces: within 1e-6
    of a hash cell face on some level (not a kink of the reference hash_encode_cells, which picks the kernel's cell; reported for
    the tests that want to know how many such points they hold).  (iv) uncert_faces: within 1e-5 of an uncertainty voxel face with
    an uncertainty cotangent, where the fp32 oracle's grid_sample may take the other voxel: left out of the rounding yardstick of
    check_point_grads, not out of the comparison."""
    W0, W1, C0 = (getattr(ora, k).detach().double() for k in ("sdf_w0", "sdf_w1", "col_w0"))
    x = x.detach().double()
    with torch.no_grad():
        raw, geo, h, c, amb, feats, pos = cell_field(ora, x, table, levels)
        h_mag = torch.cat([feats, pos], -1).abs() @ W0.abs().T
        out = torch.relu(h) @ W1.T
        c_mag = torch.cat([pos, out[:, 1:]], -1).abs() @ C0.abs().T
    relu_h = (h.abs() <= 2e-5 * h_mag).any(1)
    relu_c = (c.abs() <= 2e-5 * c_mag).any(1)
    D, Hh, W = ora.uncert_grid.shape
    fu = torch.frac(x * torch.tensor([W, Hh, D], dtype=x.dtype) - 0.5)
    u_faces = ((fu < 1e-5) | (fu > 1 - 1e-5)).any(1)
    if d_raw is not None:
        d_raw = torch.as_tensor(d_raw).detach().cpu()
        mlp = (d_raw[:, :4] != 0).any(1)
        if d_geo is not None:
            mlp |= (torch.as_tensor(d_geo).detach().cpu() != 0).any(1)
        relu_h &= mlp
        relu_c &= (d_raw[:, :3] != 0).any(1)
        amb = amb & (d_raw[:, 4] != 0)
        u_faces &= d_raw[:, 4] != 0
    faces = torch.zeros(x.shape[0], dtype=torch.bool)
    for lvl in range(ora.meta.n_levels):
        if levels is not None and lvl not in levels:
            continue
        f = torch.frac(x * float(ora.meta.scale[lvl]) + 0.5)
        faces |= ((f < 1e-6) | (f > 1 - 1e-6)).any(1)
    return {"kink": relu_h | relu_c | amb, "relu": relu_h | relu_c, "uncert": amb, "uncert_faces": u_faces, "hash_faces": faces}


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 tensors, exactly (CPU): a b is exact in fp64; the fp64 sum s and its TwoSum error e give the exact
    a b + c rounded to odd (s moved one ulp towards e when e != 0 and s is even), and rounding a round-to-odd fp64 value to fp32
    once is the correctly rounded result (53 >= 24 + 2 bits) -- no double-rounding error whatever the magnitudes."""
    a, b, c = (torch.as_tensor(t).detach().cpu().double() for t in (a, b, c))
    p = a * b
    s = p + c
    bv = s - p
    e = (p - (s - bv)) + (c - bv)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.nextafter(s, torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf"))))
    return torch.where((e != 0) & even, toward, s).float()


def ray_points(bound, ro, rd, z):
    """The kernels' normalised ray points (load_point): p = fmaf(d, z, o), then (p - bmin) / ext, the subtraction and the division
    correctly rounded fp32 operations (torch's CPU float ops).  Returns x [N*S, 3] and ext [3] (fp32)."""
    bb = torch.as_tensor(bound, dtype=torch.float32).cpu()
    bmin, ext = bb[:, 0], bb[:, 1] - bb[:, 0]
    ro, rd, z = (torch.as_tensor(t).detach().cpu().float() for t in (ro, rd, z))
    p = fma32(rd[:, None, :], z[..., None], ro[:, None, :])
    return ((p - bmin) / ext).reshape(-1, 3), ext


def check_ray_grads(ora, bound, ro, rd, z, d_raw, got_o, got_d, what, batch=16384):
    """Ray gradients against the fp64 reference: d rays_o = sum_s ref(x_s) / ext, d rays_d = sum_s z_s ref(x_s) / ext over the
    points as the kernels form them (ray_points), summed in fp64, in batches of ``batch`` points.  Relative l2 within _bound of the
    fp32 oracle's own error, and every ray element by element (check_point_grads).  At most 1 % of the points may be kinks; the rays
    that hold one are left out."""
    n = ro.shape[0]
    xr, ext = ray_points(bound, ro, rd, z)
    dr = torch.as_tensor(d_raw).detach().cpu().float().reshape(-1, 5)
    ref, o32, kp = [], [], []
    for i in range(0, xr.shape[0], batch):
        xs, ds = xr[i:i + batch], dr[i:i + batch]
        ref.append(ref_point_grad(ora, xs, ds))
        o32.append(o32_point_grad(ora, xs, ds))
        kp.append(point_kinks(ora, xs, ds)["kink"])
    ref = torch.cat(ref).reshape(n, -1, 3) / ext.double()
    o32 = torch.cat(o32).reshape(n, -1, 3) / ext.double()
    kp = torch.cat(kp)
    assert int(kp.sum()) <= max(2, int(0.01 * kp.numel())), f"{what}: {int(kp.sum())} of {kp.numel()} ray points are kinks"
    kink = kp.reshape(n, -1).any(1)
    zz = torch.as_tensor(z).detach().cpu().double()[..., None]
    for name, got, want, o in (("rays_o", got_o, ref.sum(1), o32.sum(1)), ("rays_d", got_d, (ref * zz).sum(1), (o32 * zz).sum(1))):
        got = torch.as_tensor(got).detach().cpu()
        assert rel(got, want) <= bound_l2(o, want), f"{what} {name}: rel l2 {rel(got, want):.3e}"
        check_point_grads(got, want, o, {"kink": kink, "uncert_faces": torch.zeros_like(kink)}, f"{what} {name}", budget=1.0)


def ref_point_grad(ora, x, d_raw, d_geo=None, table=None, levels=None):
    """d x of sum(raw * d_raw) + sum(geo * d_geo) by autograd of cell_field in fp64 (what naruto_query_bwd_points computes)."""
    xa = torch.as_tensor(x).detach().cpu().double().requires_grad_(True)
    raw, geo = cell_field(ora, xa, table, levels)[:2]
    loss = (raw * torch.as_tensor(d_raw).detach().cpu().double()).sum()
    if d_geo is not None:
        loss = loss + (geo * torch.as_tensor(d_geo).detach().cpu().double()).sum()
    return torch.autograd.grad(loss, xa)[0]


def o32_point_grad(ora, x, d_raw, d_geo=None):
    """The fp32 oracle's own d x (its hash cells are the kernel's: it rounds pos to fp32 once) -- the rounding yardstick."""
    xa = torch.as_tensor(x).detach().cpu().float().requires_grad_(True)
    if d_geo is None:
        loss = (ora.query_color_sdf(xa) * torch.as_tensor(d_raw).cpu().float()).sum()
    else:
        su, geo = ora.query_sdf(xa, return_geo=True, return_uncert=True)
        d_raw = torch.as_tensor(d_raw).cpu().float()
        loss = (su * d_raw[:, 3:5]).sum() + (geo * torch.as_tensor(d_geo).cpu().float()).sum()
        assert not d_raw[:, :3].any(), "query_sdf has no rgb output"
    return torch.autograd.grad(loss, xa)[0].double()          # x only: no table gradient is formed


def check_point_grads(got, ref, o32, kinks, what, budget=0.01):
    """Every point that is not a kink (point_kinks) element by element: |got - ref| <= 4 max |o32 - ref| (the oracle's own fp32
    error, the yardstick _bound uses in l2, over the points where the fp32 oracle takes the reference's pieces) + 2^-20 of the
    largest |ref| (a few roundings of the largest term).  At most ``budget`` of the points (and at least 2) may be kinks."""
    got, ref, o32 = (torch.as_tensor(t).detach().double().cpu().reshape(-1, 3) for t in (got, ref, o32))
    kink = kinks["kink"]
    n_kink = int(kink.sum())
    assert n_kink <= max(2, int(budget * kink.numel())), f"{what}: {n_kink} of {kink.numel()} points are kinks (budget {budget:g})"
    ok = ~kink
    yard = ok & ~kinks["uncert_faces"]
    scale = float(ref.abs().max())
    o_err = float((o32[yard] - ref[yard]).abs().max()) if bool(yard.any()) else 0.0
    assert_close(got[ok], ref[ok], 4.0 * o_err + 2.0 ** -20 * scale, what)

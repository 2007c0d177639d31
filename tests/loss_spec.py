"""The loss stage's fp64 twin: raw, z_vals, targets -> composite outputs, sums[0..9], losses[0..9], d_raw per loss term.

The formulas are those of oracle/spec_torch.py (raw2outputs, render_losses, total_loss) written over the 16-slot sums of
include/naruto_hip.h (the comment above k_loss_terms), so that two batches can be added as two ranks add them:

   0 sum (w rgb - w tgt)^2     1 sum_valid (D - d)^2     2 n_valid
   3 sum front (sdf - 1)^2     4 n_fs                    5 sum sdf_mask (z + sdf tr - d)^2     6 n_sdf
   7 sum_valid 1/(2(u + 1e-9)) 8 sum_valid log(u + 1e-9) 9 min u (all rays)

Every DISCRETE decision is taken once, in fp32, as the fp32 reference takes it on the same fp32 inputs (``decisions``): front / back /
sdf masks against fl(td - trunc sc) and fl(td + trunc sc), valid, the first sign change (the product sdf[s] sdf[s+1] in fp32: a
product that underflows to -0 is no change, a denormal one is), the z < limit mask.  The office config has range_d == trunc, so
samples sit on the band's edge in ordinary batches.  Everything continuous is evaluated in the dtype asked for: fp64 is the twin,
fp32 the yardstick (``o32``) the tolerances are multiples of.  A NaN measured depth is a missing measurement: 0.

d_raw comes from autograd, one call per loss slot: the weighted total is formed as the reference forms it (every slot multiplied
by its weight, a zero weight included, so that a NaN weight of an empty batch poisons what it poisons in the reference)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

TERMS = ("rgb", "depth", "sdf", "fs", "uncert")
SLOTS = (0, 1, 2, 3, 5)                    # the terms' places in losses[10] / loss_weights[10] / loss_grad[6]
REAL_SLOTS = (0, 1, 3, 5, 7, 8)
COUNT_SLOTS = (2, 4, 6)


def params_of(cfg, rgb_missing=None):
    tr = cfg["training"]
    return dict(trunc=float(tr["trunc"]), sc_factor=float(cfg["data"]["sc_factor"]), depth_trunc=float(cfg["cam"]["depth_trunc"]),
                rgb_missing=float(tr["rgb_missing"] if rgb_missing is None else rgb_missing))


def reference_weights(cfg):
    tr = cfg["training"]
    return torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.0, 0.0])


def one_hot_weights(term):
    w = torch.zeros(10)
    w[SLOTS[TERMS.index(term)]] = 1.0
    return w


def measured_depth(td):
    td = torch.as_tensor(td).detach().cpu().float().reshape(-1)
    return torch.where(torch.isnan(td), torch.zeros_like(td), td)


def decisions(raw, z, td, p):
    """The discrete decisions, in fp32 (torch's CPU float ops: correctly rounded, denormals kept)."""
    raw, z = torch.as_tensor(raw).detach().cpu().float(), torch.as_tensor(z).detach().cpu().float()
    td = measured_depth(td)
    tsc = torch.tensor(p["trunc"] * p["sc_factor"], dtype=torch.float32)
    lo, hi = (td - tsc)[:, None], (td + tsc)[:, None]
    front, back = z < lo, z > hi
    dm = td > 0.0
    sm = ~front & ~back & dm[:, None]
    valid = dm & (td < torch.tensor(p["depth_trunc"], dtype=torch.float32))
    sdf = raw[..., 3]
    change = (sdf[:, 1:] * sdf[:, :-1]) < 0.0
    if change.shape[1]:
        first = torch.argmax(change.to(torch.int8), dim=1)              # first sign change; 0 if there is none
    else:
        first = torch.zeros(z.shape[0], dtype=torch.int64)
    z_min = torch.gather(z, 1, first[:, None])
    limit = z_min + torch.tensor(p["sc_factor"] * p["trunc"], dtype=torch.float32)
    inside = z < limit
    rgb_w = valid | torch.tensor(p["rgb_missing"] != 0.0)               # rgb_missing lands in a BOOL tensor (scene_rep.py:249-250)
    return dict(front=front, back=back, sm=sm, valid=valid, first=first, any_change=change.any(1), inside=inside, rgb_w=rgb_w, td=td)


def finalize(sums, n_rays_total, S):
    """sums[>= 10] -> losses[10] in the sums' dtype: {rgb, depth, sdf, fs, psnr, uncert, min(uncert_map), n_valid, 0, 0} (differentiable)."""
    N = float(n_rays_total)
    ns = sums[4] + sums[6]
    fs_w, sdf_w = 1.0 - sums[4] / ns, 1.0 - sums[6] / ns
    rgb = sums[0] / (3.0 * N)
    depth = sums[1] / sums[2]
    fs = sums[3] / (N * S) * fs_w
    sdf = sums[5] / (N * S) * sdf_w
    psnr = -10.0 * torch.log(rgb) / torch.log(torch.tensor(10.0, dtype=sums.dtype))
    uncert = (sums[7] / sums[2]) * (sums[1] / sums[2]) + 0.5 * (sums[8] / sums[2])
    zero = torch.zeros((), dtype=sums.dtype)
    return torch.stack([rgb, depth, sdf, fs, psnr, uncert, sums[9], sums[2], zero, zero])


def total_of(losses, weights):
    """The device's total: sum_i w[i] losses[i]; a zero weight drops the slot even if it holds NaN (loss_total)."""
    t = torch.zeros((), dtype=losses.dtype)
    for i in range(9):
        if float(weights[i]) != 0.0:
            t = t + float(weights[i]) * losses[i]
    return t


def evaluate(raw, z, target_rgb, target_d, p, dtype, dec=None, n_rays_total=None, extra_sums=None, weightings=None):
    """One evaluation in ``dtype`` with the decisions ``dec``.  ``extra_sums``: another batch's sums, added as an all-reduce adds them
    (slot 9: the minimum); ``n_rays_total``: rays of all batches.  ``weightings``: {name: weights[10]} -> d_raw[name] by autograd of the
    weighted sum of the five terms; the five one-hot ones are always there under the terms' names."""
    raw32, z32 = torch.as_tensor(raw).detach().cpu().float(), torch.as_tensor(z).detach().cpu().float()
    dec = decisions(raw32, z32, target_d, p) if dec is None else dec
    N, S = z32.shape
    r = raw32.to(dtype).requires_grad_(True)
    zz = z32.to(dtype)
    td = dec["td"].to(dtype)
    tgt = torch.as_tensor(target_rgb).detach().cpu().float().to(dtype)
    trunc, tsc = p["trunc"], p["trunc"] * p["sc_factor"]
    sdf = r[..., 3]
    wb = torch.sigmoid(sdf / trunc) * torch.sigmoid(-sdf / trunc) * dec["inside"].to(dtype)
    t_eps = wb.sum(-1, keepdim=True) + 1e-8
    w = wb / t_eps
    rgb = (w[..., None] * torch.sigmoid(r[..., :3])).sum(-2)
    depth = (w * zz).sum(-1)
    acc = w.sum(-1)
    depth_var = (w * (zz - depth[:, None]) ** 2).sum(-1)
    with torch.no_grad():
        disp = 1.0 / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    um = (w * w * (F.softplus(r[..., 4]) + 0.01)).sum(-1)
    valid, fr, sm = dec["valid"], dec["front"].to(dtype), dec["sm"].to(dtype)
    wr = dec["rgb_w"].to(dtype)[:, None]
    zero = torch.zeros(N, dtype=dtype)
    e = depth - td
    u = um + 1e-9
    terms = torch.stack([((rgb * wr - tgt * wr) ** 2).sum(-1),
                         torch.where(valid, e * e, zero),
                         valid.to(dtype),
                         ((sdf * fr - fr) ** 2).sum(-1),
                         fr.sum(-1),
                         (((zz + sdf * tsc) * sm - td[:, None] * sm) ** 2).sum(-1),
                         sm.sum(-1),
                         torch.where(valid, 1.0 / (2.0 * u), zero),
                         torch.where(valid, torch.log(u), zero)], 1)                      # [N, 9]
    own = torch.cat([terms.sum(0), um.min().reshape(1), torch.zeros(6, dtype=dtype)])
    sums = own
    if extra_sums is not None:
        ex = torch.as_tensor(extra_sums).detach().to(dtype)
        lo = torch.minimum(own[9], ex[9])
        sums = torch.cat([own[:9] + ex[:9], lo.reshape(1), own[10:]])
    n_total = N if n_rays_total is None else int(n_rays_total)
    losses = finalize(sums, n_total, S)
    ws = {t: one_hot_weights(t) for t in TERMS}
    ws.update(weightings or {})
    d_raw, g_ray = {}, {}
    for name, wt in ws.items():
        obj = sum(float(wt[s]) * losses[s] for s in SLOTS)
        g = torch.autograd.grad(obj, [r, rgb, depth, um], retain_graph=True)
        d_raw[name] = g[0].detach()
        g_ray[name] = tuple(torch.nan_to_num(t.detach(), nan=0.0, posinf=0.0, neginf=0.0) for t in g[1:])      # d total / d (rgb, depth, uncert_map)
    det = lambda t: t.detach()
    cond = _conditioning(r, zz, sdf, w, rgb, depth, um, tgt, wr, td, valid, sm, e, tsc, trunc, t_eps, dec) if dtype == torch.float64 else {}
    return dict(cond=cond, g_ray=g_ray, target_rgb=tgt, rgb_w=wr, rgb=det(rgb), depth=det(depth), acc=det(acc), depth_var=det(depth_var), disp=disp, uncert_map=det(um), weights=det(w),
                terms=det(terms), sums=det(sums), own_sums=det(own), abs_sums=det(terms.abs().sum(0)), losses=det(losses), d_raw=d_raw,
                totals={k: det(total_of(losses, wt)) for k, wt in ws.items()}, dec=dec, n_rays_total=n_total, S=S, N=N)


def _conditioning(r, zz, sdf, w, rgb, depth, um, tgt, wr, td, valid, sm, e, tsc, trunc, t_eps, dec):
    """What a correctly rounded fp32 evaluation cannot deliver, to first order (u = 2^-24, gamma = (S + 8) u the dot-product bound
    of a ray's S products and the handful of roundings around them):

    * the rendered rgb, depth and uncertainty of a ray are sums of non-negative products, so each is off by up to gamma of itself;
      a DIFFERENCE formed from one -- rgb - target, depth - td, z - depth -- carries that absolute error however small it is;
    * c = (z + sdf tr) - td of the sdf term: |dc| <= u (2 |sdf tr| + |z + sdf tr| + |c|) (product, sum, difference);
      the term's own cotangent is proportional to c, so it is off by that much however small c is (``dc``, per sample).

    ``sums``: the resulting first-order error of slots 0, 1, 5 (2 |x| dx per squared difference x) and 8 (log u: gamma per ray), ADDED
    to gamma sum |summands|.  ``depth_var``: the same for sum w (z - depth)^2, per ray.  ``jac``: per ray and channel, the l2 norm
    over the samples of d(rgb_c) / d raw, d(depth) / d raw, d(uncert_map) / d raw -- a ray's d_raw is its ray-level cotangents times
    these patterns, so an absolute error of a ray-level cotangent (d_raw_slack) becomes that much of the ray's d_raw.
    ``m3``: the sdf channel's own difference.  d out / d sdf_s = (d wb_s / d sdf_s) / t (v_s - out) for out = sum_j w_j v_j (the
    normalisation's Jacobian), so on a ray whose weight sits on one or two samples v_s - out is what rounding leaves of it: per
    output the pattern (|d wb_s / d sdf_s| / t) (|v_s| + |out|) [N, S], gamma of which is the error per unit of ray-level cotangent."""
    S = zz.shape[1]
    gam = (S + 8) * U24
    with torch.no_grad():
        sums = torch.zeros(10, dtype=torch.float64)
        sums[0] = gam * (2.0 * (rgb * wr - tgt * wr).abs() * (rgb * wr).abs()).sum()
        sums[1] = gam * torch.where(valid, 2.0 * e.abs() * depth.abs(), torch.zeros_like(e)).sum()
        a = zz + sdf * tsc
        c = a * sm - td[:, None] * sm
        dc = U24 * (2.0 * (sdf * tsc).abs() + a.abs() + c.abs()) * sm                     # [N, S]: |dc| of the sdf term's difference
        sums[5] = (2.0 * c.abs() * dc).sum()
        sums[8] = gam * float(valid.sum())
        depth_var = gam * (w * 2.0 * (zz - depth[:, None]).abs()).sum(-1) * depth.abs()
        sg = torch.sigmoid(sdf / trunc)
        dwb = (sg * (1.0 - sg) * (1.0 - 2.0 * sg).abs() / trunc * dec["inside"].to(zz.dtype) / t_eps).detach()
        col = torch.sigmoid(r[..., :3]).detach()
        unc = (F.softplus(r[..., 4]) + 0.01).detach()
        m3 = {f"rgb{c}": dwb * (col[..., c] + rgb[:, c, None].abs()) for c in range(3)}
        m3["depth"] = dwb * (zz.abs() + depth[:, None].abs())
        m3["uncert_map"] = dwb * (2.0 * w * unc + 2.0 * um[:, None])
        m3 = {k: v.detach() for k, v in m3.items()}
    jac = {}
    for k, out in (("rgb0", rgb[:, 0]), ("rgb1", rgb[:, 1]), ("rgb2", rgb[:, 2]), ("depth", depth), ("uncert_map", um)):
        jac[k] = torch.autograd.grad(out.sum(), r, retain_graph=True)[0].detach().norm(dim=1)            # [N, 5]
    return dict(sums=sums, depth_var=depth_var, jac=jac, m3=m3, dc=dc.detach(), tsc=tsc)


def d_raw_slack(o, weights, name):
    """[N, 5]: per ray and channel, the absolute error of d_raw that comes from the ray-level cotangents' own conditioning
    (_conditioning): g_rgb = G 2 w^2 (rgb - tgt) / 3N, g_depth = (G_d + G_u mean_a) 2 (D - td) / n_valid and
    g_uncert = G_u (1 / 2u - mean_e / 2u^2) / n_valid are differences; each is off by gamma times the sum of the magnitudes it
    subtracts (mean_a, mean_e: by the sums' own bound), whatever is left of the difference."""
    w = torch.as_tensor(weights).double().abs()
    s, b = o["sums"].double(), sums_bound(o)
    gam = (o["S"] + 8) * U24
    nv, n_tot = s[2], float(o["n_rays_total"])
    valid = o["dec"]["valid"]
    td = o["dec"]["td"].double()
    rgb, tgt, wr, depth = o["rgb"], o["target_rgb"], o["rgb_w"], o["depth"]
    u = o["uncert_map"] + 1e-9
    zero = torch.zeros_like(depth)
    sl_rgb = gam * w[0] * 2.0 * wr * wr * (rgb.abs() + tgt.abs()) / (3.0 * n_tot)
    sl_depth = torch.where(valid, gam * (w[1] + w[5] * s[7] / nv) * 2.0 * (depth.abs() + td.abs()) / nv
                           + w[5] * (b[7] / nv) * 2.0 * (depth - td).abs() / nv, zero)
    sl_unc = torch.where(valid, gam * w[5] * (0.5 / u + (s[1] / nv) * 0.5 / (u * u)) / nv + w[5] * 0.5 / (u * u) / nv * (b[1] / nv), zero)
    jac = o["cond"]["jac"]
    out = sl_depth[:, None] * jac["depth"] + sl_unc[:, None] * jac["uncert_map"]
    for c in range(3):
        out = out + sl_rgb[:, c, None] * jac[f"rgb{c}"]
    g_rgb, g_depth, g_um = o["g_ray"][name]
    m3 = o["cond"]["m3"]
    pat = g_depth.abs()[:, None] * m3["depth"] + g_um.abs()[:, None] * m3["uncert_map"]
    for c in range(3):
        pat = pat + g_rgb[:, c].abs()[:, None] * m3[f"rgb{c}"]
    # the sdf term's direct cotangent G_sdf sdf_w 2 / (N S) tr c_s: c_s = (z + sdf tr) - td is off by dc_s however small it is
    c_sdf = w[2] * (1.0 - s[6] / (s[4] + s[6])).abs() * 2.0 / (n_tot * o["S"]) * o["cond"]["tsc"]
    out[:, 3] = out[:, 3] + gam * pat.norm(dim=1) + torch.nan_to_num(c_sdf * o["cond"]["dc"]).norm(dim=1)
    return torch.nan_to_num(out, nan=0.0, posinf=0.0, neginf=0.0)


def twin(raw, z, target_rgb, target_d, p, **kw):
    """The fp64 evaluation, with the fp32 one of the same formulas and decisions under ``o32``."""
    dec = decisions(raw, z, target_d, p)
    o64 = evaluate(raw, z, target_rgb, target_d, p, torch.float64, dec, **kw)
    o64["o32"] = evaluate(raw, z, target_rgb, target_d, p, torch.float32, dec, **kw)
    return o64


# ---- tolerances --------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24


def sums_bound(o64):
    """Real slots: (S + 8) 2^-24 sum |summands| -- the fp32 dot-product bound on a per-ray term of S products plus the handful of
    roundings around it; the fp64 accumulation over rays adds nothing visible -- plus the summands' own conditioning where a summand
    is the square of a difference (_conditioning: slots 0, 1, 5; slot 8's summand is a logarithm).  Counts: 0.  Slot 9: see check_sums."""
    a = o64["abs_sums"].double()
    b = torch.zeros(10, dtype=torch.float64)
    for k in REAL_SLOTS:
        b[k] = (o64["S"] + 8) * U24 * a[k] + o64["cond"]["sums"][k]
    return b


def losses_bound(o64, b_sums):
    """The sums' bound through finalize: sum_k |d loss_i / d sums_k| bound_k (the twin's own Jacobian) plus the finalize's own fp32
    arithmetic: at most 8 roundings per loss, each 2^-24 of the largest intermediate (for uncert_loss the two terms it adds)."""
    s = o64["sums"].double().clone().requires_grad_(True)
    l = finalize(s, o64["n_rays_total"], o64["S"])
    out = torch.zeros(10, dtype=torch.float64)
    sd = s.detach()
    for i in (0, 1, 2, 3, 4, 5):
        if bool(torch.isnan(l[i])):
            out[i] = float("nan")
            continue
        g = torch.autograd.grad(l[i], s, retain_graph=True)[0]
        g = torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0)
        mag = float(l[i].detach().abs())
        if i == 5:
            mag = float(((sd[7] / sd[2]) * (sd[1] / sd[2])).abs() + (0.5 * sd[8] / sd[2]).abs())
        if i == 4:
            mag = mag + 10.0 / 2.302585092994046               # psnr: a rounding of log(rgb_loss) is absolute
        out[i] = float((g.abs()[:10] * b_sums).sum()) + 8 * U24 * mag
    return out


def report(lines):
    path = os.environ.get("NARUTO_LOSS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


# ---- hand-made batches ---------------------------------------------------------------------------------------------------
FAR = 5.0


def _ray_sdf(z, surface, rs):
    """A plausible sdf along a ray: positive in front of ``surface``, one sign change there, a little noise that adds none."""
    s = np.clip(surface - z, -1.0, 1.0) * 0.6
    return (s + np.sign(s + 1e-30) * 0.02 * rs.uniform(0.0, 1.0, z.shape)).astype(np.float32)


def ordinary_batch(N, S, seed, zero_depth_frac=0.1):
    """An ordinary batch on hand-made raw / z_vals: depths in [0.5, 2.5] (a tenth missing), S sorted samples in [0, FAR) of which up
    to 11 lie within the +-0.1 band around the depth, an sdf that changes sign once near the depth, random colours / uncertainties."""
    rs = np.random.RandomState(seed)
    td = rs.uniform(0.5, 2.5, N).astype(np.float32)
    td[rs.uniform(0, 1, N) < zero_depth_frac] = 0.0
    surface = np.where(td > 0, td, np.float32(1.5)).astype(np.float32)
    k = min(11, S // 3)
    z = np.concatenate([rs.uniform(0.0, FAR, (N, S - k)), surface[:, None] + rs.uniform(-0.1, 0.1, (N, k))], 1).astype(np.float32)
    z = np.sort(z, 1)
    raw = np.zeros((N, S, 5), np.float32)
    raw[..., :3] = rs.normal(0, 1.0, (N, S, 3))
    raw[..., 3] = _ray_sdf(z, surface[:, None], rs)
    raw[..., 4] = rs.normal(0, 2.0, (N, S))
    tgt = rs.uniform(0, 1, (N, 3)).astype(np.float32)
    return dict(raw=torch.from_numpy(raw), z=torch.from_numpy(z), target_rgb=torch.from_numpy(tgt), target_d=torch.from_numpy(td))


def _signs(S, neg_from, mag=0.05):
    """sdf +mag on samples < neg_from, -mag from there on."""
    s = np.full(S, mag, np.float32)
    s[neg_from:] = -mag
    return s


def edge_rays(S, p):
    """The edge rays that fit S samples: name -> a function (batch, n) that rewrites ray n of an ordinary batch in place."""
    f32 = np.float32
    edges = {}

    def sdf_edge(name, values):
        def put(b, n, v=values):
            b["raw"][n, :, 3] = torch.from_numpy(np.asarray(v, f32))
            b["target_d"][n] = 1.5
        edges[name] = put

    for pair in sorted({0, 62, 63, 64, S - 2}):
        if 0 <= pair and pair + 1 < S:
            sdf_edge(f"change_at_{pair}", _signs(S, pair + 1))
    sdf_edge("no_change", _signs(S, S))
    if S >= 12:
        v = _signs(S, 4)
        v[11:] = 0.05
        sdf_edge("two_changes_first_wins", v)
        v = _signs(S, 6)
        v[5] = 0.0
        sdf_edge("zero_next_to_negative", v)                  # 0 * -0.05 = -0: not < 0
        # (4, 5) = 0.05 tiny > 0 and (6, 7) = tiny 0.05 > 0: the only candidate is (5, 6) = -tiny^2: -1e-46 -> -0, -1e-40 a denormal
        for name, tiny in (("product_underflows_to_minus_zero", 1e-23), ("product_is_a_denormal", 1e-20)):
            v = _signs(S, 6)
            v[5], v[6] = tiny, -tiny
            sdf_edge(name, v)
    if S >= 16:
        def band(b, n):
            td = f32(1.5)
            tsc = f32(p["trunc"] * p["sc_factor"])
            lo, hi = f32(td - tsc), f32(td + tsc)
            z = b["z"][n].numpy().copy()
            z[:6] = [np.nextafter(lo, f32(0)), lo, np.nextafter(lo, f32(9)), np.nextafter(hi, f32(0)), hi, np.nextafter(hi, f32(9))]
            z = np.sort(z)
            b["z"][n] = torch.from_numpy(z)
            b["raw"][n, :, 3] = torch.from_numpy(_ray_sdf(z, td, np.random.RandomState(5)))
            b["target_d"][n] = float(td)
        edges["z_on_the_band_edges"] = band
    for name, td in (("td_0", 0.0), ("td_minus_1", -1.0), ("td_nan", float("nan")), ("td_depth_trunc", p["depth_trunc"]),
                     ("td_below_depth_trunc", float(np.nextafter(f32(p["depth_trunc"]), f32(0)))), ("td_150", 150.0)):
        def put_td(b, n, td=td):
            b["target_d"][n] = td
        edges[name] = put_td
    for name, q in (("sdf_over_trunc_plus_200", 200.0), ("sdf_over_trunc_minus_200", -200.0)):
        def put_far(b, n, q=q):
            b["raw"][n, :, 3] = q * p["trunc"]
            b["target_d"][n] = 1.5
        edges[name] = put_far

    def put_uncert(b, n):
        b["raw"][n, :, 4] = torch.tensor([-100.0, 19.9, 20.1, 60.0]).repeat(S // 4 + 1)[:S]
    edges["uncert_logits"] = put_uncert

    def put_colour(b, n):
        b["raw"][n, :, :3] = torch.tensor([100.0, -100.0]).repeat(S // 2 + 1)[:S, None]
    edges["colour_logits"] = put_colour
    return edges


def edge_batch(N, S, seed, p):
    """An ordinary batch with one ray per edge embedded (as many edges as there are rays to spare: every other ray, from ray 1).
    Returns the batch and {edge name: ray}."""
    b = ordinary_batch(N, S, seed)
    where = {}
    free = list(range(1, N, 2)) + list(range(0, N, 2))
    for (name, put), n in zip(edge_rays(S, p).items(), free):
        put(b, n)
        where[name] = n
    return b, where


def degenerate_batch(kind, N, S, seed, p):
    """no_valid_depth: every depth beyond depth_trunc (all samples in front: n_fs > 0, depth and uncert losses NaN);
    no_samples: every depth missing (n_fs + n_sdf = 0: the fs / sdf weights are NaN)."""
    b = ordinary_batch(N, S, seed)
    b["target_d"][:] = 150.0 if kind == "no_valid_depth" else 0.0
    return b


def per_ray_error(got, o32, o64, slack=None):
    """Rows are rays.  A ray passes when |got - o64| <= bound max(|o64|, 1e-6 of the batch's largest |o64|) + slack (l2 over the
    ray): bound = helpers.bound(o32, o64) over the whole case (4 x the fp32 reference's own relative l2 distance from fp64, floor
    2e-5), slack [rays] the ray's own conditioning (0 if None).  Returns (worst relative error of a ray in that measure without the
    slack, bound, worst |got - o64| / tolerance)."""
    import helpers as H
    n = o64.shape[0]
    g, a, b = (torch.nan_to_num(torch.as_tensor(t).detach().cpu().double().reshape(n, -1)) for t in (got, o32, o64))
    bound = H.bound(a, b)
    nrm = b.norm(dim=1)
    scale = float(nrm.max())
    err = (g - b).norm(dim=1)
    sl = torch.zeros(n, dtype=torch.float64) if slack is None else torch.as_tensor(slack).double().reshape(n)
    if scale == 0.0:
        ok = bool((err <= sl).all())
        return float(err.max()), bound, (0.0 if ok else float("inf"))
    den = torch.clamp(nrm, min=1e-6 * scale)
    return float((err / den).max()), bound, float((err / (bound * den + sl)).max())


# ---- a device result against the twin (CPU tensors in, report lines out; every line is `case what bound observed ratio`) ----
def _line(case, what, bound, seen):
    ratio = seen / bound if bound > 0 else (0.0 if seen == 0 else float("inf"))
    return f"{case} {what} bound {bound:.3e} observed {seen:.3e} ratio {ratio:.3f}", ratio


def _nan_equal(a, b):
    return torch.equal(torch.isnan(torch.as_tensor(a)), torch.isnan(torch.as_tensor(b)))


def check_outputs(case, got, o, lines, keys=("rgb", "depth", "uncert_map")):
    """Composite outputs, per ray.  Where a NaN appears is a discrete matter (0 / 0 on a ray without weight): the fp32 reference's."""
    bad = []
    for k in keys:
        g = torch.as_tensor(got[k]).detach().cpu()
        if not _nan_equal(g, o["o32"][k]):
            bad.append(f"{case} {k}: NaN pattern differs from the fp32 reference's")
            continue
        nan = torch.isnan(o["o32"][k])
        ref = torch.where(nan, torch.zeros_like(o[k]), o[k])
        seen, bound, ratio = per_ray_error(g, o["o32"][k], ref, o["cond"].get(k))
        ln = f"{case} {k} bound {bound:.3e} observed {seen:.3e} ratio {ratio:.3f}"
        lines.append(ln)
        if not ratio <= 1.0:
            bad.append(ln)
    return bad


def check_sums(case, got_sums, got_uncert_map, o, lines):
    """This batch's sums against the twin's (``own_sums``).  Slot 9 is the minimum of the fp32 map the device itself rendered, so it
    is compared with that map's minimum (it must be THE minimum: no ulp to spare); the map is pinned to the twin by check_outputs."""
    bad = []
    s = torch.as_tensor(got_sums).detach().cpu().double()
    b = sums_bound(o)
    for k in COUNT_SLOTS:
        if float(s[k]) != float(o["own_sums"][k]):
            bad.append(f"{case} sums[{k}]: {float(s[k])} against the count {float(o['own_sums'][k])}")
    for k in REAL_SLOTS:
        ln, ratio = _line(case, f"sums[{k}]", float(b[k]), float((s[k] - o["own_sums"][k]).abs()))
        lines.append(ln)
        if not ratio <= 1.0:
            bad.append(ln)
    um = torch.as_tensor(got_uncert_map).detach().cpu()
    want = float("nan") if bool(torch.isnan(um).any()) else float(um.min())
    if not (float(s[9]) == want or (want != want and float(s[9]) != float(s[9]))):
        bad.append(f"{case} sums[9]: {float(s[9])!r} is not the minimum {want!r} of the rendered uncertainty map")
    return bad


def check_losses(case, got_losses, got_sums, o, lines, weights=None):
    """losses[0..5] within the sums' bound taken through the twin's finalize; [6] and [7] are copies of sums [9] and [2]; the total
    (with weights, losses[9]) within sum |w_i| bound_i plus its own handful of roundings."""
    bad = []
    l = torch.as_tensor(got_losses).detach().cpu().double()
    s = torch.as_tensor(got_sums).detach().cpu().double()
    b = losses_bound(o, sums_bound(o))
    ref = o["losses"]
    if not _nan_equal(l[:6], ref[:6]):
        return [f"{case} losses: NaN pattern {torch.isnan(l[:6]).tolist()} against the twin's {torch.isnan(ref[:6]).tolist()}"]
    for i in range(6):
        if bool(torch.isnan(ref[i])):
            continue
        ln, ratio = _line(case, f"losses[{i}]", float(b[i]), float((l[i] - ref[i]).abs()))
        lines.append(ln)
        if not ratio <= 1.0:
            bad.append(ln)
    if not (float(l[6]) == float(s[9].float()) or (float(l[6]) != float(l[6]) and float(s[9]) != float(s[9]))):
        bad.append(f"{case} losses[6] = {float(l[6])!r}, sums[9] = {float(s[9])!r}")
    if float(l[7]) != float(s[2]):
        bad.append(f"{case} losses[7] = {float(l[7])}, sums[2] = {float(s[2])}")
    if weights is not None:
        w = torch.as_tensor(weights).double()
        used = [i for i in SLOTS if float(w[i]) != 0.0]
        want = sum(float(w[i]) * ref[i] for i in used)
        if bool(torch.isnan(torch.as_tensor(want))) != bool(torch.isnan(l[9])):
            bad.append(f"{case} total: {float(l[9])!r} against {float(want)!r}")
        elif not bool(torch.isnan(l[9])):
            bound = sum(abs(float(w[i])) * float(b[i]) for i in used) + 8 * U24 * sum(abs(float(w[i]) * float(ref[i])) for i in used)
            ln, ratio = _line(case, "total", bound, abs(float(l[9]) - float(want)))
            lines.append(ln)
            if not ratio <= 1.0:
                bad.append(ln)
    return bad


def check_d_raw(case, got, o, name, lines, weights):
    """d_raw of the weighting ``name`` (``weights`` [10]) per channel and per ray; NaNs where the twin (and the fp32 reference) has them."""
    bad = []
    slack = d_raw_slack(o, weights, name)
    g = torch.as_tensor(got).detach().cpu()
    ref, r32 = o["d_raw"][name], o["o32"]["d_raw"][name]
    for ch in range(5):
        if not _nan_equal(g[..., ch], ref[..., ch]):
            bad.append(f"{case} d_raw[{name}] channel {ch}: NaN pattern differs from the twin's")
            continue
        seen, bound, ratio = per_ray_error(g[..., ch], r32[..., ch], ref[..., ch], slack[:, ch])
        ln = f"{case} d_raw[{name}][{ch}] bound {bound:.3e} observed {seen:.3e} ratio {ratio:.3f}"
        lines.append(ln)
        if not ratio <= 1.0:
            bad.append(ln)
    return bad


def check_list(case, d_raw, ray_count, ray_offset, n_active, active_idx, o, ordinary, predicted):
    """The active-prefix contract, exactly.  ``ordinary``: the case is no degenerate one -- then at least half of its rays must have
    a list shorter than the ray, or the prefix property would be vacuous.  ``predicted``: the counts are the forward's, taken from the
    masks before any cotangent exists (k_loss_bwd_fused's lists) -- they must reach the last front / sdf-band sample whatever the
    weights; the counts the composite backward writes itself are 1 + the last non-zero cotangent, which a zero weight shortens."""
    N, S = o["N"], o["S"]
    cnt = torch.as_tensor(ray_count).detach().cpu().long().reshape(-1)
    off = torch.as_tensor(ray_offset).detach().cpu().long().reshape(-1)
    d = torch.as_tensor(d_raw).detach().cpu().reshape(N, S, 5)
    bad = []
    if not bool((cnt <= S).all()) or not bool((cnt >= 0).all()):
        return [f"{case} ray_count outside [0, S]: max {int(cnt.max())}"]
    s_idx = torch.arange(S)[None, :]
    nz = ((d != 0) | torch.isnan(d)).any(-1)
    if bool((nz & (s_idx >= cnt[:, None])).any()):
        n = int((nz & (s_idx >= cnt[:, None])).any(1).nonzero()[0])
        bad.append(f"{case} ray {n}: a non-zero cotangent at or beyond ray_count = {int(cnt[n])}: gradient dropped")
    need = (o["dec"]["front"] | o["dec"]["sm"])
    last = torch.where(need.any(1), S - torch.argmax(need.flip(1).to(torch.int8), dim=1), torch.zeros(N, dtype=torch.long))
    if predicted and bool((cnt < last).any()):
        n = int((cnt < last).nonzero()[0])
        bad.append(f"{case} ray {n}: ray_count {int(cnt[n])} < 1 + the last front / sdf-band sample ({int(last[n])})")
    if not torch.equal(off, torch.cumsum(cnt, 0) - cnt):
        bad.append(f"{case} ray_offset is not the exclusive prefix sum of ray_count")
    total = int(cnt.sum())
    if int(torch.as_tensor(n_active).reshape(-1)[0]) != total:
        bad.append(f"{case} n_active = {int(torch.as_tensor(n_active).reshape(-1)[0])}, the counts add up to {total}")
    want = torch.cat([n * S + torch.arange(int(c)) for n, c in enumerate(cnt.tolist())]) if total else torch.zeros(0, dtype=torch.long)
    if not torch.equal(torch.as_tensor(active_idx).detach().cpu().long().reshape(-1)[:total], want):
        bad.append(f"{case} active_idx[:n_active] is not n S + arange(count[n]) in ray order")
    if ordinary and not int((cnt < S).sum()) * 2 >= N:
        bad.append(f"{case} only {int((cnt < S).sum())} of {N} rays have a list shorter than the ray: the prefix check is vacuous")
    return bad

"""numpy twin of naruto_amd/render.py's contract: the ray rule, the crossing rule and the three image metrics, in the operation orders
the module docstring states.  float32 where the contract says float32 (every operation rounded once), float64 for the metrics."""
import math

import numpy as np

F = np.float32
C1, C2 = 0.01 * 0.01, 0.03 * 0.03
WIN = 11


def camera_dirs(H, W, fx, fy, cx, cy):
    """[H,W,3] float32: ((i - cx)/fx, -(j - cy)/fy, -1)."""
    i = np.arange(W, dtype=F)[None, :].repeat(H, 0)
    j = np.arange(H, dtype=F)[:, None].repeat(W, 1)
    return np.stack([(i - F(cx)) / F(fx), -((j - F(cy)) / F(fy)), -np.ones((H, W), F)], -1)


def view_rays(c2ws, cam, p0, p1):
    """(rays_o, rays_d) float32 [p1 - p0, 3] of the flat pixels [p0, p1): the direction rotated as naruto_rays_to_world does it."""
    c2ws = np.asarray(c2ws, F).reshape(-1, 4, 4)
    H, W = cam["H"], cam["W"]
    dirs = camera_dirs(H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"]).reshape(-1, 3)
    g = np.arange(p0, p1)
    pose, pix = g // (H * W), g % (H * W)
    P, d = c2ws[pose], dirs[pix]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    # naruto_rays_to_world's arithmetic: one product rounded on its own (dx P0 in row 0, dy P1 in rows 1 and 2), the other two fused into the sum
    rays_d = np.stack([fma32(dz, P[:, 0, 2], fma32(dy, P[:, 0, 1], dx * P[:, 0, 0])),
                       fma32(dz, P[:, 1, 2], fma32(dx, P[:, 1, 0], dy * P[:, 1, 1])),
                       fma32(dz, P[:, 2, 2], fma32(dx, P[:, 2, 0], dy * P[:, 2, 1]))], -1)
    return P[:, :3, 3].copy(), rays_d


def fma32(a, b, c):
    """float32 a * b + c rounded once: the product of two float32 is exact in float64; the float64 sum is rounded to odd (its last bit set
    when the sum was inexact), which makes the final rounding to float32 the correct one."""
    p, c = np.asarray(a, np.float64) * np.asarray(b, np.float64), np.asarray(c, np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                                     # TwoSum: p + c = s + e exactly
    odd = (s.view(np.int64) & 1) == 1
    s = np.where((e == 0) | odd, s, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)))       # inexact and even: the odd neighbour on the true sum's side
    return s.astype(F)


def crossing(sdf, z):
    """z* [N] float32: the first k with sdf[k] > 0 and not (sdf[k+1] > 0); z[k] + (z[k+1] - z[k]) * (sdf[k] / (sdf[k] - sdf[k+1])); else 0.
    Also returns the index k (-1: none)."""
    sdf, z = np.asarray(sdf, F), np.asarray(z, F)
    out, idx = np.zeros(len(sdf), F), np.full(len(sdf), -1, np.int64)
    with np.errstate(all="ignore"):
        for n in range(len(sdf)):
            s = sdf[n]
            hit = np.flatnonzero((s[:-1] > 0) & ~(s[1:] > 0))
            if len(hit):
                k = int(hit[0])
                idx[n] = k
                out[n] = z[n, k] + (z[n, k + 1] - z[n, k]) * (s[k] / (s[k] - s[k + 1]))
    return out, idx


def gaussian_window():
    x = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2.0
    w = np.exp(-(x * x) / (2.0 * 1.5 * 1.5))
    return w / w.sum()


def _filter(q, w):
    """Separable, valid positions only: horizontal pass first, taps ascending, every accumulation from 0.0.  q [H,W] float64."""
    H, W = q.shape
    h = np.zeros((H, W - WIN + 1))
    for t in range(WIN):
        h = h + w[t] * q[:, t:t + W - WIN + 1]
    v = np.zeros((H - WIN + 1, W - WIN + 1))
    for t in range(WIN):
        v = v + w[t] * h[t:t + H - WIN + 1]
    return v


def ssim_map(x, y):
    """x, y [H,W,3] float32 -> float64 [H-10,W-10,3] (empty when H or W is below 11)."""
    H, W = x.shape[:2]
    if H < WIN or W < WIN:
        return np.zeros((max(H - WIN + 1, 0), max(W - WIN + 1, 0), 3))
    w = gaussian_window()
    out = []
    for c in range(3):
        a, b = x[..., c].astype(np.float64), y[..., c].astype(np.float64)
        mx, my, xx, yy, xy = (_filter(q, w) for q in (a, b, a * a, b * b, a * b))
        sx, sy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
        out.append(((2.0 * mx * my + C1) * (2.0 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2)))
    return np.stack(out, -1)


def metrics(rgb, depth, gt_rgb, gt_depth, depth_trunc=None):
    """One view -> the per-pixel maps, the six sums (math.fsum: the exactly rounded sum), the sums of |term| and the three scores."""
    rgb, gt_rgb, depth, gt_depth = (np.asarray(t, F) for t in (rgb, gt_rgb, depth, gt_depth))
    H, W = depth.shape
    e = rgb.astype(np.float64) - gt_rgb.astype(np.float64)
    se = e * e
    valid = gt_depth > 0
    if depth_trunc is not None:
        valid &= gt_depth <= F(depth_trunc)
    de = np.where(valid, np.abs(depth.astype(np.float64) - gt_depth.astype(np.float64)), 0.0)
    sm = ssim_map(rgb, gt_rgb)
    sums = np.array([math.fsum(se.ravel()), float(H * W), math.fsum(de.ravel()), float(valid.sum()), math.fsum(sm.ravel()), float(sm.size)])
    with np.errstate(all="ignore"):
        mse = sums[0] / (3.0 * sums[1])
        scores = {"psnr": float(-10.0 * np.log10(mse)), "ssim": float(np.float64(sums[4]) / np.float64(sums[5])),
                  "depth_l1_cm": float(np.float64(sums[2]) / np.float64(sums[3]) * 100.0)}
    return {"se_map": se, "depth_err_map": de, "ssim_map": sm, "sums": sums, "abs_sums": np.array([sums[0], sums[1], sums[2], sums[3], math.fsum(np.abs(sm).ravel()), sums[5]]),
            "n_terms": np.array([se.size, 1, de.size, 1, sm.size, 1]), **scores}

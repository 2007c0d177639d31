"""numpy restatement of the reconstruction-metric chain (naruto_amd/evaluation.py, csrc/naruto_recon.hip): test infrastructure only.
Written from the published algorithms (trimesh's area-weighted surface sampling rule, Euclidean nearest neighbour, the
Accuracy / Completion / Completion-ratio definitions), not from any implementation of them."""
import numpy as np

_U = np.uint64


def splitmix64(x):
    """naruto_common.h's splitmix64 on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=_U) + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def uniforms(seed, count):
    """float64 [count,3] in [0,1): draw d of sample s = top 53 bits of splitmix64(splitmix64(seed) + 3*s + d)."""
    key = splitmix64(np.array([seed & (2 ** 64 - 1)], dtype=_U))[0]
    with np.errstate(over="ignore"):
        ctr = key + np.arange(3 * count, dtype=_U)
    return ((splitmix64(ctr) >> _U(11)).astype(np.float64) * 2.0 ** -53).reshape(count, 3)


def face_areas(vertices, faces):
    """0.5 * |e1 x e2| in float64 with the device's operation order."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


def sample_surface(vertices, faces, cumulative, count, seed):
    """(points float32 [count,3], face index [count]) given the cumulative face areas (float64 [F])."""
    v = np.asarray(vertices, dtype=np.float64)
    u = uniforms(seed, count)
    face = np.searchsorted(cumulative, u[:, 0] * cumulative[-1], side="left")
    u1, u2 = u[:, 1].copy(), u[:, 2].copy()
    flip = u1 + u2 > 1.0
    u1[flip], u2[flip] = np.abs(u1[flip] - 1.0), np.abs(u2[flip] - 1.0)
    a, b, c = v[faces[face, 0]], v[faces[face, 1]], v[faces[face, 2]]
    p = a + ((b - a) * u1[:, None] + (c - a) * u2[:, None])
    return p.astype(np.float32), face.astype(np.int32)


def nearest(query, target, chunk=512):
    """Brute force in float64: d2 = (dx*dx + dy*dy) + dz*dz on the widened float32 coordinates, minimum on d2 (the FIRST minimum: the
    lowest index among equal distances), one sqrt at the end.  -> (dist float64 [N], index int32 [N])."""
    q = np.asarray(query, dtype=np.float32).astype(np.float64)
    t = np.asarray(target, dtype=np.float32).astype(np.float64)
    dist = np.empty(len(q), dtype=np.float64)
    index = np.empty(len(q), dtype=np.int32)
    for s in range(0, len(q), chunk):
        dx = q[s:s + chunk, None, 0] - t[None, :, 0]
        dy = q[s:s + chunk, None, 1] - t[None, :, 1]
        dz = q[s:s + chunk, None, 2] - t[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        i = np.argmin(d2, axis=1)
        index[s:s + chunk] = i
        dist[s:s + chunk] = np.sqrt(d2[np.arange(len(i)), i])
    return dist, index


def metrics(dist_rec_to_gt, dist_gt_to_rec, threshold=0.05):
    return {"accuracy_cm": float(np.mean(dist_rec_to_gt)) * 100.0, "completion_cm": float(np.mean(dist_gt_to_rec)) * 100.0,
            "completion_ratio_pct": float(np.count_nonzero(dist_gt_to_rec < threshold)) / len(dist_gt_to_rec) * 100.0}

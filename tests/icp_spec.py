"""numpy + scipy.spatial.cKDTree twin of the rigid-alignment contract (naruto_amd/evaluation.py ``icp``, csrc/naruto_icp.hip): test
infrastructure only.  Written from the published algorithm (point-to-point ICP as Open3D's registration_icp runs it with its defaults;
Horn / Kabsch with the determinant correction, the formula of ``evaluation.ate``), not from any implementation of it."""
import numpy as np

RANK_RATIO = 1e-10


def transform(points, T):
    """float32 [N,3] -> float32 [N,3]: fp64 arithmetic in the device's order ((r0*x + r1*y) + r2*z) + t, rounded once."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], 1)
    return out.astype(np.float32)


def kabsch(p, q):
    """The rigid dT [4,4] with q ~ dT p, or None where the rotation is not determined (fewer than 3 pairs, or the second singular
    value of the cross-covariance <= 1e-10 x the first).  fp64, centroids removed first."""
    p, q = np.asarray(p, dtype=np.float64).reshape(-1, 3), np.asarray(q, dtype=np.float64).reshape(-1, 3)
    if len(p) < 3:
        return None
    cp, cq = p.mean(0), q.mean(0)
    U, S, Vt = np.linalg.svd((p - cp).T @ (q - cq))
    if not (S[0] > 0.0 and S[1] > RANK_RATIO * S[0]):
        return None
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(Vt.T @ U.T))) or 1.0])
    R = Vt.T @ D @ U.T
    dT = np.eye(4)
    dT[:3, :3], dT[:3, 3] = R, cq - R @ cp
    return dT


def sums(p, q, d, origin=(0.0, 0.0, 0.0)):
    """The 17 sums of naruto_icp_accumulate over pairs that are ALL inliers, as float64 (numpy's summation order)."""
    o = np.asarray(origin, dtype=np.float64)
    p, q = np.asarray(p, dtype=np.float64) - o, np.asarray(q, dtype=np.float64) - o
    d = np.asarray(d, dtype=np.float64)
    return np.concatenate([[float(len(p)), (d * d).sum()], p.sum(0), q.sum(0), (p[:, :, None] * q[:, None, :]).sum(0).reshape(9)])


def evaluate(moved, tree, max_distance):
    """-> (fitness, inlier_rmse, inlier mask, nearest index) of the float32 cloud ``moved`` against the tree's cloud."""
    d, i = tree.query(moved)
    inl = d <= max_distance
    k = int(inl.sum())
    return k / len(moved), (float(np.sqrt((d[inl] * d[inl]).sum() / k)) if k else 0.0), inl, i


def icp(source, target, max_correspondence_distance=0.1, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, init=None):
    """The loop of the contract.  -> dict(transformation, fitness, inlier_rmse, iterations, converged, status, history)."""
    from scipy.spatial import cKDTree
    src = np.asarray(source, dtype=np.float32).reshape(-1, 3)
    tgt = np.asarray(target, dtype=np.float32).reshape(-1, 3)
    tree = cKDTree(tgt)
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).reshape(4, 4).copy()
    moved = transform(src, T)
    fitness, rmse, inl, idx = evaluate(moved, tree, max_correspondence_distance)
    history, status, it = [(fitness, rmse)], "max_iteration", 0
    while it < max_iteration:
        dT = kabsch(moved[inl], tgt[idx[inl]])
        if dT is None:
            status = "degenerate"
            break
        T = dT @ T
        it += 1
        moved = transform(src, T)
        prev = (fitness, rmse)
        fitness, rmse, inl, idx = evaluate(moved, tree, max_correspondence_distance)
        history.append((fitness, rmse))
        if abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            status = "converged"
            break
    return {"transformation": T, "fitness": fitness, "inlier_rmse": rmse, "iterations": it, "converged": status == "converged", "status": status,
            "history": history}


AXIS = np.array([0.3, -0.5, 0.8])


def rigid(angle_deg, t, centre, axis=AXIS):
    """[4,4]: the rotation by ``angle_deg`` about ``axis`` through ``centre``, then the translation (t, -0.7 t, 0.5 t)."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(angle_deg)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
    c = np.asarray(centre, dtype=np.float64)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, c - R @ c + np.array([t, -0.7 * t, 0.5 * t])
    return M

"""Time the planner's device pieces on an MI355X and write profiles/time_planner.json.

    python tools/time_planner.py [--out profiles/time_planner.json] [--repeats 200]

At the office_0 size (goal space 25 x 28 x 3 = 2100 candidates, 300 targets, obs_per_goal 10):
  * goal_search_ms           naruto_goal_search including its one read-back (naruto_amd.planner.goal_search)
  * goal_search_reference_ms the reference's expression (naruto_planner.py:478-507) on the same aggregator outputs: the [G] volume to
                             the host, np.argpartition, torch.topk on the winning row, the gather, one host conversion per target
  * planning_step_ms         one whole uncertainty_aware_planning_v2 in a mapped room, the goal reachable by run()
  * planning_step_traversability_ms   the same with an uncertainty volume none of whose targets can be seen at first, so that
                             compute_traversability_mask (run_full + get_reachable_mask) and a second aggregation run
Host timers around synchronised calls (every piece ends in a read-back), the median of --repeats after a warm-up; no target is fixed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (49, 56, 35)                       # office_0 at 0.1 m
BBOX = [[0.0, 4.8], [0.0, 5.5], [0.0, 3.4]]


def median_ms(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - a) * 1e3)
    return float(np.median(t)), float(np.min(t))


def room():
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in DIMS), indexing="ij")
    sdf = np.minimum.reduce([x - 1, DIMS[0] - 2 - x, y - 1, DIMS[1] - 2 - y, z - 1, DIMS[2] - 2 - z])
    pillar = np.sqrt((x - 24.0) ** 2 + (y - 28.0) ** 2) - 3.0
    return np.minimum(sdf, pillar).astype(np.float32)


def reference_goal_search(out, gs_shape, ranges, obs_per_goal, bbox_min, voxel):
    agg = out["gs_aggre_uncerts"].cpu().numpy()
    best = np.unravel_index(np.argpartition(agg, -1, axis=None)[-1], agg.shape)
    goal = np.array([ranges[0][best[0]], ranges[1][best[1]], ranges[2][best[2]]])
    row = out["gs_uncert_collections"].reshape(*gs_shape, -1)[best]
    vals, idx = row.topk(k=obs_per_goal, largest=True)
    idx = idx[:max((vals > 0).sum(), 1)]
    vxl = out["topk_uncert_vxl"][idx].cpu().numpy()
    return goal, [v * voxel + bbox_min for v in vxl]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_planner.json"))
    ap.add_argument("--repeats", type=int, default=200)
    a = ap.parse_args()
    from naruto_amd import planner as P
    dev = torch.device("cuda")
    rs = np.random.RandomState(0)
    sdf = room()
    uncert = (rs.randint(1, 512, size=DIMS) / 64.0 * ((sdf >= 0) & (sdf < 1.5))).astype(np.float32)
    p = P.NarutoPlannerHIP(dataset="Replica", device=dev, gs_z_levels=[5, 11, 17], rrt_max_iter=2000)
    p.init_data(BBOX)
    p.init_local_planner()
    p.update_step(1)
    p.traversability_mask = np.ones(DIMS, dtype=np.float32)
    u_dev, s_dev = torch.from_numpy(uncert).to(dev), torch.from_numpy(sdf).to(dev)
    agg = p._aggregator()
    ok, out = agg.uncertainty_aggregation_v2([u_dev, s_dev])
    assert ok
    G, K = agg._goal_idx.shape[0], out["topk_uncert_vxl"].shape[0]
    tgt32 = out["topk_uncert_vxl"].to(torch.int32).contiguous()
    flat = out["gs_aggre_uncerts"].reshape(-1)
    res = {"device": torch.cuda.get_device_name(0), "G": G, "K": K, "obs_per_goal": 10, "repeats": a.repeats}
    res["goal_search_ms"], res["goal_search_min_ms"] = median_ms(
        lambda: P.goal_search(flat, out["gs_uncert_collections"], tgt32, agg._goal_idx, 10, p.bbox[:, 0], p.voxel_size), a.repeats)
    gs_shape = tuple(out["gs_aggre_uncerts"].shape)
    ranges = (agg.gs_x_range, agg.gs_y_range, agg.gs_z_range)
    res["goal_search_reference_ms"], res["goal_search_reference_min_ms"] = median_ms(
        lambda: reference_goal_search(out, gs_shape, ranges, 10, p.bbox[:, 0], p.voxel_size), a.repeats)
    mine = P.goal_search(flat, out["gs_uncert_collections"], tgt32, agg._goal_idx, 10, p.bbox[:, 0], p.voxel_size)
    theirs = reference_goal_search(out, gs_shape, ranges, 10, p.bbox[:, 0], p.voxel_size)
    res["same_goal_as_reference_expression"] = bool(np.array_equal(mine["goal_vxl"], np.asarray(theirs[0])))

    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = [1.0, 1.2, 1.1]
    np.random.seed(0)
    n = max(5, a.repeats // 10)
    res["planning_step_ms"], res["planning_step_min_ms"] = median_ms(lambda: p.uncertainty_aware_planning_v2([u_dev, s_dev], pose), n, warmup=2)
    res["planning_step_reachable"] = bool(p.uncertainty_aware_planning_v2([u_dev, s_dev], pose)["is_goal_reachable"])
    # uncertainty only inside the pillar's shell, where no safe goal sees it: the first aggregation is invalid
    hidden = (rs.randint(1, 512, size=DIMS) / 64.0 * (sdf < -1.0) * (np.abs(np.arange(DIMS[0])[:, None, None] - 24.0) < 2)).astype(np.float32)
    h_dev = torch.from_numpy(hidden).to(dev)
    ok2, _ = agg.uncertainty_aggregation_v2([h_dev, s_dev])
    res["traversability_case_first_aggregation_valid"] = bool(ok2)
    p.planner_cfg["force_uncert_aggre"] = True                      # (the second aggregation is invalid too: keep its outputs, as the config key allows)

    def trav():
        p.traversability_mask = np.ones(DIMS, dtype=np.float32)
        orig = p.planner_cfg["force_uncert_aggre"]
        first = {"done": False}
        real = p._aggregate

        def aggregate(u, s):
            if not first["done"]:
                first["done"] = True
                p.planner_cfg["force_uncert_aggre"] = False
                try:
                    return real(u, s)
                finally:
                    p.planner_cfg["force_uncert_aggre"] = orig
            return real(u, s)
        p._aggregate = aggregate
        try:
            return p.uncertainty_aware_planning_v2([h_dev, s_dev], pose)
        finally:
            p._aggregate = real
    res["planning_step_traversability_ms"], res["planning_step_traversability_min_ms"] = median_ms(trav, max(3, n // 2), warmup=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

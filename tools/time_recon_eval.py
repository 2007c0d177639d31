"""Time the reconstruction metrics on the device (naruto_amd.evaluation): surface sampling, grid build, nearest-neighbour query through
the grid (queries in cell order and as they come, several ring budgets and cell sizes), the tiled scan, the share of queries the scan
had to serve, the reduction, and a whole ReconEvaluatorHIP.evaluate_field at voxel 0.05 on the office_0 box.  Clouds: surface samples
of a synthetic room-plus-sphere mesh pair (reconstruction = walls moved by 2 cm, sphere radius + 1 cm), 200 000 x 200 000 and
800 000 queries x 2 000 000 targets.  Next to the device times: scipy's cKDTree build + query on the same host for the same clouds, as
context only -- it is NOT the reference's own run (which samples with trimesh and needs its own environment), and there is no time bar.

    python tools/time_recon_eval.py --section small|large|field [--out profiles/r11_time_recon_eval.json]

Each section is one process (run each under its own timeout); sections merge into the output file.  Times are wall clock ending in a
device synchronise, every shape warmed up first, best of --repeat."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from naruto_amd import evaluation as E  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402


def timed(fn, repeat, warm=1):
    for _ in range(warm):
        fn()
    best, out = None, None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best * 1e3, out


def meshes(dev):
    vg, fg = syn.room_sphere_mesh(0.0, 0.8)
    vr, fr = syn.room_sphere_mesh(0.02, 0.81)
    gt = (torch.from_numpy(vg).to(dev), torch.from_numpy(fg).to(dev))
    rec = (torch.from_numpy(vr).to(dev), torch.from_numpy(fr).to(dev))
    return gt, rec


def pair(n_query, n_target, repeat, scan_repeat, sweeps):
    dev = torch.device("cuda:0")
    gt, rec = meshes(dev)
    res = {"queries": n_query, "targets": n_target}
    res["sample_target_ms"], (target, _) = timed(lambda: E.sample_surface(*gt, n_target, 0), repeat)
    res["sample_queries_ms"], (query, _) = timed(lambda: E.sample_surface(*rec, n_query, 1), repeat)
    res["grid_build_ms"], grid = timed(lambda: E.PointGridHIP(target), repeat)
    res["cell_m"], res["dims"] = grid.cell, list(grid.dims)
    res["grid_query_cell_ordered_ms"], (d, i) = timed(lambda: grid.query(query, sort_queries=True), repeat)
    res["fallback_share"] = int(grid.last_fallback[0]) / n_query
    res["grid_query_as_given_ms"], (d2, i2) = timed(lambda: grid.query(query, sort_queries=False), repeat)
    assert torch.equal(d.view(torch.int64), d2.view(torch.int64)) and torch.equal(i, i2)
    res["scan_query_ms"], (d3, i3) = timed(lambda: grid.query(query, method="scan"), scan_repeat, warm=0 if scan_repeat == 1 else 1)
    assert torch.equal(d.view(torch.int64), d3.view(torch.int64)) and torch.equal(i, i3)
    res["reduce_ms"], out = timed(lambda: E.reduce_distances(d, 0.05), repeat)
    res["mean_distance_cm"], res["share_below_5cm"] = float(out[0]) * 100.0, float(out[1]) / n_query
    if sweeps:
        res["ring_budget_sweep"] = {}
        for budget in (2, 3, 4, 6, 8):
            ms, _ = timed(lambda: grid.query(query, ring_budget=budget), repeat)
            res["ring_budget_sweep"][str(budget)] = {"query_ms": ms, "fallback_share": int(grid.last_fallback[0]) / n_query}
        res["cell_sweep"] = {}
        for factor in (0.5, 0.75, 1.0, 1.5, 2.0, 4.0):
            build_ms, g2 = timed(lambda: E.PointGridHIP(target, cell=grid.cell * factor), repeat)
            ms, _ = timed(lambda: g2.query(query), repeat)
            res["cell_sweep"][str(factor)] = {"cell_m": g2.cell, "build_ms": build_ms, "query_ms": ms, "fallback_share": int(g2.last_fallback[0]) / n_query}
    # context: the host's kd-tree on the same clouds
    from scipy.spatial import cKDTree
    tq, tt = query.cpu().numpy(), target.cpu().numpy()
    t0 = time.perf_counter()
    tree = cKDTree(tt)
    t1 = time.perf_counter()
    dk, _ = tree.query(tq)
    t2 = time.perf_counter()
    res["host_ckdtree_context"] = {"build_ms": (t1 - t0) * 1e3, "query_ms": (t2 - t1) * 1e3, "threads": 1,
                                   "note": "scipy cKDTree on this host, same clouds; not the reference's own run"}
    assert np.array_equal(dk.view(np.uint64), d.cpu().numpy().view(np.uint64))
    res["distances_equal_ckdtree_bitwise"] = True
    return res


def field(repeat):
    import helpers as H
    dev = torch.device("cuda:0")
    cfg = H.office_cfg(16)
    ora = H.make_oracle(cfg, 0.2, 1)
    m = H.make_hip_from_oracle(cfg, ora, dev).eval()
    bound = np.asarray(cfg["mapping"]["bound"], dtype=np.float64)
    mid = bound.mean(1)
    vg, fg = syn.room_sphere_mesh(0.0, 0.5, lo=bound[:, 0] + 0.1, hi=bound[:, 1] - 0.1, centre=mid)
    res = {"voxel_m": 0.05, "box": bound.tolist(), "n_samples": 200000}
    res["evaluator_setup_ms"], ev = timed(lambda: E.ReconEvaluatorHIP((vg, fg), device=dev), repeat)
    with torch.no_grad():
        res["evaluate_field_ms"], out = timed(lambda: ev.evaluate_field(m, cfg, m.bounding_box, 0.05), repeat)
        v, f = E.M.extract_surface(m.query_sdf, cfg, m.bounding_box, voxel_size=0.05)
        res["extract_surface_ms"], _ = timed(lambda: E.M.extract_surface(m.query_sdf, cfg, m.bounding_box, voxel_size=0.05), repeat)
        res["evaluate_mesh_ms"], _ = timed(lambda: ev.evaluate_mesh(v, f), repeat)
    res["mesh_vertices"], res["mesh_faces"] = len(v), len(f)
    res["fallback_share_rec_to_gt"] = int(ev.gt_grid.last_fallback[0]) / ev.n_samples
    res["fallback_share_gt_to_rec"] = int(ev.rec_grid.last_fallback[0]) / ev.n_samples
    res["metrics_of_the_untrained_closed_form_field"] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=["small", "large", "field"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    if args.section == "small":
        res = pair(200000, 200000, args.repeat, args.repeat, sweeps=True)
    elif args.section == "large":
        res = pair(800000, 2000000, 3, 1, sweeps=False)
    else:
        res = field(3)
    print(json.dumps({args.section: res}, indent=1))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc.setdefault("device", torch.cuda.get_device_name(0))
        doc.setdefault("what", "tools/time_recon_eval.py: wall clock ending in a device synchronise, warmed up, best of --repeat; milliseconds")
        doc[args.section] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

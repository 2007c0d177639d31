"""Time the planner's RRT on the device (naruto_amd.rrt.RRTNarutoHIP): the scenes of tests/golden/g12_rrt_*.npz replayed from their
recorded rows, and a full run_full at office_0 size (96 040 iterations, the reference's default max_iter) with the nearest-node
search over the cell lists and as a plain scan.  Next to each device time: the numpy restatement (tests/rrt_spec.py) on the same
host, as context only -- it is not the reference (which needs its own environment) and there is no time bar.

    python tools/time_rrt.py [--out profiles/r10_time_rrt.json]

Times are wall clock around the call with the device idle before and after (they include the host's part: drawing / uploading
rows, the one state read-back per launch, buffer growth), best of `--repeat`."""
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

import rrt_spec as RS  # noqa: E402
from naruto_amd import _lib  # noqa: E402
from naruto_amd.rrt import RRTNarutoHIP  # noqa: E402


def load(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", f"g12_rrt_{name}.npz")))


def planner(rec, **kw):
    args = dict(bbox=rec["bbox"], voxel_size=float(rec["voxel_size"]), max_iter=int(rec["max_iter"]), step_size=float(rec["step_size"]), maxz=int(rec["maxz"]),
                step_amplifier=float(rec["step_amplifier"]), collision_thre=float(rec["collision_thre"]), enable_direct_line=bool(rec["direct"]))
    args.update(kw)
    return RRTNarutoHIP(**args)


def timed(fn, repeat):
    best = None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best, out


def scene(name, repeat):
    rec = load(name)
    p = planner(rec)
    vol = torch.from_numpy(rec["vol"]).cuda()

    def calls():
        p.start_new_plan(rec["start"], rec["goal"], vol)
        used = 0
        for c, upto in zip(rec["calls"], rec["rows_after_call"]):
            (p.run if c == 0 else p.run_full)(points=rec["rows"][used:int(upto)])
            used = int(upto)
        return p.n_nodes
    calls()                                                  # warm-up: library load, buffers at their final size
    t_dev, n = timed(calls, repeat)
    assert n == len(rec["parents"]), (name, n)
    row = {"scene": name, "calls": ["run" if c == 0 else "run_full" for c in rec["calls"]], "max_iter": int(rec["max_iter"]), "extensions": len(rec["rows"]),
           "nodes": int(n), "device_ms": round(t_dev * 1e3, 3)}
    t = time.perf_counter()
    s, _ = RS.replay_fixture(rec)
    row["numpy_spec_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    if "mask" in rec:
        row["mask_device_ms"] = round(timed(p.get_reachable_mask, repeat)[0] * 1e3, 3)
        t = time.perf_counter()
        s.reachable_mask()
        row["mask_numpy_spec_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    print(row, flush=True)
    return row


def full(repeat, n_iter, thresholds):
    rec = load("d")
    vol = torch.from_numpy(rec["vol"]).cuda()
    np.random.seed(2024)
    rows = RS.draw_rows(n_iter, [0, 0, 0], [48, 55, 34])
    out = {"volume": list(rec["vol"].shape), "iterations": n_iter, "by_cell_threshold": []}
    trees = []
    for thr in thresholds:
        p = planner(rec, max_iter=n_iter, cell_threshold=thr)

        def go():
            p.start_new_plan(rec["start"], rec["goal"], vol)
            p.run_full(points=rows)
            return p.n_nodes
        go()
        t_dev, n = timed(go, repeat)
        t_mask = timed(p.get_reachable_mask, repeat)[0]
        trees.append((p.parents(), p.nodes_xyz()))
        row = {"cell_threshold": "default (%d)" % _lib.RRT_CELL_THRESHOLD if thr == 0 else ("plain scan" if thr >= 1 << 30 else thr), "nodes": int(n),
               "run_full_ms": round(t_dev * 1e3, 2), "us_per_iteration": round(t_dev * 1e6 / n_iter, 2), "mask_ms": round(t_mask * 1e3, 3)}
        print(row, flush=True)
        out["by_cell_threshold"].append(row)
    out["same_tree_for_every_threshold"] = all(np.array_equal(t[0], trees[0][0]) and np.array_equal(t[1], trees[0][1]) for t in trees)
    # context: the restatement on the first iterations only (its nearest-node scan and Python loop make the full run a matter of hours)
    k = min(3000, n_iter)
    s = RS.SpecRRT(rec["vol"], 1.0, 10, 0.5, True)
    s.start_new_plan(rec["start"], rec["goal"])
    t = time.perf_counter()
    s.run_full(rows, k)
    out["numpy_spec_first_iterations"] = {"iterations": k, "ms": round((time.perf_counter() - t) * 1e3, 1), "nodes": s.n}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_time_rrt.json"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=96040)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res = {"device": torch.cuda.get_device_name(0), "what": "wall clock per call sequence incl. host side, best of %d; numpy_spec_* = tests/rrt_spec.py on this host, context only" % a.repeat,
           "scenes": [scene(n, a.repeat) for n in ("a", "b", "c", "d", "e")],
           "run_full_office0": full(a.repeat, a.iterations, (0, 256, 16384, 1 << 30))}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

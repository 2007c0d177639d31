"""Time the rigid alignment on the device (naruto_amd.evaluation.icp, csrc/naruto_icp.hip): the cost of one iteration split into
transform / nearest-neighbour query / accumulate / step, and a whole ``icp``, at 4 099 x 20 000 points (the test table's first row) and at
about 800 000 x 1 000 000 points (evaluation size).  Clouds: two ``sample_surface`` clouds of the synthetic room-plus-sphere mesh (target
seed 0, source seed 1), the source displaced by 2 degrees about (0.3, -0.5, 0.8) through the target's centroid and by 3 cm.  Next to the
device times: the numpy + scipy cKDTree twin (tests/icp_spec.py) on the same host for the same clouds (one iteration at both sizes, a
whole run at the small one), as context only -- there is no time bar.

    python tools/time_icp.py --section small|large [--out profiles/time_icp.json]

Each section is one process (run each under its own timeout); sections merge into the output file.  Times are host wall clock ending
in a device synchronise, every shape warmed up first, the MEDIAN of --repeat."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import icp_spec as IS  # noqa: E402
from naruto_amd import _lib  # noqa: E402
from naruto_amd import evaluation as E  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402


def timed(fn, repeat, warm=1):
    for _ in range(warm):
        fn()
    times, out = [], None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return statistics.median(times) * 1e3, out


def section(n_source, n_target, repeat, twin_whole):
    dev = torch.device("cuda:0")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_icp.py measures on the GPU; there is none here")
    lib = _lib.load()
    v, f = syn.room_sphere_mesh(0.0, 0.8)
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    target, _ = E.sample_surface(vd, fd, n_target, 0)
    raw, _ = E.sample_surface(vd, fd, n_source, 1)
    known = IS.rigid(2.0, 0.03, target.double().mean(0).cpu().numpy())
    source = E.transform_points(raw, known)
    res = {"source_points": n_source, "target_points": n_target}
    res["grid_build_ms"], grid = timed(lambda: E.PointGridHIP(target), repeat)
    # one iteration, stage by stage, at the initial transformation
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    state = torch.zeros(_lib.ICP_STATE_DOUBLES, dtype=torch.float64, device=dev)
    state[:16] = torch.eye(4, dtype=torch.float64).reshape(16)
    moved = torch.empty_like(source)
    sums = torch.empty(_lib.ICP_SUMS, dtype=torch.float64, device=dev)
    ws = _lib.workspace(lib.naruto_icp_accumulate_workspace(n_source), dev, torch.float64)
    origin = (C.c_double * 3)(*(0.5 * (grid.box[0] + grid.box[1])))
    res["transform_ms"], _ = timed(lambda: _lib.check(lib.naruto_icp_transform(n_source, source.data_ptr(), 0, state.data_ptr(), moved.data_ptr(), stream())), repeat)
    res["query_ms"], (dist, index) = timed(lambda: grid.query(moved), repeat)
    res["accumulate_ms"], _ = timed(lambda: _lib.check(lib.naruto_icp_accumulate(n_source, moved.data_ptr(), n_target, grid.target.data_ptr(), index.data_ptr(),
                                                                                dist.data_ptr(), 0.1, origin, ws.data_ptr(), sums.data_ptr(), stream())), repeat)
    scratch = state.clone()

    def step():
        scratch.copy_(state)
        _lib.check(lib.naruto_icp_step(sums.data_ptr(), n_source, origin, 30, 1e-6, 1e-6, scratch.data_ptr(), stream()))
    res["step_with_state_copy_ms"], _ = timed(step, repeat)
    res["status_row_read_ms"], _ = timed(lambda: scratch[16:24].cpu(), repeat)
    res["icp_ms"], out = timed(lambda: E.icp(source, grid), repeat)
    res["icp_with_grid_build_ms"], _ = timed(lambda: E.icp(source, target), repeat)
    res["iterations"], res["status"], res["fitness"], res["inlier_rmse"] = out.iterations, out.status, out.fitness, out.inlier_rmse
    res["icp_ms_per_evaluation"] = res["icp_ms"] / len(out.history)
    res["max_abs_T_times_known_minus_identity"] = float(np.abs(out.transformation @ known - np.eye(4)).max())
    # context: the twin on this host
    from scipy.spatial import cKDTree
    src_np, tgt_np = source.cpu().numpy(), target.cpu().numpy()
    t0 = time.perf_counter()
    tree = cKDTree(tgt_np)
    t1 = time.perf_counter()
    fit, rmse, inl, idx = IS.evaluate(IS.transform(src_np, np.eye(4)), tree, 0.1)
    IS.kabsch(src_np[inl], tgt_np[idx[inl]])
    t2 = time.perf_counter()
    ctx = {"tree_build_ms": (t1 - t0) * 1e3, "one_iteration_ms": (t2 - t1) * 1e3, "threads": 1,
           "note": "tests/icp_spec.py (numpy + scipy cKDTree) on this host, same clouds; context only"}
    assert fit == out.history[0][0]
    if twin_whole:
        t0 = time.perf_counter()
        twin = IS.icp(src_np, tgt_np)
        ctx["icp_ms"], ctx["iterations"] = (time.perf_counter() - t0) * 1e3, twin["iterations"]
    res["host_twin_context"] = ctx
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=["small", "large"], required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    res = section(4099, 20000, args.repeat, True) if args.section == "small" else section(800000, 1000000, min(args.repeat, 3), False)
    print(json.dumps({args.section: res}, indent=1))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                doc = json.load(fh)
        doc.setdefault("device", torch.cuda.get_device_name(0))
        doc.setdefault("what", "tools/time_icp.py: host wall clock ending in a device synchronise, warmed up, median of --repeat; milliseconds")
        doc[args.section] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

"""Record tests/golden/g12_rrt_*.npz from the REFERENCE's own RRTNaruto / is_collision_free, on the CPU.

    python tools/make_rrt_golden.py --reference /path/to/the/reference/checkout

The reference's un-vendored imports are stood in by oracle.coslam_standins (imported, not edited), Node's device default is set
to 'cpu' and tqdm is replaced by the identity.  Only data is recorded: the volume, start, goal, seed, the random rows the
reference drew, its nodes (float64), parents, rrt_iter, reachable flags, path and mask.

A seed is kept only if tests/rrt_spec.py, fed the same rows, builds the same tree AND every decision it took has a margin of at
least 1000 rounding units (see the docstring of rrt_spec); the kept minimum is stored as `min_margin`.
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import rrt_spec as RS  # noqa: E402

DIMS = (49, 56, 35)                       # office_0 at 0.1 m
BBOX = np.array([[0.0, 4.8], [0.0, 5.5], [0.0, 3.4]])
STEP, AMP, THRE, MAXZ = 1.0, 10, 0.5, 28


def _grid():
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in DIMS), indexing="ij")


def _quant(v):
    return (np.round(v * 64.0) / 64.0).astype(np.float32)          # few mantissa bits: the fixtures compress well


def vol_room():
    x, y, z = _grid()
    return np.minimum.reduce([x - 1, DIMS[0] - 2 - x, y - 1, DIMS[1] - 2 - y, z - 1, DIMS[2] - 2 - z])


def vol_wall_door():
    x, y, z = _grid()
    door = np.maximum(np.abs(y - 44.0) - 4.0, np.abs(z - 12.0) - 8.0)
    return _quant(np.minimum(vol_room(), np.maximum(np.abs(x - 24.0) - 1.0, -door)))


def vol_pocket(c):
    x, y, z = _grid()
    r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    return _quant(np.minimum(vol_room(), np.abs(r - 2.5) - 1.2))


def load_reference(path):
    from oracle import coslam_standins
    coslam_standins.install()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
            sys.modules["tqdm"].tqdm = lambda it, **k: it
    sys.path.insert(0, path)
    from src.planner import rrt as ref_rrt, rrt_naruto as ref_naruto
    ident = lambda it, **k: it  # noqa: E731
    ref_rrt.tqdm = ident
    ref_naruto.tqdm = ident
    ref_rrt.Node.__init__.__defaults__ = ("cpu",)
    return ref_rrt, ref_naruto


def run_reference(ref_naruto, vol, start, goal, seed, calls, max_iter, direct=True):
    """calls: list of 'run' / 'full'.  -> dict of recorded arrays, the planner."""
    p = ref_naruto.RRTNaruto(bbox=BBOX, voxel_size=0.1, max_iter=max_iter, step_size=STEP, maxz=MAXZ, step_amplifier=AMP, collision_thre=THRE,
                             device="cpu", enable_direct_line=direct)
    assert tuple(p.reachable_3d_mask.shape) == DIMS, p.reachable_3d_mask.shape
    rows, draw = [], p.generate_random_point

    def logged(full_range=False):
        r = draw(full_range)
        rows.append(r)
        return r
    p.generate_random_point = logged
    np.random.seed(seed)
    p.start_new_plan(np.asarray(start, dtype=np.float64), np.asarray(goal, dtype=np.float64), vol)
    flags, counts, rows_after = [], [], []
    for c in calls:
        if c == "run":
            flags.append(bool(p.run()))
        else:
            p.run_full()
        counts.append(len(p.nodes))
        rows_after.append(len(rows))
    index = {id(n): i for i, n in enumerate(p.nodes)}
    out = {"vol": vol, "start": np.asarray(start, dtype=np.float64), "goal": np.asarray(goal, dtype=np.float64), "seed": np.int64(seed),
           "rows": np.array(rows, dtype=np.float64).reshape(-1, 3), "rows_after_call": np.array(rows_after, dtype=np.int64),
           "nodes": np.stack([n._xyz_arr for n in p.nodes]).astype(np.float64),
           "parents": np.array([-1 if n.parent is None else index[id(n.parent)] for n in p.nodes], dtype=np.int32),
           "nodes_after_call": np.array(counts, dtype=np.int64), "rrt_iter": np.int64(p.rrt_iter), "reachable": np.array(flags, dtype=np.bool_),
           "calls": np.array([0 if c == "run" else 1 for c in calls], dtype=np.int64), "max_iter": np.int64(max_iter),
           "step_size": np.float64(STEP), "step_amplifier": np.float64(AMP), "collision_thre": np.float64(THRE), "maxz": np.int64(MAXZ),
           "direct": np.bool_(direct), "bbox": BBOX, "voxel_size": np.float64(0.1),
           "x_range": np.array(p.x_range, dtype=np.float64), "y_range": np.array(p.y_range, dtype=np.float64), "z_range": np.array(p.z_range, dtype=np.float64)}
    if "run" in calls:
        out["path"] = np.array([index[id(n)] for n in p.find_path()[1:]], dtype=np.int32)
    return out, p


def run_spec(rec):
    s, flags = RS.replay_fixture(rec)
    try:
        RS.same_tree(rec, s.n, s.parent, s.nodes_xyz(), s.rrt_iter, flags, s.path())
    except AssertionError:
        return s, False
    return s, True


def scene(ref_naruto, name, vol, start, goal, calls, max_iter, want_mask, accept, first_seed, out_dir):
    for seed in range(first_seed, first_seed + 200):
        rec, p = run_reference(ref_naruto, vol, start, goal, seed, calls, max_iter)
        try:
            s, same = run_spec(rec)
        except Exception as e:          # the spec ran out of rows: it took another turn than the reference
            print(f"  {name}: seed {seed} refused: spec diverged ({e})")
            continue
        m = s.marg.smallest
        if not same or m < RS.NEED or not accept(rec):
            print(f"  {name}: seed {seed} refused: same tree {same}, smallest margin {m:.3g}, scene as wanted {bool(accept(rec))} "
                  f"(reachable {list(rec['reachable'])}, rows {len(rec['rows'])}, nodes {len(rec['parents'])})")
            continue
        rec["min_margin"] = np.float64(m)
        if want_mask:
            rec["mask"] = p.get_reachable_mask().astype(np.float32)
            sm, d64 = s.reachable_mask()
            band = np.abs(d64 - STEP) <= 1e-4
            rec["mask_band_voxels"] = np.int64(band.sum())
            assert band.mean() <= 0.005 and np.array_equal(sm[~band], rec["mask"][~band]), (band.sum(), (sm != rec["mask"]).sum())
        path = os.path.join(out_dir, f"g12_rrt_{name}.npz")
        np.savez_compressed(path, **rec)
        print(f"{name}: seed {seed}, {len(rec['parents'])} nodes, rrt_iter {int(rec['rrt_iter'])}, rows {len(rec['rows'])}, reachable {list(rec['reachable'])}, "
              f"min margin {m:.3g} units {({k: float(f'{v:.3g}') for k, v in s.marg.by_kind.items()})}, {os.path.getsize(path)} bytes")
        return rec
    raise SystemExit(f"{name}: no seed accepted")


def segments(ref_rrt, vol, out_dir, n=2000):
    rng = np.random.RandomState(12)
    hi = np.array(DIMS, dtype=np.float64) - 1.0
    pa, pb, cnt, comp, worst = [], [], [], [], np.inf
    while len(pa) < n:
        a = rng.uniform(0.01, hi - 0.01)
        d = rng.normal(size=3)
        b = np.clip(a + d / np.linalg.norm(d) * rng.uniform(0.05, 12.0), 0.01, hi - 0.01)
        m = RS.Margins()
        got = RS.collision_free(a, b, vol, STEP, THRE, m)
        ref = ref_rrt.is_collision_free(a, b, vol, step_size=STEP, collision_thre=THRE)
        if m.smallest < RS.NEED:
            continue
        assert (int(ref[0]), bool(ref[1])) == got, (a, b, ref, got)
        worst = min(worst, m.smallest)
        pa.append(a); pb.append(b); cnt.append(int(ref[0])); comp.append(bool(ref[1]))
    path = os.path.join(out_dir, "g12_rrt_segments.npz")
    np.savez_compressed(path, vol=vol, pa=np.array(pa), pb=np.array(pb), num_collision_free=np.array(cnt, dtype=np.int32), complete_free=np.array(comp, dtype=np.bool_),
                        step_size=np.float64(STEP), collision_thre=np.float64(THRE), min_margin=np.float64(worst))
    print(f"segments: {n}, complete {int(np.sum(comp))}, counts {min(cnt)}..{max(cnt)}, min margin {worst:.3g}, {os.path.getsize(path)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NARUTO_REFERENCE"), required=os.environ.get("NARUTO_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    ref_rrt, ref_naruto = load_reference(a.reference)
    only = set(a.only.split(",")) - {""}
    room, wall = _quant(vol_room()), vol_wall_door()
    pocket_goal = np.array([40.013, 12.021, 14.008])
    todo = {
        "a": lambda: scene(ref_naruto, "a", room, [8.3, 9.7, 12.2], [38.6, 44.1, 17.4], ["run"], 3000, False, lambda r: r["reachable"][0] and int(r["rrt_iter"]) == 1, 0, a.out),
        "b": lambda: scene(ref_naruto, "b", wall, [8.3, 9.7, 12.2], [26.4, 12.1, 14.4], ["run"], 3000, False, lambda r: r["reachable"][0] and len(r["rows"]) > 20, 0, a.out),
        "c": lambda: scene(ref_naruto, "c", vol_pocket([40.0, 12.0, 14.0]), [8.3, 9.7, 12.2], pocket_goal, ["run", "run"], 300, True, lambda r: not r["reachable"].any(), 0, a.out),
        "d": lambda: scene(ref_naruto, "d", wall, [8.3, 9.7, 12.2], [40.6, 12.1, 14.4], ["full"], 1500, True, lambda r: len(r["parents"]) > 2 * 2048 - 1024, 0, a.out),
        "e": lambda: scene(ref_naruto, "e", (wall * 0.0 + 100.0).astype(np.float32), [20.5, 30.25, 10.0], [25.5, 12.75, 10.0], ["run"], 3000, False,
                           lambda r: r["reachable"][0], 0, a.out),
        "segments": lambda: segments(ref_rrt, wall, a.out),
    }
    for k, fn in todo.items():
        if not only or k in only:
            fn()


if __name__ == "__main__":
    main()

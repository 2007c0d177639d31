"""Time mesh subdivision on the device (naruto_amd.remesh) at the evaluation protocol's size: tools/time_cull.py's scene, the room-plus-sphere
mesh of about 1.6 M faces, subdivided to max_edge = 0.015.  Recorded: per generation the faces in and out and the time of each stage (mark,
the two prefix sums, the edge table, the prefix copy of the vertices, emit), the whole subdivision, and the whole 2 000-pose cull at
1200 x 680 with and without it.  Beside each stage stand its algorithmic bytes -- faces read, vertex gathers, 48 B per split face, 12 or
24 B per midpoint, the table's fill and probes -- and those bytes over the stage's time as a fraction of the 6.29 TB/s DESIGN uses as
achievable HBM bandwidth.

    python tools/time_subdivide.py [--out profiles/time_subdivide.json] [--poses 2000] [--repeat 5]

There is NO parent and NO reference number: trimesh and pyrender are not on this stack, so nothing passes or fails on time.  Context only:
the numpy restatement's host time for the same mesh (tests/subdivide_spec.py).  Times are host clocks that end in a device synchronise,
one warm-up, medians of --repeat; the per-stage times come from a run with a synchronise after every stage, the whole from a run without."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from naruto_amd import culling as CU  # noqa: E402
from naruto_amd import remesh as RM  # noqa: E402
from naruto_amd import synthetic as syn  # noqa: E402
import cull_spec as CS  # noqa: E402
import subdivide_spec as SD  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
STAGES = ("mark_s", "scan_s", "edges_s", "copy_s", "emit_s")


def stage_bytes(row, vertex_bytes, colors):
    """Algorithmic bytes of one generation's stages from its counts: what the algorithm must read and write, not what the caches moved."""
    F, V, L, Mi, T = row["faces_in"], row["vertices_in"], row.get("n_long", 0), row.get("n_mid", 0), row.get("table_slots", 0)
    out = {"mark_s": F * 12 + 3 * F * vertex_bytes + F,                                           # faces, three vertex gathers, one flag byte
           "scan_s": F * (1 + 4) + 3 * L * (1 + 4)}                                               # flags -> rank, own -> mid_rank
    if L:
        out["edges_s"] = (F * (1 + 4) + L * 12 + T * 12 + 3 * L * 4                                # flags, rank, long faces; the table's fill
                          + 3 * L * (8 + 4 + 4) + 3 * L * (4 + 4 + 1))                           # probe, minimum, cell; cell, ordinal -> own
        out["copy_s"] = 2 * V * (vertex_bytes + (4 if colors else 0))                             # the existing rows into the new arrays
        out["emit_s"] = (F * (12 + 1 + 4) + (F - L) * 12 + L * (3 * (4 + 4 + 4) + 48)              # faces, flags, rank; short rows; cells, owners, numbers, 48 B of children
                         + Mi * (3 * vertex_bytes + (12 if colors else 0)))                      # two gathers and one row per midpoint
    return out


def median_rows(runs, vertex_bytes, colors):
    rows = []
    for g in range(len(runs[0])):
        row = {k: v for k, v in runs[0][g].items() if not k.endswith("_s")}
        nbytes = stage_bytes(runs[0][g], vertex_bytes, colors)
        for s in STAGES:
            if all(s in r[g] for r in runs):
                sec = statistics.median(r[g][s] for r in runs)
                row[s[:-2]] = {"ms": sec * 1e3, "algorithmic_bytes": nbytes.get(s, 0),
                               "share_of_6.29_TB_per_s": nbytes.get(s, 0) / sec / HBM_BYTES_PER_S if sec > 0 else None}
        rows.append(row)
    return rows


def wall(fn, repeat, warm=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--poses", type=int, default=2000)
    ap.add_argument("--pose-chunk", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-lat", type=int, default=632)
    ap.add_argument("--max-edge", type=float, default=0.015)
    ap.add_argument("--skip-host", action="store_true", help="leave the numpy restatement's host time out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_subdivide: no GPU; a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    cam = {"H": 680, "W": 1200, "fx": 600.0, "fy": 600.0, "cx": 599.5, "cy": 339.5}
    vn, fn = syn.room_sphere_mesh(n_lat=args.n_lat, n_lon=2 * args.n_lat)
    v, f = torch.from_numpy(vn).to(dev), torch.from_numpy(fn).to(dev)
    res = {"faces": len(fn), "vertices": len(vn), "max_edge": args.max_edge, "vertex_dtype": "float32", "colors": False, "repeat": args.repeat,
           "reference": "none: trimesh and pyrender are not on this stack; nothing passes or fails on time"}

    def staged():
        rows = []
        RM.subdivide_on_device(v, f, None, args.max_edge, timings=rows)
        return rows

    staged()                                                                  # the warm-up
    runs = [staged() for _ in range(args.repeat)]
    res["generations"] = median_rows(runs, 12, False)
    ms, out = wall(lambda: RM.subdivide_on_device(v, f, None, args.max_edge), args.repeat)
    res["whole_subdivision_ms"] = ms
    res["result"] = {"faces": len(out[1]), "vertices": len(out[0]), "generations": out[3].generations, "remaining_long": out[3].remaining_long}
    del out

    poses = CS.ring_poses(args.poses)
    for name, kw in (("whole_cull_ms", {}), ("whole_cull_with_subdivision_ms", {"max_edge": args.max_edge})):
        ms, out = wall(lambda: CU.cull_mesh((v, f), poses, cam, pose_chunk=args.pose_chunk, **kw), 3)
        res[name] = ms
        res[name.replace("_ms", "_kept_faces")] = len(out[1])
        del out

    if not args.skip_host:
        t = time.perf_counter()
        host = SD.subdivide_to_size(vn, fn, args.max_edge)
        res["host_restatement_context"] = {"ms": (time.perf_counter() - t) * 1e3, "faces": len(host[1]),
                                           "note": "tests/subdivide_spec.py in numpy on this host; context only, not the reference"}
    print(json.dumps(res, indent=1))
    if args.out:
        doc = {"device": torch.cuda.get_device_name(0),
               "what": "tools/time_subdivide.py: host clocks ending in a device synchronise, one warm-up, medians; milliseconds",
               "protocol_size": res}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

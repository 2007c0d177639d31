"""Record tests/golden/g14_planner_*.npz from the REFERENCE's own NarutoPlanner, rotation_planning and compute_camera_pose, on the CPU.

    python tools/make_planner_golden.py --reference /path/to/the/reference/checkout

The reference's un-vendored imports are stood in by oracle.coslam_standins (imported, not edited), its ``.cuda()`` calls are no-ops and
the RRT's device default is 'cpu', as in tools/make_rrt_golden.py.  Only data is recorded:

  g14_planner_rotations.npz   (a) camera poses and rotation plans: one and several targets, hops below max_rot_deg and hops that are
                              no multiple of it, the vertical look-at edge; no hop within 1 degree of 180 (the slerp axis is
                              ill-conditioned there).  Also the planner entries of configs/default.py, as JSON.
  g14_planner_traj_<name>.npz (b) + (c) a main() trajectory over a 24 x 28 x 17 volume at 0.1 m, driven as src/naruto/main.py:90-140
                              drives it (the returned float32 pose is the next step's), with a stub simulator that returns scripted
                              scalars and ONE np.random.seed for the RRT's stream.  Per step: state, returned pose, path, look-at
                              list, is_new_vols; per aggregation call the targets the reference chose; per goal search its inputs
                              and results; per planning call its results; per collision test its result.

Fixture conditions (the reference has no tie rule, and its sums cannot be read off), checked here, a seed being searched until all hold:
  * uncertainties are multiples of 2^-6 below 8: any fp32 summation order of up to 4000 terms is exact;
  * at every goal search the maximum of the aggregated volume is unique and the positive values among the winning row's top
    obs_per_goal + 1 are distinct (the one more: no tie across the cut either);
  * every RRT plan, replayed by tests/rrt_spec.py on the rows the reference drew, is the same tree with every decision at least 1000
    rounding units clear, and so is every collision segment; no voxel of a reachable mask within 1e-4 of the reach carries
    uncertainty in any volume; no plan starts within a voxel of its goal;
  * tests/planner_spec.py replays the states exactly and every pose and rotation matrix within 1e-12 (stored as max_abs_diff).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "tools"))

import planner_spec as PS  # noqa: E402
import rrt_spec as RS  # noqa: E402

DIMS = (24, 28, 17)
BBOX = np.array([[0.0, 2.3], [0.0, 2.7], [0.0, 1.6]])
VOXEL = 0.1
PLANNER_KEYS = dict(uncert_top_k=400, uncert_top_k_subset=60, gs_sensing_range=[0.5, 0.8], safe_sdf=0.8, force_uncert_aggre=False, gs_z_levels=[6, 10],
                    obs_per_goal=4, enable_uncert_filtering=True, up_dir=[0, 0, 1], local_planner_method="RRTNaruto", invalid_region_ratio_thre=0.5,
                    collision_dist_thre=0.05, max_rot_deg=25, rrt_step_size=1.0, rrt_step_amplifier=10, rrt_maxz=100, rrt_max_iter=300, rrt_z_levels=None,
                    enable_eval=False, enable_direct_line=True, voxel_size=VOXEL, step_size=0.1, method="naruto", enable_timing=False)
NEW_VOLS_EVERY = 10


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_reference(path):
    import torch
    import make_rrt_golden as MR
    ref_rrt, ref_naruto = MR.load_reference(path)
    torch.Tensor.cuda = lambda self, *a, **k: self
    init = ref_naruto.RRTNaruto.__init__                                  # (the planner does not pass a device: the default becomes 'cpu')
    init.__defaults__ = tuple("cpu" if d == "cuda" else d for d in init.__defaults__)
    from src.planner import naruto_planner as ref_np, planner as ref_p, rotation_planning as ref_rot
    return ref_rrt, ref_naruto, ref_np, ref_p, ref_rot


# ---- (a) rotations ---------------------------------------------------------------------------------------------------------------
def random_rotation(rs):
    q = rs.normal(size=4)
    return PS.to_matrix(q / np.linalg.norm(q))


def rotations(ref_p, ref_rot, out_dir, default_planner):
    rs = np.random.RandomState(14)
    cases = []
    def add(A, Bs, R0, deg):
        cases.append((np.asarray(A, dtype=np.float64), np.asarray(Bs, dtype=np.float64).reshape(-1, 3), np.asarray(R0), float(deg)))
    for n_t in (1, 1, 2, 3, 5, 10):
        for deg in (10, 7.5, 33):
            A = rs.uniform(0.3, 2.0, 3)
            add(A, A + rs.normal(size=(n_t, 3)), random_rotation(rs).astype(np.float32 if n_t % 2 else np.float64), deg)
    A = np.array([1.0, 1.25, 0.5])
    R_small = PS.camera_pose(A, A + np.array([-1.0, 0.0, 0.0]))
    add(A, [A + np.array([-1.0, 0.05, 0.0])], R_small, 10)                            # a hop below max_rot_deg: no step in between
    add(A, [A + np.array([-1.0, 0.05, 0.0]), A + np.array([-1.0, 0.4, 0.1])], R_small.astype(np.float32), 10)
    add(A, [A + np.array([0.0, 0.0, 0.7])], R_small, 10)                             # the vertical look-at edge, above
    add(A, [A + np.array([0.0, 0.0, -0.7]), A + np.array([-0.3, 0.1, -0.7])], R_small.astype(np.float32), 10)    # ... and below, then a target beside it
    kept, worst = [], 0.0
    for A, Bs, R0, deg in cases:
        cams = [ref_p.compute_camera_pose(A.copy(), b.copy()) for b in Bs]
        hops = PS.hop_degrees(R0, cams)
        if max(hops) > 179.0:
            print(f"  rotations: a case with a hop of {max(hops):.2f} degrees refused")
            continue
        planned = ref_rot.rotation_planning(R0, cams, deg)
        mine_c = [PS.camera_pose(A.copy(), b.copy()) for b in Bs]
        mine = PS.plan_rotations(R0, mine_c, deg)
        assert len(mine) == len(planned), (len(mine), len(planned), hops, deg)
        worst = max([worst] + [float(np.abs(a - b).max()) for a, b in zip(mine_c + mine, cams + planned)])
        kept.append((A, Bs, R0, deg, np.stack(cams), np.stack(planned), np.array(hops)))
    assert worst <= 1e-12, worst
    assert any((k[6] < k[3]).any() for k in kept) and any(len(k[1]) == 1 for k in kept) and any(len(k[1]) > 3 for k in kept)
    T = max(len(k[1]) for k in kept)
    pad = lambda a: np.concatenate([a, np.zeros((T - len(a),) + a.shape[1:])])  # noqa: E731
    path = os.path.join(out_dir, "g14_planner_rotations.npz")
    np.savez_compressed(path, A=np.stack([k[0] for k in kept]), B=np.stack([pad(k[1]) for k in kept]), n_targets=np.array([len(k[1]) for k in kept]),
                        R0=np.stack([k[2].astype(np.float64) for k in kept]), max_rot_deg=np.array([k[3] for k in kept]),
                        cam=np.stack([pad(k[4]) for k in kept]), planned_len=np.array([len(k[5]) for k in kept]), planned=np.concatenate([k[5] for k in kept]),
                        max_abs_diff=np.float64(worst), default_planner=np.array(json.dumps(default_planner)))
    print(f"rotations: {len(kept)} cases, {sum(len(k[5]) for k in kept)} planned rotations, spec vs reference max abs diff {worst:.3g}, {os.path.getsize(path)} bytes")


def default_planner_entries(reference):
    ns = {}
    exec(compile(open(os.path.join(reference, "configs", "default.py")).read(), "default.py", "exec"), ns)
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in ns["planner"].items()}


# ---- (b) + (c) trajectories ------------------------------------------------------------------------------------------------------
def _grid():
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in DIMS), indexing="ij")


def _quant(v):
    return (np.round(v * 64.0) / 64.0).astype(np.float32)


def sdf_room():
    x, y, z = _grid()
    return np.minimum.reduce([x - 1, DIMS[0] - 2 - x, y - 1, DIMS[1] - 2 - y, z - 1, DIMS[2] - 2 - z])


def sdf_chamber():
    """The room with a sealed chamber x > 12, y > 14 behind two slabs 1.5 voxels thick."""
    x, y, z = _grid()
    slab_x = np.maximum(np.abs(x - 12.0) - 0.75, 13.25 - y)
    slab_y = np.maximum(np.abs(y - 14.0) - 0.75, 11.25 - x)
    return np.minimum.reduce([sdf_room(), slab_x, slab_y])


def blob(rs, box):
    """Uncertainty on the voxels of box = (x0, x1, y0, y1, z0, z1), distinct multiples of 2^-6 in [1, 8)."""
    u = np.zeros(DIMS, dtype=np.float32)
    (x0, x1, y0, y1, z0, z1) = box
    n = (x1 - x0) * (y1 - y0) * (z1 - z0)
    u[x0:x1, y0:y1, z0:z1] = (rs.choice(np.arange(64, 512), size=n, replace=False) / 64.0).reshape(x1 - x0, y1 - y0, z1 - z0)
    return u


class StubSim:
    """simulate(..., return_erp=True) -> a 4 x 8 distance map with the scripted minimum and number of invalid pixels."""

    def __init__(self, dist, invalid):
        self.dist, self.invalid, self.calls = dist, invalid, 0

    def simulate(self, c2w, return_erp=False, no_print=False):
        i = min(self.calls, len(self.dist) - 1)
        self.calls += 1
        erp = np.full(32, 1.5, dtype=np.float32)
        erp[0] = self.dist[i]
        erp[1:1 + int(self.invalid[i])] = 1e8
        return None, None, None, erp.reshape(4, 8)


class Refused(Exception):
    pass


def run_trajectory(ref, name, dataset, sdf, versions, start_xyz, n_steps, seed, sim_dist, sim_invalid, want, overrides=None):
    KEYS = {**PLANNER_KEYS, **(overrides or {})}
    _, ref_naruto, ref_np, _, _ = ref
    cfg = Cfg(planner=Cfg(KEYS), general=Cfg(dataset=dataset))
    cfg.planner["up_dir"] = np.array(KEYS["up_dir"])
    p = ref_np.NarutoPlanner(cfg, lambda *a, **k: None)
    rs = np.random.RandomState(1000 + seed)
    versions = [sum(blob(rs, box) for box in boxes) for boxes in versions]                 # (disjoint boxes)
    p.update_sim(StubSim(sim_dist, sim_invalid))
    p.init_data(BBOX.tolist())
    p.init_local_planner()
    lp = p.local_planner
    log = dict(agg_targets=[], agg_step=[], gs=[], plans=[], col_result=[], col_step=[], rrt=[])
    marg = RS.Margins()
    all_uncert = np.max(np.stack(versions), axis=0)

    # -- the RRT: rows drawn, calls made; each plan is replayed by the spec when the next one starts or the planning step ends
    draw = lp.generate_random_point
    cur = {}

    def logged_point(full_range=False):
        r = draw(full_range)
        cur["rows"].append(r)
        return r
    lp.generate_random_point = logged_point

    def close_plan():
        if not cur:
            return
        rec = dict(vol=cur["vol"], start=cur["start"], goal=cur["goal"], rows=np.array(cur["rows"], dtype=np.float64).reshape(-1, 3),
                   rows_after_call=np.array(cur["rows_after"], dtype=np.int64), calls=np.array(cur["calls"], dtype=np.int64), max_iter=lp.max_iter,
                   step_size=lp.step_size, step_amplifier=lp.step_amplifier, collision_thre=lp.collision_thre, direct=lp.enable_direct_line)
        index = {id(n): i for i, n in enumerate(lp.nodes)}
        rec["parents"] = np.array([-1 if n.parent is None else index[id(n.parent)] for n in lp.nodes], dtype=np.int32)
        rec["nodes"] = np.stack([n._xyz_arr for n in lp.nodes]).astype(np.float64)
        rec["rrt_iter"], rec["reachable"] = lp.rrt_iter, np.array(cur["flags"], dtype=np.bool_)
        try:
            s, flags = RS.replay_fixture(rec)
            RS.same_tree(rec, s.n, s.parent, s.nodes_xyz(), s.rrt_iter, flags)
        except Exception as e:
            raise Refused(f"the RRT spec took another turn ({type(e).__name__}: {e})")
        if s.marg.smallest < RS.NEED:
            raise Refused(f"an RRT decision with a margin of {s.marg.smallest:.3g} units")
        if cur["mask"]:
            _, d64 = s.reachable_mask()
            band = np.abs(d64 - lp.step_size) <= 1e-4
            if (all_uncert[band] > 0).any():
                raise Refused("a mask voxel on the edge of the reach carries uncertainty")
        log["rrt"].append((len(rec["parents"]), list(cur["calls"]), list(cur["flags"])))
        cur.clear()

    start_new_plan, run, run_full, get_mask = lp.start_new_plan, lp.run, lp.run_full, lp.get_reachable_mask

    def w_start(start, goal, sdf_map):
        close_plan()
        cur.update(vol=np.asarray(sdf_map, dtype=np.float32), start=np.asarray(start, dtype=np.float64), goal=np.asarray(goal, dtype=np.float64), rows=[], rows_after=[],
                   calls=[], flags=[], mask=False)
        return start_new_plan(start=start, goal=goal, sdf_map=sdf_map)

    def w_run():
        ok = run()
        cur["calls"].append(0); cur["flags"].append(bool(ok)); cur["rows_after"].append(len(cur["rows"]))
        return ok

    def w_full():
        run_full()
        cur["calls"].append(1); cur["rows_after"].append(len(cur["rows"]))

    def w_mask():
        cur["mask"] = True
        return get_mask()
    lp.start_new_plan, lp.run, lp.run_full, lp.get_reachable_mask = w_start, w_run, w_full, w_mask

    # -- the planner's own pieces
    aggregate, search, collide, planning = p.uncertainty_aggregation_v2, p.goal_search_v2, p.detect_collision_v2, p.uncertainty_aware_planning_v2

    def w_aggregate(vols, force_running=False):
        u = np.asarray(vols[0])
        assert np.array_equal(u * 64, np.round(u * 64)) and u.max() < 8
        ok, out = aggregate(vols, force_running=force_running)
        top_k, sub = KEYS["uncert_top_k"], KEYS["uncert_top_k_subset"]
        tgt = np.column_stack(np.unravel_index(np.argpartition(u, -top_k, axis=None)[-sub:], u.shape))
        if ok:
            assert np.array_equal(tgt, out["topk_uncert_vxl"].numpy())
        log["agg_targets"].append(tgt.astype(np.int64)); log["agg_step"].append(p.step)
        return ok, out

    def w_search(out):
        goal_vxl, looks = search(out)
        agg, coll = out["gs_aggre_uncerts"].numpy().reshape(-1), out["gs_uncert_collections"].numpy()
        tgt = out["topk_uncert_vxl"].numpy()
        if (agg == agg.max()).sum() != 1:
            raise Refused("tied maxima in the aggregated volume")
        top = np.sort(coll[int(agg.argmax())])[::-1][:KEYS["obs_per_goal"] + 1]       # (one more: no tie across the cut either)
        pos = top[top > 0]
        if len(np.unique(pos)) != len(pos):
            raise Refused("equal positive values among the winning row's top obs_per_goal (or across the cut)")
        mine = PS.goal_search(agg, coll, tgt, p.goal_space_pts.numpy(), KEYS["obs_per_goal"], BBOX[:, 0], VOXEL)
        goal_vxl = np.array([int(v) for v in goal_vxl], dtype=np.int64)
        assert np.array_equal(mine["goal_vxl"], goal_vxl) and mine["n_lookat"] == len(looks)
        assert all(np.array_equal(a, b) for a, b in zip(mine["lookat_loc"], looks)), (mine, looks, np.sort(coll[mine["goal"]])[-6:])
        log["gs"].append(dict(agg=agg.copy(), coll=coll.copy(), targets=tgt.astype(np.int64), goal_vxl=goal_vxl, looks=np.array(looks, dtype=np.float64).reshape(-1, 3)))
        return goal_vxl, looks

    def w_collide(sdf_vol, cur_pose, next_pt_loc):
        got = collide(sdf_vol=sdf_vol, cur_pose=cur_pose, next_pt_loc=next_pt_loc)
        free = RS.collision_free(p.loc2vox(next_pt_loc), p.loc2vox(cur_pose[:3, 3]), np.asarray(sdf_vol), KEYS["rrt_step_size"], 0.5, marg)
        if marg.smallest < RS.NEED:
            raise Refused(f"a collision segment with a margin of {marg.smallest:.3g} units")
        if dataset == "Replica":
            assert bool(got) == (not free[1])
        log["col_result"].append(bool(got)); log["col_step"].append(p.step)
        return got

    def w_planning(vols, cur_pose):
        out = planning(vols, cur_pose)
        close_plan()
        path = np.array([n._xyz_arr for n in out["path"]], dtype=np.float64).reshape(-1, 3)
        if len(path) > 1 and np.linalg.norm(path[0] - path[-1]) < 1.0:
            raise Refused(f"a plan that starts within a voxel of its goal (step {p.step}: {path[-1]} -> {path[0]})")
        log["plans"].append(dict(step=p.step, reachable=bool(out["is_goal_reachable"]), path=path, looks=np.array(out["lookat_tgts"], dtype=np.float64).reshape(-1, 3),
                                 second_run=log["rrt"][-1][1].count(0) > 1, mask=p.traversability_mask is not None and float(np.min(p.traversability_mask)) == 0.0))
        return out
    p.uncertainty_aggregation_v2, p.goal_search_v2, p.detect_collision_v2, p.uncertainty_aware_planning_v2 = w_aggregate, w_search, w_collide, w_planning

    np.random.seed(seed)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = start_xyz
    start_pose = pose.copy()
    rec = dict(states=[], poses=[], path_len=[], path_xyz=[], lookat_len=[], lookat_xyz=[], is_new_vols=[], vol_id=[])
    for step in range(n_steps):
        p.update_step(step)
        vid = min(step // NEW_VOLS_EVERY, len(versions) - 1)
        is_new = step % NEW_VOLS_EVERY == 0
        new = p.main([versions[vid], sdf], pose, is_new).numpy()
        assert new.dtype == np.float32
        rec["states"].append(PS.STATES.index(p.state)); rec["poses"].append(new); rec["is_new_vols"].append(is_new); rec["vol_id"].append(vid)
        path = np.array([n._xyz_arr for n in (p.path or [])], dtype=np.float64).reshape(-1, 3)
        looks = np.array(p.lookat_tgts or [], dtype=np.float64).reshape(-1, 3)
        rec["path_len"].append(len(path)); rec["path_xyz"].append(path); rec["lookat_len"].append(len(looks)); rec["lookat_xyz"].append(looks)
        pose = new
    names = [PS.STATES[s] for s in rec["states"]]
    if not want(names, log):
        raise Refused(f"not the scene wanted: {[(pl['step'], pl['reachable'], pl['second_run'], pl['mask']) for pl in log['plans']]}, collisions {sum(log['col_result'])}")
    cat = lambda xs, w=3: np.concatenate(xs) if len(xs) else np.zeros((0, w))  # noqa: E731
    out = dict(
        bbox=BBOX, voxel_size=np.float64(VOXEL), dataset=np.array(dataset), seed=np.int64(seed), planner=np.array(json.dumps(KEYS)),
        up_dir=np.array(KEYS["up_dir"]), max_rot_deg=np.float64(KEYS["max_rot_deg"]), start_pose=start_pose, sdf=sdf, uncert_versions=np.stack(versions),
        vol_id=np.array(rec["vol_id"]), is_new_vols=np.array(rec["is_new_vols"]), states=np.array(rec["states"]), poses=np.stack(rec["poses"]),
        path_len=np.array(rec["path_len"]), path_xyz=cat(rec["path_xyz"]), lookat_len=np.array(rec["lookat_len"]), lookat_xyz=cat(rec["lookat_xyz"]),
        agg_targets=np.stack(log["agg_targets"]), agg_step=np.array(log["agg_step"]),
        plan_step=np.array([pl["step"] for pl in log["plans"]]), plan_reachable=np.array([pl["reachable"] for pl in log["plans"]]),
        plan_second_run=np.array([pl["second_run"] for pl in log["plans"]]),
        plan_path_len=np.array([len(pl["path"]) for pl in log["plans"]]), plan_path_xyz=cat([pl["path"] for pl in log["plans"]]),
        plan_lookat_len=np.array([len(pl["looks"]) for pl in log["plans"]]), plan_lookat_xyz=cat([pl["looks"] for pl in log["plans"]]),
        gs_agg=np.stack([g["agg"] for g in log["gs"]]), gs_coll=np.stack([g["coll"] for g in log["gs"]]), gs_targets=np.stack([g["targets"] for g in log["gs"]]),
        gs_goal_vxl=np.stack([g["goal_vxl"] for g in log["gs"]]), gs_lookat_len=np.array([len(g["looks"]) for g in log["gs"]]),
        gs_lookat_xyz=cat([g["looks"] for g in log["gs"]]), goal_idx=p.goal_space_pts.numpy().astype(np.int32),
        col_result=np.array(log["col_result"], dtype=np.bool_), col_step=np.array(log["col_step"], dtype=np.int64),
        sim_dist=np.asarray(sim_dist, dtype=np.float64), sim_invalid=np.asarray(sim_invalid, dtype=np.int64), min_margin=np.float64(marg.smallest))
    states, poses = PS.replay(out)
    assert np.array_equal(states, out["states"]), "planner_spec took another state"
    diff = float(np.abs(poses.astype(np.float64) - out["poses"].astype(np.float64)).max())
    assert diff <= 1e-12, diff
    out["max_abs_diff"] = np.float64(diff)
    return out, names, log


def trajectory(ref, name, out_dir, **kw):
    for seed in range(kw.pop("first_seed", 0), 200):
        try:
            out, names, log = run_trajectory(ref, name, seed=seed, **kw)
        except Refused as e:
            print(f"  {name}: seed {seed} refused: {e}")
            continue
        path = os.path.join(out_dir, f"g14_planner_traj_{name}.npz")
        np.savez_compressed(path, **out)
        runs = "".join(n[0] if n != "movingToGoal" else "m" for n in names)
        print(f"{name}: seed {seed}, {len(names)} steps, states {runs}, plans {[(pl['step'], pl['reachable'], pl['second_run']) for pl in log['plans']]}, "
              f"collisions {int(sum(log['col_result']))} of {len(log['col_result'])}, spec vs reference max abs diff {float(out['max_abs_diff']):.3g}, {os.path.getsize(path)} bytes")
        return
    raise SystemExit(f"{name}: no seed accepted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NARUTO_REFERENCE"), required=os.environ.get("NARUTO_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    ref = load_reference(a.reference)
    only = set(a.only.split(",")) - {""}
    far_wall, near_wall, side_wall, in_chamber = (21, 22, 3, 25, 2, 14), (2, 3, 3, 25, 2, 14), (3, 21, 25, 26, 2, 14), (21, 22, 17, 25, 2, 14)
    room, chamber = _quant(sdf_room()), _quant(sdf_chamber())
    calm = ([1.5], [2])
    todo = {
        "rotations": lambda: rotations(ref[3], ref[4], a.out, default_planner_entries(a.reference)),
        # reaches its first goal directly, looks around, plans again in the mapped room
        "direct": lambda: trajectory(ref, "direct", a.out, dataset="Replica", sdf=room, versions=[[far_wall], [near_wall], [side_wall]],
                                     start_xyz=[0.6, 0.7, 0.6], n_steps=60, sim_dist=calm[0], sim_invalid=calm[1],
                                     want=lambda names, log: log["plans"][0]["reachable"] and len(log["plans"]) >= 2 and "rotatingAtGoal" in names and not any(log["col_result"])),
        # the second goal lies in a sealed chamber: second run(), traversability mask, staying, then a goal the mask leaves.  Without the direct line:
        # the reference's extend_tree_straight counts free steps from the GOAL's side and adds that many nodes from the tree's side, which walks
        # through any wall towards a goal that is itself in free space -- with it no safe goal is ever unreachable
        "mask": lambda: trajectory(ref, "mask", a.out, dataset="MP3D", sdf=chamber,
                                   versions=[[near_wall], [in_chamber, (14, 21, 25, 26, 2, 14)], [in_chamber, (3, 12, 25, 26, 2, 14)]],
                                   start_xyz=[0.6, 0.7, 0.6], n_steps=80, sim_dist=calm[0], sim_invalid=calm[1], overrides=dict(enable_direct_line=False, rrt_max_iter=500),
                                   want=lambda names, log: any(pl["second_run"] and not pl["reachable"] and pl["mask"] for pl in log["plans"])
                                   and log["plans"][-1]["reachable"] and log["plans"][-1]["step"] > [pl["step"] for pl in log["plans"] if pl["mask"]][0]),
        # the simulator reports a surface 1 cm ahead on the fourth move: staying until new volumes arrive
        "collision": lambda: trajectory(ref, "collision", a.out, dataset="NARUTO", sdf=room, versions=[[far_wall], [side_wall], [side_wall], [side_wall], [near_wall]],
                                        start_xyz=[0.6, 0.7, 0.6], n_steps=60, sim_dist=[1.5, 1.5, 1.5, 0.01, 1.5], sim_invalid=[2, 2, 2, 2, 2],
                                        want=lambda names, log: sum(log["col_result"]) == 1 and names.count("planning") >= 2
                                        and "staying" in names[log["col_step"][log["col_result"].index(True)]:]),
    }
    for k, fn in todo.items():
        if not only or k in only:
            fn()


if __name__ == "__main__":
    main()

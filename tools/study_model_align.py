"""The study the model alignment's defaults rest on (naruto_amd.registration.FieldRegistrationHIP; DESIGN 7n prints its table): the room, the
config, the camera and the mapping schedule of tests/test_gpu_odometry.py; the field is mapped FROM THE TRUE POSES over the stop-and-go
trajectory's first 21 frames, so that a true pose is the pose the map is registered to.  Over three viewpoints (frames 3, 8 and 13 of
the trajectory, none of them a keyframe) x eight perturbations from 1 cm / 0.5 degrees to 15 cm / 8 degrees the alignment runs with the
defaults; printed and written: the start's error, the final error, the verdict and every figure of the record.  An estimate is CONVERGED
when it ends within 1.5 cm / 0.75 degrees of the true pose (the tracker's reach per call is 1 cm / 0.57 degrees beyond the field's own
error), else LOST; a lost estimate that passes or a converged one that is refused is counted and named.  Nothing is asserted.

    python tools/study_model_align.py [--out profiles/study_model_align.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import field_registration_spec as FS  # noqa: E402
import test_gpu_odometry as TO  # noqa: E402
from naruto_amd.registration import FieldRegistrationHIP  # noqa: E402
from naruto_amd.slam import CoSLAMNarutoHIP  # noqa: E402

PERTURBATIONS = ((0.01, 0.5), (0.02, 1.0), (0.03, 1.5), (0.05, 2.0), (0.07, 3.0), (0.10, 4.0), (0.12, 6.0), (0.15, 8.0))
VIEWS = (3, 8, 13)
CONVERGED_M, CONVERGED_DEG = 0.015, 0.75


def sig(v):
    """Floats at five significant digits, lists of them too."""
    if isinstance(v, list):
        return [sig(x) for x in v]
    return float(f"{v:.5g}") if isinstance(v, float) and not v.is_integer() else v


def write(path, head, rows):
    """The document with one estimate per line."""
    with open(path, "w") as fh:
        fh.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in head.items()) + ' "rows": [\n')
        fh.write(",\n".join("  " + json.dumps({k: sig(v) for k, v in r.items()}) for r in rows) + "\n ]\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = TO._cfg()
    cfg["tracking"]["disable"] = True
    slam = CoSLAMNarutoHIP(cfg, voxel_size=0.1, active_ray=False, num_frames=TO.N_RUN, seed=3, device=dev)
    cam = {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
    traj = TO._stop_and_go(TO.N_RUN)
    color, depth = TO._sim(dev, cam).simulate_batch(traj)
    for i in range(TO.N_RUN):
        slam.online_recon_step(i, color[i], depth[i], traj[i])
    reg = FieldRegistrationHIP(slam.model, cfg, cam)
    rows, wrong = [], {"lost_but_passed": [], "converged_but_refused": []}
    for v in VIEWS:
        true = traj[v].double().numpy()
        maps = reg.frame_maps(depth[v])
        s, _ = reg.evaluate(maps, true, reg.levels[-1])
        print(f"view {v}: at the true pose {int(s[28])} rows of {int(s[29])} valid points, rmse {np.sqrt(s[27] / max(s[28], 1.0)) * 1e3:.3f} mm")
        for k, (m, deg) in enumerate(PERTURBATIONS):
            start = FS.perturb(true, m, FS.START_ALONG if k % 2 == 0 else (-0.3, 0.8, 0.52), deg, FS.START_AXIS if k % 2 == 0 else (0.0, 1.0, 0.0))
            out = reg.align(maps, start)
            # the free estimate, whatever the verdict: the state's T after a FAIL is the start, so judge the record's own motion instead
            e0, e1 = FS.pose_error(start, true), FS.pose_error(out.T, true)
            converged = bool(e1[0] <= CONVERGED_M and e1[1] <= CONVERGED_DEG) if out.passed else None
            row = {"view": v, "perturbation_m": m, "perturbation_deg": deg, "start_error_mm": e0[0] * 1e3, "start_error_deg": e0[1], "passed": out.passed,
                   "final_error_mm": e1[0] * 1e3, "final_error_deg": e1[1], "record": out.record.tolist(), "status": out.status, "iterations": out.iterations}
            rows.append(row)
            if out.passed and not converged:
                wrong["lost_but_passed"].append([v, m, deg])
            print(f"  {m * 100:5.1f} cm {deg:4.1f} deg: {e0[0] * 1e3:7.2f} mm {e0[1]:6.3f} deg -> {e1[0] * 1e3:7.2f} mm {e1[1]:6.3f} deg  "
                  f"{'PASS' if out.passed else 'FAIL'}  record {np.array2string(out.record, precision=4)} {out.status[1:]} {out.iterations[1:]}", flush=True)
    # a refused estimate: would it have been a converged one?  Run it again with the verdict's motion bounds wide open
    from naruto_amd.registration import RegistrationGate
    free = FieldRegistrationHIP(slam.model, cfg, cam, gate=RegistrationGate(min_overlap=0.0, max_trans=10.0, max_rot_deg=180.0))
    for row in rows:
        if not row["passed"]:
            true = traj[row["view"]].double().numpy()
            k = [p[0] for p in PERTURBATIONS].index(row["perturbation_m"])
            start = FS.perturb(true, row["perturbation_m"], FS.START_ALONG if k % 2 == 0 else (-0.3, 0.8, 0.52), row["perturbation_deg"],
                               FS.START_AXIS if k % 2 == 0 else (0.0, 1.0, 0.0))
            out = free.align(free.frame_maps(depth[row["view"]]), start)
            e = FS.pose_error(free.read_state().transformation, true)
            row["free_estimate_error_mm"], row["free_estimate_error_deg"], row["free_passed"] = e[0] * 1e3, e[1], out.passed
            if e[0] <= CONVERGED_M and e[1] <= CONVERGED_DEG:
                wrong["converged_but_refused"].append([row["view"], row["perturbation_m"], row["perturbation_deg"]])
            print(f"  refused: view {row['view']} {row['perturbation_m'] * 100:.0f} cm: the free estimate ends {e[0] * 1e3:.2f} mm {e[1]:.3f} deg from the true pose")
    print("lost but passed:", wrong["lost_but_passed"], "converged but refused:", wrong["converged_but_refused"])
    if args.out:
        head = {"device": torch.cuda.get_device_name(0), "what": __doc__.split("\n\n")[0], "defaults": {"levels": reg.levels, "iters": reg.iters,
                "sdf_gate": float(reg.desc.sdf_gate), "min_overlap": reg.gate.min_overlap, "max_trans": reg.trunc, "max_rot_deg": reg.gate.max_rot_deg},
                "converged_within": [CONVERGED_M, CONVERGED_DEG], **wrong}
        write(args.out, head, rows)


if __name__ == "__main__":
    main()

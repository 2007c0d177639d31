"""Writes tests/golden/ba_pose_field.npz: the field of the pose-refinement tests (tests/ba_pose_scene.py), mapped on the device from
the TRUE poses of the AnalyticRoom camera ring -- N_KF keyframes + the current frame, 300 first_frame_mapping iterations of 2048 rays,
hash size 12, uncertainty voxel 0.2 (about 0.6 MB).  Needs the GPU; deterministic for a given build.

    python tools/make_ba_pose_fixture.py [OUT.npz]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ba_pose_scene as B  # noqa: E402
from naruto_amd import trainer  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else B.field_path()
    gpu = torch.device("cuda:0")
    c = B.cfg()
    sc = B.scene(c)
    torch.manual_seed(0)
    tr = trainer.MappingTrainer(c, torch.tensor(c["mapping"]["bound"], dtype=torch.float32), gpu, B.UNCERT_VOXEL, fused_adam=True)
    frames = [sc.rays(k, B.N_CAM, H=B.HH, W=B.WW, f=B.FOC) for k in range(B.N_KF + 1)]
    keys = ("rays_o", "rays_d", "target_rgb", "target_d")
    pool = {k: np.concatenate([f[k] for f in frames]) for k in keys}
    rs = np.random.RandomState(0)
    batches = []
    for _ in range(300):
        idx = rs.randint(0, len(pool["target_d"]), 2048)
        batches.append(tuple(torch.from_numpy(pool[k][idx]).to(gpu) for k in keys))
    tr.first_frame_mapping(batches)
    torch.cuda.synchronize()
    arrays = {n: p.detach().cpu().numpy().astype(np.float32) for n, p in B.hip_params(tr.model).items()}
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes; last loss", float(tr._train_steps[next(iter(tr._train_steps))].losses[9]))


if __name__ == "__main__":
    main()

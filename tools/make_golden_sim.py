"""Record tests/golden/g13_c2e.npz from the REFERENCE's own cube-to-panorama layer and depth-to-distance conversion, on the CPU.

    python tools/make_golden_sim.py --reference /path/to/the/reference/checkout

Imported from the reference, not edited: src.layers.c2e.C2E and src.layers.erp_conversions.depth2dist (both run with device 'cpu').
Only data is recorded.  For (face_w, h, w) in (8, 16, 32) and (5, 12, 24), with the key suffix _<face_w>:
  index   int32 [h,w]        C2E.forward(mode='nearest') of the cube arange(6*s*s): which cube word every panorama pixel reads
  cube    float32 [2,6,s,s]  a random two-channel cube (seeded)
  pano    float32 [2,h,w]    C2E.forward of it
  grid    float32 [h,w,3]    the layer's normalised sampling grid (x, y, face)
and for face_w = 8:
  depth   float32 [6,8,8]    random depths in [0.5, 3.5] (seeded)
  dist    float32 [6,8,8]    depth2dist with K = diag(4, 4, 1, 1) + principal point (4, 4)
  K       float32 [4,4]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((8, 16, 32), (5, 12, 24))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("NARUTO_REFERENCE"), required=os.environ.get("NARUTO_REFERENCE") is None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g13_c2e.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    from src.layers.c2e import C2E
    from src.layers.erp_conversions import depth2dist

    rng = np.random.RandomState(13)
    rec = {}
    for s, h, w in SHAPES:
        layer = C2E(s, h, w)
        ids = torch.arange(6 * s * s, dtype=torch.float32).reshape(1, 1, 6, s, s)
        index = layer(ids, mode="nearest")[0, 0, 0].numpy()
        assert np.array_equal(index, np.round(index)) and index.min() >= 0 and index.max() < 6 * s * s
        cube = rng.uniform(-1.0, 1.0, (2, 6, s, s)).astype(np.float32)
        pano = layer(torch.from_numpy(cube)[None], mode="nearest")[0, :, 0].numpy()
        assert np.array_equal(pano, cube.reshape(2, -1)[:, index.astype(np.int64)])
        rec[f"index_{s}"] = index.astype(np.int32)
        rec[f"cube_{s}"], rec[f"pano_{s}"] = cube, pano.astype(np.float32)
        rec[f"grid_{s}"] = layer.grid.detach()[0, 0].numpy().astype(np.float32)
    s = 8
    depth = rng.uniform(0.5, 3.5, (6, s, s)).astype(np.float32)
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = K[0, 2] = K[1, 2] = s / 2
    dist = depth2dist(torch.from_numpy(depth)[:, None], torch.from_numpy(K)[None].repeat(6, 1, 1))[:, 0].numpy()
    rec["depth_8"], rec["dist_8"], rec["K_8"] = depth, dist.astype(np.float32), K
    np.savez_compressed(a.out, **rec)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes; " + ", ".join(f"{k}{tuple(v.shape)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()

"""The depth-ordered walk (k_query_fwd_loss<*, true>, k_query_fwd_loss_img) gathers a ray's first tile at a priority that depends on the ray: a ray
whose 64th depth is not beyond measured depth + truncation, or that has no measured depth, needs its second tile whatever the field says and keeps
the top priority; the others step down (NARUTO_FWD_SHORT_RAY_PRIO).  Priority is not arithmetic: every class of ray must come out of the walk as it
comes out of the flat forward (NARUTO_DEBUG_NO_EARLY_EXIT=1: plain 64-point tiles over all samples, the loss stage in a launch of its own).

One workgroup's worth and a bit -- 9 rays x 128 samples, perturb off -- with the classes mixed over the wave slots of consecutive workgroups (wave w of
one workgroup shares its SIMD with wave w of the other workgroup on its compute unit): short, long, no depth, and two rays whose measured depths are
NEIGHBOURING floats on either side of the class boundary.  Both MLP modes.  Each launch structure is chosen once per process, so the two forwards
run in fresh interpreters, as in test_short_and_partial_walk_forwards_equal_the_flat_one, whose bound (2e-5 of the array's scale: OneBlob's closed
against its dense form) is the one used here; in the exact mode the losses, maps, sums and gradients are also held to test_launch_variants_give_the_same_bits'
equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import helpers as H
from naruto_amd import ops, synthetic as syn
gpu = torch.device("cuda", 0)
cfg = H.office_cfg(12, perturb=0.0, n_samples_d=117)                 # 117 + 11 = 128 samples: two tiles per ray
cfg["decoder"]["mlp_precision"] = sys.argv[3]
tr, cam = cfg["training"], cfg["cam"]
ora = H.make_oracle(cfg, 0.25, 23)
m = H.make_hip_from_oracle(cfg, ora, gpu)
N, S = 9, 128
f32 = np.float32
trunc_sc = f32(tr["trunc"]) * f32(cfg["data"]["sc_factor"])

def stops_after_tile0(td):
    # the walk's a-priori test on the depths this ray gets (no jitter): z[63] beyond measured depth + truncation + ee_lane_live's margin
    z = ops.sample_z(1, torch.tensor([td], device=gpu), cam["near"], cam["far"], tr["n_samples_d"], tr["n_range_d"], tr["range_d"]).cpu().numpy()[0]
    lim = f32(td) + trunc_sc
    return bool(z[63] > lim + f32(1e-5) * abs(lim) + f32(1e-6)), float(z[63])

lo, hi = f32(0.6), f32(2.6)                                          # short (stops), long (cannot stop)
assert stops_after_tile0(lo)[0] and not stops_after_tile0(hi)[0]
while np.nextafter(lo, hi) < hi:                                     # two neighbouring floats with different answers
    mid = f32(0.5) * (lo + hi)
    if stops_after_tile0(mid)[0]: lo = mid
    else: hi = mid
assert np.nextafter(lo, f32(10.0)) == hi
td = np.array([0.6, 2.6, 0.0, hi,   3.0, 0.9, lo, 0.0,   0.7], dtype=f32)      # workgroups of four rays: a slot's class changes from one to the next
rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=23)
rays["target_d"] = td.reshape(np.asarray(rays["target_d"]).shape)
w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.1, 0.0])
ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                   near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                   perturb=False, loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=True, seed=5)
args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(td).to(gpu).contiguous()]
for _ in range(2):
    losses = ts.run(*args).clone()
torch.cuda.synchronize()
out = {"losses": losses.cpu().numpy(), "rgb": ts.rgb.cpu().numpy(), "depth": ts.depth.cpu().numpy(), "sums": ts.sums.cpu().numpy()[:10],
       "raw": ts.raw.cpu().numpy(), "feat": ts.feat.cpu().numpy(), "z_vals": ts.z_vals.cpu().numpy(), "td": td, "trunc_sc": np.array([trunc_sc])}
out.update({"g_" + k: v.detach().cpu().numpy() for k, v in ts.grads.items()})
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("mlp", ["fp32", "bf16"])
def test_every_class_of_ray_walks_to_the_flat_forwards_values(gpu, tmp_path, mlp):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "walk_classes.py"
    script.write_text(_SCRIPT)
    res = []
    for k, env in enumerate(({}, {"NARUTO_DEBUG_NO_EARLY_EXIT": "1"})):
        out = tmp_path / f"{mlp}_{k}.npz"
        e = dict(os.environ)
        e.pop("NARUTO_DEBUG_NO_EARLY_EXIT", None)
        e.update(env)
        subprocess.run([sys.executable, str(script), root, str(out), mlp], check=True, env=e, timeout=300)
        res.append(dict(np.load(out)))
    walk, flat = res
    N, S = 9, 128
    # the batch holds every class: by the depths the run used, with the walk's own test
    td, z63 = walk["td"], walk["z_vals"].reshape(N, S)[:, 63]
    lim = td + walk["trunc_sc"][0]
    stops = z63 > lim + np.float32(1e-5) * np.abs(lim) + np.float32(1e-6)
    print(f"{mlp}: measured depths {td.tolist()}; z[63] {z63.tolist()}; may stop after tile 0: {stops.tolist()}")
    assert np.array_equal(walk["z_vals"], flat["z_vals"])
    assert (td == 0).sum() == 2 and stops[[0, 5, 8]].all() and not stops[[1, 4]].any()
    assert np.nextafter(td[6], np.float32(10.0)) == td[3] and td[6] > 0.6 and td[3] < 2.6
    # what the walk evaluated is a prefix of every ray and holds at least the first tile; the long rays and the rays without a depth hold more
    ev = np.abs(walk["raw"].reshape(N, S, 5)).sum(-1) > 0
    n_ev = ev.sum(1)
    assert all(ev[r, :n_ev[r]].all() for r in range(N)) and (n_ev >= 64).all() and (n_ev[[1, 4]] > 64).all()
    print(f"{mlp}: samples evaluated per ray {n_ev.tolist()}")
    for k in walk:
        if k in ("td", "trunc_sc", "z_vals"):
            continue
        a, b = walk[k].astype(np.float64), flat[k].astype(np.float64)
        if k == "raw":                       # behind the walk's band raw is zeros by construction; the flat forward evaluates every sample
            a, b = a.reshape(N, S, 5)[ev], b.reshape(N, S, 5)[ev]
        if k == "feat":                      # saved features [16][N * S][2]: the backward reads the evaluated samples' only
            a, b = a.reshape(16, N * S, 2)[:, ev.reshape(-1)], b.reshape(16, N * S, 2)[:, ev.reshape(-1)]
        scale = float(np.abs(b).max()) + 1e-30
        d = float(np.abs(a - b).max())
        print(f"{mlp}: {k}: max distance {d:.3e} at scale {scale:.3e}")
        assert d <= 2e-5 * scale, f"{mlp}: {k} differs by {d:.3e} at scale {scale:.3e}"
        if mlp == "fp32" and k not in ("raw", "feat"):
            assert np.array_equal(walk[k], flat[k], equal_nan=True), f"{k}: the walk and the flat forward differ in the exact mode"

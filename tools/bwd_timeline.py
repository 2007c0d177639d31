"""Per-phase timeline of the fp32 MLP backward's tile loop (k_query_bwd): while naruto_debug_bwd_timeline holds a buffer the backward launches the
stamped build of the kernel, in which every WAVE sums the 100 MHz global counter per phase of its tiles and stamps the kernel's own four events.
Printed: the mean time per tile and phase with its share of the tile, split by how many tiles a wave ran, and the kernel's prologue / epilogue.
A stamp drains the wave's LDS traffic and fences the scheduler, so the stamped build is slower than the product kernel: read the shares.
    python tools/bwd_timeline.py [workload] [training steps before the stamped one: 600 = the state bench.py's timed region sees]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
from naruto_amd import _lib
from naruto_amd.trainer import MappingTrainer

wl = sys.argv[1] if len(sys.argv) > 1 else "office0_2048x128"
n_warm = int(sys.argv[2]) if len(sys.argv) > 2 else 600
dev = torch.device("cuda:0")
cfg, n_rays = bench.workload(wl)
cfg["decoder"]["mlp_precision"] = "fp32"
torch.manual_seed(0)
tr = MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32), dev, 0.1, fused_adam=True)
rays = {k: torch.from_numpy(v).to(dev) for k, v in bench.bench_rays(cfg, n_rays).items()}
step = lambda: tr.step(rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"], smooth=True)
for _ in range(n_warm):
    step()
SLOTS, WAVES, MAX_BLOCKS = 16, 4, 512
buf = torch.zeros(SLOTS * WAVES * MAX_BLOCKS, dtype=torch.int64, device=dev)
lib = _lib.load()
lib.naruto_debug_bwd_timeline(buf.data_ptr())
step()
torch.cuda.synchronize()
lib.naruto_debug_bwd_timeline(None)
t = buf.cpu().numpy().reshape(-1, SLOTS).astype(np.float64)
t = t[t[:, 8] > 0]                                  # waves of the workgroups that ran
ts = tr._train_step(n_rays, True)
n_active = int(ts.n_active.item()) if getattr(ts, "n_active", None) is not None else -1
tiles = t[:, 7].astype(int)
us = lambda ticks: ticks / 100.0
t0 = t[:, 8].min()
print(f"{wl}, fp32, after {n_warm} training steps: {n_active} active samples, {tiles.sum()} tiles on {len(t)} waves "
      f"({', '.join(f'{int((tiles == k).sum())} waves x {k}' for k in sorted(set(tiles)))})")
print(f"kernel (us after the first wave's start): weight image in LDS p50 {np.percentile(us(t[:, 9] - t0), 50):.2f} max {us(t[:, 9] - t0).max():.2f} | "
      f"tile loop ends p50 {np.percentile(us(t[:, 10] - t0), 50):.2f} max {us(t[:, 10] - t0).max():.2f} | end p50 {np.percentile(us(t[:, 11] - t0), 50):.2f} max {us(t[:, 11] - t0).max():.2f}")
print(f"epilogue (cross-wave sum + partial write) per wave: mean {us(t[:, 11] - t[:, 10]).mean():.2f} us")
names = ["inputs ready", "layer-0 recompute", "OneBlob + colour recompute", "colour backward + dW(col_w0)", "dW(sdf_w1)", "dW(sdf_w0)", "dgrad to features + stores"]
for sel_name, sel in [("all waves", tiles > 0)] + [(f"waves with {k} tiles", tiles == k) for k in sorted(set(tiles)) if k > 0]:
    if not sel.any():
        continue
    per_tile = us(t[sel, :7]) / tiles[sel, None]
    tot = per_tile.sum(axis=1)
    print(f" {sel_name} ({int(sel.sum())}): {tot.mean():.2f} us per tile (p10 {np.percentile(tot, 10):.2f}, p90 {np.percentile(tot, 90):.2f})")
    for k, nm in enumerate(names):
        v = per_tile[:, k]
        print(f"   {nm:30s} mean {v.mean():6.2f} us  {100.0 * v.mean() / tot.mean():5.1f} %   p10 {np.percentile(v, 10):6.2f}  p90 {np.percentile(v, 90):6.2f}")

#!/usr/bin/env python3
"""Headline benchmark: rendered rays/s of one NARUTO mapping iteration ("train step") on MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): Replica office_0 volume, 2048 rays x 128 samples per GPU, hash grid
L=16 F=2 T=2^16, MLPs 2x32, uncertainty grid on; synthetic rays (seeded), random-init weights.
One step = the iteration body of the reference's global_BA (reference src/slam/coslam/coslam.py:361-399):
zero_grad -> forward (z sampling with jitter, hash gather, MLPs, compositing, uncertainty aggregation,
five losses + smoothness term) -> backward -> Adam on decoder + hash table (+ uncertainty-grid Adam every
5th iteration).  N > 1: one process per GPU, every rank renders its own 2048-ray shard of a 2048*N batch
(weak scaling), the loss sums and the flat gradient are all-reduced over RCCL.

Prints ONE JSON line on rank 0 (see the driver contract).  A plain run sets up, warms up, times the K steps and prints
the line (metric, value, unit, ms_per_step, ...).  --full adds what takes runs of its own (each can be left out with
its --no-* option):
  roofline     -- the dominant kernel's algorithmic rate against the roof that bounds it, from HIP events on
                  the launch stream around K launches of that kernel (the per-kernel table is in "kernels");
  dropin, mapping_iter, ms_per_step_median_of_5_chunks -- the reference's unchanged loop body, the BA iteration
                  end to end, the step time as the median over five further chunks;
  cpu_baseline -- the oracle's (CPU PyTorch restatement, oracle/spec_torch.py) identical mapping iteration on
                  this host's cores, on a bounded sample.
--dump-outputs DIR writes what the timed path computed in its last step as DIR/<name>.npy (see dump_outputs).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

# multi-process GPU work on this pool needs dmabuf IPC (the host driver has no legacy IPC): RCCL's peer-to-peer setup
# fails with "hipIpcGetMemHandle: invalid argument" otherwise.  Already exported on the boxes; kept here for any other launcher.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from naruto_amd import config as C  # noqa: E402
from naruto_amd import parallel, synthetic as syn  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
FP32_MFMA_PEAK_TF = 157.3      # v_mfma_f32_32x32x2_f32 peak = fp32 vector peak
BF16_MFMA_PEAK_TF = 2500.0     # v_mfma_f32_32x32x16_bf16 dense peak (MI355X_MICROARCH.md; AMD's 5 PF figure includes 2:1 sparsity)
L2_PEAK_GBS = 34500.0          # aggregate L2 bandwidth (MI355X_MICROARCH.md, "L2 (per XCD)")


WORKLOADS = {
    # name: (config factory, rays per GPU (weak) or rays per job (strong), BASELINE.json config it is)
    "office0_2048x128": (lambda: C.office0_config(perturb=1.0, n_samples_d=117), 2048, "configs[1]"),
    "office0_2048x43": (lambda: C.office0_config(perturb=1.0), 2048, "configs[1] with the shipped 32+11 sampling"),
    "office0_8192x43": (lambda: C.office0_config(perturb=1.0), 8192, "configs[2] (train step at the planner batch size)"),
    "office0_8192x43_eval": (lambda: C.office0_config(perturb=1.0), 8192, "configs[2] (uncertainty head on, planner query path: eval render + dense lattice query)"),
    "mp3d_2048x256": (lambda: C.mp3d_large_config(perturb=1.0, n_samples_d=245), 2048, "configs[3], one GPU's shard"),
    "mp3d_16384x256": (lambda: C.mp3d_large_config(perturb=1.0, n_samples_d=245), 16384, "configs[3], the whole batch (use --scaling strong)"),
    # configs[4]: 2^20 rays over 8 GPUs = 131072 per GPU, unit cube, finest level 1024^3.  T16: the shipped table size (7 MB,
    # cache resident); T22: 2^22 entries per hashed level, 281 MB -- the HBM-resident table
    "unit1024_131072x43": (lambda: C.unit_cube_config(1024, 16, perturb=1.0), 131072, "configs[4] at T=2^16"),
    "unit1024_T22_131072x43": (lambda: C.unit_cube_config(1024, 22, perturb=1.0), 131072, "configs[4] at T=2^22 (HBM-resident table)"),
    "unit1024_T22_16384x43": (lambda: C.unit_cube_config(1024, 22, perturb=1.0), 16384, "configs[4] at T=2^22, reduced ray count"),
    # the metric's second half: "mapping-iter ms" = one global_BA iteration END TO END (coslam.py:310-399): keyframe-store draw + pose
    # transform (N2) -> active ray selection (N1, --active-ray) -> training step, shipped sampling, the reference's ray count
    "office0_ba_iter": (lambda: C.office0_config(perturb=1.0), 2148, "metric 'mapping-iter ms': one global_BA iteration end to end, 2048 + max(2048 // n_kf, 100) rays x (32 + 11)"),
}


# what "f32" means on this path since round 5: every value is fp32 in memory and in the reference's sense; the MLP forward's products are formed
# from EXACT three-way bf16 splits of the fp32 operands on the bf16 matrix pipe (six partial products, fp32 accumulation: one fp32 rounding
# per product, tests/test_gpu_parity.py::test_x3_chain_against_the_fp32_chain bounds the two chains at full size), the backward runs fp32 MFMA
DTYPE_F32 = "f32 (MLP forward products as exact bf16x3 splits on the bf16 MFMA, fp32 accumulate; backward fp32 MFMA; everything else fp32)"


def workload(name: str):
    if name not in WORKLOADS:
        raise SystemExit(f"unknown workload {name}; choose from {sorted(WORKLOADS)}")
    make, n_rays, _ = WORKLOADS[name]
    return make(), n_rays


def events_ms(fn, iters: int) -> float:
    """Average duration of fn() in ms, HIP events on the current (= launch) stream."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_table(tr, rays, cfg, iters: int):
    """Per-kernel average durations + algorithmic work, each measured alone on the launch stream."""
    import ctypes as CT
    from naruto_amd import _lib, ops
    lib = _lib.load()
    m = tr.model
    h = m._handle()
    dev = rays["rays_o"].device
    N = rays["rays_o"].shape[0]
    trc, cam = cfg["training"], cfg["cam"]
    S = trc["n_samples_d"] + trc["n_range_d"]
    M = N * S
    rand = torch.rand(N, S, device=dev)
    z = ops.sample_z(N, rays["target_d"], float(cam["near"]), float(cam["far"]), trc["n_samples_d"], trc["n_range_d"],
                     float(trc["range_d"]), rand=rand)
    params = {k: v.detach() for k, v in m._params().items()}
    ps = ops._params_struct(params)
    pts, _ = ops._points_struct(None, rays["rays_o"], rays["rays_d"], z)
    raw = torch.empty(M, 5, device=dev)
    feat = torch.empty(16, M, 2, device=dev)
    st = lambda: ops._stream()
    p = ops._p
    rows = []

    def add(name, fn, bytes_, flops, bound):
        ms = events_ms(fn, iters)
        rows.append({"kernel": name, "ms": round(ms, 5), "alg_bytes": int(bytes_), "alg_flops": int(flops),
                     "GBps": round(bytes_ / ms / 1e6, 1), "TFLOPs": round(flops / ms / 1e9, 3), "bound": bound})

    # algorithmic work per sample: 16 levels x 8 corners x 8 B gathered + 32 B uncert corners
    gather = 16 * 8 * 8 + 32
    mlp_fwd = 2 * (80 * 32 + 32 * 16 + 63 * 32 + 32 * 3)          # 10 368 FLOP
    add("k_sample_z", lambda: _lib.check(lib.naruto_sample_z(N, p(rays["target_d"]), float(cam["near"]), float(cam["far"]),
        trc["n_samples_d"], trc["n_range_d"], float(trc["range_d"]), 0, p(rand), p(z), st())), N * S * 8 + N * 4, 0, "hbm")
    # k_query_fwd: SURVEY.md 8(d) "render inference, per ray of S samples: S x 1056 B gathered + 28 B in + 36 B out"; the launch
    # also streams per sample 4 B of depth in, 20 B of raw out and 128 B of saved hash features (training only) -- kept as a
    # second figure ("alg_bytes_incl_saved"), never as the roofline's
    add("k_query_fwd<color>", lambda: _lib.check(lib.naruto_query_fwd(h.ptr, CT.byref(ps), M, CT.byref(pts), p(raw), None, None,
        p(feat), st())), M * gather + N * 64, M * mlp_fwd, "hbm")
    rows[-1]["alg_bytes_incl_saved"] = int(M * (gather + 4 + 20 + 128) + N * 24)
    rows[-1]["launch"] = "all samples (flat 64-sample tiles)"
    rgb = torch.empty(N, 3, device=dev)
    outs = [torch.empty(N, device=dev) for _ in range(5)]
    add("k_composite_fwd", lambda: _lib.check(lib.naruto_composite_fwd(h.ptr, N, S, p(raw), p(z), p(rgb), p(outs[0]), p(outs[1]), None,
        p(outs[2]), p(outs[3]), p(outs[4]), st())), M * 24 + N * 32, 0, "hbm")
    sums = torch.empty(16, dtype=torch.float64, device=dev)
    losses = torch.empty(8, device=dev)
    ws = torch.empty(N * 16, device=dev)
    tgt, td = rays["target_rgb"], rays["target_d"].reshape(-1)
    add("k_loss_terms+reduce", lambda: _lib.check(lib.naruto_loss_sums(h.ptr, N, S, p(raw), p(z), p(rgb), p(outs[2]), p(outs[4]), p(tgt), p(td),
        float(cam["depth_trunc"]), float(trc["rgb_missing"]), p(sums), p(losses), p(ws), st())), M * 8 + N * 100, 0, "hbm")
    gl = torch.tensor([trc["rgb_weight"], trc["depth_weight"], trc["sdf_weight"], trc["fs_weight"], 0.0, trc["uncert_weight"]],
                      dtype=torch.float32, device=dev)
    d_raw = torch.empty(M, 5, device=dev)
    cnt, off = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    act, nact = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    add("k_composite_bwd<loss>", lambda: _lib.check(lib.naruto_loss_bwd(h.ptr, N, S, p(raw), p(z), p(tgt), p(td), float(cam["depth_trunc"]),
        float(trc["rgb_missing"]), p(sums), N, p(gl), p(d_raw), p(cnt), st())), M * 44 + N * 20, 0, "hbm")
    add("k_compact_active", lambda: _lib.check(lib.naruto_compact_active(N, S, p(cnt), p(off), p(act), p(nact), st())), M * 4 + N * 8, 0, "hbm")
    frac = float(nact.item()) / M
    grads = {k: torch.zeros_like(v) for k, v in params.items()}
    gs = _lib.NarutoGrads()
    for k, v in grads.items():
        setattr(gs, k, p(v))
    wsb = torch.empty(lib.naruto_query_bwd_workspace(h.ptr, M) // 4, device=dev)
    # the three kernels of naruto_query_bwd, split by giving each call only the outputs one kernel produces
    gs_mlp = _lib.NarutoGrads()                 # k_query_bwd alone: no table / uncertainty grid (scatter), no weight outputs (k_wgrad_reduce)
    Ma = int(round(frac * M))                                                           # active (non-zero cotangent) samples
    mlp_bwd_flops = Ma * 2 * (5184 + (15 * 32 + 16 * 32 + 32 * 32 + 3 * 32) + 5184)   # recompute + dgrad + wgrad
    add("k_query_bwd", lambda: _lib.check(lib.naruto_query_bwd(h.ptr, CT.byref(ps), M, CT.byref(pts), p(feat), p(d_raw), None,
        p(act), p(nact), None, 0, CT.byref(gs_mlp), p(wsb), st())), Ma * (128 + 20 + 128 + 4 + 4) + N * 24, mlp_bwd_flops, "mfma")
    t_mlp = rows[-1]["ms"]
    ms_all = events_ms(lambda: _lib.check(lib.naruto_query_bwd(h.ptr, CT.byref(ps), M, CT.byref(pts), p(feat), p(d_raw), None, p(act), p(nact),
                                                               None, 0, CT.byref(gs), p(wsb), st())), iters)
    sc_bytes = Ma * (16 * 8 * 2 * 8 + 128 + 12)         # 256 fp32 read-modify-writes + d_feat + point
    ms_sc = max(ms_all - t_mlp, 1e-6)
    rows.append({"kernel": "k_hash_scatter+reduce+k_wgrad_reduce", "ms": round(ms_sc, 5), "alg_bytes": int(sc_bytes), "alg_flops": 0,
                 "GBps": round(sc_bytes / ms_sc / 1e6, 1), "TFLOPs": 0.0, "bound": "hbm"})
    # the two calls the trainer actually makes per iteration (naruto_train.hip), for reference: not roofline rows
    ts = tr._train_step(N, True)
    args = (rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"].reshape(-1))
    ts.run_forward(*args)                      # the two halves WITHOUT the collective in between: this runs on rank 0 only
    ts.run_backward()
    t = ts.t
    t.rays_o, t.rays_d, t.target_rgb, t.target_d = (p(a) for a in args)
    fwd_ms = events_ms(lambda: _lib.check(lib.naruto_train_forward(h.ptr, CT.byref(ts.ps), CT.byref(t), 1, st())), iters)
    bwd_ms = events_ms(lambda: _lib.check(lib.naruto_train_backward(h.ptr, CT.byref(ts.ps), CT.byref(t), CT.byref(ts.gs), ts.flags, None, st())), iters)
    # the field query in the launch shape the ITERATION uses (one wave per ray, depth-ordered early termination when S % 64 == 0)
    qit_ms = events_ms(lambda: _lib.check(lib.naruto_debug_train_query_fwd(h.ptr, CT.byref(ts.ps), CT.byref(t), st())), iters)
    # the table scatter in the launch shape the ITERATION uses: k_hash_scatter_lds alone over the list the backward above left behind
    # (smoothness lattice + active samples; level units + uncertainty-grid units).  Algorithmic bytes: SURVEY 8(d) counts the
    # backward as a read-modify-write of the gather term -- per list point 2 x (16 levels x 8 corners x 8 B), per active sample
    # 2 x 32 B of uncertainty-grid corners -- plus what the launch streams in per list point: 128 B of feature cotangents, 16 B of
    # position + raw[...,4] cotangent.  Fields with binned levels (T > 2^17) spread the scatter over five kernels: no such row.
    n_act = int(ts.n_active.item())
    n_lat = (int(trc["smooth_pts"]) - 1) ** 3
    if lib.naruto_debug_train_scatter(h.ptr, CT.byref(ts.ps), CT.byref(t), st()) == 0:
        sc_it_ms = events_ms(lambda: _lib.check(lib.naruto_debug_train_scatter(h.ptr, CT.byref(ts.ps), CT.byref(t), st())), iters)
        sc_it_bytes = (n_act + n_lat) * (2 * 16 * 8 * 8 + 128 + 16) + n_act * 2 * 32
        rows.append({"kernel": "k_hash_scatter_lds as launched by the iteration", "ms": round(sc_it_ms, 5), "alg_bytes": int(sc_it_bytes), "alg_flops": 0,
                     "GBps": round(sc_it_bytes / sc_it_ms / 1e6, 1), "TFLOPs": 0.0, "bound": None, "list_points": n_act + n_lat, "active_samples": n_act,
                     "alg_bytes_all_samples": int((M + n_lat) * (2 * 16 * 8 * 8 + 128 + 16) + M * 2 * 32)})
    for name, ms in (("naruto_train_forward (eager)", fwd_ms), ("naruto_train_backward (eager)", bwd_ms),
                     ("k_query_fwd<color> as launched by the iteration (with the loss stage in the same launch when S % 64 == 0)", qit_ms)):
        rows.append({"kernel": name, "ms": round(ms, 5), "alg_bytes": 0, "alg_flops": 0, "GBps": 0.0, "TFLOPs": 0.0, "bound": None})
    # what the iteration's forward launch actually evaluates: samples behind the end of a ray's band are skipped and their raw written as
    # zeros (depth-ordered early termination) -- counted from the raw the launch above left (an evaluated sample's sdf is 0.0 with
    # probability nil), charged SURVEY 8(d)'s 1 056 B each + 64 B per ray
    try:
        raw_t = ts.raw.reshape(N, S, 5)
        n_eval = int((raw_t.abs().sum(dim=-1) > 0).sum().item())
        it_bytes = n_eval * (16 * 8 * 8 + 32) + N * 64
        rows[-1].update({"evaluated_samples": n_eval, "samples": int(M), "alg_bytes": int(it_bytes), "GBps": round(it_bytes / qit_ms / 1e6, 1)})
    except Exception:
        pass
    rows.append({"kernel": "(active sample fraction)", "ms": 0.0, "alg_bytes": 0, "alg_flops": 0, "GBps": 0.0, "TFLOPs": 0.0,
                 "bound": "hbm", "fraction": round(frac, 4)})
    return rows


def pmc_profile(workload_name: str, kernel: str):
    """Per-launch PMC figures of ``kernel`` from the committed passes (profiles/rNN_pmc.json, newest round; collected by
    tools/profile_round.sh: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, eager launches), or ({}, None).
    The file is keyed by workload (older rounds: by kernel only = the default workload)."""
    import glob
    here = os.path.dirname(os.path.abspath(__file__))
    for f in sorted(glob.glob(os.path.join(here, "profiles", "r*_pmc.json")), reverse=True):
        try:
            d = json.load(open(f))
        except (ValueError, OSError):
            continue
        d = d.get(workload_name, d if workload_name == "office0_2048x128" else {})
        if isinstance(d.get(kernel), dict):
            return d[kernel], os.path.basename(f)
    return {}, None


def physical_cores() -> int:
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n)
    except Exception:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def cpu_baseline(cfg, n_rays: int, device=None, budget_s: float = 30.0):
    """The oracle's mapping iteration (plain PyTorch ops; oracle/spec_torch.py, pinned against the reference by
    oracle/make_golden.py), same body as the timed GPU step: forward + losses + smoothness + backward + Adam.

    Host (the reported ``cpu_baseline``): the thread count is swept FIRST (on the cheap shipped sampling), then the
    TIMED WORKLOAD ITSELF (its own samples per ray) runs at the best count: 5 warm-ups, median of 20 iterations, bounded to
    ~``budget_s`` of CPU work by shrinking the iteration count, never the workload; the shipped 32 + 11 sampling is a second field.
    ``device`` given: the same oracle as unfused torch ops on the GPU -- the stand-in for "the reference in single-GPU PyTorch"
    (the reference itself needs the CUDA-only tiny-cuda-nn)."""
    import copy
    from oracle import spec_torch as S
    on_gpu = device is not None
    dev = device if on_gpu else torch.device("cpu")
    n_threads_before = torch.get_num_threads()

    def build(c):
        torch.manual_seed(0)
        bbox = torch.tensor(c["mapping"]["bound"], dtype=torch.float32)
        ora = S.OracleField(c, bbox, 0.1).to(dev)
        g1, g2 = ora.param_groups()
        o_map = torch.optim.Adam(g1, betas=(0.9, 0.99))
        o_unc = torch.optim.Adam(g2, lr=1)
        rays = {k: torch.from_numpy(v).to(dev) for k, v in bench_rays(c, n_rays).items()}
        trc = c["training"]
        ora.train()

        def step(i):
            o_map.zero_grad()
            ret = ora.forward(rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"])
            sm = S.smoothness(ora, trc["smooth_pts"], trc["smooth_vox"], trc["smooth_margin"], torch.rand(3).to(dev), torch.rand(3).to(dev))
            S.total_loss(ret, trc, smooth_term=sm).backward()
            o_map.step()
            if (i + 1) % 5 == 0:
                o_unc.step()
                o_unc.zero_grad()
            if on_gpu:
                torch.cuda.synchronize()
        return step

    def timed(step, warm, iters):
        for i in range(warm):
            step(i)
        ts = []
        for i in range(iters):
            t0 = time.perf_counter()
            step(warm + i)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts

    trc = cfg["training"]
    S_tot = trc["n_samples_d"] + trc["n_range_d"]

    def stats(ts):
        med = float(np.median(ts))
        p10, p90 = (float(np.percentile(ts, q)) for q in (10, 90))
        return med, ((p90 - p10) / med if med > 0 else 0.0), ((max(ts) - min(ts)) / med if med > 0 else 0.0)

    if on_gpu:
        # the unfused iteration is ~600 small launches: it runs at the speed of the HOST, and with torch's default of one intra-op thread
        # per core (128 here) its few CPU-side ops stall for milliseconds at a time -- eight threads, as for the drop-in figures
        torch.set_num_threads(min(8, n_threads_before))
        step = build(cfg)
        for i in range(3):
            step(i)                                      # cold: allocator, kernel selection
        med, ts = timed(step, 5, 25)
        med, idr, full = stats(ts)
        torch.set_num_threads(n_threads_before)
        return {"value": round(n_rays / med, 1), "unit": "rays/s", "kind": "port, unfused torch ops on the same GPU", "host_threads": min(8, n_threads_before),
                "sample": f"median of 25 mapping iterations after 8 warm-ups, {n_rays} rays x {S_tot} samples (oracle/spec_torch.py: forward + losses + smoothness + "
                          f"backward + Adam), {med * 1e3:.1f} ms/iter, spread (p90 - p10) / median {idr * 100:.0f} %, (max - min) / median {full * 100:.0f} %"}

    # 1. thread count FIRST (many-core hosts: torch's CPU kernels stop scaling -- and fall back -- well before all cores: 128 threads
    #    measured 4x SLOWER than 16 on the MI355X hosts), on the cheap shipped sampling (32 + 11 samples per ray), ascending, stopping
    #    once a count is clearly past the optimum so that the sweep never runs the slow many-thread configurations
    c43 = copy.deepcopy(cfg)
    c43["training"]["n_samples_d"], c43["training"]["n_range_d"] = 32, 11
    step43 = build(c43)
    torch.set_num_threads(min(16, physical_cores()))
    step43(0)                                           # cold
    cand = sorted({n for n in (8, 16, 32, 64, physical_cores()) if n <= physical_cores()})
    best, res = None, []
    for n in cand:
        torch.set_num_threads(n)
        m_, _ = timed(step43, 1, 2)
        res.append(f"{n}: {m_ * 1e3:.0f} ms")
        if best is None or m_ < best[0]:
            best = (m_, n)
        elif m_ > 1.5 * best[0]:
            break
    used_threads = best[1]
    torch.set_num_threads(used_threads)
    sweep = "; thread sweep at 32 + 11 samples per ray (ms/iter, ascending until 1.5x past the best): " + ", ".join(res)
    # 2. the TIMED WORKLOAD ITSELF at that thread count, bounded to ~budget_s: the iteration count shrinks before the workload does
    step = build(cfg) if S_tot != 43 else step43
    step(0)                                             # cold
    t0 = time.perf_counter()
    step(1)
    pilot = time.perf_counter() - t0
    warm = 5 if pilot * 25 <= budget_s * 1.2 else 2
    iters = 20 if pilot * 25 <= budget_s * 1.2 else max(5, int(budget_s / max(pilot, 1e-6)) - warm)
    med, ts = timed(step, warm, iters)
    med, idr, full = stats(ts)
    out = {"value": round(n_rays / med, 1), "unit": "rays/s", "cores": used_threads, "kind": "port",
           "sample": f"median of {iters} mapping iterations after {warm} warm-ups of THE TIMED WORKLOAD, {n_rays} rays x {S_tot} samples (oracle/spec_torch.py: forward + "
                     f"losses + smoothness + backward + Adam), {med * 1e3:.0f} ms/iter, spread (p90 - p10) / median {idr * 100:.0f} %, (max - min) / median "
                     f"{full * 100:.0f} %" + sweep,
           "samples_per_ray": S_tot, "physical_cores": physical_cores(), "logical_cpus": os.cpu_count()}
    # 3. beside it: the shipped sampling (what a real NARUTO run executes)
    if S_tot != 43:
        med43, ts43 = timed(step43, 2, 8)
        out["shipped_sampling"] = {"value": round(n_rays / med43, 1), "unit": "rays/s", "samples_per_ray": 43, "ms_per_iter": round(med43 * 1e3, 1)}
    torch.set_num_threads(n_threads_before)
    return out


PREWARM_MS = 100.0


def timed_chunks(fn, steps: int, chunks: int = 5) -> float:
    """ms per call of fn(i): the MEDIAN over `chunks` consecutive chunks of the loop, each bracketed by device syncs (host-bound eager
    loops on these boxes are disturbed for tens of milliseconds at a time by whatever else the host is doing)."""
    per = max(1, steps // chunks)
    res, i = [], 0
    for _ in range(chunks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _k in range(per):
            fn(i)
            i += 1
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) / per * 1e3)
    timed_chunks.last_mean = float(np.mean(res))
    return float(np.median(res))


def dropin_timing(cfg, n_rays: int, dev, steps: int, warmup: int, which=None):
    """The UNCHANGED caller: the reference's own global_BA loop body (coslam.py:361-399; restated in tools/dropin_caller.py) around
    ``NarutoFieldHIP`` -- model.forward (the fused training node), get_loss_from_ret as ten scalar torch ops with Co-SLAM's torch
    smoothness through query_sdf(embed=True) autograd, loss.backward(retain_graph=True), torch.optim.Adam over 1.63 M parameters,
    the uncertainty grid's Adam every 5th iteration: what INTEGRATION.md's two-line swap buys without touching anything else, and
    the optional one-line changes after it.  Eager launches, wall clock with a device sync on both sides (the loop is host bound:
    the caller's own ~60 small torch ops per iteration)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    from dropin_caller import DropInCaller           # the caller's restated loop body: a harness, not product code
    from naruto_amd.field import NarutoFieldHIP
    variants = (("swap_only", "torch", "reference", "the two-line swap at coslam.py:65, nothing else changed"),
                ("fused_adam", "fused", "reference", "+ optim.Adam -> naruto_amd.FusedAdam in create_optimizer / init_uncert_grid_optim"),
                ("fused_adam_fused_smoothness", "fused", "fused", "+ self.smoothness -> naruto_amd.trainer.smoothness (fused TV kernels)"))
    rays = {k: torch.from_numpy(v).to(dev) for k, v in bench_rays(cfg, n_rays).items()}
    out = {}
    # The caller's own host-side torch ops (Co-SLAM builds the smoothness lattice on the CPU and copies it over in EVERY iteration)
    # run with 8 intra-op threads here: with torch's default on these hosts (one thread per core, 128+) that lattice alone takes
    # 10 - 50 ms per iteration -- listed once as `swap_only_default_threads`.
    threads_before = torch.get_num_threads()
    variants = variants + (("swap_only_default_threads", "torch", "reference", "as swap_only, torch's default intra-op thread count on this host"),)
    for name, opt, sm, what in variants:
        if which is not None and name not in which:
            continue
        torch.set_num_threads(threads_before if name.endswith("default_threads") else min(8, threads_before))
        if name.endswith("default_threads"):
            steps, warmup = min(steps, 10), min(warmup, 3)
        torch.manual_seed(0)
        m = NarutoFieldHIP(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32, device=dev)).to(dev).train()
        caller = DropInCaller(m, cfg, 0.1, optimizer=opt, smoothness=sm)
        for i in range(warmup):
            caller.ba_iteration(i, rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"])
        m.check_asserts(block=True)
        ms = timed_chunks(lambda i: caller.ba_iteration(warmup + i, rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"]), steps)
        m.check_asserts(block=True)
        out[name] = {"ms_per_step": round(ms, 4), "mean_ms_per_step": round(timed_chunks.last_mean, 4), "rays_per_s": round(n_rays / ms * 1e3, 1), "change": what,
                     "host_threads": torch.get_num_threads()}
        if name == "fused_adam_fused_smoothness":
            # the same loop body, recorded once with torch's whole-iteration capture and replayed (naruto_amd.graphed.GraphedIteration): no
            # host work is left in it after the two one-line changes, so it can be
            from naruto_amd.graphed import GraphedIteration
            step = GraphedIteration(caller, n_rays)
            a_ = (rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"])
            for i in range(warmup):
                step(i, *a_)
            ms = timed_chunks(lambda i: step(warmup + i, *a_), steps)
            m.check_asserts(block=True)
            out["graphed_loop_body"] = {"ms_per_step": round(ms, 4), "mean_ms_per_step": round(timed_chunks.last_mean, 4), "rays_per_s": round(n_rays / ms * 1e3, 1), "host_threads": torch.get_num_threads(),
                                        "change": "+ the loop body (model.forward ... optimiser steps) wrapped in naruto_amd.graphed.GraphedIteration: hipGraph replay of the caller's own autograd iteration"}
            del step
        del caller, m
    torch.set_num_threads(threads_before)
    return out


def bench_rays(cfg, n_rays: int, seed: int = 0):
    """Synthetic ray batch of a workload: origins in the box shrunk by 20 %, directions uniform on the sphere, measured depths
    U(0.5, 2.5) m (5 % missing) -- scaled to the box for the unit-cube volumes."""
    unit = max(b[1] - b[0] for b in cfg["mapping"]["bound"]) <= 1.0 + 1e-6
    return syn.random_rays(n_rays, cfg["mapping"]["bound"], seed=seed, depth_range=(0.15, 0.7) if unit else (0.5, 2.5))


DUMP_BYTES = 64 << 20          # --dump-outputs: all files together
DUMP_SAMPLE = 4 << 20          # elements kept of an array larger than DUMP_SAMPLE_OVER elements
DUMP_SAMPLE_OVER = 8 << 20


def dump_outputs(out_dir: str, arrays):
    """--dump-outputs: one DIR/<name>.npy per array, float64 kept, everything else as float32.  An array of more than
    DUMP_SAMPLE_OVER elements (the hash table at T = 2^22) is written as <name>_sample.npy: its flattened elements at DUMP_SAMPLE
    indices drawn with a fixed seed (np.random.default_rng(0), sorted), the same indices in every run of the same workload."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_SAMPLE_OVER:
            idx = np.sort(np.random.default_rng(0).integers(0, t.numel(), DUMP_SAMPLE))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
            name += "_sample"
        a = t.cpu().numpy()
        a = a if a.dtype == np.float64 else a.astype(np.float32)
        total += a.nbytes
        assert total <= DUMP_BYTES, f"--dump-outputs: more than {DUMP_BYTES >> 20} MB"
        np.save(os.path.join(out_dir, name + ".npy"), a)


def train_state(tr):
    """The tensors a training step carries into the next one: parameters, the uncertainty grid's accumulated gradient, both
    optimisers' moments and step counts, the iteration word the kernels key their random numbers by (the set
    MappingTrainer.capture puts back after its own warm-up iterations)."""
    ts = tr.parameters() + [tr.model.uncert_grid.grad]
    opts = [tr.map_optimizer, tr.uncert_optim]
    if tr.table_shard is not None:
        ts.append(tr.table_shard["store"])
        opts.append(tr.table_optimizer)
    if tr.direct:
        ts.append(tr.iter_state)
    for o in opts:
        if hasattr(o, "step_dev"):
            ts.append(o.step_dev)
        ts += [v for st in o.state.values() for v in st.values() if torch.is_tensor(v)]
    return ts


def train_outputs(tr, ret, loss):
    """What a caller of a training step receives from it: the rendered colour and depth, the loss vector (ops.TrainStep.losses
    slots), the total loss and the parameters the step's optimisers left."""
    return dict({"rgb": ret["rgb"], "depth": ret["depth"], "losses": ret["_losses"], "loss": loss.reshape(1)}, **tr.model._params())


def run_eval(args, dev):
    """--workload office0_8192x43_eval (BASELINE configs[2], the planner query path): one step = the eval-mode render of 8192
    rays (naruto_render_fwd: sampling + field query + compositing + uncertainty aggregation in one launch, raw kept on chip);
    the dense uncertainty / SDF lattice query of get_map_volumes is timed next to it."""
    from naruto_amd.field import NarutoFieldHIP, get_map_volumes
    cfg, n_rays = workload(args.workload)
    cfg["decoder"]["mlp_precision"] = args.mlp
    torch.manual_seed(0)
    bbox = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32, device=dev)
    m = NarutoFieldHIP(cfg, bbox).to(dev)
    m.get_uncert_grid(0.1)
    with torch.no_grad():
        m.embed_fn.params.copy_(torch.from_numpy(syn.closed_form_table(m.embed_fn.params.numel(), 0.05)).to(dev))
    m.eval()
    rays = {k: torch.from_numpy(v).to(dev) for k, v in bench_rays(cfg, n_rays).items()}
    trc = cfg["training"]
    S_tot = trc["n_samples_d"] + trc["n_range_d"]
    rand = torch.rand(n_rays, S_tot, device=dev)

    def step():
        with torch.no_grad():
            return m.render_rays(rays["rays_o"], rays["rays_d"], target_d=rays["target_d"], rand=rand, want_raw=False)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ret = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = dt / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {k: v for k, v in ret.items() if torch.is_tensor(v)})
    k_ms = events_ms(step, max(10, min(args.steps, 50)))
    gather = 16 * 8 * 8 + 32
    alg = n_rays * (S_tot * gather + 64)                       # render inference, per ray S x 1056 B + 28 B in + 36 B out
    mfma_peak = FP32_MFMA_PEAK_TF if args.mlp == "fp32" else BF16_MFMA_PEAK_TF
    flops = n_rays * S_tot * 2 * (80 * 32 + 32 * 16 + 63 * 32 + 32 * 3)
    with torch.no_grad():
        unfused = events_ms(lambda: m.render_rays(rays["rays_o"], rays["rays_d"], target_d=rays["target_d"], rand=rand, fused=False), 20)
    # the planner's dense query (coslam_utils.py:58-97): [49,56,35] lattice -> sdf + uncertainty volumes
    get_map_volumes(m.query_sdf, m.bounding_box, 0.1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(20):
        vols = get_map_volumes(m.query_sdf, m.bounding_box, 0.1)
    map_ms = (time.perf_counter() - t1) / 20 * 1e3
    n_vox = int(np.prod(vols[0].shape))
    out = {
        "metric": "rendered rays/sec (eval render), Replica office_0", "value": round(n_rays * args.steps / dt, 1), "unit": "rays/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": DTYPE_F32 if args.mlp == "fp32" else "bf16 (MLP operands; fp32 accumulate, fp32 elsewhere)", "data": "synthetic",
        "config": {"workload": f"{args.workload} = BASELINE {WORKLOADS[args.workload][2]}: office_0 bbox, {n_rays} rays x {S_tot} samples, uncertainty grid on, "
                               f"eval-mode render_rays in one launch (naruto_render_fwd), MLP {args.mlp}", "rays_per_gpu": n_rays, "samples_per_ray": S_tot},
        "roofline": {"bound": "hbm", "achieved": round(alg / k_ms / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / k_ms / 1e6 / HBM_PEAK_GBS, 4),
                     "traffic": None, "kernel": "k_render_fwd", "kernel_ms": round(k_ms, 5), "alg_bytes": int(alg),
                     "mfma_util": round(flops / k_ms / 1e9 / mfma_peak, 6)},
        "render_unfused_ms": round(unfused, 5),
        "map_volumes": {"voxels": n_vox, "ms_end_to_end": round(map_ms, 4), "points_per_s": round(n_vox / map_ms * 1e3, 1),
                        "note": "get_map_volumes: query_sdf(return_uncert) on the cached lattice + post-processing kernel + one D2H copy"},
    }
    return out


def ba_scene(mlp: str, active_ray: bool, dev):
    """The synthetic Replica-sized mapping state of the `office0_ba_iter` workload: trainer, device-resident keyframe store (40 keyframes x
    5 % of 680 x 1200 pixels), current frame, poses, planner volume, active ray sampler (or None)."""
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    from naruto_amd.trainer import MappingTrainer
    cfg, _ = workload("office0_ba_iter")
    cfg["decoder"]["mlp_precision"] = mlp
    cfg["mapping"].update(sample=2048, min_pixels_cur=100, filter_depth=True, keyframe_every=5, active_ray=active_ray)
    Hh, Ww, n_kf = 680, 1200, 40
    R = int(Hh * Ww * 0.05)
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    tr = MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32), dev, 0.1, fused_adam=True)
    store = KeyFrameStoreHIP(cfg, Hh, Ww, num_kf=n_kf + 8, num_rays_to_save=R, device=dev, seed=1)

    def frame_rays(n):
        d = torch.randn(n, 3, device=dev, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        depth = 0.5 + 2.0 * torch.rand(n, 1, device=dev, generator=g)
        depth[torch.rand(n, 1, device=dev, generator=g) < 0.05] = 0.0
        return torch.cat([d, torch.rand(n, 3, device=dev, generator=g), depth], -1)
    store.rays[:n_kf] = frame_rays(n_kf * R).reshape(n_kf, R, 7)
    store.attach_ids(torch.arange(n_kf) * 5)
    current = frame_rays(Hh * Ww)
    bound = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32)
    poses = torch.eye(4).repeat(n_kf + 1, 1, 1)
    for p_ in poses:
        q, _ = torch.linalg.qr(torch.randn(3, 3))
        p_[:3, :3] = q
        p_[:3, 3] = bound[:, 0] + (0.3 + 0.4 * torch.rand(3)) * (bound[:, 1] - bound[:, 0])
    vol = (torch.rand(49, 56, 35) * 3 * (torch.rand(49, 56, 35) < 0.5)).numpy()
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=500, oversample_mul=4) if active_ray else None
    return cfg, tr, store, smp, current, poses, vol, (Hh, Ww, n_kf, R)


def mapping_iter_ms(mlp: str, dev, steps: int, warmup: int):
    """BASELINE's second metric, in the --full line: one global_BA iteration END TO END (ray assembly -> [active ray selection] ->
    training iteration, one hipGraph: naruto_amd.ba_loop.FusedBA), shipped sampling (32 + 11), active rays off and on; ms per iteration,
    median of five chunks after >= PREWARM_MS of untimed replays.  `--workload office0_ba_iter` gives the long form."""
    from naruto_amd.ba_loop import FusedBA
    out = {}
    for active in (False, True):
        cfg, tr, store, smp, current, poses, vol, _dims = ba_scene(mlp, active, dev)
        ba = FusedBA(tr, store, smp, max_poses=256, use_graph=True)
        n_cur, n_train = ba.prepare(current, poses, vol if active else None)
        # the iterations of whole global_BA calls (mapping.iters = 10 each: the call's first assembles its own batch, the others find theirs
        # prepared by the previous iteration's last launch, every 5th steps the grid), one graph launch per call; ms per ITERATION
        iters = int(cfg["mapping"]["iters"])
        for i in range(max(1, warmup // iters)):
            ba.call_iterations()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < PREWARM_MS * 1e-3:
            for _ in range(4):
                ba.call_iterations()
            torch.cuda.synchronize()
        ms = timed_chunks(lambda k: ba.call_iterations(), max(5, 5 * steps // iters)) / iters
        tr.model.check_asserts(block=True)
        out["active_ray_on" if active else "active_ray_off"] = {"ms": round(ms, 4), "rays_per_iteration": n_train, "rays_per_s": round(n_train / ms * 1e3, 1)}
        del ba, tr, store, smp
    return out


def run_ba_iter(args, dev):
    """--workload office0_ba_iter: what ONE iteration of the reference's global_BA loop costs here end to end (coslam.py:310-399):
    batch draw from the device-resident keyframe store + current frame and the pose transform (naruto_assemble_rays), the active ray
    selection when mapping.active_ray is on (naruto_active_ray_select over the 4x oversampled batch), and the training iteration
    (forward, losses incl. smoothness, backward, both Adams) -- one stream, one hipGraph (naruto_amd.ba_loop.FusedBA).  Synthetic
    Replica-sized inputs: 680 x 1200 frames, 40 keyframes x 5 % of the pixels stored, [49,56,35] planner volume."""
    from naruto_amd.ba_loop import FusedBA
    cfg, tr, store, smp, current, poses, vol, (Hh, Ww, n_kf, R) = ba_scene(args.mlp, bool(args.active_ray), dev)
    res = {}
    for mode in ("graph", "eager"):
        ba = FusedBA(tr, store, smp, max_poses=256, use_graph=(mode == "graph"))
        n_cur, n_train = ba.prepare(current, poses, vol if args.active_ray else None)
        iters = int(cfg["mapping"]["iters"])       # whole calls of mapping.iters iterations (graph mode: one graph launch per call)
        n_calls = max(1, args.steps // iters)
        for i in range(max(1, args.warmup // iters)):
            ba.call_iterations()
        tr.model.check_asserts(block=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_calls):
            last = ba.call_iterations()
        torch.cuda.synchronize()
        res[mode] = (time.perf_counter() - t0) / (n_calls * iters) * 1e3
        if mode == "graph" and args.dump_outputs:            # the headline's path; the eager mode below trains the same model further
            tr.model.check_asserts(block=True)
            dump_outputs(args.dump_outputs, train_outputs(tr, *last))
        if mode == "graph":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n_calls * iters):
                ba.iteration(i % iters)
            torch.cuda.synchronize()
            res["graph_per_iteration"] = (time.perf_counter() - t0) / (n_calls * iters) * 1e3
        tr.model.check_asserts(block=True)
        if mode == "graph":
            per_call = []                          # a whole global_BA call of mapping.iters iterations incl. its per-call preparation
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ba.global_BA(current, poses, uncert_vol=vol if args.active_ray else None)
                torch.cuda.synchronize()
                per_call.append((time.perf_counter() - t0) * 1e3)
            res["call"] = float(np.median(per_call))
    # the pieces alone (HIP events, eager)
    ba = FusedBA(tr, store, smp, max_poses=256, use_graph=False)
    ba.prepare(current, poses, vol if args.active_ray else None)
    bufs = ba._eager_bufs
    t_pro = events_ms(lambda: ba._pro(*bufs), 50)
    t_step = events_ms(lambda: tr.step(*bufs, smooth=True, uncert_step=False), 50)
    trc = cfg["training"]
    S_tot = trc["n_samples_d"] + trc["n_range_d"]
    ms = res["graph"]
    out = {"metric": "mapping-iter ms (one global_BA iteration end to end), Replica office_0", "value": round(ms, 4), "unit": "ms", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(ms, 4), "mapping_iter_ms": round(ms, 4), "higher_is_better": False, "scaling": "weak", "vs_baseline": None,
           "dtype": DTYPE_F32 if args.mlp == "fp32" else "bf16 (MLP operands; fp32 accumulate, fp32 elsewhere)", "data": "synthetic",
           "rays_per_s": round(n_train / ms * 1e3, 1),
           "config": {"workload": f"{args.workload} = BASELINE {WORKLOADS[args.workload][2]}: office_0 bbox, {n_kf} keyframes x {R} stored rays, {Hh} x {Ww} current frame, "
                                  f"mapping.sample 2048, active_ray {'on (4x oversampled batch of ' + str(ba.sample_num + n_cur) + ' rays, K = 500)' if args.active_ray else 'off'}, "
                                  f"{n_train} rays x {S_tot} samples into the training step; hash L16 F2 T2^16, MLP 2x32 {args.mlp}; one hipGraph per global_BA call of {int(cfg['mapping']['iters'])} iterations",
                      "rays_per_step": n_train, "samples_per_ray": S_tot, "n_cur": n_cur, "active_ray": bool(args.active_ray)},
           "eager_ms_per_iteration": round(res["eager"], 4), "one_graph_per_iteration_ms": round(res["graph_per_iteration"], 4),
           "global_BA_call_ms": {"iters": int(cfg["mapping"]["iters"]), "ms": round(res["call"], 4),
                                 "note": "per call: frame + pose upload into the static buffers, one valid-pixel count read back, mapping.iters replays"},
           "pieces_eager_ms": {"assemble" + (" + active ray select" if args.active_ray else ""): round(t_pro, 5), "training step": round(t_step, 5)}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="office0_2048x128", help="one of: " + ", ".join(sorted(WORKLOADS)))
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: the workload's ray count PER GPU; strong: the workload's ray count per JOB, sharded over the GPUs")
    ap.add_argument("--mlp", choices=("fp32", "bf16"), default="fp32",
                    help="fp32: exact fp32 MFMA chain (the parity mode, the headline); bf16: bf16 operands on v_mfma_f32_32x32x16_bf16 (speed mode)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--torch-adam", action="store_true", help="torch.optim.Adam instead of the fused HIP Adam")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying the captured hipGraph")
    ap.add_argument("--no-chain", action="store_true", help="one graph launch per iteration instead of one per global_BA call of mapping.iters iterations")
    ap.add_argument("--path", choices=("trainer", "dropin"), default="trainer",
                    help="trainer: MappingTrainer's fused iteration (hipGraph replay), the headline; dropin: the reference's unchanged loop body "
                         "(coslam.py:361-399) around NarutoFieldHIP is the timed step (its figures ride in the --full line too, as `dropin`)")
    ap.add_argument("--no-dropin", action="store_true")
    ap.add_argument("--no-mapping-iter", action="store_true", help="skip the mapping-iter ms (office0_ba_iter) figures of the --full line")
    ap.add_argument("--active-ray", action="store_true", help="office0_ba_iter: mapping.active_ray on (4x oversampled batch -> active ray selection)")
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: per-kernel table and rooflines, drop-in caller, mapping-iter ms, median-of-chunks step times, "
                         "CPU and torch-on-GPU baselines (each can be left out with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed path computed in its last step as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.path == "dropin":
        ap.error("--dump-outputs: --path dropin times several variants of the caller's loop, none of which is kept")

    # `python bench.py --gpus N` WITHOUT a launcher (no WORLD_SIZE in the environment): run the documented launch line -- one process per
    # GPU through torch.distributed.run on 127.0.0.1 -- instead of failing on the world-size check (round-3 review: a scaling run issued like
    # the 1-GPU command would have wasted its 8-GPU lease).  The launcher is a child process that inherits stdout: rank 0's one JSON line
    # is this command's, and its exit status is this command's.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        print("[bench] --gpus %d without a launcher: running %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
        rc = subprocess.run(cmd).returncode
        sys.exit(rc if rc >= 0 else 128 - rc)              # killed by signal s: the shell's 128 + s

    # stdout carries exactly ONE line, the JSON result.  RCCL writes its version banner to the C-level stdout (it lands in
    # libc's buffer and would come out after the result); route file descriptor 1 to stderr for the whole run and give it
    # back only for the result line.
    import ctypes
    libc = ctypes.CDLL(None)
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    # NARUTO_DIST_BACKEND=gloo: a REHEARSAL of the multi-rank launch line on a box with fewer GPUs than ranks (RCCL refuses two ranks on
    # one device; gloo carries device tensors through the host): ranks share GPU LOCAL_RANK % device_count.  Timings of such a run
    # mean nothing; the line says so.
    backend = os.environ.get("NARUTO_DIST_BACKEND", "nccl")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    group = parallel.init_from_env(backend) if (args.gpus > 1 or os.environ.get("NARUTO_FORCE_DIST") == "1") else None
    world, rank = parallel.world_size(group), parallel.rank(group)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE is {world}"
    dev = torch.device("cuda", local)

    if args.workload.endswith("_eval") or args.workload == "office0_ba_iter":
        assert world == 1, "the eval / mapping-iteration workloads are single-GPU paths"
        out = run_eval(args, dev) if args.workload.endswith("_eval") else run_ba_iter(args, dev)
        sys.stdout.flush()
        libc.fflush(None)
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
        return
    cfg, n_workload = workload(args.workload)
    cfg["decoder"]["mlp_precision"] = args.mlp
    if args.path == "dropin":
        assert world == 1, "--path dropin times the single-process caller"
        d = dropin_timing(cfg, n_workload, dev, args.steps, args.warmup, which=("swap_only",))["swap_only"]
        trc = cfg["training"]
        S_tot = trc["n_samples_d"] + trc["n_range_d"]
        out = {"metric": "rendered rays/sec (train step), Replica office_0", "value": d["rays_per_s"], "unit": "rays/s", "n_gpus": 1, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": d["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": DTYPE_F32 if args.mlp == "fp32" else "bf16 (MLP operands; fp32 accumulate, fp32 elsewhere)", "data": "synthetic",
               "config": {"workload": f"{args.workload} = BASELINE {WORKLOADS[args.workload][2]}: {n_workload} rays x {S_tot} samples, one global_BA iteration of the "
                                      "reference's UNCHANGED loop body (coslam.py:361-399: model.forward, get_loss_from_ret with Co-SLAM's torch smoothness, "
                                      "loss.backward(retain_graph=True), torch.optim.Adam, uncertainty-grid Adam every 5th) around NarutoFieldHIP, eager launches",
                          "path": "dropin", "rays_per_gpu": n_workload, "samples_per_ray": S_tot}}
        sys.stdout.flush()
        libc.fflush(None)
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
        return
    if args.scaling == "strong":
        n_total = n_workload
        assert n_total % world == 0, f"strong scaling: {n_total} rays do not split over {world} GPUs"
    else:
        n_total = n_workload * world
    lo, hi = parallel.shard_bounds(n_total, rank, world)
    n_rays = hi - lo
    from naruto_amd.trainer import MappingTrainer
    torch.manual_seed(0)                                     # identical replicas on every rank
    tr = MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32), dev, 0.1, group=group,
                        fused_adam=not args.torch_adam)
    # Single process: the whole iteration replays from one hipGraph.  Data parallel: EAGER launches by default (round 4) -- measured at world
    # size 1 with real RCCL calls (NARUTO_FORCE_DIST=1, tools/dp_world1.sh): eager 0.274 ms, four graph segments with the collectives
    # eager in between 0.297 (a hipGraph launch costs more than the three or four kernel launches it replaces), everything incl. the
    # collectives in ONE graph 0.235 -- the fastest, but a captured RCCL collective over several ranks cannot be exercised on the one-GPU
    # build boxes, so it stays opt-in.  NARUTO_GRAPH_DIST=segmented|whole selects the graph forms.
    use_graph = (not args.no_graph) and (group is None or os.environ.get("NARUTO_GRAPH_DIST", "eager") in ("segmented", "whole"))
    if use_graph:
        try:
            # single process: besides the per-iteration graphs ONE graph that holds the mapping.iters (10) iterations of a global_BA call -- the
            # launch-to-launch gap between graphs (5 - 8 us) is paid once per call instead of once per iteration (--no-chain: per-iteration graphs)
            chain_n = int(cfg["mapping"]["iters"]) if (group is None and not args.no_chain) else 0
            tr.capture(n_rays, smooth=True, n_rays_total=n_total, chain=[(i + 1) % 5 == 0 for i in range(chain_n)] if chain_n else None)
        except Exception as e:                      # data parallel only: a failed capture must not cost the run -- eager launches instead
            if group is None:
                raise
            print(f"[bench] rank {rank}: graph capture failed ({e!r}); continuing with eager launches", file=sys.stderr, flush=True)
            tr._graphs, tr._static = None, None
            torch.cuda.synchronize()
    all_rays = bench_rays(cfg, n_total)
    rays = {k: torch.from_numpy(v[lo:hi]).to(dev) for k, v in all_rays.items()}
    del all_rays
    from naruto_amd.trainer import pack_rays
    bufs = tr.ray_buffers()
    if bufs is not None:
        # the batch sits where the ray assembly (KeyframeRayStore.assemble_batch(out=...)) writes it: the replay's own input buffers
        for b, k in zip(bufs, ("rays_o", "rays_d", "target_rgb", "target_d")):
            b.copy_(rays[k].reshape(b.shape))
            rays[k] = b
    else:
        rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"] = pack_rays(rays["rays_o"], rays["rays_d"], rays["target_rgb"],
                                                                                          rays["target_d"])

    def step():
        return tr.step(rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"], smooth=True, n_rays_total=n_total)

    chain_n = tr.chain_length() if use_graph and tr._graphs is not None else 0

    def steps(k: int):
        """k iterations: whole calls of chain_n iterations as one graph launch each, the remainder iteration by iteration; returns the
        last iteration's (ret, loss)"""
        out = None
        while chain_n and k >= chain_n:
            out = tr.step_chain(n_rays_total=n_total)
            k -= chain_n
        for _ in range(k):
            out = step()
        return out

    steps(args.warmup)
    # pre-warm: the timed window of the default run is ~5 ms (20 - 50 steps of ~0.23 ms) -- short enough to be read at ramping clocks right
    # after the captures and copies above.  Untimed steps for >= PREWARM_MS of wall time first (every rank the same count: the collectives
    # of a data-parallel step must pair up), stated in the line.  Their count depends on the speed of the build, so the training state
    # is put back afterwards: the timed steps start from the state after the warm-up steps, and what they compute depends on the
    # arguments alone (--dump-outputs).
    state = train_state(tr)
    saved = [t.detach().clone() for t in state]
    saved_iter = tr.iter
    saved_rng = None if tr.direct else torch.cuda.get_rng_state(dev)          # the autograd iteration's jitter comes from torch's RNG
    torch.cuda.synchronize()
    t_w = time.perf_counter()
    for _ in range(8):
        step()
    torch.cuda.synchronize()
    per_step = max((time.perf_counter() - t_w) / 8, 1e-5)
    n_prewarm = int(min(max(PREWARM_MS * 1e-3 / per_step, 0), 20000))
    if group is not None:
        t = torch.tensor([n_prewarm], dtype=torch.int64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=group)
        n_prewarm = int(t.item())
    steps(n_prewarm)
    tr.model.check_asserts(block=True)
    with torch.no_grad():
        for t, s in zip(state, saved):
            t.copy_(s)
    tr.iter = saved_iter
    if saved_rng is not None:
        torch.cuda.set_rng_state(saved_rng, dev)
    del saved
    if group is not None:
        torch.distributed.barrier(group)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = steps(args.steps)
    torch.cuda.synchronize()
    if group is not None:
        torch.distributed.barrier(group)
    dt = time.perf_counter() - t0
    if group is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX, group=group)
        dt = float(t.item())
    tr.model.check_asserts(block=True)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, train_outputs(tr, *last))
    # beside the contract's figure (exactly K steps between two syncs, above): the MEDIAN over five further chunks of K steps each, which a
    # single disturbed chunk cannot move (single process only: the chunks' syncs would need barriers of their own)
    ms_chunks = ms_single = None
    if args.full and group is None:
        if chain_n:
            per = max(chain_n, args.steps // chain_n * chain_n)
            ms_chunks = timed_chunks(lambda i: steps(per), 5) / per
            ms_single = timed_chunks(lambda i: step(), 5 * args.steps)          # one graph launch per iteration
        else:
            ms_chunks = timed_chunks(lambda i: step(), 5 * args.steps)

    if rank == 0:
        trc = cfg["training"]
        S_tot = trc["n_samples_d"] + trc["n_range_d"]
        ms = dt / args.steps * 1e3
        volume = "MP3D YmJkqBEsHnH bbox (largest shipped)" if args.workload.startswith("mp3d") else (
            "unit cube, finest level 1024^3" if args.workload.startswith("unit") else "office_0 bbox")
        n_params = int(tr.model.embed_fn.params.numel()) + 5184 + int(tr.model.uncert_grid.numel())
        out = {
            "metric": "rendered rays/sec (train step), Replica office_0",
            "value": round(n_total * args.steps / dt, 1), "unit": "rays/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": DTYPE_F32 if args.mlp == "fp32" else "bf16 (MLP operands; fp32 accumulate, fp32 elsewhere)", "data": "synthetic",
            "prewarm": {"untimed_steps_before_the_timed_region": args.warmup + 8 + n_prewarm, "target_ms": PREWARM_MS,
                        "training_state": f"put back to where the {args.warmup} warm-up steps left it"},
            "ms_per_step_median_of_5_chunks": None if ms_chunks is None else round(ms_chunks, 4),
            "graph_launches": (f"one hipGraph per {chain_n} iterations (= one global_BA call, mapping.iters); the remainder of K and --no-chain: one per iteration"
                               if chain_n else ("one hipGraph per iteration" if use_graph and tr._graphs is not None else "eager")),
            "ms_per_step_one_graph_per_iteration": None if ms_single is None else round(ms_single, 4),
            "multi_gpu_note": "no multi-GPU scaling curve has been measured by the builder (one-GPU boxes only): values at n_gpus > 1 come from the driver's runs",

            "config": {"workload": f"{args.workload} = BASELINE {WORKLOADS[args.workload][2]}: {volume}, {n_rays} rays x {S_tot} samples per GPU "
                                   f"({n_total} rays per step over {world} GPU), hash L16 F2 T2^{cfg['grid']['hash_size']} ({n_params * 4 / 1e6:.1f} MB of parameters), "
                                   f"MLP 2x32 {args.mlp}, uncert grid; one global_BA mapping iteration incl. smoothness + Adam",
                       "rays_per_gpu": n_rays, "rays_per_step": n_total, "samples_per_ray": S_tot, "parallelism": f"ray-sharded dp{world}",
                       "optimizer": "torch.optim.Adam" if args.torch_adam else "fused HIP Adam", "hip_graph": bool(use_graph and tr._graphs is not None),
                       "table_optimizer": "sharded over the ranks (reduce-scatter | Adam on 1/world | all-gather)" if tr.table_shard is not None else "replicated"},
        }
        if group is not None and backend != "nccl":
            out["config"]["rehearsal"] = f"NARUTO_DIST_BACKEND={backend}: {world} ranks over {torch.cuda.device_count()} GPU(s) through the host -- launch-line rehearsal, not a measurement"
        # whole-step roofline figures: per ray S x 3168 B + 44 B and S x 31104 FLOP; per step Adam's 28 B / parameter
        mfma_peak = FP32_MFMA_PEAK_TF if args.mlp == "fp32" else BF16_MFMA_PEAK_TF
        rays_s = n_total * args.steps / dt
        step_bytes = n_rays * (S_tot * 3168 + 44) + n_params * 28
        out["step_roofline"] = {"alg_bytes_per_step_per_gpu": int(step_bytes), "achieved_GBps": round(step_bytes / (ms * 1e-3) / 1e9, 1),
                                "hbm_frac": round(step_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "mfma_util": round(rays_s / world * S_tot * 31104 / (mfma_peak * 1e12), 6),
                                "mfma_peak": f"{mfma_peak} TFLOP/s " + ("(fp32 MFMA = fp32 vector rate)" if args.mlp == "fp32" else "(bf16 MFMA, dense)")}
        if args.full and not args.no_kernels:
            rows = kernel_table(tr, rays, cfg, max(10, min(args.steps, 50)))
            dom = max((r for r in rows if r["bound"] is not None), key=lambda r: r["ms"])
            # the dominant kernel OF THE ITERATION: the table scatter when its launch (iteration shape, timed alone) outlasts the field
            # query's launch of the iteration; otherwise the largest modular row (the field query over all samples)
            sc_it = next((r for r in rows if r["kernel"].startswith("k_hash_scatter_lds as launched")), None)
            q_it = next(r for r in rows if r["kernel"].startswith("k_query_fwd<color> as launched"))
            if sc_it is not None and sc_it["ms"] >= q_it["ms"]:
                dom = dict(sc_it, kernel="k_hash_scatter_lds", bound="hbm", launch="as launched by the iteration (lattice + active samples, level + uncertainty-grid units)")
            elif sc_it is not None:
                dom = next(r for r in rows if r["kernel"].startswith("k_query_fwd<color>") and "launch" in r)      # the field query over all samples
            if dom["bound"] == "mfma":
                roof = {"bound": "mfma", "achieved": dom["TFLOPs"], "peak": mfma_peak, "unit": "TFLOP/s",
                        "frac": round(dom["TFLOPs"] / mfma_peak, 4), "traffic": None}
            else:
                roof = {"bound": "hbm", "achieved": dom["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(dom["GBps"] / HBM_PEAK_GBS, 4), "traffic": None}
            roof["kernel"] = dom["kernel"]
            roof["kernel_ms"] = dom["ms"]
            roof["alg_bytes"] = dom["alg_bytes"]
            if "launch" in dom:
                roof["launch"] = dom["launch"]
            if "alg_bytes_all_samples" in dom:
                # SURVEY 8(d)'s figure over ALL samples of the batch (the reference scatters every sample; this launch only the active
                # prefix + the lattice): reported beside, never as frac
                roof["list_points"] = dom["list_points"]
                roof["alg_bytes_all_samples"] = dom["alg_bytes_all_samples"]
                roof["frac_all_samples"] = round(dom["alg_bytes_all_samples"] / dom["ms"] / 1e6 / HBM_PEAK_GBS, 4)
            if "alg_bytes_incl_saved" in dom:
                b2 = dom["alg_bytes_incl_saved"]
                roof["alg_bytes_incl_saved"] = b2
                roof["frac_incl_saved"] = round(b2 / dom["ms"] / 1e6 / HBM_PEAK_GBS, 4)
            if dom["kernel"].startswith("k_query_fwd"):
                it = next(r for r in rows if r["kernel"].startswith("k_query_fwd<color> as launched"))
                roof["kernel_ms_in_iteration"] = it["ms"]
                roof["mfma_util"] = round(dom["TFLOPs"] / mfma_peak, 6)
                # L2 line rate (MI355X_MICROARCH.md: ~34.5 TB/s aggregate): a wave's 64 8-byte gathers touch ~36 distinct 64-byte
                # lines (x-neighbour corners share a line, tools/gather_coalesce_bench.hip), i.e. 4.5 lines per (sample, level)
                l2_bytes = n_rays * S_tot * (16 * 4.5 * 64 + 4 * 64) + dom.get("alg_bytes_incl_saved", 0) - n_rays * S_tot * (16 * 8 * 8 + 32)
                roof["l2_bytes_model"] = int(l2_bytes)
                roof["l2_frac"] = round(l2_bytes / dom["ms"] / 1e6 / L2_PEAK_GBS, 4)
            # the hash gather (north star: "HBM GB/s on the hash gather") always gets its own object, dominant or not
            fwd = next(r for r in rows if r["kernel"].startswith("k_query_fwd<color>") and "launch" in r)
            it = next(r for r in rows if r["kernel"].startswith("k_query_fwd<color> as launched"))
            l2_bytes = n_rays * S_tot * (16 * 4.5 * 64 + 4 * 64) + fwd["alg_bytes_incl_saved"] - n_rays * S_tot * (16 * 8 * 8 + 32)
            gprof, gsrc = pmc_profile(args.workload, fwd["kernel"])
            out["roofline_gather"] = {"bound": "hbm", "kernel": fwd["kernel"], "launch": fwd["launch"], "kernel_ms": fwd["ms"], "kernel_ms_in_iteration": it["ms"],
                                      "alg_bytes": fwd["alg_bytes"], "achieved": fwd["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": round(fwd["GBps"] / HBM_PEAK_GBS, 4), "alg_bytes_incl_saved": fwd["alg_bytes_incl_saved"],
                                      "frac_incl_saved": round(fwd["alg_bytes_incl_saved"] / fwd["ms"] / 1e6 / HBM_PEAK_GBS, 4),
                                      "l2_bytes_model": int(l2_bytes), "l2_frac": round(l2_bytes / fwd["ms"] / 1e6 / L2_PEAK_GBS, 4),
                                      "mfma_util": round(fwd["TFLOPs"] / mfma_peak, 6), "traffic": gprof.get("traffic_bytes"),
                                      "traffic_source": f"profiles/{gsrc}" if gsrc else None}
            prof, src = pmc_profile(args.workload, dom["kernel"])
            if prof.get("traffic_bytes") is not None:
                roof["traffic"] = prof["traffic_bytes"]                      # bytes per launch (FETCH_SIZE + WRITE_SIZE), same launch shape
                roof["traffic_source"] = f"profiles/{src}"
                roof["traffic_GBps"] = round(prof["traffic_bytes"] / dom["ms"] / 1e6, 1)       # what actually crossed the L2 <-> fabric boundary per second
                roof["traffic_frac"] = round(prof["traffic_bytes"] / dom["ms"] / 1e6 / HBM_PEAK_GBS, 4)
            g_ = out["roofline_gather"]
            if g_.get("traffic") is not None:
                g_["traffic_GBps"] = round(g_["traffic"] / g_["kernel_ms"] / 1e6, 1)
                g_["traffic_frac"] = round(g_["traffic"] / g_["kernel_ms"] / 1e6 / HBM_PEAK_GBS, 4)
            # the launch the TIMED STEP runs (the depth-ordered walk / the short-ray form: depth sampling, field query over the samples some
            # consumer can see, loss stage, lattice encode in its tail workgroups), on the samples it actually evaluates
            if it.get("evaluated_samples") is not None:
                out["roofline_in_iteration"] = {"bound": "hbm", "kernel": "k_query_fwd_loss / k_query_fwd_loss_short as launched by the timed step "
                                                "(with depth sampling, loss stage and the smoothness lattice's encode in the same launch)",
                                                "kernel_ms": it["ms"], "evaluated_samples": it["evaluated_samples"], "samples": it["samples"],
                                                "alg_bytes": it["alg_bytes"], "achieved": it["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                                "frac": round(it["GBps"] / HBM_PEAK_GBS, 4)}
            # What actually binds the hash gather: the rate at which a CU's vector memory path takes RANDOM 64-byte lines -- out of L2 for
            # the shipped 6.5 MB table (one line per ~3 cycles and CU, whatever the occupancy: tools/gather_valu_overlap_bench.hip), out
            # of HBM for tables no cache holds (T = 2^22: 281 MB; tools/hbm_random_line_bench.hip).  Measured here, live, by a launch that
            # does nothing else over this very table (naruto_debug_random_lines: the forward's own access pattern, 32 lines per load
            # instruction); the kernel's line count is a MODEL (four lines per sample and level whose slice exceeds the cache in front
            # of that path -- an upper bound where neighbouring samples share lines) next to the PMC figure where there is one.
            try:
                import ctypes as CT
                from naruto_amd import _lib, ops
                lib_ = _lib.load()
                table_bytes = int(tr.model.embed_fn.params.numel()) * 4
                hbm_resident = table_bytes > (64 << 20)
                sink = torch.zeros(1, device=dev)
                n_lines = CT.c_uint64(0)
                tb = tr.model.embed_fn.params
                run = lambda: _lib.check(lib_.naruto_debug_random_lines(tb.data_ptr(), table_bytes, 64, sink.data_ptr(), CT.byref(n_lines), ops._stream()))
                rl_ms = events_ms(run, 5)
                rate = n_lines.value / (rl_ms * 1e-3)
                g_ = out["roofline_gather"]
                # (round 5: the four-lines-per-sample-and-level MODEL is gone -- it put the kernel at 1.3 of a roof, i.e. it overcounted what
                # ray neighbours share; the kernel's line count is now MEASURED: requests arriving at the L2 per launch, TCC_REQ_sum from a
                # rocprofv3 --pmc pass over eager launches (tools/profile_round.sh), for HBM-resident tables also the fabric-side traffic / 64)
                rr = {"lines_per_s": round(rate, 1), "TBps_of_64B_lines": round(rate * 64 / 1e12, 3), "served_from": "HBM" if hbm_resident else "L2",
                      "measured": "naruto_debug_random_lines over this table (32 random lines per load instruction, 8 loads in flight per wave, 8 waves per SIMD), HIP events"}
                if gprof.get("tcc_req") is not None:
                    rr["l2_requests_per_launch_pmc"] = int(gprof["tcc_req"])
                    rr["frac_l2_requests"] = round(gprof["tcc_req"] / (g_["kernel_ms"] * 1e-3) / rate, 4)
                    rr["l2_requests_source"] = f"profiles/{gsrc} (TCC_REQ_sum: every request the L1s pass on, gathers and streamed rows alike)"
                if hbm_resident and g_.get("traffic") is not None:
                    rr["lines_per_launch_pmc"] = int(g_["traffic"] // 64)
                    rr["frac_pmc"] = round(g_["traffic"] / 64 / (g_["kernel_ms"] * 1e-3) / rate, 4)
                g_["random_line_roof"] = rr
                if roof["kernel"].startswith("k_query_fwd"):
                    roof["random_line_roof"] = rr
            except Exception as e:                               # informational: never fail the bench line over it
                out["roofline_gather"]["random_line_roof"] = {"error": repr(e)[:200]}
            out["roofline"] = roof
            # Round 6: when the iteration's dominant launch is its forward, `roofline` is THAT launch -- the depth-ordered walk /
            # short-ray kernel the timed step runs (depth sampling, field query over the samples some consumer can see, loss stage, lattice encode),
            # timed alone with HIP events in the iteration's launch shape, SURVEY 8(d)'s 1 056 B per sample it EVALUATES + 64 B per ray -- and
            # the flat all-samples launch of the same arithmetic stays in `roofline_gather`.
            if roof["kernel"].startswith("k_query_fwd") and it.get("evaluated_samples") is not None:
                S_it = int(it["samples"]) // int(n_rays)
                k_it = "k_query_fwd_loss_short" if S_it <= 64 else "k_query_fwd_loss"
                n_table_bytes = int(tr.model.embed_fn.params.numel()) * 4
                sorted_env = os.environ.get("NARUTO_FWD_SORTED", "1")
                if sorted_env == "2" or (sorted_env == "1" and (n_table_bytes > (64 << 20) or (int(it["samples"]) >= 4000000 and S_it <= 64))):
                    k_it = "k_query_fwd_list"          # the Morton-ordered forward (naruto_sorted.hip): sort launches + two list passes, timed together
                iprof, isrc = pmc_profile(args.workload, k_it)
                if k_it == "k_query_fwd_list" and iprof:
                    # two launches of this kernel per iteration (first list, second list: same grid, so the PMC table averages them): per ITERATION = 2 x
                    iprof = dict(iprof)
                    for kk in ("traffic_bytes", "fetch_bytes", "write_bytes", "tcc_req"):
                        if iprof.get(kk) is not None:
                            iprof[kk] = 2 * iprof[kk]
                roof_it = {"bound": "hbm", "achieved": it["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(it["GBps"] / HBM_PEAK_GBS, 4),
                           "traffic": iprof.get("traffic_bytes"), "kernel": k_it,
                           "launch": "as launched by the timed step (naruto_debug_train_query_fwd: the same launch, alone)",
                           "kernel_ms": it["ms"], "alg_bytes": it["alg_bytes"], "evaluated_samples": it["evaluated_samples"], "samples": it["samples"],
                           "alg_bytes_all_samples": roof["alg_bytes"], "frac_all_samples_flat_launch": roof["frac"], "flat_launch_kernel_ms": roof["kernel_ms"]}
                if iprof.get("traffic_bytes") is not None:
                    roof_it["traffic_source"] = f"profiles/{isrc}"
                    roof_it["traffic_GBps"] = round(iprof["traffic_bytes"] / it["ms"] / 1e6, 1)
                    roof_it["traffic_frac"] = round(iprof["traffic_bytes"] / it["ms"] / 1e6 / HBM_PEAK_GBS, 4)
                if iprof.get("tcc_req") is not None and "random_line_roof" in roof and "lines_per_s" in roof["random_line_roof"]:
                    rr_it = dict(roof["random_line_roof"])
                    rr_it["l2_requests_per_launch_pmc"] = int(iprof["tcc_req"])
                    rr_it["frac_l2_requests"] = round(iprof["tcc_req"] / (it["ms"] * 1e-3) / rr_it["lines_per_s"], 4)
                    rr_it["l2_requests_source"] = f"profiles/{isrc} (TCC_REQ_sum)"
                    roof_it["random_line_roof"] = rr_it
                out["roofline"] = roof_it
            if sc_it is not None and "active_samples" in sc_it:
                # the same figure with the backward's share (3168 B minus the forward's 1056 B per sample) charged only for the samples the
                # backward actually processes (the compacted list: non-zero loss gradient), not for every sample of the batch: the honest
                # denominator for "how close is the whole step to the HBM roof"
                fwd_b = next(r for r in rows if r["kernel"].startswith("k_query_fwd<color>") and "launch" in r)["alg_bytes"] / (n_rays * S_tot)
                act_bytes = n_rays * (S_tot * fwd_b + 44) + sc_it["active_samples"] * (3168 - fwd_b) + n_params * 28
                out["step_roofline"].update({"alg_bytes_active_samples": int(act_bytes), "active_samples": int(sc_it["active_samples"]),
                                             "samples": int(n_rays * S_tot), "achieved_GBps_active_samples": round(act_bytes / (ms * 1e-3) / 1e9, 1),
                                             "hbm_frac_active_samples": round(act_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
            out["kernels"] = rows
            out["kernels_ms_sum"] = round(sum(r["ms"] for r in rows if r["bound"] is not None), 4)
        if args.full and not args.no_dropin and world == 1:
            try:
                d = dropin_timing(cfg, n_rays, dev, max(10, min(args.steps, 50)), 10)
                out["dropin"] = d
                out["dropin_ms_per_step"] = d["swap_only"]["ms_per_step"]
                out["dropin_note"] = ("the reference's unchanged loop body around NarutoFieldHIP (bench.py dropin_timing, tools/dropin_caller.py), eager, wall clock, median (and mean) "
                                      "over five chunks of the timed loop; "
                                      "ms_per_step / value above are MappingTrainer's fused iteration under hipGraph replay")
            except Exception as e:                               # informational: never fail the bench line over it
                out["dropin"] = {"error": repr(e)[:300]}
        if args.full and world == 1 and args.workload.startswith("office0") and not args.no_mapping_iter:
            # BASELINE's metric is "rays/sec (train step) + mapping-iter ms": the second half, measured by the same --full run
            try:
                mi = mapping_iter_ms(args.mlp, dev, max(10, min(args.steps, 50)), 10)
                # the shipped setting is active rays ON (configs/default.py:54 enable_active_ray = True, read at coslam.py:100): that is the headline figure
                out["mapping_iter_ms"] = mi["active_ray_on"]["ms"]
                out["mapping_iter_ms_active_ray_off"] = mi["active_ray_off"]["ms"]
                out["mapping_iter"] = dict(mi, note="one global_BA iteration end to end (coslam.py:310-399): ray assembly from the device-resident keyframe store + "
                                           "current frame (2148 rays) -> [active ray selection over the 4x oversampled batch] -> training iteration at the shipped "
                                           "32 + 11 samples, one hipGraph (naruto_amd.ba_loop.FusedBA); median of five chunks; long form: --workload office0_ba_iter")
            except Exception as e:                               # informational: never fail the bench line over it
                out["mapping_iter"] = {"error": repr(e)[:300]}
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(cfg, n_rays)
            try:
                out["torch_gpu_baseline"] = dict(cpu_baseline(cfg, n_rays, device=dev),
                                                 what="the ORACLE's unfused torch ops (oracle/spec.py) run on the MI355X -- NOT tiny-cuda-nn / the reference's CUDA "
                                                      "path, which has no ROCm build; a floor for 'any GPU code', not a competitor")
            except Exception as e:                               # informational: never fail the bench line over it
                out["torch_gpu_baseline"] = {"error": repr(e)[:200]}
        sys.stdout.flush()
        libc.fflush(None)
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if group is not None:
        torch.distributed.barrier(group)
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

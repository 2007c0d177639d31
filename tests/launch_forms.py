"""The launch forms of the training forward (train_fwd_plan) and of the eval render (render_plan): how each is forced, which one a
case must get, and the case matrix.  tests/test_launch_plans_host.py pins the plans on the CPU (naruto_debug_train_plan /
naruto_debug_render_plan need no GPU); tests/test_gpu_launch_forms.py runs every form against the oracle."""
import ctypes as C
import json
import os
import subprocess
import sys

FLAT, WALK, PACKED, SHORT, SORTED = range(5)
FORM_NAMES = ("Flat", "Walk", "Packed", "Short", "Sorted")
RENDER_RAY, RENDER_PACKED4, RENDER_PACKED8 = range(3)
RENDER_NAMES = ("k_render_fwd", "k_render_fwd_packed<*, 256>", "k_render_fwd_packed<*, 512>")
LDS_BYTES = 160 * 1024
N_CU = 256                      # MI355X (and the host-only default of a field created without a GPU)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The knobs are read once per process: every form runs in a child interpreter of its own.
TRAIN_ENVS = {
    "flat": {"NARUTO_FWD_SORTED": "0", "NARUTO_FWD_PACKED": "0", "NARUTO_WALK_PARTIAL": "0", "NARUTO_DEBUG_NO_EARLY_EXIT": "1"},
    "unfused": {"NARUTO_DEBUG_NO_FUSED_LOSS_STAGE": "1"},       # Flat + k_loss_stage, or the unfused walk at S = 64 k
    "partial": {"NARUTO_WALK_PARTIAL": "2"},                    # Short at S <= 64, the partial walk at 64 < S <= 384
    "default": {},                                              # (run at S = 64 k only: the exact walk, fused up to 384)
    "packed": {"NARUTO_FWD_PACKED": "2", "NARUTO_FWD_SORTED": "0"},
    "sorted": {"NARUTO_FWD_SORTED": "2"},
}
RENDER_ENVS = {"w0": {"NARUTO_RENDER_WIDE": "0"}, "w2": {"NARUTO_RENDER_WIDE": "2"}, "default": {}}


def short_rays(S):
    """Short's rays per workgroup (short_rays_per_block)."""
    return min(8, max(1, 256 // S))


def packed_rows(S, static_lds, waves=8):
    """Loss rows a Packed workgroup holds (0: the flat launch instead), from the kernel's static LDS."""
    free = LDS_BYTES // (2 if waves == 4 else 1) - static_lds - 256
    rows = 3
    while rows > 0 and rows * 4 * S * (8 * 4 + 2) + 16 > free:
        rows -= 1
    return rows


def render8_rays(S, static_exact512):
    """Rays per group of the eight-wave render (render_packed8_rays), from the fp32 kernel's static LDS."""
    room = LDS_BYTES - (static_exact512 + 1024)
    return min(32, room // (8 * S * 4))


def expected_train(env, S, packed_static):
    """(form, fused) the plan must report for this forcing environment at S samples per ray, or None where the form is not run."""
    exact = S % 64 == 0 and S > 64
    can_fuse = S <= 384
    if env == "flat":
        return FLAT, False
    if env == "unfused":
        return (WALK, False) if exact else (FLAT, False)
    if env == "partial":
        if S <= 64:
            return SHORT, True
        return (WALK, True) if (can_fuse and not exact) else None
    if env == "default":
        return (WALK, can_fuse) if exact else None
    if env == "packed":
        return (PACKED, True) if packed_rows(S, packed_static) > 0 else (FLAT, False)
    if env == "sorted":
        return SORTED, False
    raise KeyError(env)


TRAIN_S = [2, 3, 5, 17, 31, 32, 33, 43, 63, 64, 65, 75, 127, 128, 129, 192, 255, 256, 383, 384, 385, 448, 512, 1000, 1024]


def train_cases():
    """The training matrix: every S with N around the forms' granularity (1; R, R + 1 with R = Short's rays per workgroup at S <= 64,
    else four rays: a walk workgroup / a loss row; an odd count of up to 129, fewer where S is large), plus one count beyond a full
    pass of the capped grid for Short (1 024 workgroups x R) and for Flat at small S (256 eight-wave workgroups x 2 048 tiles)."""
    out = []
    for S in TRAIN_S:
        splits = [(2, 0), (1, 1)] if S == 2 else [(S - min(11, S // 3), min(11, S // 3))]
        R = short_rays(S) if S <= 64 else 4
        odd = max(5, min(129, 1200 // S)) | 1                                   # (the CPU oracle: ~1 ms per sample and iteration)
        Ns = sorted({1, R, R + 1, odd} - {0})
        for nd, nr in splits:
            for N in Ns:
                out.append(dict(S=S, nd=nd, nr=nr, N=N))
    out.append(dict(S=2, nd=2, nr=0, N=1024 * 8 + 1))                           # Short, one workgroup beyond 1 024 x 8 rays
    out.append(dict(S=3, nd=2, nr=1, N=N_CU * 8 * 64 // 3 + 37))                 # Flat: 2 050 tiles on 256 x 8 waves
    # (these two: losses and gradients against the Flat form of the same batch, rgb / depth of a subset of the rays against the oracle)
    for i, c in enumerate(out):
        c["id"] = f"S{c['nd']}+{c['nr']}_N{c['N']}"
        c["perturb"] = i % 2 == 1
        c["seed"] = 300 + i
    return out


# bf16 mode: Short, Walk, Packed and Sorted at a few shapes, against the bf16 Flat form and the exact oracle (batches of at least the
# 64 x 43 samples of the golden batch test_bf16_mode_error_against_the_exact_mode bounds the losses on: they are means)
BF16_CASES = [dict(S=43, nd=32, nr=11, N=65), dict(S=17, nd=12, nr=5, N=165), dict(S=192, nd=181, nr=11, N=16),
              dict(S=75, nd=64, nr=11, N=37), dict(S=384, nd=373, nr=11, N=16)]
for _i, _c in enumerate(BF16_CASES):
    _c.update(id=f"bf16_S{_c['nd']}+{_c['nr']}_N{_c['N']}", perturb=True, seed=700 + _i)

RENDER_S = [2, 3, 17, 31, 32, 33, 43, 61, 62, 63, 64, 65, 128, 129, 1024]


def render_cases(static_exact512):
    """The eval-render matrix: every S with N = 1, R - 1, R, R + 1 of the 256 form (16 rays per group) and of the 512 form (R8(S)),
    an odd 203, and one full pass of the grid-stride loop plus 37 rays for each kernel; with a depth (n_samples_d + n_range_d) at
    even positions of the list, without one (n_samples) at odd ones; want_raw both ways per case."""
    out = []
    for S in RENDER_S:
        Ns = {1, 15, 16, 17, 203}
        if S <= 64:
            r8 = render8_rays(S, static_exact512)
            Ns |= {r8 - 1, r8, r8 + 1}
        else:
            Ns |= {3, 4, 5}
        for N in sorted(Ns):
            out.append(dict(S=S, N=N))
    r8_2, r8_43 = render8_rays(2, static_exact512), render8_rays(43, static_exact512)
    out += [dict(S=2, N=N_CU * r8_2 + 37), dict(S=43, N=N_CU * r8_43 + 37),        # the 512 form: one pass + 37
            dict(S=3, N=N_CU * 4 * 16 + 37),                                       # the 256 form
            dict(S=65, N=N_CU * 4 * 4 + 37)]                                       # k_render_fwd
    for i, c in enumerate(out):
        c["depth"] = i % 2 == 0 and c["S"] >= 3                                 # (n_samples_d >= 2 next to a range sample)
        c["nr"] = min(11, c["S"] // 3) if c["depth"] else 0
        c["seed"] = 500 + i
        c["id"] = f"S{c['S']}_N{c['N']}_{'d' if c['depth'] else 'u'}"
    return out


def static_lds(name):
    """A kernel's static LDS from the built code object (the loader's group_segment_fixed_size)."""
    from naruto_amd import _lib
    return _lib.kernel_resources()[name]["group_segment_fixed_size"]


def train_plan(handle_ptr, t, with_loss=1, deferred=1):
    from naruto_amd import _lib
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().naruto_debug_train_plan(handle_ptr, C.byref(t), with_loss, deferred, out), "naruto_debug_train_plan")
    return list(out)


def render_plan(handle_ptr, n_rays, S, bf16, wide):
    from naruto_amd import _lib
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().naruto_debug_render_plan(handle_ptr, n_rays, S, bf16, wide, out), "naruto_debug_render_plan")
    return list(out)


def run_child(script, args, env_update, timeout):
    """One forced form in a fresh interpreter (the knobs are read once per process); the first failure ends the test."""
    e = dict(os.environ)
    for k in ("NARUTO_FWD_SORTED", "NARUTO_FWD_PACKED", "NARUTO_WALK_PARTIAL", "NARUTO_DEBUG_NO_EARLY_EXIT", "NARUTO_DEBUG_NO_FUSED_LOSS_STAGE",
              "NARUTO_RENDER_WIDE", "NARUTO_PACK_WAVES", "NARUTO_WALK_PARTIAL_MAX", "NARUTO_TV_MOVE"):
        e.pop(k, None)
    e.update(env_update)
    return subprocess.run([sys.executable, str(script), ROOT] + [str(a) for a in args], check=True, env=e, timeout=timeout,
                          capture_output=True, text=True)


def dump(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f)


def train_inputs(c):
    """The case's field (oracle weights), rays with a few depth-less ones, explicit jitter and lattice draws, loss weights."""
    import numpy as np
    import torch
    import helpers as H
    from naruto_amd import synthetic as syn
    cfg = H.office_cfg(12, perturb=1.0 if c["perturb"] else 0.0, n_samples_d=c["nd"], n_range_d=c["nr"])
    ora = H.make_oracle(cfg, 0.25, c["seed"])
    rays = syn.random_rays(c["N"], cfg["mapping"]["bound"], seed=c["seed"], zero_depth_frac=0.2)
    if not (rays["target_d"] > 0).any():                  # the reference's depth loss is a mean over the rays with a depth
        rays = syn.random_rays(c["N"], cfg["mapping"]["bound"], seed=c["seed"], zero_depth_frac=0.0)
    if c["N"] > 1:                                        # the last ray's depth just short of far: its last samples are inside the truncation band
        rays["target_d"][-1] = cfg["cam"]["far"] - 0.03
    rand = torch.rand(c["N"], c["S"], generator=torch.Generator().manual_seed(c["seed"]))
    r6 = torch.from_numpy(np.random.RandomState(c["seed"]).uniform(0, 1, 6).astype(np.float32))
    tr = cfg["training"]
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, SMOOTH_W, 0.0])
    return cfg, ora, rays, rand, r6, w


SMOOTH = (8, 0.1, 0.05)
SMOOTH_W = 0.11


def render_inputs(c):
    import torch
    import helpers as H
    from naruto_amd import synthetic as syn
    if c["depth"]:
        cfg = H.office_cfg(12, perturb=1.0, n_samples_d=c["S"] - c["nr"], n_range_d=c["nr"])
    else:
        cfg = H.office_cfg(12, perturb=1.0)
        cfg["training"]["n_samples"] = c["S"]
    ora = H.make_oracle(cfg, 0.25, c["seed"]).eval()
    rays = syn.random_rays(c["N"], cfg["mapping"]["bound"], seed=c["seed"], zero_depth_frac=0.1)
    rand = torch.rand(c["N"], c["S"], generator=torch.Generator().manual_seed(c["seed"]))
    return cfg, ora, rays, rand

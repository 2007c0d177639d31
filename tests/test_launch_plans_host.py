"""CPU tests of the launch plans (naruto_debug_train_plan / naruto_debug_render_plan: host only, nothing is launched): the LDS every
eval-render launch asks for is what its kernel reserved and what a CU has; the training forward's form for the shipped shapes, the
precedence of the forcing knobs, and that every forcing environment of tests/test_gpu_launch_forms.py selects the form it claims."""
import json
import os

import pytest

import launch_forms as LF

_PLAN_SCRIPT = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import launch_forms as LF
from naruto_amd import _lib, ops
handles = {}
out = []
for c in json.load(open(sys.argv[2])):
    key = (c.get("T", 12), c.get("mode", "fp32"))
    if key not in handles:
        handles[key] = ops.FieldHandle(log2_hashmap_size=key[0], per_level_scale=1.38, uncert_dims=(4, 5, 6), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1),
                                       trunc=0.1, sc_factor=1.0, mlp_mode=key[1])
    t = _lib.NarutoTrainStep()
    t.n_rays, t.n_samples_d, t.n_range_d, t.smooth_points = c["N"], c["nd"], c["nr"], c.get("smooth", 0)
    out.append(LF.train_plan(handles[key].ptr, t, c.get("with_loss", 1), c.get("deferred", 1)))
json.dump(out, open(sys.argv[3], "w"))
"""


def _plans(tmp_path, cases, env, tag):
    script = tmp_path / "plan.py"
    script.write_text(_PLAN_SCRIPT)
    LF.dump(tmp_path / f"{tag}_in.json", cases)
    LF.run_child(script, [tmp_path / f"{tag}_in.json", tmp_path / f"{tag}_out.json"], env, timeout=300)
    return json.load(open(tmp_path / f"{tag}_out.json"))


def _handle(mode="fp32"):
    from naruto_amd import ops
    return ops.FieldHandle(log2_hashmap_size=12, per_level_scale=1.38, uncert_dims=(4, 5, 6), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1),
                           trunc=0.1, sc_factor=1.0, mlp_mode=mode)


def test_render_plan_lds_fits_its_reservation_and_the_cu(built_lib):
    """Every S the render takes x both MLP modes x every NARUTO_RENDER_WIDE setting: the launch's dynamic LDS is within what
    naruto_render_fwd reserved for that kernel (k_render_fwd_packed<*, 512> reserved R8(64)'s 61 440 B and launched up to 62 496 B at
    S = 61 .. 63), the reservation plus the kernel's static LDS (from the code object) fits a CU's 160 KB, and the grid-stride loop
    takes the stated rays per pass."""
    h = {m: _handle(m) for m in ("fp32", "bf16")}
    st = {(m, f): LF.static_lds(k) for m, bf in (("fp32", "false"), ("bf16", "true"))
          for f, k in ((LF.RENDER_RAY, f"k_render_fwd<{bf}>"), (LF.RENDER_PACKED4, f"k_render_fwd_packed<{bf},256>"),
                       (LF.RENDER_PACKED8, f"k_render_fwd_packed<{bf},512>"))}
    exact512 = st[("fp32", LF.RENDER_PACKED8)]
    bad = []
    for mode in ("fp32", "bf16"):
        for wide in (-1, 0, 1, 2):
            for S in list(range(2, 66)) + [127, 128, 129, 384, 1000, 1024]:
                for N in (1, 4097, 20000):
                    form, rpg, blocks, per_pass, dyn, reserved, stat, threads = LF.render_plan(h[mode].ptr, N, S, mode == "bf16", wide)
                    what = f"{mode} wide={wide} S={S} N={N} {LF.RENDER_NAMES[form]}"
                    if dyn > reserved:
                        bad.append(f"{what}: {dyn} B of dynamic LDS, {reserved} reserved")
                    if st[(mode, form)] + reserved > LF.LDS_BYTES:
                        bad.append(f"{what}: static {st[(mode, form)]} + reserved {reserved} > 160 KB")
                    assert stat == st[(mode, form)], f"{what}: the plan's static LDS {stat}, the code object's {st[(mode, form)]}"
                    if S > 64:
                        assert (form, rpg, per_pass, threads, dyn) == (LF.RENDER_RAY, 4, 4096, 256, 4 * 8 * S * 4), what
                    elif form == LF.RENDER_PACKED4:
                        assert (rpg, per_pass, threads, dyn) == (16, 16384, 256, 16 * 8 * S * 4), what
                        assert wide == 0 or (wide in (-1, 1) and (mode == "bf16" or (N + 31) // 32 < LF.N_CU)), what
                    else:
                        r8 = LF.render8_rays(S, exact512)
                        assert form == LF.RENDER_PACKED8 and wide != 0, what
                        assert (rpg, per_pass, threads, dyn) == (r8, LF.N_CU * r8, 512, r8 * 8 * S * 4), what
                        assert wide == 2 or (mode == "fp32" and (N + r8 - 1) // r8 >= LF.N_CU), what
                    assert blocks == min((N + rpg - 1) // rpg, per_pass // rpg), what
    assert not bad, "\n".join(bad[:12]) + f"\n... {len(bad)} launches"
    assert LF.render8_rays(43, exact512) == 32                       # 8 192 rays per pass at the shipped 32 + 11


def test_packed_static_lds_matches_the_code_object(tmp_path, built_lib):
    """Packed's fall-back to the flat launch (not even one row of four rays fits next to its static LDS) is decided on the host from
    the kernel's __shared__ declarations: the S where the plan switches must be where the code object's static LDS puts it, for the
    eight-wave and the four-wave workgroup."""
    for waves, kernel in ((8, "k_query_fwd_loss_packed<false,8>"), (4, "k_query_fwd_loss_packed<false,4>")):
        st = LF.static_lds(kernel)
        assert LF.static_lds(kernel.replace("false", "true")) <= st             # the plan sizes by the fp32 form
        cases = [dict(N=333, nd=S - 11, nr=11) for S in range(12, 1025)]
        plans = _plans(tmp_path, cases, {**LF.TRAIN_ENVS["packed"], "NARUTO_PACK_WAVES": str(waves)}, f"packed{waves}")
        switched = [c["nd"] + c["nr"] for c, p in zip(cases, plans) if p[0] != LF.PACKED]
        first = next(S for S in range(12, 1025) if LF.packed_rows(S, st, waves) == 0)
        assert switched and switched[0] == first and switched == list(range(first, 1025)), (waves, st, switched[:3], first)
        for c, p in zip(cases, plans):
            S = c["nd"] + c["nr"]
            if p[0] == LF.PACKED:
                assert p[1] == 1 and p[6] == min((333 + 3) // 4, LF.N_CU * (2 if waves == 4 else 1)) and p[7] == 64 * waves, (S, p)
            else:
                assert p[:4] == [LF.FLAT, 0, 0, 0], (S, p)


def test_train_plan_defaults_and_precedence(tmp_path, built_lib):
    """The default form of the shipped shapes, and Sorted > Packed > Short > Walk > Flat when several knobs force a form."""
    shipped = [dict(N=2048, nd=32, nr=11, smooth=12), dict(N=2048, nd=117, nr=11, smooth=12), dict(N=131072, nd=32, nr=11, smooth=12),
               dict(N=2048, nd=32, nr=11, T=22, smooth=12), dict(N=8192, nd=32, nr=11), dict(N=333, nd=89, nr=11), dict(N=64, nd=374, nr=11),
               dict(N=64, nd=437, nr=11), dict(N=64, nd=1013, nr=11), dict(N=5, nd=2, nr=0)]
    p = _plans(tmp_path, shipped, {}, "default")
    form = [q[0] for q in p]
    assert form == [LF.SHORT, LF.WALK, LF.SORTED, LF.SORTED, LF.FLAT, LF.WALK, LF.FLAT, LF.WALK, LF.WALK, LF.SHORT], form
    assert p[0][1:4] == [1, 1, 1] and p[0][5] == 5                  # 2 048 x 43: Short, five rays per workgroup, the lattice moved
    assert p[1][1:5] == [1, 1, 1, 2]                                  # 2 048 x 128: the fused two-phase exact walk, five launches
    assert p[5][1:5] == [1, 1, 0, 2]                                  # a partial walk of two tiles (no smoothness term: nothing moved)
    assert p[6][1] == 0 and p[7][1] == 0 and p[8][1] == 0              # 385: flat tiles; 448, 1 024: the exact walk; k_loss_stage in its own launch
    assert p[4][6:8] == [256, 512] and p[2][6:8] == [256, 512]        # the eight-wave flat launch / the list queries
    # precedence of the forcing knobs, at S = 43 and S = 128
    order = [({"NARUTO_FWD_SORTED": "2", "NARUTO_FWD_PACKED": "2", "NARUTO_WALK_PARTIAL": "2"}, LF.SORTED),
             ({"NARUTO_FWD_SORTED": "0", "NARUTO_FWD_PACKED": "2", "NARUTO_WALK_PARTIAL": "2"}, LF.PACKED),
             ({"NARUTO_FWD_SORTED": "0", "NARUTO_FWD_PACKED": "0", "NARUTO_WALK_PARTIAL": "2"}, None),
             ({"NARUTO_FWD_SORTED": "0", "NARUTO_FWD_PACKED": "0", "NARUTO_WALK_PARTIAL": "0"}, None)]
    cases = [dict(N=333, nd=32, nr=11), dict(N=333, nd=89, nr=11), dict(N=333, nd=117, nr=11)]
    for k, (env, want) in enumerate(order):
        got = [q[0] for q in _plans(tmp_path, cases, env, f"prec{k}")]
        if want is not None:
            assert got == [want] * 3, (env, got)
        elif k == 2:
            assert got == [LF.SHORT, LF.WALK, LF.WALK], (env, got)   # Short at S <= 64, else the (partial / exact) walk
        else:
            assert got == [LF.FLAT, LF.FLAT, LF.WALK], (env, got)    # no partial walk: flat tiles, the exact walk at S = 64 k
    # without the loss stage (naruto_debug_train_query_fwd's plan for the forward alone) nothing fused, no Sorted / Packed / Short
    q = _plans(tmp_path, [dict(N=333, nd=32, nr=11, with_loss=0), dict(N=333, nd=117, nr=11, with_loss=0)], {"NARUTO_FWD_SORTED": "2"}, "noloss")
    assert [x[:2] for x in q] == [[LF.FLAT, 0], [LF.WALK, 0]], q


@pytest.mark.parametrize("env", list(LF.TRAIN_ENVS))
def test_train_plan_forced_forms_select_the_claimed_form(tmp_path, built_lib, env):
    """Every case tests/test_gpu_launch_forms.py runs under this forcing environment gets the form it is compared as (Packed's
    fall-back included), in both MLP modes, with its workgroup count."""
    st = LF.static_lds("k_query_fwd_loss_packed<false,8>")
    cases = [dict(c, mode=m) for c in LF.train_cases() + LF.BF16_CASES for m in ("fp32", "bf16")
             if LF.expected_train(env, c["S"], st) is not None]
    plans = _plans(tmp_path, cases, LF.TRAIN_ENVS[env], env)
    for c, p in zip(cases, plans):
        want = LF.expected_train(env, c["S"], st)
        assert (p[0], bool(p[1])) == want, (env, c, p)
        S, N = c["S"], c["N"]
        if p[0] == LF.SHORT:
            assert p[5] == LF.short_rays(S) and p[6] == min((N + p[5] - 1) // p[5], 4 * LF.N_CU), (c, p)
        elif p[0] == LF.WALK:
            assert p[4] == (S + 63) // 64 and p[6] == min((N + 3) // 4, 4 * LF.N_CU), (c, p)
        elif p[0] == LF.FLAT:
            tiles = (N * S + 63) // 64
            want_wg = ((tiles + 1) // 2, 128) if 4 * LF.N_CU < tiles < 8 * LF.N_CU else (LF.N_CU, 512) if tiles >= 8 * LF.N_CU else (min((tiles + 3) // 4, 4 * LF.N_CU), 256)
            assert tuple(p[6:8]) == want_wg, (c, p)
    # the beyond-one-pass cases really are beyond one pass
    big = {c["id"]: p for c, p in zip(cases, plans) if c["N"] > 8000 and c["mode"] == "fp32"}
    if env == "partial":
        assert big["S2+0_N8193"][6] == 4 * LF.N_CU and (8193 + 7) // 8 > 4 * LF.N_CU
    if env == "flat":
        assert big["S2+1_N43727"][6:8] == [LF.N_CU, 512] and (43727 * 3 + 63) // 64 > 8 * LF.N_CU


def test_debug_plans_validate_arguments(built_lib):
    import ctypes as C
    from naruto_amd import _lib
    out = (C.c_uint32 * 8)()
    h = _handle()
    assert built_lib.naruto_debug_render_plan(h.ptr, 16, 1, 0, -1, out) == -22
    assert built_lib.naruto_debug_render_plan(h.ptr, 16, 1025, 0, -1, out) == -22
    assert built_lib.naruto_debug_render_plan(h.ptr, 16, 43, 0, 3, out) == -22
    assert built_lib.naruto_debug_render_plan(None, 16, 43, 0, -1, out) == -22
    t = _lib.NarutoTrainStep()
    t.n_rays, t.n_samples_d = 0, 43
    assert built_lib.naruto_debug_train_plan(h.ptr, C.byref(t), 1, 1, out) == -22
    t.n_rays = 5
    assert built_lib.naruto_debug_train_plan(h.ptr, C.byref(t), 1, 1, out) == 0
    assert built_lib.naruto_debug_train_plan(h.ptr, None, 1, 1, out) == -22

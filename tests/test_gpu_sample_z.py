"""Depth sampling (stage A1) against its float32 twin (sample_z_spec.py), bit for bit: the stand-alone kernel over its parameters at
the depths where a rank can go wrong (a near-surface sample meeting a uniform one exactly and one ulp either side, plus the special
depths), exact ties, rays without a depth, and z_vals of every launch form that samples -- each training-forward form with explicit
and device-drawn jitter, each eval-render kernel -- forced in a child interpreter of its own (launch_forms.py).

Every comparison is sample_z_spec.mismatch: the uint32 view of the non-NaN elements, and the NaN positions (not the NaN bits: the
payload and sign of inf - inf differ between the host and the device).  A failure names the setting and the ray's depth (float.hex)."""
import numpy as np
import pytest
import torch

import launch_forms as LF
import sample_z_spec as Z

pytestmark = pytest.mark.gpu


def _kernel(gpu, n, d, near, far, nd, nr, rd, rand=None, n_samples=0):
    from naruto_amd import ops
    got = ops.sample_z(n, None if d is None else torch.from_numpy(d).to(gpu), near, far, nd, nr, rd, n_samples=n_samples,
                       rand=None if rand is None else torch.from_numpy(rand).to(gpu), device=gpu)
    return got.cpu().numpy()


# ---- a. the stand-alone kernel over its parameters ----
@pytest.mark.parametrize("jittered", [False, True], ids=["plain", "rand"])
@pytest.mark.parametrize("near,far", Z.NEAR_FAR)
def test_kernel_over_its_parameters(gpu, near, far, jittered):
    """k_sample_z at every (n_samples_d, n_range_d, range_d) of the grid with 2 <= S <= 1 024: the special depths, the boundary depths
    of the setting and 256 random ones; without jitter, and with an explicit rand whose first two rows are all 0 and all 1 - 2^-24."""
    bad = []
    for setting in Z.grid(near, far):
        _, _, nd, nr, rd = setting
        d, rand = Z.setting_inputs(setting)
        r = rand if jittered else None
        got = _kernel(gpu, len(d), d, near, far, nd, nr, rd, rand=r)
        msg = Z.mismatch(got, Z.sample_z(len(d), d, near, far, nd, nr, rd, rand=r), d, f"{setting} {'rand' if jittered else 'no jitter'}")
        if msg:
            bad.append(msg)
    assert not bad, f"{len(bad)} settings differ from the twin:\n" + "\n".join(bad[:20])


# ---- b. exact ties ----
def test_exact_ties(gpu):
    """near 0, far 4, 33 + 5 samples, range_d 0.25: both steps are 0.125 and every value is exact, so at a depth k / 8 every
    near-surface sample that lies in [0, 4] equals a uniform one.  The row is the twin's, and each duplicate sits next to its equal."""
    near, far, nd, nr, rd = 0.0, 4.0, 33, 5, 0.25
    d = (np.arange(1, 41) / 8.0).astype(np.float32)
    got = _kernel(gpu, len(d), d, near, far, nd, nr, rd)
    msg = Z.mismatch(got, Z.sample_z(len(d), d, near, far, nd, nr, rd), d, "ties")
    assert msg is None, msg
    uniform = set((np.arange(33) / 8.0).tolist())
    for n, k in enumerate(range(1, 41)):
        dup = [(k + j) / 8.0 for j in (-2, -1, 0, 1, 2) if (k + j) / 8.0 in uniform]
        row = got[n].tolist()
        assert len(dup) == max(0, min(k + 2, 32) - max(k - 2, 0) + 1), (k, dup)      # 5 of 5 for 2 <= k <= 30
        for v in dup:
            i = row.index(v)
            assert row[i + 1] == v and row.count(v) == 2, f"depth {float(d[n]).hex()}: {v} is not next to its equal in {row}"
    rand = Z.form_rand(len(d), nd + nr, 5)
    msg = Z.mismatch(_kernel(gpu, len(d), d, near, far, nd, nr, rd, rand=rand), Z.sample_z(len(d), d, near, far, nd, nr, rd, rand=rand), d, "ties, rand")
    assert msg is None, msg


# ---- c. no measured depth ----
@pytest.mark.parametrize("n_samples", [2, 3, 63, 64, 65, 1024])
def test_no_measured_depth(gpu, n_samples):
    for near, far in Z.NEAR_FAR:
        rand = Z.form_rand(5, n_samples, n_samples)
        for r in (None, rand):
            got = _kernel(gpu, 5, None, near, far, 0, 0, 0.0, rand=r, n_samples=n_samples)
            msg = Z.mismatch(got, Z.sample_z(5, None, near, far, 0, 0, 0.0, rand=r, n_samples=n_samples), None,
                             f"no depth, ({near}, {far}), n_samples {n_samples}, {'rand' if r is not None else 'no jitter'}")
            assert msg is None, msg


# ---- d. every launch form that samples ----
_HEAD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import helpers as H, launch_forms as LF, sample_z_spec as Z
from naruto_amd import ops, synthetic as syn
gpu = torch.device("cuda", 0)
cases, out_dir = json.load(open(sys.argv[2])), sys.argv[3]
for c in cases:
    nd, nr, S = c["nd"], c["nr"], c["nd"] + c["nr"]
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=nd, n_range_d=nr)
    tr, cam = cfg["training"], cfg["cam"]
    d = Z.form_depths(cam["near"], cam["far"], nd, nr, tr["range_d"])
    N = len(d)
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=c["seed"])
    ro, rd, rgb = (torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb"))
    td = torch.from_numpy(d).to(gpu)
    rand = torch.from_numpy(Z.form_rand(N, S, c["seed"])).to(gpu)
"""

_TRAIN_CHILD = _HEAD + r"""
    m = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.25, c["seed"]), gpu)
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, LF.SMOOTH_W, 0.0])
    res = {}
    for rng in (False, True):
        ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=nd, n_range_d=nr, near=cam["near"],
                           far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True,
                           loss_weights=w.to(gpu), smooth=LF.SMOOTH, device_rng=rng, seed=c["seed"] if rng else None)
        res["plan_rng" if rng else "plan_rand"] = np.array(LF.train_plan(m._handle().ptr, ts.t), np.int64)
        if rng:
            for it in range(2):
                ts.run(ro, rd, rgb, td)
                torch.cuda.synchronize()
                res[f"z_rng{it}"] = ts.z_vals.cpu().numpy().copy()
            res["rng_state"] = ts.rng_state.cpu().numpy()
        else:
            ts.rand[N * S:].fill_(0.5)
            ts.run(ro, rd, rgb, td, rand=rand)
            torch.cuda.synchronize()
            res["z_rand"] = ts.z_vals.cpu().numpy().copy()
    np.savez(f"{out_dir}/{c['id']}.npz", **res)
"""

_RENDER_CHILD = _HEAD + r"""
    m = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.25, c["seed"]), gpu).eval()
    res = {"plan": np.array(LF.render_plan(m._handle().ptr, N, S, 0, -1), np.int64)}
    kw = dict(near=cam["near"], far=cam["far"], range_d=tr["range_d"], want_raw=True)
    with torch.no_grad():
        if c["depth"]:
            res["z_rand"] = ops.render_fused(m._handle(), m._params(), ro, rd, td, n_samples_d=nd, n_range_d=nr, rand=rand, **kw)["z_vals"].cpu().numpy()
            res["z_plain"] = ops.render_fused(m._handle(), m._params(), ro, rd, td, n_samples_d=nd, n_range_d=nr, **kw)["z_vals"].cpu().numpy()
        else:
            res["z_rand"] = ops.render_fused(m._handle(), m._params(), ro, rd, None, n_samples_d=0, n_range_d=0, n_samples=S, rand=rand, **kw)["z_vals"].cpu().numpy()
    torch.cuda.synchronize()
    np.savez(f"{out_dir}/{c['id']}.npz", **res)
"""


def _cases(with_no_depth):
    cs = [dict(nd=nd, nr=nr, depth=True, seed=40 + i, id=f"S{nd}+{nr}") for i, (nd, nr) in enumerate(Z.FORM_SPLITS)]
    if with_no_depth:
        cs.append(dict(nd=32, nr=11, depth=False, seed=50, id="S43_no_depth"))
    return cs


def _run(tmp_path, child, envs, cases_for):
    script = tmp_path / "child.py"
    script.write_text(child)
    out = {}
    for env, update in envs.items():
        cases = cases_for(env)
        if not cases:
            continue
        d = tmp_path / env
        d.mkdir()
        LF.dump(tmp_path / f"{env}.json", cases)
        LF.run_child(script, [tmp_path / f"{env}.json", d], update, timeout=300)
        out[env] = {c["id"]: dict(np.load(d / f"{c['id']}.npz")) for c in cases}
    return out


def _setting(c):
    import helpers as H
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=c["nd"], n_range_d=c["nr"])
    return float(cfg["cam"]["near"]), float(cfg["cam"]["far"]), c["nd"], c["nr"], float(cfg["training"]["range_d"])


def test_training_forms_sample_the_twins_z_vals(gpu, tmp_path):
    """ts.z_vals of Flat, Flat + k_loss_stage / the unfused walk, Short, the partial and the exact walk, Packed and Sorted at
    S = 43, 64, 75 and 128 (75 is there for the partial walk: at 43 and 64 the partial environment runs Short, and 128 is the exact
    walk's), on the boundary depths of each setting plus 0, -1, NaN and far: with an explicit rand, and
    with the device generator for two consecutive iterations (the twin: counters 0 and 1).  The plan each case reports is the one
    launch_forms.expected_train names."""
    st = LF.static_lds("k_query_fwd_loss_packed<false,8>")
    cases = _cases(False)
    res = _run(tmp_path, _TRAIN_CHILD, LF.TRAIN_ENVS, lambda env: [c for c in cases if LF.expected_train(env, c["nd"] + c["nr"], st) is not None])
    bad, forms = [], set()
    for c in cases:
        near, far, nd, nr, rd = _setting(c)
        d = Z.form_depths(near, far, nd, nr, rd)
        N, S = len(d), nd + nr
        want = {"z_rand": Z.sample_z(N, d, near, far, nd, nr, rd, rand=Z.form_rand(N, S, c["seed"])),
                "z_rng0": Z.sample_z(N, d, near, far, nd, nr, rd, rng=(c["seed"], 0)),
                "z_rng1": Z.sample_z(N, d, near, far, nd, nr, rd, rng=(c["seed"], 1))}
        for env, rs in res.items():
            if c["id"] not in rs:
                continue
            r = rs[c["id"]]
            expect = LF.expected_train(env, S, st)
            for k in ("plan_rand", "plan_rng"):
                plan = [int(x) for x in r[k]]
                assert (plan[0], bool(plan[1])) == expect, f"{env} {c['id']} {k}: the plan says {plan}, the test claims {expect}"
            forms.add((env, LF.FORM_NAMES[expect[0]], expect[1], S))
            assert r["rng_state"].tolist() == [c["seed"], 2], f"{env} {c['id']}: rng state {r['rng_state'].tolist()}"
            for k, w in want.items():
                msg = Z.mismatch(r[k], w, d, f"train {env} ({LF.FORM_NAMES[expect[0]]}) {(near, far, nd, nr, rd)} {k}")
                if msg:
                    bad.append(msg)
    reached = {(f, S > 64 and S % 64 != 0) for _, f, _, S in forms}
    assert {("Flat", False), ("Short", False), ("Walk", True), ("Walk", False), ("Packed", False), ("Sorted", False)} <= reached, sorted(forms)
    print("\n".join(f"train {e}: {f} {'fused' if u else 'unfused'} S={S}" for e, f, u, S in sorted(forms)))
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])


def _expected_render(env, N, S, exact512):
    if S > 64:
        return LF.RENDER_RAY
    if env != "default":
        return LF.RENDER_PACKED4 if env == "w0" else LF.RENDER_PACKED8
    r8 = LF.render8_rays(S, exact512)
    return LF.RENDER_PACKED8 if (N + r8 - 1) // r8 >= LF.N_CU else LF.RENDER_PACKED4


def test_render_forms_sample_the_twins_z_vals(gpu, tmp_path):
    """z_vals of naruto_render_fwd's three kernels (S = 43 and 64: both packed forms; 75 and 128: k_render_fwd) in every render
    environment, on the same depths with and without jitter, and one case without a depth."""
    exact512 = LF.static_lds("k_render_fwd_packed<false,512>")
    cases = _cases(True)
    res = _run(tmp_path, _RENDER_CHILD, LF.RENDER_ENVS, lambda env: cases)
    bad, forms = [], set()
    for c in cases:
        near, far, nd, nr, rd = _setting(c)
        d = Z.form_depths(near, far, nd, nr, rd)
        N, S = len(d), nd + nr
        rand = Z.form_rand(N, S, c["seed"])
        if c["depth"]:
            want = {"z_rand": Z.sample_z(N, d, near, far, nd, nr, rd, rand=rand), "z_plain": Z.sample_z(N, d, near, far, nd, nr, rd)}
        else:
            want = {"z_rand": Z.sample_z(N, None, near, far, 0, 0, 0.0, rand=rand, n_samples=S)}
        for env, rs in res.items():
            r = rs[c["id"]]
            expect = _expected_render(env, N, S, exact512)
            assert int(r["plan"][0]) == expect, f"render {env} {c['id']}: plan {r['plan'].tolist()}, the test claims {expect}"
            forms.add((env, LF.RENDER_NAMES[expect], S))
            for k, w in want.items():
                msg = Z.mismatch(r[k], w, d if c["depth"] else None, f"render {env} ({LF.RENDER_NAMES[expect]}) {c['id']} {k}")
                if msg:
                    bad.append(msg)
    assert {f for _, f, _ in forms} == set(LF.RENDER_NAMES), sorted(forms)
    print("\n".join(f"render {e}: {f} S={S}" for e, f, S in sorted(forms)))
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:20])

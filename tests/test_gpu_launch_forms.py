"""Every launch form of the training forward and of the eval render against the CPU oracle.  Each form is forced by its environment
(tests/launch_forms.py) in a child interpreter of its own, which runs the whole case list, writes one .npz per case and records the
plan naruto_debug_train_plan / naruto_debug_render_plan reports; the parent computes the oracle once per case and compares every form
with it, and asserts the recorded form (a silent fall-back to another form fails)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import spec_torch as S

import helpers as H
import launch_forms as LF

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
BIG = 8000                  # N x S beyond which a case is checked against the Flat form (losses, gradients) and on a ray subset (oracle)

_TRAIN_CHILD = r"""
import ctypes as C, json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import helpers as H, launch_forms as LF
from naruto_amd import _lib, ops
gpu = torch.device("cuda", 0)
lib = _lib.load()
cases, out_dir = json.load(open(sys.argv[2])), sys.argv[3]
for i, c in enumerate(cases):
    cfg, ora, rays, rand, r6, w = LF.train_inputs(c)
    if c.get("mode") == "bf16":
        cfg["decoder"]["mlp_precision"] = "bf16"
    tr, cam = cfg["training"], cfg["cam"]
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    N, S = c["N"], c["S"]
    ug = torch.zeros_like(m.uncert_grid)
    ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=c["nd"], n_range_d=c["nr"], near=cam["near"], far=cam["far"],
                       range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=c["perturb"],
                       loss_weights=w.to(gpu), smooth=LF.SMOOTH, device_rng=False)
    args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]
    ts.rand[N * S:].copy_(r6.to(gpu))
    res = {"plan": np.array(LF.train_plan(m._handle().ptr, ts.t), np.int64)}
    if i == 0:
        # ABI: a forward on its own leaves raw / rgb / depth as the full iteration does; feat_save = NULL is refused, nothing launched
        ts.run_forward(*args, rand=rand.to(gpu))
        torch.cuda.synchronize()
        res.update(fwd_raw=ts.raw.cpu().numpy().copy(), fwd_rgb=ts.rgb.cpu().numpy().copy(), fwd_depth=ts.depth.cpu().numpy().copy())
        keep = ts.t.feat_save
        ts.t.feat_save = None
        res["null_feat_save_rc"] = np.array(lib.naruto_train_forward(ts.handle.ptr, C.byref(ts.ps), C.byref(ts.t), 1, None))
        ts.t.feat_save = keep
    losses = ts.run(*args, rand=rand.to(gpu))
    torch.cuda.synchronize()
    res.update(losses=losses.cpu().numpy(), rgb=ts.rgb.cpu().numpy(), depth=ts.depth.cpu().numpy(), raw=ts.raw.cpu().numpy(),
               z_vals=ts.z_vals.cpu().numpy(), active=(ts.d_raw.abs().sum(-1) > 0).cpu().numpy(), g_uncert_grid=ug.cpu().numpy())
    res.update({"g_" + k: v.detach().cpu().numpy() for k, v in ts.grads.items()})
    np.savez(f"{out_dir}/{c['id']}_{c.get('mode', 'fp32')}.npz", **res)
"""

_RENDER_CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import helpers as H, launch_forms as LF
gpu = torch.device("cuda", 0)
cases, out_dir = json.load(open(sys.argv[2])), sys.argv[3]
for c in cases:
    cfg, ora, rays, rand = LF.render_inputs(c)
    if c.get("mode") == "bf16":
        cfg["decoder"]["mlp_precision"] = "bf16"
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    ro, rd = torch.from_numpy(rays["rays_o"]).to(gpu), torch.from_numpy(rays["rays_d"]).to(gpu)
    td = torch.from_numpy(rays["target_d"]).to(gpu) if c["depth"] else None
    res = {"plan": np.array(LF.render_plan(m._handle().ptr, c["N"], c["S"], int(c.get("mode") == "bf16"), -1), np.int64)}
    with torch.no_grad():
        a = m.render_rays(ro, rd, target_d=td, rand=rand.to(gpu))
        b = m.render_rays(ro, rd, target_d=td, rand=rand.to(gpu), want_raw=False)
        if c.get("mode") == "bf16":
            o = m.render_rays(ro, rd, target_d=td, rand=rand.to(gpu), fused=False)
            res.update({"ops_" + k: v.cpu().numpy() for k, v in o.items() if torch.is_tensor(v)})
    torch.cuda.synchronize()
    res.update({k: v.cpu().numpy() for k, v in a.items() if torch.is_tensor(v)})
    res.update({"noraw_" + k: v.cpu().numpy() for k, v in b.items() if torch.is_tensor(v)})
    np.savez(f"{out_dir}/{c['id']}_{c.get('mode', 'fp32')}.npz", **res)
"""


def _run_forms(tmp_path, child, envs, cases_for, timeout):
    script = tmp_path / "child.py"
    script.write_text(child)
    out = {}
    for name, env in envs.items():
        cases = cases_for(name)
        if not cases:
            continue
        d = tmp_path / name
        d.mkdir()
        LF.dump(tmp_path / f"{name}.json", cases)
        LF.run_child(script, [tmp_path / f"{name}.json", d], env, timeout=timeout)
        out[name] = {(c["id"], c.get("mode", "fp32")): dict(np.load(d / f"{c['id']}_{c.get('mode', 'fp32')}.npz")) for c in cases}
    return out


def _report(lines):
    path = os.environ.get("NARUTO_LAUNCH_FORMS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def _oracle_train(c):
    cfg, ora, rays, rand, r6, w = LF.train_inputs(c)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    ora.train()
    ret = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand if c["perturb"] else None)
    total = S.total_loss(ret, cfg["training"]) + LF.SMOOTH_W * S.smoothness(ora, *LF.SMOOTH, r6[:3], r6[3:])
    total.backward()
    return cfg, ora, t, ret, total


def _oracle_train_subset(c, idx):
    cfg, ora, rays, rand, r6, w = LF.train_inputs(c)
    t = {k: torch.from_numpy(v)[idx] for k, v in rays.items()}
    ora.train()
    with torch.no_grad():
        ret = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand[idx] if c["perturb"] else None)
    return ret


def _check_train_vs_oracle(c, r, cfg, ora, t, ret_o, total_o, what):
    bad = []

    def close(a, b, tol, name, rel=0.0):
        try:
            H.assert_close(torch.as_tensor(a), b, tol, f"{what}: {name}", rel=rel)
        except AssertionError as e:
            bad.append(str(e)[:300])
    losses = r["losses"]
    for i, k in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")):
        close(losses[i:i + 1], ret_o[k].detach().reshape(-1), 1e-6, k, rel=1e-4)
    close(losses[5:6], ret_o["uncert_loss"].detach().reshape(-1), 1e-5, "uncert_loss", rel=1e-4)
    close(losses[9:10], total_o.detach().reshape(-1), 1e-5, "total", rel=1e-4)
    close(r["rgb"], ret_o["rgb"].detach(), 1e-5, "rgb")
    close(r["depth"], ret_o["depth"].detach(), 1e-5, "depth", rel=1e-5)
    _, n_kink = H.relu_kink_distance(ora, cfg, t["rays_o"], t["rays_d"], torch.from_numpy(r["z_vals"]), torch.from_numpy(r["active"]))
    go = H.ora_grads(ora)
    budget = {"table": 128 * n_kink, "sdf_w0": 80 * n_kink, "col_w0": 63 * n_kink, "sdf_w1": 0, "col_w1": 0}
    for k in budget:
        got, want = torch.from_numpy(r["g_" + k]).reshape(-1).double(), go[k].reshape(-1).double()
        scale = max(float(want.abs().max()), 1e-12)
        n_bad = int(((got - want).abs() > 1e-4 * scale + 1e-3 * want.abs()).sum())
        if n_bad > budget[k]:
            bad.append(f"{what}: grad.{k}: {n_bad} entries beyond tolerance (allowed {budget[k]}), max err {float((got - want).abs().max()):.3e}, scale {scale:.3e}")
    try:
        H.grad_close(torch.from_numpy(r["g_uncert_grid"]).reshape(-1), ora.uncert_grid.grad.reshape(-1), f"{what}: grad.uncert_grid")
    except AssertionError as e:
        bad.append(str(e)[:300])
    return bad


def _check_vs_twin(r, ref, what, frac=2e-5):
    bad = []
    for k in ["losses", "rgb", "depth"] + [k for k in ref if k.startswith("g_")]:
        a, b = r[k].astype(np.float64), ref[k].astype(np.float64)
        scale = max(float(np.abs(b).max()), 1e-12)
        if not np.isfinite(a).all() or float(np.abs(a - b).max()) > frac * scale:
            bad.append(f"{what}: {k} differs from the Flat form by {float(np.abs(a - b).max()):.3e} (scale {scale:.3e})")
    return bad


def test_training_forms_against_the_oracle(gpu, tmp_path):
    """Flat, Flat / walk with k_loss_stage in its own launch, Short, the partial and the exact walk (fused and unfused), Packed and
    Sorted at S = 2 .. 1 024 and ray counts around each form's granularity, in the fp32 mode against the oracle (losses 1e-6 / 1e-4
    relative, total 1e-5, rgb / depth 1e-5, gradients per entry with the ReLU-kink budget of test_train_step_random_shapes); the bf16
    mode's Short / Walk / Packed / Sorted against the bf16 Flat form and, with the bounds of test_bf16_mode_error_against_the_exact_mode
    (up to the 192 samples per ray those were measured near), the oracle.  Under every form a forward on its own leaves raw / rgb / depth as the iteration does, and feat_save = NULL is refused."""
    st = LF.static_lds("k_query_fwd_loss_packed<false,8>")
    all_cases = LF.train_cases()
    bf_envs = {"flat", "partial", "default", "packed", "sorted"}

    def cases_for(env):
        cs = [c for c in all_cases if LF.expected_train(env, c["S"], st) is not None]
        if env in bf_envs:
            cs += [dict(c, mode="bf16") for c in LF.BF16_CASES if LF.expected_train(env, c["S"], st) is not None]
        return cs
    res = _run_forms(tmp_path, _TRAIN_CHILD, LF.TRAIN_ENVS, cases_for, timeout=900)
    bad, report = [], []
    for env, rs in res.items():
        ran = {}
        for (cid, mode), r in rs.items():
            c = next(x for x in all_cases + LF.BF16_CASES if x["id"] == cid)
            want = LF.expected_train(env, c["S"], st)
            plan = [int(x) for x in r["plan"]]
            assert (plan[0], bool(plan[1])) == want, f"{env} {cid} {mode}: the plan says {plan}, the test claims {want}"
            ran.setdefault((LF.FORM_NAMES[plan[0]], "fused" if plan[1] else "unfused", mode), []).append(f"{c['S']}x{c['N']}")
            if "null_feat_save_rc" in r:
                assert int(r["null_feat_save_rc"]) == -22, f"{env}: feat_save = NULL was not refused ({int(r['null_feat_save_rc'])})"
                for k in ("raw", "rgb", "depth"):
                    assert np.array_equal(r["fwd_" + k], r[k]), f"{env} {cid}: {k} of the forward alone differs from the iteration's"
        report += [f"train {env}: {f} {u} {m}: " + " ".join(v) for (f, u, m), v in sorted(ran.items())]
    oracle_cache = {}
    for c in all_cases:
        forms = [(env, rs[(c["id"], "fp32")]) for env, rs in res.items() if (c["id"], "fp32") in rs]
        if c["N"] * c["S"] > BIG:
            ref = res["flat"][(c["id"], "fp32")]
            idx = torch.cat([torch.arange(0, 37), torch.arange(c["N"] - 101, c["N"])])
            ret_o = _oracle_train_subset(c, idx)
            for env, r in forms:
                what = f"{env} {c['id']}"
                try:
                    H.assert_close(torch.from_numpy(r["rgb"])[idx], ret_o["rgb"], 1e-5, f"{what}: rgb (ray subset)")
                    H.assert_close(torch.from_numpy(r["depth"])[idx], ret_o["depth"], 1e-5, f"{what}: depth (ray subset)", rel=1e-5)
                except AssertionError as e:
                    bad.append(str(e)[:300])
                if env != "flat":
                    bad += _check_vs_twin(r, ref, what)
            continue
        cfg, ora, t, ret_o, total_o = oracle_cache.setdefault(c["id"], _oracle_train(c))
        for env, r in forms:
            bad += _check_train_vs_oracle(c, r, cfg, ora, t, ret_o, total_o, f"{env} {c['id']} (plan {list(r['plan'])})")
        oracle_cache.pop(c["id"])
    # bf16: each form against the bf16 Flat form, and all of them against the exact oracle within the bf16 mode's bounds
    for c in LF.BF16_CASES:
        ref = res["flat"][(c["id"], "bf16")]
        cfg, ora, t, ret_o, total_o = _oracle_train(c)
        go = H.ora_grads(ora)
        go["uncert_grid"] = ora.uncert_grid.grad
        for env, rs in res.items():
            if (c["id"], "bf16") not in rs:
                continue
            r, what = rs[(c["id"], "bf16")], f"bf16 {env} {c['id']}"
            if env != "flat":
                bad += _check_vs_twin(r, ref, what)
            if c["S"] > 192:        # the bounds were measured at 43 and 128 samples; longer rays (384: fs_loss 2.2e-4 in every form) only vs Flat
                continue
            bound = {"rgb_loss": 3e-4, "depth_loss": 1.5e-2, "sdf_loss": 1e-4, "fs_loss": 2e-4, "uncert_loss": 1e-2}
            for i, nm in ((0, "rgb_loss"), (1, "depth_loss"), (2, "sdf_loss"), (3, "fs_loss"), (5, "uncert_loss")):
                la, lb = float(ret_o[nm]), float(r["losses"][i])
                if not abs(la - lb) <= bound[nm] * abs(la):
                    bad.append(f"{what}: {nm}: oracle {la} bf16 {lb}")
            if not abs(float(total_o) - float(r["losses"][9])) <= 1e-3 * abs(float(total_o)):
                bad.append(f"{what}: total: oracle {float(total_o)} bf16 {float(r['losses'][9])}")
            for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1", "uncert_grid"):
                x, y = torch.from_numpy(r["g_" + k]).reshape(-1).double(), go[k].reshape(-1).double()
                cos = float((x @ y) / (x.norm() * y.norm() + 1e-300))
                if cos < 0.985:
                    bad.append(f"{what}: grad {k}: cosine {cos:.6f} against the oracle")
    _report(report)
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:30])


def _expected_render(env, c, exact512):
    S, N = c["S"], c["N"]
    if S > 64:
        return LF.RENDER_RAY
    if env == "w0":
        return LF.RENDER_PACKED4
    if env == "w2":
        return LF.RENDER_PACKED8
    r8 = LF.render8_rays(S, exact512)
    return LF.RENDER_PACKED8 if c.get("mode") != "bf16" and (N + r8 - 1) // r8 >= LF.N_CU else LF.RENDER_PACKED4


def test_eval_render_forms_against_the_oracle(gpu, tmp_path):
    """naruto_render_fwd's three kernels (the 256-thread and 512-thread packed forms, k_render_fwd above 64 samples) at S = 2 .. 1 024,
    with and without a depth, N = 1, around each form's rays per group, and one full pass of the grid-stride loop + 37 rays (the
    second pass reuses the ray images: the barrier behind a group is exercised), want_raw both ways: raw, z_vals and every map against
    the oracle's render_rays (rays of the larger batches: the first 37 and the last 101, the second pass's); bf16 mode: both packed forms
    against the operator chain at the 2e-3 of test_render_fused_equals_the_three_operators."""
    exact512 = LF.static_lds("k_render_fwd_packed<false,512>")
    all_cases = LF.render_cases(exact512)
    bf_cases = [dict(S=17, N=203, depth=True, nr=5, seed=900, mode="bf16"), dict(S=43, N=8229, depth=True, nr=11, seed=901, mode="bf16"),
                dict(S=64, N=61, depth=False, nr=0, seed=902, mode="bf16")]
    for c in bf_cases:
        c["id"] = f"bf16_S{c['S']}_N{c['N']}"

    def cases_for(env):
        cs = [c for c in all_cases if env == "default" or c["S"] <= 64]
        return cs + (bf_cases if env != "default" else [])
    res = _run_forms(tmp_path, _RENDER_CHILD, LF.RENDER_ENVS, cases_for, timeout=900)
    bad, report = [], []
    for env, rs in res.items():
        ran = {}
        for (cid, mode), r in rs.items():
            c = next(x for x in all_cases + bf_cases if x["id"] == cid)
            plan = [int(x) for x in r["plan"]]
            assert plan[0] == _expected_render(env, c, exact512), f"render {env} {cid} {mode}: plan {plan}"
            assert plan[4] <= plan[5], f"render {env} {cid}: {plan[4]} B of dynamic LDS, {plan[5]} reserved"
            ran.setdefault((LF.RENDER_NAMES[plan[0]], mode), []).append(f"{c['S']}x{c['N']}{'' if c['N'] <= plan[3] else '(2 passes)'}")
        report += [f"render {env}: {f} {m}: " + " ".join(v) for (f, m), v in sorted(ran.items())]
    for c in all_cases:
        cfg, ora, rays, rand = LF.render_inputs(c)
        idx = torch.arange(c["N"]) if c["N"] <= 2000 else torch.cat([torch.arange(0, 37), torch.arange(c["N"] - 101, c["N"])])
        ro, rd, td = (torch.from_numpy(rays[k])[idx] for k in ("rays_o", "rays_d", "target_d"))
        with torch.no_grad():
            o = ora.render_rays(ro, rd, target_d=td if c["depth"] else None, rand=rand[idx])
        for env, rs in res.items():
            if (c["id"], "fp32") not in rs:
                continue
            r, what = rs[(c["id"], "fp32")], f"render {env} {c['id']}"
            try:
                for pre in ("", "noraw_"):
                    for k in ("rgb", "depth", "acc_map", "depth_var", "uncert_map"):
                        H.assert_close(torch.from_numpy(r[pre + k])[idx], o[k], TOL_OUT, f"{what}: {pre}{k}")
                    H.assert_close(torch.from_numpy(r[pre + "disp_map"])[idx], o["disp_map"], TOL_OUT, f"{what}: {pre}disp_map", rel=1e-4)
                for k in ("raw", "z_vals"):
                    H.assert_close(torch.from_numpy(r[k])[idx], o[k], TOL_OUT, f"{what}: {k}")
                assert "noraw_raw" not in r and "noraw_z_vals" not in r
            except AssertionError as e:
                bad.append(str(e)[:300])
    for env, rs in res.items():
        for c in bf_cases:
            if (c["id"], "bf16") not in rs:
                continue
            r, what = rs[(c["id"], "bf16")], f"render bf16 {env} {c['id']}"
            for k in ("raw", "rgb", "depth", "disp_map", "acc_map", "depth_var", "uncert_map"):
                try:
                    H.assert_close(torch.from_numpy(r[k]), torch.from_numpy(r["ops_" + k]), 2e-3, f"{what}: {k}", rel=1e-5)
                except AssertionError as e:
                    bad.append(str(e)[:300])
    _report(report)
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:30])

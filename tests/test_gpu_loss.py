"""The loss stage and its backward against their fp64 twin (tests/loss_spec.py), term by term.

A. The modular operators (ops.composite, ops.render_loss; naruto_loss_sums / naruto_loss_bwd / naruto_compact_active /
   naruto_composite_bwd through ctypes) on hand-made raw / z_vals: ordinary batches with one ray per edge embedded, and the
   degenerate batches.
B. The training path (ops.TrainStep) on the device's own raw: after each run ts.raw and ts.z_vals go to the twin, which is compared
   with ts.rgb / depth / uncert_map / sums / losses / d_raw -- six weightings (five one-hot, the reference's) over four backward
   routes (the tail deferred into k_loss_bwd_fused; run_forward | run_backward; the sums given, with a second batch's sums added
   on the host as a second rank's would be; NARUTO_DEBUG_NO_FUSED_TAIL), and the forced launch forms in child interpreters.

Every case and every weighting also meets the active-list contract exactly (loss_spec.check_list).

Tolerances (loss_spec.per_ray_error, sums_bound, losses_bound, d_raw_slack).  d_raw per term, channel and ray, and the composite
outputs per ray: relative l2 against the twin within helpers.bound(o32, o64) of the case (4 x the fp32 reference's own distance from
fp64, floor 2e-5), rays below 1e-6 of the batch's largest compared at that scale.  Count slots exact; real slots within
(S + 8) 2^-24 sum |summands|; slot 9 is the minimum of the rendered map; losses within the sums' bound taken through the twin's
finalize.  On top of these, the first-order conditioning of the differences the formulas take (rgb - target, depth - td,
1 / 2u - mean_e / 2u^2, v_s - out of the weight normalisation, (z + sdf tr) - td; loss_spec._conditioning): a ray or a slot whose
value is what rounding leaves of such a difference is as far off in the fp32 reference itself -- without these terms the reference
misses its own bound (tests/test_loss_spec_host.py::test_the_fp32_reference_meets_the_bounds_it_sets).
NARUTO_LOSS_REPORT names a file that receives one line per comparison: case, quantity, bound, observed error, error / tolerance.

WORST: error / tolerance on MI355X, the worst case per quantity (0.56 at most: d_raw of the sdf term, training path).  Mutants, tried once
and not kept: a halved g_depth fails 42 of these tests, `<=` in depth_valid 10, and a forward ray_count without the `front` term the two
cases without samples around the measured depth (with the shipped 11 such samples the sdf band always reaches beyond the last front
sample, and no list length depends on that term)."""
import ctypes as C
import json

import pytest
import torch

import helpers as H
import launch_forms as LF
import loss_spec as L
from naruto_amd import synthetic as syn

pytestmark = pytest.mark.gpu

CFG = H.office_cfg(12)
WEIGHTINGS = dict({t: L.one_hot_weights(t) for t in L.TERMS}, reference=L.reference_weights(CFG))

# worst error / tolerance on MI355X over all cases of this file, per quantity (from the NARUTO_LOSS_REPORT file of a whole run)
WORST = {"modular": {"outputs": 0.240, "sums": 0.218, "losses": 0.206, "d_raw[rgb]": 0.138, "d_raw[depth]": 0.102, "d_raw[sdf]": 0.493, "d_raw[fs]": 0.015,
                     "d_raw[uncert]": 0.141, "d_raw[reference]": 0.137},
         "train": {"outputs": 0.017, "sums": 0.146, "losses": 0.184, "total": 0.125, "d_raw[rgb]": 0.073, "d_raw[depth]": 0.324, "d_raw[sdf]": 0.562, "d_raw[fs]": 0.008,
                   "d_raw[uncert]": 0.260, "d_raw[reference]": 0.166}}


def _fail(bad):
    assert not bad, f"{len(bad)} comparisons out of bounds:\n" + "\n".join(bad[:20])


@pytest.fixture(scope="module")
def field(gpu):
    return H.make_hip_from_oracle(CFG, H.make_oracle(CFG, 0.25, 3), gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# A. modular operators
# ---------------------------------------------------------------------------------------------------------------------------
def _modular(field, gpu, b, p, case, ordinary, lines):
    from naruto_amd import _lib, ops
    lib, h = _lib.load(), field._handle()
    N, S = b["z"].shape
    o = L.twin(b["raw"], b["z"], b["target_rgb"], b["target_d"], p, weightings=WEIGHTINGS)
    raw, z, tgt, td = (b[k].to(gpu).contiguous() for k in ("raw", "z", "target_rgb", "target_d"))
    bad = []
    # ops.composite: all seven outputs
    names = ("rgb", "disp", "acc", "weights", "depth", "depth_var", "uncert_map")
    comp = dict(zip(names, (t.cpu() for t in ops.composite(h, raw, z))))
    bad += L.check_outputs(case + " composite", comp, o, lines, keys=names)
    # ops.render_loss: outputs, losses, d_raw per weighting by autograd
    rg = raw.clone().requires_grad_(True)
    out = ops.render_loss(h, rg, z, tgt, td, p["depth_trunc"], p["rgb_missing"])
    rl = dict(zip(("rgb", "depth", "disp", "acc", "depth_var", "uncert_map"), (t.detach().cpu() for t in out[:6])))
    for k, v in rl.items():
        assert torch.equal(torch.nan_to_num(v), torch.nan_to_num(comp[k])) and L._nan_equal(v, comp[k]), f"{case}: render_loss.{k} is not composite's"
    losses = out[6]
    # the sums, through the C entry point
    st = torch.cuda.current_stream().cuda_stream
    sums = torch.zeros(_lib.LOSS_NSUMS, dtype=torch.float64, device=gpu)
    l2 = torch.zeros(8, device=gpu)
    ws = _lib.workspace(lib.naruto_loss_workspace(N), gpu)
    dev = {k: comp[k].to(gpu).contiguous() for k in ("rgb", "depth", "uncert_map")}
    _lib.check(lib.naruto_loss_sums(h.ptr, N, S, raw.data_ptr(), z.data_ptr(), dev["rgb"].data_ptr(), dev["depth"].data_ptr(),
                                    dev["uncert_map"].data_ptr(), tgt.data_ptr(), td.data_ptr(), p["depth_trunc"], p["rgb_missing"],
                                    sums.data_ptr(), l2.data_ptr(), ws.data_ptr(), st), "naruto_loss_sums")
    torch.cuda.synchronize()
    assert torch.equal(torch.nan_to_num(l2), torch.nan_to_num(losses.detach())) and L._nan_equal(l2.cpu(), losses.detach().cpu())
    bad += L.check_sums(case, sums.cpu(), comp["uncert_map"], o, lines)
    bad += L.check_losses(case, losses.detach().cpu(), sums.cpu(), o, lines)
    # naruto_loss_finalize on the same sums with another ray total: the twin's finalize
    lf = torch.zeros(8, device=gpu)
    _lib.check(lib.naruto_loss_finalize(sums.data_ptr(), N + 7, S, lf.data_ptr(), st), "naruto_loss_finalize")
    o7 = dict(o, n_rays_total=N + 7, losses=L.finalize(o["sums"], N + 7, S))
    bad += L.check_losses(case + " n_total+7", lf.cpu(), sums.cpu(), o7, lines)
    cnt, off = torch.zeros(N, dtype=torch.int32, device=gpu), torch.zeros(N, dtype=torch.int32, device=gpu)
    idx, n_act = torch.zeros(N * S, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    for name, w in WEIGHTINGS.items():
        rg.grad = None
        (losses * w[:8].to(gpu)).sum().backward(retain_graph=True)
        d_raw = rg.grad.detach().clone()
        bad += L.check_d_raw(case, d_raw.cpu(), o, name, lines, w)
        # the C entry point: the same bits, and the ray lists
        d2 = torch.full_like(raw, 7.0)
        lg = w[:6].to(gpu).contiguous()
        _lib.check(lib.naruto_loss_bwd(h.ptr, N, S, raw.data_ptr(), z.data_ptr(), tgt.data_ptr(), td.data_ptr(), p["depth_trunc"], p["rgb_missing"],
                                       sums.data_ptr(), N, lg.data_ptr(), d2.data_ptr(), cnt.data_ptr(), st), "naruto_loss_bwd")
        _lib.check(lib.naruto_compact_active(N, S, cnt.data_ptr(), off.data_ptr(), idx.data_ptr(), n_act.data_ptr(), st), "naruto_compact_active")
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(d2), torch.nan_to_num(d_raw)) and L._nan_equal(d2.cpu(), d_raw.cpu()), f"{case} {name}: naruto_loss_bwd"
        bad += L.check_list(f"{case} {name}", d2.cpu(), cnt.cpu(), off.cpu(), n_act.cpu(), idx.cpu(), o, ordinary, predicted=False)
    # naruto_composite_bwd(accumulate = 1) on top of naruto_loss_bwd (reference weights, still in d2): fl(prior + fresh), bit for bit
    g = torch.Generator().manual_seed(N * 1031 + S)
    d_rgb, d_depth = torch.randn(N, 3, generator=g).to(gpu), torch.randn(N, generator=g).to(gpu)
    fresh, acc = torch.empty_like(raw), d2.clone()
    for buf, flag in ((fresh, 0), (acc, 1)):
        _lib.check(lib.naruto_composite_bwd(h.ptr, N, S, raw.data_ptr(), z.data_ptr(), d_rgb.data_ptr(), None, None, None, d_depth.data_ptr(), None, None,
                                            buf.data_ptr(), flag, st), "naruto_composite_bwd")
    torch.cuda.synchronize()
    want = d2.cpu() + fresh.cpu()
    assert torch.equal(torch.nan_to_num(acc.cpu()), torch.nan_to_num(want)) and L._nan_equal(acc.cpu(), want), f"{case}: accumulate is not fl(prior + fresh)"
    assert float(fresh.abs().nan_to_num().max()) > 0
    return o, bad


MODULAR = [(1, 1), (3, 2), (257, 1), (1025, 2), (4, 64), (257, 64), (5, 65), (1025, 65), (4, 70), (257, 70), (1, 1024), (3, 1024), (5, 1024)]


@pytest.mark.parametrize("N,S", MODULAR, ids=[f"N{n}_S{s}" for n, s in MODULAR])
@pytest.mark.parametrize("rgb_missing", [0.05, 0.0])
def test_modular_operators_on_edge_rays(gpu, field, N, S, rgb_missing):
    p = L.params_of(CFG, rgb_missing)
    b, where = L.edge_batch(N, S, 1000 + 7 * N + S, p)
    case = f"modular N{N} S{S} missing{rgb_missing:g}"
    lines = []
    o, bad = _modular(field, gpu, b, p, case, ordinary=S >= 64, lines=lines)
    L.report(lines)
    if "product_is_a_denormal" in where:
        # the CPU reference calls the denormal product a sign change; so must the device (the twin's weights say where the limit fell)
        assert int(o["dec"]["first"][where["product_is_a_denormal"]]) == 5
    _fail(bad)


@pytest.mark.parametrize("kind", ["no_valid_depth", "no_samples"])
def test_modular_operators_on_degenerate_batches(gpu, field, kind):
    p = L.params_of(CFG)
    b = L.degenerate_batch(kind, 37, 70, 21, p)
    lines = []
    o, bad = _modular(field, gpu, b, p, f"modular {kind}", ordinary=False, lines=lines)
    L.report(lines)
    _fail(bad)
    nan = torch.isnan(o["losses"][:6]).tolist()
    assert nan == ([False, True, False, False, False, True] if kind == "no_valid_depth" else [False, True, True, True, False, True])


# ---------------------------------------------------------------------------------------------------------------------------
# B. the training path
# ---------------------------------------------------------------------------------------------------------------------------
ROUTES = ("deferred_tail", "forward_then_backward", "sums_given", "no_fused_tail")


def _train_setup(gpu, S, N, seed, nr=11):
    from naruto_amd import ops
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=S - nr, n_range_d=nr)
    tr, cam = cfg["training"], cfg["cam"]
    m = H.make_hip_from_oracle(cfg, H.make_oracle(cfg, 0.25, seed), gpu)
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=seed, zero_depth_frac=0.1)
    if not (rays["target_d"] > 0).any():
        rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=seed, zero_depth_frac=0.0)
    rand = torch.rand(N, S, generator=torch.Generator().manual_seed(seed)).to(gpu)
    args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + \
           [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]

    def step():
        return ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=S - nr, n_range_d=nr, near=cam["near"],
                             far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True,
                             loss_weights=WEIGHTINGS["reference"].to(gpu), device_rng=False)
    return cfg, m, rays, rand, args, step


def _snapshot(ts):
    torch.cuda.synchronize()
    return {k: getattr(ts, k).detach().cpu().clone() for k in ("raw", "z_vals", "rgb", "depth", "uncert_map", "sums", "losses", "d_raw", "ray_count",
                                                              "ray_offset", "n_active", "active_idx")}


def _run_route(ts, route, args, rand, w, second=None):
    """One iteration with the weights w by ``route``.  sums_given: the forward stops at its sums, the host adds ``second`` = (sums of a
    second batch, its ray count) and the backward runs with NARUTO_TRAIN_BWD_SUMS_GIVEN; returns this batch's own sums as well."""
    from naruto_amd import _lib, ops
    lib = _lib.load()
    ts.loss_weights.copy_(w.to(ts.loss_weights.device))
    own = None
    if route in ("deferred_tail", "no_fused_tail"):
        ts.run(*args, rand=rand)
    elif route == "forward_then_backward":
        ts.run_forward(*args, rand=rand)
        ts.run_backward()
    else:
        extra, n2 = second
        ts.run_forward(*args, rand=rand)                     # (sets the pointers and the jitter; run again below, stopping at the sums)
        ts.t.n_rays_total = ts.N + n2
        try:
            with ops._on_device(ts.device):
                st = ops._stream()
                _lib.check(lib.naruto_train_forward(ts.handle.ptr, C.byref(ts.ps), C.byref(ts.t), 0, st), "naruto_train_forward")
                torch.cuda.synchronize()
                own = ts.sums.detach().cpu().clone()
                both = own.clone()
                both[:9] += extra[:9]
                both[9] = torch.minimum(own[9], extra[9])
                ts.sums.copy_(both.to(ts.device))
                _lib.check(lib.naruto_train_backward(ts.handle.ptr, C.byref(ts.ps), C.byref(ts.t), C.byref(ts.gs), ts.flags | _lib.TRAIN_BWD_SUMS_GIVEN,
                                                     None, st), "naruto_train_backward")
                torch.cuda.synchronize()
        finally:
            ts.t.n_rays_total = ts.N
    got = _snapshot(ts)
    got["own_sums"] = own if own is not None else got["sums"]
    return got


def check_training_case(gpu, S, N, seed, routes=ROUTES, monkeypatch=None, lines=None, nr=11):
    """All weightings over ``routes`` for one shape; returns the out-of-bound lines.  The twin is evaluated once per case (the forward is
    deterministic: every run must leave the same raw and z_vals, which is asserted) and once more for the union with the second batch."""
    cfg, m, rays, rand, args, step = _train_setup(gpu, S, N, seed, nr)
    p = L.params_of(cfg)
    lines = [] if lines is None else lines
    bad = []
    ts = step()
    o = o_union = first = None
    N2 = 37
    b2 = L.ordinary_batch(N2, S, seed + 1)
    o2 = L.evaluate(b2["raw"], b2["z"], b2["target_rgb"], b2["target_d"], p, torch.float64)
    bits = {}
    for route in routes:
        if route == "no_fused_tail":
            monkeypatch.setenv("NARUTO_DEBUG_NO_FUSED_TAIL", "1")
            ts = step()
            assert not ts.fuse_tail
        for name, w in WEIGHTINGS.items():
            case = f"train S{S - nr}+{nr} N{N} {route} {name}"
            got = _run_route(ts, route, args, rand, w, second=(o2["own_sums"], N2))
            if first is None:
                first = got
                tw = dict(raw=got["raw"], z=got["z_vals"], target_rgb=torch.from_numpy(rays["target_rgb"]), target_d=torch.from_numpy(rays["target_d"]))
                o = L.twin(tw["raw"], tw["z"], tw["target_rgb"], tw["target_d"], p, weightings=WEIGHTINGS)
                o_union = L.twin(tw["raw"], tw["z"], tw["target_rgb"], tw["target_d"], p, weightings=WEIGHTINGS, n_rays_total=N + N2,
                                 extra_sums=o2["own_sums"])
            assert torch.equal(got["raw"], first["raw"]) and torch.equal(got["z_vals"], first["z_vals"]), f"{case}: the forward is not deterministic"
            ref = o_union if route == "sums_given" else o
            if name == "reference" or route == "deferred_tail":
                bad += L.check_outputs(case, got, ref, lines)
                bad += L.check_sums(case, got["own_sums"], got["uncert_map"], ref, lines)
                bad += L.check_losses(case, got["losses"], got["sums"], ref, lines, weights=w)
            bad += L.check_d_raw(case, got["d_raw"], ref, name, lines, w)
            bad += L.check_list(case, got["d_raw"], got["ray_count"], got["ray_offset"], got["n_active"], got["active_idx"], ref, ordinary=True,
                                predicted=route in ("deferred_tail", "sums_given") and N <= 4096)
            if route != "sums_given":
                # the three single-process routes: the same d_raw and losses bit for bit
                key = bits.setdefault(name, (got["d_raw"], got["losses"], route))
                assert torch.equal(got["d_raw"], key[0]) and torch.equal(got["losses"], key[1]), f"{case}: not the bits of route {key[2]}"
    if nr == 0:
        # without samples placed around the measured depth the sdf band is empty on most rays, and the forward's list length is decided
        # by the LAST FRONT sample wherever the rendering weights end before it: the case that needs `front` in the prediction
        last = lambda mask: torch.where(mask.any(1), S - torch.argmax(mask.flip(1).to(torch.int8), dim=1), torch.zeros(N, dtype=torch.long))
        decisive = last(o["dec"]["front"]) > torch.maximum(last(o["dec"]["sm"]), last(o["o32"]["weights"] != 0))
        assert int(decisive.sum()) * 10 >= N, f"the front mask decides the list length on {int(decisive.sum())} of {N} rays only"
    return bad, ts, m


# (S, N, n_range_d): the shipped 11 samples around the measured depth; 0: uniform samples only (the front mask decides the lists)
TRAIN = [(S, N, 11) for S in (27, 43, 64, 70, 128) for N in (1, 5, 515)] + [(27, 4096, 11), (27, 4097, 11), (16, 515, 0), (9, 515, 0)]


@pytest.mark.parametrize("S,N,nr", TRAIN, ids=[f"S{s - r}+{r}_N{n}" for s, n, r in TRAIN])
def test_training_path_against_the_twin(gpu, monkeypatch, S, N, nr):
    lines = []
    bad, ts, m = check_training_case(gpu, S, N, 4000 + 13 * S + N + nr, monkeypatch=monkeypatch, lines=lines, nr=nr)
    L.report(lines)
    _fail(bad)


_FORM_CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import launch_forms as LF, loss_spec as L
import test_gpu_loss as T
S, N, seed, out = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
lines = []
bad, ts, m = T.check_training_case(torch.device("cuda", 0), S, N, seed, routes=("deferred_tail",), lines=lines)
L.report(lines)
json.dump({"plan": LF.train_plan(m._handle().ptr, ts.t), "bad": bad}, open(out, "w"))
"""


@pytest.mark.parametrize("env", ["unfused", "partial", "packed", "sorted"])
def test_forced_forms_against_the_twin(gpu, tmp_path, env):
    S, N = 43, 515
    script = tmp_path / "child.py"
    script.write_text(_FORM_CHILD)
    out = tmp_path / f"{env}.json"
    LF.run_child(script, [S, N, 4900, out], LF.TRAIN_ENVS[env], timeout=300)
    r = json.load(open(out))
    want = LF.expected_train(env, S, LF.static_lds("k_query_fwd_loss_packed<false,8>"))
    assert (r["plan"][0], bool(r["plan"][1])) == want, f"{env}: the plan says {r['plan']}, the test claims {want}"
    _fail(r["bad"])

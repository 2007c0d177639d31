"""The loss stage's twin (tests/loss_spec.py) against the reference it restates -- oracle/spec_torch.py's raw2outputs, render_losses and
total_loss with autograd -- on the CPU: agreement in fp64 to 1e-12, the sums' finalize, two batches added as two ranks add them, the
fp32 reference's discrete decisions on the edge rays and its NaN patterns on the degenerate batches."""
import contextlib

import pytest
import torch

from oracle import spec_torch as S

import helpers as H
import loss_spec as L

CFG = H.office_cfg(12)
P = L.params_of(CFG)
NAMES = ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "uncert_loss")
WEIGHTINGS = dict({t: L.one_hot_weights(t) for t in L.TERMS}, reference=L.reference_weights(CFG))


@contextlib.contextmanager
def _default_dtype(dtype):
    # get_masks divides two integer counts: the quotient takes torch's DEFAULT dtype whatever the inputs' is
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _reference(b, p, dtype, weightings):
    """S.raw2outputs | S.render_losses | S.total_loss in ``dtype``; d_raw per weighting by autograd.  A NaN depth is replaced by 0
    first (the documented deviation)."""
    with _default_dtype(dtype):
        raw = b["raw"].to(dtype).requires_grad_(True)
        z = b["z"].to(dtype)
        td = L.measured_depth(b["target_d"]).to(dtype)[:, None]
        rgb, disp, acc, weights, depth, depth_var, um = S.raw2outputs(raw, z, p["trunc"], p["sc_factor"])
        rend = {"rgb": rgb, "depth": depth, "z_vals": z, "raw": raw, "uncert_map": um}
        ret = S.render_losses(rend, b["target_rgb"].to(dtype), td, p["depth_trunc"], p["rgb_missing"], p["trunc"], p["sc_factor"])
        d_raw = {}
        for name, w in weightings.items():
            tr = {"rgb_weight": float(w[0]), "depth_weight": float(w[1]), "sdf_weight": float(w[2]), "fs_weight": float(w[3]),
                  "uncert_weight": float(w[5])}
            d_raw[name] = torch.autograd.grad(S.total_loss(ret, tr), raw, retain_graph=True)[0]
    out = dict(rgb=rgb, depth=depth, acc=acc, weights=weights, depth_var=depth_var, disp=disp, uncert_map=um)
    return {k: v.detach() for k, v in out.items()}, torch.stack([ret[k].detach().reshape(()) for k in NAMES]), d_raw


def _close(a, b, tol, what):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaN pattern"
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    assert err <= tol, f"{what}: {err:.3e} of the largest entry"


@pytest.mark.parametrize("N,S", [(37, 70), (5, 2)])
def test_twin_is_the_reference_in_fp64(N, S):
    b = L.ordinary_batch(N, S, 11)
    o = L.evaluate(b["raw"], b["z"], b["target_rgb"], b["target_d"], P, torch.float64, weightings=WEIGHTINGS)
    # no decision of this batch sits where fp64 would take it differently from fp32
    dec64 = dict(front=b["z"].double() < (b["target_d"].double()[:, None] - P["trunc"]), sm=None)
    assert torch.equal(dec64["front"], o["dec"]["front"])
    out, losses, d_raw = _reference(b, P, torch.float64, WEIGHTINGS)
    for k, v in out.items():
        _close(o[k], v, 1e-12, k)
    _close(o["losses"][:6], losses, 1e-12, "losses")
    for k in WEIGHTINGS:
        _close(o["d_raw"][k], d_raw[k], 1e-12, f"d_raw[{k}]")
    if N == 37:
        dep = float(o["d_raw"]["depth"][..., 3].abs().max()) * 0.1 / float(o["d_raw"]["reference"][..., 3].abs().max())
        assert dep < 1e-2, "the depth term is a small part of the weighted total's sdf cotangent: why it needs a check of its own"


def test_finalize_reproduces_the_losses():
    b = L.ordinary_batch(37, 70, 12)
    o = L.evaluate(b["raw"], b["z"], b["target_rgb"], b["target_d"], P, torch.float64)
    _, losses, _ = _reference(b, P, torch.float64, {})
    _close(L.finalize(o["sums"], 37, 70)[:6], losses, 1e-12, "finalize(sums)")
    per_ray = torch.cat([o["terms"].sum(0), o["uncert_map"].min().reshape(1)])
    _close(L.finalize(per_ray, 37, 70)[:8], o["losses"][:8], 0.0, "finalize(sum of the per-ray terms)")
    assert float(o["losses"][7]) == float(o["dec"]["valid"].sum()) and float(o["losses"][6]) == float(o["uncert_map"].min())


def test_two_batches_add_like_two_ranks():
    b1, b2 = L.ordinary_batch(37, 43, 13), L.ordinary_batch(21, 43, 14)
    both = {k: torch.cat([b1[k], b2[k]]) for k in b1}
    o2 = L.evaluate(b2["raw"], b2["z"], b2["target_rgb"], b2["target_d"], P, torch.float64)
    o1 = L.evaluate(b1["raw"], b1["z"], b1["target_rgb"], b1["target_d"], P, torch.float64, n_rays_total=58, extra_sums=o2["own_sums"],
                    weightings=WEIGHTINGS)
    oc = L.evaluate(both["raw"], both["z"], both["target_rgb"], both["target_d"], P, torch.float64, weightings=WEIGHTINGS)
    _close(o1["sums"][:10], oc["sums"][:10], 1e-12, "sums")
    _close(o1["losses"], oc["losses"], 1e-12, "losses")
    for k in WEIGHTINGS:
        _close(o1["d_raw"][k], oc["d_raw"][k][:37], 1e-12, f"d_raw[{k}] of the first batch's rows")
    alone = L.evaluate(b1["raw"], b1["z"], b1["target_rgb"], b1["target_d"], P, torch.float64)
    assert float((alone["d_raw"]["sdf"] - o1["d_raw"]["sdf"]).abs().max()) > 0.0        # the second batch does change the first's cotangents


@pytest.mark.parametrize("rgb_missing", [0.05, 0.0])
def test_fp32_twin_takes_the_reference_decisions_on_the_edge_rays(rgb_missing):
    p = dict(P, rgb_missing=rgb_missing)
    b, where = L.edge_batch(257, 70, 15, p)
    assert len(where) == len(L.edge_rays(70, p)) == 21
    o = L.twin(b["raw"], b["z"], b["target_rgb"], b["target_d"], p, weightings=WEIGHTINGS)
    out, losses, d_raw = _reference(b, p, torch.float32, WEIGHTINGS)
    assert torch.equal(out["weights"] != 0, o["o32"]["weights"] != 0), "the z < limit mask"
    first = o["dec"]["first"]
    assert int(first[where["change_at_0"]]) == 0 and int(first[where["change_at_62"]]) == 62 and int(first[where["change_at_68"]]) == 68
    assert int(first[where["two_changes_first_wins"]]) == 3
    for k in ("no_change", "zero_next_to_negative", "product_underflows_to_minus_zero"):
        assert not bool(o["dec"]["any_change"][where[k]]), k
    assert int(first[where["product_is_a_denormal"]]) == 5, "the CPU reference keeps denormals: -1e-40 < 0"
    n = where["z_on_the_band_edges"]
    assert int(o["dec"]["front"][n].sum()) >= 1 and int(o["dec"]["back"][n].sum()) >= 1
    for k in ("sdf_over_trunc_plus_200", "sdf_over_trunc_minus_200"):
        assert float(o["o32"]["weights"][where[k]].abs().max()) == 0.0 and bool(torch.isnan(o["o32"]["disp"][where[k]]))
    valid = o["dec"]["valid"]
    assert [bool(valid[where[k]]) for k in ("td_0", "td_minus_1", "td_nan", "td_depth_trunc", "td_below_depth_trunc", "td_150")] == \
        [False, False, False, False, True, False]
    for k, v in out.items():
        _close(o["o32"][k], v, 1e-5, k)
    _close(o["o32"]["losses"][:6], losses, 1e-5, "losses")
    for k in WEIGHTINGS:
        assert H.rel(o["o32"]["d_raw"][k], o["d_raw"][k]) < 1e-3 and H.rel(d_raw[k], o["d_raw"][k]) < 1e-3, k


@pytest.mark.parametrize("kind", ["no_valid_depth", "no_samples"])
def test_nan_patterns_of_the_degenerate_batches(kind):
    b = L.degenerate_batch(kind, 37, 70, 16, P)
    o = L.twin(b["raw"], b["z"], b["target_rgb"], b["target_d"], P, weightings=WEIGHTINGS)
    out, losses, d_raw = _reference(b, P, torch.float32, WEIGHTINGS)
    for ev in (o, o["o32"]):
        assert torch.equal(torch.isnan(ev["losses"][:6]), torch.isnan(losses))
        for k in WEIGHTINGS:
            assert torch.equal(torch.isnan(ev["d_raw"][k]), torch.isnan(d_raw[k])), f"{kind}: d_raw[{k}]"
    nan = [bool(x) for x in torch.isnan(o["losses"][:6])]
    if kind == "no_valid_depth":
        assert nan == [False, True, False, False, False, True]
        assert bool(torch.isfinite(o["d_raw"]["reference"]).all()) and bool(torch.isfinite(o["totals"]["rgb"]))
    else:
        assert nan == [False, True, True, True, False, True]
        assert bool(torch.isnan(o["d_raw"]["rgb"][..., 3]).all()) and bool(torch.isfinite(o["d_raw"]["rgb"][..., :3]).all())


SHAPES = [(1, 1), (3, 2), (257, 1), (1025, 2), (5, 65), (257, 70), (3, 1024), (515, 43)]


@pytest.mark.parametrize("N,S", SHAPES)
def test_the_fp32_reference_meets_the_bounds_it_sets(N, S):
    """The comparisons the device results go through (loss_spec.check_*), applied to the fp32 reference itself on the edge batches:
    a bound that a correctly rounded fp32 evaluation of the reference formulas cannot meet would say nothing about a kernel.  This
    is what the conditioning terms are for: without them the reference misses the sums' bound at S <= 2 (slot 5: 1.5 x) and on
    single-ray batches (slot 1: 1.1 x), and the per-ray measure on every ray whose rendered depth lands within rounding of the measured one."""
    b, _ = L.edge_batch(N, S, 1000 + 7 * N + S, P)
    o = L.twin(b["raw"], b["z"], b["target_rgb"], b["target_d"], P, weightings=WEIGHTINGS)
    r = o["o32"]
    lines = []
    bad = L.check_outputs("ref", r, o, lines, keys=("rgb", "disp", "acc", "weights", "depth", "depth_var", "uncert_map"))
    bad += L.check_sums("ref", r["own_sums"], r["uncert_map"], o, lines)
    bad += L.check_losses("ref", r["losses"], r["sums"], o, lines)
    for k, w in WEIGHTINGS.items():
        bad += L.check_d_raw("ref", r["d_raw"][k], o, k, lines, w)
    assert not bad, "\n".join(bad)


def test_a_halved_depth_cotangent_is_seen_only_term_by_term():
    """The gap this closes: with the reference weights the depth term is 1e-4 of the sdf channel, so a depth cotangent wrong by a
    factor of two stays inside any bound on the weighted total -- and outside the one on the depth term alone."""
    b, _ = L.edge_batch(257, 70, 17, P)
    o = L.twin(b["raw"], b["z"], b["target_rgb"], b["target_d"], P, weightings=WEIGHTINGS)
    r = o["o32"]
    wrong = r["d_raw"]["reference"] - 0.5 * float(WEIGHTINGS["reference"][1]) * r["d_raw"]["depth"]
    assert H.rel(wrong, o["d_raw"]["reference"]) < 1e-3
    assert L.check_d_raw("halved", 0.5 * r["d_raw"]["depth"], o, "depth", [], WEIGHTINGS["depth"])
    assert not L.check_d_raw("exact", r["d_raw"]["depth"], o, "depth", [], WEIGHTINGS["depth"])


def test_list_contract_sees_a_count_one_too_short():
    b = L.ordinary_batch(37, 70, 18)
    o = L.twin(b["raw"], b["z"], b["target_rgb"], b["target_d"], P, weightings=WEIGHTINGS)
    d = o["o32"]["d_raw"]["reference"]
    cnt = ((d != 0).any(-1) * torch.arange(1, 71)[None, :]).max(1).values
    off = torch.cumsum(cnt, 0) - cnt
    idx = torch.cat([n * 70 + torch.arange(int(c)) for n, c in enumerate(cnt.tolist())])
    assert not L.check_list("exact", d, cnt, off, cnt.sum().reshape(1), idx, o, True, True)
    assert int((cnt < 70).sum()) >= 19
    short = cnt.clone()
    short[5] -= 1
    assert L.check_list("short", d, short, off, cnt.sum().reshape(1), idx, o, True, True)

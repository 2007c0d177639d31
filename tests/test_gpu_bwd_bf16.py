"""The bf16 MLP backward (k_query_bwd_bf) and forward (k_query_fwd_bf) at tile edges, on lists and on dense OneBlob steps.

Against the torch restatement a bf16 rounding flip moves an entry by up to a bf16 ulp of one term, so at a few points no per-entry tolerance
holds.  What these tests state instead: ONE POINT'S CONTRIBUTION DOES NOT DEPEND ON WHERE THE POINT SITS.  Its forward row, its feature
cotangents and its addends to the six gradients come from its own column of each matrix product; bf16 rounding is applied per point, before any
sum over points, and the product of two bf16 numbers is exact in fp32.  Position changes only the order of the fp32 additions over points and
whether the point's 64-entry step takes the closed or the dense OneBlob form (dense when any of the step's 64 entries -- the padding lanes
repeat the list's last one -- has a normalised coordinate outside (-0.93, 1.93)).  So
  1. single points are pinned to the restatement (tests/bf16_twin.py), where a flip can be seen and counted point by point, in both flavours:
     "closed" is the point alone (M = 1), "dense" the point followed by a far point with an all-zero cotangent (M = 2; the far point adds exact
     zeros everywhere);
  2. every batch shape is pinned to the sum of the kernel's own single-point results of the predicted flavours: forward rows bit for bit,
     gradients within M 2^-23 sum |G_i| + 1e-9 max |sum G_i| (bf16_twin.composition_bound) -- no flip can occur there;
  3. the uncertainty grid too large for the scatter (float atomics in the kernel), both MLP modes;
  4. the backward on the weight images k_loss_bwd_fused prepared against the one that stages the weights itself.
Harness of test_gpu_bwd_oneblob.py: H.office_cfg(12), H.make_oracle(cfg, 0.25, 21), one module-scoped field; the singles are cached."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import bf16_twin as T
import helpers as H
import launch_forms as LF
from test_gpu_bwd_tiles import _nonzero_where_the_reference_is

pytestmark = pytest.mark.gpu


class Field:
    """The bf16 field, the oracle it was made from, the point sets and the cache of single-point results."""

    def __init__(self, gpu, n_in=257, uncert_voxel=0.1, mode="bf16"):
        cfg = H.office_cfg(12)
        self.ora = H.make_oracle(cfg, 0.25, 21, uncert_voxel=uncert_voxel)
        cfg_m = H.office_cfg(12)
        cfg_m["decoder"]["mlp_precision"] = mode
        self.m = H.make_hip_from_oracle(cfg_m, self.ora, gpu, uncert_voxel=uncert_voxel)
        assert self.m._handle().mlp_mode == mode
        self.gpu = gpu
        self.pts = T.Points(self.ora, n_in=n_in)
        self.singles = {}

    def params(self):
        p = self.m._params()
        return {k: p[k] for k in T.NAMES}

    def run(self, x, cot, route):
        """One autograd call -> (forward outputs, the six gradients), detached copies on the device."""
        params = self.params()
        for t in params.values():
            t.grad = None
        xg = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.gpu)
        if route == "raw":
            raw = self.m.query_color_sdf(xg)
            fwd = {"raw": raw}
            (raw * torch.from_numpy(cot["raw"]).to(self.gpu)).sum().backward()
        else:
            su, geo = self.m.query_sdf(xg, return_geo=True, return_uncert=True)
            fwd = {"su": su, "geo": geo}
            ((su * torch.from_numpy(cot["su"]).to(self.gpu)).sum() + (geo * torch.from_numpy(cot["geo"]).to(self.gpu)).sum()).backward()
        torch.cuda.synchronize()
        return ({k: v.detach().clone() for k, v in fwd.items()},
                {k: (torch.zeros_like(t) if t.grad is None else t.grad.detach().clone()) for k, t in params.items()})

    def single(self, flavour, route, i):
        """Point i of the pool on its own in the given flavour: (forward row(s) [1, .], gradients).  A far point is dense whatever it is asked for."""
        far = i >= self.pts.n_in
        key = ("dense" if far else flavour, route, i)
        if key not in self.singles:
            x, cot = self.pts.x[i:i + 1], self.pts.cot_of([i], route)
            if key[0] == "dense" and not far:
                x = np.concatenate([x, self.pts.companion])
                cot = {k: np.concatenate([v, np.zeros_like(v)]) for k, v in cot.items()}
            fwd, grads = self.run(x, cot, route)
            self.singles[key] = ({k: v[:1] for k, v in fwd.items()}, grads)
        return self.singles[key]

    def sum_of_singles(self, flavours, route, idx):
        """fp64 sums over the listed points of G_i and of |G_i|, and the stacked forward rows."""
        tot, tot_abs, rows = None, None, {}
        for fl, i in zip(flavours, idx):
            fwd, g = self.single(fl, route, int(i))
            if tot is None:
                tot = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in g.items()}
                tot_abs = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in g.items()}
            for k, v in g.items():
                tot[k] += v.double()
                tot_abs[k] += v.double().abs()
            for k, v in fwd.items():
                rows.setdefault(k, []).append(v)
        return tot, tot_abs, {k: torch.cat(v) for k, v in rows.items()}


@pytest.fixture(scope="module")
def field(gpu):
    return Field(gpu)


def _bound_ratio(got, tot, tot_abs, n_points, what):
    """Worst |got - sum G_i| / bound over the six gradients (asserted <= 1), and the non-zero rules of test_gpu_bwd_tiles against the sum."""
    worst = {}
    for k in T.NAMES:
        err = (got[k].double() - tot[k]).abs()
        bound = T.composition_bound(n_points, tot_abs[k], tot[k])
        r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        worst[k] = float(r.max())
    print(f"{what}: worst error / bound {worst}")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what}: gradients outside M 2^-23 sum |G_i| + 1e-9 max |sum G_i| of the sum of the singles: error / bound {bad}"
    ref = {k: (tot[k].float().cpu() if float(tot[k].abs().max()) > 0.0 else None) for k in T.NAMES}
    _nonzero_where_the_reference_is({k: got[k].cpu() for k in T.NAMES}, ref, what)
    return worst


def _rows_equal(got, want, what):
    for k in want:
        same = (got[k] == want[k]).reshape(got[k].shape[0], -1).all(1)
        assert bool(same.all()), f"{what}: forward rows of {k} differ from the singles' at entries {torch.nonzero(~same).reshape(-1)[:8].tolist()} ({int((~same).sum())} in all)"
        assert float(want[k].abs().max()) > 0.0, k


def _check_batch(field, idx, route, what):
    """The pool's points idx as one batch through autograd against the singles of the predicted flavours."""
    idx = [int(i) for i in idx]
    x = field.pts.x[idx]
    flavours = T.step_flavours(x)
    fwd, grads = field.run(x, field.pts.cot_of(idx, route), route)
    tot, tot_abs, rows = field.sum_of_singles(flavours, route, idx)
    _rows_equal(fwd, rows, what)
    _bound_ratio(grads, tot, tot_abs, len(idx), what)
    return flavours, fwd, grads, (tot, tot_abs)


# --------------------------------------------------------------------------------------------- 1. anchor: single points against the restatement
@pytest.fixture(scope="module")
def restated(field):
    """The restatement of every anchor on its own, by both routes: {(route, i): (forward, gradients)}, computed once."""
    return {(route, i): T.restate(field.ora, field.pts.x[i:i + 1], field.pts.cot_of([i], route), route) for route in T.ROUTES for i in field.pts.anchor_idx}


@pytest.mark.parametrize("route", T.ROUTES)
@pytest.mark.parametrize("flavour", ["closed", "dense"])
def test_single_points_match_the_restatement(field, restated, flavour, route):
    """96 filtered points (64 inside the box with every coordinate in centre bins 0 and 15 and eight points on bin edges, 24 outside the box, 8
    far ones), each alone (closed: the 8 far ones are dense by themselves) and each of the 88 in-range ones again with a far companion of zero
    cotangent (dense).  Per point and tensor, scale = max |want|: tight = forward within 2e-5 + 1e-5 |want|, gradients within 2e-5 scale.  At
    least 90 % of the points are tight in every tensor, every point is within 2^-6 scale; the channels that do not pass through the MLPs (the
    uncertainty sample, the uncertainty grid's gradient) get no flip allowance.

    Measured on MI355X: no point that is not tight, in either flavour by either route (0 of 96 closed, 0 of 88 dense).  Worst error / scale per
    tensor over all four runs: raw 5.7e-7, (sdf, uncertainty) 1.6e-7, geo 7.3e-8, sdf_w0 2.4e-6 (dense; 6.7e-7 closed), sdf_w1 0, col_w0 2.4e-6
    (dense; 6.7e-7 closed), col_w1 0, uncert_grid 1.3e-6, table 2.0e-7.  (Before the padding lanes' geo cotangent was masked, the closed geo
    singles came out with sdf_w1 at 64 times the restatement's: error / scale 63.)"""
    idx = list(range(T.N_ANCHOR_IN_RANGE)) + (field.pts.far_idx if flavour == "closed" else [])
    not_tight, worst, over_cap = [], {}, []
    for i in idx:
        fwd, grads = field.single(flavour, route, i)
        want_f, want_g = restated[(route, i)]
        tight = True
        for k in want_f:
            u = T.FWD_UNCERT[k] if k in T.FWD_UNCERT else None
            if u is not None:                  # the uncertainty sample: always tight
                t, _, _ = T.point_errors(fwd[k][:, u], want_f[k][:, u], forward=True)
                assert t, f"point {i}: the uncertainty channel of {k} is {float(fwd[k][0, u])!r}, wanted {float(want_f[k][0, u])!r}"
            t, r, scale = T.point_errors(fwd[k], want_f[k], forward=True)
            assert float(fwd[k].abs().max()) > 0.0 or scale == 0.0, (i, k)
            tight, worst[k] = tight and t, max(worst.get(k, 0.0), r)
            if r > T.CAP and not t:
                over_cap.append((i, k, r))
        got = {k: grads[k].cpu() for k in T.NAMES}
        _nonzero_where_the_reference_is(got, want_g, f"point {i} ({flavour}, {route})")
        for k in T.NAMES:
            if want_g[k] is None:
                continue
            t, r, _ = T.point_errors(got[k], want_g[k], forward=False)
            if k == "uncert_grid":             # no MLP on the way: no flip allowance
                H.grad_close(got[k], want_g[k], f"point {i} ({flavour}, {route}).grad.uncert_grid")
                assert t, f"point {i}: uncert_grid gradient error / scale {r:.3e}"
            tight, worst[k] = tight and t, max(worst.get(k, 0.0), r)
            if r > T.CAP:
                over_cap.append((i, k, r))
        if not tight:
            not_tight.append(i)
    print(f"{flavour}, {route}: {len(not_tight)} of {len(idx)} points not tight {not_tight}; worst error / scale {worst}")
    assert not over_cap, f"{flavour}, {route}: beyond 2^-6 of the scale (point, tensor, error / scale): {over_cap[:8]}"
    assert len(idx) - len(not_tight) >= 0.9 * len(idx), f"{flavour}, {route}: {len(not_tight)} of {len(idx)} points are not tight: {not_tight}"


# --------------------------------------------------------------------------------------------- 2. composition: batches against the sum of singles
# a. all closed form.  32 / 33 cross the half A | half B boundary, 64 / 65 a wave's step, 256 / 257 a workgroup
@pytest.mark.parametrize("n_pts,route", [(n, "raw") for n in (2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)] + [(n, "geo") for n in (32, 33, 65, 257)])
def test_batches_are_sums_of_singles(field, n_pts, route):
    flavours, _, _, _ = _check_batch(field, range(n_pts), route, f"{n_pts} points, {route}")
    assert set(flavours) == {"closed"}


def _dense_case(field, name):
    far = field.pts.far_idx[0]
    if name == "far_first":          # step 0 dense, step 1 (one entry) closed
        return [far] + list(range(64)), ["dense"] * 64 + ["closed"]
    if name == "far_last_alone":     # step 0 closed; the far point alone in step 1, its padding lanes repeat it
        return list(range(64)) + [far], ["closed"] * 64 + ["dense"]
    return list(range(70)) + [far] + list(range(70, 128)), ["closed"] * 64 + ["dense"] * 64 + ["closed"]          # only the middle step dense


# b. dense steps
@pytest.mark.parametrize("route", T.ROUTES)
@pytest.mark.parametrize("name", ["far_first", "far_last_alone", "far_at_70_of_129"])
def test_dense_steps_are_sums_of_singles(field, name, route):
    """A far point sends its own 64-entry step, and no other, to the dense form.  Where the two forms give a point other bits, the prediction of
    the wrong form fails: their OneBlob values are ~1e-6 apart BEFORE the rounding to bf16, so most points agree -- measured, 12 of the 63
    in-range points of a dense step (far point first) and 3 of 63 (far point at entry 70) by the raw route, none by the geo route."""
    idx, expect = _dense_case(field, name)
    flavours, fwd, _, _ = _check_batch(field, idx, route, f"{name}, {route}")
    assert flavours == expect
    dense_in_range = [(pos, i) for pos, (i, fl) in enumerate(zip(idx, flavours)) if fl == "dense" and i < field.pts.n_in]
    out = "raw" if route == "raw" else "geo"
    differ = [(pos, i) for pos, i in dense_in_range if not torch.equal(field.single("dense", route, i)[0][out], field.single("closed", route, i)[0][out])]
    print(f"{name}, {route}: {len(differ)} of {len(dense_in_range)} in-range points of the dense step have other forward bits in the closed form")
    for pos, i in differ:
        assert not torch.equal(fwd[out][pos:pos + 1], field.single("closed", route, i)[0][out]), (pos, i)


# c. position
@pytest.mark.parametrize("route", T.ROUTES)
def test_position_in_the_batch(field, route):
    base = list(range(65))
    perm = [int(i) for i in np.random.RandomState(31).permutation(65)]
    runs = {}
    for name, order in (("in order", base), ("reversed", base[::-1]), ("permuted", perm)):
        _, fwd, grads, sums = _check_batch(field, order, route, f"65 points {name}, {route}")
        inv = torch.from_numpy(np.argsort(np.asarray(order))).to(field.gpu)
        runs[name] = ({k: v[inv] for k, v in fwd.items()}, grads)
    tot, tot_abs = sums
    for name in ("reversed", "permuted"):
        for k, v in runs["in order"][0].items():
            assert torch.equal(runs[name][0][k], v), f"{name}: forward rows of {k} change with the position"
        for k in T.NAMES:
            err = (runs[name][1][k].double() - runs["in order"][1][k].double()).abs()
            assert bool((err <= T.composition_bound(65, tot_abs[k], tot[k])).all()), f"{name}: gradient {k} moves by more than the bound with the position"


# d. lists, through the C entry point
def _c_entry(field, x, d_raw, d_geo, active, color):
    """naruto_query_fwd with feat_save, then naruto_query_bwd on the list ``active`` (or on all points: None) -> (forward outputs, gradients)."""
    from naruto_amd import _lib, ops
    lib = _lib.load()
    gpu, h = field.gpu, field.m._handle()
    params = {k: v.detach() for k, v in field.m._params().items()}
    M = x.shape[0]
    xg = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)
    ps = ops._params_struct(params)
    pts, _ = ops._points_struct(xg, None, None, None)
    out = torch.empty(M, 5 if color else 2, device=gpu)
    geo = None if color else torch.empty(M, 15, device=gpu)
    feat = torch.empty(16, M, 2, device=gpu)
    ops.check(lib.naruto_query_fwd(h.ptr, C.byref(ps), M, C.byref(pts), ops._p(out) if color else None, None if color else ops._p(out), ops._p(geo),
                                   ops._p(feat), ops._stream()), "naruto_query_fwd")
    grads = {k: torch.zeros_like(params[k]) for k in T.NAMES}
    gs = _lib.NarutoGrads()
    for k in T.NAMES:
        setattr(gs, k, ops._p(grads[k]))
    ws = _lib.workspace(lib.naruto_query_bwd_workspace(h.ptr, M), gpu)
    lst = n_act = None
    if active is not None:
        assert 1 <= len(active) <= M and 0 <= min(active) and max(active) < M
        rest = [i for i in range(M) if i not in set(active)]                 # beyond n_active: never read -- and if read, points with a cotangent of 1e6
        lst = torch.tensor(list(active) + rest, dtype=torch.int32, device=gpu)
        assert lst.numel() == M or len(set(active)) < len(active)
        n_act = torch.tensor([len(active)], dtype=torch.int32, device=gpu)
    dr = torch.from_numpy(d_raw).to(gpu).contiguous()
    dg = None if d_geo is None else torch.from_numpy(d_geo).to(gpu).contiguous()
    ops.check(lib.naruto_query_bwd(h.ptr, C.byref(ps), M, C.byref(pts), ops._p(feat), ops._p(dr), ops._p(dg), ops._p(lst), ops._p(n_act), None, 0,
                                   C.byref(gs), ops._p(ws), ops._stream()), "naruto_query_bwd")
    torch.cuda.synchronize()
    return ({"raw": out} if color else {"su": out, "geo": geo}), grads


def _list_cotangents(field, idx, route, listed):
    """d_raw [M,5] (and d_geo [M,15]) of the pool's points idx as the autograd routes hand them to the kernel; rows that are not listed hold 1e6."""
    cot = field.pts.cot_of(idx, route)
    M = len(idx)
    if route == "raw":
        d_raw, d_geo = cot["raw"].copy(), None
    else:
        d_raw = np.zeros((M, 5), dtype=np.float32)
        d_raw[:, 3:5] = cot["su"]
        d_geo = cot["geo"].copy()
    off = np.ones(M, dtype=bool)
    off[list(listed)] = False
    d_raw[off] = 1e6
    if d_geo is not None:
        d_geo[off] = 1e6
    return d_raw, d_geo


_LISTS = {"first_1": list(range(1)), "first_63": list(range(63)), "first_64": list(range(64)), "first_65": list(range(65)),
          "permutation": [int(i) for i in np.random.RandomState(32).permutation(200)], "every_third": list(range(0, 200, 3))}


@pytest.mark.parametrize("route", T.ROUTES)
@pytest.mark.parametrize("name", list(_LISTS))
def test_active_lists_are_sums_of_their_singles(field, name, route):
    idx, active = list(range(200)), _LISTS[name]
    x = field.pts.x[idx]
    d_raw, d_geo = _list_cotangents(field, idx, route, active)
    fwd, grads = _c_entry(field, x, d_raw, d_geo, active, color=route == "raw")
    # the forward knows no list: all 200 points, all in range
    _, _, rows = field.sum_of_singles(["closed"] * 200, route, idx)
    _rows_equal(fwd, rows, f"list {name}, {route}")
    # the backward's steps are those of the list
    flavours = T.step_flavours(x[active])
    assert set(flavours) == {"closed"}
    tot, tot_abs, _ = field.sum_of_singles(flavours, route, active)
    _bound_ratio(grads, tot, tot_abs, len(active), f"list {name}, {route}")


# e. several steps per wave: one workgroup (NARUTO_DEBUG_BWD_BLOCKS is read once per process: a child interpreter)
_ONE_BLOCK_CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import bf16_twin as T
import test_gpu_bwd_bf16 as B
gpu = torch.device("cuda", 0)
field = B.Field(gpu, n_in=577)
idx = list(range(577))
x = field.pts.x[idx]
assert set(T.step_flavours(x)) == {"closed"}
out = {}
tot, tot_abs, rows = field.sum_of_singles(["closed"] * 577, "raw", idx)
fwd, grads = field.run(x, field.pts.cot_of(idx, "raw"), "raw")
B._rows_equal(fwd, rows, "577 points, one workgroup")
out["autograd"] = B._bound_ratio(grads, tot, tot_abs, 577, "577 points, one workgroup")
d_raw, _ = B._list_cotangents(field, idx, "raw", idx)
fwd, grads = B._c_entry(field, x, d_raw, None, idx, color=True)
B._rows_equal(fwd, rows, "577 points, one workgroup, identity list")
out["identity list"] = B._bound_ratio(grads, tot, tot_abs, 577, "577 points, one workgroup, identity list")
json.dump(out, open(sys.argv[2], "w"))
"""


def test_several_steps_per_wave(gpu, tmp_path):
    """577 = 2 * 4 * 64 + 65 in-range points on ONE workgroup: wave 0 runs the steps 0, 4, 8, wave 1 ends on a one-entry step -- later steps
    re-read their list entries.  Through autograd and with the identity list through the C entry point; the singles come from the same child."""
    script = tmp_path / "child.py"
    script.write_text(_ONE_BLOCK_CHILD)
    try:
        LF.run_child(script, [tmp_path / "out.json"], {"NARUTO_DEBUG_BWD_BLOCKS": "1"}, timeout=300)
    except Exception as e:
        raise AssertionError(f"the one-workgroup child failed:\n{getattr(e, 'stdout', '')}\n{getattr(e, 'stderr', '')}") from e
    out = json.load(open(tmp_path / "out.json"))
    print(f"one workgroup, 577 points: worst error / bound {out}")
    assert set(out) == {"autograd", "identity list"} and all(v <= 1.0 for r in out.values() for v in r.values()), out


# f. repeatability
@pytest.mark.parametrize("n_pts", [65, 257])
def test_all_six_gradients_repeat_bitwise(field, n_pts):
    idx = list(range(n_pts))
    _, a = field.run(field.pts.x[idx], field.pts.cot_of(idx, "raw"), "raw")
    _, b = field.run(field.pts.x[idx], field.pts.cot_of(idx, "raw"), "raw")
    for k in T.NAMES:
        assert float(a[k].abs().max()) > 0.0, k
        assert torch.equal(a[k], b[k]), f"gradient {k}: {int((a[k] != b[k]).sum())} entries differ between identical runs"


# --------------------------------------------------------------------------------------------- 3. uncertainty grid too large for the scatter
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_uncertainty_grid_beyond_the_scatter(gpu, field, mode):
    """uncert_voxel = 0.04 on the office box: 121 x 139 x 86 voxels = 89 chunks of 16 384, more than the 64 the scatter takes, so the backward
    adds to the grid with float atomics.  65 points inside the box, raw cotangents (fifth column non-zero): the grid's gradient against oracle
    autograd, the other five against the 0.1-voxel run of the same points (which do not see the grid)."""
    big = Field(gpu, n_in=T.N_ANCHOR_IN_RANGE, uncert_voxel=0.04, mode=mode)
    small = field if mode == "bf16" else Field(gpu, n_in=T.N_ANCHOR_IN_RANGE, mode=mode)
    assert tuple(big.ora.uncert_grid.shape) == (121, 139, 86) and big.ora.uncert_grid.numel() > 64 * 16384
    inside = [i for i in range(field.pts.n_in) if ((field.pts.x[i] >= 0.0) & (field.pts.x[i] <= 1.0)).all()]
    idx = inside[:65]
    x, cot = field.pts.x[idx], field.pts.cot_of(idx, "raw")
    assert x.shape == (65, 3) and idx[:T.N_INSIDE] == list(range(T.N_INSIDE)) and (cot["raw"][:, 4] != 0.0).all()
    _, got = big.run(x, cot, "raw")
    _, ref = small.run(x, cot, "raw")
    for p in T.leaves(big.ora).values():
        p.grad = None
    (big.ora.query_color_sdf(torch.from_numpy(x)) * torch.from_numpy(cot["raw"])).sum().backward()
    want = big.ora.uncert_grid.grad
    assert float(want.abs().max()) > 0.0 and bool((got["uncert_grid"].cpu()[want != 0] != 0).any())
    H.grad_close(got["uncert_grid"], want, f"{mode}: uncert_grid gradient through the atomics")
    others = [k for k in T.NAMES if k != "uncert_grid"]
    _nonzero_where_the_reference_is({k: got[k].cpu() for k in others}, {k: ref[k].cpu() for k in others}, f"{mode}, large grid")
    if mode == "fp32":
        for k in others:
            H.grad_close(got[k], ref[k], f"fp32, large grid: {k} against the 0.1-voxel run")
        return
    # bf16: section 2's bound, with the singles of the 0.1-voxel field (these five gradients do not see the grid)
    tot, tot_abs, _ = field.sum_of_singles(["closed"] * 65, "raw", idx)
    for k in others:
        bound = T.composition_bound(65, tot_abs[k], tot[k])
        for what, a, b in (("the 0.1-voxel run", got[k].double(), ref[k].double()), ("the sum of the singles", got[k].double(), tot[k])):
            err = (a - b).abs()
            assert bool((err <= bound).all()), f"bf16, large grid: {k} differs from {what} by up to {float(err.max()):.3e} (worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3g})"


# --------------------------------------------------------------------------------------------- 4. the weight image against in-kernel staging
def _rays_33(cfg, in_range):
    """33 rays of syn.random_rays (a tenth without a depth).  in_range: the first 33 of 400 whose samples all stay inside the closed-form OneBlob's
    range -- origin and the point at far + 0.5 are inside (-0.93, 1.93), and the range is convex."""
    from naruto_amd import synthetic as syn
    if not in_range:
        return syn.random_rays(33, cfg["mapping"]["bound"], seed=41, zero_depth_frac=0.1)
    rays = syn.random_rays(400, cfg["mapping"]["bound"], seed=41, zero_depth_frac=0.1)
    bb = np.array(cfg["mapping"]["bound"], dtype=np.float32)
    ends = [(rays["rays_o"] + rays["rays_d"] * z - bb[:, 0]) / (bb[:, 1] - bb[:, 0]) for z in (0.0, cfg["cam"]["far"] + 0.5)]
    keep = np.nonzero(~T.is_far(ends[0]) & ~T.is_far(ends[1]))[0][:33]
    rays = {k: np.ascontiguousarray(v[keep]) for k, v in rays.items()}
    assert len(keep) == 33 and (rays["target_d"] <= 0).any() and (rays["target_d"] > 0).sum() > 20
    return rays


@pytest.mark.parametrize("in_range", [True, False], ids=["rays_in_range", "rays_with_far_samples"])
def test_weight_image_against_in_kernel_staging(gpu, in_range):
    """One bf16 mapping iteration at 33 rays x 43 samples twice: through the fused training path, whose backward fetches the weight images that
    k_loss_bwd_fused prepared (w_img), and through the modular operators (the steps of NarutoFieldHIP.forward with fused_train = False), where
    k_query_bwd_bf stages the weights itself.

    The two routes' forwards tile the samples differently -- the fused one a ray at a time (43 samples and padding lanes), the flat one 64
    consecutive entries of the point list, across rays -- and each tile takes the closed or the dense OneBlob form by __all.  With every sample
    inside the closed form's range both take the closed form everywhere: raw agrees bit for bit on the samples both evaluated, so the
    cotangents are the same bits and the six gradients meet test_fused_train_node_equals_the_modular_operators' 2e-6 of the scale + 1e-4
    relative.  With rays that leave the range (5 of the 33 drawn without the selection) a sample can sit in a dense tile by one route and a
    closed one by the other, raw differs by design (measured: 2 of 1419 samples, by up to 3.7e-9), and only losses and maps are compared."""
    from naruto_amd import ops
    from oracle import spec_torch as S
    cfg = H.office_cfg(14, perturb=1.0, n_samples_d=32)
    cfg["decoder"]["mlp_precision"] = "bf16"
    ora = H.make_oracle(cfg, 0.2, 41)
    rays = _rays_33(cfg, in_range)
    t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    rand = torch.rand(33, 43, device=gpu, generator=torch.Generator(gpu).manual_seed(5))
    # fused
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    assert m._handle().mlp_mode == "bf16" and m.fused_train
    m.strict_assert = True
    ret_f = m.forward(*t, rand=rand)
    S.total_loss(ret_f, cfg["training"]).backward()
    torch.cuda.synchronize()
    (st,) = m._node_states.values()
    raw_f, z_f = st.raw.reshape(33, 43, 5).clone(), st.z_vals.reshape(33, 43).clone()
    g_f = {k: v.detach().clone() for k, v in H.hip_grads(m).items()}
    # modular
    m2 = H.make_hip_from_oracle(cfg, ora, gpu).train()
    z = m2._sample_z(t[0], t[3], rand)
    rgb, depth, _, _, _, _, raw_m, losses = ops.render_train(m2._handle(), m2._params(), t[0], t[1], z, t[2], t[3], cfg["cam"]["depth_trunc"],
                                                            cfg["training"]["rgb_missing"], group=None, n_rays_total=0, smooth=None)
    ret_m = {"rgb": rgb, "depth": depth, "rgb_loss": losses[0], "depth_loss": losses[1], "sdf_loss": losses[2], "fs_loss": losses[3],
             "psnr": losses[4].detach(), "uncert_loss": losses[5]}
    S.total_loss(ret_m, cfg["training"]).backward()
    torch.cuda.synchronize()
    g_m = H.hip_grads(m2)
    assert torch.equal(z_f, z), "the two routes sampled different depths"
    bb = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32, device=gpu)
    xn = ((t[0][:, None, :] + t[1][:, None, :] * z[..., None] - bb[:, 0]) / (bb[:, 1] - bb[:, 0])).reshape(-1, 3).cpu().numpy()
    assert bool(T.is_far(xn).any()) != in_range
    evaluated = (raw_f != 0).any(-1)                    # (the fused forward leaves the samples behind a ray's early exit at zero)
    differ = (raw_f != raw_m).any(-1) & evaluated
    print(f"weight image, rays in range {in_range}: {int(evaluated.sum())} of {evaluated.numel()} samples evaluated by both routes, raw differs at {int(differ.sum())}")
    assert int(evaluated.sum()) > evaluated.numel() // 2
    for k in ("rgb", "depth", "rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "uncert_loss"):
        H.assert_close(ret_f[k].reshape(-1), ret_m[k].reshape(-1), 1e-6, f"weight image.{k}", rel=1e-5)
    if not in_range:
        return
    assert not bool(differ.any()), f"raw differs between the fused and the flat bf16 forward at {int(differ.sum())} of {int(evaluated.sum())} samples, by up to {float((raw_f - raw_m)[differ].abs().max()):.3e}"
    for k, g in g_f.items():
        want = g_m[k]
        assert float(want.abs().max()) > 0.0, k
        H.assert_close(g, want, 2e-6 * float(want.abs().max()), f"weight image.grad.{k}", rel=1e-4)

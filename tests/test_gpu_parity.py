"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the golden fixtures.

Tolerances (north_star: outputs within 1e-4 fp32 of the reference PyTorch path on identical rays):
  TOL_OUT  = 1e-4 absolute on every rendered / queried output (values are O(1));
  gradients: 1e-4 of the largest gradient magnitude of that tensor + 1e-3 relative.
"""
import os

import numpy as np
import pytest
import torch

from naruto_amd import synthetic as syn
from oracle import spec_torch as S

import helpers as H

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4


grad_close = H.grad_close


# --------------------------------------------------------------------------------------------- hardware layout probes
def test_mfma_layout(gpu, built_lib):
    """D = A.B with v_mfma_f32_32x32x2_f32: A lane l = A[l&31][l>>5], B lane l = B[l>>5][l&31],
    D lane l reg r = D[(r&3)+8(r>>2)+4(l>>5)][l&31].  Asymmetric operands catch transposes."""
    rs = np.random.RandomState(0)
    A = rs.normal(size=(32, 2)).astype(np.float32)
    B = rs.normal(size=(2, 32)).astype(np.float32)
    a = torch.tensor([A[l & 31, l >> 5] for l in range(64)], device=gpu)
    b = torch.tensor([B[l >> 5, l & 31] for l in range(64)], device=gpu)
    out = torch.zeros(64 * 16, device=gpu)
    from naruto_amd import _lib
    _lib.check(built_lib.naruto_debug_mfma_layout(a.data_ptr(), b.data_ptr(), out.data_ptr(), None))
    torch.cuda.synchronize()
    out = out.cpu().numpy().reshape(64, 16)
    D = A.astype(np.float64) @ B.astype(np.float64)
    for l in range(64):
        for r in range(16):
            row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
            assert abs(out[l, r] - D[row, l & 31]) < 1e-5, (l, r)


def test_mfma_bf16_layout(gpu, built_lib):
    """D = A.B with v_mfma_f32_32x32x16_bf16: A lane l = A[l&31][8(l>>5) + e], B lane l = B[8(l>>5) + e][l&31] (e = 0..7, eight bf16
    in four registers), D as the fp32 form.  Operands are rounded to bf16 (nearest even), products are exact in fp32."""
    from naruto_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(1)
    A = torch.from_numpy(rs.normal(size=(32, 16)).astype(np.float32))
    B = torch.from_numpy(rs.normal(size=(16, 32)).astype(np.float32))
    out = torch.empty(64 * 16, device=gpu)
    Ag, Bg = A.to(gpu), B.to(gpu)                       # keep them alive: a temporary's block is recycled by the next allocation
    _lib.check(lib.naruto_debug_mfma_bf16_layout(Ag.data_ptr(), Bg.data_ptr(), out.data_ptr(), None), "debug_mfma_bf16_layout")
    torch.cuda.synchronize()
    D = (A.bfloat16().double() @ B.bfloat16().double()).float()
    got = out.cpu().reshape(64, 16)
    want = torch.empty(64, 16)
    for l in range(64):
        for r in range(16):
            want[l, r] = D[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5), l & 31]
    H.assert_close(got, want, 2e-6, "mfma bf16 layout", rel=1e-6)


def test_permlane32_swap(gpu, built_lib):
    v0 = torch.arange(64, dtype=torch.float32, device=gpu)
    v1 = torch.arange(64, dtype=torch.float32, device=gpu) + 100
    out = torch.zeros(128, device=gpu)
    from naruto_amd import _lib
    _lib.check(built_lib.naruto_debug_permlane_swap(v0.data_ptr(), v1.data_ptr(), out.data_ptr(), None))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    a, b = out[:64], out[64:]
    assert np.array_equal(a[:32], np.arange(32)) and np.array_equal(a[32:], 100 + np.arange(32))
    assert np.array_equal(b[:32], 32 + np.arange(32)) and np.array_equal(b[32:], 132 + np.arange(32))


# --------------------------------------------------------------------------------------------- A1
@pytest.mark.parametrize("n_samples_d,perturb", [(32, 0.0), (32, 1.0), (117, 1.0), (0, 0.0)])
def test_sample_z(gpu, n_samples_d, perturb):
    from naruto_amd import ops
    rs = np.random.RandomState(3)
    n = 257
    td = rs.uniform(0.2, 4.9, size=(n, 1)).astype(np.float32)
    td[::7] = 0.0
    td[5] = -1.0
    td[6] = 250.0
    td[8] = 2.5            # exact tie with a uniform sample when 5/(n-1) divides it
    S_tot = n_samples_d + 11
    rand = rs.uniform(size=(n, S_tot)).astype(np.float32) if perturb > 0 else None
    want = S.sample_z(n, torch.from_numpy(td), 0.0, 5.0, n_samples_d, 11, 0.1, perturb,
                      rand=None if rand is None else torch.from_numpy(rand))
    got = ops.sample_z(n, torch.from_numpy(td).to(gpu), 0.0, 5.0, n_samples_d, 11, 0.1,
                       rand=None if rand is None else torch.from_numpy(rand).to(gpu))
    H.assert_close(got, want, 2e-6, "z_vals", rel=5e-7)
    if perturb == 0:
        assert bool((got[:, 1:] >= got[:, :-1]).all()), "z_vals must be sorted"


def test_sample_z_no_depth(gpu):
    from naruto_amd import ops
    want = S.sample_z(9, None, 0.0, 5.0, 0, 0, 0.0, 0.0, n_samples=64)
    got = ops.sample_z(9, None, 0.0, 5.0, 0, 0, 0.0, n_samples=64, device=gpu)
    H.assert_close(got, want, 1e-6, "z_vals(no depth)")


# --------------------------------------------------------------------------------------------- A3 / A9
@pytest.mark.parametrize("hash_size", [12, 16])
def test_query_golden(gpu, hash_size):
    g = H.load_golden(f"g3_query_volume_t{hash_size}")
    cfg = H.office_cfg(hash_size)
    w = {k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")}
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights=w)
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    with torch.no_grad():
        for tag in ("pts", "oob"):
            p = torch.from_numpy(g[tag]).to(gpu)
            H.assert_close(m.query_sdf(p, embed=True), g[f"{tag}_embed"], 1e-6, f"{tag}.embed")
            H.assert_close(m.query_sdf(p, return_uncert=True), g[f"{tag}_sdf_uncert"], TOL_OUT, f"{tag}.sdf_uncert")
            sdf, geo = m.query_sdf(p, return_geo=True)
            H.assert_close(sdf, g[f"{tag}_sdf"], TOL_OUT, f"{tag}.sdf")
            H.assert_close(geo, g[f"{tag}_geo"], TOL_OUT, f"{tag}.geo")
            H.assert_close(m.query_color_sdf(p), g[f"{tag}_raw"].reshape(-1, 5), TOL_OUT, f"{tag}.raw")
            H.assert_close(m.query_color(p), g[f"{tag}_color"].reshape(-1, 3), TOL_OUT, f"{tag}.color")
    from naruto_amd.field import get_map_volumes
    um, sv = get_map_volumes(m.query_sdf, m.bounding_box, float(g["map_voxel"]))
    H.assert_close(sv, g["map_sdf"], TOL_OUT, "map.sdf")
    H.assert_close(um, g["map_uncert"], TOL_OUT, "map.uncert")


@pytest.mark.parametrize("hash_size", [12, 16])
def test_query_boundary_sweeps(gpu, hash_size):
    """Lines through the unit cube and well beyond it on every axis (-1.2 .. 2.2, 4001 steps, incl. the exact values 0, 1,
    the bin edges k/16 and the switch-over points of the kernels' fast paths: the closed-form OneBlob inside (-0.93, 1.93),
    the wrap-free dense-level indices inside the grid): every output against the oracle."""
    cfg = H.office_cfg(hash_size)
    ora = H.make_oracle(cfg, 0.25, 61).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    rs = np.random.RandomState(61)
    sweep = np.unique(np.concatenate([np.linspace(-1.2, 2.2, 4001), np.arange(-19, 36) / 16.0, [-0.93, 1.93, -0.9375, 1.9375],
                                      1.0 - 2.0 ** -np.arange(1, 24), 2.0 ** -np.arange(1, 24)])).astype(np.float32)
    pts = []
    for axis in range(3):
        p = np.tile(rs.uniform(0.05, 0.95, (1, 3)).astype(np.float32), (len(sweep), 1))
        p[:, axis] = sweep
        pts.append(p)
        q = rs.uniform(-0.3, 1.3, (len(sweep), 3)).astype(np.float32)         # the other two coordinates anywhere, some outside
        q[:, axis] = sweep
        pts.append(q)
    x = torch.from_numpy(np.concatenate(pts))
    with torch.no_grad():
        want_raw = ora.query_color_sdf(x)
        want_su, want_geo = ora.query_sdf(x, return_geo=True)
        want_emb = ora.query_sdf(x, embed=True)
        xg = x.to(gpu)
        H.assert_close(m.query_sdf(xg, embed=True), want_emb, 2e-6, "sweep.embed")
        H.assert_close(m.query_color_sdf(xg), want_raw.reshape(-1, 5), TOL_OUT, "sweep.raw")
        got_su, got_geo = m.query_sdf(xg, return_geo=True)
        H.assert_close(got_su, want_su, TOL_OUT, "sweep.sdf")
        H.assert_close(got_geo, want_geo, TOL_OUT, "sweep.geo")


@pytest.mark.parametrize("case", list(range(10)))
def test_random_field_configs(gpu, case):
    """Drawn scene boxes (anisotropic, 1 .. 25 m), finest voxel sizes and table sizes 2^10 .. 2^18 (18: larger than the LDS-tiled
    scatter takes: the binned scatter): level tables, features, outputs and every gradient of the fused query against the oracle, on
    points inside and outside the box."""
    cfg, rs = H.drawn_field_config(case)
    ora = H.make_oracle(cfg, 0.25, 500 + case)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    sc, res, size, off = m._handle().levels()
    assert [int(v) for v in res] == [int(v) for v in ora.meta.resolution] and [int(v) for v in size] == [int(v) for v in ora.meta.size]
    n = int(rs.choice([1, 31, 64, 333, 1500]))
    x = torch.from_numpy(rs.uniform(-0.3, 1.3, (n, 3)).astype(np.float32))
    c = torch.from_numpy(rs.normal(size=(n, 5)).astype(np.float32))
    raw_o = ora.query_color_sdf(x)
    (raw_o * c).sum().backward()
    H.assert_close(m.query_sdf(x.to(gpu), embed=True), ora.query_sdf(x, embed=True).detach(), 2e-6, f"case {case}: embed")
    raw_h = m.query_color_sdf(x.to(gpu))
    H.assert_close(raw_h, raw_o.detach().reshape(-1, 5), TOL_OUT, f"case {case}: raw")
    (raw_h * c.to(gpu)).sum().backward()
    # a sample on a ReLU kink may move its 128 table entries and one row of each first layer (see test_train_step_random_shapes)
    with torch.no_grad():
        feats, pos = S.hash_encode(x, ora.table, ora.meta).double(), S.oneblob_encode(x, 16).double()
        h = torch.cat([feats, pos], -1) @ ora.sdf_w0.double().T
        cc = torch.cat([pos, (torch.relu(h) @ ora.sdf_w1.double().T)[:, 1:]], -1) @ ora.col_w0.double().T
        n_kink = int(((h.abs() < 2e-6).any(1) | (cc.abs() < 2e-6).any(1)).sum())
    gh, go = H.hip_grads(m), H.ora_grads(ora)
    budget = {"table": 128 * n_kink, "sdf_w0": 80 * n_kink, "col_w0": 63 * n_kink}
    for k in gh:
        got, want = gh[k].reshape(-1).double().cpu(), go[k].reshape(-1).double()
        scale = max(float(want.abs().max()), 1e-12)
        bad = (got - want).abs() > 1e-4 * scale + 1e-3 * want.abs()
        assert int(bad.sum()) <= budget.get(k, 0), f"case {case} (T=2^{cfg['grid']['hash_size']}, n={n}): grad.{k}: {int(bad.sum())} entries off, max err {float((got - want).abs().max()):.3e}, scale {scale:.3e}"


@pytest.mark.parametrize("kind", ["office_t16", "mp3d", "unit1024"])
def test_hash_encode_vs_oracle(gpu, kind):
    from naruto_amd import config as C
    if kind == "office_t16":
        cfg = H.office_cfg(16)
    elif kind == "mp3d":
        cfg = C.mp3d_large_config()
    else:
        cfg = C.unit_cube_config(1024, 16)
    ora = H.make_oracle(cfg, 0.3, 11)
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    scale, res, size, off = m._handle().levels()
    assert np.array_equal(np.asarray(res), ora.meta.resolution) and np.array_equal(np.asarray(size), ora.meta.size)
    assert np.array_equal(np.asarray(off), ora.meta.offset)
    assert np.array_equal(np.asarray(scale, np.float32), ora.meta.scale)
    rs = np.random.RandomState(5)
    x = np.concatenate([rs.uniform(0, 1, size=(3000, 3)), rs.uniform(-0.7, 1.7, size=(1000, 3)),
                        np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 1]])]).astype(np.float32)
    with torch.no_grad():
        want = ora.query_sdf(torch.from_numpy(x), embed=True)
        got = m.query_sdf(torch.from_numpy(x).to(gpu), embed=True)
    H.assert_close(got, want, 2e-6, f"{kind}.embed")


# --------------------------------------------------------------------------------------------- fused inference render
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("n_samples_d,with_depth", [(32, True), (117, True), (181, True), (40, False)])
def test_render_fused_equals_the_three_operators(gpu, mode, n_samples_d, with_depth):
    """naruto_render_fwd (render_rays without autograd: sampling + field query + compositing in one launch, raw kept on chip)
    against the sample_z / field_query / composite operators it replaces -- same kernels' arithmetic, so the rendered maps are
    bit-identical; rays of 128 / 192 samples also stop early (raw zero behind the truncation band), which no output can see."""
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=n_samples_d)
    cfg["training"]["n_samples"] = n_samples_d
    cfg["decoder"]["mlp_precision"] = mode
    ora = H.make_oracle(cfg, 0.25, 91)
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    N = 203
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=91, zero_depth_frac=0.1)
    ro, rd = torch.from_numpy(rays["rays_o"]).to(gpu), torch.from_numpy(rays["rays_d"]).to(gpu)
    td = torch.from_numpy(rays["target_d"]).to(gpu) if with_depth else None
    S_tot = n_samples_d + (cfg["training"]["n_range_d"] if with_depth else 0)
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(5)).to(gpu)
    with torch.no_grad():
        a = m.render_rays(ro, rd, target_d=td, rand=rand, fused=False)
        b = m.render_rays(ro, rd, target_d=td, rand=rand)                      # no autograd: the fused launch
        c = m.render_rays(ro, rd, target_d=td, rand=rand, want_raw=False)
    assert "raw" in b and "raw" not in c and "z_vals" not in c
    assert torch.equal(a["z_vals"], b["z_vals"])
    # Same tile code; what can differ is which points share a 64-point tile (the operator chain tiles the flat point list, the fused
    # kernel tiles ray by ray): the OneBlob closed form / dense form is chosen per tile, and the two agree to ~1e-6.  When the
    # samples per ray are a multiple of 64 the tilings coincide and everything is bit-identical.
    # (Round 5, exact mode: the operator chain's field query runs its matrix phase as three-piece bf16 products on the XDL pipe, the fused
    # render's register-form tile -- rays of more than 64 samples -- keeps the fp32 matrix instruction: both within one fp32 rounding of the
    # exact sums, 6e-8 apart (tools/fwd_lab.hip).  The bf16 mode runs the same chain in both and stays bit-identical.)
    same_tiles = S_tot % 64 == 0 and mode != "fp32"
    for k in ("raw", "rgb", "depth", "disp_map", "acc_map", "depth_var", "uncert_map"):
        if same_tiles:
            assert torch.equal(a[k], b[k]), f"{k}: fused render differs from the operator chain ({mode}, S={S_tot})"
        else:
            H.assert_close(b[k], a[k], 5e-6 if mode == "fp32" else 2e-3, f"fused.{k} ({mode}, S={S_tot})", rel=1e-5)
    # without raw the rays may stop early behind the truncation band: invisible in every rendered map
    for k in ("rgb", "depth", "disp_map", "acc_map", "depth_var", "uncert_map"):
        assert torch.equal(b[k], c[k]), f"{k}: want_raw=False changes the result"
    if mode == "fp32":                                                        # and the oracle, for good measure
        ora.eval()
        with torch.no_grad():
            o = ora.render_rays(ro.cpu(), rd.cpu(), target_d=td.cpu() if with_depth else None, rand=rand.cpu())
        for k in ("rgb", "depth", "depth_var", "uncert_map", "acc_map"):
            H.assert_close(b[k], o[k], TOL_OUT, f"fused.{k}")


# --------------------------------------------------------------------------------------------- bf16 MLP mode
from oracle import spec_bf16 as BF          # the bf16 mode's arithmetic restated (rounding points cited against the kernels) + its bound to the exact network


def _bf16_emulated_raw(ora, x):
    """raw and the sdf net's outputs of the bf16 mode: oracle/spec_bf16.py (pinned to the exact network by tests/test_oracle.py)."""
    with torch.no_grad():
        raw, out = BF.query_color_sdf_bf16(ora, x)
    return raw, out


# Both sides round intermediate activations to bf16; where an fp32 sum lands within its accumulation-order noise of a bf16
# rounding boundary the two can round it to neighbouring bf16 values (a 2^-8 relative step on ONE operand).  So: nearly every
# element agrees to fp32 accuracy, a handful may differ by such a step -- and nothing by more.
def _close_up_to_bf16_flips(a, b, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs()
    tight = err <= 2e-5 + 1e-5 * b.abs()
    assert float(tight.float().mean()) > 0.998, f"{what}: only {float(tight.float().mean()):.4f} of the elements agree to fp32 accuracy"
    assert float(err.max()) <= 2e-3 * float(b.abs().max()), f"{what}: max err {float(err.max()):.3e} at scale {float(b.abs().max()):.3e}"


@pytest.mark.parametrize("hash_size", [12, 16])
def test_bf16_mode_matches_its_restatement(gpu, hash_size):
    """decoder.mlp_precision = 'bf16' (v_mfma_f32_32x32x16_bf16): raw, sdf / uncertainty and geo features against a torch
    restatement of exactly that arithmetic -- a layout or packing mistake cannot hide in a precision tolerance.  Points inside
    and outside the box, a count that leaves a partly filled 64-point tile."""
    cfg = H.office_cfg(hash_size)
    ora = H.make_oracle(cfg, 0.3, 61)
    cfg_bf = H.office_cfg(hash_size)
    cfg_bf["decoder"]["mlp_precision"] = "bf16"
    m = H.make_hip_from_oracle(cfg_bf, ora, gpu).eval()
    assert m._handle().mlp_mode == "bf16"
    rs = np.random.RandomState(61)
    x = torch.from_numpy(np.concatenate([rs.uniform(0, 1, (2000, 3)), rs.uniform(-0.4, 1.4, (333, 3))]).astype(np.float32))
    want, out = _bf16_emulated_raw(ora, x)
    with torch.no_grad():
        got = m.query_color_sdf(x.to(gpu))
        su, geo = m.query_sdf(x.to(gpu), return_geo=True, return_uncert=True)
    _close_up_to_bf16_flips(got, want, "bf16.raw")
    _close_up_to_bf16_flips(su[:, 0], out[:, 0], "bf16.sdf")
    _close_up_to_bf16_flips(geo, out[:, 1:], "bf16.geo")
    # and the distance to the exact (fp32) network is the bf16 rounding of the operands: ~2^-9 relative per product
    exact = ora.query_color_sdf(x).detach()
    err = (got.cpu() - exact).abs().max(0).values
    scale = exact.abs().max(0).values
    assert (err[:4] <= 2e-2 * scale[:4] + 1e-4).all(), f"bf16 vs fp32 network: {err.tolist()} at scales {scale.tolist()}"
    assert float(err[4]) <= 4e-6                              # the uncertainty channel does not pass through the MLPs


def test_query_fwd_flat_launch_shapes(gpu):
    """naruto_query_fwd in each of its three flat launch shapes, both MLP modes, against the oracle (exact mode) and the bf16
    restatement, at the neighbouring tests' tolerances.  The shapes go by tiles (of 64 points) per compute unit: 4 per CU is the last
    count of four-wave workgroups (256 threads), 6 per CU takes two-wave workgroups (128), and from 8 per CU on one eight-wave
    workgroup per CU walks the list (512) -- here 21 points short of 8 per CU, so that the last tile is partly filled.  One point
    list, one reference: the smaller cases are its prefixes."""
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.3, 73)
    cfg_bf = H.office_cfg(12)
    cfg_bf["decoder"]["mlp_precision"] = "bf16"
    m, m_bf = H.make_hip_from_oracle(cfg, ora, gpu).eval(), H.make_hip_from_oracle(cfg_bf, ora, gpu).eval()
    assert m_bf._handle().mlp_mode == "bf16"
    n_max = 8 * cu * 64 - 21
    x = torch.from_numpy(np.random.RandomState(73).uniform(-0.2, 1.2, (n_max, 3)).astype(np.float32))
    with torch.no_grad():
        want = ora.query_color_sdf(x).reshape(-1, 5)
    want_bf, _ = _bf16_emulated_raw(ora, x)
    xg = x.to(gpu)
    for n, shape in ((4 * cu * 64, "256 threads"), (6 * cu * 64, "128 threads"), (n_max, "512 threads")):
        with torch.no_grad():
            got, got_bf = m.query_color_sdf(xg[:n]), m_bf.query_color_sdf(xg[:n])
        H.assert_close(got, want[:n], TOL_OUT, f"{n} points ({shape}): raw")
        _close_up_to_bf16_flips(got_bf, want_bf[:n], f"{n} points ({shape}): bf16 raw")


def test_bf16_mode_backward_matches_its_restatement(gpu):
    """k_query_bwd_bf (everything in registers, transposes on the matrix core) against a torch restatement of its arithmetic:
    every matrix product with bf16-rounded operands and fp32 accumulation, ReLU masks from the bf16 forward.  All six gradients,
    incl. the table gradient through the scatter; a point count that leaves partly filled tiles in both 32-point halves."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.3, 67)
    cfg_bf = H.office_cfg(12)
    cfg_bf["decoder"]["mlp_precision"] = "bf16"
    m = H.make_hip_from_oracle(cfg_bf, ora, gpu)
    rs = np.random.RandomState(67)
    n = 2049 + 40
    x = torch.from_numpy(np.concatenate([rs.uniform(0, 1, (2049, 3)), rs.uniform(-0.3, 1.3, (40, 3))]).astype(np.float32))
    cot = torch.from_numpy(rs.normal(size=(n, 5)).astype(np.float32))
    cot[rs.uniform(size=n) < 0.1] = 0.0
    raw_o, _ = BF.query_color_sdf_bf16(ora, x)
    (raw_o * cot).sum().backward()
    raw_h = m.query_color_sdf(x.to(gpu))
    (raw_h * cot.to(gpu)).sum().backward()
    gh, go = H.hip_grads(m), H.ora_grads(ora)
    for k in gh:
        got, want = gh[k].reshape(-1).double().cpu(), go[k].reshape(-1).double()
        scale = float(want.abs().max())
        err = (got - want).abs()
        # bf16 rounding flips of single operands (see test_bf16_mode_matches_its_restatement) move an entry by <= ~2^-8 of ONE of its
        # ~2000 terms: far below 1e-3 of the scale; everything else agrees to accumulation-order accuracy
        assert float((err <= 2e-5 * scale).float().mean()) > 0.97, f"bf16 backward, {k}: {float((err <= 2e-5 * scale).float().mean()):.4f} within 2e-5 of the scale"
        assert float(err.max()) <= 1e-3 * scale, f"bf16 backward, {k}: max err {float(err.max()):.3e}, scale {scale:.3e}"


def _iteration_in_mode(cfg0, ora, rays, rand, smooth, mode, gpu):
    """One mapping iteration (forward + losses + backward) through naruto_train_* in the given MLP mode."""
    from naruto_amd import ops
    c = H.office_cfg(cfg0["grid"]["hash_size"], perturb=cfg0["training"]["perturb"], n_samples_d=cfg0["training"]["n_samples_d"])
    c["decoder"]["mlp_precision"] = mode
    m = H.make_hip_from_oracle(c, ora, gpu)
    tr, cam = c["training"], c["cam"]
    N = rays["rays_o"].shape[0]
    S_tot = tr["n_samples_d"] + tr["n_range_d"]
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0,
                      tr["smooth_weight"] if smooth else 0.0, 0.0], device=gpu)
    ug = torch.zeros_like(m.uncert_grid)
    ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"], far=cam["far"],
                       range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=rand is not None,
                       loss_weights=w, smooth=(tr["smooth_pts"], tr["smooth_vox"], tr["smooth_margin"]) if smooth else None, device_rng=False)
    args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]
    if smooth:
        ts.rand[N * S_tot:].copy_(torch.tensor([0.3, 0.6, 0.2, 0.1, 0.7, 0.4]))
    losses = ts.run(*args, rand=rand.to(gpu) if rand is not None else None).clone()
    torch.cuda.synchronize()
    grads = {k: v.detach().double().reshape(-1).clone() for k, v in ts.grads.items()}
    grads["uncert_grid"] = ug.double().reshape(-1).clone()
    return {"raw": ts.raw.reshape(-1, 5).clone(), "rgb": ts.rgb.clone(), "depth": ts.depth.clone(), "losses": losses, "grads": grads}


def test_bf16_mode_error_against_the_exact_mode(gpu):
    """What the bf16 speed mode costs in accuracy, as asserted bounds (3-5x what tools/bf16_error_study.py measured on MI355X,
    profiles/r02_bf16_error_study.txt): raw outputs, rendered maps, the five losses and every gradient against the exact fp32 mode
    of the same library on the same inputs -- the golden rays (64 x 43, no early termination) and BASELINE configs[1]'s batch
    (2048 x 128, jitter + smoothness).  At the full size a handful of rays change their first sdf sign change under bf16 noise
    (random-initialised network: the sdf hovers around zero), which moves their depth by metres: per-sample / per-ray maxima are
    meaningless there, means, losses and gradient directions are what is bounded."""
    g = H.load_golden("g1_render_train_t16")
    cfg = H.office_cfg(int(g["hash_size"]), perturb=float(g["perturb"]), n_samples_d=int(g["n_samples_d"]))
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights={k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")})
    rays = {k: g[k] for k in ("rays_o", "rays_d", "target_rgb", "target_d")}
    a = _iteration_in_mode(cfg, ora, rays, None, False, "fp32", gpu)
    b = _iteration_in_mode(cfg, ora, rays, None, False, "bf16", gpu)
    d_raw = (a["raw"] - b["raw"]).abs()
    assert float(d_raw[:, :4].max()) <= 2.5e-3 and float(d_raw[:, :4].mean()) <= 4e-4, f"golden raw: max {float(d_raw[:, :4].max()):.2e} mean {float(d_raw[:, :4].mean()):.2e}"
    assert float(d_raw[:, 4].max()) == 0.0                                       # the uncertainty channel does not pass through the MLPs
    assert float((a["rgb"] - b["rgb"]).abs().max()) <= 4e-4 and float((a["depth"] - b["depth"]).abs().max()) <= 1.5e-3
    for i, nm in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "uncert_loss")):
        la, lb = float(a["losses"][i]), float(b["losses"][i])
        assert abs(la - lb) <= 2e-4 * abs(la), f"golden {nm}: fp32 {la} bf16 {lb}"

    def cosine(x, y):
        return float((x @ y) / (x.norm() * y.norm() + 1e-300))
    floor = {"table": 0.998, "sdf_w0": 0.9995, "sdf_w1": 0.9999, "col_w0": 0.999, "col_w1": 0.9999, "uncert_grid": 0.9999}
    for k, lo in floor.items():
        c = cosine(a["grads"][k], b["grads"][k])
        assert c >= lo, f"golden grad {k}: cosine {c:.6f} < {lo}"
    rel = float((a["grads"]["table"] - b["grads"]["table"]).norm() / a["grads"]["table"].norm())
    assert rel <= 0.1, f"golden grad table: relative L2 error {rel:.3e}"

    cfg = H.office_cfg(16, perturb=1.0, n_samples_d=117)
    ora = H.make_oracle(cfg, 0.05, 77)
    rays = syn.random_rays(2048, cfg["mapping"]["bound"], seed=77, zero_depth_frac=0.05)
    rand = torch.rand(2048, 128, generator=torch.Generator().manual_seed(11))
    a = _iteration_in_mode(cfg, ora, rays, rand, True, "fp32", gpu)
    b = _iteration_in_mode(cfg, ora, rays, rand, True, "bf16", gpu)
    live = (a["raw"].abs().sum(1) > 0) & (b["raw"].abs().sum(1) > 0)               # samples both modes evaluated (early termination)
    assert float((a["raw"][live][:, :4] - b["raw"][live][:, :4]).abs().mean()) <= 5e-4
    bound = {"rgb_loss": 3e-4, "depth_loss": 1.5e-2, "sdf_loss": 1e-4, "fs_loss": 2e-4, "psnr": 1e-4, "uncert_loss": 1e-2}
    for i, nm in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "uncert_loss")):
        la, lb = float(a["losses"][i]), float(b["losses"][i])
        assert abs(la - lb) <= bound[nm] * abs(la), f"full-size {nm}: fp32 {la} bf16 {lb}"
    assert abs(float(a["losses"][9]) - float(b["losses"][9])) <= 1e-3 * abs(float(a["losses"][9]))
    for k in floor:
        c = cosine(a["grads"][k], b["grads"][k])
        assert c >= 0.985, f"full-size grad {k}: cosine {c:.6f}"


# --------------------------------------------------------------------------------------------- large tables: the binned scatter
@pytest.mark.parametrize("log2_T", [18, 20, 22])
def test_hash_encode_backward_large_tables(gpu, log2_T):
    """Tables of 2^18 .. 2^22 entries per level (configs[4]: unit cube, finest level 1024^3, 2^22 = the HBM-resident table):
    the levels beyond 2^17 entries go through the binned scatter (counting sort into 8 192-entry bins + one LDS accumulation
    per bin, no global float atomics).  Against oracle autograd on points inside / outside the box and with colliding
    points; and bitwise reproducible -- a second run and a permuted point order give the identical gradient."""
    from naruto_amd import config as C, ops
    cfg = C.unit_cube_config(1024, log2_T)
    ora = H.make_oracle(cfg, 0.3, 13)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    sc, res, size, off = m._handle().levels()
    assert np.array_equal(np.asarray(size), ora.meta.size) and np.array_equal(np.asarray(off), ora.meta.offset)
    assert max(size) == min(1 << log2_T, 1 << 22) or log2_T > 22
    rs = np.random.RandomState(log2_T)
    base = rs.uniform(0, 1, size=(6000, 3))
    x = np.concatenate([base, base[:500], base[:500] + 1e-4,                     # exact repeats and near neighbours: collisions inside a bin
                        rs.uniform(-0.6, 1.6, size=(700, 3)), np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5]])]).astype(np.float32)
    c = rs.normal(size=(x.shape[0], 32)).astype(np.float32)
    c[rs.uniform(size=x.shape[0]) < 0.2] = 0.0                                    # points without a cotangent are skipped by the sort
    xt, ct = torch.from_numpy(x), torch.from_numpy(c)
    feat_o = ora.query_sdf(xt, embed=True)
    (feat_o * ct).sum().backward()
    want = ora.table.grad
    table = m.embed_fn.params

    def run(xx, cc):
        table.grad = None
        f = ops.hash_encode(m._handle(), xx.to(gpu), table)
        (f * cc.to(gpu)).sum().backward()
        return table.grad.detach().clone()

    got = run(xt, ct)
    H.assert_close(ops.hash_encode(m._handle(), xt.to(gpu), table), feat_o.detach(), 2e-6, f"T{log2_T}.embed")
    grad_close(got, want, f"T{log2_T}.grad.table")
    for l in range(16):                                                           # every level carries its share (tiled and binned ones)
        a, b = got[2 * off[l]:2 * off[l + 1]].double().cpu(), want[2 * off[l]:2 * off[l + 1]].double()
        assert abs(float(a.abs().sum()) - float(b.abs().sum())) <= 1e-4 * float(b.abs().sum()) + 1e-12, f"level {l}"
    assert torch.equal(run(xt, ct), got), "second run differs: the scatter is not reproducible"
    # the binned levels (more than 2^17 entries) accumulate in fixed point: ANY point order gives the same bits.  (The small dense
    # levels of the LDS-tiled scatter pre-sum runs of consecutive points in fp32 registers: reproducible, not order-free.)
    first_big = next(l for l in range(16) if size[l] > (1 << 17))
    perm = torch.from_numpy(rs.permutation(x.shape[0]))
    got_p = run(xt[perm], ct[perm])
    assert torch.equal(got_p[2 * off[first_big]:], got[2 * off[first_big]:]), "permuted point order changes the binned levels' gradient"
    grad_close(got_p, want, f"T{log2_T}.grad.table (permuted)")


def test_configs4_in_its_defining_form(gpu):
    """BASELINE configs[4] as named: unit cube, finest level 1024^3, T = 2^22 (281 MB, HBM-resident table: counting-sort scatter), MLPs in
    the bf16 mode -- one mapping iteration (reduced ray count, smoothness lattice included) against the CPU oracle.  The table and
    uncertainty paths are fp32 in both modes, so the losses and the gradient directions are bounded as in the bf16 study
    (tools/bf16_error_study.py), and against the exact mode of the same library the table gradient stays within the bf16 noise of
    the cotangents that feed it."""
    from naruto_amd import config as C, ops
    cfg = C.unit_cube_config(1024, 22, perturb=1.0)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.05, 53)
    N = 301
    S_tot = tr["n_samples_d"] + tr["n_range_d"]
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=53, zero_depth_frac=0.1)
    rays["target_d"] = (rays["target_d"] * 0.25).astype(np.float32)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    r6 = torch.tensor([0.35, 0.1, 0.75, 0.2, 0.9, 0.5])
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(5))
    sp, vox, mar, w_s = 12, 0.02, 0.01, 0.5
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, w_s, 0.0])
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    sm_o = S.smoothness(ora, sp, vox, mar, r6[:3], r6[3:])
    total_o = S.total_loss(ret_o, tr) + w_s * sm_o
    total_o.backward()
    go = H.ora_grads(ora)
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    out = {}
    for mode in ("fp32", "bf16"):
        c = C.unit_cube_config(1024, 22, perturb=1.0)
        c["decoder"]["mlp_precision"] = mode
        m = H.make_hip_from_oracle(c, ora, gpu)
        assert m._handle().n_params == ora.table.numel()
        ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                           near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                           perturb=True, loss_weights=w.to(gpu), smooth=(sp, vox, mar), device_rng=False)
        ts.rand[N * S_tot:].copy_(r6)
        losses = ts.run(*args, rand=rand.to(gpu)).clone()
        torch.cuda.synchronize()
        out[mode] = (losses.cpu(), {k: v.detach().double().cpu().reshape(-1) for k, v in ts.grads.items()})
        del ts, m
    lb, gb = out["bf16"]
    la, ga = out["fp32"]
    for i, k in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")):
        ref = float(ret_o[k].detach())
        assert abs(float(lb[i]) - ref) <= 5e-3 * abs(ref) + 1e-6, f"bf16 T22 {k}: {float(lb[i])} vs {ref}"
    H.assert_close(lb[8].reshape(-1), sm_o.reshape(-1), 1e-7, "bf16 T22 smoothness term (fp32 path)", rel=1e-4)
    assert abs(float(lb[9]) - float(total_o.detach())) <= 5e-3 * abs(float(total_o.detach()))
    for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
        want = go[k].reshape(-1).double()
        cos = float(torch.dot(gb[k], want) / (gb[k].norm() * want.norm() + 1e-300))
        assert cos >= 0.99, f"bf16 T22 grad {k}: cosine {cos:.5f} against the oracle"
        rel = float((gb[k] - ga[k]).norm() / (ga[k].norm() + 1e-300))
        assert rel <= 0.12, f"bf16 T22 grad {k}: relative l2 distance {rel:.4f} from the exact mode"
    # the exact mode on the same inputs is the parity statement (as in test_train_step_large_tables)
    for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
        grad_close(ga[k], go[k].reshape(-1), f"fp32 T22 grad.{k}")


@pytest.mark.parametrize("log2_T", [18, 20, 22])
def test_train_step_large_tables(gpu, log2_T):
    """The trainer's fast path (naruto_train_forward / naruto_train_backward) on the unit-cube volume of configs[4] with 2^18 ..
    2^22-entry levels, reduced ray count: every loss and every gradient against the CPU oracle, with the smoothness lattice
    riding in the same scatter; then the optimiser fused into the backward (the binned scatter's last kernel steps the large
    levels in place) against gradients + a separate Adam launch, three iterations."""
    from naruto_amd import config as C, ops, trainer
    cfg = C.unit_cube_config(1024, log2_T, perturb=1.0)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.05, 29)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    N = 301
    S_tot = tr["n_samples_d"] + tr["n_range_d"]
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=29, zero_depth_frac=0.1)
    rays["target_d"] = (rays["target_d"] * 0.25).astype(np.float32)                # depths inside the unit cube (far = 1)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    r6 = torch.tensor([0.35, 0.1, 0.75, 0.2, 0.9, 0.5])
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(3))
    sp, vox, mar = 12, 0.02, 0.01
    w_s = 0.5
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, w_s, 0.0])
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    sm_o = S.smoothness(ora, sp, vox, mar, r6[:3], r6[3:])
    total_o = S.total_loss(ret_o, tr) + w_s * sm_o
    total_o.backward()
    go = H.ora_grads(ora)
    ug = torch.zeros_like(m.uncert_grid)
    ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"], far=cam["far"],
                       range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True,
                       loss_weights=w.to(gpu), smooth=(sp, vox, mar), device_rng=False)
    assert ops.handle_supports_overwrite(m._handle())
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    for rep in range(2):                                     # written, not accumulated: a second run gives the same table gradient
        ts.rand[N * S_tot:].copy_(r6)
        losses = ts.run(*args, rand=rand.to(gpu))
        torch.cuda.synchronize()
        for i, k in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")):
            H.assert_close(losses[i].reshape(-1), ret_o[k].reshape(-1), 1e-6, f"T{log2_T}.{k}", rel=1e-4)
        H.assert_close(losses[8].reshape(-1), sm_o.reshape(-1), 1e-7, f"T{log2_T}.smooth", rel=1e-4)
        H.assert_close(losses[9].reshape(-1), total_o.detach().reshape(-1), 1e-5, f"T{log2_T}.total", rel=1e-4)
        for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
            grad_close(ts.grads[k].reshape(-1), go[k].reshape(-1), f"T{log2_T}.rep{rep}.grad.{k}")
    del ts, ora, go
    # fused optimiser vs gradients + separate Adam, same in-kernel random numbers
    bound = torch.tensor(cfg["mapping"]["bound"])
    torch.manual_seed(4)
    a = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    with torch.no_grad():
        a.model.embed_fn.params.mul_(500.0)                  # tcnn's U(-1e-4, 1e-4) init scaled up so that the table matters
    b.model.load_state_dict(a.model.state_dict())
    b.iter_state.copy_(a.iter_state)
    a.fuse_optimizer = False
    for it in range(3):
        rays = syn.random_rays(257, cfg["mapping"]["bound"], seed=40 + it, zero_depth_frac=0.1)
        rays["target_d"] = (rays["target_d"] * 0.25).astype(np.float32)
        tt = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        ra, la = a.step(*tt, smooth=True)
        rb, lb = b.step(*tt, smooth=True)
        H.assert_close(lb.reshape(-1), la.reshape(-1), 1e-7, f"T{log2_T}.iter{it}.loss", rel=1e-6)
    assert next(iter(b._train_steps.values())).opt is not None and next(iter(a._train_steps.values())).opt is None
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        H.assert_close(q, p, 5e-6, f"T{log2_T}.param {n}", rel=1e-5)


# --------------------------------------------------------------------------------------------- A6 / A7
def test_composite_edges_golden(gpu):
    g = H.load_golden("g5_composite_edges")
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 1e-4, 7)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    raw = torch.from_numpy(g["raw"]).to(gpu).requires_grad_(True)
    z = torch.from_numpy(g["z_vals"]).to(gpu)
    outs = m.raw2outputs(raw, z, False)
    names = ("rgb", "disp_map", "acc_map", "weights", "depth", "depth_var", "uncert_map")
    for k, o in zip(names, outs):
        H.assert_close(o, g["out_" + k], TOL_OUT, f"composite.{k}", rel=1e-5)
    total = sum((torch.from_numpy(g["cot_" + k]).to(gpu) * o).sum() for k, o in zip(names, outs)
                if k in ("rgb", "depth", "uncert_map"))
    total.backward()
    grad_close(raw.grad, g["grad_raw"], "composite.grad_raw")


def test_composite_backward_all_cotangents(gpu):
    """Every output's cotangent path (incl. disp / acc / depth_var / weights) against oracle autograd."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 1e-4, 7)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rs = np.random.RandomState(1)
    n, s = 33, 70
    raw = rs.normal(size=(n, s, 5)).astype(np.float32)
    raw[..., 3] = np.sort(rs.normal(size=(n, s)).astype(np.float32) * 0.3, axis=1)[:, ::-1] + 0.05
    z = np.sort(rs.uniform(0.1, 5, size=(n, s)).astype(np.float32), axis=1)
    names = ("rgb", "disp_map", "acc_map", "weights", "depth", "depth_var", "uncert_map")
    r_c = torch.from_numpy(raw).requires_grad_(True)
    o_c = S.raw2outputs(r_c, torch.from_numpy(z), 0.1, 1.0, False)
    cot = [rs.normal(size=tuple(o.shape)).astype(np.float32) for o in o_c]
    sum((torch.from_numpy(c) * o).sum() for c, o in zip(cot, o_c)).backward()
    r_g = torch.from_numpy(raw).to(gpu).requires_grad_(True)
    o_g = m.raw2outputs(r_g, torch.from_numpy(z).to(gpu), False)
    for k, a, b in zip(names, o_g, o_c):
        H.assert_close(a, b, TOL_OUT, f"composite.{k}", rel=1e-5)
    sum((torch.from_numpy(c).to(gpu) * o).sum() for c, o in zip(cot, o_g)).backward()
    grad_close(r_g.grad, r_c.grad, "composite.grad_raw(all cotangents)")


# --------------------------------------------------------------------------------------------- A1-A8 end to end
@pytest.mark.parametrize("name", ["g1_render_train_t12", "g1_render_train_t16", "g1_render_train_init",
                                  "g6_render_train_perturb", "g1_render_train_s128"])
def test_render_train_golden(gpu, name):
    g = H.load_golden(name)
    cfg = H.office_cfg(int(g["hash_size"]), perturb=float(g["perturb"]), n_samples_d=int(g["n_samples_d"]))
    w = {k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")}
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights=w)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    t = {k: torch.from_numpy(g[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")}
    rand = torch.from_numpy(g["rand"]).to(gpu) if "rand" in g else None
    m.eval()
    with torch.no_grad():
        rend = m.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    H.assert_close(rend["z_vals"], g["out_z_vals"], 2e-6, f"{name}.z_vals")
    for k in ("raw", "rgb", "depth", "acc_map", "depth_var", "uncert_map"):
        H.assert_close(rend[k], g["out_" + k], TOL_OUT, f"{name}.{k}")
    H.assert_close(rend["disp_map"], g["out_disp_map"], TOL_OUT, f"{name}.disp_map", rel=1e-4)
    w_hip = m.raw2outputs(rend["raw"], rend["z_vals"], False)[3]
    H.assert_close(w_hip, g["out_weights"], TOL_OUT, f"{name}.weights")
    # training forward + backward with the reference's loss weights (coslam.py:154-174)
    m.train()
    m.strict_assert = True
    ret = m.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "uncert_loss"):
        H.assert_close(ret[k].reshape(-1), g["loss_" + k], 1e-5, f"{name}.{k}", rel=1e-4)
    loss = S.total_loss(ret, cfg["training"])
    H.assert_close(loss.reshape(-1), g["loss_total"], 1e-4, f"{name}.total", rel=1e-4)
    loss.backward()
    gh = H.hip_grads(m)
    for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1"):
        grad_close(gh[k], g["grad_" + k], f"{name}.grad.{k}")
    ug = np.zeros(int(np.prod(g["uncert_dims"])), np.float32)
    ug[g["grad_uncert_idx"]] = g["grad_uncert_val"]
    grad_close(gh["uncert_grid"].reshape(-1), ug, f"{name}.grad.uncert_grid")
    tg = gh["table"].detach().cpu().numpy()
    grad_close(tg[g["grad_table_idx"]], g["grad_table_val"], f"{name}.grad.table(probes)")
    meta = ora.meta
    lvl_sum = np.asarray([tg[meta.offset[l] * 2: meta.offset[l + 1] * 2].astype(np.float64).sum() for l in range(16)])
    lvl_abs = np.asarray([np.abs(tg[meta.offset[l] * 2: meta.offset[l + 1] * 2]).astype(np.float64).sum() for l in range(16)])
    np.testing.assert_allclose(lvl_abs, g["grad_table_level_abs"], rtol=2e-3, atol=1e-4 * g["grad_table_level_abs"].max())
    np.testing.assert_allclose(lvl_sum, g["grad_table_level_sum"], rtol=0, atol=2e-3 * g["grad_table_level_abs"].max())


@pytest.mark.parametrize("n_pts,with_geo", [(777, False), (2049, True)])
def test_query_backward_vs_oracle(gpu, n_pts, with_geo):
    """Full table / MLP / uncertainty-grid gradients of the fused query against oracle autograd."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 21)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rs = np.random.RandomState(2)
    x = rs.uniform(-0.2, 1.2, size=(n_pts, 3)).astype(np.float32)
    if with_geo:
        c_su = rs.normal(size=(n_pts, 2)).astype(np.float32)
        c_geo = rs.normal(size=(n_pts, 15)).astype(np.float32)
        su, geo = ora.query_sdf(torch.from_numpy(x), return_geo=True, return_uncert=True)
        ((su * torch.from_numpy(c_su)).sum() + (geo * torch.from_numpy(c_geo)).sum()).backward()
        su_g, geo_g = m.query_sdf(torch.from_numpy(x).to(gpu), return_geo=True, return_uncert=True)
        H.assert_close(su_g, su, TOL_OUT, "sdf_uncert")
        H.assert_close(geo_g, geo, TOL_OUT, "geo")
        ((su_g * torch.from_numpy(c_su).to(gpu)).sum() + (geo_g * torch.from_numpy(c_geo).to(gpu)).sum()).backward()
    else:
        c_raw = rs.normal(size=(n_pts, 5)).astype(np.float32)
        raw = ora.query_color_sdf(torch.from_numpy(x))
        (raw * torch.from_numpy(c_raw)).sum().backward()
        raw_g = m.query_color_sdf(torch.from_numpy(x).to(gpu))
        H.assert_close(raw_g, raw, TOL_OUT, "raw")
        (raw_g * torch.from_numpy(c_raw).to(gpu)).sum().backward()
    gh, go = H.hip_grads(m), H.ora_grads(ora)
    for k in gh:
        if go[k] is None:
            assert gh[k] is None or float(gh[k].abs().max()) == 0.0, k
            continue
        grad_close(gh[k], go[k], f"grad.{k}")


def test_backward_is_bitwise_reproducible(gpu):
    """No float atomics on the hot path: table (fixed-point LDS scatter), MLP weights (fixed summation order) and the uncertainty
    grid (units of the same scatter) come out bit-identical run after run."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 23)
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    rays = syn.random_rays(333, cfg["mapping"]["bound"], seed=23, zero_depth_frac=0.1)
    t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    runs = []
    for rep in range(3):
        for p_ in m.parameters():
            p_.grad = None
        ret = m.forward(*t)
        S.total_loss(ret, cfg["training"]).backward()
        runs.append({k: v.detach().clone() for k, v in H.hip_grads(m).items()})
    for k in runs[0]:
        assert float(runs[0][k].abs().max()) > 0, k
        assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), f"gradient {k} differs between identical runs"


def test_smoothness_backward(gpu):
    """query_sdf(embed=True) under autograd (Co-SLAM smoothness term, coslam.py:168)."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 22)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    off, jit = torch.tensor([0.3, 0.6, 0.2]), torch.tensor([0.1, 0.7, 0.4])
    want = S.smoothness(ora, 12, 0.1, 0.05, off, jit)
    want.backward()
    got = trainer.smoothness(m, cfg, 12, 0.1, 0.05, off, jit)
    got.backward()
    H.assert_close(got, want, 1e-7, "smoothness", rel=1e-4)
    grad_close(m.embed_fn.params.grad, ora.table.grad, "smoothness.grad.table")


def test_mapping_iterations_track_oracle(gpu):
    """Five full mapping iterations (forward, losses, backward, both Adams) stay on the oracle's trajectory."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.1, 31)
    tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), gpu)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    tr.model.load_state_dict(m.state_dict())
    g1, g2 = ora.param_groups()
    o_map = torch.optim.Adam(g1, betas=(0.9, 0.99))
    o_unc = torch.optim.Adam(g2, lr=1)
    ora.train()
    for it in range(5):
        rays = syn.random_rays(256, cfg["mapping"]["bound"], seed=100 + it)
        t = {k: torch.from_numpy(v) for k, v in rays.items()}
        if it % 5 == 0:
            o_unc.zero_grad()
        o_map.zero_grad()
        ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"])
        S.total_loss(ret_o, cfg["training"]).backward()
        o_map.step()
        if (it + 1) % 5 == 0:
            o_unc.step()
        ret_h, loss_h = tr.step(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")))
        for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "uncert_loss"):
            H.assert_close(ret_h[k].reshape(-1), ret_o[k].reshape(-1), 1e-5, f"iter{it}.{k}", rel=2e-3)
    # Adam normalises by sqrt(v): an entry whose gradient is at noise level can move by a full +-lr in either
    # implementation, so compare the bulk of the entries, not the max
    def frac_within(a, b, tol):
        return ((a.detach().cpu() - b.detach()).abs() <= tol).float().mean().item()
    assert frac_within(tr.model.decoder.sdf_net.model[0].weight, ora.sdf_w0, 2e-3) > 0.995
    assert frac_within(tr.model.decoder.color_net.model[0].weight, ora.col_w0, 2e-3) > 0.995
    assert frac_within(tr.model.uncert_grid, ora.uncert_grid, 2e-2) > 0.995
    assert frac_within(tr.model.embed_fn.params, ora.table, 2e-3) > 0.995


# --------------------------------------------------------------------------------------------- full-size properties
def test_full_size_properties(gpu):
    """BASELINE.json configs[1] size (2048 rays x 128 samples): size-independent invariants."""
    cfg = H.office_cfg(16, perturb=1.0, n_samples_d=117)
    ora_small = None
    from naruto_amd.field import NarutoFieldHIP
    bbox = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32, device=gpu)
    torch.manual_seed(0)
    m = NarutoFieldHIP(cfg, bbox).to(gpu)
    m.get_uncert_grid(0.1)
    with torch.no_grad():
        m.embed_fn.params.copy_(torch.from_numpy(syn.closed_form_table(m.embed_fn.params.numel(), 0.2)))
    rays = syn.random_rays(2048, cfg["mapping"]["bound"], seed=9)
    t = {k: torch.from_numpy(v).to(gpu) for k, v in rays.items()}
    m.eval()
    with torch.no_grad():
        r1 = m.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=torch.rand(2048, 128, device=gpu, generator=torch.Generator(gpu).manual_seed(1)))
        w = m.raw2outputs(r1["raw"], r1["z_vals"], False)[3]
    acc = w.sum(-1)
    assert bool(((acc - 1).abs() < 1e-4).logical_or(acc.abs() < 1e-4).all()), "weights sum to ~1 (or 0 on empty rays)"
    assert bool((r1["z_vals"][:, 1:] >= r1["z_vals"][:, :-1]).all())
    assert bool((r1["uncert_map"] > 0).all())
    # same points through the x path == through the ray path (two point sources, one field)
    pts = t["rays_o"][:, None, :] + t["rays_d"][:, None, :] * r1["z_vals"][..., None]
    with torch.no_grad():
        raw2 = m.run_network(pts)
    H.assert_close(raw2, r1["raw"], TOL_OUT, "run_network(pts) vs fused ray path")
    # splitting the batch changes nothing (bitwise): tiles are independent
    with torch.no_grad():
        a = m.query_color_sdf(pts.reshape(-1, 3)[:100000])
        b = m.query_color_sdf(pts.reshape(-1, 3)[:50000])
    assert torch.equal(a[:50000], b)
    # gradient conservation: trilinear weights sum to 1 => per level, sum(d_table) == sum over samples of d_feat
    m.train()
    m.zero_grad()
    x = torch.rand(200000, 3, device=gpu)
    e = m.query_sdf(x, embed=True)
    cot = torch.randn_like(e)
    (e * cot).sum().backward()
    tg = m.embed_fn.params.grad.double()
    _, _, _, off = m._handle().levels()
    for l in range(16):
        got = tg[off[l] * 2: off[l + 1] * 2].reshape(-1, 2).sum(0)
        want = cot[:, 2 * l: 2 * l + 2].double().sum(0)
        assert torch.allclose(got, want, rtol=1e-3, atol=1e-2), (l, got, want)


# --------------------------------------------------------------------------------------------- A10: optimiser + graph
def test_fused_adam_matches_torch(gpu):
    from naruto_amd.trainer import FusedAdam
    torch.manual_seed(3)
    p1 = [torch.nn.Parameter(torch.randn(1000, device=gpu)), torch.nn.Parameter(torch.randn(33, 7, device=gpu))]
    p2 = [torch.nn.Parameter(p.detach().clone()) for p in p1]
    groups = lambda ps: [{'params': [ps[0]], 'weight_decay': 1e-6, 'lr': 0.01}, {'params': [ps[1]], 'eps': 1e-15, 'lr': 0.02}]
    o1 = torch.optim.Adam(groups(p1), betas=(0.9, 0.99))
    o2 = FusedAdam(groups(p2), betas=(0.9, 0.99))
    for it in range(7):
        gs = [torch.randn_like(p) * (10.0 ** (-it)) for p in p1]
        for p, q, g in zip(p1, p2, gs):
            p.grad, q.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
    for p, q in zip(p1, p2):
        H.assert_close(q, p, 2e-6, "fused adam", rel=1e-5)


@pytest.mark.parametrize("n_samples_d,n_range_d", [(32, 0), (21, 11)])
def test_reference_workload_config0_on_gpu(gpu, n_samples_d, n_range_d):
    """BASELINE.json configs[0] through the HIP path: office_0, the 64 x 64 pinhole fan, 32 samples per ray (32 uniform +
    no depth-guided ones -- SURVEY 8(d) row 1 -- and the 21 + 11 split), forward + losses + backward against the CPU oracle."""
    cfg = H.office_cfg(16, n_samples_d=n_samples_d, n_range_d=n_range_d)
    rays = syn.pinhole_rays(64, 64, 32.0, 32.0, cfg["mapping"]["bound"])
    ora = H.make_oracle(cfg, 0.2, 3).train()
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"])
    S.total_loss(ret_o, cfg["training"]).backward()
    ret_h = m.forward(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")))
    assert ret_h["rgb"].shape == (4096, 3)
    for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "uncert_loss"):
        H.assert_close(ret_h[k].reshape(-1), ret_o[k].reshape(-1), 1e-6, f"config0.{k}", rel=1e-4)
    H.assert_close(ret_h["rgb"], ret_o["rgb"], TOL_OUT, "config0.rgb")
    H.assert_close(ret_h["depth"], ret_o["depth"], TOL_OUT, "config0.depth")
    S.total_loss(ret_h, cfg["training"]).backward()
    gh, go = H.hip_grads(m), H.ora_grads(ora)
    for k in gh:
        grad_close(gh[k], go[k], f"config0.grad.{k}")
    m.eval()
    with torch.no_grad():
        rend = m.forward(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")))
    ora.eval()
    with torch.no_grad():
        rend_o = ora.render_rays(t["rays_o"], t["rays_d"], target_d=t["target_d"])
    for k in ("raw", "rgb", "depth", "depth_var", "uncert_map", "acc_map"):
        H.assert_close(rend[k], rend_o[k], TOL_OUT, f"config0.render.{k}")


def test_second_backward_over_a_retained_graph(gpu):
    """The reference calls ``loss.backward(retain_graph=True)`` (coslam.py:368): the training node's saved tensors must survive
    a backward and a second backward over the SAME graph must add the same gradients again."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 19)
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    rays = syn.random_rays(130, cfg["mapping"]["bound"], seed=19, zero_depth_frac=0.1)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    ora.train()
    S.total_loss(ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"]), cfg["training"]).backward()
    go = H.ora_grads(ora)
    ret = m.forward(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")))
    loss = S.total_loss(ret, cfg["training"])
    loss.backward(retain_graph=True)
    for k, g in H.hip_grads(m).items():
        grad_close(g, go[k], f"retain.first.{k}")
    loss.backward()                                    # same graph, saved tensors still there: gradients accumulate
    for k, g in H.hip_grads(m).items():
        grad_close(g, 2 * go[k], f"retain.second.{k}")


def test_graph_replay_equals_eager(gpu):
    """The captured hipGraph iteration reproduces the eager iteration (same inputs, same jitter stream is not
    possible -- the graph owns its RNG offsets -- so perturb is off here)."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12, perturb=0.0)
    bound = torch.tensor(cfg["mapping"]["bound"])
    torch.manual_seed(5)
    a = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b.model.load_state_dict(a.model.state_dict())
    b.capture(192, smooth=False)
    for it in range(6):
        rays = syn.random_rays(192, cfg["mapping"]["bound"], seed=200 + it)
        t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        ra, la = a.step(*t)
        rb, lb = b.step(*t)
        H.assert_close(lb.reshape(-1), la.reshape(-1), 1e-6, f"iter{it}.loss", rel=1e-5)
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        H.assert_close(q, p, 1e-6, f"param {n}", rel=1e-5)


def test_capture_mid_training_keeps_the_trajectory(gpu):
    """capture() after some training must not change the training state: parameters, both optimisers' moments and step
    counts, the accumulated uncertainty-grid gradient and the iteration counter are restored after the warm-up / capture
    iterations (a re-capture is needed whenever the ray count changes).  Twin trainers: one runs 8 eager iterations, the other
    3 eager + capture + 5 replayed; an uncertainty-grid step (iteration 5) lies after the capture, fed by gradient
    accumulated before it."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12, perturb=1.0)
    bound = torch.tensor(cfg["mapping"]["bound"])
    torch.manual_seed(21)
    a = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b.model.load_state_dict(a.model.state_dict())
    b.iter_state.copy_(a.iter_state)
    for it in range(8):
        if it == 3:
            b.capture(176, smooth=True)
            assert torch.equal(b.iter_state.cpu(), a.iter_state.cpu())
            for sa, sb in zip(a.map_optimizer.state.values(), b.map_optimizer.state.values()):
                assert torch.equal(sa['exp_avg'], sb['exp_avg']) and torch.equal(sa['exp_avg_sq'], sb['exp_avg_sq'])
            # (the uncertainty grid's gradient goes through the fixed-point scatter as well: bit-identical between the two trainers)
            assert float(a.model.uncert_grid.grad.abs().max()) > 0
            assert torch.equal(b.model.uncert_grid.grad, a.model.uncert_grid.grad), "uncert-grid gradient carried over the capture"
        rays = syn.random_rays(176, cfg["mapping"]["bound"], seed=700 + it, zero_depth_frac=0.1)
        t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        ra, la = a.step(*t, smooth=True)
        rb, lb = b.step(*t, smooth=True)
        H.assert_close(lb.reshape(-1), la.reshape(-1), 1e-7, f"iter{it}.loss", rel=1e-6)
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        H.assert_close(q, p, 5e-6, f"param {n}", rel=1e-5)


def test_reference_loop_shapes_for_the_uncert_grid(gpu):
    """MappingTrainer.first_frame_mapping / global_BA reproduce when the reference steps the uncertainty grid
    (coslam.py:197-217: once, after ALL first-frame iterations, gradient kept; coslam.py:397-399: after iterations 5, 10, ...
    of EACH global_BA call) -- against the oracle driven by the reference's own loop shapes."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.1, 77)
    tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), gpu, fused_adam=True)
    tr.model.load_state_dict(H.make_hip_from_oracle(cfg, ora, gpu).state_dict())
    g1, g2 = ora.param_groups()
    o_map = torch.optim.Adam(g1, betas=(0.9, 0.99))
    o_unc = torch.optim.Adam(g2, lr=1)
    ora.train()

    def batch(seed):
        rays = syn.random_rays(96, cfg["mapping"]["bound"], seed=seed)
        return {k: torch.from_numpy(v) for k, v in rays.items()}

    def ora_iter(t):
        o_map.zero_grad()
        ret = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"])
        S.total_loss(ret, cfg["training"]).backward()
        o_map.step()

    keys = ("rays_o", "rays_d", "target_rgb", "target_d")
    first = [batch(900 + i) for i in range(3)]
    o_unc.zero_grad()
    for t in first:                                   # first_frame_mapping: no uncert step inside the loop
        ora_iter(t)
    o_unc.step()                                      # ... one at the end, gradient NOT zeroed
    tr.first_frame_mapping([[t[k].to(gpu) for k in keys] for t in first])
    H.assert_close(tr.model.uncert_grid.grad, ora.uncert_grid.grad, 1e-6 * float(ora.uncert_grid.grad.abs().max()), "uncert grad after first frame", rel=1e-3)
    for call in range(2):                             # two global_BA calls of 7 iterations: the counter restarts per call
        ba = [batch(950 + 10 * call + i) for i in range(7)]
        for i, t in enumerate(ba):
            ora_iter(t)
            if (i + 1) % 5 == 0:
                o_unc.step()
                o_unc.zero_grad()
        tr.global_BA([[t[k].to(gpu) for k in keys] for t in ba], smooth=False)
    def frac_within(a, b, tol):
        return ((a.detach().cpu() - b.detach()).abs() <= tol).float().mean().item()
    assert frac_within(tr.model.uncert_grid, ora.uncert_grid, 2e-2) > 0.995
    g_o = ora.uncert_grid.grad if ora.uncert_grid.grad is not None else torch.zeros_like(ora.uncert_grid)
    H.assert_close(tr.model.uncert_grid.grad, g_o, 2e-3 * float(g_o.abs().max()) + 1e-12, "uncert grad carried between BA calls", rel=1e-2)


def _dp_worker(rank, world, port, backend, n_rays, steps, out, n_samples_d=None):
    import os
    import torch.distributed as dist
    from naruto_amd import trainer, parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    cfg = H.office_cfg(12, perturb=0.0) if n_samples_d is None else H.office_cfg(12, perturb=0.0, n_samples_d=n_samples_d)   # no depth jitter: the in-kernel numbers are keyed by the LOCAL ray index
    torch.manual_seed(5)
    tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), dev, fused_adam=True, group=dist.group.WORLD)
    losses = []
    for it in range(steps):
        rays = syn.random_rays(n_rays, cfg["mapping"]["bound"], seed=400 + it, zero_depth_frac=0.1)
        t = [torch.from_numpy(rays[k]) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        shard = [a.to(dev) for a in parallel.shard_rays(t, rank, world)]
        ret, loss = tr.step(*shard, smooth=True, n_rays_total=n_rays)
        losses.append(float(loss))
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({"params": {n: p.detach().cpu() for n, p in tr.model.named_parameters()}, "losses": losses}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_samples_d", [None, 117])
def test_two_rank_data_parallel_training(gpu, tmp_path, n_samples_d):
    """(n_samples_d = 117: 128 samples per ray, where a single process runs the five-launch iteration with the smoothness term evaluated in
    the backward -- the data-parallel backward must NOT evaluate it a second time: round-4 advisor finding, the total loss counted it twice.)
    The data-parallel iteration of the PRODUCT path (MappingTrainer with a process group: sharded rays, all-reduce of the loss
    sums between forward and backward, two-phase backward with the MLP-gradient bucket reduced under the table scatter, table
    bucket, identical Adam steps) over two ranks reproduces the single-process trajectory on the whole batch.  With two GPUs
    visible the ranks use one GPU each over RCCL ("nccl"); on a one-GPU box both ranks share the GPU and the collectives go
    through gloo (staged through the host) -- same protocol, same kernels."""
    import socket
    import torch.multiprocessing as mp
    from naruto_amd import trainer
    n_rays, steps = 192, 6                               # 6 iterations: one uncertainty-grid step (its gradient is reduced then)
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "dp_r0.pt")
    mp.spawn(_dp_worker, args=(2, port, backend, n_rays, steps, out, n_samples_d), nprocs=2, join=True)
    got = torch.load(out)
    cfg = H.office_cfg(12, perturb=0.0) if n_samples_d is None else H.office_cfg(12, perturb=0.0, n_samples_d=n_samples_d)
    torch.manual_seed(5)
    ref = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), gpu, fused_adam=True)
    ref.fuse_optimizer = False                            # same kernels as the data-parallel ranks (gradients, then k_adam_multi)
    for it in range(steps):
        rays = syn.random_rays(n_rays, cfg["mapping"]["bound"], seed=400 + it, zero_depth_frac=0.1)
        t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        ret, loss = ref.step(*t, smooth=True)
        assert abs(float(loss) - got["losses"][it]) <= 1e-6 + 1e-5 * abs(float(loss)), f"iteration {it}: loss {got['losses'][it]} vs {float(loss)}"
    # Adam normalises by sqrt(v): an entry whose gradient is at noise level can move by a full +-lr under a different summation
    # order (two shards vs one batch), so compare the bulk of the entries, not the max
    for n, p in ref.model.named_parameters():
        if p.numel() == 0:
            continue
        within = ((got["params"][n] - p.detach().cpu()).abs() <= 1e-4 + 1e-3 * p.detach().cpu().abs()).float().mean().item()
        assert within > 0.995, f"dp param {n} ({backend}): only {within:.4f} of the entries agree"


def test_optimizer_in_backward_equals_separate_adam(gpu):
    """k_bwd_finish (gradient reduction + Adam in one launch, gradients never materialised) walks the same trajectory as
    the backward followed by k_adam_multi, incl. the smoothness term and the uncertainty-grid optimiser."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12, perturb=1.0)
    bound = torch.tensor(cfg["mapping"]["bound"])
    torch.manual_seed(9)
    a = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b.model.load_state_dict(a.model.state_dict())
    b.iter_state.copy_(a.iter_state)                 # same in-kernel random numbers
    a.fuse_optimizer = False
    assert b.fuse_optimizer
    for it in range(6):
        rays = syn.random_rays(160, cfg["mapping"]["bound"], seed=300 + it, zero_depth_frac=0.1)
        t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        ra, la = a.step(*t, smooth=True)
        rb, lb = b.step(*t, smooth=True)
        H.assert_close(lb.reshape(-1), la.reshape(-1), 1e-7, f"iter{it}.loss", rel=1e-6)
    assert next(iter(b._train_steps.values())).opt is not None and next(iter(a._train_steps.values())).opt is None
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        # same formulas in two kernels: fused-multiply-add contraction may differ by an ulp, Adam's normalisation carries that
        # into the parameters at the 1e-6 level over six steps
        H.assert_close(q, p, 5e-6, f"param {n}", rel=1e-5)


def test_train_node_with_fused_smoothness(gpu):
    """The training node with the smoothness term riding along (one scatter pass, written-not-accumulated
    gradients) against the oracle: rendering losses + smooth_weight * TV(hash features)."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 41)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rays = syn.random_rays(160, cfg["mapping"]["bound"], seed=41, zero_depth_frac=0.15)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    r6 = torch.tensor([0.3, 0.6, 0.2, 0.1, 0.7, 0.4])
    w_s = 0.37                                   # a large weight so that the term matters in the comparison
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"])
    sm_o = S.smoothness(ora, 12, 0.1, 0.05, r6[:3], r6[3:])
    (S.total_loss(ret_o, cfg["training"]) + w_s * sm_o).backward()
    m.train()
    ret_h = m.forward(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")), _smooth=(12, 0.1, 0.05, r6.to(gpu)))
    H.assert_close(ret_h["_smooth_loss"], sm_o, 1e-7, "smooth_loss", rel=1e-4)
    (S.total_loss(ret_h, cfg["training"]) + w_s * ret_h["_smooth_loss"]).backward()
    gh, go = H.hip_grads(m), H.ora_grads(ora)
    for k in gh:
        grad_close(gh[k], go[k], f"fused.grad.{k}")
    # a second backward pass into the same .grad accumulates (the node writes fresh tensors, autograd adds them)
    ret_h = m.forward(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")), _smooth=(12, 0.1, 0.05, r6.to(gpu)))
    (S.total_loss(ret_h, cfg["training"]) + w_s * ret_h["_smooth_loss"]).backward()
    for k in gh:
        grad_close(H.hip_grads(m)[k], 2 * go[k], f"fused.grad2.{k}")


@pytest.mark.parametrize("n_samples_d", [32, 117, 181])
def test_train_step_direct_against_oracle(gpu, n_samples_d):
    """naruto_train_forward / naruto_train_backward (the trainer's fast path: role blocks, last-workgroup reductions,
    no autograd) against the oracle, with the smoothness term, zero-depth rays and a given jitter draw; run twice to
    check that the self-resetting tickets and the written-not-accumulated gradients hold up, and that the
    uncertainty-grid gradient accumulates.  n_samples_d = 117 / 181 make S = 128 / 192 = 2 / 3 tiles of 64 samples per
    ray: the forward then walks each ray front to back and stops evaluating once nothing behind can matter (EarlyExit in
    naruto_field.hip) -- losses and gradients must not change, and some rays must actually have stopped early."""
    from naruto_amd import ops
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=n_samples_d)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.25, 43)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    N = 150                                                     # not a multiple of 4: a partly filled ray block
    S_tot = tr["n_samples_d"] + tr["n_range_d"]
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=43, zero_depth_frac=0.15)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    r6 = torch.tensor([0.3, 0.6, 0.2, 0.1, 0.7, 0.4])
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(7))
    w_s = 0.37
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, w_s, 0.0])
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    sm_o = S.smoothness(ora, 12, 0.1, 0.05, r6[:3], r6[3:])
    total_o = S.total_loss(ret_o, tr) + w_s * sm_o
    total_o.backward()
    go = H.ora_grads(ora)
    ug = torch.zeros_like(m.uncert_grid)
    ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"], far=cam["far"],
                       range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True,
                       loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=False)
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    for rep in range(2):
        ts.rand[N * S_tot:].copy_(r6)
        torch.cuda.synchronize()
        # run() with an explicit jitter leaves the six lattice numbers alone
        losses = ts.run(*args, rand=rand.to(gpu))
        torch.cuda.synchronize()
        for i, k in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")):
            H.assert_close(losses[i].reshape(-1), ret_o[k].reshape(-1), 1e-6, f"direct.{k}", rel=1e-4)
        H.assert_close(losses[5].reshape(-1), ret_o["uncert_loss"].reshape(-1), 1e-5, "direct.uncert_loss", rel=1e-4)
        H.assert_close(losses[8].reshape(-1), sm_o.reshape(-1), 1e-7, "direct.smooth", rel=1e-4)
        H.assert_close(losses[9].reshape(-1), total_o.detach().reshape(-1), 1e-5, "direct.total", rel=1e-4)
        H.assert_close(ts.rgb, ret_o["rgb"], 1e-5, "direct.rgb")
        H.assert_close(ts.depth, ret_o["depth"], 1e-5, "direct.depth", rel=1e-5)
        for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
            grad_close(ts.grads[k].reshape(-1), go[k].reshape(-1), f"direct.rep{rep}.grad.{k}")
        grad_close(ug.reshape(-1), (rep + 1) * ora.uncert_grid.grad.reshape(-1), f"direct.rep{rep}.grad.uncert_grid")
    if S_tot % 64 == 0:
        tail = ts.raw[:, 64:, :].reshape(N, -1)
        n_stopped = int((tail.abs().sum(1) == 0).sum().item())
        assert 0 < n_stopped < N, f"early termination: {n_stopped} of {N} rays stopped after the first tile"


def test_train_step_with_large_cotangents(gpu):
    """Loss weights 3e7 times the shipped ones: the feature cotangents of the scatter's list reach the thousands, beyond the range of
    the fp64 magic-number conversion (+-2047 per contribution, a run's sum on the dense levels), so waves take the fp32 split next to
    waves that do not (naruto_field.hip: fix_add_corners, the dense / uncertainty units' flush).  Gradients against the oracle with
    the same weights."""
    from naruto_amd import ops
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=32)
    tr, cam = dict(cfg["training"]), cfg["cam"]
    big = 3e7
    for k in ("rgb_weight", "depth_weight", "sdf_weight", "fs_weight", "uncert_weight"):
        tr[k] = tr[k] * big
    ora = H.make_oracle(cfg, 0.25, 47)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    N, S_tot = 150, tr["n_samples_d"] + tr["n_range_d"]
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=47, zero_depth_frac=0.1)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    r6 = torch.tensor([0.3, 0.6, 0.2, 0.1, 0.7, 0.4])
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(9))
    w_s = 0.37 * big
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, w_s, 0.0])
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    (S.total_loss(ret_o, tr) + w_s * S.smoothness(ora, 12, 0.1, 0.05, r6[:3], r6[3:])).backward()
    go = H.ora_grads(ora)
    assert float(go["table"].abs().max()) > 2047.0            # the sums certainly are out of the magic number's range
    ug = torch.zeros_like(m.uncert_grid)
    ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"], far=cam["far"],
                       range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True,
                       loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=False)
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    ts.rand[N * S_tot:].copy_(r6)
    ts.run(*args, rand=rand.to(gpu))
    torch.cuda.synchronize()
    for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
        grad_close(ts.grads[k].reshape(-1), go[k].reshape(-1), f"large.grad.{k}")
    grad_close(ug.reshape(-1), ora.uncert_grid.grad.reshape(-1), "large.grad.uncert_grid")


@pytest.mark.parametrize("workload", ["office0_2048x128", "office0_4100x128", "office0_8192x43", "mp3d_2048x256", "unit1024_T22_16384x43"])
def test_train_step_full_size_against_oracle(gpu, workload):
    """BASELINE.json's configurations at their full per-GPU sizes -- configs[1] 2048 rays x 128 samples, configs[2] 8192
    rays with the shipped sampling, configs[3]'s per-GPU shard 2048 rays x 256 samples on the MP3D volume; 2^16-entry
    tables, smoothness term, the trainer's fast path (early termination, active-sample compaction, LDS-tiled scatter over
    all CUs) -- against the CPU oracle on the same jitter draw: every loss, the rendered maps and every gradient.  4 100 rays x 128
    samples: more ray groups than the forward has workgroups (a workgroup walks two groups with the loss stage riding along), a
    partly filled last group, and beyond the 4 096 rays up to which the loss tail and the compaction ride in the backward's first
    launch (so the ordinary tail / compaction launches with the two-level prefix run).  unit1024_T22_16384x43: BASELINE configs[4]'s
    volume and table (unit cube, finest level 1024^3, T = 2^22: 281 MB, HBM resident, counting-sort scatter) at 16 384 rays x 43."""
    from naruto_amd import ops
    from naruto_amd import config as C
    depth_range = (0.5, 2.5)
    if workload == "unit1024_T22_16384x43":
        cfg, N, depth_range = C.unit_cube_config(1024, 22, perturb=1.0), 16384, (0.15, 0.7)
    elif workload == "office0_2048x128":
        cfg, N = H.office_cfg(16, perturb=1.0, n_samples_d=117), 2048
    elif workload == "office0_4100x128":
        cfg, N = H.office_cfg(16, perturb=1.0, n_samples_d=117), 4100
    elif workload == "office0_8192x43":
        cfg, N = H.office_cfg(16, perturb=1.0), 8192
    else:
        cfg, N = C.mp3d_large_config(perturb=1.0, n_samples_d=245), 2048
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.05, 77)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    S_tot = tr["n_samples_d"] + tr["n_range_d"]
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=77, zero_depth_frac=0.05, depth_range=depth_range)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    r6 = torch.tensor([0.15, 0.8, 0.45, 0.6, 0.05, 0.9])
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(11))
    w_s = 0.05
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, w_s, 0.0])
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
    sm_o = S.smoothness(ora, tr["smooth_pts"], tr["smooth_vox"], tr["smooth_margin"], r6[:3], r6[3:])
    total_o = S.total_loss(ret_o, tr) + w_s * sm_o
    total_o.backward()
    go = H.ora_grads(ora)
    ug = torch.zeros_like(m.uncert_grid)
    ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"], far=cam["far"],
                       range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True,
                       loss_weights=w.to(gpu), smooth=(tr["smooth_pts"], tr["smooth_vox"], tr["smooth_margin"]), device_rng=False)
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    ts.rand[N * S_tot:].copy_(r6)
    losses = ts.run(*args, rand=rand.to(gpu))
    torch.cuda.synchronize()
    for i, k in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")):
        H.assert_close(losses[i].reshape(-1), ret_o[k].reshape(-1), 1e-6, f"full.{k}", rel=1e-4)
    H.assert_close(losses[5].reshape(-1), ret_o["uncert_loss"].reshape(-1), 1e-5, "full.uncert_loss", rel=1e-4)
    H.assert_close(losses[8].reshape(-1), sm_o.reshape(-1), 1e-7, "full.smooth", rel=1e-4)
    H.assert_close(losses[9].reshape(-1), total_o.detach().reshape(-1), 1e-5, "full.total", rel=1e-4)
    H.assert_close(ts.rgb, ret_o["rgb"], TOL_OUT, "full.rgb")
    H.assert_close(ts.depth, ret_o["depth"], TOL_OUT, "full.depth", rel=1e-4)
    # Gradient entries are sums over up to 10^5 samples with heavy cancellation, so at these sizes the small-batch bound of 1e-4 of
    # max|grad| can lie below the fp32 reference's OWN arithmetic noise.  That noise is measured here, not assumed: the same
    # oracle is evaluated once more in fp64 (same inputs, same jitter draw), noise_k = max|grad32_k - grad64_k|, and the HIP
    # gradient has to be as close to the fp64 result as max(1e-4 of the scale, the fp32 oracle's own deviation from it).
    # (Measured, 8192 x 43: the fp32 oracle deviates from fp64 by 4.2e-3 of max|grad| on the table and 9.0e-4 on col_w0.)
    import copy
    o64 = copy.deepcopy(ora).double()
    for p_ in o64.parameters():
        p_.grad = None
    ret64 = o64.forward(*(t[k].double() for k in ("rays_o", "rays_d", "target_rgb", "target_d")), rand=rand.double())
    sm64 = S.smoothness(o64, tr["smooth_pts"], tr["smooth_vox"], tr["smooth_margin"], r6[:3].double(), r6[3:].double())
    (S.total_loss(ret64, tr) + w_s * sm64).backward()
    g64 = H.ora_grads(o64)
    budget = {}
    for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1", "uncert_grid"):
        scale = float(g64[k].abs().max())
        noise = float((go[k].double() - g64[k]).abs().max())
        budget[k] = max(1e-4 * scale, 1.25 * noise)
        got = (ug if k == "uncert_grid" else ts.grads[k]).reshape(-1).double().cpu()
        err64 = (got - g64[k].reshape(-1)).abs()
        assert float(err64.max()) <= budget[k], (f"full.grad.{k}: {float(err64.max()):.3e} from the fp64 result; the fp32 oracle itself is "
                                                 f"{noise:.3e} away (scale {scale:.3e})")
        # and against the fp32 oracle: both sit within the budget of the fp64 result
        H.assert_close(got, go[k].reshape(-1), 2.0 * budget[k], f"full.grad.{k} vs fp32 oracle", rel=1e-3)
        if k == "table":
            # how many entries lie beyond 1e-4 of the scale: no more than for the fp32 oracle itself (x 1.5), or 1e-4 of the table
            frac_h = float((err64 > 1e-4 * scale).float().mean())
            frac_o = float(((go[k].reshape(-1).double() - g64[k].reshape(-1)).abs() > 1e-4 * scale).float().mean())
            assert frac_h <= max(1e-4, 1.5 * frac_o), f"full.grad.table: {frac_h:.2e} of the entries beyond 1e-4 of the scale (fp32 oracle: {frac_o:.2e})"
    if S_tot % 64 == 0 and S_tot > 64:
        n_stopped = int((ts.raw[:, 64:, :].reshape(N, -1).abs().sum(1) == 0).sum().item())
        assert 0 < n_stopped < N, f"early termination: {n_stopped} of {N} rays stopped after the first tile"


_relu_kink_distance = H.relu_kink_distance


@pytest.mark.parametrize("case", list(range(24)))
def test_train_step_random_shapes(gpu, case):
    """The trainer's fast path against the oracle over odd batch shapes: ray counts around the 4-rays-per-workgroup and
    64-sample-tile boundaries (1, 3, 5, 63 .. 257), sample counts that make S = 64 (one tile, flat mode), 128 / 192 (ray mode)
    or nothing in particular, 0 / 1 / 5 / 11 / 21 samples around the depth, jitter on / off, many or no depth-less rays.  (A draw in
    which a small batch has a hidden unit of an active sample within 2e-6 of the ReLU kink is re-drawn: there the gradient is decided by
    fp32 rounding -- one such sample moved 12 % of a sdf_w0 row in a single-ray batch, in the oracle's fp32 as well.)"""
    from naruto_amd import ops
    for attempt in range(8):
        rs = np.random.RandomState(1000 + case + 100 * attempt)
        N = int(rs.choice([1, 3, 5, 63, 64, 65, 130, 257]))
        n_range = int(rs.choice([0, 1, 5, 11, 21]))
        S_tot = int(rs.choice([43, 64, 100, 128, 192]))
        n_d = S_tot - n_range
        perturb = bool(case % 2)
        cfg = H.office_cfg(12, perturb=1.0 if perturb else 0.0, n_samples_d=n_d, n_range_d=n_range)
        tr, cam = cfg["training"], cfg["cam"]
        seed = 90 + case + 100 * attempt
        ora = H.make_oracle(cfg, 0.25, seed)
        m = H.make_hip_from_oracle(cfg, ora, gpu)
        rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=seed, zero_depth_frac=float(rs.choice([0.0, 0.2, 0.6])))
        t = {k: torch.from_numpy(v) for k, v in rays.items()}
        r6 = torch.from_numpy(rs.uniform(0, 1, 6).astype(np.float32))
        rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(seed))
        w_s = 0.11
        w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, w_s, 0.0])
        ug = torch.zeros_like(m.uncert_grid)
        ts = ops.TrainStep(m._handle(), m._params(), ug, N, n_samples_d=n_d, n_range_d=n_range, near=cam["near"], far=cam["far"],
                           range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=perturb,
                           loss_weights=w.to(gpu), smooth=(8, 0.1, 0.05), device_rng=False)
        args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
        ts.rand[N * S_tot:].copy_(r6)
        losses = ts.run(*args, rand=rand.to(gpu))          # an explicit draw (unused without perturb) keeps the six lattice numbers
        torch.cuda.synchronize()
        active = (ts.d_raw.abs().sum(-1) > 0).cpu()
        if not bool((t["target_d"] > 0).any()):
            continue              # no ray with a depth: the reference's depth loss is a mean over nothing (NaN everywhere)
        # a small batch is re-drawn until no active sample sits on a kink; a large one always has a few (expected: 1e-5 per
        # unit and sample): each may move the 128 table entries of its corners and one row of sdf_w0 / col_w0
        kink_dist, n_kink = _relu_kink_distance(ora, cfg, t["rays_o"], t["rays_d"], ts.z_vals.cpu(), active)
        if n_kink == 0 or int(active.sum()) > 2000:
            break
    else:
        pytest.skip("no draw without a ReLU-kink sample in 8 attempts")
    ora.train()
    ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand if perturb else None)
    sm_o = S.smoothness(ora, 8, 0.1, 0.05, r6[:3], r6[3:])
    total_o = S.total_loss(ret_o, tr) + w_s * sm_o
    total_o.backward()
    go = H.ora_grads(ora)
    what = f"N={N} S={n_d}+{n_range} perturb={perturb} (attempt {attempt})"
    for i, k in enumerate(("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")):
        H.assert_close(losses[i].reshape(-1), ret_o[k].reshape(-1), 1e-6, f"{what}: {k}", rel=1e-4)
    H.assert_close(losses[5].reshape(-1), ret_o["uncert_loss"].reshape(-1), 1e-5, f"{what}: uncert_loss", rel=1e-4)
    H.assert_close(losses[9].reshape(-1), total_o.detach().reshape(-1), 1e-5, f"{what}: total", rel=1e-4)
    H.assert_close(ts.rgb, ret_o["rgb"], 1e-5, f"{what}: rgb")
    H.assert_close(ts.depth, ret_o["depth"], 1e-5, f"{what}: depth", rel=1e-5)
    budget = {"table": 128 * n_kink, "sdf_w0": 80 * n_kink, "col_w0": 63 * n_kink, "sdf_w1": 0, "col_w1": 0}
    for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
        got, want = ts.grads[k].reshape(-1).double().cpu(), go[k].reshape(-1).double()
        scale = max(float(want.abs().max()), 1e-12)
        bad = (got - want).abs() > 1e-4 * scale + 1e-3 * want.abs()
        assert int(bad.sum()) <= budget[k], (f"{what}: grad.{k}: {int(bad.sum())} entries beyond tolerance (allowed {budget[k]} for {n_kink} samples on a "
                                             f"ReLU kink), max err {float((got - want).abs().max()):.3e}, scale {scale:.3e}")
    grad_close(ug.reshape(-1), ora.uncert_grid.grad.reshape(-1), f"{what}: grad.uncert_grid")


def test_ray_sharding_is_exact_at_full_size(gpu):
    """BASELINE.json configs[4]'s per-GPU size (2^20 rays / 8 GPUs = 131 072 rays x 43 samples, unit cube with a 1024^3 finest
    level): the data-parallel protocol on one GPU.  Two shards of the batch, each run as a rank would run it (forward to the
    loss sums, sums added, finalize, backward with the smoothness gradient scaled by 1/world), reproduce the single-process
    iteration: identical losses, gradients that add up.  A checksum of checksums at a size the oracle cannot reach."""
    from naruto_amd import ops
    from naruto_amd import config as C
    from naruto_amd.field import NarutoFieldHIP
    cfg = C.unit_cube_config(1024, 16, perturb=1.0)
    tr, cam = cfg["training"], cfg["cam"]
    N, S_tot = 131072, tr["n_samples_d"] + tr["n_range_d"]
    bbox = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32, device=gpu)
    torch.manual_seed(3)
    m = NarutoFieldHIP(cfg, bbox).to(gpu)
    m.get_uncert_grid(0.1)
    with torch.no_grad():
        m.embed_fn.params.copy_(torch.from_numpy(syn.closed_form_table(m.embed_fn.params.numel(), 0.05)))
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=21, zero_depth_frac=0.05)
    args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]
    rand = torch.rand(N, S_tot, device=gpu, generator=torch.Generator(gpu).manual_seed(5))
    r6 = torch.tensor([0.15, 0.8, 0.45, 0.6, 0.05, 0.9], device=gpu)
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.05, 0.0], device=gpu)

    def make(n):
        ug = torch.zeros_like(m.uncert_grid)
        ts = ops.TrainStep(m._handle(), m._params(), ug, n, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"], near=cam["near"], far=cam["far"],
                           range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"], perturb=True, loss_weights=w,
                           smooth=(tr["smooth_pts"], tr["smooth_vox"], tr["smooth_margin"]), device_rng=False)
        ts.rand[n * S_tot:].copy_(r6)
        return ts, ug

    full, ug_full = make(N)
    losses_full = full.run(*args, rand=rand).clone()
    g_full = {k: v.clone() for k, v in full.grads.items()}
    assert torch.isfinite(losses_full).all()
    half = N // 2
    shards = []
    for r in range(2):
        ts, ug = make(half)
        ts.group = "two ranks, emulated"              # run_forward stops at the sums, run_backward finalises from them
        ts.t.n_rays_total = N
        ts.t.smooth_grad_scale = 0.5
        sl = slice(r * half, (r + 1) * half)
        ts.run_forward(*(a[sl].contiguous() for a in args), rand[sl].contiguous())
        shards.append((ts, ug))
    total = shards[0][0].sums[:9] + shards[1][0].sums[:9]           # what the all-reduce of the nine additive slots leaves on every rank
    for ts, _ in shards:
        ts.sums[:9].copy_(total)
        ts.run_backward()
    torch.cuda.synchronize()
    for ts, _ in shards:
        for i in (0, 1, 2, 3, 5, 8, 9):
            H.assert_close(ts.losses[i].reshape(-1), losses_full[i].reshape(-1), 1e-6, f"shard.loss[{i}]", rel=1e-5)
    for k in ("table", "sdf_w0", "sdf_w1", "col_w0", "col_w1"):
        got = shards[0][0].grads[k].double() + shards[1][0].grads[k].double()
        grad_close(got.reshape(-1), g_full[k].reshape(-1), f"shard.grad.{k}", frac=1e-5)
    grad_close((shards[0][1].double() + shards[1][1].double()).reshape(-1), ug_full.reshape(-1), "shard.grad.uncert_grid", frac=1e-5)


def test_train_step_device_rng(gpu):
    """With device_rng the kernels draw the depth jitter and the lattice placement themselves (splitmix64 keyed by seed,
    iteration counter, index): z_vals and the lattice points equal the oracle's for exactly those numbers, and the
    counter advances once per forward."""
    from naruto_amd import ops
    cfg = H.office_cfg(12, perturb=1.0)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.25, 47)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    N, S_tot, seed = 96, tr["n_samples_d"] + tr["n_range_d"], 0x1234567
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=47, zero_depth_frac=0.1)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.1, 0.0])
    ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                       near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                       perturb=True, loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=True, seed=seed)
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    ora.train()
    for it in range(2):
        losses = ts.run(*args).clone()
        torch.cuda.synchronize()
        assert ts.rng_state.cpu().tolist() == [seed, it + 1]
        rand = torch.from_numpy(H.device_rng_uniform(seed, it, range(N * S_tot))).view(N, S_tot)
        assert rand.min() >= 0.0 and rand.max() < 1.0 and abs(rand.mean().item() - 0.5) < 0.02
        r6 = torch.from_numpy(H.device_rng_uniform(seed, it, [(1 << 40) + i for i in range(6)]))
        ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], rand=rand)
        H.assert_close(ts.z_vals, ret_o["z_vals"] if "z_vals" in ret_o else ora.render_rays(t["rays_o"], t["rays_d"], target_d=t["target_d"],
                       rand=rand)["z_vals"], 2e-6, f"iter{it}.z_vals", rel=2e-6)
        sm_o = S.smoothness(ora, 12, 0.1, 0.05, r6[:3], r6[3:])
        H.assert_close(losses[8].reshape(-1), sm_o.reshape(-1), 1e-7, f"iter{it}.smooth", rel=1e-4)
        H.assert_close(losses[0].reshape(-1), ret_o["rgb_loss"].reshape(-1), 1e-6, f"iter{it}.rgb_loss", rel=1e-4)


@pytest.mark.parametrize("n_rays,s_d,s_r", [(96, 32, 11), (401, 96, 32), (4096, 11, 5)])
def test_train_step_with_the_tail_in_the_backward(gpu, n_rays, s_d, s_r):
    """TrainStep.run() issues forward and backward back to back, so the loss tail and the compaction ride in the backward's first
    launch (NARUTO_TRAIN_FWD_DEFER_TAIL / NARUTO_TRAIN_BWD_DEFERRED_TAIL).  Against the ordinary sequence (fuse_tail = False):
    the same losses bit for bit (both reduce the loss stage's rows in one order); ray lists that cover the exact ones (the fused
    launch takes each ray's length from the forward's masks, the ordinary one from the cotangents themselves: never shorter, and
    equal unless a product underflows); the same gradients (bit for bit where the lists agree)."""
    from naruto_amd import ops
    cfg = H.office_cfg(12, perturb=1.0)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.25, 31)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rays = syn.random_rays(n_rays, cfg["mapping"]["bound"], seed=131, zero_depth_frac=0.1)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.1, 0.0])
    args = [t[k].to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [t["target_d"].to(gpu).reshape(-1).contiguous()]
    out = []
    for fuse in (False, True):
        ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), n_rays, n_samples_d=s_d, n_range_d=s_r,
                           near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                           perturb=True, loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=True, seed=77)
        ts.fuse_tail = fuse
        for _ in range(2):                        # second iteration: the iteration counter advanced through the fused launch as well
            losses = ts.run(*args).clone()
        torch.cuda.synchronize()
        assert ts.rng_state.cpu().tolist() == [77, 2]
        out.append((losses.cpu(), ts.ray_count.cpu().clone(), int(ts.n_active.cpu()), {k: v.detach().cpu().clone() for k, v in ts.grads.items()},
                    ts.sums.cpu().clone(), ts.ray_offset.cpu().clone()))
    (l0, c0, n0, g0, s0, o0), (l1, c1, n1, g1, s1, o1) = out
    assert torch.equal(l0, l1) and torch.equal(s0[:10], s1[:10]), (l0, l1)
    assert bool((c1 >= c0).all()) and n1 >= n0 and n1 == int(c1.sum())
    assert torch.equal(o1, torch.cumsum(c1.long(), 0).sub(c1.long()).to(o1.dtype))
    assert float((c1 != c0).float().mean()) < 0.02, "the forward's masks predict the last non-zero cotangent"
    same = bool((c1 == c0).all())
    for k in g0:
        if same:
            assert torch.equal(g0[k], g1[k]), k
        else:
            grad_close(g1[k].reshape(-1).double(), g0[k].reshape(-1).double(), f"fused-tail.grad.{k}", frac=1e-6)


_KNOB_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import helpers as H
from naruto_amd import ops, synthetic as syn
gpu = torch.device("cuda", 0)
cfg = H.office_cfg(12, perturb=1.0, n_samples_d=117)                 # 117 + 11 = 128 samples: the forward walks one ray per wave
tr, cam = cfg["training"], cfg["cam"]
ora = H.make_oracle(cfg, 0.25, 19)
m = H.make_hip_from_oracle(cfg, ora, gpu)
N = 333
rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=19, zero_depth_frac=0.1)
w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.1, 0.0])
ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                   near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                   perturb=True, loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=True, seed=5)
args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]
for _ in range(2):
    losses = ts.run(*args).clone()
torch.cuda.synchronize()
out = {"losses": losses.cpu().numpy(), "rgb": ts.rgb.cpu().numpy(), "depth": ts.depth.cpu().numpy(), "sums": ts.sums.cpu().numpy()[:10]}
out.update({"g_" + k: v.detach().cpu().numpy() for k, v in ts.grads.items()})
np.savez(sys.argv[2], **out)
"""


def test_launch_variants_give_the_same_bits(gpu, tmp_path):
    """The launch-structure choices of the training path are claimed to change no bit of any result: the loss stage inside the field
    query's launch vs its own launch, the loss tail + compaction inside the backward's first launch vs three launches, the scatter's
    workgroup order and (fixed-point sums) its point splits.  Each knob is an environment variable read once per process, so the same
    iteration runs in fresh interpreters and the saved losses, rendered maps, sums and gradients are compared bit for bit."""
    import subprocess, sys
    script = tmp_path / "iteration.py"
    script.write_text(_KNOB_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    results = {}
    variants = {"default": {}, "no_fused_loss_stage": {"NARUTO_DEBUG_NO_FUSED_LOSS_STAGE": "1"}, "no_fused_tail": {"NARUTO_DEBUG_NO_FUSED_TAIL": "1"},
                "natural_order": {"NARUTO_DEBUG_SCATTER_XCD_AWARE": "0"}, "no_early_exit": {"NARUTO_DEBUG_NO_EARLY_EXIT": "1"},
                "six_launches": {"NARUTO_TV_MOVE": "0"}}        # default: the walk samples its own depths and encodes the lattice, the term is evaluated in the backward's first launch
    for name, env in variants.items():
        out = tmp_path / f"{name}.npz"
        e = dict(os.environ)
        e.update(env)
        subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=600)
        results[name] = dict(np.load(out))
    ref = results["default"]
    for name, r in results.items():
        for k, v in ref.items():
            assert np.array_equal(v, r[k], equal_nan=True), f"{name}: {k} differs from the default launch structure"
    # the scatter's point splits repartition fixed-point sums: the table gradient keeps its bits; the dense levels pre-sum runs of 8
    # points in fp32 per thread, and a split boundary moves with the split count, so they are compared to the accumulation noise
    out = tmp_path / "splits_x4.npz"
    e = dict(os.environ)
    e["NARUTO_DEBUG_SCATTER_SPLIT_MULT"] = "4"
    subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=600)
    r = dict(np.load(out))
    for k, v in ref.items():
        if k == "g_table":
            d = np.abs(v - r[k])
            assert float(d.max()) <= 1e-6 * float(np.abs(v).max()), f"split multiplier: table gradient moved by {d.max():.3e}"
            assert float((d > 0).mean()) < 0.2
        else:
            assert np.array_equal(v, r[k], equal_nan=True), f"split multiplier: {k} differs"


def test_binned_scatter_round_size_changes_no_bit(gpu, tmp_path):
    """Levels of more than 2^17 entries go through the counting-sort scatter (naruto_binned.hip): 1 024-point sorting rounds, or 512-point
    ones where a level has more than 1 024 bins (T = 2^24) -- forced here by NARUTO_DEBUG_BIN_ROUND=512 on a T = 2^18 field.  The sums are
    fixed point, so how the items are cut into rounds and runs must not change a bit of any gradient."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "iteration_T18.py"
    script.write_text(_KNOB_SCRIPT.replace("H.office_cfg(12,", "H.office_cfg(18,"))
    res = []
    for k, env in enumerate(({}, {"NARUTO_DEBUG_BIN_ROUND": "512"})):
        out = tmp_path / f"T18_{k}.npz"
        e = dict(os.environ)
        e.update(env)
        subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=900)
        res.append(dict(np.load(out)))
    a, b = res
    assert float(np.abs(a["g_table"]).max()) > 0
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{k} differs between 1 024- and 512-point rounds"


def test_packed_forward_equals_the_flat_one(gpu, tmp_path):
    """The shipped 32 + 11 sampling goes through k_query_fwd_loss_packed (only the samples a consumer can see, packed across rays, loss stage
    from LDS) when its rows fall evenly on the workgroups (NARUTO_FWD_PACKED=3: whatever the row count); NARUTO_FWD_PACKED=0 runs the flat
    field query over every sample + k_loss_stage instead.  Same losses, rendered maps, sums and
    gradients -- not bit for bit: a point's OneBlob takes the closed form or the dense one depending on the tile it shares (both forms of
    the same function, 1.2e-6 apart), so the comparison is at that distance.  NARUTO_FWD_PACKED=2 (the packed kernel for S = 128 too)
    against the depth-ordered walk likewise; a three-ray batch (fewer rays than a loss row), and a batch of several chunks per workgroup
    with every sample in one pass (NARUTO_PACK_ONE_PASS)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tag, n_samples_d, n_rays, env_a, env_b in (("43", 32, 333, {"NARUTO_FWD_PACKED": "3"}, {"NARUTO_FWD_PACKED": "0"}),
                                                   ("43_three_rays", 32, 3, {"NARUTO_FWD_PACKED": "3"}, {"NARUTO_FWD_PACKED": "0"}),
                                                   ("43_one_pass", 32, 4100, {"NARUTO_FWD_PACKED": "3", "NARUTO_PACK_ONE_PASS": "1"}, {"NARUTO_FWD_PACKED": "0"}),
                                                   ("128", 117, 333, {"NARUTO_FWD_PACKED": "2"}, {"NARUTO_FWD_PACKED": "0"})):
        script = tmp_path / f"iteration_{tag}.py"
        script.write_text(_KNOB_SCRIPT.replace("n_samples_d=117", f"n_samples_d={n_samples_d}").replace("N = 333", f"N = {n_rays}"))
        res = []
        for k, env in enumerate((env_a, env_b)):
            out = tmp_path / f"{tag}_{k}.npz"
            e = dict(os.environ)
            e.update(env)
            subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=600)
            res.append(dict(np.load(out)))
        a, b = res
        for k in a:
            scale = float(np.abs(b[k]).max()) + 1e-30
            d = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
            assert d <= 2e-5 * scale, f"S = {tag}: {k} differs by {d:.3e} at scale {scale:.3e}"


def test_backward_refuses_a_forward_that_left_the_smoothness_term_unannounced(gpu):
    """(advisor, round 5) NARUTO_TRAIN_FWD_SUMS_TV_LATER leaves the smoothness term to the backward; a backward on the same workspace with
    NARUTO_TRAIN_BWD_SUMS_GIVEN but without NARUTO_TRAIN_BWD_TV_MOVED would drop the term silently -- it is refused; with the flag it runs; an
    ordinary forward afterwards clears the record."""
    import ctypes as CT
    from naruto_amd import _lib, ops
    cfg = H.office_cfg(12, perturb=1.0, n_samples_d=117)
    tr, cam = cfg["training"], cfg["cam"]
    ora = H.make_oracle(cfg, 0.25, 19)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    N = 64
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=19)
    w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.1, 0.0])
    step = lambda: ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                                 near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                                 perturb=True, loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=True, seed=5)
    ts = step()
    args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]
    ts.run(*args)                                           # fills the step's pointers; an ordinary iteration
    lib = _lib.load()
    t = ts.t
    st = ops._stream()
    fwd = lambda fin: lib.naruto_train_forward(ts.handle.ptr, CT.byref(ts.ps), CT.byref(t), fin, st)
    bwd = lambda fl: lib.naruto_train_backward(ts.handle.ptr, CT.byref(ts.ps), CT.byref(t), CT.byref(ts.gs), ts.flags | fl, None, st)
    if os.environ.get("NARUTO_FWD_SORTED") == "2" or os.environ.get("NARUTO_TV_MOVE") == "0":
        pytest.skip("this launch plan never leaves the smoothness term to the backward")
    assert fwd(_lib.TRAIN_FWD_SUMS_TV_LATER) == 0
    rc = bwd(_lib.TRAIN_BWD_SUMS_GIVEN)
    assert rc != 0 and b"NARUTO_TRAIN_BWD_TV_MOVED" in lib.naruto_last_error()
    assert bwd(_lib.TRAIN_BWD_SUMS_GIVEN | _lib.TRAIN_BWD_TV_MOVED) == 0
    assert fwd(0) == 0 and bwd(_lib.TRAIN_BWD_SUMS_GIVEN) == 0          # a forward that evaluated the term itself: nothing to announce
    # the record outlives any number of other workspaces' iterations in between (a ring of 16 records once forgot it here)
    assert fwd(_lib.TRAIN_FWD_SUMS_TV_LATER) == 0
    others = [step() for _ in range(17)]                    # all alive at once: seventeen further workspace addresses
    for o in others:
        o.run(*args)
    rc = bwd(_lib.TRAIN_BWD_SUMS_GIVEN)
    assert rc != 0 and b"NARUTO_TRAIN_BWD_TV_MOVED" in lib.naruto_last_error()
    assert bwd(_lib.TRAIN_BWD_SUMS_GIVEN | _lib.TRAIN_BWD_TV_MOVED) == 0
    assert fwd(0) == 0 and bwd(_lib.TRAIN_BWD_SUMS_GIVEN) == 0
    torch.cuda.synchronize()


def test_sorted_forward_equals_the_flat_one(gpu, tmp_path):
    """Round 6: the Morton-ordered training forward of the tables no cache holds (naruto_sorted.hip: the samples needed whatever the network says, counting-
    sorted by the cell of their position, evaluated in that order; the rest of each ray's band in a second pass; feat_save sample-major, read by the
    backward through its row multiplier) -- forced onto a small table by NARUTO_FWD_SORTED=2 and compared with the flat field query over every sample
    (NARUTO_FWD_SORTED=0, NARUTO_FWD_PACKED=0): same losses, rendered maps, sums and every gradient, at the distance between OneBlob's closed and dense
    forms (the flat launch picks the form per tile, the sorted one per sample -- its tiles are composed by the counting sort's atomics, and a sample's
    bits must not depend on its neighbours: with NARUTO_FWD_SORTED=2 the whole GPU suite's graph-vs-eager and twin tests pass bit for bit).  43 and 128
    samples per ray, a batch smaller than a tile, one of several thousand rays; both MLP modes; and the same sorted iteration twice: same bits."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tag, n_samples_d, n_rays, bf in (("43", 32, 333, False), ("43_one_ray", 32, 1, False), ("43_many", 32, 4100, False), ("128", 117, 333, False), ("43_bf16", 32, 333, True)):
        script = tmp_path / f"iteration_sorted_{tag}.py"
        text = _KNOB_SCRIPT.replace("n_samples_d=117", f"n_samples_d={n_samples_d}").replace("N = 333", f"N = {n_rays}")
        if bf:
            text = text.replace('tr, cam = cfg["training"], cfg["cam"]', 'cfg["decoder"]["mlp_precision"] = "bf16"\ntr, cam = cfg["training"], cfg["cam"]')
        script.write_text(text)
        res = []
        for k, env in enumerate(({"NARUTO_FWD_SORTED": "2"}, {"NARUTO_FWD_SORTED": "0", "NARUTO_FWD_PACKED": "0"})):
            out = tmp_path / f"sorted_{tag}_{k}.npz"
            e = dict(os.environ)
            e.update(env)
            subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=600)
            res.append(dict(np.load(out)))
        a, b = res
        assert float(np.abs(b["g_table"]).max()) > 0
        for k in a:
            scale = float(np.abs(b[k]).max()) + 1e-30
            d = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
            assert d <= 2e-5 * scale, f"S = {tag}: {k} differs by {d:.3e} at scale {scale:.3e}"
        if tag == "43_many":               # run-to-run: the order inside a cell is the atomics', the bits are not
            out = tmp_path / f"sorted_{tag}_again.npz"
            e = dict(os.environ)
            e["NARUTO_FWD_SORTED"] = "2"
            subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=600)
            c = dict(np.load(out))
            for k in a:
                assert np.array_equal(a[k], c[k], equal_nan=True), f"sorted forward, second run: {k} differs"


_FULL_T22_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import bench
from naruto_amd import ops
from naruto_amd.field import NarutoFieldHIP
gpu = torch.device("cuda", 0)
cfg, N = bench.workload("unit1024_T22_131072x43")
tr, cam = cfg["training"], cfg["cam"]
torch.manual_seed(3)
m = NarutoFieldHIP(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32)).to(gpu)
m.get_uncert_grid(0.1)
with torch.no_grad():
    m.embed_fn.params.uniform_(-0.3, 0.3)           # a field with structure: sign changes on most rays
rays = bench.bench_rays(cfg, N)
w = torch.tensor([tr["rgb_weight"], tr["depth_weight"], tr["sdf_weight"], tr["fs_weight"], 0.0, tr["uncert_weight"], 0.0, 0.0, 0.1, 0.0])
ts = ops.TrainStep(m._handle(), m._params(), torch.zeros_like(m.uncert_grid), N, n_samples_d=tr["n_samples_d"], n_range_d=tr["n_range_d"],
                   near=cam["near"], far=cam["far"], range_d=tr["range_d"], depth_trunc=cam["depth_trunc"], rgb_missing=tr["rgb_missing"],
                   perturb=True, loss_weights=w.to(gpu), smooth=(12, 0.1, 0.05), device_rng=True, seed=5)
args = [torch.from_numpy(rays[k]).to(gpu).contiguous() for k in ("rays_o", "rays_d", "target_rgb")] + [torch.from_numpy(rays["target_d"]).to(gpu).reshape(-1).contiguous()]
losses = ts.run(*args).clone()
torch.cuda.synchronize()
S = tr["n_samples_d"] + tr["n_range_d"]
raw = ts.raw.reshape(N, S, 5)
z = ts.z_vals.reshape(N, S)
ev = raw.abs().sum(-1) > 0
# size-independent properties of ANY correct forward of this path: what is evaluated is a PREFIX of every ray (depths are sorted), it reaches at least
# to measured depth + truncation, and nothing is evaluated behind max(first sign change, measured depth) + truncation + one sample
first_gap = (~ev).float().argmax(1)
n_ev = ev.sum(1)
prefix_ok = bool(((n_ev == first_gap) | (n_ev == S)).all())
td = args[3].reshape(-1, 1)
tsc = float(cfg["training"]["trunc"])
need = (~(td > 0)) | (z <= td + tsc)
covers = bool((ev | ~need).all())
g = ts.grads["table"]
idx = torch.arange(0, g.numel(), 9973, device=gpu)
out = {"losses": losses.cpu().numpy(), "rgb": ts.rgb.cpu().numpy(), "depth": ts.depth.cpu().numpy(), "sums": ts.sums.cpu().numpy()[:10],
       "g_table_probe": g.reshape(-1)[idx].cpu().numpy(), "g_table_abs_sum": np.array([float(g.double().abs().sum())]),
       "g_sdf_w0": ts.grads["sdf_w0"].cpu().numpy(), "g_col_w1": ts.grads["col_w1"].cpu().numpy(), "g_uncert_grid": ts.grads["uncert_grid"].cpu().numpy(),
       "n_eval": np.array([int(ev.sum())]), "n_active": np.array([int(ts.n_active.item())]), "prefix_ok": np.array([prefix_ok]), "covers": np.array([covers])}
np.savez(sys.argv[2], **out)
"""


def test_configs4_at_its_full_per_gpu_size(gpu, tmp_path):
    """BASELINE configs[4] at the FULL size of one GPU's shard -- 131 072 rays x 43 samples, T = 2^22 (281 MB table), 5.6 M samples: too large for the CPU
    oracle in a test, so (i) size-independent properties of the band every forward of this path must respect (evaluated samples form a prefix of their
    ray, reaching at least to measured depth + truncation) and (ii) the two independent implementations against each other -- the Morton-ordered forward
    (round 6, the default here) and the packed forward (round 4; NARUTO_FWD_SORTED=0), which share neither the launch structure nor the order of
    evaluation nor the layout of the saved features: losses, rendered maps, loss sums, weight / uncertainty-grid gradients and a strided probe of the table
    gradient (the binned scatter's path) agree to OneBlob's closed-vs-dense distance."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "t22_full.py"
    script.write_text(_FULL_T22_SCRIPT)
    res = []
    for k, env in enumerate(({"NARUTO_FWD_SORTED": "1"}, {"NARUTO_FWD_SORTED": "0"})):
        out = tmp_path / f"t22_full_{k}.npz"
        e = dict(os.environ)
        e.update(env)
        subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=900)
        res.append(dict(np.load(out)))
    a, b = res
    for r in res:
        assert bool(r["prefix_ok"][0]) and bool(r["covers"][0])
        assert np.isfinite(r["losses"]).all() and 0 < int(r["n_active"][0]) <= int(r["n_eval"][0]) <= 131072 * 43
    assert int(a["n_active"][0]) == int(b["n_active"][0]), "the backward's list (what can receive a cotangent) does not depend on the forward's form"
    for k in a:
        if k in ("n_eval", "n_active", "prefix_ok", "covers"):
            continue
        scale = float(np.abs(b[k]).max()) + 1e-30
        d = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
        assert d <= 5e-5 * scale, f"{k} differs by {d:.3e} at scale {scale:.3e}"


def test_short_and_partial_walk_forwards_equal_the_flat_one(gpu, tmp_path):
    """Round 5: sample counts that are not a multiple of 64 get the five-launch iteration too -- S <= 64 (the shipped 32 + 11) through
    k_query_fwd_loss_short (a workgroup packs 256 / S rays into its four waves' tiles, samples the depths itself, loss stage inside, one
    row of loss partials per workgroup), 64 < S through the depth-ordered walk with a partly filled last tile.  NARUTO_WALK_PARTIAL=0 is the
    round-4 form (flat tiles + k_sample_encode + k_loss_stage); both against it at the distance between OneBlob's closed and dense
    forms (a point's tile decides which one it gets), incl. ray counts that leave the last workgroup partly filled, fewer rays than one
    workgroup takes, S = 64 exactly (R = 4), S = 32 (R = 8) and a tile boundary inside a ray (S = 75, 139)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tag, n_samples_d, n_rays in (("43", 32, 333), ("43_three_rays", 32, 3), ("43_partial_group", 32, 2148), ("64", 53, 257), ("32", 21, 130),
                                     ("75", 64, 333), ("139", 128, 101)):
        script = tmp_path / f"iteration_{tag}.py"
        script.write_text(_KNOB_SCRIPT.replace("n_samples_d=117", f"n_samples_d={n_samples_d}").replace("N = 333", f"N = {n_rays}"))
        res = []
        for k, env in enumerate(({"NARUTO_WALK_PARTIAL": "2"}, {"NARUTO_WALK_PARTIAL": "0"})):
            out = tmp_path / f"{tag}_{k}.npz"
            e = dict(os.environ)
            e.update(env)
            subprocess.run([sys.executable, str(script), root, str(out)], check=True, env=e, timeout=600)
            res.append(dict(np.load(out)))
        a, b = res
        for k in a:
            scale = float(np.abs(b[k]).max()) + 1e-30
            d = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
            assert d <= 2e-5 * scale, f"S = {tag}: {k} differs by {d:.3e} at scale {scale:.3e}"


def test_trainer_ray_buffers_skip_the_copy(gpu):
    """A batch assembled straight into a captured trainer's ray_buffers() replays without the input copy and trains exactly
    like the same batch handed over from outside (KeyFrameStoreHIP.assemble_batch(out=...) writes there)."""
    from naruto_amd import trainer
    cfg = H.office_cfg(12, perturb=1.0)
    bound = torch.tensor(cfg["mapping"]["bound"])
    torch.manual_seed(5)
    a = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
    b.model.load_state_dict(a.model.state_dict())
    b.iter_state.copy_(a.iter_state)
    assert a.ray_buffers() is None
    a.capture(160, smooth=True)
    b.capture(160, smooth=True)
    bufs = b.ray_buffers()
    for it in range(4):
        rays = syn.random_rays(160, cfg["mapping"]["bound"], seed=900 + it, zero_depth_frac=0.1)
        t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        for dst, src in zip(bufs, t):
            dst.copy_(src.reshape(dst.shape))
        _, la = a.step(*t, smooth=True)
        _, lb = b.step(*bufs, smooth=True)
        assert torch.equal(la, lb)
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n


# --------------------------------------------------------------------------------------------- N1 / N2 ("next" rows)
def test_active_ray_sampler_golden(gpu):
    """ActiveRaySamplerHIP against the reference's sampler (golden) and the oracle's deterministic variant."""
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    g = H.load_golden("g8_active_ray")
    cfg = H.office_cfg(16)
    cfg["mapping"]["sample"], cfg["mapping"]["min_pixels_cur"] = int(g["base"]), 25
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=int(g["K"]), oversample_mul=int(g["mul"]))
    assert smp.oversample_num == 1024 and smp.min_pixels_cur == 100
    t = {k: torch.from_numpy(g[k]) for k in ("rays_o", "rays_d", "target_rgb", "target_d")}
    n_cur, K = int(g["n_cur"]), int(g["K"])
    bound = [list(map(float, b)) for b in g["bound"]]
    got = smp.sample_rays(t["rays_o"].to(gpu), t["rays_d"].to(gpu), t["target_rgb"].to(gpu), t["target_d"].to(gpu), list(range(n_cur)), g["vol"], bound)
    want, vals, sel = S.active_ray_sample(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], n_cur, g["vol"], bound, int(g["base"]), K,
                                          int(g["mul"]), deterministic=True)
    for a, b, k in zip(got, want, ("rays_o", "rays_d", "target_rgb", "target_d")):
        assert torch.equal(a.cpu(), b), f"{k}: HIP sampler != deterministic oracle"
    # against the reference itself: everything but the order / tie choice of the K selected rays is identical
    ref = [g[k] for k in ("out_rays_o", "out_rays_d", "out_target_rgb", "out_target_d")]
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy()[K:], b[K:])
    # the selected rays' cached-uncertainty values are the reference's K smallest
    ref_rows = {tuple(r) for r in np.concatenate([ref[0][:K], ref[1][:K]], 1).round(6)}
    got_vals = np.sort(vals[sel])
    ref_sel_vals = np.sort(np.partition(vals, K)[:K])
    assert np.array_equal(got_vals, ref_sel_vals)
    assert len(ref_rows) > 0


def test_rays_to_world_golden(gpu):
    from naruto_amd.active_ray_sampler import rays_to_world
    g = H.load_golden("g8_active_ray")
    ids = torch.from_numpy(g["ids"])
    ids = torch.where(ids < 0, ids + g["poses"].shape[0], ids)          # torch indexing semantics of -1
    o, d = rays_to_world(torch.from_numpy(g["dcam"]).to(gpu), ids.to(gpu), torch.from_numpy(g["poses"]).to(gpu))
    assert np.array_equal(o.cpu().numpy(), g["world_o"])
    H.assert_close(d, g["world_d"], 1e-6, "rays_to_world.d")


# --------------------------------------------------------------------------------------------- N3 ("next" row)
def test_planner_aggregation_golden(gpu):
    """GoalSpaceAggregatorHIP against the reference's uncertainty_aggregation_v2 (golden, the reference's own targets) and the
    oracle's deterministic target selection."""
    from naruto_amd.planner_aggregation import GoalSpaceAggregatorHIP
    g = H.load_golden("g9_planner_aggregation")
    bbox = [list(map(float, b)) for b in g["bbox"]]
    top_k, sub = int(g["top_k"]), int(g["top_k_subset"])
    ag = GoalSpaceAggregatorHIP(bbox, 0.1, uncert_top_k=top_k, uncert_top_k_subset=sub, gs_sensing_range=(0.5, 2.0), safe_sdf=0.8,
                                gs_z_levels=list(g["gs_z_levels"]), device=gpu)
    dims, ranges, goal_idx = S.goal_space(bbox, 0.1, list(g["gs_z_levels"]))
    assert (ag.Nx, ag.Ny, ag.Nz) == dims and torch.equal(ag.goal_space_pts.cpu(), goal_idx.float())
    ok, out = ag.uncertainty_aggregation_v2([g["uncert"], g["sdf"]], targets=g["targets"])
    assert ok
    assert np.array_equal(out["gs_uncert_collections"].cpu().numpy(), g["collections"])          # exact: pure selection
    H.assert_close(out["gs_aggre_uncerts"], g["aggregated"], 1e-6, "gs_aggre_uncerts", rel=1e-6)   # summation order differs
    assert torch.equal(out["topk_uncert_vxl"].cpu(), torch.from_numpy(g["targets"]))
    # own target selection == the oracle's deterministic rule; aggregation on those targets == oracle
    ok, out2 = ag.uncertainty_aggregation_v2([torch.from_numpy(g["uncert"]).to(gpu), torch.from_numpy(g["sdf"]).to(gpu)])
    det = S.topk_targets_deterministic(g["uncert"], top_k, sub)
    assert ok and np.array_equal(out2["topk_uncert_vxl"].cpu().numpy(), det)
    coll, agg, _ = S.uncert_aggregation(g["uncert"], g["sdf"], det, goal_idx, dims, 0.1, (0.5, 2.0), 0.8)
    assert np.array_equal(out2["gs_uncert_collections"].cpu().numpy(), coll.numpy())
    H.assert_close(out2["gs_aggre_uncerts"].reshape(-1), agg, 1e-6, "gs_aggre_uncerts (own targets)", rel=1e-6)
    # an all-solid sdf volume: nothing is safe or visible -> invalid goal space, as in the reference
    ok3, out3 = ag.uncertainty_aggregation_v2([g["uncert"], -np.ones_like(g["sdf"])])
    assert ok3 is False and out3 == {}


def test_planner_aggregation_full_size(gpu):
    """N3 at the office_0 size the planner runs (49 x 56 x 35 volumes of 0.1 m, 2 100 goal candidates, top 4000 -> 300 targets;
    configs/default.py:93-98) on random-walk volumes, against the oracle: selections exact, sums to 1e-6."""
    from naruto_amd import config as C
    from naruto_amd.planner_aggregation import GoalSpaceAggregatorHIP
    bbox = C.office0_config()["mapping"]["bound"]
    ag = GoalSpaceAggregatorHIP(bbox, 0.1, device=gpu)
    dims, ranges, goal_idx = S.goal_space(bbox, 0.1, [5, 11, 17])
    assert (ag.Nx, ag.Ny, ag.Nz) == dims == (49, 56, 35) and goal_idx.shape[0] == 25 * 28 * 3
    rs = np.random.RandomState(71)
    X, Y, Z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    room = np.minimum.reduce([X - 1.5, dims[0] - 2.5 - X, Y - 1.5, dims[1] - 2.5 - Y, Z - 1.5, dims[2] - 2.5 - Z]).astype(np.float32)
    blobs = np.minimum.reduce([np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) - r for cx, cy, cz, r in
                               zip(rs.uniform(5, 44, 9), rs.uniform(5, 50, 9), rs.uniform(3, 30, 9), rs.uniform(1.5, 5, 9))]).astype(np.float32)
    sdf = (np.minimum(room, blobs) * 0.5 + rs.normal(0, 0.03, dims)).astype(np.float32)
    uncert = (rs.uniform(0.01, 3.0, dims) * ((sdf >= 0) & (sdf < 0.5))).astype(np.float32)
    ok, out = ag.uncertainty_aggregation_v2([torch.from_numpy(uncert).to(gpu), torch.from_numpy(sdf).to(gpu)])
    det = S.topk_targets_deterministic(uncert, 4000, 300)
    assert ok and np.array_equal(out["topk_uncert_vxl"].cpu().numpy(), det)
    coll, agg, valid = S.uncert_aggregation(uncert, sdf, det, goal_idx, dims, 0.1, (0.5, 2.0), 0.8)
    assert 0 < int(valid.sum()) < valid.numel()
    assert np.array_equal(out["gs_uncert_collections"].cpu().numpy(), coll.numpy())
    H.assert_close(out["gs_aggre_uncerts"].reshape(-1), agg, 1e-5, "gs_aggre_uncerts (full size)", rel=1e-6)


def test_active_ray_sampler_full_size(gpu):
    """N1 at the size of a mapping iteration (2048 + 4 x 2048 oversampled + 100 current rays, K = 500) against the
    deterministic oracle: identical batches."""
    from naruto_amd import config as C
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    cfg = C.office0_config()
    cfg["mapping"]["sample"] = 2048
    bound = cfg["mapping"]["bound"]
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=500, oversample_mul=4)
    n_cur = 100
    n = smp.oversample_num + n_cur
    rays = syn.random_rays(n, bound, seed=72)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    rs = np.random.RandomState(72)
    vol = (rs.uniform(0, 3, (49, 56, 35)) * (rs.uniform(size=(49, 56, 35)) < 0.3)).astype(np.float32)     # many exact zeros: ties
    got = smp.sample_rays(t["rays_o"].to(gpu), t["rays_d"].to(gpu), t["target_rgb"].to(gpu), t["target_d"].to(gpu), list(range(n_cur)), vol, bound)
    want, vals, sel = S.active_ray_sample(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], n_cur, vol, bound, 2048, 500, 4, deterministic=True)
    for a, b, k in zip(got, want, ("rays_o", "rays_d", "target_rgb", "target_d")):
        assert a.shape == b.shape and torch.equal(a.cpu(), b), f"{k}: HIP sampler != deterministic oracle"


@pytest.mark.parametrize("case", list(range(6)))
def test_next_rows_random_configs(gpu, case):
    """N1 and N3 over drawn configurations (scene box, voxel size, batch / K / oversampling, top-k sizes, sensing range, safety
    margin, goal levels) against the oracle: identical batches, identical collections."""
    from naruto_amd import config as C
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    from naruto_amd.planner_aggregation import GoalSpaceAggregatorHIP
    rs = np.random.RandomState(700 + case)
    ext = rs.uniform(2.0, 7.0, 3)
    lo = rs.uniform(-4.0, 1.0, 3)
    bbox = [[float(lo[i]), float(lo[i] + ext[i])] for i in range(3)]
    # ---- N3
    vox = float(rs.choice([0.1, 0.2]))
    levels = sorted(int(v) for v in rs.choice(np.arange(2, int(ext[2] / vox) - 1), size=min(3, int(ext[2] / vox) - 3), replace=False))
    top_k, sub = int(rs.choice([50, 400, 3000])), int(rs.choice([7, 60, 300]))
    rng_lo, rng_hi, safe = float(rs.uniform(0.2, 0.8)), float(rs.uniform(1.2, 3.0)), float(rs.uniform(0.2, 1.0))
    dims, ranges, goal_idx = S.goal_space(bbox, vox, levels)
    top_k = min(top_k, int(np.prod(dims)))
    sub = min(sub, top_k)
    ag = GoalSpaceAggregatorHIP(bbox, vox, uncert_top_k=top_k, uncert_top_k_subset=sub, gs_sensing_range=(rng_lo, rng_hi), safe_sdf=safe, gs_z_levels=levels,
                                device=gpu)
    assert (ag.Nx, ag.Ny, ag.Nz) == dims
    X, Y, Z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    room = np.minimum.reduce([X - 1.5, dims[0] - 2.5 - X, Y - 1.5, dims[1] - 2.5 - Y, Z - 1.5, dims[2] - 2.5 - Z]).astype(np.float32)
    blob = (np.sqrt((X - dims[0] * 0.4) ** 2 + (Y - dims[1] * 0.6) ** 2 + (Z - dims[2] * 0.5) ** 2) - min(dims) * 0.15).astype(np.float32)
    sdf = (np.minimum(room, blob) * 0.5 + rs.normal(0, 0.03, dims)).astype(np.float32)
    uncert = (rs.uniform(0.01, 3.0, dims) * ((sdf >= 0) & (sdf < 0.5))).astype(np.float32)
    ok, out = ag.uncertainty_aggregation_v2([torch.from_numpy(uncert).to(gpu), torch.from_numpy(sdf).to(gpu)], force_running=True)
    det = S.topk_targets_deterministic(uncert, top_k, sub)
    coll, agg, valid = S.uncert_aggregation(uncert, sdf, det, goal_idx, dims, vox, (rng_lo, rng_hi), safe)
    if ok:
        assert np.array_equal(out["topk_uncert_vxl"].cpu().numpy(), det)
        assert np.array_equal(out["gs_uncert_collections"].cpu().numpy(), coll.numpy())
        H.assert_close(out["gs_aggre_uncerts"].reshape(-1), agg, 1e-5, f"case {case}: gs_aggre_uncerts", rel=1e-6)
    else:
        assert float(agg.abs().sum()) == 0.0                   # the reference reports an invalid goal space when nothing is in view
    # ---- N1
    cfg = C.office0_config()
    cfg["mapping"]["bound"] = bbox
    cfg["mapping"]["sample"] = int(rs.choice([256, 1024, 2048]))
    cfg["mapping"]["min_pixels_cur"] = int(rs.choice([10, 25, 100]))
    mul, K = int(rs.choice([2, 4])), int(rs.choice([50, 200, 500]))
    K = min(K, cfg["mapping"]["sample"] - 1)
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=K, oversample_mul=mul)
    n_cur = int(rs.choice([3, 40, 100]))                        # 0 is rejected: the reference then appends rays[-0:] = every ray
    n = smp.oversample_num + n_cur
    rays = syn.random_rays(n, bbox, seed=700 + case)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    vdims = S.goal_space(bbox, 0.1)[0]
    vol = (rs.uniform(0, 3, vdims) * (rs.uniform(size=vdims) < 0.4)).astype(np.float32)
    got = smp.sample_rays(t["rays_o"].to(gpu), t["rays_d"].to(gpu), t["target_rgb"].to(gpu), t["target_d"].to(gpu), list(range(n_cur)), vol, bbox)
    want, vals, sel = S.active_ray_sample(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], n_cur, vol, bbox, cfg["mapping"]["sample"], K, mul,
                                          deterministic=True)
    for a, b, k in zip(got, want, ("rays_o", "rays_d", "target_rgb", "target_d")):
        assert a.shape == b.shape and torch.equal(a.cpu(), b), f"case {case}: {k}: HIP sampler != deterministic oracle"


# --------------------------------------------------------------------------------------------- edge cases
def test_edge_sizes_and_degenerate_inputs(gpu):
    """Empty and minimal inputs, the per-ray sample limit, depths that are zero / negative / beyond depth_trunc.  (A NaN
    depth is treated like a missing one here; the reference lets it poison every loss of the batch -- INTEGRATION.md.)"""
    from naruto_amd import _lib, ops
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 51)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    # empty and single-point queries
    assert m.query_color_sdf(torch.zeros(0, 3, device=gpu)).shape == (0, 5)
    one = torch.tensor([[0.31, 0.72, 0.55]])
    H.assert_close(m.query_color_sdf(one.to(gpu)), ora.query_color_sdf(one), TOL_OUT, "raw(1 point)")
    # one ray; rays with zero / NaN / over-range depth: the masks of get_masks and the near-far fallback of render_rays
    m.train(), ora.train()
    rays = syn.random_rays(6, cfg["mapping"]["bound"], seed=51)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    t["target_d"][1] = 0.0
    t["target_d"][2] = -1.0                      # negative depth: the near-far fallback as well (target_d <= 0)
    t["target_d"][3] = 150.0                     # > cam.depth_trunc = 100: excluded from the depth / uncertainty losses
    t["target_d"][5] = 0.0                       # the oracle's view of the NaN depth below: a missing measurement
    for n in (1, 5, 6):
        a = {k: v[:n] for k, v in t.items()}
        ret_o = ora.forward(a["rays_o"], a["rays_d"], a["target_rgb"], a["target_d"])
        hd = a["target_d"].clone()
        if n == 6:
            hd[5] = float("nan")                 # found broken by tests/accuracy_study.py in round 4: 0 * NaN made sdf_loss NaN
        for fused in (True, False):
            m.fused_train = fused
            ret_h = m.forward(a["rays_o"].to(gpu), a["rays_d"].to(gpu), a["target_rgb"].to(gpu), hd.to(gpu))
            for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "uncert_loss"):
                H.assert_close(ret_h[k].reshape(-1), ret_o[k].reshape(-1), 1e-5, f"{n} rays.{k} (fused {fused})", rel=1e-4)
        if n == 6:                               # ... and the gradients of such a batch are finite and equal the oracle's
            m.zero_grad()
            ora.zero_grad()
            trainer_loss = sum(ret_h[k] for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss"))
            trainer_loss.backward()
            sum(ret_o[k] for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss")).backward()
            g_h, g_o = H.hip_grads(m), H.ora_grads(ora)
            for k in ("sdf_w0", "col_w0", "table"):
                assert bool(torch.isfinite(g_h[k]).all()), k
                H.assert_close(g_h[k], g_o[k], 1e-4 * float(g_o[k].abs().max()), f"nan-depth batch: grad {k}", rel=1e-3)
    m.fused_train = True
    # the per-ray sample limit (kMaxSamples = 1024) and one past it
    lib = _lib.load()
    N = 3
    td = torch.tensor([1.3, 0.0, 2.2])
    z_o = S.sample_z(N, td.view(-1, 1), 0.0, 5.0, 1013, 11, 0.1, 0.0)
    z_h = ops.sample_z(N, td.to(gpu), 0.0, 5.0, 1013, 11, 0.1, 0, None, device=gpu)
    H.assert_close(z_h, z_o, 1e-6, "z_vals S=1024", rel=1e-6)
    with pytest.raises(_lib.NarutoError):
        ops.sample_z(N, td.to(gpu), 0.0, 5.0, 1014, 11, 0.1, 0, None, device=gpu)
    raw = torch.randn(N, 1024, 5, generator=torch.Generator().manual_seed(3))
    out_o = S.raw2outputs(raw, z_o, cfg["training"]["trunc"], cfg["data"]["sc_factor"])
    out_h = ops.composite(m._handle(), raw.to(gpu), z_h)             # rgb, disp, acc, weights, depth, depth_var, uncert_map
    for a, b, name in zip(out_h, out_o, ("rgb", "disp", "acc", "weights", "depth", "depth_var", "uncert_map")):
        H.assert_close(a, b, 2e-5, f"{name} S=1024", rel=1e-4)


def test_scatter_collisions(gpu):
    """Every point in ONE cell (all updates of a level collide on eight entries, the worst case for the LDS accumulators) plus a
    block of distinct points: the table gradient of hash_encode equals the oracle's."""
    from naruto_amd import ops
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 52)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rs = np.random.RandomState(52)
    same = np.tile(np.array([[0.4137, 0.2871, 0.6312]], np.float32), (3000, 1)) + rs.uniform(0, 1e-5, (3000, 3)).astype(np.float32)
    x = np.concatenate([same, rs.uniform(0, 1, (1500, 3)).astype(np.float32)])
    c = rs.normal(size=(x.shape[0], 32)).astype(np.float32)
    f_o = S.hash_encode(torch.from_numpy(x), ora.table, ora.meta)
    (f_o * torch.from_numpy(c)).sum().backward()
    f_h = m.query_sdf(torch.from_numpy(x).to(gpu), embed=True)
    H.assert_close(f_h, f_o, 5e-6, "features")
    (f_h * torch.from_numpy(c).to(gpu)).sum().backward()
    grad_close(m.embed_fn.params.grad, ora.table.grad, "collisions.grad.table")


@pytest.mark.parametrize("size", ["tiny", "large"])
def test_scatter_small_contributions_are_exact(gpu, size):
    """The table gradient is accumulated in 2^-40 fixed point.  Tiny cotangents of both signs (1e-7 .. 1e-5, the size of a
    real iteration's contributions) must come out with fp64-like accuracy: a float -> fixed conversion that splits with
    floor / fract loses the low bits of every small NEGATIVE contribution (1 + t rounded next to 1.0).  "large": cotangents of
    10 .. 8 000 -- beyond +-2047 the hashed levels' fp64 conversion (naruto_field.hip, fix_add_corners) is out of its range and
    the wave takes the fp32 split; every wave here holds both kinds."""
    lo_exp, hi_exp, rel_tol, abs_tol = (-7, -5, 1e-7, 2e-11) if size == "tiny" else (1.0, 3.9, 1e-6, 0.0)
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 53)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rs = np.random.RandomState(53)
    x = rs.uniform(0, 1, (20000, 3)).astype(np.float32)
    c = (rs.choice([-1.0, 1.0], size=(x.shape[0], 32)) * 10.0 ** rs.uniform(lo_exp, hi_exp, size=(x.shape[0], 32))).astype(np.float32)
    # fp64 truth with the oracle's own indices and weights
    xt = torch.from_numpy(x)
    truth = np.zeros((ora.meta.n_params // 2, 2))
    for lvl in range(ora.meta.n_levels):
        pos = (xt.double() * float(ora.meta.scale[lvl]) + 0.5).to(torch.float32)
        g = torch.floor(pos)
        w = pos - g
        gi = g.to(torch.int64) & S.U32
        for corner in range(8):
            wgt = torch.ones(x.shape[0])
            cc = []
            for dim in range(3):
                if (corner >> dim) & 1:
                    wgt = wgt * w[:, dim]
                    cc.append((gi[:, dim] + 1) & S.U32)
                else:
                    wgt = wgt * (1 - w[:, dim])
                    cc.append(gi[:, dim])
            idx = (S.hash_grid_index(ora.meta, lvl, cc[0], cc[1], cc[2]) + int(ora.meta.offset[lvl])).numpy()
            np.add.at(truth, idx, wgt.numpy().astype(np.float64)[:, None] * c[:, 2 * lvl:2 * lvl + 2].astype(np.float64))
    f_h = m.query_sdf(torch.from_numpy(x).to(gpu), embed=True)
    (f_h * torch.from_numpy(c).to(gpu)).sum().backward()
    got = m.embed_fn.params.grad.double().cpu().numpy().reshape(-1, 2)
    err = np.abs(got - truth)
    scale = np.abs(truth).max()
    # fp32 output rounding of each entry (6e-8 relative) + 2^-40 per contribution; the floor / fract split gave 2e-10 per entry
    # ("large": the fp32 split rounds every product w * g to fp32 first, 6e-8 of up to a hundred contributions per coarse entry)
    assert err.max() <= rel_tol * scale + abs_tol, f"table gradient off by {err.max():.3e} (scale {scale:.3e})"


def test_scatter_drops_nan_cotangents(gpu):
    """a point whose cotangent is NaN / Inf (or beyond the fixed point's 2^22) contributes nothing to the table gradient
    -- the reference's float atomics would spread it -- and takes nothing of its neighbours with it (the dense levels sum the points
    of a cell in registers first).  Every 97th point's cotangents are NaN, Inf or 1e9: the result must be the gradient of the same batch
    with those cotangents zeroed, bit for bit on every level.  (office_cfg(12) has no binned level: the same on levels of more than 2^17
    entries, and per feature component, is test_gpu_binned.py::test_binned_levels_drop_out_of_range_cotangents.)"""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 59)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rs = np.random.RandomState(59)
    x = torch.from_numpy(rs.uniform(0, 1, (30000, 3)).astype(np.float32)).to(gpu)
    c = torch.from_numpy((rs.standard_normal((30000, 32)) * 1e-3).astype(np.float32)).to(gpu)
    bad = torch.arange(0, 30000, 97, device=gpu)
    c_bad = c.clone()
    c_bad[bad[0::3]] = float("nan")
    c_bad[bad[1::3]] = float("inf")
    c_bad[bad[2::3]] = 1e9
    c_zero = c.clone()
    c_zero[bad] = 0.0
    grads = []
    for cot in (c_bad, c_zero):
        m.embed_fn.params.grad = None
        m.query_sdf(x, embed=True).backward(cot)
        grads.append(m.embed_fn.params.grad.clone())
    assert torch.isfinite(grads[0]).all()
    assert torch.equal(grads[0], grads[1])


def test_active_ray_sampler_ties(gpu):
    """An all-zero cached uncertainty volume (the state before the first planner query): every candidate ties, the K
    lowest-index candidates are taken, exactly as the oracle's deterministic rule."""
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    cfg = H.office_cfg(16)
    cfg["mapping"]["sample"], cfg["mapping"]["min_pixels_cur"] = 128, 20
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=40, oversample_mul=4)
    n_cur = 33
    n = smp.oversample_num + n_cur
    rays = syn.random_rays(n, cfg["mapping"]["bound"], seed=53)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    vol = np.zeros((49, 56, 35), np.float32)
    got = smp.sample_rays(*(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")), list(range(n_cur)), vol, cfg["mapping"]["bound"])
    want, vals, sel = S.active_ray_sample(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"], n_cur, vol, cfg["mapping"]["bound"], 128, 40, 4,
                                          deterministic=True)
    assert np.array_equal(sel, np.arange(40))
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b)


@pytest.mark.parametrize("n_cand,K", [(33, 1), (33, 32), (1000, 999), (4097, 500), (8191, 2048), (8192, 1), (8192, 8191), (8192, 3000)])
def test_active_ray_select_edges_through_the_c_abi(gpu, n_cand, K):
    """naruto_active_ray_select (k_ars_fused: lookup, bit-sliced threshold search, gather in one launch) at the edges of its range: candidate
    counts that are not multiples of a thread's 32 keys, the largest count it takes (8 192), K = 1 and K = n - 1, and a volume full of ties,
    negative values, +-0 and NaNs (a NaN sorts last).  The rays are placed ON voxel centres (direction 0), so the expected keys are the volume's
    values at known voxels and the expected batch is [the K smallest by (value, index), ascending index | the first base - K rays | the tail]."""
    import ctypes as C
    from naruto_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(n_cand * 7 + K)
    X, Y, Z = 49, 56, 35
    vol = rs.choice(np.array([0.0, -0.0, 0.5, 0.5, 1.25, -3.0, 7.0, np.nan, 2.0 ** -130], np.float32), size=(X, Y, Z)).astype(np.float32)
    vol[rs.rand(X, Y, Z) < 0.3] = np.float32(rs.uniform(-1, 4))                                        # one more heavily tied value
    base, n_tail = max(K, 64), 25
    n_total = base + n_cand + n_tail
    bmin = np.array([-1.5, 0.25, -2.0], np.float32)
    vox = np.stack([rs.randint(0, X, n_total), rs.randint(0, Y, n_total), rs.randint(0, Z, n_total)], 1)
    rays_o = (bmin + vox.astype(np.float32) / np.float32(10.0)).astype(np.float32)                    # (o - bmin) * 10 rounds back to the voxel
    assert np.array_equal(np.rint((rays_o - bmin) * np.float32(10.0)).astype(int), vox)
    rays_d = np.zeros((n_total, 3), np.float32)
    target_s = rs.rand(n_total, 3).astype(np.float32)
    target_d = rs.uniform(0.5, 3.0, n_total).astype(np.float32)
    cand_vals = vol[vox[base:base + n_cand, 0], vox[base:base + n_cand, 1], vox[base:base + n_cand, 2]]
    # order: float order with -0 < +0 as the sortable key has it (sign bit), NaN last; ties by index
    bits = cand_vals.view(np.uint32).astype(np.uint64)
    keys = np.where(bits & 0x80000000, (~bits) & 0xFFFFFFFF, bits | 0x80000000)
    order = np.lexsort((np.arange(n_cand), keys))
    sel = np.sort(order[:K])
    src = np.concatenate([base + sel, np.arange(0, base - K), np.arange(n_total - n_tail, n_total)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    o, d, c, td, v = t(rays_o), t(rays_d), t(target_s), t(target_d), t(vol)
    n_out = base + n_tail
    outs = [torch.full((n_out, 3), -7.0, device=gpu) for _ in range(3)] + [torch.full((n_out,), -7.0, device=gpu)]
    ws = torch.empty(lib.naruto_active_ray_workspace(n_total, K) // 4 + 4, dtype=torch.int32, device=gpu)
    dims = (C.c_uint32 * 3)(X, Y, Z)
    bm = (C.c_float * 3)(*[float(b) for b in bmin])
    p = lambda a: C.c_void_p(a.data_ptr())
    _lib.check(lib.naruto_active_ray_select(n_total, base, K, n_tail, p(o), p(d), p(c), p(td), p(v), dims, bm, 10.0, p(outs[0]), p(outs[1]), p(outs[2]),
                                            p(outs[3]), p(ws), None), "naruto_active_ray_select")
    torch.cuda.synchronize()
    for got, want, name in ((outs[0], rays_o[src], "rays_o"), (outs[1], rays_d[src], "rays_d"), (outs[2], target_s[src], "target_s"), (outs[3], target_d[src], "target_d")):
        assert np.array_equal(got.cpu().numpy(), want), f"{name}: selected batch differs (n_cand {n_cand}, K {K})"


# --------------------------------------------------------------------------------------------- N2, store side
def test_keyframe_store_batch_assembly(gpu):
    """KeyFrameStoreHIP: add_keyframe keeps distinct (valid) pixels and tiles short frames; assemble_batch draws distinct
    stored rays + distinct current-frame pixels (exactly the host permutation naruto_perm_index), gathers them and rotates
    them to world bit for bit like coslam.py:337-344 (oracle rays_to_world)."""
    from naruto_amd import _lib
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    lib = _lib.load()
    cfg = H.office_cfg(16)
    cfg["mapping"]["keyframe_every"] = 5
    Hh, Ww, R = 24, 32, 200
    st = KeyFrameStoreHIP(cfg, Hh, Ww, num_kf=6, num_rays_to_save=R, device=gpu, seed=77, filter_depth_mode="valid_only")
    rs = np.random.RandomState(61)
    frames = []
    for k in range(4):
        depth = rs.uniform(0.3, 4.0, (1, Hh, Ww)).astype(np.float32)
        if k == 2:
            depth[:] = 0.0
            depth[0, :3, :20] = 1.5                       # only 60 valid pixels: the stored rows are a periodic tiling of them
        depth[0, rs.uniform(size=(Hh, Ww)) < 0.2] = 0.0
        b = {"direction": torch.from_numpy(rs.normal(size=(1, Hh, Ww, 3)).astype(np.float32)), "rgb": torch.from_numpy(rs.uniform(size=(1, Hh, Ww, 3)).astype(np.float32)),
             "depth": torch.from_numpy(depth), "frame_id": 5 * k}
        frames.append(torch.cat([b["direction"], b["rgb"], b["depth"][..., None]], -1).reshape(-1, 7))
        st.add_keyframe(b, filter_depth=True)
    assert len(st) == 4 and st.frame_ids.cpu().tolist() == [0, 5, 10, 15]
    for k in range(4):
        rows = st.rays[k].cpu()
        src = frames[k]
        assert (rows[:, 6] > 0).all()                                                 # filter_depth: only valid pixels
        keys = {tuple(r.tolist()) for r in src}
        assert all(tuple(r.tolist()) in keys for r in rows)                           # every stored row is a pixel of that frame
        n_valid = int(((src[:, 6] > 0) & (src[:, 6] <= cfg["cam"]["depth_trunc"])).sum())
        uniq = len({tuple(r.tolist()) for r in rows})
        assert uniq == min(n_valid, R)                                                # distinct pixels, tiled when the frame is short
        if n_valid < R:
            assert torch.equal(rows[:n_valid], rows[n_valid:2 * n_valid][:n_valid]) or R < 2 * n_valid
    # batch assembly
    cur = frames[3].to(gpu)
    poses = torch.eye(4).repeat(4, 1, 1)
    for i in range(4):
        a = 0.4 * i + 0.2
        poses[i, :3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32)
        poses[i, :3, 3] = torch.tensor(rs.uniform(-1, 1, 3), dtype=torch.float32)
    bs = 300
    o, d, s, t, n_cur, ids = st.assemble_batch(bs, cur, poses, min_pixels_cur=40, filter_depth=True, return_ids=True)
    assert n_cur == max(bs // 4, 40) and o.shape == (bs + n_cur, 3) and t.shape == (bs + n_cur, 1)
    ctr = st.counter
    n_pop = 4 * R
    gidx = np.array([lib.naruto_perm_index(i, n_pop, 77, ctr, 2) for i in range(bs)])
    assert len(np.unique(gidx)) == bs
    flat = st.rays[:4].reshape(-1, 7).cpu()
    valid_list = torch.nonzero((frames[3][:, 6] > 0) & (frames[3][:, 6] <= cfg["cam"]["depth_trunc"])).reshape(-1)
    cidx = valid_list[[lib.naruto_perm_index(i, int(valid_list.shape[0]), 77, ctr, 3) for i in range(n_cur)]]
    assert len(set(cidx.tolist())) == n_cur
    rows = torch.cat([flat[gidx], frames[3][cidx]], 0)
    want_ids = torch.cat([st.frame_ids.cpu()[gidx // R] // 5, -torch.ones(n_cur, dtype=torch.int64)])
    assert torch.equal(ids.cpu(), want_ids)
    w_o, w_d = S.rays_to_world(rows[:, :3], want_ids, poses)
    assert torch.equal(o.cpu(), w_o)
    H.assert_close(d, w_d, 1e-6, "assemble.rays_d", rel=1e-6)           # torch.sum's association over the 3 products differs by an ulp
    assert torch.equal(s.cpu(), rows[:, 3:6]) and torch.equal(t.cpu(), rows[:, 6:7])
    # the same draw written into caller-provided buffers (a captured trainer's ray_buffers())
    st.counter = ctr - 1
    bufs = tuple(torch.full((bs + n_cur, c), -7.0, device=gpu) for c in (3, 3, 3, 1))
    o2, d2, s2, t2, n_cur2 = st.assemble_batch(bs, cur, poses, min_pixels_cur=40, filter_depth=True, out=bufs)
    assert n_cur2 == n_cur and o2 is bufs[0] and t2 is bufs[3]
    assert torch.equal(o2, o) and torch.equal(d2, d) and torch.equal(s2, s) and torch.equal(t2, t)
    with pytest.raises(RuntimeError):
        st.assemble_batch(bs, cur, poses, min_pixels_cur=40, filter_depth=True, out=tuple(b[:-1] for b in bufs))
    # sample_global_rays: distinct rows with their frame ids
    r2, f2 = st.sample_global_rays(128)
    assert r2.shape == (128, 7) and set(f2.cpu().tolist()) <= {0, 5, 10, 15}


def test_keyframe_store_filter_depth_reference_quirk(gpu):
    """filter_depth_mode="reference" (the default) reproduces the reference's indexing: indices drawn from range(num_valid)
    are applied to the UNFILTERED pixel list (keyframe.py:27-36, coslam.py:318-327), so the kept pixels are distinct pixels among
    the first num_valid of the frame, invalid-depth ones included."""
    from naruto_amd import _lib
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    lib = _lib.load()
    cfg = H.office_cfg(16)
    cfg["mapping"]["keyframe_every"] = 5
    Hh, Ww, R = 16, 20, 64
    st = KeyFrameStoreHIP(cfg, Hh, Ww, num_kf=3, num_rays_to_save=R, device=gpu, seed=5)
    assert st.filter_depth_mode == "reference"
    rs = np.random.RandomState(8)
    depth = rs.uniform(0.3, 4.0, (1, Hh, Ww)).astype(np.float32)
    depth[0, rs.uniform(size=(Hh, Ww)) < 0.4] = 0.0
    b = {"direction": torch.from_numpy(rs.normal(size=(1, Hh, Ww, 3)).astype(np.float32)), "rgb": torch.from_numpy(rs.uniform(size=(1, Hh, Ww, 3)).astype(np.float32)),
         "depth": torch.from_numpy(depth), "frame_id": 0}
    frame = torch.cat([b["direction"], b["rgb"], b["depth"][..., None]], -1).reshape(-1, 7)
    n_valid = int(((frame[:, 6] > 0) & (frame[:, 6] <= cfg["cam"]["depth_trunc"])).sum())
    st.add_keyframe(b, filter_depth=True)
    idx = [lib.naruto_perm_index(i, n_valid, 5, st.counter, 1) for i in range(R)]
    assert max(idx) < n_valid and len(set(idx)) == R
    assert torch.equal(st.rays[0].cpu(), frame[idx])                     # rows of the UNFILTERED frame
    assert (st.rays[0][:, 6] == 0).any()                                 # ... so invalid-depth pixels are among them
    poses = torch.eye(4).repeat(2, 1, 1)
    o, d, s, t, n_cur = st.assemble_batch(32, frame.to(gpu), poses, min_pixels_cur=24, filter_depth=True)
    assert n_cur == min(n_valid, 32)
    cidx = [lib.naruto_perm_index(i, n_valid, 5, st.counter, 3) for i in range(n_cur)]
    assert torch.equal(t.cpu()[32:, 0], frame[cidx, 6]) and torch.equal(s.cpu()[32:], frame[cidx, 3:6])


# --------------------------------------------------------------------------------------------- N4: dense volume -> mesh
def _mc_volumes():
    rs = np.random.RandomState(3)
    n = 23
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, n)] * 3, indexing="ij"), -1)
    sphere = (np.linalg.norm(g - np.array([0.05, -0.03, 0.02]), axis=-1) - 0.6).astype(np.float32)
    noise = rs.standard_normal((17, 9, 31)).astype(np.float32)
    planes = np.round(rs.standard_normal((12, 13, 14)) * 2).astype(np.float32) * 0.5          # many values exactly on the isolevel
    thin = rs.standard_normal((2, 2, 70)).astype(np.float32)
    big = (np.sin(np.arange(70 * 65 * 61, dtype=np.float64).reshape(70, 65, 61) * 0.37) +
           0.3 * np.cos(np.arange(70)[:, None, None] * 0.2)).astype(np.float32)               # > 1 scan block, > 1024 blocks would need 2M+ voxels
    return {"sphere": (sphere, 0.0, 3.0), "noise": (noise, 0.1, 1e9), "noise_trunc": (noise, 0.0, 1.2), "on_isolevel": (planes, 0.0, 3.0),
            "thin": (thin, 0.0, 3.0), "single_voxel": (np.zeros((1, 1, 1), np.float32), 0.0, 3.0), "no_cells": (noise[:1], 0.0, 3.0),
            "empty_surface": (np.ones((5, 6, 7), np.float32), 0.0, 3.0), "multi_block": (big, 0.05, 3.0)}


@pytest.mark.parametrize("name", list(_mc_volumes()))
def test_marching_cubes_vs_oracle(gpu, name):
    """bit-exact vertices (float64) and triangles against the numpy restatement, through naruto_mesh_count / naruto_mesh_emit"""
    from naruto_amd import mesh as M
    from oracle import mesh_numpy as MN
    vol, iso, trunc = _mc_volumes()[name]
    v, f = M.marching_cubes(torch.from_numpy(vol).to(gpu), iso, trunc)
    ov, of = MN.marching_cubes(vol, iso, trunc, H.load_golden("mc_table"))
    assert v.dtype == torch.float64 and f.dtype == torch.int32
    assert v.shape == ov.shape and f.shape == of.shape, (v.shape, ov.shape, f.shape, of.shape)
    assert np.array_equal(f.cpu().numpy(), of)
    assert np.array_equal(v.cpu().numpy(), ov)
    if name in ("single_voxel", "no_cells", "empty_surface"):
        assert len(ov) == 0 and len(of) == 0
    else:
        assert len(of) > 0


def test_marching_cubes_large_volume_properties(gpu):
    """a volume with > 1024 scan blocks (the block-total scan loops): closed surface of a sphere, vertex count = crossed edges"""
    from naruto_amd import mesh as M
    n = 160
    t = torch.linspace(-1, 1, n, device=gpu)
    g = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1)
    vol = (torch.linalg.norm(g - torch.tensor([0.01, 0.02, -0.03], device=gpu), dim=-1) - 0.7).float().contiguous()
    assert vol.numel() > 1024 * 2048
    v, f = M.marching_cubes(vol, 0.0, 3.0)
    inside = vol.double() < 0
    n_cross = int((inside[1:] != inside[:-1]).sum() + (inside[:, 1:] != inside[:, :-1]).sum() + (inside[:, :, 1:] != inside[:, :, :-1]).sum())
    assert len(v) == n_cross and len(v) - len(f) // 2 == 2                       # Euler: V - E + F = V - 3F/2 + F = 2
    fl = f.long()
    e = torch.cat([fl[:, [0, 1]], fl[:, [1, 2]], fl[:, [2, 0]]])
    key = e[:, 0] * len(v) + e[:, 1]
    rkey = e[:, 1] * len(v) + e[:, 0]
    assert len(torch.unique(key)) == len(key) and torch.equal(torch.sort(key).values, torch.sort(rkey).values)     # closed, oriented
    p = v / (n - 1) * 2 - 1 - torch.tensor([0.01, 0.02, -0.03], device=gpu, dtype=torch.float64)
    assert (torch.linalg.norm(p, dim=-1) - 0.7).abs().max() < 1e-3
    nrm = torch.cross(p[fl[:, 1]] - p[fl[:, 0]], p[fl[:, 2]] - p[fl[:, 0]], dim=-1)
    assert ((nrm * p[fl].mean(1)).sum(-1) > 0).all()


def test_lattice_points(gpu):
    from naruto_amd import mesh as M
    tx, ty, tz = torch.linspace(0, 1, 7), torch.linspace(-2, 3, 5), torch.linspace(0.25, 0.5, 11)
    want = torch.stack(torch.meshgrid(tx, ty, tz, indexing="ij"), -1).reshape(-1, 3)
    got = M.lattice_points(tx.to(gpu), ty.to(gpu), tz.to(gpu))
    assert torch.equal(got.cpu(), want)


def test_extract_mesh_golden(gpu, tmp_path):
    """N4 end to end against what the reference's own extract_mesh returned (tests/golden/g10_extract_mesh.npz)."""
    from naruto_amd import mesh as M
    g = H.load_golden("g10_extract_mesh")
    cfg = H.office_cfg(int(g["hash_size"]))
    cfg["data"]["sc_factor"], cfg["data"]["translation"] = float(g["sc_factor"]), float(g["translation"])
    w = {k: g[k] for k in ("sdf_w0", "sdf_w1", "col_w0", "col_w1")}
    ora = H.make_oracle(cfg, float(g["table_amp"]), int(g["seed"]), weights=w)
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    mcb = torch.from_numpy(g["mcb"])
    # marching cubes on the golden's own volume: exact
    v, f = M.marching_cubes(torch.from_numpy(g["vol"]).to(gpu), float(g["isolevel"]), 3.0)
    assert np.array_equal(v.cpu().numpy(), g["verts_index"]) and np.array_equal(f.cpu().numpy(), g["faces"])
    for tag, color_func in (("color", m.query_color), ("uncert", None)):
        path = tmp_path / tag / "mesh.ply"
        mesh = M.extract_mesh(m.query_sdf, cfg, m.bounding_box, marching_cube_bound=mcb, color_func=color_func, voxel_size=float(g["voxel"]),
                              isolevel=float(g["isolevel"]), mesh_savepath=str(path))
        assert path.exists() and path.stat().st_size > 0
        # the fixture's isolevel keeps every lattice value 1e-4 away, so fp32 noise cannot change the topology
        assert np.array_equal(mesh.faces, g["faces"])
        H.assert_close(mesh.vertices, g[f"{tag}_vertices"], 2e-3 * float(g["voxel"]), f"{tag}.vertices")
        want = np.round(np.clip(g[f"{tag}_colors"], 0, 1) * 255.0)
        got = mesh.vertex_colors[:, :3].astype(np.float64)
        assert mesh.vertex_colors.shape == (len(mesh.vertices), 4) and (mesh.vertex_colors[:, 3] == 255).all()
        if tag == "color":
            assert np.abs(got - want).max() <= 1.0
        else:
            assert (np.abs(got - want).max(-1) > 0).mean() < 0.02          # a jet bin edge may flip with the 1e-6 noise of the uncertainty


def test_submodules_called_on_their_own(gpu):
    """model.embedpos_fn(x), model.calc_embedding(x), model.decoder(embed, embed_pos), model.sdf_net(x), model.color_net(x): the
    reference's sub-modules as standalone forward operators (scene_rep.py:58-64, decoder.py:29-41, 99-116) against the oracle's
    pieces, and their composition against the fused query; with autograd enabled they refuse (the differentiable path is the fused one)."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 83).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    rs = np.random.RandomState(83)
    x = torch.from_numpy(rs.uniform(-0.1, 1.1, (1234, 3)).astype(np.float32))
    xg = x.to(gpu)
    with torch.no_grad():
        pos = m.embedpos_fn(xg)
        H.assert_close(pos, S.oneblob_encode(x, 16), 1e-6, "embedpos_fn", rel=2e-6)           # fp32 evaluation of the quartic cdf: a few ulp at 0.75
        emb = m.calc_embedding(xg)
        H.assert_close(emb, ora.calc_embedding(x), TOL_OUT, "calc_embedding", rel=1e-5)
        h_o = ora.sdf_net(ora.calc_embedding(x), S.oneblob_encode(x, 16))
        h = m.sdf_net(torch.cat([emb, pos], -1))
        assert h.shape == (1234, 17)
        H.assert_close(h, h_o, TOL_OUT, "sdf_net", rel=1e-5)
        assert torch.equal(m.sdf_net(torch.cat([emb, pos], -1), return_geo=False), h[:, :1])
        raw = m.decoder(emb, pos)
        H.assert_close(raw, ora.query_color_sdf(x), TOL_OUT, "decoder", rel=1e-5)
        H.assert_close(raw, m.query_color_sdf(xg), TOL_OUT, "decoder vs the fused query", rel=1e-5)
        rgb = m.color_net(torch.cat([pos, h[:, 1:16]], -1))
        H.assert_close(rgb, raw[:, :3], 1e-7, "color_net", rel=1e-6)
    with pytest.raises(NotImplementedError):
        m.decoder(emb, pos)                              # parameters require grad and autograd is on
    with pytest.raises(ValueError):
        with torch.no_grad():
            m.sdf_net(emb)


def test_render_surface_color(gpu):
    """Co-SLAM's render_surface_color (the mesh colour function under mesh.render_color): n_range_d samples at linspace(-trunc, trunc)
    along a surface normal, run_network + raw2outputs -> rgb.  The one-launch no-grad form and the differentiable operator chain
    against the oracle; then extract_mesh with mesh.render_color = True (trimesh-style angle-weighted vertex normals) against the
    oracle's restatement."""
    from naruto_amd import mesh as M
    from oracle import mesh_numpy as MN
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 61).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    rs = np.random.RandomState(61)
    bb = np.asarray(cfg["mapping"]["bound"])
    pts = torch.from_numpy((bb[:, 0] + rs.uniform(0.1, 0.9, (777, 3)) * (bb[:, 1] - bb[:, 0])).astype(np.float32))
    nrm = rs.normal(size=(777, 3))
    nrm = torch.from_numpy((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32))
    with torch.no_grad():
        want = ora.render_surface_color(pts, nrm)
        got = m.render_surface_color(pts.to(gpu), nrm.to(gpu))
    assert got.shape == (777, 3)
    H.assert_close(got, want, TOL_OUT, "render_surface_color (one launch)", rel=1e-5)
    got_g = m.render_surface_color(pts.to(gpu), nrm.to(gpu))
    assert got_g.requires_grad
    H.assert_close(got_g, want, TOL_OUT, "render_surface_color (operators)", rel=1e-5)
    g_hip = torch.autograd.grad(got_g.sum(), m.decoder.color_net.model[2].weight)[0]
    g_ora = torch.autograd.grad(ora.render_surface_color(pts, nrm).sum(), ora.col_w1 if hasattr(ora, "col_w1") else list(ora.parameters())[-1])[0]
    if g_ora.shape == g_hip.shape:
        H.assert_close(g_hip, g_ora, 1e-6 * float(g_ora.abs().max()) + 1e-9, "render_surface_color d/d(colour layer 2)", rel=1e-4)
    # the mesh colour branch
    table = H.load_golden("mc_table")
    cfg["mesh"] = dict(cfg.get("mesh", {}), render_color=True)
    mcb = torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32)
    o = MN.extract_mesh(ora.query_sdf, cfg, ora.bounding_box, table, marching_cube_bound=mcb, voxel_size=0.4, isolevel=1e9, render_uncert=False)
    srt = np.sort(o["vol"].reshape(-1).astype(np.float64))
    mid = srt[int(0.3 * len(srt)):int(0.7 * len(srt))]
    at = int(np.argmax(np.diff(mid)))
    iso = float(np.float32(0.5 * (mid[at] + mid[at + 1])))
    mesh = M.extract_mesh(m.query_sdf, cfg, m.bounding_box, marching_cube_bound=mcb, color_func=m.render_surface_color, voxel_size=0.4, isolevel=iso)
    want = MN.extract_mesh(ora.query_sdf, cfg, ora.bounding_box, table, marching_cube_bound=mcb, color_func=ora.render_surface_color, voxel_size=0.4,
                           isolevel=iso)
    assert len(want["faces"]) > 0 and float(np.abs(o["vol"] - iso).min()) > 2e-5
    assert np.array_equal(mesh.faces, want["faces"])
    n_dev = M.vertex_normals(torch.from_numpy(mesh.vertices).to(gpu), torch.from_numpy(mesh.faces).to(gpu)).cpu().numpy()
    assert np.abs(n_dev - MN.vertex_normals(mesh.vertices, mesh.faces)).max() < 1e-9
    diff = np.abs(mesh.vertex_colors[:, :3].astype(np.float64) - np.round(np.clip(want["colors"], 0, 1) * 255.0))
    assert diff.max() <= 1.0, diff.max()


@pytest.mark.parametrize("case", list(range(4)))
def test_extract_mesh_random_configs(gpu, case):
    """N4 over drawn scene boxes, marching-cubes bounds, voxel sizes / resolutions, metric transforms and isolevels: the SDF
    volume against the oracle, marching cubes on the device's own volume bit-exact against the numpy restatement, the vertex
    transform and the colour branch against the oracle's restatement of extract_mesh."""
    from naruto_amd import config as C, mesh as M
    from oracle import mesh_numpy as MN
    table = H.load_golden("mc_table")
    rs = np.random.RandomState(800 + case)
    ext, lo = rs.uniform(2.0, 6.0, 3), rs.uniform(-3.0, 1.0, 3)
    cfg = C.office0_config()
    cfg["mapping"]["bound"] = [[float(lo[i]), float(lo[i] + ext[i])] for i in range(3)]
    cfg["grid"]["hash_size"] = 12
    cfg["data"]["sc_factor"], cfg["data"]["translation"] = float(rs.choice([1.0, 2.0])), float(rs.choice([0.0, 0.5]))
    ora = H.make_oracle(cfg, 0.25, 800 + case).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    shrink = rs.uniform(0.0, 0.15, (3, 2)) * ext[:, None]
    mcb = torch.tensor([[lo[i] + shrink[i, 0], lo[i] + ext[i] - shrink[i, 1]] for i in range(3)], dtype=torch.float32)
    voxel = float(rs.choice([0.25, 0.4]))
    # the volume the device meshes
    tx, ty, tz = M.get_voxels(mcb[0, 1], mcb[0, 0], mcb[1, 1], mcb[1, 0], mcb[2, 1], mcb[2, 0], voxel)
    bb = m.bounding_box.cpu()
    axes = [((t - bb[i, 0]) / (bb[i, 1] - bb[i, 0])).to(gpu) for i, t in enumerate((tx, ty, tz))]
    with torch.no_grad():
        vol = m.query_sdf(M.lattice_points(*axes)[:, None, :]).reshape(tx.numel(), ty.numel(), tz.numel()).contiguous()
    o = MN.extract_mesh(ora.query_sdf, cfg, ora.bounding_box, table, marching_cube_bound=mcb, voxel_size=voxel, isolevel=1e9, render_uncert=False)
    H.assert_close(vol, o["vol"], TOL_OUT, f"case {case}: sdf volume")
    srt = np.sort(o["vol"].reshape(-1).astype(np.float64))
    mid = srt[int(0.3 * len(srt)):int(0.7 * len(srt))]
    at = int(np.argmax(np.diff(mid)))
    iso = float(np.float32(0.5 * (mid[at] + mid[at + 1])))                      # in the widest gap between lattice values: same topology on both sides
    v, f = M.marching_cubes(vol, iso, 3.0)
    ov, of = MN.marching_cubes(vol.cpu().numpy(), iso, 3.0, table)
    assert np.array_equal(v.cpu().numpy(), ov) and np.array_equal(f.cpu().numpy(), of) and len(of) > 0
    mesh = M.extract_mesh(m.query_sdf, cfg, m.bounding_box, marching_cube_bound=mcb, color_func=m.query_color, voxel_size=voxel, isolevel=iso)
    want = MN.extract_mesh(ora.query_sdf, cfg, ora.bounding_box, table, marching_cube_bound=mcb, color_func=ora.query_color, voxel_size=voxel, isolevel=iso)
    if float(np.abs(o["vol"] - iso).min()) > 2e-5:                               # otherwise fp32 noise may flip a corner: compare the surface loosely
        assert np.array_equal(mesh.faces, want["faces"])
        H.assert_close(mesh.vertices, want["vertices"], 5e-3 * voxel, f"case {case}: vertices")
        assert np.abs(mesh.vertex_colors[:, :3].astype(np.float64) - np.round(np.clip(want["colors"], 0, 1) * 255.0)).max() <= 1.0
    else:
        assert abs(len(mesh.faces) - len(want["faces"])) <= 0.02 * len(want["faces"]) + 8


def test_deferred_min_uncert_assert(gpu):
    """scene_rep.py:280 asserts uncert_map.min() > 0 inside forward; here the value is copied to the host asynchronously and
    checked when it has landed: no sync per iteration, and a violation is still reported (within a few iterations, or at once
    with check_asserts(block=True) / strict_assert)."""
    from naruto_amd.trainer import MappingTrainer, pack_rays
    cfg = H.office_cfg(12, perturb=1.0)
    tr = MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"], dtype=torch.float32), gpu, 0.1, fused_adam=True)
    rays = {k: torch.from_numpy(v).to(gpu) for k, v in syn.random_rays(64, cfg["mapping"]["bound"], seed=5).items()}
    o, d, s, t = pack_rays(rays["rays_o"], rays["rays_d"], rays["target_rgb"], rays["target_d"])
    for _ in range(3):
        tr.step(o, d, s, t, smooth=True, n_rays_total=64)
    tr.model.check_asserts(block=True)                                   # healthy so far
    assert not tr.model._min_uncert_queue
    with torch.no_grad():
        tr.model.uncert_grid.fill_(float("nan"))                         # every ray's uncert_map becomes NaN: "min() > 0" is false
    tr.step(o, d, s, t, smooth=True, n_rays_total=64)                    # queues the bad value; may or may not have landed yet
    with pytest.raises(AssertionError, match="uncert_map.min"):
        tr.step(o, d, s, t, smooth=True, n_rays_total=64)
        tr.model.check_asserts(block=True)


# --------------------------------------------------------------------------------------------- the unchanged caller (coslam.py:361-399)
def _weights_from(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("S_d", [32, 117])
def test_fused_train_node_equals_the_modular_operators(gpu, S_d):
    """model.forward in training mode: the ONE autograd node over naruto_train_forward / naruto_train_backward (the unchanged caller's
    route) against the modular operators (field query | composite + losses) on the same rays and jitter draw -- losses, rendered maps
    and every gradient, with the reference's get_loss_from_ret weights arriving as the cotangents of the scalar losses."""
    cfg = H.office_cfg(14, perturb=1.0, n_samples_d=S_d)
    ora = H.make_oracle(cfg, 0.2, 41)
    rays = syn.random_rays(515, cfg["mapping"]["bound"], seed=41, zero_depth_frac=0.1)
    t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    rand = torch.rand(515, S_d + 11, device=gpu, generator=torch.Generator(gpu).manual_seed(5))
    out = {}
    for fused in (False, True):
        m = H.make_hip_from_oracle(cfg, ora, gpu).train()
        m.fused_train = fused
        m.strict_assert = True
        ret = m.forward(*t, rand=rand)
        S.total_loss(ret, cfg["training"]).backward()
        out[fused] = (ret, H.hip_grads(m))
    for k in ("rgb", "depth", "rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "psnr", "uncert_loss"):
        H.assert_close(out[True][0][k].reshape(-1), out[False][0][k].reshape(-1), 1e-6, f"node.{k}", rel=1e-5)
    for k, g in out[True][1].items():
        want = out[False][1][k]
        H.assert_close(g, want, 2e-6 * float(want.abs().max()), f"node.grad.{k}", rel=1e-4)


def test_fused_train_node_autograd_contract(gpu):
    """What an unchanged caller may do with the node: accumulate into existing .grad (no zero_grad in between), differentiate a SUBSET
    of the losses, read ret after the next forward (outputs are fresh tensors), second backward over the same graph; and what it may
    not: backward over a graph whose buffers a later forward has reused, cotangents on the rendered rgb / depth."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, 7)
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    ref = H.make_hip_from_oracle(cfg, ora, gpu).train()
    ref.fused_train = False
    rays = syn.random_rays(130, cfg["mapping"]["bound"], seed=7, zero_depth_frac=0.1)
    t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    # a subset of the losses with odd weights, twice without zero_grad: gradients accumulate
    for model in (m, ref):
        for rep in range(2):
            ret = model.forward(*t)
            (3.0 * ret["sdf_loss"] + 0.25 * ret["uncert_loss"]).backward()
    for k, g in H.hip_grads(m).items():
        want = H.hip_grads(ref)[k]
        H.assert_close(g, want, 2e-6 * float(want.abs().max()) + 1e-30, f"contract.accumulate.{k}", rel=1e-4)
    # outputs are fresh tensors: a kept ret is not overwritten by the next forward of the same ray count
    ret1 = m.forward(*t)
    keep = {k: ret1[k].clone() for k in ("rgb", "depth", "rgb_loss")}
    t2 = [a.clone() for a in t]
    t2[3] = t2[3] * 0.5
    ret2 = m.forward(*t2)
    for k, v in keep.items():
        assert torch.equal(ret1[k], v), k
    assert not torch.equal(ret2["depth"], ret1["depth"])
    # ... but its graph's buffers are gone
    with pytest.raises(RuntimeError, match="later forward"):
        ret1["rgb_loss"].backward()
    ret2["rgb_loss"].backward(retain_graph=True)
    ret2["rgb_loss"].backward()                         # second backward over the same (latest) graph
    with pytest.raises(NotImplementedError, match="fused_train"):
        m.forward(*t)["rgb"].sum().backward()
    # the dot-product form MappingTrainer's autograd path uses
    m.zero_grad()
    ref.zero_grad()
    w = torch.tensor([5.0, 0.1, 1000.0, 10.0, 0.0, 0.005, 0.0, 0.0, 0.0, 0.0], device=gpu)
    for model in (m, ref):
        torch.dot(model.forward(*t)["_losses"], w).backward()
    for k, g in H.hip_grads(m).items():
        want = H.hip_grads(ref)[k]
        H.assert_close(g, want, 2e-6 * float(want.abs().max()) + 1e-30, f"contract.dot.{k}", rel=1e-4)


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
def test_dropin_caller_tracks_the_oracle(gpu, optimizer):
    """The reference's UNCHANGED loop body (tools/dropin_caller.py = coslam.py:154-174, 361-399 + Co-SLAM's torch smoothness through
    query_sdf(embed=True) autograd, loss.backward(retain_graph=True), Adam, the uncertainty grid's Adam every 5th iteration) around
    NarutoFieldHIP against the oracle driven by the same loop with the same host random draws: per-iteration losses and the
    parameters after seven iterations."""
    from dropin_caller import DropInCaller
    cfg = H.office_cfg(12)
    trc = cfg["training"]
    ora = H.make_oracle(cfg, 0.1, 31).train()
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    caller = DropInCaller(m, cfg, 0.1, optimizer=optimizer)            # init_uncert_grid_optim re-creates the grid (coslam.py:240-243)
    with torch.no_grad():
        m.uncert_grid.copy_(ora.uncert_grid)
    g1, g2 = ora.param_groups()
    o_map = torch.optim.Adam(g1, betas=(0.9, 0.99))
    o_unc = torch.optim.Adam(g2, lr=1)
    for it in range(7):
        rays = syn.random_rays(256, cfg["mapping"]["bound"], seed=100 + it, zero_depth_frac=0.05)
        t = {k: torch.from_numpy(v) for k, v in rays.items()}
        torch.manual_seed(1000 + it)
        ret_o = ora.forward(t["rays_o"], t["rays_d"], t["target_rgb"], t["target_d"])
        sm = S.smoothness(ora, trc["smooth_pts"], trc["smooth_vox"], trc["smooth_margin"], torch.rand(3), torch.rand((1, 1, 1, 3)).reshape(3))
        loss_o = S.total_loss(ret_o, trc, smooth_term=sm)
        loss_o.backward()
        o_map.step()
        o_map.zero_grad()
        if (it + 1) % 5 == 0:
            o_unc.step()
            o_unc.zero_grad()
        torch.manual_seed(1000 + it)
        ret_h, loss_h = caller.ba_iteration(it, *(t[k].to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")))
        for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "uncert_loss"):
            H.assert_close(ret_h[k].reshape(-1), ret_o[k].reshape(-1), 1e-5, f"dropin.iter{it}.{k}", rel=2e-3)
        H.assert_close(loss_h.reshape(-1), loss_o.reshape(-1), 1e-5, f"dropin.iter{it}.total", rel=2e-3)
    m.check_asserts(block=True)

    def frac_within(a, b, tol):
        return ((a.detach().cpu() - b.detach()).abs() <= tol).float().mean().item()
    assert frac_within(m.decoder.sdf_net.model[0].weight, ora.sdf_w0, 2e-3) > 0.995
    assert frac_within(m.decoder.color_net.model[0].weight, ora.col_w0, 2e-3) > 0.995
    assert frac_within(m.uncert_grid, ora.uncert_grid, 2e-2) > 0.995
    # table entries the rays miss see only the smoothness term's gradient (weight 1e-6: ~1e-12, at the noise level of its own
    # summation order) and Adam (eps 1e-15) turns a sign flip there into a full +-lr step: the bulk criterion is looser here than in
    # the trajectories without the term, the per-iteration losses above are not
    assert frac_within(m.embed_fn.params, ora.table, 2e-3) > 0.98
    assert float((m.embed_fn.params.detach().cpu() - ora.table.detach()).abs().mean()) < 2e-4


def test_dropin_variants_run_and_agree(gpu):
    """INTEGRATION.md's optional one-line changes after the swap (FusedAdam; the fused smoothness) leave the first iteration's render
    losses untouched and keep training: same rgb / depth / sdf / fs / uncert losses at iteration 0 (the smoothness lattice is drawn
    differently), finite and decreasing total afterwards."""
    from dropin_caller import DropInCaller
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.1, 3)
    rays = syn.random_rays(300, cfg["mapping"]["bound"], seed=3)
    t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    first = {}
    for opt, sm in (("torch", "reference"), ("fused", "reference"), ("fused", "fused")):
        m = H.make_hip_from_oracle(cfg, ora, gpu).train()
        caller = DropInCaller(m, cfg, 0.1, optimizer=opt, smoothness=sm)
        totals = []
        for i in range(12):
            ret, loss = caller.ba_iteration(i, *t)
            if i == 0:
                first[(opt, sm)] = {k: float(ret[k].detach()) for k in ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "uncert_loss")}
            totals.append(float(loss))
        m.check_asserts(block=True)
        assert all(np.isfinite(totals)) and totals[-1] < totals[0], totals
    base = first[("torch", "reference")]
    for key, d in first.items():
        for k, v in d.items():
            assert abs(v - base[k]) <= 1e-6 + 1e-5 * abs(base[k]), (key, k, v, base[k])


def test_running_min_uncert_is_checked(gpu):
    """The reference asserts uncert_map.min() > 0 in every forward (scene_rep.py:280).  Here every fused forward folds its minimum
    into one device word and the host reads it late: a violation in ANY iteration -- not only the sampled ones -- is reported."""
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.2, 9)
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    rays = syn.random_rays(64, cfg["mapping"]["bound"], seed=9)
    t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    m.assert_every = 4
    for i in range(5):
        m.forward(*t)
    m.check_asserts(block=True)
    assert float(m.min_uncert_running()) > 0
    good = m.uncert_grid.detach().clone()
    with torch.no_grad():
        m.uncert_grid.fill_(float("nan"))               # softplus(nan) + 0.01 = nan: the assertion must fire
    m.forward(*t)                                       # call 6: not a sampled one
    with torch.no_grad():
        m.uncert_grid.copy_(good)
    m.forward(*t)
    with pytest.raises(AssertionError, match="uncert_map"):
        m.forward(*t)                                   # call 8 queues the running minimum ...
        m.check_asserts(block=True)                     # ... which still carries the NaN of call 6


# --------------------------------------------------------------------------------------------- the mapping iteration end to end
def _ba_scene(cfg, gpu, Hh=48, Ww=64, n_kf=6, R=400, seed=0):
    """A small device-resident keyframe store + current frame + poses + planner volume."""
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    rs = np.random.RandomState(seed)
    store = KeyFrameStoreHIP(cfg, Hh, Ww, num_kf=n_kf + 2, num_rays_to_save=R, device=gpu, seed=11)

    def frame(fid):
        d = rs.normal(size=(1, Hh, Ww, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        depth = rs.uniform(0.4, 2.5, (1, Hh, Ww)).astype(np.float32)
        depth[rs.uniform(size=depth.shape) < 0.1] = 0.0
        return {"direction": torch.from_numpy(d), "rgb": torch.from_numpy(rs.uniform(size=(1, Hh, Ww, 3)).astype(np.float32)),
                "depth": torch.from_numpy(depth), "frame_id": torch.tensor([fid])}
    every = cfg["mapping"]["keyframe_every"]
    for k in range(n_kf):
        store.add_keyframe(frame(k * every), filter_depth=cfg["mapping"]["filter_depth"])
    cur = frame(n_kf * every)
    current = torch.cat([cur["direction"], cur["rgb"], cur["depth"][..., None]], -1).reshape(-1, 7)
    bound = np.array(cfg["mapping"]["bound"], np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (n_kf + 1, 1, 1))
    for p in poses:
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        p[:3, :3] = q.astype(np.float32)
        p[:3, 3] = bound[:, 0] + (0.3 + 0.4 * rs.uniform(size=3)) * (bound[:, 1] - bound[:, 0])
    vol = (rs.uniform(0, 3, (49, 56, 35)) * (rs.uniform(size=(49, 56, 35)) < 0.5)).astype(np.float32)
    return store, current, torch.from_numpy(poses), vol


@pytest.mark.parametrize("active", [False, True])
def test_fused_ba_iteration_equals_its_pieces(gpu, active):
    """naruto_amd.ba_loop.FusedBA -- ray assembly (N2) -> active ray selection (N1) -> training iteration recorded in ONE hipGraph,
    draws keyed by the trainer's device-side iteration counter, counts read from device memory -- against the same three operators
    launched one by one: identical batches, identical losses, bit-identical parameters after two global_BA calls between which the
    store grows by a keyframe (no re-capture: the ray count stays)."""
    from naruto_amd import trainer
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    from naruto_amd.ba_loop import FusedBA
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["mapping"].update(sample=256, min_pixels_cur=40, filter_depth=True, keyframe_every=5)
    bound = torch.tensor(cfg["mapping"]["bound"])
    twins = []
    for use_graph in (True, False):
        torch.manual_seed(33)
        tr = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
        store, current, poses, vol = _ba_scene(cfg, gpu, n_kf=8)
        smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=48, oversample_mul=4) if active else None
        # (the graph twin draws and selects in ONE launch, naruto_assemble_select -- round 5, off by default --, the eager twin in two)
        # and has every iteration's last launch assemble the NEXT iteration's batch (prefetch, round 5), the eager twin assembles its own
        twins.append((FusedBA(tr, store, smp, max_poses=64, use_graph=use_graph, one_launch_prologue=use_graph, prefetch=use_graph), current, poses, vol))
    (a, cur, poses, vol), (b, _, _, _) = twins
    b.trainer.model.load_state_dict(a.trainer.model.state_dict())
    b.trainer.iter_state.copy_(a.trainer.iter_state)
    for ba in (a, b):
        n_cur, n_train = ba.prepare(cur, poses, vol if active else None)
        assert n_cur == (160 if active else 40) and n_train == (256 + 40 if active else 256 + 40)
    assert a.trainer._graphs is not None and b.trainer._graphs is None
    losses = {}
    for tag, ba in (("graph", a), ("eager", b)):
        ls = []
        for i in range(7):
            ret, loss = ba.iteration(i)
            ls.append(float(loss))
        losses[tag] = ls
    assert losses["graph"] == losses["eager"], losses
    assert len(set(losses["graph"])) == 7, "every iteration draws another batch"
    # the batch the last replay trained on, recomputed from the host-keyed operators: seed / counter of the iteration state BEFORE it
    st = b.trainer.iter_state.cpu()
    bufs = a.trainer.ray_buffers()
    # (without active rays the prefetching twin's input buffers already hold the batch of the iteration that WOULD come next; with them
    # the prefetched draw sits in the stage and the input buffers still hold the last selection)
    seed, counter = int(st[0]), int(st[1]) - (1 if active else 0)
    store = b.store
    saved_seed, saved_counter = store.seed, store.counter
    store.seed, store.counter = seed, counter - 1            # assemble_batch pre-increments its host counter
    n_cur = 160 if active else 40
    o, d, s_, t_, _ = store.assemble_batch(b.sample_num, b.current, b.poses[:poses.shape[0]], b.min_pixels_cur, filter_depth=True,
                                           n_cur=n_cur, n_cur_pop=b._n_cur_pop)
    store.seed, store.counter = saved_seed, saved_counter
    if active:
        o, d, s_, t_ = b.sampler.sample_rays(o, d, s_, t_, n_cur, None, b.bbox)
    for got, want, k in zip(bufs, (o, d, s_, t_), ("rays_o", "rays_d", "target_rgb", "target_d")):
        assert torch.equal(got, want.reshape(got.shape)), k
    # a second global_BA call after the store grew by a keyframe: same ray count -> same graph, new counts from device memory
    for ba in (a, b):
        fr_rs = np.random.RandomState(5)
        Hh, Ww = 48, 64
        dirs = fr_rs.normal(size=(1, Hh, Ww, 3)).astype(np.float32)
        ba.store.add_keyframe({"direction": torch.from_numpy(dirs), "rgb": torch.from_numpy(fr_rs.uniform(size=(1, Hh, Ww, 3)).astype(np.float32)),
                               "depth": torch.from_numpy(fr_rs.uniform(0.5, 2.0, (1, Hh, Ww)).astype(np.float32)), "frame_id": torch.tensor([40])}, filter_depth=True)
        poses2 = torch.cat([poses, poses[-1:]], 0)
        graphs_before = ba.trainer._graphs
        ba.global_BA(cur, poses2, n_iters=6, uncert_vol=vol if active else None)
        assert ba.trainer._graphs is graphs_before, "the ray count did not change: no re-capture"
    for (n, p), (_, q) in zip(a.trainer.model.named_parameters(), b.trainer.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: graph replay != eager launches"
    # a call of the CONFIGURED length: the graph twin replays ONE graph that holds all mapping.iters iterations (round 5)
    assert a.trainer.chain_length() == (cfg["mapping"]["iters"] if a.call_graph else 0) and b.trainer.chain_length() == 0      # (NARUTO_BA_CALL_GRAPH=0: iteration by iteration)
    outs = [ba.global_BA(cur, poses2, uncert_vol=vol if active else None) for ba in (a, b)]
    assert float(outs[0][1]) == float(outs[1][1]), "last iteration's loss: call graph != eager launches"
    for (n, p), (_, q) in zip(a.trainer.model.named_parameters(), b.trainer.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: call graph != eager launches"
    assert torch.equal(a.trainer.iter_state, b.trainer.iter_state)
    a.trainer.model.check_asserts(block=True)


@pytest.mark.parametrize("active", [False, True])
def test_fused_ba_prefetch_survives_eviction_and_close(gpu, active):
    """Two advisor findings of round 5.  (i) The eager prefetch rides on ONE TrainStep; the trainer's cache (keyed on ray count / smoothness,
    LRU of max_cached_steps) may hand the next iteration another one: every iteration must then still train on its own freshly drawn batch
    (trajectory = the twin that assembles every batch itself, bit for bit), not silently on stale rays.  (ii) The NarutoRayBatch the fused
    optimiser points at lives on the TrainStep, and close() / dropping the FusedBA disarms it: a later trainer.step on the same TrainStep
    neither reads freed host memory nor overwrites anybody's ray buffers."""
    import gc
    from naruto_amd import trainer
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    from naruto_amd.ba_loop import FusedBA
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["mapping"].update(sample=256, min_pixels_cur=40, filter_depth=True, keyframe_every=5)
    bound = torch.tensor(cfg["mapping"]["bound"])
    twins = []
    for prefetch in (True, False):
        torch.manual_seed(35)
        tr = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
        store, current, poses, vol = _ba_scene(cfg, gpu, n_kf=8)
        smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=48, oversample_mul=4) if active else None
        twins.append((FusedBA(tr, store, smp, max_poses=64, use_graph=False, prefetch=prefetch), current, poses, vol))
    (a, cur, poses, vol), (b, _, _, _) = twins
    b.trainer.model.load_state_dict(a.trainer.model.state_dict())
    b.trainer.iter_state.copy_(a.trainer.iter_state)
    a.trainer.max_cached_steps = 1                       # every other ray count evicts the armed TrainStep
    rays = syn.random_rays(64, cfg["mapping"]["bound"], seed=3)
    other = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
    losses = {"a": [], "b": []}
    for tag, ba in (("a", a), ("b", b)):
        ba.prepare(cur, poses, vol if active else None)
        for i in range(6):
            if i in (2, 4):
                # a foreign step of another size between two iterations (both twins, so the trajectories stay comparable): on twin a it evicts
                # the TrainStep whose finishing launch was to draw iteration i's batch
                ba.trainer.step(*other, smooth=True, uncert_step=False)
            ret, loss = ba.iteration(i)
            losses[tag].append(float(loss))
    assert losses["a"] == losses["b"], losses
    assert len(set(losses["a"])) == 6, "every iteration draws another batch"
    for (n, p), (_, q) in zip(a.trainer.model.named_parameters(), b.trainer.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: prefetching twin (with evictions) != the twin that assembles every batch"
    # (ii) the struct lives on the TrainStep; close() disarms
    ts = a._armed
    assert ts is not None and ts.opt.next_batch and ts._next_batch_keep is not None
    bufs = [t.clone() for t in a._eager_bufs]
    stage = [t.clone() for t in a._stage] if active else None
    tr_a = a.trainer
    n_train = bufs[0].shape[0]
    a.close()
    assert not ts.opt.next_batch and ts._next_batch_keep is None
    eager_bufs, stage_live = a._eager_bufs, a._stage
    del a
    gc.collect()
    mine = [t.clone() for t in bufs]
    tr_a.step(*mine, smooth=True, uncert_step=False)     # same ray count: the TrainStep the FusedBA had armed
    torch.cuda.synchronize()
    for t0, t1 in zip(bufs, eager_bufs):
        assert torch.equal(t0, t1), "a disarmed TrainStep no longer draws into the FusedBA's ray buffers"
    if active:
        for t0, t1 in zip(stage, stage_live):
            assert torch.equal(t0, t1), "... nor into its stage"
    assert tr_a._train_step(n_train, True) is ts


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_stale_fused_ba_does_not_disarm_the_live_one(gpu, use_graph):
    """The trainer's cache hands the SAME TrainStep to a second FusedBA on the same trainer.  What rides on its backward belongs to the
    object that attached it last (ops.TrainStep.attach): close() of the first object, or the finaliser of any other, neither disarms the
    second one's prefetch nor drops the graphs it captured -- the trajectory is that of a trainer that only ever had one FusedBA, bit for bit.
    And when the graphs ARE taken away (trainer._graphs = None), the next iteration captures again instead of failing."""
    import gc
    from naruto_amd import trainer
    from naruto_amd.ba_loop import FusedBA
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["mapping"].update(sample=256, min_pixels_cur=40, filter_depth=True, keyframe_every=5)
    bound = torch.tensor(cfg["mapping"]["bound"])
    twins = []
    for _ in range(2):
        torch.manual_seed(37)
        tr = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
        store, current, poses, _ = _ba_scene(cfg, gpu, n_kf=8)
        twins.append((tr, store))
    (tr_a, store_a), (tr_b, store_b) = twins
    tr_b.model.load_state_dict(tr_a.model.state_dict())
    tr_b.iter_state.copy_(tr_a.iter_state)

    def make(tr, store):
        ba = FusedBA(tr, store, None, max_poses=64, use_graph=use_graph)
        assert ba.prepare(current, poses) == (40, 296)
        return ba
    stale = make(tr_a, store_a)
    live = make(tr_a, store_a)
    only = make(tr_b, store_b)
    ts = tr_a._train_step(296, True)
    assert ts.opt.next_batch, "the prefetch rides on the TrainStep both objects were handed"
    losses = {"a": [float(live.iteration(i)[1]) for i in range(2)]}
    graphs = tr_a._graphs
    assert (graphs is not None) == use_graph
    stale.close()
    third = FusedBA(tr_a, store_a, None, max_poses=64, use_graph=use_graph)
    del third
    gc.collect()
    assert tr_a._graphs is graphs, "a stale close() dropped the live object's graphs"
    assert ts.opt.next_batch, "a stale close() disarmed the live object's prefetch"
    assert ts.riders_of(live)[0] is ts._next_batch_keep is not None and ts.riders_of(stale) == (None, None)
    losses["a"] += [float(live.iteration(i)[1]) for i in range(2, 6)]
    losses["b"] = [float(only.iteration(i)[1]) for i in range(6)]
    if use_graph:
        tr_a._graphs = None                      # (what another driver of the same trainer does): iteration 6 captures again
        losses["a"].append(float(live.iteration(6)[1]))
        losses["b"].append(float(only.iteration(6)[1]))
        assert tr_a._graphs is not None
    assert losses["a"] == losses["b"], losses
    assert len(set(losses["a"])) == len(losses["a"]), "every iteration draws another batch"
    for (n, p), (_, q) in zip(tr_a.model.named_parameters(), tr_b.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: a trainer with a stale FusedBA != a trainer with one"


def test_active_ray_keys_looked_up_by_the_assembly(gpu):
    """NarutoRayBatch.keys_out + naruto_active_ray_select_keyed (round 5): the candidates' keys looked up by the batch assembly, while the
    rows are in registers, and the selection started from them -- the same selected batch, bit for bit, as assembly | selection with its
    own lookup; keys_out leaves every other output of the assembly untouched."""
    from naruto_amd import _lib
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["mapping"].update(sample=256, min_pixels_cur=40, filter_depth=True, keyframe_every=5)
    store, current, poses, vol = _ba_scene(cfg, gpu, n_kf=8)
    smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=48, oversample_mul=4)
    smp.set_volume(torch.from_numpy(vol), gpu)
    bbox = [[float(b[0]), float(b[1])] for b in cfg["mapping"]["bound"]]
    sample_num, min_cur = smp.oversample_num, smp.min_pixels_cur
    cur = current.to(gpu)
    pos = poses.to(gpu)
    store.seed, store.counter = 1234, 7
    o, d, s_, t_, n_cur = store.assemble_batch(sample_num, cur, pos, min_cur, filter_depth=True)
    want = smp.sample_rays(o, d, s_, t_, n_cur, None, bbox)
    keys = torch.full((o.shape[0],), -1, dtype=torch.int32, device=gpu)
    store.counter = 7
    o2, d2, s2, t2, n_cur2 = store.assemble_batch(sample_num, cur, pos, min_cur, filter_depth=True, keys=smp.key_lookup(o.shape[0], n_cur, bbox, keys))
    assert n_cur2 == n_cur
    for a_, b_ in ((o, o2), (d, d2), (s_, s2), (t_, t2)):
        assert torch.equal(a_, b_)
    n_tail = -((-n_cur) // smp.oversample_mul)
    n_cand = o.shape[0] - n_tail - smp.base_sample_num
    assert (keys[n_cand:] == -1).all(), "keys beyond the candidates are not written"
    got = smp.sample_rays(o2, d2, s2, t2, n_cur, None, bbox, keys=keys)
    for a_, b_, k in zip(got, want, ("rays_o", "rays_d", "target_s", "target_d")):
        assert torch.equal(a_, b_), k
    # errors: too many candidates / NULL keys
    lib = _lib.load()
    big = 2 * 8192 + 1024
    z = torch.zeros(big * 3, device=gpu)
    rc = lib.naruto_active_ray_select_keyed(big, 512, 48, 8, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), keys.data_ptr(), z.data_ptr(), z.data_ptr(),
                                            z.data_ptr(), z.data_ptr(), None)
    assert rc != 0 and b"candidates" in lib.naruto_last_error()


def test_fused_ba_back_to_back_calls_and_volume_refresh(gpu):
    """Two advisor findings of round 3.  (i) FusedBA.prepare refreshes {n_kf, n_poses, n_cur_pop} through pinned staging with an
    asynchronous copy: two global_BA calls issued back to back WITHOUT a host sync in between (filter_depth off, so nothing reads back)
    must each train on the counts of their own call -- the second call's staging write may not overtake the first call's queued copy.
    (ii) ActiveRaySamplerHIP.set_volume with the device spelled "cuda" (not "cuda:0") must refresh the pinned tensor IN PLACE, the
    pointer a captured launch reads; a volume of another shape re-captures."""
    from naruto_amd import trainer
    from naruto_amd.active_ray_sampler import ActiveRaySamplerHIP
    from naruto_amd.ba_loop import FusedBA
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["mapping"].update(sample=256, min_pixels_cur=40, filter_depth=False, keyframe_every=5)
    bound = torch.tensor(cfg["mapping"]["bound"])

    def make(use_graph):
        torch.manual_seed(5)
        tr = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
        store, current, poses, vol = _ba_scene(cfg, gpu, n_kf=8)
        smp = ActiveRaySamplerHIP(config=cfg, num_uncert_sample=48, oversample_mul=4)
        return FusedBA(tr, store, smp, max_poses=64, use_graph=use_graph), current, poses, vol
    (a, cur, poses, vol), (b, _, _, _) = make(True), make(False)
    b.trainer.model.load_state_dict(a.trainer.model.state_dict())
    b.trainer.iter_state.copy_(a.trainer.iter_state)
    fr = np.random.RandomState(9)
    Hh, Ww = 48, 64
    extra = {"direction": torch.from_numpy(fr.normal(size=(1, Hh, Ww, 3)).astype(np.float32)), "rgb": torch.from_numpy(fr.uniform(size=(1, Hh, Ww, 3)).astype(np.float32)),
             "depth": torch.from_numpy(fr.uniform(0.5, 2.0, (1, Hh, Ww)).astype(np.float32)), "frame_id": torch.tensor([40])}
    poses2 = torch.cat([poses, poses[-1:]], 0)
    vol_gpu = torch.from_numpy(vol)
    for ba, sync in ((a, False), (b, True)):
        ba.sampler.set_volume(vol_gpu, "cuda")                         # the spelling without an index
        ptr = ba.sampler._vol_dev.data_ptr()
        ba.global_BA(cur, poses, n_iters=4, uncert_vol=vol_gpu * 0.5)  # refresh: same shape -> in place
        assert ba.sampler._vol_dev.data_ptr() == ptr, "set_volume reallocated a volume of the same shape and device"
        if sync:
            torch.cuda.synchronize()
        ba.store.add_keyframe(extra, filter_depth=False)
        ba.global_BA(cur, poses2, n_iters=4, uncert_vol=vol_gpu * 0.25)
        if sync:
            torch.cuda.synchronize()
        ba.global_BA(cur, poses2, n_iters=4, uncert_vol=vol_gpu)
    torch.cuda.synchronize()
    assert torch.equal(a.sampler._vol_dev, b.sampler._vol_dev)
    for (n, p), (_, q) in zip(a.trainer.model.named_parameters(), b.trainer.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: back-to-back graph replays != synchronised eager calls"
    # another shape: a new tensor, and the graph is captured again
    graphs = a.trainer._graphs
    small = torch.from_numpy(vol[:-1].copy())
    a.global_BA(cur, poses2, n_iters=2, uncert_vol=small)
    assert a.trainer._graphs is not graphs, "the captured launch still reads the volume of the old shape"


# --------------------------------------------------------------------------------------------- matched reconstruction accuracy
def test_matched_reconstruction_accuracy(gpu):
    """BASELINE north_star: the speed-up is claimed "at matched reconstruction accuracy".  tests/accuracy_study.py maps a consistent analytic
    scene (box room + sphere, closed-form RGB-D frames from a ring of poses) with the reference's schedule (first_frame_mapping, then one
    global_BA call per keyframe; jitter and smoothness on) through the CPU oracle and through MappingTrainer (fp32, bf16) from the SAME
    initial parameters over the SAME batches; this is a reduced schedule of it (1024 rays, 8 frames, 60 + 7 x 8 iterations).  Checked: the
    map is LEARNT (error of the predicted sdf against the TRUE distance field and held-out depth L1 collapse against the untrained field),
    and HIP fp32 / bf16 end within the run-to-run band of the oracle on every metric -- eval_mad's mean |sdf| at ground-truth surface points
    (eval_mad.py:84-90), the band sdf error, the held-out depth L1 -- with 1 % NaN depths costing nothing (a NaN depth is a
    missing one).  The full schedule's numbers are in profiles/r04_accuracy_study.json and README.md."""
    import accuracy_study as A
    res = A.study(n_rays=1024, n_frames=8, n_first=60, n_ba=8, n_surface=40000, extra_seeds=(1,), oracle_threads=16, with_nan=True, verbose=False)
    r, u = res["runs"], res["untrained"]
    for name in ("hip_fp32", "hip_bf16", "oracle_cpu_fp32", "hip_fp32_jitter_seed1", "hip_fp32_1pct_nan_depth"):
        assert r[name]["band_sdf_err_cm"] < 0.75 * u["band_sdf_err_cm"], (name, r[name], u)
        assert r[name]["heldout_depth_l1_cm"] < 0.1 * u["heldout_depth_l1_cm"], (name, r[name], u)
    o = r["oracle_cpu_fp32"]
    # run-to-run band of this reduced schedule: two jitter streams of the SAME implementation differ by up to ~10 % in MAD / depth L1
    for name in ("hip_fp32", "hip_bf16", "hip_fp32_1pct_nan_depth"):
        assert abs(r[name]["mad_cm"] / o["mad_cm"] - 1.0) < 0.2, (name, r[name]["mad_cm"], o["mad_cm"])
        assert abs(r[name]["band_sdf_err_cm"] / o["band_sdf_err_cm"] - 1.0) < 0.1, (name, r[name]["band_sdf_err_cm"], o["band_sdf_err_cm"])
        assert abs(r[name]["heldout_depth_l1_cm"] / o["heldout_depth_l1_cm"] - 1.0) < 0.35, (name, r[name]["heldout_depth_l1_cm"], o["heldout_depth_l1_cm"])
        assert abs(r[name]["heldout_psnr_db"] - o["heldout_psnr_db"]) < 1.0, (name, r[name]["heldout_psnr_db"], o["heldout_psnr_db"])
    # the planner's uncertainty volume: rank correlation between implementations no worse than between two jitter streams of ONE
    # implementation (measured: 0.71 - 0.81 HIP vs HIP here, 0.48 - 0.60 over the full schedule; HIP vs oracle 0.74 - 0.78)
    sp = res["uncert_volume_spearman"]
    assert sp["hip_fp32_vs_oracle"] > 0.5 and sp["hip_bf16_vs_oracle"] > 0.5, sp
    assert sp["hip_fp32_vs_oracle"] > sp["hip_fp32_vs_hip_fp32_seed1"] - 0.25, sp


# --------------------------------------------------------------------------------------------- configs[2] at its own size
def test_configs2_eval_render_at_full_size(gpu):
    """BASELINE configs[2], planner query path (i): eval-mode render_rays of 8192 rays x (32 + 11) samples with the uncertainty head on,
    one launch (naruto_render_fwd), against the CPU oracle on the same jitter draw -- every map the reference's dict carries."""
    cfg = H.office_cfg(16, perturb=1.0)
    ora = H.make_oracle(cfg, 0.2, 17).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    N, S_tot = 8192, 43
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=17, zero_depth_frac=0.05)
    ro, rd, td = (torch.from_numpy(rays[k]) for k in ("rays_o", "rays_d", "target_d"))
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        got = m.forward(ro.to(gpu), rd.to(gpu), torch.from_numpy(rays["target_rgb"]).to(gpu), td.to(gpu), rand=rand.to(gpu))     # eval mode: the render dict
        want = ora.render_rays(ro, rd, target_d=td, rand=rand)
    assert {'rgb', 'depth', 'disp_map', 'acc_map', 'depth_var', 'z_vals', 'raw', 'uncert_map'} <= set(got)            # scene_rep.py:216-225
    H.assert_close(got["z_vals"], want["z_vals"], 2e-6, "configs2.z_vals")
    for k in ("raw", "rgb", "depth", "acc_map", "depth_var", "uncert_map"):
        H.assert_close(got[k], want[k], TOL_OUT, f"configs2.{k}")
    H.assert_close(got["disp_map"], want["disp_map"], TOL_OUT, "configs2.disp_map", rel=1e-4)
    assert float(got["uncert_map"].min()) > 0


def test_x3_chain_against_the_fp32_chain(gpu):
    """What the bench line's dtype "f32 (... exact bf16x3 splits on the bf16 MFMA ...)" claims, at full size: the exact mode's
    matrix phase as six bf16 products of exactly split fp32 operands (fwd_mlp_tile_x3, round 5) is fp32-grade arithmetic -- compared here
    against the fp32 matrix-instruction chain (fwd_mlp_tile) on the SAME 8192 x 43 = 352 256 samples: the eval render of all 8192 rays in one
    call runs the eight-wave kernel (x3 chain), the same rays in calls of 2048 the four-wave kernel (fp32 MFMA chain; naruto_render_fwd picks by
    ray count).  far = 3 m keeps every sample inside OneBlob's closed-form range, so both take the same OneBlob form and what is left IS the two
    chains' distance: each rounds a handful of times per output, in different places."""
    cfg = H.office_cfg(16, perturb=1.0)
    cfg["cam"]["far"] = 3.0
    ora = H.make_oracle(cfg, 0.2, 29).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    N, S_tot = 8192, 43
    rays = syn.random_rays(N, cfg["mapping"]["bound"], seed=29, zero_depth_frac=0.05)
    ro, rd, td = (torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_d"))
    rand = torch.rand(N, S_tot, generator=torch.Generator().manual_seed(7)).to(gpu)
    with torch.no_grad():
        whole = m.render_rays(ro, rd, target_d=td, rand=rand)["raw"]
        parts = torch.cat([m.render_rays(ro[i:i + 2048], rd[i:i + 2048], target_d=td[i:i + 2048], rand=rand[i:i + 2048])["raw"] for i in range(0, N, 2048)], 0)
        want = ora.render_rays(ro.cpu(), rd.cpu(), target_d=td.cpu(), rand=rand.cpu())["raw"]
    assert whole.shape == parts.shape == (N, S_tot, 5)
    assert torch.isfinite(whole).all() and torch.isfinite(parts).all()
    for c, name in enumerate(("r", "g", "b", "sdf")):
        a, b = whole[..., c].double(), parts[..., c].double()
        scale = float(b.abs().max())
        d = float((a - b).abs().max())
        # measured (tools/x3_chain_stats.py, MI355X): max 6.0e-8 absolute = 2.9e-7 ... 4.3e-7 of the channel's largest magnitude (0.12 ... 0.20), mean
        # 6e-9; both chains 4.2e-7 ... 1.7e-6 from the CPU oracle, within 2 % of each other
        assert d <= 5e-7 * scale, f"raw[...,{name}]: x3 chain vs fp32 chain {d:.3e} (scale {scale:.3e})"
        # ... and both sit equally close to the fp64-free CPU oracle (its own fp32 rounding is of the same size)
        da, db = float((a - want[..., c].double().to(gpu)).abs().max()), float((b - want[..., c].double().to(gpu)).abs().max())
        assert da <= TOL_OUT and db <= TOL_OUT and da <= 2.0 * db + 1e-7 * scale, (name, da, db)
    assert bool((whole[..., :4] != parts[..., :4]).any()), "the two calls were meant to run DIFFERENT matrix chains"
    assert torch.equal(whole[..., 4], parts[..., 4])        # the uncertainty channel never sees the MLP
    # non-finite operands: the exact split of +-inf is (inf, NaN, NaN) -- the x3 chain answers NaN where the fp32 chain answers +-inf (or NaN, for
    # inf * 0).  Pinned here for an infinite weight of the sdf net's OUTPUT layer: the sdf is non-finite at every sample in both chains (and the
    # colour, which does not see row 0, stays finite in both).  Behind a hidden layer BOTH chains can lose a non-finite value: their ReLU is
    # fmaxf(a, 0), which answers 0 for NaN where torch.relu answers NaN -- a diverged network is caught by the losses' own
    # non-finiteness and the deferred `uncert_map.min() > 0` check, not by this path.
    with torch.no_grad():
        m.decoder.sdf_net.model[2].weight[0, 3] = float("inf")
        bad_whole = m.render_rays(ro, rd, target_d=td, rand=rand)["raw"]
        bad_parts = torch.cat([m.render_rays(ro[i:i + 2048], rd[i:i + 2048], target_d=td[i:i + 2048], rand=rand[i:i + 2048])["raw"] for i in range(0, N, 2048)], 0)
    assert torch.equal(torch.isfinite(bad_whole), torch.isfinite(bad_parts))
    assert not torch.isfinite(bad_whole[..., 3]).any() and torch.isfinite(bad_whole[..., :3]).all() and torch.isfinite(bad_whole[..., 4]).all()


def test_configs2_map_volumes_on_the_full_lattice(gpu):
    """BASELINE configs[2], planner query path (ii): get_map_volumes (coslam_utils.py:58-97) on the FULL [49,56,35] lattice of office_0
    at 0.1 m -- 96 040 points through query_sdf(return_uncert=True) + the post-processing kernel -- against the oracle's restatement
    driven by the oracle's query_sdf; plus query_sdf itself with every flag the reference's callers use."""
    from naruto_amd.field import get_map_volumes
    cfg = H.office_cfg(16)
    ora = H.make_oracle(cfg, 0.2, 23).eval()
    m = H.make_hip_from_oracle(cfg, ora, gpu).eval()
    um, sv = get_map_volumes(m.query_sdf, m.bounding_box, 0.1)
    with torch.no_grad():
        oum, osv = S.get_map_volumes(ora.query_sdf, ora.bounding_box, 0.1)
    assert um.shape == (49, 56, 35) and sv.shape == (49, 56, 35)
    H.assert_close(sv, osv, TOL_OUT, "configs2.sdf volume")
    # the uncertainty volume is masked by 0 <= sdf < 0.5: a voxel whose sdf sits within rounding of a mask edge may flip
    flip = (np.abs(np.asarray(osv)) < 1e-5) | (np.abs(np.asarray(osv) - 0.5) < 1e-5)
    H.assert_close(np.where(flip, 0.0, um), np.where(flip, 0.0, np.asarray(oum)), TOL_OUT, "configs2.uncertainty volume")
    assert flip.mean() < 1e-3 and (np.asarray(oum) > 0).mean() > 0.05
    q = torch.rand(5000, 3, generator=torch.Generator().manual_seed(2)) * 1.2 - 0.1          # some points outside the unit cube
    with torch.no_grad():
        a, ga = m.query_sdf(q.to(gpu), return_geo=True, return_uncert=True)
        b, gb = ora.query_sdf(q, return_geo=True, return_uncert=True)
        H.assert_close(a, b, TOL_OUT, "configs2.query_sdf(sdf, uncert)")
        H.assert_close(ga, gb, TOL_OUT, "configs2.query_sdf geo")
        H.assert_close(m.query_sdf(q.to(gpu), embed=True), ora.query_sdf(q, embed=True), 2e-6, "configs2.query_sdf embed")


# --------------------------------------------------------------------------------------------- the driver's multi-GPU launch line
def test_bench_launch_line_at_two_ranks(gpu):
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py --gpus 2 ...` --
    the command the driver runs for the scaling curve -- end to end on whatever this box has: RCCL when two GPUs are visible, otherwise
    a gloo REHEARSAL with both ranks on the one GPU (NARUTO_DIST_BACKEND=gloo).  Exactly one JSON line from rank 0, the contract's
    keys, n_gpus = 2, weak scaling = the workload's ray count per rank."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if torch.cuda.device_count() < 2:
        env["NARUTO_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--no-kernels", "--no-cpu-baseline", "--workload", "office0_2048x43"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out, k
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["scaling"] == "weak" and out["unit"] == "rays/s"
    assert out["config"]["rays_per_gpu"] == 2048 and out["config"]["rays_per_step"] == 4096
    assert abs(out["value"] - 4096 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    assert ("rehearsal" in out["config"]) == (torch.cuda.device_count() < 2)


def test_bench_self_launches_without_a_launcher(gpu):
    """`python bench.py --gpus 2 ...` with NO WORLD_SIZE in the environment (how the driver issues its 1-GPU command): bench.py must turn
    itself into the torch.distributed.run launch line instead of failing on the world-size check, and still print exactly one JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    if torch.cuda.device_count() < 2:
        env["NARUTO_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--no-kernels", "--no-cpu-baseline", "--workload", "office0_2048x43"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["rays_per_step"] == 4096 and "multi_gpu_note" in out


def test_bench_plain_run_dumps_the_same_outputs_twice(gpu, tmp_path):
    """A plain `bench.py --steps K --warmup W` times K steps and measures nothing of --full's; with --dump-outputs two runs write the
    same last-step outputs, although their time-based pre-warm runs a different number of untimed steps."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "13", "--warmup", "3", "--workload", "office0_2048x43",
               "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 13 and abs(out["value"] - 2048 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
        for k in ("kernels", "roofline", "dropin", "mapping_iter", "cpu_baseline", "torch_gpu_baseline"):
            assert k not in out, k
        assert out["ms_per_step_median_of_5_chunks"] is None
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = outs
    assert sorted(a) == sorted(b) and {"rgb.npy", "depth.npy", "losses.npy", "loss.npy", "table.npy", "sdf_w0.npy"} <= set(a)
    assert a["rgb.npy"].shape == (2048, 3) and a["rgb.npy"].dtype == np.float32
    for f in a:
        assert np.all(np.isfinite(a[f])), f
        np.testing.assert_allclose(a[f], b[f], rtol=1e-5, atol=1e-7, err_msg=f)


def test_fused_adam_is_a_torch_optimizer(gpu):
    """FusedAdam behind the torch.optim.Optimizer surface the reference's driver and checkpointing use: param groups edited in place
    (a scheduler's lr change), a parameter without gradient skipped, add_param_group, state_dict -> load_state_dict into a fresh
    optimiser continuing bit for bit, closure, zero_grad(set_to_none)."""
    from naruto_amd.trainer import FusedAdam
    torch.manual_seed(9)
    mk = lambda: [torch.nn.Parameter(torch.randn(513, device=gpu)), torch.nn.Parameter(torch.randn(7, 33, device=gpu)), torch.nn.Parameter(torch.randn(64, device=gpu))]
    pa = mk()
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    groups = lambda ps: [{'params': ps[:1], 'weight_decay': 1e-6, 'lr': 0.01}, {'params': ps[1:2], 'eps': 1e-15, 'lr': 0.02}]
    oa, ob = FusedAdam(groups(pa), betas=(0.9, 0.99)), torch.optim.Adam(groups(pb), betas=(0.9, 0.99))
    assert isinstance(oa, torch.optim.Optimizer)
    sched = torch.optim.lr_scheduler.StepLR(oa, step_size=2, gamma=0.5), torch.optim.lr_scheduler.StepLR(ob, step_size=2, gamma=0.5)
    gen = torch.Generator(gpu).manual_seed(1)

    def feed(ps_a, ps_b, skip=None):
        for k, (p, q) in enumerate(zip(ps_a, ps_b)):
            if k == skip:
                p.grad = q.grad = None
                continue
            g = torch.randn(p.shape, device=gpu, generator=gen)
            p.grad, q.grad = g.clone(), g.clone()
    for it in range(5):
        if it == 2:
            oa.add_param_group({'params': pa[2:], 'lr': 0.005})
            ob.add_param_group({'params': pb[2:], 'lr': 0.005})
        feed(pa[:len(oa.state)], pb[:len(oa.state)], skip=1 if it == 3 else None)
        oa.step()
        ob.step()
        for s_ in sched:
            s_.step()
    for p, q in zip(pa, pb):
        H.assert_close(p, q, 2e-6, "FusedAdam vs torch.optim.Adam", rel=1e-5)
    # checkpoint round trip: a fresh optimiser restored from the state_dict continues exactly like the original
    import copy
    sd = copy.deepcopy(oa.state_dict())            # what torch.save / torch.load hands back: load_state_dict itself does not copy tensors
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oc = FusedAdam(groups(pc), betas=(0.9, 0.99))
    oc.add_param_group({'params': pc[2:], 'lr': 0.005})
    oc.load_state_dict(sd)
    assert oc.param_groups[0]['lr'] == oa.param_groups[0]['lr']
    feed(pa, pc)
    assert oa.step(closure=lambda: torch.tensor(3.0)) == 3.0
    oc.step()
    for p, q in zip(pa, pc):
        assert torch.equal(p, q), "restored optimiser diverges from the original"
    oa.zero_grad()
    assert all(p.grad is None for p in pa)
    # interchange with torch.optim.Adam in BOTH directions (advisor, round 3): a torch checkpoint loads into FusedAdam (no 'lag' / 'naruto_step'
    # in it: the count comes from the per-parameter 'step', a late-added or skipped parameter's lag from the difference) and FusedAdam's loads
    # into torch (every state carries 'step'); all three then take the same further step
    sd_t = copy.deepcopy(ob.state_dict())
    pd = [torch.nn.Parameter(q.detach().clone()) for q in pb]
    od = FusedAdam(groups(pd), betas=(0.9, 0.99))
    od.add_param_group({'params': pd[2:], 'lr': 0.005})
    od.load_state_dict(sd_t)
    sd_f = copy.deepcopy(od.state_dict())
    assert all('step' in st for st in sd_f['state'].values())
    pe = [torch.nn.Parameter(q.detach().clone()) for q in pb]
    oe = torch.optim.Adam(groups(pe), betas=(0.9, 0.99))
    oe.add_param_group({'params': pe[2:], 'lr': 0.005})
    oe.load_state_dict(sd_f)
    for k in range(3):
        g = [torch.randn(q.shape, device=gpu, generator=gen) for q in pb]
        for ps in (pb, pd, pe):
            for q, gg in zip(ps, g):
                q.grad = gg.clone()
        ob.step(); od.step(); oe.step()
    for q, r, t in zip(pb, pd, pe):
        assert torch.equal(q, t), "torch.optim.Adam restored from FusedAdam's state_dict diverges from the original torch optimiser"
        H.assert_close(r, q, 2e-6, "FusedAdam restored from a torch.optim.Adam state_dict", rel=1e-5)
    # a parameter WITHOUT state in a torch checkpoint (it never received a gradient there) has taken 0 steps, whatever count the loading
    # optimiser held before (advisor, round 4): its lag is the loaded global count and its first real steps match torch's
    pf = [torch.nn.Parameter(torch.randn(40, device=gpu, generator=gen)), torch.nn.Parameter(torch.randn(24, device=gpu, generator=gen))]
    pg = [torch.nn.Parameter(q.detach().clone()) for q in pf]
    of_t = torch.optim.Adam([{'params': pf}], lr=0.01)
    for k in range(3):
        pf[0].grad = torch.randn(40, device=gpu, generator=gen)
        of_t.step()
    sd_p = copy.deepcopy(of_t.state_dict())
    assert len(sd_p['state']) == 1
    og = FusedAdam([{'params': pg}], lr=0.01)
    for k in range(2):                               # the loading optimiser has a history of its own (a stale step count)
        for q in pg:
            q.grad = torch.randn(q.shape, device=gpu, generator=gen)
        og.step()
    with torch.no_grad():
        for q, r in zip(pg, pf):
            q.copy_(r)
    og.load_state_dict(sd_p)
    st_g = og.state_dict()['state']
    assert float(st_g[0]['step']) == 3.0 and float(st_g[1]['step']) == 0.0, (st_g[0]['step'], st_g[1]['step'])
    for k in range(2):
        g = [torch.randn(q.shape, device=gpu, generator=gen) for q in pf]
        for ps in (pf, pg):
            for q, gg in zip(ps, g):
                q.grad = gg.clone()
        of_t.step(); og.step()
    for q, r in zip(pf, pg):
        H.assert_close(r, q, 2e-6, "FusedAdam: parameter without state in a torch checkpoint", rel=1e-5)


def test_graphed_caller_iteration_equals_eager(gpu):
    """naruto_amd.graphed.GraphedIteration: the caller's own loop body (model.forward -> get_loss_from_ret incl. the fused smoothness ->
    loss.backward(retain_graph=True) -> FusedAdam steps, uncertainty grid every 5th) captured with torch's whole-iteration capture and
    replayed, against the same body launched eagerly: identical losses per iteration and bit-identical parameters after 12 iterations
    (two uncertainty-grid steps, its gradient accumulating over five replays in between).  The smoothness lattice is pinned to one
    placement on both sides (torch's device generator advances differently under replay)."""
    from naruto_amd import trainer
    from dropin_caller import DropInCaller
    from naruto_amd.graphed import GraphedIteration

    off, jit = torch.tensor([0.3, 0.6, 0.1], device=gpu), torch.tensor([0.2, 0.9, 0.5], device=gpu)

    class Caller(DropInCaller):
        def smoothness(self, sample_points=256, voxel_size=0.1, margin=0.05, color=False):
            return trainer.smoothness(self.model, self.config, sample_points, voxel_size, margin, offset_rand=off, jitter_rand=jit)
    cfg = H.office_cfg(12, perturb=1.0)
    ora = H.make_oracle(cfg, 0.1, 13)
    twins = []
    for _ in range(2):
        m = H.make_hip_from_oracle(cfg, ora, gpu).train()
        twins.append((m, Caller(m, cfg, 0.1, optimizer="fused", smoothness="fused")))
    (ma, ca), (mb, cb) = twins
    step = GraphedIteration(cb, 200)
    ma._node_state(200, False)                          # creates the eager side's {seed, counter}
    mb._rng_state.copy_(ma._rng_state)                  # same depth jitter on both sides
    losses = {"eager": [], "graph": []}
    keys = ("rgb_loss", "depth_loss", "sdf_loss", "fs_loss", "uncert_loss")
    for i in range(12):
        rays = syn.random_rays(200, cfg["mapping"]["bound"], seed=300 + i, zero_depth_frac=0.05)
        t = [torch.from_numpy(rays[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        ret, loss = ca.ba_iteration(i, *t)
        losses["eager"].append([float(ret[k].detach()) for k in keys] + [float(loss.detach())])
        ret, loss = step(i, *t)
        losses["graph"].append([float(ret[k].detach()) for k in keys] + [float(loss.detach())])
    assert losses["eager"] == losses["graph"], (losses["eager"][-1], losses["graph"][-1])
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: graph replay != eager launches"
    ma.check_asserts(block=True)
    mb.check_asserts(block=True)


# --------------------------------------------------------------------------------------------- sharded table optimiser (large-table data parallelism)
def _dp_shard_worker(rank, world, port, backend, n_rays, steps, out, shard, graph):
    import torch.distributed as dist
    from naruto_amd import trainer, parallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    cfg = H.office_cfg(12, perturb=0.0)
    torch.manual_seed(5)
    tr = trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), dev, fused_adam=True, group=dist.group.WORLD, shard_table_optimizer=shard)
    assert (tr.table_shard is not None) == shard
    lo, hi = parallel.shard_bounds(n_rays, rank, world)
    if graph:
        tr.capture(hi - lo, smooth=True, n_rays_total=n_rays)
    losses = []
    for it in range(steps):
        rays = syn.random_rays(n_rays, cfg["mapping"]["bound"], seed=400 + it, zero_depth_frac=0.1)
        t = [torch.from_numpy(rays[k]) for k in ("rays_o", "rays_d", "target_rgb", "target_d")]
        shard_rays = [a.to(dev) for a in parallel.shard_rays(t, rank, world)]
        ret, loss = tr.step(*shard_rays, smooth=True, n_rays_total=n_rays)
        losses.append(float(loss))
    torch.cuda.synchronize()
    # every rank must hold the same table after the all-gather
    tab = tr.model.embed_fn.params.detach().cpu()
    gathered = [torch.empty_like(tab) for _ in range(world)]
    dist.all_gather(gathered, tab)
    same = all(torch.equal(gathered[0], g) for g in gathered)
    moments = sum(s_["exp_avg"].numel() for o in ((tr.map_optimizer, tr.table_optimizer) if shard else (tr.map_optimizer,)) for s_ in o.state.values())
    if rank == 0:
        torch.save({"params": {n: p.detach().cpu() for n, p in tr.model.named_parameters()}, "losses": losses, "replicas_equal": same, "moments": moments}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("graph", [False, True])
def test_sharded_table_optimizer_equals_replicated(gpu, tmp_path, graph):
    """MappingTrainer(shard_table_optimizer=True) -- reduce-scatter of the table gradient, Adam on each rank's 1/world slice (moments for
    that slice only), all-gather of the updated table: the form for tables beyond 2^22 parameters -- against the replicated optimiser
    (all-reduce + the identical full Adam on every rank) over two ranks: bit-identical parameters and losses after six iterations,
    eager launches and the three-segment hipGraph form; half the optimiser state per rank."""
    import socket
    import torch.multiprocessing as mp
    n_rays, steps = 160, 6
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    res = {}
    for shard in (False, True):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        out = str(tmp_path / f"dp_shard{int(shard)}.pt")
        mp.spawn(_dp_shard_worker, args=(2, port, backend, n_rays, steps, out, shard, graph), nprocs=2, join=True)
        res[shard] = torch.load(out)
    a, b = res[False], res[True]
    assert a["replicas_equal"] and b["replicas_equal"]
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    for n in a["params"]:
        assert torch.equal(a["params"][n], b["params"][n]), f"{n}: sharded optimiser != replicated ({backend}, graph={graph})"
    n_table = a["params"]["embed_fn.params"].numel()
    assert b["moments"] <= a["moments"] - n_table // 2 + 8, (a["moments"], b["moments"])


def test_fused_ba_recaptures_when_the_ray_count_changes(gpu):
    """FusedBA across keyframes while n_cur = max(sample // n_kf, min_pixels_cur) still moves (the first ~20 keyframes of a run): a
    new ray count means new static buffers and a new capture; the trajectory stays the eager one, bit for bit."""
    from naruto_amd import trainer
    from naruto_amd.ba_loop import FusedBA
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["mapping"].update(sample=256, min_pixels_cur=10, filter_depth=True, keyframe_every=5)
    bound = torch.tensor(cfg["mapping"]["bound"])
    twins = []
    for use_graph in (True, False):
        torch.manual_seed(44)
        tr = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
        store, current, poses, _ = _ba_scene(cfg, gpu, n_kf=8)
        twins.append((FusedBA(tr, store, None, max_poses=64, use_graph=use_graph), current, poses))
    (a, cur, poses), (b, _, _) = twins
    b.trainer.model.load_state_dict(a.trainer.model.state_dict())
    b.trainer.iter_state.copy_(a.trainer.iter_state)
    counts = []
    for call in range(2):
        for ba in (a, b):
            if call == 1:
                rs = np.random.RandomState(9)
                ba.store.add_keyframe({"direction": torch.from_numpy(rs.normal(size=(1, 48, 64, 3)).astype(np.float32)),
                                       "rgb": torch.from_numpy(rs.uniform(size=(1, 48, 64, 3)).astype(np.float32)),
                                       "depth": torch.from_numpy(rs.uniform(0.5, 2.0, (1, 48, 64)).astype(np.float32)), "frame_id": torch.tensor([40])}, filter_depth=True)
            p_all = poses if call == 0 else torch.cat([poses, poses[-1:]], 0)
            n_cur, n_train = ba.prepare(cur, p_all)
            for i in range(6):
                ba.iteration(i)
        counts.append(n_train)
    assert counts == [256 + 32, 256 + 28], counts                       # 256 // 8 and 256 // 9
    for (n, p), (_, q) in zip(a.trainer.model.named_parameters(), b.trainer.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}: graph replay (re-captured) != eager launches"

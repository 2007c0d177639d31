"""The fp32 MLP backward's tiles (k_query_bwd): its 16-wide dW tiles run on the 16x16x4 matrix instruction as 16x16 blocks, the others on the
32x32x2 form.  Against oracle autograd with the harness and the tolerance of test_query_backward_vs_oracle (H.office_cfg(12), grad_close:
1e-4 of the largest gradient magnitude of the tensor + 1e-3 relative), at the point counts where the tile loop and its cross-wave sum can go
wrong: a lone lane, a last tile one short / full / one over, an odd tile count, and a count that gives a wave three tiles."""
import numpy as np
import pytest
import torch

from naruto_amd import synthetic as syn
from oracle import spec_torch as S

import helpers as H

pytestmark = pytest.mark.gpu

grad_close = H.grad_close
WEIGHTS = ("sdf_w0", "sdf_w1", "col_w0", "col_w1")


def three_tile_count():
    """The launcher's grid rule (query_bwd_impl): 32 points per tile, four waves per workgroup, at most one workgroup per compute unit and at most
    512 workgroups; a wave runs the tiles wave, wave + 4 * workgroups, ...  So one tile more than two per wave gives a wave three tiles (the count
    ends in a partial tile on top)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = 4 * min(cus, 512)
    return 32 * 2 * waves + 33


def _nonzero_where_the_reference_is(gh, go, what):
    """_compare's rules without its tolerance (for a caller that brings a tolerance of its own): a gradient the reference does not have is absent
    or all zeros, every other one is non-zero somewhere the reference is -- the weight gradients in every 16 x 16 block."""
    for k in gh:
        if go[k] is None:
            assert gh[k] is None or float(gh[k].abs().max()) == 0.0, k
            continue
        nz = go[k].detach().cpu() != 0
        if bool(nz.any()):          # (a lone point outside the box leaves the uncertainty grid without a gradient; query_sdf has no colour output)
            assert gh[k] is not None and bool((gh[k].detach().cpu()[nz] != 0).any()), f"{what}: {k} is zero wherever the oracle's is not"
        if k in WEIGHTS:
            # block by block (16 x 16: the unit the kernel's tiles are written in -- a 32 x 32 register tile is four of them, a half-shape tile two):
            # a block left at zero must not hide behind the tensor's largest entry
            got = gh[k].detach().cpu()
            for r0 in range(0, got.shape[0], 16):
                for c0 in range(0, got.shape[1], 16):
                    bn = nz[r0:r0 + 16, c0:c0 + 16]
                    if bool(bn.any()):
                        assert bool((got[r0:r0 + 16, c0:c0 + 16][bn] != 0).any()), f"{what}: block ({r0}, {c0}) of {k} is zero where the oracle's is not"


def _compare(gh, go, what):
    _nonzero_where_the_reference_is(gh, go, what)
    for k in gh:
        if go[k] is not None:
            grad_close(gh[k], go[k], f"{what}.grad.{k}")


def _query_grads(gpu, n_pts, with_geo, seed=21):
    cfg = H.office_cfg(12)
    ora = H.make_oracle(cfg, 0.25, seed)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    rs = np.random.RandomState(2)
    x = rs.uniform(-0.2, 1.2, size=(n_pts, 3)).astype(np.float32)
    if with_geo:
        c_su = rs.normal(size=(n_pts, 2)).astype(np.float32)
        c_geo = rs.normal(size=(n_pts, 15)).astype(np.float32)
        su, geo = ora.query_sdf(torch.from_numpy(x), return_geo=True, return_uncert=True)
        ((su * torch.from_numpy(c_su)).sum() + (geo * torch.from_numpy(c_geo)).sum()).backward()
        su_g, geo_g = m.query_sdf(torch.from_numpy(x).to(gpu), return_geo=True, return_uncert=True)
        ((su_g * torch.from_numpy(c_su).to(gpu)).sum() + (geo_g * torch.from_numpy(c_geo).to(gpu)).sum()).backward()
    else:
        c_raw = rs.normal(size=(n_pts, 5)).astype(np.float32)
        raw = ora.query_color_sdf(torch.from_numpy(x))
        (raw * torch.from_numpy(c_raw)).sum().backward()
        raw_g = m.query_color_sdf(torch.from_numpy(x).to(gpu))
        (raw_g * torch.from_numpy(c_raw).to(gpu)).sum().backward()
    return H.hip_grads(m), H.ora_grads(ora), m


@pytest.mark.parametrize("with_geo", [False, True])
@pytest.mark.parametrize("n_pts", [1, 31, 32, 33, 65, "three_tiles"])
def test_query_backward_tiles_vs_oracle(gpu, n_pts, with_geo):
    n = three_tile_count() if n_pts == "three_tiles" else n_pts
    gh, go, _ = _query_grads(gpu, n, with_geo)
    _compare(gh, go, f"{n} points, d_geo {with_geo}")
    # the same call once more on the stamped build of the kernel, which counts the tiles each wave ran (slot 7 of a wave's row of 16): the count
    # above did give a wave three tiles (the gradients compared above are the product kernel's)
    from naruto_amd import _lib
    lib = _lib.load()
    rows = torch.zeros(16 * 4 * 512, dtype=torch.int64, device=gpu)
    lib.naruto_debug_bwd_timeline(rows.data_ptr())
    try:
        _query_grads(gpu, n, with_geo)
        torch.cuda.synchronize()
    finally:
        lib.naruto_debug_bwd_timeline(None)
    tiles = rows.reshape(-1, 16)[:, 7]
    assert int(tiles.sum()) == (n + 31) // 32, (int(tiles.sum()), n)
    assert int(tiles.max()) == (3 if n_pts == "three_tiles" else 1), int(tiles.max())


@pytest.mark.parametrize("n_samples_d", [32, 117])          # 33 rays x 43 and 33 x 128 samples
def test_training_backward_active_list_vs_oracle(gpu, n_samples_d):
    """Through the training path: a tenth of the rays has no depth, the truncation band leaves most samples without a cotangent, and the backward
    works on the compacted list of the others."""
    cfg = H.office_cfg(12, n_samples_d=n_samples_d)
    ora = H.make_oracle(cfg, 0.25, 23).train()
    m = H.make_hip_from_oracle(cfg, ora, gpu).train()
    rays = syn.random_rays(33, cfg["mapping"]["bound"], seed=23, zero_depth_frac=0.1)
    t = {k: torch.from_numpy(v) for k, v in rays.items()}
    names = ("rays_o", "rays_d", "target_rgb", "target_d")
    S.total_loss(ora.forward(*(t[k] for k in names)), cfg["training"]).backward()
    S.total_loss(m.forward(*(t[k].to(gpu) for k in names)), cfg["training"]).backward()
    _compare(H.hip_grads(m), H.ora_grads(ora), f"33 rays x {n_samples_d + 11}")


def test_weight_gradients_repeat_bitwise(gpu):
    """The order in which tiles, waves and workgroups are summed is fixed: two identical runs, same bits (65 points: three tiles on three waves)."""
    a, _, _ = _query_grads(gpu, 65, False)
    b, _, _ = _query_grads(gpu, 65, False)
    for k in WEIGHTS:
        assert float(a[k].abs().max()) > 0.0, k
        assert torch.equal(a[k], b[k]), f"gradient {k} differs between identical runs"

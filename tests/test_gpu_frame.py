"""A mapped frame on the device: naruto_frame_ingest / naruto_keyframe_row against the torch expressions they replace
(``torch.cat`` + the valid-depth count; ``KeyFrameStoreHIP.add_keyframe``), ``FusedBA.first_frame_mapping`` against the eager twin,
``get_map_volumes(to_host=False)`` against the host form.  Everything is compared bit for bit.

Run: timeout -k 10 300 python -m pytest tests/test_gpu_frame.py -m gpu -q
"""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

TRUNC = 2.5


def _cfg(**mapping):
    c = H.office_cfg(12, perturb=1.0)
    c["cam"]["depth_trunc"] = TRUNC
    c["mapping"].update(sample=192, min_pixels_cur=16, keyframe_every=5, filter_depth=True)
    c["mapping"].update(mapping)
    return c


def _frame(Hh, Ww, seed, n_valid=None):
    """direction / rgb / depth of one frame on the host.  ``n_valid``: exactly that many valid depths, scattered; default: about 85 %
    valid, with every edge value the mask has -- 0, a negative depth, exactly depth_trunc (valid), the next float above (invalid),
    inf and NaN -- as far as the frame has room for them."""
    rs = np.random.RandomState(seed)
    n = Hh * Ww
    d = rs.normal(size=(Hh, Ww, 3)).astype(np.float32)
    rgb = rs.uniform(size=(Hh, Ww, 3)).astype(np.float32)
    depth = rs.uniform(0.3, TRUNC - 0.1, n).astype(np.float32)
    if n_valid is not None:
        depth[rs.permutation(n)[:n - n_valid]] = 0.0
    else:
        depth[rs.uniform(size=n) < 0.15] = 0.0
        edge = np.array([0.0, -1.0, TRUNC, np.nextafter(np.float32(TRUNC), np.float32(np.inf)), np.inf, np.nan, -0.0], np.float32)
        k = min(n, edge.size)
        depth[rs.permutation(n)[:k]] = edge[:k]
        d.reshape(-1)[0] = -0.0                       # a bit pattern a float comparison would not tell from +0
    return torch.from_numpy(d), torch.from_numpy(rgb), torch.from_numpy(depth.reshape(Hh, Ww))


def _torch_rays(d, rgb, depth):
    return torch.cat([d, rgb, depth[..., None]], -1).reshape(-1, 7)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ingest(gpu, d, rgb, depth, out=None):
    from naruto_amd.keyframe_store import frame_ingest
    n = depth.numel()
    out = torch.full((n, 7), -7.0, device=gpu) if out is None else out
    word = torch.full((1,), 12345, dtype=torch.int64, device=gpu)          # the launch zeroes it itself
    frame_ingest(d.to(gpu), rgb.to(gpu), depth.to(gpu), TRUNC, out, word)
    return out, word


@pytest.mark.parametrize("Hh,Ww", [(30, 40), (7, 9), (1, 1)])
def test_ingest_equals_the_torch_expression(gpu, Hh, Ww):
    """30 x 40: 8 400 words, the last workgroup is partial; 7 x 9: less than one wave of depth words; 1 x 1."""
    for seed in range(3):
        d, rgb, depth = _frame(Hh, Ww, seed)
        if Hh * Ww == 1:
            depth[0, 0] = [1.0, float("nan"), TRUNC][seed]
        want = _torch_rays(d, rgb, depth)
        count = int(((depth > 0.0) & (depth <= TRUNC)).sum())
        out, word = _ingest(gpu, d, rgb, depth)
        assert torch.equal(_bits(out).cpu(), _bits(want)), (Hh, Ww, seed)
        assert int(word.item()) == count, (Hh, Ww, seed, int(word.item()), count)
    if Hh * Ww > 1:
        assert count not in (0, Hh * Ww)


def _twin_stores(gpu, cfg, Hh, Ww, R, mode="reference"):
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    return [KeyFrameStoreHIP(cfg, Hh, Ww, num_kf=5, num_rays_to_save=R, device=gpu, seed=17, filter_depth_mode=mode) for _ in range(2)]


@pytest.mark.parametrize("case", ["unfiltered", "filtered", "tiled5", "tiled1"])
def test_keyframe_row_equals_add_keyframe(gpu, case):
    """Four keyframes through ``add_keyframe_device`` and through ``add_keyframe`` on a twin store with the same seed: rows, ids and the
    draw counter.  unfiltered: all 1 200 pixels are the population; filtered: n_valid > rays_per_kf; tiled5 / tiled1: n_valid = 5 / 1
    against rays_per_kf = 12, the periodic tiling."""
    Hh, Ww = 30, 40
    filt = case != "unfiltered"
    R = 12 if case.startswith("tiled") else 100
    n_valid = {"tiled5": 5, "tiled1": 1}.get(case)
    cfg = _cfg()
    dev_store, ref_store = _twin_stores(gpu, cfg, Hh, Ww, R)
    buf = torch.zeros(Hh * Ww, 7, device=gpu)
    for k in range(4):
        d, rgb, depth = _frame(Hh, Ww, 10 + k, n_valid=n_valid)
        _, word = _ingest(gpu, d, rgb, depth, out=buf)
        if n_valid is not None:
            assert int(word.item()) == n_valid
        elif filt:
            assert int(word.item()) > R
        dev_store.add_keyframe_device(buf, 5 * k, filter_depth=filt, n_valid=word)
        ref_store.add_keyframe({"direction": d[None], "rgb": rgb[None], "depth": depth[None], "frame_id": torch.tensor([5 * k])}, filter_depth=filt)
        assert dev_store.counter == ref_store.counter
    assert torch.equal(dev_store.frame_ids, ref_store.frame_ids) and dev_store.frame_ids.tolist() == [0, 5, 10, 15]
    assert torch.equal(_bits(dev_store.rays), _bits(ref_store.rays)), case
    assert len({tuple(r) for r in _bits(dev_store.rays[3]).tolist()}) == (n_valid or R), "distinct pixels, tiled periodically"


def test_keyframe_without_a_valid_pixel_and_valid_only(gpu):
    """n_valid = 0: the id is attached and the row stays as it was (keyframe.py:56-57); told the count, the draw counter rests as
    add_keyframe's does.  The 'valid_only' mode needs add_keyframe's compacted list: refused."""
    Hh, Ww, R = 7, 9, 12
    cfg = _cfg()
    dev_store, ref_store = _twin_stores(gpu, cfg, Hh, Ww, R)
    d, rgb, depth = _frame(Hh, Ww, 3, n_valid=0)
    buf, word = _ingest(gpu, d, rgb, depth)
    assert int(word.item()) == 0
    for st in (dev_store, ref_store):
        st.rays.fill_(3.25)
    dev_store.add_keyframe_device(buf, 0, filter_depth=True, n_valid=word)                      # the kernel reads 0 and writes nothing
    assert dev_store.frame_ids.tolist() == [0] and bool((dev_store.rays == 3.25).all())
    dev_store.add_keyframe_device(buf, 5, filter_depth=True, n_valid=word, n_valid_host=0)
    assert dev_store.frame_ids.tolist() == [0, 5] and bool((dev_store.rays == 3.25).all()) and dev_store.counter == 1
    ref_store.add_keyframe({"direction": d[None], "rgb": rgb[None], "depth": depth[None], "frame_id": 0}, filter_depth=True)
    assert ref_store.frame_ids.tolist() == [0] and bool((ref_store.rays == 3.25).all()) and ref_store.counter == 0
    only = _twin_stores(gpu, cfg, Hh, Ww, R, mode="valid_only")[0]
    with pytest.raises(NotImplementedError):
        only.add_keyframe_device(buf, 0, filter_depth=True, n_valid=word)
    assert len(only) == 0


def test_first_frame_mapping_equals_the_eager_twin(gpu):
    """``FusedBA.first_frame_mapping`` (graphs, prefetched draws) against ``MappingTrainer.first_frame_mapping`` over batches the twin
    draws with ``assemble_batch`` and the same keys: 7 iterations (not a multiple of 5: no grid step may slip in), 192 rays out of the
    1 200 pixels of a 30 x 40 frame.  Every parameter, the uncertainty grid and its kept gradient, bit for bit."""
    from naruto_amd import trainer
    from naruto_amd.ba_loop import FusedBA
    from naruto_amd.keyframe_store import KeyFrameStoreHIP
    Hh, Ww, N = 30, 40, 192
    cfg = _cfg(first_iters=7)
    bound = torch.tensor(cfg["mapping"]["bound"])
    d, rgb, depth = _frame(Hh, Ww, 21)
    depth = torch.nan_to_num(depth, nan=0.0, posinf=0.0).clamp_min(0.0)          # a frame a sensor could deliver
    d = d / d.norm(dim=-1, keepdim=True)
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([float(b[0] + 0.5 * (b[1] - b[0])) for b in cfg["mapping"]["bound"]])
    twins = []
    for _ in range(2):
        torch.manual_seed(5)
        tr = trainer.MappingTrainer(cfg, bound, gpu, fused_adam=True)
        store = KeyFrameStoreHIP(cfg, Hh, Ww, num_kf=3, num_rays_to_save=50, device=gpu, seed=2)
        twins.append((tr, store))
    (tr_a, store_a), (tr_b, store_b) = twins
    tr_b.model.load_state_dict(tr_a.model.state_dict())
    tr_b.iter_state.copy_(tr_a.iter_state)
    for tr in (tr_a, tr_b):
        tr.model.uncert_grid.grad.fill_(0.5)                                     # zeroed once at the start, by both
    ba = FusedBA(tr_a, store_a, None, max_poses=8, use_graph=True)
    _ingest(gpu, d, rgb, depth, out=ba.current)
    ret_a, loss_a = ba.first_frame_mapping(pose)
    assert len(store_a) == 0 and tr_a.iter == 7
    current = _torch_rays(d, rgb, depth).to(gpu)

    def batches():
        for _ in range(7):
            yield store_b.assemble_batch(0, current, pose[None].to(gpu), 0, rng=tr_b.iter_state, n_cur=N, n_cur_pop=Hh * Ww)[:4]
    ret_b, loss_b = tr_b.first_frame_mapping(batches())
    assert float(loss_a) == float(loss_b)
    assert torch.equal(tr_a.iter_state, tr_b.iter_state)
    for (n, p), (_, q) in zip(tr_a.model.named_parameters(), tr_b.model.named_parameters()):
        assert torch.equal(p, q), f"parameter {n}"
    assert torch.equal(tr_a.model.uncert_grid, tr_b.model.uncert_grid)
    g_a, g_b = tr_a.model.uncert_grid.grad, tr_b.model.uncert_grid.grad
    assert torch.equal(g_a, g_b) and bool((g_a != 0).any()), "the grid's gradient is kept, not zeroed, after its one step"


def test_map_volumes_stay_on_the_device(gpu):
    from naruto_amd.field import get_map_volumes
    cfg = _cfg()
    ora = H.make_oracle(cfg, 0.2, 1)
    m = H.make_hip_from_oracle(cfg, ora, gpu)
    host = get_map_volumes(m.query_sdf, m.bounding_box, 0.4)
    dev = get_map_volumes(m.query_sdf, m.bounding_box, 0.4, to_host=False)
    assert all(v.is_cuda and v.dtype == torch.float32 for v in dev)
    for h, v in zip(host, dev):
        assert tuple(v.shape) == h.shape and np.array_equal(v.cpu().numpy().view(np.int32), h.view(np.int32))
    buf = torch.full((2 * host[0].size,), -1.0, device=gpu)
    ptrs = None
    for _ in range(2):
        own = get_map_volumes(m.query_sdf, m.bounding_box, 0.4, to_host=False, out=buf)
        now = (own[0].data_ptr(), own[1].data_ptr())
        assert ptrs is None or now == ptrs
        ptrs = now
        assert now[0] == buf.data_ptr() and now[1] == buf.data_ptr() + 4 * host[0].size
        for h, v in zip(host, own):
            assert np.array_equal(v.cpu().numpy().view(np.int32), h.view(np.int32))
    with pytest.raises(ValueError):
        get_map_volumes(m.query_sdf, m.bounding_box, 0.4, out=buf)

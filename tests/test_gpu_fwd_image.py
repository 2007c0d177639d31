"""The training forward's weight image (NarutoTrainStep.fwd_image): kept in step with the MLP weights by the fused-Adam finishing launch and
read by the chained iterations' forwards (k_query_fwd_loss_img, k_query_fwd_loss_short_img) instead of staging the weights in every workgroup.

(a) the maintained buffer equals what a forward workgroup stages from the weights, as raw bytes, zero padding included;
(b) a chain captured with the image gives the same bits as one captured without, MappingTrainer.capture(chain=...) and FusedBA.call_iterations();
(c) weights changed from outside between replays: iteration 0 of a chain never trusts the buffer.

Smallest shapes that take every path: 6 rays x 128 samples (the walk: one full workgroup of four rays and one with two, the other two waves on
loss_stage_no_ray), 7 rays x 43 samples (the short kernel: five rays per workgroup, the second one partly filled)."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
from naruto_amd import _lib, synthetic as syn, trainer

pytestmark = pytest.mark.gpu

CHAIN = [False, False, False, False, True, False]           # the uncertainty-grid step on the 5th iteration
SHAPES = [(6, 117, 1), (7, 32, 3)]                          # rays, n_samples_d (+ 11 range samples), the launch form: 1 walk, 3 short


def _cfg(n_samples_d):
    return H.office_cfg(12, perturb=1.0, n_samples_d=n_samples_d)


def _trainer(cfg, gpu, seed=7):
    torch.manual_seed(seed)
    return trainer.MappingTrainer(cfg, torch.tensor(cfg["mapping"]["bound"]), gpu, fused_adam=True)


def _rays(cfg, n, gpu, seed=3):
    r = syn.random_rays(n, cfg["mapping"]["bound"], seed=seed)
    return tuple(torch.from_numpy(r[k]).to(gpu) for k in ("rays_o", "rays_d", "target_rgb", "target_d"))


def _same_state(dst, src):
    dst.model.load_state_dict(src.model.state_dict())
    dst.iter_state.copy_(src.iter_state)


def _assert_form(tr, ts, form):
    """the launch plan of this step's forward: the kernel the test is about (1 walk in its two-phase tile form, 3 short)"""
    out = (C.c_uint32 * 8)()
    _lib.check(_lib.load().naruto_debug_train_plan(tr.model._handle().ptr, C.byref(ts.t), 1, 1, out))
    assert out[0] == form and out[1] == 1 and (form != 1 or out[2] == 1), list(out)


def _state(tr, ret):
    out = {"rgb": ret["rgb"].clone(), "depth": ret["depth"].clone(), "losses": ret["_losses"].clone()}
    for n, p in tr.model.named_parameters():
        out["p." + n] = p.detach().clone()
    for i, gp in enumerate(tr.map_optimizer.param_groups):
        for j, p in enumerate(gp["params"]):
            m, v = tr.map_optimizer.moments(p)
            out[f"m.{i}.{j}"], out[f"v.{i}.{j}"] = m.clone(), v.clone()
    return out


def _assert_equal_states(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max |d| {(a[k].double() - b[k].double()).abs().max().item():.3e})"


@pytest.mark.parametrize("n_rays,n_samples_d,form", SHAPES)
def test_image_equals_staging(gpu, n_rays, n_samples_d, form):
    """(a): after creation, after 1 fused-Adam iteration and after 3."""
    lib = _lib.load()
    cfg = _cfg(n_samples_d)
    tr = _trainer(cfg, gpu)
    rays = _rays(cfg, n_rays, gpu)
    ts = tr._train_step(n_rays, True)
    assert ts.opt is not None and ts.fwd_image is not None
    _assert_form(tr, ts, form)
    img_bytes = C.c_size_t()
    total = lib.naruto_fwd_image_bytes(C.byref(img_bytes), None)
    assert ts.fwd_image.numel() >= total
    staged = torch.zeros(img_bytes.value, dtype=torch.uint8, device=gpu)

    def check(when):
        staged.fill_(0xA5)
        with torch.cuda.device(gpu):
            _lib.check(lib.naruto_debug_fwd_image(tr.model._handle().ptr, C.byref(ts.ps), staged.data_ptr(), torch.cuda.current_stream().cuda_stream))
        kept = ts.fwd_image[:img_bytes.value]
        bad = (kept != staged).nonzero().flatten()
        assert bad.numel() == 0, f"{when}: {bad.numel()} bytes of the maintained image differ from the staged one, first at {int(bad[0])}"

    check("after creation")
    w0 = tr.model.decoder.sdf_net.model[0].weight.detach().clone()
    for k in range(3):
        tr.step(*rays, smooth=True)
        assert tr._train_step(n_rays, True) is ts
        if k in (0, 2):
            check(f"after {k + 1} iterations")
    assert not torch.equal(w0, tr.model.decoder.sdf_net.model[0].weight)          # (the iterations did step the weights)


def _chain_twin(cfg, gpu, n_rays, image, src=None):
    tr = _trainer(cfg, gpu)
    if src is not None:
        _same_state(tr, src)
    tr.capture(n_rays, smooth=True, chain=CHAIN, fwd_image=image)
    assert tr._static["chain_fwd_image"] is image
    assert tr._static["ts"].t.fwd_image_fresh == 0                # outside the chain's capture nobody is told the image is fresh
    return tr


@pytest.mark.parametrize("n_rays,n_samples_d,form", SHAPES)
def test_chain_with_the_image_gives_the_same_bits(gpu, n_rays, n_samples_d, form):
    """(b) capture(chain=[F,F,F,F,T,F]) with the image on and off from identical state, two replays; then (c): the decoder weights changed in
    place from Python, a third replay against the twin given the same weights."""
    cfg = _cfg(n_samples_d)
    rays = _rays(cfg, n_rays, gpu)
    a = _chain_twin(cfg, gpu, n_rays, True)
    b = _chain_twin(cfg, gpu, n_rays, False, src=a)
    _same_state(b, a)                                         # (capture restores what it found; the twins start from a's state)
    _assert_form(a, a._static["ts"], form)
    for tr in (a, b):
        for buf, r in zip(tr.ray_buffers(), rays):
            buf.copy_(r.reshape(buf.shape))
    for _ in range(2):
        ra, _la = a.step_chain()
        rb, _lb = b.step_chain()
    _assert_equal_states(_state(a, ra), _state(b, rb), "two replays")
    # (c) a stale image: new decoder weights from outside; the buffer still holds the images of the old ones
    with torch.no_grad():
        for tr in (a, b):
            for p in tr.model.decoder.parameters():
                noise = torch.randn(p.shape, generator=torch.Generator().manual_seed(11 + p.numel()))
                p.mul_(0.5).add_(0.05 * noise.to(gpu))
    ra, _la = a.step_chain()
    rb, _lb = b.step_chain()
    _assert_equal_states(_state(a, ra), _state(b, rb), "replay after the weights were changed from outside")


def _ba_scene(cfg, gpu, Hh=24, Ww=32, n_kf=3, R=100, seed=0):
    """a small device-resident keyframe store + current frame + poses"""
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
    return store, current, torch.from_numpy(poses)


def test_fused_ba_call_graph_with_the_image_gives_the_same_bits(gpu, monkeypatch):
    """(b) through FusedBA.call_iterations(): a call of mapping.iters = 6 iterations is one replay of the chained graph; the switch is the
    environment's, read when the graph is captured."""
    from naruto_amd.ba_loop import FusedBA
    cfg = _cfg(32)
    cfg["mapping"].update(sample=24, min_pixels_cur=4, filter_depth=True, keyframe_every=5, iters=len(CHAIN))
    twins = []
    for image in (True, False):
        tr = _trainer(cfg, gpu)
        store, current, poses = _ba_scene(cfg, gpu)
        twins.append((FusedBA(tr, store, None, max_poses=16, use_graph=True), current, poses, image))
    _same_state(twins[1][0].trainer, twins[0][0].trainer)
    out = []
    for ba, current, poses, image in twins:
        monkeypatch.setenv("NARUTO_FWD_WEIGHT_IMAGE", "1" if image else "0")
        for _ in range(2):
            ret, _loss = ba.global_BA(current, poses)             # prepare (captures on the first call) + call_iterations: one replay
        assert ba.trainer.chain_length() == len(CHAIN) and ba.trainer._static["chain_fwd_image"] is image
        out.append(_state(ba.trainer, ret))
    _assert_equal_states(out[0], out[1], "two global_BA calls")

"""Host side of the device tracker (naruto_amd.tracking), no GPU: Rodrigues' formula and its VJP as the tracking kernels compute them
(naruto_debug_rodrigues runs the kernels' own __host__ __device__ code), the interior pixel draw, the C entry points' argument checks
and the tracker's refusals.  No call here passes validation: nothing is launched."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H


def _skew(w):
    z = w[0] * 0
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


@pytest.mark.parametrize("theta", [0.0, 1e-8, 1e-4, 0.5, 3.1])
def test_rodrigues_and_its_vjp_match_fp64_autograd(built_lib, theta):
    from naruto_amd import tracking as TK
    for case in range(3):
        g = torch.Generator().manual_seed(100 * case + int(theta * 1000) + 1)
        axis = torch.randn(3, generator=g, dtype=torch.float64)
        axis = axis / axis.norm()
        w = (axis * theta).requires_grad_(True)
        R = torch.linalg.matrix_exp(_skew(w))
        G = torch.randn(3, 3, generator=g, dtype=torch.float64)
        (R * G).sum().backward()
        wa = (C.c_double * 3)(*w.detach().tolist())
        Ga = (C.c_double * 9)(*G.reshape(-1).tolist())
        Ro, dw = (C.c_double * 9)(), (C.c_double * 3)()
        assert built_lib.naruto_debug_rodrigues(wa, Ga, Ro, dw) == 0
        np.testing.assert_allclose(np.array(Ro[:]).reshape(3, 3), R.detach().numpy(), rtol=0, atol=1e-14)
        np.testing.assert_allclose(np.array(dw[:]), w.grad.numpy(), rtol=1e-10, atol=1e-13)
        # the package's torch restatement of R(omega) (the oracle tests' rays) agrees too
        np.testing.assert_allclose(TK.axis_angle_to_matrix(w.detach()).numpy(), R.detach().numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("theta", [0.0, 1e-6, 0.5, 2.0, 3.1])
def test_axis_angle_round_trip(theta):
    from naruto_amd import tracking as TK
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)
    w = axis / axis.norm() * theta
    np.testing.assert_allclose(TK.matrix_to_axis_angle(TK.axis_angle_to_matrix(w)).numpy(), w.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("Hh,Ww,eh,ew,n", [(120, 160, 20, 20, 1024), (60, 80, 20, 20, 800), (30, 40, 0, 0, 1200), (31, 40, 3, 7, 100)])
def test_interior_pixel_draw(built_lib, Hh, Ww, eh, ew, n):
    """Distinct pixels inside the margins; the flat interior index is h-fastest (h = eh + k % Hi, w = ew + k // Hi) and is the keyed
    permutation's value (salt 4).  Drawing every interior pixel gives each one once."""
    from naruto_amd import tracking as TK
    pix = TK.draw_pixels_host(Hh, Ww, eh, ew, n, seed=12345, counter=7)
    assert len(set(pix.tolist())) == n
    h, w = pix // Ww, pix % Ww
    assert bool((h >= eh).all() and (h < Hh - eh).all() and (w >= ew).all() and (w < Ww - ew).all())
    Hi, Wi = Hh - 2 * eh, Ww - 2 * ew
    k = (w - ew) * Hi + (h - eh)
    assert k.tolist() == [built_lib.naruto_perm_index(i, Hi * Wi, 12345, 7, 4) for i in range(n)]
    if n == Hi * Wi:
        assert sorted(k.tolist()) == list(range(n))
    assert not torch.equal(pix, TK.draw_pixels_host(Hh, Ww, eh, ew, n, seed=12345, counter=8)) or n == Hi * Wi


def test_tracking_entry_points_validate_arguments(built_lib):
    from naruto_amd import _lib
    lib = built_lib
    assert lib.naruto_track_workspace(None, 1024, 43) >= 3 * 4 * 1024 * 43
    assert lib.naruto_track_workspace(None, 1 << 20, 1024) == 0
    assert lib.naruto_track_draw(None, None, None) < 0
    assert b"NULL" in lib.naruto_last_error()
    assert lib.naruto_track_backward(None, None, None, None, None) < 0
    k, t = _lib.NarutoTrackStep(), _lib.NarutoTrainStep()
    assert lib.naruto_track_rays(C.byref(k), C.byref(t), None) < 0          # n_rays 0
    assert b"n_rays" in lib.naruto_last_error()
    k.n_rays, t.n_rays = 16, 32
    assert lib.naruto_track_rays(C.byref(k), C.byref(t), None) < 0          # not the training step's
    t.n_rays = 16
    assert lib.naruto_track_rays(C.byref(k), C.byref(t), None) < 0
    assert b"NULL" in lib.naruto_last_error()
    fake = [0x10000 + 0x100 * i for i in range(32)]                        # never dereferenced: every call below fails validation
    t.rays_o, t.rays_d, t.target_rgb, t.target_d = fake[0:4]
    for j, name in enumerate(("rng", "d_cam", "pose_init", "pose", "exp_avg", "exp_avg_sq", "state", "best_pose", "best_loss", "c2w",
                              "d_rays_o", "d_rays_d", "workspace")):
        setattr(k, name, fake[4 + j])
    k.beta1, k.beta2, k.eps, k.lr_rot, k.lr_trans = 0.9, 0.999, 1e-8, -1.0, 1e-3
    assert lib.naruto_track_rays(C.byref(k), C.byref(t), None) < 0
    assert b"Adam" in lib.naruto_last_error()
    k.lr_rot = 1e-3
    k.trace_loss = fake[20]                                                  # a partial trace
    assert lib.naruto_track_rays(C.byref(k), C.byref(t), None) < 0
    assert b"trace" in lib.naruto_last_error()
    k.trace_loss = None
    assert lib.naruto_track_draw(C.byref(k), C.byref(t), None) < 0           # no frame
    assert b"frame" in lib.naruto_last_error()
    k.direction, k.rgb, k.depth = fake[21:24]
    k.H, k.W, k.edge_h, k.edge_w = 60, 80, 30, 20
    assert lib.naruto_track_draw(C.byref(k), C.byref(t), None) < 0           # no interior left
    assert b"interior" in lib.naruto_last_error()
    k.edge_h, k.n_rays, t.n_rays = 20, 801, 801
    assert lib.naruto_track_draw(C.byref(k), C.byref(t), None) < 0           # 801 of 800 interior pixels
    assert b"800 interior" in lib.naruto_last_error()
    # the backward checks the training step first (NULL parameters / buffers)
    ps = _lib.NarutoParams()
    assert lib.naruto_track_backward(C.c_void_p(fake[24]), C.byref(ps), C.byref(t), C.byref(k), None) < 0
    assert lib.naruto_debug_rodrigues(None, None, None, None) < 0


def test_tracker_refusals():
    from naruto_amd import tracking as TK
    base = H.office_cfg(16)
    cfg = copy.deepcopy(base)
    cfg["tracking"] = {"iter_point": 5}
    with pytest.raises(NotImplementedError, match="tracking_pc"):
        TK.TrackerHIP(None, cfg, 120, 160, device="cpu")
    cfg = copy.deepcopy(base)
    cfg["training"]["rot_rep"] = "quat"
    with pytest.raises(NotImplementedError, match="axis-angle"):
        TK.TrackerHIP(None, cfg, 120, 160, device="cpu")
    cfg = copy.deepcopy(base)
    with pytest.raises(ValueError, match="800 interior"):          # the default 60 x 80 frame with 20-pixel edges
        TK.TrackerHIP(None, cfg, 60, 80, device="cpu")
    cfg["tracking"] = {"ignore_edge_H": 30}
    with pytest.raises(ValueError, match="no interior"):
        TK.TrackerHIP(None, cfg, 60, 80, device="cpu")
    cfg["tracking"] = {"ignore_edge_H": 0, "ignore_edge_W": 0, "sample": 4800}     # no margin: all 60 x 79 pixels, one column short
    with pytest.raises(ValueError, match="out of 4740 interior"):
        TK.TrackerHIP(None, cfg, 60, 79, device="cpu")
    z = torch.zeros(60, 80, 3)
    with pytest.raises(ValueError, match="GPU"):
        TK.check_frame(z, z, torch.zeros(60, 80), 60, 80)
    with pytest.raises(ValueError, match="GPU"):
        TK.check_frame(z.double(), z, torch.zeros(60, 80), 60, 80)
    assert TK.tracking_settings(base) == TK.TRACKING_DEFAULTS


def test_predict_current_pose():
    from naruto_amd import tracking as TK
    a = torch.eye(4, dtype=torch.float64)
    b = TK.pose_matrix(torch.tensor([0.0, 0.0, 0.1, 1.0, 0.5, 0.0], dtype=torch.float64))
    c = TK.predict_current_pose(a, b, True)
    want = TK.pose_matrix(torch.tensor([0.0, 0.0, 0.2, 0.0, 0.0, 0.0], dtype=torch.float64))
    want[:3, 3] = b[:3, 3] + b[:3, :3] @ b[:3, 3]
    np.testing.assert_allclose(c.numpy(), want.numpy(), atol=1e-12)
    assert torch.equal(TK.predict_current_pose(a, b, False), b)

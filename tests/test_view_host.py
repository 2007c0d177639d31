"""Host tests of the view renderer's contract (naruto_amd/render.py): the numpy twin against itself and an independent formulation, the
crossing rule on hand-made rows, the C ABI's structs, the command lines, and run_exploration's unchanged default."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from naruto_amd import _lib

import view_spec as VS


def _images(seed, H=20, W=24):
    rs = np.random.RandomState(seed)
    x = rs.rand(H, W, 3).astype(np.float32)
    y = np.clip(x + 0.1 * rs.randn(H, W, 3), 0, 1).astype(np.float32)
    return x, y


def test_ssim_of_an_image_with_itself_is_exactly_one():
    x, _ = _images(0)
    m = VS.ssim_map(x, x)
    assert m.shape == (10, 14, 3) and bool((m == 1.0).all())
    out = VS.metrics(x, x[..., 0] + 1, x, x[..., 0] + 1)
    assert out["ssim"] == 1.0 and out["psnr"] == float("inf") and out["depth_l1_cm"] == 0.0


def test_twin_agrees_with_a_full_window_formulation():
    signal = pytest.importorskip("scipy.signal")
    x, y = _images(1)
    w = VS.gaussian_window()
    assert abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1])
    w2 = np.outer(w, w)
    got = VS.ssim_map(x, y)
    for c in range(3):
        a, b = x[..., c].astype(np.float64), y[..., c].astype(np.float64)
        f = lambda q: signal.correlate2d(q, w2, mode="valid")                                     # noqa: E731
        mx, my = f(a), f(b)
        sx, sy, sxy = f(a * a) - mx * mx, f(b * b) - my * my, f(a * b) - mx * my
        want = ((2 * mx * my + VS.C1) * (2 * sxy + VS.C2)) / ((mx * mx + my * my + VS.C1) * (sx + sy + VS.C2))
        assert np.abs(got[..., c] - want).max() <= 1e-12
    assert 0.0 < VS.metrics(x, x[..., 0], y, y[..., 0])["ssim"] < 1.0


def test_small_views_and_empty_depth():
    x, y = _images(2, H=10, W=24)
    out = VS.metrics(x, x[..., 0], y, np.zeros((10, 24), np.float32))
    assert np.isnan(out["ssim"]) and np.isnan(out["depth_l1_cm"]) and np.isfinite(out["psnr"])
    d = np.array([[1.0, 2.0, 0.0, 9.0]], np.float32)
    out = VS.metrics(np.zeros((1, 4, 3), np.float32), np.array([[1.5, 1.0, 7.0, 9.0]], np.float32), np.zeros((1, 4, 3), np.float32), d, depth_trunc=5.0)
    assert out["sums"][3] == 2 and out["depth_l1_cm"] == 75.0                                  # (0.5 + 1.0) / 2 m; d = 0 and d > trunc are out


def test_crossing_rule_on_hand_made_rows():
    nan = float("nan")
    z = np.arange(5, dtype=np.float32)[None].repeat(7, 0) + 1
    sdf = np.array([[1.0, 0.8, 0.6, 0.4, 0.2],            # no crossing
                    [1.0, 0.8, 0.6, 0.4, -0.4],           # at the last pair
                    [1.0, nan, -1.0, 1.0, -1.0],          # a NaN counts as not positive: k = 0, z* NaN
                    [-1.0, 1.0, 3.0, -1.0, 1.0],          # sdf[0] <= 0: the first pair that starts positive is k = 2
                    [0.5, 0.0, -1.0, 1.0, -1.0],          # a tie at exactly 0 is a crossing (not positive): z* = z[1] exactly
                    [0.0, 0.0, -1.0, -2.0, -3.0],         # never positive
                    [nan, 1.0, -3.0, 0.0, 0.0]], np.float32)
    got, k = VS.crossing(sdf, z)
    assert k.tolist() == [-1, 3, 0, 2, 0, -1, 1]
    assert got[0] == 0 and got[5] == 0
    assert got[1] == np.float32(4) + np.float32(1) * (np.float32(0.4) / (np.float32(0.4) - np.float32(-0.4)))
    assert np.isnan(got[2])
    assert got[3] == np.float32(3.75) and got[4] == np.float32(2.0) and got[6] == np.float32(2.25)


def test_rays_of_the_twin_equal_camera_rays_and_a_rotation():
    from naruto_amd.slam import camera_rays
    cam = dict(H=5, W=7, fx=3.0, fy=2.5, cx=3.25, cy=1.75)
    assert np.array_equal(VS.camera_dirs(**cam), camera_rays(**cam).numpy())
    P = np.eye(4, dtype=np.float32)[None].repeat(2, 0)
    P[1, :3, :3] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    P[1, :3, 3] = [1, 2, 3]
    o, d = VS.view_rays(P, cam, 30, 40)                     # spans the two poses, starts and ends mid-row
    dirs = VS.camera_dirs(**cam).reshape(-1, 3)
    assert np.array_equal(d[:5], dirs[30:35]) and np.array_equal(o[:5], np.zeros((5, 3), np.float32))
    assert np.array_equal(d[5:, 0], -dirs[:5, 1]) and np.array_equal(d[5:, 1], dirs[:5, 0]) and np.array_equal(o[5:], np.tile(np.float32([1, 2, 3]), (5, 1)))


def test_new_abi_symbols_and_argument_checks(built_lib):
    header = open(_lib.HEADER).read()
    want = {"naruto_view_rays": (C.c_int, 8), "naruto_view_crossing": (C.c_int, 6), "naruto_render_view": (C.c_int, 5),
            "naruto_image_metrics_workspace": (C.c_size_t, 3), "naruto_image_metrics": (C.c_int, 16)}
    for name, (res, n_args) in want.items():
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args, name
        decl = header[header.rindex(name + "("):]                              # (the last mention is the declaration: the comment above names some)
        assert decl[:decl.index(";")].count(",") + 1 == n_args, name
        assert hasattr(built_lib, name)
    assert "naruto_view.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "naruto_view.hip"))
    cam = _lib.NarutoCullCam(4, 6, 1.5, 1.5, 1.5, 1.5, 0.0, 5.0)
    one = C.c_void_p(8)                                                        # never dereferenced: every call below fails its checks first
    assert built_lib.naruto_view_rays(C.byref(cam), 2, one, 0, 49, one, one, None) != 0 and b"pixel range" in built_lib.naruto_last_error()
    assert built_lib.naruto_view_rays(C.byref(cam), 2, one, 5, 4, one, one, None) != 0
    assert built_lib.naruto_view_rays(C.byref(cam), 0, one, 0, 0, one, one, None) != 0
    assert built_lib.naruto_view_crossing(4, 1, one, one, one, None) != 0 and built_lib.naruto_view_crossing(4, 1025, one, one, one, None) != 0
    assert built_lib.naruto_image_metrics_workspace(0, 4, 4) == 0 and built_lib.naruto_image_metrics_workspace(1, 0, 4) == 0
    assert built_lib.naruto_image_metrics_workspace(3, 20, 24) >= 3 * 2 * 2 * 6 * 8
    win = (C.c_double * 11)()
    assert built_lib.naruto_image_metrics(1, 4, 4, one, one, one, None, 0, 0.0, win, one, one, None, None, None, None) != 0


def test_view_kernels_keep_the_render_kernels_budget(built_lib):
    """No vector register spilled, no scratch, inside the 256 registers of the render kernels' two waves per SIMD, and the static LDS of the render
    kernel each one extends (the packed form adds the 16 rays' origins, directions and z*: 448 bytes)."""
    res = _lib.kernel_resources()
    for mine, base, extra_lds in (("k_render_view<false>", "k_render_fwd<false>", 0), ("k_render_view<true>", "k_render_fwd<true>", 0),
                                  ("k_render_view_packed<false>", "k_render_fwd_packed<false,256>", 448), ("k_render_view_packed<true>", "k_render_fwd_packed<true,256>", 448)):
        k, b = res[mine], res[base]
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (mine, k)
        assert k["vgpr_count"] + k["agpr_count"] <= 256 and k["group_segment_fixed_size"] == b["group_segment_fixed_size"] + extra_lds, (mine, k, b)
    for name in ("k_view_rays", "k_view_crossing", "k_metrics_tile", "k_metrics_finish"):
        assert res[name]["vgpr_spill_count"] == 0 and res[name]["sgpr_spill_count"] == 0 and res[name]["private_segment_fixed_size"] == 0, (name, res[name])


def test_render_refuses_sample_counts_beyond_the_ray_limit():
    from naruto_amd import render as R
    import helpers as H
    cfg = H.office_cfg(12)
    cfg["cam"].update(H=4, W=6)
    r = R.FieldViewRendererHIP(None, cfg)
    assert (r.H, r.W, r.cam.near_, r.cam.far_) == (4, 6, 0.0, 5.0)
    with pytest.raises(ValueError, match="n_coarse"):
        r.render(torch.eye(4)[None], n_coarse=1025)
    with pytest.raises(ValueError, match="n_coarse"):
        r.render(torch.eye(4)[None], n_coarse=1)
    with pytest.raises(ValueError, match="outputs"):
        r.render(torch.eye(4)[None], outputs=("rgb", "normals"))
    cfg["training"]["n_samples_d"] = 1020
    with pytest.raises(ValueError, match="fine samples"):
        R.FieldViewRendererHIP(None, cfg).render(torch.eye(4)[None])
    with pytest.raises(ValueError, match="near < far"):
        R.FieldViewRendererHIP(None, cfg, cam=dict(H=4, W=6, fx=1, fy=1, cx=1, cy=1, near=2.0, far=1.0))
    w = R.gaussian_window()
    assert np.array_equal(w, VS.gaussian_window())
    s = np.array([[3.0, 1.0, 2.0, 4.0, 0.0, 0.0]])
    sc = R.scores_from_sums(s)
    assert sc["psnr"][0] == 0.0 and sc["depth_l1_cm"][0] == 50.0 and np.isnan(sc["ssim"][0])


def test_command_lines():
    from naruto_amd import render as R
    from naruto_amd import run as RUN
    a = R.parse_args(["--config", "c.yaml", "--ckpt", "k.pt", "--mesh", "m.ply", "--traj", "t.txt", "--out_dir", "o", "--every", "5", "--png", "--result_txt", "r.txt"])
    assert (a.traj, a.poses, a.every, a.png, a.result_txt, a.depth_guided) == ("t.txt", False, 5, True, "r.txt", False)
    a = R.parse_args(["--config", "c.yaml", "--ckpt", "k.pt", "--mesh", "m.ply", "--poses", "--out_dir", "o"])
    assert a.poses and a.traj is None and a.every == 1 and not a.png and a.result_txt is None
    for bad in (["--traj", "t.txt", "--poses"], [], ["--poses", "--every", "0"]):
        with pytest.raises(SystemExit):
            R.parse_args(["--config", "c.yaml", "--ckpt", "k.pt", "--mesh", "m.ply", "--out_dir", "o"] + bad)
    with pytest.raises(SystemExit):
        R.parse_args(["--config", "c.yaml", "--ckpt", "k.pt", "--mesh", "m.obj", "--poses", "--out_dir", "o"])
    base = ["--config", "c.yaml", "--mesh", "m.ply", "--num_iter", "4", "--result_dir", "d"]
    assert RUN.parse_args(base).eval_views is None and RUN.parse_args(base + ["--eval_views", "2"]).eval_views == 2
    with pytest.raises(SystemExit):
        RUN.parse_args(base + ["--eval_views", "0"])
    assert R.results_rows({"psnr": 1.0, "ssim": 0.5, "depth_l1_cm": 2.0}) == {"psnr": 1.0, "ssim": 0.5, "depth_l1(cm)": 2.0}


class _Slam:
    result_dir, config = None, {"mesh": {"voxel_final": 0.1}}

    def online_recon_step(self, i, color, depth, c2w):
        return None

    def save_mesh(self, i, voxel_size, suffix):
        return "mesh"


class _Sim:
    def simulate(self, c2w, no_print=False):
        return None, None


def test_default_run_keeps_its_result_keys():
    from naruto_amd.run import run_exploration
    traj = torch.eye(4)[None].repeat(3, 1, 1)
    out = run_exploration(_Slam(), _Sim(), None, None, 3, traj=traj)
    assert set(out) == {"poses", "states", "fresh", "timing", "mesh", "ckpt_path"}
    assert set(run_exploration(_Slam(), _Sim(), None, None, 3, traj=traj, eval_views=None)) == set(out)
    with pytest.raises(ValueError, match="eval_views"):
        run_exploration(_Slam(), _Sim(), None, None, 3, traj=traj, eval_views=0)

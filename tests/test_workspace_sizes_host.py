"""Every naruto_*_workspace() size is ABI: callers allocate by it, and the launchers carve their sections from the same layout function
(the Carve cursor of naruto_api.hip).  The table below was recorded by running this file's own argument list (``_sizes``) against the
library of the commit BEFORE the layouts were restated with that cursor -- never against the code under test -- so a layout edit that
moves a byte shows here.  Host only: field creation and the size functions need no device, and without one the field plans for 256
CUs, the MI355X count."""
import ctypes as C

from naruto_amd import _lib

LIST_M = (1, 3, 4, 5, 1000, 300000, 300001, 1500000, 1500001)             # edges of list_cap, xcd_aware and split_multiplier
FIELDS = tuple((T, mode) for T in (12, 16, 22) for mode in ("fp32", "bf16"))          # T = 22 has binned levels (its scatter grows with M)
TRAIN = ((1, 1, 1, 0), (128, 32, 11, 0), (2048, 32, 11, 33), (2048, 64, 0, 257))       # rays, n_samples_d, n_range_d, smooth_points
DIMS = ((1, 1, 1), (4, 5, 6), (65, 33, 17))
RASTER = ((1, 1, 1), (100, 200, 8))                                       # vertices, faces, poses


def _sizes(lib):
    from naruto_amd import ops
    out = {}
    for T, mode in FIELDS:
        h = ops.FieldHandle(log2_hashmap_size=T, per_level_scale=1.38, uncert_dims=(4, 5, 6), bbox_min=(0, 0, 0), bbox_max=(1, 1, 1),
                            trunc=0.1, sc_factor=1.0, mlp_mode=mode)
        for M in LIST_M:
            for fn in ("scatter", "query_bwd", "query_bwd_points"):
                out[f"{fn} T={T} {mode} M={M}"] = getattr(lib, f"naruto_{fn}_workspace")(h.ptr, M)
        for N, nd, nr, sp in TRAIN:
            t = _lib.NarutoTrainStep()
            t.n_rays, t.n_samples_d, t.n_range_d, t.smooth_points = N, nd, nr, sp
            out[f"train T={T} {mode} {N}x({nd}+{nr}) smooth={sp}"] = lib.naruto_train_workspace(h.ptr, C.byref(t))
        for N, S in ((1, 2), (1024, 43)):
            out[f"track T={T} {mode} {N}x{S}"] = lib.naruto_track_workspace(h.ptr, N, S)
            out[f"ba_poses T={T} {mode} {N}x{S}"] = lib.naruto_ba_poses_workspace(h.ptr, N, S)
    for sp in (0, 1, 2, 3, 33, 257):
        out[f"smoothness {sp}"] = lib.naruto_smoothness_workspace(sp)
    for N in (1, 2048):
        out[f"loss {N}"] = lib.naruto_loss_workspace(N)
    out["active_ray 100,10"] = lib.naruto_active_ray_workspace(100, 10)
    out["goal_targets 120,8"] = lib.naruto_goal_targets_workspace(120, 8)
    for d in DIMS:
        dims = (C.c_uint32 * 3)(*d)
        out[f"rrt {d}"] = lib.naruto_rrt_workspace(dims)
        out[f"mesh {d}"] = lib.naruto_mesh_workspace(dims)
    for n in (100, 100000):
        g = _lib.NarutoNnGrid()
        assert lib.naruto_nn_grid_plan(n, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 2, 3), 0.0, 0, C.byref(g)) == 0
        out[f"nn_grid {n} dims={tuple(g.dims)}"] = lib.naruto_nn_grid_workspace(C.byref(g))
    for n in (1, 200000, 2 ** 31 - 1):
        out[f"dist_reduce {n}"] = lib.naruto_dist_reduce_workspace(n)
    for r in RASTER:
        out[f"render_depth {r}"] = lib.naruto_render_depth_workspace(*r)
        for hw in ((1, 1), (6, 8)):
            out[f"render_rgbd {r} {hw}"] = lib.naruto_render_rgbd_workspace(*r, *hw)
    return out


EXPECTED = {
    'scatter T=12 fp32 M=1': 4198144,
    'query_bwd T=12 fp32 M=1': 18878848,
    'query_bwd_points T=12 fp32 M=1': 268,
    'scatter T=12 fp32 M=3': 4198144,
    'query_bwd T=12 fp32 M=3': 18878848,
    'query_bwd_points T=12 fp32 M=3': 292,
    'scatter T=12 fp32 M=4': 4198144,
    'query_bwd T=12 fp32 M=4': 18878848,
    'query_bwd_points T=12 fp32 M=4': 304,
    'scatter T=12 fp32 M=5': 4198144,
    'query_bwd T=12 fp32 M=5': 18879424,
    'query_bwd_points T=12 fp32 M=5': 316,
    'scatter T=12 fp32 M=1000': 4198144,
    'query_bwd T=12 fp32 M=1000': 19022272,
    'query_bwd_points T=12 fp32 M=1000': 12256,
    'scatter T=12 fp32 M=300000': 4198144,
    'query_bwd T=12 fp32 M=300000': 62078272,
    'query_bwd_points T=12 fp32 M=300000': 3600256,
    'scatter T=12 fp32 M=300001': 4198144,
    'query_bwd T=12 fp32 M=300001': 62078848,
    'query_bwd_points T=12 fp32 M=300001': 3600268,
    'scatter T=12 fp32 M=1500000': 4198144,
    'query_bwd T=12 fp32 M=1500000': 234878272,
    'query_bwd_points T=12 fp32 M=1500000': 18000256,
    'scatter T=12 fp32 M=1500001': 4198144,
    'query_bwd T=12 fp32 M=1500001': 234878848,
    'query_bwd_points T=12 fp32 M=1500001': 18000268,
    'train T=12 fp32 1x(1+1) smooth=0': 22094592,
    'train T=12 fp32 128x(32+11) smooth=0': 23046912,
    'train T=12 fp32 2048x(32+11) smooth=33': 46287104,
    'train T=12 fp32 2048x(64+0) smooth=257': 4608185856,
    'track T=12 fp32 1x2': 280,
    'ba_poses T=12 fp32 1x2': 280,
    'track T=12 fp32 1024x43': 528640,
    'ba_poses T=12 fp32 1024x43': 528640,
    'scatter T=12 bf16 M=1': 4198144,
    'query_bwd T=12 bf16 M=1': 18878848,
    'query_bwd_points T=12 bf16 M=1': 268,
    'scatter T=12 bf16 M=3': 4198144,
    'query_bwd T=12 bf16 M=3': 18878848,
    'query_bwd_points T=12 bf16 M=3': 292,
    'scatter T=12 bf16 M=4': 4198144,
    'query_bwd T=12 bf16 M=4': 18878848,
    'query_bwd_points T=12 bf16 M=4': 304,
    'scatter T=12 bf16 M=5': 4198144,
    'query_bwd T=12 bf16 M=5': 18879424,
    'query_bwd_points T=12 bf16 M=5': 316,
    'scatter T=12 bf16 M=1000': 4198144,
    'query_bwd T=12 bf16 M=1000': 19022272,
    'query_bwd_points T=12 bf16 M=1000': 12256,
    'scatter T=12 bf16 M=300000': 4198144,
    'query_bwd T=12 bf16 M=300000': 62078272,
    'query_bwd_points T=12 bf16 M=300000': 3600256,
    'scatter T=12 bf16 M=300001': 4198144,
    'query_bwd T=12 bf16 M=300001': 62078848,
    'query_bwd_points T=12 bf16 M=300001': 3600268,
    'scatter T=12 bf16 M=1500000': 4198144,
    'query_bwd T=12 bf16 M=1500000': 234878272,
    'query_bwd_points T=12 bf16 M=1500000': 18000256,
    'scatter T=12 bf16 M=1500001': 4198144,
    'query_bwd T=12 bf16 M=1500001': 234878848,
    'query_bwd_points T=12 bf16 M=1500001': 18000268,
    'train T=12 bf16 1x(1+1) smooth=0': 22094592,
    'train T=12 bf16 128x(32+11) smooth=0': 23046912,
    'train T=12 bf16 2048x(32+11) smooth=33': 46287104,
    'train T=12 bf16 2048x(64+0) smooth=257': 4608185856,
    'track T=12 bf16 1x2': 280,
    'ba_poses T=12 bf16 1x2': 280,
    'track T=12 bf16 1024x43': 528640,
    'ba_poses T=12 bf16 1024x43': 528640,
    'scatter T=16 fp32 M=1': 28738304,
    'query_bwd T=16 fp32 M=1': 43419008,
    'query_bwd_points T=16 fp32 M=1': 268,
    'scatter T=16 fp32 M=3': 28738304,
    'query_bwd T=16 fp32 M=3': 43419008,
    'query_bwd_points T=16 fp32 M=3': 292,
    'scatter T=16 fp32 M=4': 28738304,
    'query_bwd T=16 fp32 M=4': 43419008,
    'query_bwd_points T=16 fp32 M=4': 304,
    'scatter T=16 fp32 M=5': 28738304,
    'query_bwd T=16 fp32 M=5': 43419584,
    'query_bwd_points T=16 fp32 M=5': 316,
    'scatter T=16 fp32 M=1000': 28738304,
    'query_bwd T=16 fp32 M=1000': 43562432,
    'query_bwd_points T=16 fp32 M=1000': 12256,
    'scatter T=16 fp32 M=300000': 28738304,
    'query_bwd T=16 fp32 M=300000': 86618432,
    'query_bwd_points T=16 fp32 M=300000': 3600256,
    'scatter T=16 fp32 M=300001': 28738304,
    'query_bwd T=16 fp32 M=300001': 86619008,
    'query_bwd_points T=16 fp32 M=300001': 3600268,
    'scatter T=16 fp32 M=1500000': 28739840,
    'query_bwd T=16 fp32 M=1500000': 259419968,
    'query_bwd_points T=16 fp32 M=1500000': 18000256,
    'scatter T=16 fp32 M=1500001': 57476608,
    'query_bwd T=16 fp32 M=1500001': 288157312,
    'query_bwd_points T=16 fp32 M=1500001': 18000268,
    'train T=16 fp32 1x(1+1) smooth=0': 46634752,
    'train T=16 fp32 128x(32+11) smooth=0': 47587072,
    'train T=16 fp32 2048x(32+11) smooth=33': 70827264,
    'train T=16 fp32 2048x(64+0) smooth=257': 4661465088,
    'track T=16 fp32 1x2': 280,
    'ba_poses T=16 fp32 1x2': 280,
    'track T=16 fp32 1024x43': 528640,
    'ba_poses T=16 fp32 1024x43': 528640,
    'scatter T=16 bf16 M=1': 28738304,
    'query_bwd T=16 bf16 M=1': 43419008,
    'query_bwd_points T=16 bf16 M=1': 268,
    'scatter T=16 bf16 M=3': 28738304,
    'query_bwd T=16 bf16 M=3': 43419008,
    'query_bwd_points T=16 bf16 M=3': 292,
    'scatter T=16 bf16 M=4': 28738304,
    'query_bwd T=16 bf16 M=4': 43419008,
    'query_bwd_points T=16 bf16 M=4': 304,
    'scatter T=16 bf16 M=5': 28738304,
    'query_bwd T=16 bf16 M=5': 43419584,
    'query_bwd_points T=16 bf16 M=5': 316,
    'scatter T=16 bf16 M=1000': 28738304,
    'query_bwd T=16 bf16 M=1000': 43562432,
    'query_bwd_points T=16 bf16 M=1000': 12256,
    'scatter T=16 bf16 M=300000': 28738304,
    'query_bwd T=16 bf16 M=300000': 86618432,
    'query_bwd_points T=16 bf16 M=300000': 3600256,
    'scatter T=16 bf16 M=300001': 28738304,
    'query_bwd T=16 bf16 M=300001': 86619008,
    'query_bwd_points T=16 bf16 M=300001': 3600268,
    'scatter T=16 bf16 M=1500000': 28739840,
    'query_bwd T=16 bf16 M=1500000': 259419968,
    'query_bwd_points T=16 bf16 M=1500000': 18000256,
    'scatter T=16 bf16 M=1500001': 57476608,
    'query_bwd T=16 bf16 M=1500001': 288157312,
    'query_bwd_points T=16 bf16 M=1500001': 18000268,
    'train T=16 bf16 1x(1+1) smooth=0': 46634752,
    'train T=16 bf16 128x(32+11) smooth=0': 47587072,
    'train T=16 bf16 2048x(32+11) smooth=33': 70827264,
    'train T=16 bf16 2048x(64+0) smooth=257': 4661465088,
    'track T=16 bf16 1x2': 280,
    'ba_poses T=16 bf16 1x2': 280,
    'track T=16 bf16 1024x43': 528640,
    'ba_poses T=16 bf16 1024x43': 528640,
    'scatter T=22 fp32 M=1': 8099328,
    'query_bwd T=22 fp32 M=1': 22784640,
    'query_bwd_points T=22 fp32 M=1': 268,
    'scatter T=22 fp32 M=3': 8102400,
    'query_bwd T=22 fp32 M=3': 22784640,
    'query_bwd_points T=22 fp32 M=3': 292,
    'scatter T=22 fp32 M=4': 8103936,
    'query_bwd T=22 fp32 M=4': 22784640,
    'query_bwd_points T=22 fp32 M=4': 304,
    'scatter T=22 fp32 M=5': 8105472,
    'query_bwd T=22 fp32 M=5': 22791360,
    'query_bwd_points T=22 fp32 M=5': 316,
    'scatter T=22 fp32 M=1000': 9633792,
    'query_bwd T=22 fp32 M=1000': 24457920,
    'query_bwd_points T=22 fp32 M=1000': 12256,
    'scatter T=22 fp32 M=300000': 473785600,
    'query_bwd T=22 fp32 M=300000': 531665728,
    'query_bwd_points T=22 fp32 M=300000': 3600256,
    'scatter T=22 fp32 M=300001': 473787136,
    'query_bwd T=22 fp32 M=300001': 531672448,
    'query_bwd_points T=22 fp32 M=300001': 3600268,
    'scatter T=22 fp32 M=1500000': 2316985600,
    'query_bwd T=22 fp32 M=1500000': 2547665728,
    'query_bwd_points T=22 fp32 M=1500000': 18000256,
    'scatter T=22 fp32 M=1500001': 2316987136,
    'query_bwd T=22 fp32 M=1500001': 2547672448,
    'query_bwd_points T=22 fp32 M=1500001': 18000268,
    'train T=22 fp32 1x(1+1) smooth=0': 26000384,
    'train T=22 fp32 128x(32+11) smooth=0': 35496704,
    'train T=22 fp32 2048x(32+11) smooth=33': 238027520,
    'train T=22 fp32 2048x(64+0) smooth=257': 30588103680,
    'track T=22 fp32 1x2': 280,
    'ba_poses T=22 fp32 1x2': 280,
    'track T=22 fp32 1024x43': 528640,
    'ba_poses T=22 fp32 1024x43': 528640,
    'scatter T=22 bf16 M=1': 8099328,
    'query_bwd T=22 bf16 M=1': 22784640,
    'query_bwd_points T=22 bf16 M=1': 268,
    'scatter T=22 bf16 M=3': 8102400,
    'query_bwd T=22 bf16 M=3': 22784640,
    'query_bwd_points T=22 bf16 M=3': 292,
    'scatter T=22 bf16 M=4': 8103936,
    'query_bwd T=22 bf16 M=4': 22784640,
    'query_bwd_points T=22 bf16 M=4': 304,
    'scatter T=22 bf16 M=5': 8105472,
    'query_bwd T=22 bf16 M=5': 22791360,
    'query_bwd_points T=22 bf16 M=5': 316,
    'scatter T=22 bf16 M=1000': 9633792,
    'query_bwd T=22 bf16 M=1000': 24457920,
    'query_bwd_points T=22 bf16 M=1000': 12256,
    'scatter T=22 bf16 M=300000': 473785600,
    'query_bwd T=22 bf16 M=300000': 531665728,
    'query_bwd_points T=22 bf16 M=300000': 3600256,
    'scatter T=22 bf16 M=300001': 473787136,
    'query_bwd T=22 bf16 M=300001': 531672448,
    'query_bwd_points T=22 bf16 M=300001': 3600268,
    'scatter T=22 bf16 M=1500000': 2316985600,
    'query_bwd T=22 bf16 M=1500000': 2547665728,
    'query_bwd_points T=22 bf16 M=1500000': 18000256,
    'scatter T=22 bf16 M=1500001': 2316987136,
    'query_bwd T=22 bf16 M=1500001': 2547672448,
    'query_bwd_points T=22 bf16 M=1500001': 18000268,
    'train T=22 bf16 1x(1+1) smooth=0': 26000384,
    'train T=22 bf16 128x(32+11) smooth=0': 35496704,
    'train T=22 bf16 2048x(32+11) smooth=33': 238027520,
    'train T=22 bf16 2048x(64+0) smooth=257': 30588103680,
    'track T=22 bf16 1x2': 280,
    'ba_poses T=22 bf16 1x2': 280,
    'track T=22 bf16 1024x43': 528640,
    'ba_poses T=22 bf16 1024x43': 528640,
    'smoothness 0': 200,
    'smoothness 1': 200,
    'smoothness 2': 200,
    'smoothness 3': 1096,
    'smoothness 33': 4227136,
    'smoothness 257': 2164260928,
    'loss 1': 64,
    'loss 2048': 131072,
    'active_ray 100,10': 504,
    'goal_targets 120,8': 768,
    'rrt (1, 1, 1)': 132,
    'mesh (1, 1, 1)': 1024,
    'rrt (4, 5, 6)': 608,
    'mesh (4, 5, 6)': 1792,
    'rrt (65, 33, 17)': 145988,
    'mesh (65, 33, 17)': 365312,
    'nn_grid 100 dims=(2, 3, 4)': 1024,
    'nn_grid 100000 dims=(34, 68, 102)': 1344000,
    'dist_reduce 1': 512,
    'dist_reduce 200000': 2048,
    'dist_reduce 2147483647': 16777216,
    'render_depth (1, 1, 1)': 1024,
    'render_rgbd (1, 1, 1) (1, 1)': 1280,
    'render_rgbd (1, 1, 1) (6, 8)': 1536,
    'render_depth (100, 200, 8)': 32256,
    'render_rgbd (100, 200, 8) (1, 1)': 32512,
    'render_rgbd (100, 200, 8) (6, 8)': 35328,
}


def test_every_workspace_size_is_what_it_was(built_lib):
    got = _sizes(built_lib)
    assert set(got) == set(EXPECTED), sorted(set(got) ^ set(EXPECTED))
    assert all(v > 0 for v in EXPECTED.values())
    bad = {k: (got[k], EXPECTED[k]) for k in EXPECTED if got[k] != EXPECTED[k]}
    assert not bad, f"(got, expected) bytes: {bad}"

"""GPU tests of the textured mesh simulator (naruto_amd/simulator.py -> C ABI -> k_tex_down and k_sim_shade_tex of csrc/naruto_sim.hip)
against the numpy restatement tests/sim_texture_spec.py: the mip chains equal it in every byte; colour equals it in every bit whatever
the launch plan; depth and face id are the untextured render's bits; the panorama; the C boundary's guards; a run from a .glb."""
import ctypes as C

import numpy as np
import pytest
import torch

import cull_spec as CS
import gltf_scene as GS
import sim_spec as SS
import sim_texture_spec as TS

pytestmark = pytest.mark.gpu

FAR = 100.0


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(got, want, what=""):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = a != b
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def _mesh(s):
    from naruto_amd.mesh import Material, TexturedMesh
    return TexturedMesh(s.vertices, s.faces, s.vertex_colors, uv=s.uv, face_material=s.face_material, materials=[Material(*m) for m in s.materials], textures=s.textures)


def _sim(mesh, cam=TS.CAMERA, **kw):
    from naruto_amd import simulator as SIM
    kw.setdefault("erp_hw", (16, 32))
    kw.setdefault("face_w", 16)
    return SIM.MeshSimHIP(mesh, cam, far=FAR, **kw)


@pytest.fixture(scope="module")
def box(gpu):
    """The textured box from three poses at 40 x 30 and the restatement's frames of it (computed once, never written to).  The condition
    on the input is checked here, on the restatement, before any test looks at the device."""
    s, poses, info = TS.textured_box(), TS.box_poses(), {}
    depth, colour, fid = TS.render_rgbd_tex(s, poses, TS.CAMERA, far=FAR, info=info)
    for a in (depth, colour, fid):
        a.setflags(write=False)
    per_texture = {t: sorted(l for tt, l in info["levels"] if tt == t) for t in range(3)}
    chains = [TS.n_levels(im.shape[1], im.shape[0]) for im in s.textures]
    assert all(per_texture[t] for t in range(3)), per_texture                                                     # every texture is seen
    assert any(l == 0 for ls in per_texture.values() for l in ls)
    assert max(sum(1 for l in per_texture[t] if 0 < l < chains[t] - 1) for t in range(3)) >= 2, per_texture     # two intermediate levels
    assert any(per_texture[t][-1] == chains[t] - 1 for t in range(3)), per_texture                               # a texture's last level
    assert info["negative"] == {(axis, m) for axis in "st" for m in TS.WRAPS}, info["negative"]                  # every wrap mode, each axis
    walls = s.wall[fid[fid >= 0]]
    assert set(np.unique(walls)) == set(range(6)) and (fid >= 0).all()
    return {"scene": s, "poses": poses, "depth": depth, "colour": colour, "fid": fid}


@pytest.mark.parametrize("sizes", [[(1, 1)], [(5, 3)], [(64, 16)], [(16, 64)], [(5, 3), (1, 1), (16, 64), (64, 16)]], ids=["1x1", "5x3", "64x16", "16x64", "four"])
def test_pyramid_equals_the_restatement_in_every_byte(gpu, sizes):
    from naruto_amd import simulator as SIM
    images = [TS.hashed_image(h, w, 7 + k) for k, (w, h) in enumerate(sizes)]
    want_bytes, want_desc = TS.pyramid_buffer(images)
    texels, desc = SIM.texture_pyramid(images, gpu)
    assert texels.is_cuda and texels.dtype == torch.int32 and desc.dtype == torch.int32
    assert np.array_equal(_np(desc), want_desc)
    got = _np(texels).view(np.uint8)
    assert got.shape == want_bytes.shape and np.array_equal(got, want_bytes), np.argwhere(got != want_bytes)[:5]
    assert want_desc[:, 3].tolist() == [1 + int(np.floor(np.log2(max(w, h)))) for w, h in sizes]


def test_pyramid_refuses_what_it_cannot_hold(gpu):
    from naruto_amd import simulator as SIM
    for bad in ([], [np.zeros((2, 2, 3), dtype=np.uint8)], [np.zeros((2, 2, 4), dtype=np.float32)], [np.zeros((1, 16385, 4), dtype=np.uint8)]):
        with pytest.raises(ValueError, match="texture"):
            SIM.texture_pyramid(bad, gpu)


def test_textured_frames_equal_the_restatement_in_every_bit(gpu, box):
    s = box["scene"]
    color, depth, fid = _sim(_mesh(s)).simulate_batch(box["poses"], pose_chunk=2, return_face_id=True)
    _same_bits(color, box["colour"], "colour")
    _same_bits(depth, box["depth"], "depth")
    _same_bits(fid, box["fid"], "face id")
    # depth and face id are the untextured render's bits; the faces without a material are its colours too
    plain = _sim((s.vertices, s.faces, s.vertex_colors))
    assert plain.tex is None
    c0, d0, f0 = plain.simulate_batch(box["poses"], pose_chunk=2, return_face_id=True)
    assert torch.equal(depth.view(torch.int32), d0.view(torch.int32)) and torch.equal(fid, f0)
    bare = s.face_material[box["fid"]] < 0
    assert bare.sum() > 300
    t, _ = SS.render_winner(s.vertices, s.faces, box["poses"], TS.CAMERA, far=FAR)
    _, want = SS.shade(s.vertices, s.faces, s.vertex_colors, box["poses"], TS.CAMERA, t, box["fid"])
    _same_bits(_np(color)[bare], want[bare], "faces without a material")
    _same_bits(_np(color)[bare], _np(c0)[bare], "faces without a material, the untextured render")
    # the factor-only wall is its factor
    flat = s.wall[box["fid"]] == 3
    assert flat.sum() > 100 and (_np(color)[flat] == np.float32([0.2, 0.4, 0.6])).all()
    assert len(np.unique(_np(color)[~bare & ~flat])) > 500                                                        # textured, not flat


@pytest.mark.parametrize("threshold", [0, 2 ** 32], ids=["all-large", "all-small"])
@pytest.mark.parametrize("pose_chunk", [1, 3])
def test_no_bit_depends_on_the_launch_plan(gpu, box, threshold, pose_chunk):
    from naruto_amd import culling as CU
    sim = _sim(_mesh(box["scene"]), plan=CU.RasterPlan(threshold))
    color, depth, fid = sim.simulate_batch(box["poses"], pose_chunk=pose_chunk, return_face_id=True)
    _same_bits(color, box["colour"], "colour")
    _same_bits(depth, box["depth"], "depth")
    _same_bits(fid, box["fid"], "face id")


def test_panorama_is_textured(gpu, box):
    from naruto_amd import simulator as SIM
    s, pose = box["scene"], box["poses"][0]
    sim = _sim(_mesh(s))
    color, depth, erp_color, erp_dist = sim.simulate(pose, return_erp=True, no_print=True)
    want_c, want_d = TS.erp_tex(s, pose, 16, SIM.cube_table(16, 16, 32), far=FAR)
    _same_bits(erp_color, want_c, "erp colour")
    _same_bits(erp_dist, want_d, "erp distance")
    _same_bits(color, box["colour"][0], "colour")
    plain_c, plain_d = SS.erp(s.vertices, s.faces, s.vertex_colors, pose, 16, SIM.cube_table(16, 16, 32), far=FAR)
    assert np.array_equal(plain_d, want_d) and (plain_c != want_c).any()


def test_c_boundary_guards(gpu, box):
    """A material id or a texture index out of range (which MeshSimHIP refuses on the host) reaches the kernel: those faces take the
    vertex-colour path and nothing is read through the index.  A NarutoSimTextures shorter than the library's is refused."""
    from naruto_amd import _lib
    s = box["scene"]
    sim = _sim(_mesh(s))
    t, _ = SS.render_winner(s.vertices, s.faces, box["poses"], TS.CAMERA, far=FAR)
    _, vertex = SS.shade(s.vertices, s.faces, s.vertex_colors, box["poses"], TS.CAMERA, t, box["fid"])
    # wall 0's faces name material 1000; material 1 (wall 1) names texture 3 of 3; material 2 (wall 2) names texture 2^31 - 1
    fm = s.face_material.copy()
    fm[s.wall == 0] = 1000
    sim.tex.face_material.copy_(torch.from_numpy(fm))
    table = sim.tex.materials.clone()
    table[1, 0], table[2, 0] = 3, 2 ** 31 - 1
    sim.tex.materials.copy_(table)
    color = sim.simulate_batch(box["poses"], pose_chunk=2)[0]
    torch.cuda.synchronize()
    guarded = np.isin(s.wall[box["fid"]], (0, 1, 2))
    want = np.where(guarded[..., None], vertex, box["colour"])
    assert guarded.sum() > 1000
    _same_bits(color, want, "out-of-range materials and textures")
    materials = [list(m) for m in s.materials]
    materials[1][0] = 3
    materials[2][0] = 2 ** 31 - 1
    twin = TS.Scene(**{**s.__dict__, "face_material": fm, "materials": materials})
    _same_bits(color, TS.render_rgbd_tex(twin, box["poses"], TS.CAMERA, far=FAR)[1], "the restatement's own guard")
    # the struct's size
    sim.tex.struct.struct_size = C.sizeof(_lib.NarutoSimTextures) - 8
    with pytest.raises(_lib.NarutoError, match="NarutoSimTextures"):
        sim.simulate_batch(box["poses"][:1])
    r = sim._raster("pinhole", 2)
    out = torch.empty(1, 30, 40, dtype=torch.float32, device=sim.device)
    pose = torch.from_numpy(box["poses"][:1]).to(sim.device)
    args = (C.byref(r.cam), len(sim.v), sim.v.data_ptr(), len(sim.f), sim.f.data_ptr(), sim.col.data_ptr(), int(sim.col_f32), 1, pose.data_ptr(), sim.threshold, 0,
            r.ws.data_ptr(), out.data_ptr(), None, None)
    assert _lib.load().naruto_render_rgbd_tex(*args, C.byref(sim.tex.struct), None) == _lib.ERR_INVALID
    assert _lib.load().naruto_render_rgbd_tex(*args, None, None) == _lib.ERR_INVALID
    sim.tex.struct.struct_size = C.sizeof(_lib.NarutoSimTextures)
    assert _lib.load().naruto_render_rgbd_tex(*args, C.byref(sim.tex.struct), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32).cpu(), torch.from_numpy(box["depth"][:1].copy().view(np.int32)))


def test_host_validation(gpu, box):
    from naruto_amd.mesh import Material
    s = box["scene"]

    def broken(**kw):
        m = _mesh(s)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    fm = s.face_material.copy()
    fm[0] = 5
    uv = s.uv.copy()
    uv[3, 1] = np.nan
    far_uv = s.uv.copy()
    far_uv[0, 0] = 1025.0
    for bad, what in ((broken(face_material=fm), "face material"), (broken(face_material=fm[:-1]), "per face"), (broken(uv=uv), "uv"), (broken(uv=far_uv), "uv"),
                      (broken(uv=s.uv[:-1]), "uv"), (broken(materials=[Material(3)] * 5), "texture 3"), (broken(materials=[Material(0, 1, 10497)] * 5), "wrap"),
                      (broken(materials=[Material(0, factor=(1.0, np.inf, 1.0, 1.0))] * 5), "factor"), (broken(textures=[np.zeros((2, 2, 3), dtype=np.uint8)] * 3), "texture 0")):
        with pytest.raises(ValueError, match=what):
            _sim(bad)
    # a mesh whose faces have no material goes through the untextured launches
    assert _sim(broken(face_material=np.full(len(s.faces), -1, dtype=np.int32))).tex is None


def test_a_run_from_a_glb(gpu, tmp_path):
    """A .glb written here -> MeshSimHIP by its path -> run_exploration for three steps at 40 x 30: the first frame is the restatement's
    render of the loaded scene, and it is not one colour."""
    import copy
    import helpers as H
    from naruto_amd.gltf import load_gltf
    from naruto_amd.planner import compute_camera_pose
    from naruto_amd.run import run_exploration
    from naruto_amd.simulator import MeshSimHIP
    from naruto_amd.slam import CoSLAMNarutoHIP
    room = [[0.0, 6.0], [0.0, 5.0], [0.0, 3.0]]
    path = GS.room_glb(tmp_path / "room.glb", room, TS.hashed_image(16, 16, 9))
    cfg = H.office_cfg(12, perturb=1.0)
    cfg["cam"].update(TS.CAMERA, depth_trunc=100.0, near=0, far=5)
    cfg["mapping"]["bound"] = copy.deepcopy(room)
    cfg["mapping"]["marching_cubes_bound"] = copy.deepcopy(room)
    cfg["mapping"].update(sample=128, min_pixels_cur=16, keyframe_every=5, map_every=5, iters=5, first_iters=10, n_pixels=0.5, filter_depth=True)
    cfg["tracking"] = {"disable": True}
    cfg["mesh"].update(vis=500, voxel_eval=0.1, voxel_final=0.1)
    traj = []
    for k in range(3):
        pos = np.array([1.2 + 0.3 * k, 1.0 + 0.2 * k, 1.2])
        p = np.eye(4, dtype=np.float32)
        p[:3, :3], p[:3, 3] = compute_camera_pose(pos, np.array([3.0, 2.5, 1.5])).astype(np.float32), pos
        traj.append(p)
    traj = torch.from_numpy(np.stack(traj))
    slam = CoSLAMNarutoHIP(cfg, voxel_size=0.1, active_ray=False, num_frames=3, seed=3, result_dir=str(tmp_path / "run"), device=gpu)
    cam = {k: getattr(slam, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}                # (the SLAM object's own sensor, as run.py hands it on)
    assert (cam["W"], cam["H"]) == (40, 30)
    sim = MeshSimHIP(path, cam, erp_hw=(16, 32), face_w=16, far=FAR, device=gpu)
    assert sim.tex is not None
    frames, simulate = [], sim.simulate
    sim.simulate = lambda *a, **kw: frames.append(simulate(*a, **kw)) or frames[-1]
    out = run_exploration(slam, sim, None, None, 3, traj=traj)
    assert len(frames) == 3 and len(out["poses"]) == 3 and len(out["mesh"].faces) > 0
    want_d, want_c, _ = TS.render_rgbd_tex(load_gltf(path), _np(traj[:1]), cam, far=FAR)
    _same_bits(frames[0][0], want_c[0], "first frame's colour")
    _same_bits(frames[0][1], want_d[0], "first frame's depth")
    assert len(np.unique(_np(frames[0][0]).reshape(-1, 3), axis=0)) > 100

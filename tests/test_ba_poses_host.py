"""Host side of the pose refinement inside global_BA (naruto_amd/ba_loop.py, naruto_bapose.hip), no GPU: the torch restatement of the
contract against fp64 central differences, the id-segmented sums + VJP-at-the-step against per-iteration autograd accumulation, the
kernels' own Adam through the host-only entry point, the ctypes mirror of the new struct, the entry points' argument checks, and the
oracle half of the GPU tests' schedules (tests/ba_pose_scene.py): the trajectory test's 5 % cap and the refinement schedule's recovery.
No call here passes validation with device pointers: nothing is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import ba_pose_scene as B
import helpers as H
from naruto_amd import tracking as TK


def _fp(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


# --------------------------------------------------------------------------------------------- the pose arithmetic
def test_batched_matrix_to_pose6_is_the_single_one():
    g = torch.Generator().manual_seed(3)
    mats = []
    for theta in (0.0, 1e-9, 1e-3, 0.4, 1.7, 3.0, 3.14159):
        axis = torch.randn(3, generator=g, dtype=torch.float64)
        m = torch.eye(4, dtype=torch.float64)
        m[:3, :3] = TK.axis_angle_to_matrix(axis / axis.norm() * theta)
        m[:3, 3] = torch.randn(3, generator=g, dtype=torch.float64)
        mats.append(m)
    mats = torch.stack(mats)
    got = TK.matrices_to_pose6(mats)
    for k, m in enumerate(mats):
        np.testing.assert_allclose(got[k, :3].numpy(), TK.matrix_to_axis_angle(m[:3, :3]).numpy(), rtol=0, atol=1e-15)
        assert torch.equal(got[k, 3:], m[:3, 3])
        np.testing.assert_allclose(TK.pose_matrix(got[k]).numpy(), m.numpy(), rtol=0, atol=1e-7 if k == 6 else 1e-12)


def test_pose_adam_is_torch_adam(built_lib):
    """naruto_debug_pose_adam runs pose_adam_step, the code of k_track_step and k_ba_pose_step: five steps against torch.optim.Adam in
    fp64 with lr_rot / lr_trans groups.  fp32 moments and updates: 1e-6 relative to the step size per step."""
    g = torch.Generator().manual_seed(9)
    p0 = torch.randn(6, generator=g, dtype=torch.float64)
    w = p0[:3].clone().requires_grad_(True)
    t = p0[3:].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [w], "lr": 2e-3}, {"params": [t], "lr": 5e-4}], betas=(0.9, 0.999), eps=1e-8)
    p = p0.numpy().astype(np.float32)
    m, v = np.zeros(6, np.float32), np.zeros(6, np.float32)
    for step in range(1, 6):
        grad = torch.randn(6, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=g))
        if step == 3:
            grad[1] = 0.0
        w.grad, t.grad = grad[:3].clone(), grad[3:].clone()
        opt.step()
        ga = grad.numpy().astype(np.float32)
        assert built_lib.naruto_debug_pose_adam(_fp(p), _fp(ga), _fp(m), _fp(v), step, 2e-3, 5e-4, 0.9, 0.999, 1e-8) == 0
        want = torch.cat([w, t]).detach().numpy()
        np.testing.assert_allclose(p, want, rtol=0, atol=step * 2e-3 * 1e-5 + 1e-7)
    assert built_lib.naruto_debug_pose_adam(_fp(p), _fp(ga), _fp(m), _fp(v), 0, 2e-3, 5e-4, 0.9, 0.999, 1e-8) < 0


def test_segmented_sums_and_vjp_at_the_step_equal_autograd_accumulation(built_lib):
    """Two iterations at constant poses: d_t[p] = sum d_rays_o, H[p] = sum d_rays_d (x) rays_d per pose id (naruto_debug_ba_pose_sums: the
    accumulation kernel's order and the pose step's gradient code), then ONE Rodrigues VJP with cotangent H R -- against omega.grad /
    t.grad accumulated by autograd over the same two iterations through rays_d = R(omega) d_cam, rays_o = t (fp64).  Rows pass through
    a permutation (src_rows) and the current frame's rays carry id -1."""
    P, n_stage, n = 5, 700, 500
    g = torch.Generator().manual_seed(4)
    W = (torch.randn(P, 3, generator=g, dtype=torch.float64) * 0.7).float().double().requires_grad_(True)
    T = torch.randn(P, 3, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    sums = [np.zeros(12, np.float64) for _ in range(P)]
    for it in range(2):
        ids = torch.randint(0, P - 1, (n_stage,), generator=g)
        ids[-60:] = -1
        src = torch.randperm(n_stage, generator=g)[:n]
        pid = torch.where(ids[src] < 0, torch.full_like(ids[src], P - 1), ids[src])
        d_cam = torch.randn(n, 3, generator=g, dtype=torch.float64)
        R = torch.stack([TK.axis_angle_to_matrix(W[p]) for p in range(P)])
        rays_d = torch.sum(d_cam[:, None, :] * R[pid], -1)
        rays_o = T[pid]
        a, b = torch.randn(n, 3, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64)
        rd32, ro32 = rays_d.detach().float().requires_grad_(True), rays_o.detach().float().requires_grad_(True)
        (torch.sin((rd32.double() * a).sum(1)) * torch.cos((ro32.double() * b).sum(1))).sum().backward()
        (torch.sin((rays_d * a).sum(1)) * torch.cos((rays_o * b).sum(1))).sum().backward()          # accumulates into W.grad / T.grad
        idn, srn = ids.numpy().astype(np.int64), src.numpy().astype(np.uint32)
        rdn, dro, drd = rd32.detach().numpy(), ro32.grad.numpy(), rd32.grad.numpy()
        for p in range(P):
            assert built_lib.naruto_debug_ba_pose_sums(n, idn.ctypes.data, n_stage, srn.ctypes.data, P, p, rdn.ctypes.data, dro.ctypes.data, drd.ctypes.data,
                                                       None, sums[p].ctypes.data, None) == 0
    got = np.zeros((P, 6), np.float32)
    zero = np.zeros(12, np.float64)
    for p in range(P):
        p6 = torch.cat([W[p], T[p]]).detach().numpy().astype(np.float32)
        assert built_lib.naruto_debug_ba_pose_sums(0, idn.ctypes.data, n_stage, None, P, p, rdn.ctypes.data, dro.ctypes.data, drd.ctypes.data, p6.ctypes.data,
                                                   sums[p].ctypes.data, got[p].ctypes.data) == 0
        np.testing.assert_array_equal(sums[p] + zero, sums[p])
    want = torch.cat([W.grad, T.grad], 1)
    H.grad_close(torch.from_numpy(got[:, :3]), want[:, :3], "d_omega from the segmented sums")
    H.grad_close(torch.from_numpy(got[:, 3:]), want[:, 3:], "d_t from the segmented sums")
    assert float(want[P - 1].abs().max()) > 0, "the id -1 rows belong to the last pose"
    assert built_lib.naruto_debug_ba_pose_sums(n, idn.ctypes.data, n_stage, None, P, P, rdn.ctypes.data, dro.ctypes.data, drd.ctypes.data, None, sums[0].ctypes.data, None) < 0


# --------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_mirror_of_the_struct(built_lib):
    """Every field written through ctypes is read back by the library (naruto_debug_ba_poses_fields): a shifted offset fails here."""
    from naruto_amd import _lib
    b = _lib.NarutoBAPoses()
    want = []
    for i, (name, typ) in enumerate(_lib.NarutoBAPoses._fields_):
        if typ is C.c_float:
            val = np.float32(0.125 + i)
            setattr(b, name, float(val))
            want.append(int(val.view(np.uint32)))
        elif typ is C.c_void_p:
            setattr(b, name, 0x100000 + 0x1000 * i)
            want.append(0x100000 + 0x1000 * i)
        else:
            setattr(b, name, 1000 + i)
            want.append(1000 + i)
    out = (C.c_uint64 * 25)()
    assert len(want) == 25 and built_lib.naruto_debug_ba_poses_fields(C.byref(b), out) == 0
    assert list(out) == want
    assert C.sizeof(_lib.NarutoBAPoses) % 8 == 0


def test_entry_points_validate_arguments(built_lib):
    from naruto_amd import _lib
    lib = built_lib
    assert lib.naruto_ba_poses_workspace(None, 2148, 43) >= 3 * 4 * 2148 * 43
    assert lib.naruto_ba_poses_workspace(None, 1 << 20, 1024) == 0
    assert lib.naruto_ba_poses_init(None, None) < 0 and b"NULL" in lib.naruto_last_error()
    assert lib.naruto_train_backward_poses(None, None, None, None, 0, None, None, None) < 0
    assert lib.naruto_debug_ba_poses_fields(None, None) < 0
    b = _lib.NarutoBAPoses()
    check = lambda: lib.naruto_debug_ba_poses_check(C.byref(b), 100)           # noqa: E731
    assert check() < 0 and b"max_poses" in lib.naruto_last_error()
    b.max_poses = 64
    assert check() < 0 and b"pose_accum_step" in lib.naruto_last_error()
    b.pose_accum_step = 5
    assert check() < 0 and b"NULL buffer" in lib.naruto_last_error()
    fake = [0x10000 + 0x100 * i for i in range(32)]                          # never dereferenced: nothing is launched
    for j, name in enumerate(("dyn", "poses", "pose_init", "pose6", "exp_avg", "exp_avg_sq", "accum", "state")):
        setattr(b, name, fake[j])
    b.lr_rot, b.lr_trans, b.beta1, b.beta2, b.eps = 1e-3, 1e-3, 0.9, 1.0, 1e-8
    assert check() < 0 and b"Adam" in lib.naruto_last_error()
    b.beta2 = 0.999
    b.trace_pose = fake[10]
    assert check() < 0 and b"trace" in lib.naruto_last_error()
    b.trace_grad, b.max_trace = fake[11], 2
    assert check() < 0 and b"ids" in lib.naruto_last_error()
    b.ids, b.d_rays_o, b.d_rays_d, b.workspace = fake[12:16]
    assert check() < 0 and b"n_ids" in lib.naruto_last_error()               # no ids at all
    b.n_ids = 50
    assert check() < 0 and b"50 pose ids for 100 rays" in lib.naruto_last_error()
    b.src_rows = fake[16]                                                    # with source rows the id list may be any length
    assert check() == 0
    b.src_rows, b.n_ids = None, 100
    assert check() == 0
    # the backward refuses the two-phase / data-parallel forms with poses, after the training step's own checks
    t, ps = _lib.NarutoTrainStep(), _lib.NarutoParams()
    assert lib.naruto_train_backward_poses(C.c_void_p(fake[20]), C.byref(ps), C.byref(t), None, 0, None, C.byref(b), None) < 0
    # the selection's new entry points check like the old ones
    assert lib.naruto_active_ray_select_keyed_rows(100, 10, 5, 2, None, None, None, None, None, None, None, None, None, None, None) < 0
    assert lib.naruto_active_ray_select_rows(100, 10, 5, 2, None, None, None, None, None, None, None, 10.0, None, None, None, None, None, None, None) < 0


def test_refusals_need_no_device():
    """FusedBA's refusals are decided from the configuration alone (the method reads no device state)."""
    from naruto_amd.ba_loop import FusedBA

    class _T:
        group = None
    ba = FusedBA.__new__(FusedBA)
    ba.config, ba.trainer, ba.active, ba.one_launch_prologue = B.cfg(), _T(), True, False
    ba._check_pose_refinement()
    ba.config["training"]["rot_rep"] = "quat"
    with pytest.raises(NotImplementedError, match="rot_rep"):
        ba._check_pose_refinement()
    ba.config = B.cfg(map_accum_step=2)
    with pytest.raises(NotImplementedError, match="map_accum_step"):
        ba._check_pose_refinement()
    ba.config = B.cfg(pose_accum_step=0)
    with pytest.raises(ValueError, match="pose_accum_step"):
        ba._check_pose_refinement()
    ba.config, ba.one_launch_prologue = B.cfg(), True
    with pytest.raises(NotImplementedError, match="one_launch_prologue"):
        ba._check_pose_refinement()
    ba.one_launch_prologue, ba.trainer.group = False, object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        ba._check_pose_refinement()
    ba._armed = ba._pose_ts = None               # (so that __del__ finds what it looks for)
    ba.use_graph = False


# --------------------------------------------------------------------------------------------- the oracle halves
@pytest.fixture(scope="module")
def world():
    c = B.cfg()
    sc = B.scene(c)
    frames = [B.frame(sc, k) for k in range(B.N_KF + 1)]
    true = B.true_poses(sc, B.N_KF + 1)
    return {"cfg": c, "frames": frames, "true": true, "poses": B.perturbed(true)}


def test_restatement_pose_gradient_against_central_differences(world):
    """The torch restatement itself, in fp64: autograd's d loss / d (omega, t) of one perturbed keyframe pose against central differences
    of the same loss (h = 1e-6: truncation ~h^2, round-off ~1e-16 |loss| / h ~ 1e-9; the field is piecewise smooth -- ReLU and
    trilinear cells -- and a sample within h of a kink contributes half its derivative jump, a 1e-4 fraction of the samples at the
    finest level: inside grad_close at 1e-3 of the largest component)."""
    c = world["cfg"]
    ora = B.load_oracle(c).double()
    for p in ora.parameters():
        p.requires_grad_(False)
    ora.train()
    rs = np.random.RandomState(1)
    d_cam, pid, rgb, dep = B.host_draw(rs, world["frames"], 96, 32)
    rand = torch.rand(128, 43, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    pose6 = TK.matrices_to_pose6(world["poses"])
    k = 2

    def loss_of(x):
        P6 = torch.cat([pose6[:k], x[None], pose6[k + 1:]])
        R = torch.stack([TK.axis_angle_to_matrix(P6[p, :3]) for p in range(P6.shape[0])])
        rays_d = torch.sum(d_cam.double()[:, None, :] * R[pid], -1)
        ret = ora.forward(P6[pid, 3:], rays_d, rgb.double(), dep.double().reshape(-1, 1), rand=rand)
        from oracle import spec_torch as S
        return S.total_loss(ret, c["training"])
    x = pose6[k].clone().requires_grad_(True)
    loss_of(x).backward()
    fd = torch.zeros(6, dtype=torch.float64)
    h = 1e-6
    with torch.no_grad():
        for j in range(6):
            e = torch.zeros(6, dtype=torch.float64)
            e[j] = h
            fd[j] = (loss_of(pose6[k] + e) - loss_of(pose6[k] - e)) / (2 * h)
    print("autograd", x.grad.tolist(), "central differences", fd.tolist())
    H.grad_close(x.grad[:3], fd[:3], "d_omega: autograd vs central differences", frac=1e-3)
    H.grad_close(x.grad[3:], fd[3:], "d_t: autograd vs central differences", frac=1e-3)


def _oracle_call(ora, c, frames, pose6, rs, g, n_global, n_cur, net_opts=None):
    o = B.OracleBA(ora, c, pose6, step_network=True, net_opts=net_opts)
    for i in range(int(c["mapping"]["iters"])):
        d_cam, pid, rgb, dep = B.host_draw(rs, frames, n_global, n_cur)
        o.iteration(i, d_cam, pid, rgb, dep, torch.rand(n_global + n_cur, 43, generator=g), rand6=torch.rand(6, generator=g))
    return o


def test_trajectory_cap_holds_on_the_oracle_alone(world):
    """test_gpu_ba_poses.py's trajectory test leaves out the stepped components whose reference gradient lies within 10 x the gradient
    bound of zero, at most 5 % of them: on the oracle loop alone (host draws, the oracle stepping its own network), for the committed
    perturbation, the cap holds with room."""
    c = world["cfg"]
    ora = B.load_oracle(c)
    o = _oracle_call(ora, c, world["frames"], TK.matrices_to_pose6(world["poses"]).float(), np.random.RandomState(6), torch.Generator().manual_seed(6), 384, 100)
    assert len(o.trace) == 2
    n_all = 2 * int(o.mask.sum()) * 6
    n_out = n_all - sum(int((B.trajectory_mask(gr) & o.mask[:, None]).sum()) for _, gr in o.trace)
    print(f"left out {n_out} of {n_all}")
    assert n_out <= 0.05 * n_all


def test_refinement_schedule_recovers_on_the_oracle_alone(world):
    """B.REFINE (found here, with the oracle alone): the oracle loop's mean rotation and translation errors drop below 0.7 x the start."""
    sch = B.REFINE
    c = B.cfg(lr_rot=sch["lr_rot"], lr_trans=sch["lr_trans"], pose_accum_step=sch["pose_accum_step"])
    ora = B.load_oracle(c)
    rs, g = np.random.RandomState(8), torch.Generator().manual_seed(8)
    poses, opts = world["poses"], None
    for k in range(sch["calls"]):
        o = _oracle_call(ora, c, world["frames"], TK.matrices_to_pose6(poses).float(), rs, g, 384, 100, net_opts=opts)
        opts = o.net_opts
        poses = B.pose6_matrices(o.pose6()).float()
    e0, e1 = B.errors(world["poses"], world["true"]), B.errors(poses, world["true"])
    print(f"oracle loop alone: start {e0[0]:.3f} deg {100 * e0[1]:.2f} cm -> {e1[0]:.3f} deg {100 * e1[1]:.2f} cm")
    assert e1[0] < 0.7 * e0[0] and e1[1] < 0.7 * e0[1]

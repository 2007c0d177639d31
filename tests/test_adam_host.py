"""The fp64 twin of torch.optim.Adam (tests/adam_spec.py) and its error bound, without a GPU: the twin IS torch.optim.Adam on float64 tensors
(1e-12), the kernels' formula in numpy float32 stays within 0.75 of the bound over the whole grid of hyper-parameter rows and steps (the
condition the reference implementation alone passes), every mutant -- a step that is wrong in one of the ways a fused optimiser goes wrong --
leaves the bound on at least half of the elements somewhere on the grid, and the host build of pose_adam_step (the tracking / BA poses'
step, fp64 bias corrections) matches the twin with the powf allowance removed."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_spec as A

N = 20000
GRID_ROWS = dict(A.ROWS, **A.EXTRA_ROWS)
LAG = 5                                            # what "lag ignored" forgets to subtract


def _neighbour(name):
    names = list(GRID_ROWS)
    return GRID_ROWS[names[(names.index(name) + 1) % len(names)]]


def _seed(name, t):
    return 1000 * (1 + list(GRID_ROWS).index(name)) + A.STEPS.index(t)


@pytest.fixture(scope="module")
def grid():
    """(row name, t) -> (inputs, twin): computed once, shared, never written."""
    out = {}
    for name, row in GRID_ROWS.items():
        for t in A.STEPS:
            x = A.make_inputs(N, t, _seed(name, t))
            out[name, t] = (x, A.adam_twin(*x, t=t, **A.row_kw(row)))
    return out


# ------------------------------------------------------------------------------------------------ the twin is torch.optim.Adam
def _torch_params(arrays):
    return [torch.from_numpy(a.astype(np.float64)).clone().requires_grad_(True) for a in arrays]


def test_twin_is_torch_adam_in_fp64():
    """Four steps with weight decay, two groups with their own lr / eps / wd, and a third parameter added after two steps (torch counts steps
    per parameter: it lags by two).  Betas are the widened fp32 values, as the twin takes them."""
    rs = np.random.RandomState(5)
    n = 257
    betas = (0.9, 0.999)
    wb = tuple(float(np.float32(b)) for b in betas)
    groups = [dict(lr=0.01, eps=1e-8, wd=1e-6), dict(lr=1e-3, eps=1e-15, wd=0.1), dict(lr=0.5, eps=1e-3, wd=0.0)]
    w32 = lambda x: float(np.float32(x))
    ps = _torch_params([rs.randn(n).astype(np.float32) for _ in groups])
    opt = torch.optim.Adam([dict(params=[ps[k]], lr=w32(g["lr"]), eps=w32(g["eps"]), weight_decay=w32(g["wd"])) for k, g in enumerate(groups[:2])],
                           betas=wb, foreach=False)
    state = [[p.detach().numpy().astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)] for p in ps]
    # the twin takes fp32 state: keep torch's state ON fp32 values by writing the rounded twin state back before each step
    born = [0, 0, 2]
    for step in range(1, 5):
        if step == 3:
            g = groups[2]
            opt.add_param_group(dict(params=[ps[2]], lr=w32(g["lr"]), eps=w32(g["eps"]), weight_decay=w32(g["wd"])))
        live = [k for k in range(3) if born[k] < step]
        grads = {k: (rs.randn(n) * 10.0 ** rs.uniform(-6, 2, n)).astype(np.float32) for k in live}
        for k in live:
            ps[k].grad = torch.from_numpy(grads[k].astype(np.float64))
        opt.step()
        for k in live:
            t = step - born[k]
            p, m, v = state[k]
            tw = A.adam_twin(p, grads[k], m, v, lr=groups[k]["lr"], betas=betas, eps=groups[k]["eps"], wd=groups[k]["wd"], t=t)
            st = opt.state[ps[k]]
            assert int(st["step"]) == t
            for got, want, what in ((ps[k].detach().numpy(), tw[0], "p"), (st["exp_avg"].numpy(), tw[1], "m"), (st["exp_avg_sq"].numpy(), tw[2], "v")):
                np.testing.assert_allclose(want, got, rtol=1e-12, atol=0, err_msg=f"step {step} tensor {k} {what}")
            # next step from fp32-representable state on both sides
            state[k] = [tw[0].astype(np.float32), tw[1].astype(np.float32), tw[2].astype(np.float32)]
            with torch.no_grad():
                ps[k].copy_(torch.from_numpy(state[k][0].astype(np.float64)))
                st["exp_avg"].copy_(torch.from_numpy(state[k][1].astype(np.float64)))
                st["exp_avg_sq"].copy_(torch.from_numpy(state[k][2].astype(np.float64)))


# ------------------------------------------------------------------------------------------------ the bound admits the reference ...
def test_fp32_emulation_stays_within_three_quarters_of_the_bound(grid):
    worst = np.zeros(3)
    for (name, t), (x, tw) in grid.items():
        got = A.emulate_fp32(*x, t=t, **A.row_kw(GRID_ROWS[name]))
        r = A.ratios(got, tw)
        print(f"row {name} t {t}: |error| / bound  p {r[0]:.3f}  m {r[1]:.3f}  v {r[2]:.3f}")
        worst = np.maximum(worst, r)
    print("worst  p %.3f  m %.3f  v %.3f" % tuple(worst))
    assert (worst <= 0.75).all(), worst


# ------------------------------------------------------------------------------------------------ ... and rejects the mutants
@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutant_leaves_the_bound(grid, mutant):
    caught = []
    for (name, t), (x, tw) in grid.items():
        nb = _neighbour(name)
        got = A.emulate_fp32(*x, t=t, mutant=mutant, lag=LAG, nb_lr=nb[2], nb_eps=nb[3], **A.row_kw(GRID_ROWS[name]))
        if got is None:
            continue
        share = A.share_over_bound(got[0], tw)
        if share >= 0.5:
            caught.append((name, t, round(share, 3)))
    print(f"{mutant}: caught (>= 50 % of elements over bound_p) at {caught}")
    assert caught, f"no (row, t) of the grid catches the mutant '{mutant}': a hole in the grid"


# ------------------------------------------------------------------------------------------------ form 7: pose_adam_step, host build
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.99)])
@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
def test_pose_adam_step_matches_the_twin(built_lib, betas, t):
    """naruto_debug_pose_adam = pose_adam_step, the code of k_track_step and k_ba_pose_step.  lr_rot steps components 0-2, lr_trans 3-5; the
    bias corrections are fp64 there, so the bound's powf allowance is dropped."""
    K = 256
    lr_rot, lr_trans, eps = 2e-3, 5e-4, 1e-8
    p, g, m, v = A.make_inputs(6 * K, t, 77 + t % 97)
    lr = np.tile(np.array([lr_rot] * 3 + [lr_trans] * 3, np.float32), K)
    tw = A.adam_twin(p, g, m, v, lr=lr, betas=betas, eps=eps, wd=0.0, t=t, fp64_bias=True)
    wrong = A.adam_twin(p, g, m, v, lr=lr[::-1].copy(), betas=betas, eps=eps, wd=0.0, t=t, fp64_bias=True)      # lr_rot and lr_trans exchanged
    gp, gm, gv = p.copy(), m.copy(), v.copy()
    g0 = g.copy()
    for k in range(K):
        s = slice(6 * k, 6 * k + 6)
        a, b, c, d = (np.ascontiguousarray(x[s]) for x in (gp, g, gm, gv))
        assert built_lib.naruto_debug_pose_adam(_fp(a), _fp(b), _fp(c), _fp(d), t, lr_rot, lr_trans, betas[0], betas[1], eps) == 0
        gp[s], gm[s], gv[s] = a, c, d
    assert np.array_equal(g, g0)
    r = A.assert_within((gp, gm, gv), tw, f"pose_adam_step betas {betas} t {t}")
    print(f"pose_adam_step betas {betas} t {t}: |error| / bound  p {r[0]:.3f}  m {r[1]:.3f}  v {r[2]:.3f}")
    assert A.share_over_bound(gp, wrong) >= 0.5, "the test cannot tell lr_rot from lr_trans"

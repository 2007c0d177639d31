"""k_adam (naruto_adam_step) and k_adam_multi (naruto_adam_multi, FusedAdam.step) at the C boundary against the fp64 twin of torch.optim.Adam
(tests/adam_spec.py): every case is ONE launch from prepared state, compared per element with the twin under its derived bound for the
parameter and both moments.  Every tensor is a slice of a larger buffer with 64 sentinel floats on each side; the sentinels -- and, without
NARUTO_ADAM_ZERO_GRAD, the gradients -- must come back bit for bit.  Covered: the hyper-parameter rows of the workload (the uncertainty grid's
lr = 1 / beta2 = 0.999 among them) at steps 1 .. 100000 from a host step, a device word and the ADVANCE ticket; the block-count edges and both
stride loops; 1, 2, 5 and 8 segments with per-segment lr / eps / wd / lag (each must ALSO leave the bound under its neighbour's settings, so
that no case passes vacuously); unaligned views; ZERO_GRAD; three ADVANCE launches in a row over ~2000 workgroups; entries that must not move;
gradients whose square underflows; the argument checks; and FusedAdam's multi-launch paths (two beta groups, more than eight tensors, an
external step word, a non-contiguous .grad with zero_grad)."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_spec as A
from naruto_amd import _lib

pytestmark = pytest.mark.gpu

PAD = 64
SENT = np.float32(-7.25e17)
K_ADAM, K_MULTI = "1 k_adam", "2 k_adam_multi"


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    A.dump_worst()


class Slab:
    """``a`` inside a larger device buffer: PAD sentinel floats on each side, the payload ``off`` elements past a 16-byte boundary."""

    def __init__(self, a, dev, off=0):
        n = a.size
        self.big = torch.full((PAD + 4 + n + PAD,), float(SENT), dtype=torch.float32, device=dev)
        self.lo, self.n = PAD + off, n
        self.t = self.big[self.lo:self.lo + n]
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        assert self.big.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * (off % 4)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy()

    def assert_sentinels(self, what):
        big = self.big.cpu().numpy()
        outside = np.concatenate([big[:self.lo], big[self.lo + self.n:]])
        assert (outside.view(np.uint32) == SENT.view(np.uint32)).all(), f"{what}: written outside its {self.n} elements"


class Seg:
    """One tensor's prepared state on the device, its settings, and the comparison with the twin."""

    def __init__(self, n, t_own, seed, dev, *, lr, eps, wd, lag=0, off=(0, 0, 0, 0), zero_frac=0.25, host=None):
        self.n, self.lr, self.eps, self.wd, self.lag = n, lr, eps, wd, lag
        self.host = host if host is not None else A.make_inputs(n, t_own, seed, zero_frac)
        self.p, self.g, self.m, self.v = (Slab(a, dev, o) for a, o in zip(self.host, off))

    def fill(self, sg):
        sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq = self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr
        sg.n, sg.lr, sg.eps, sg.weight_decay, sg.step_lag = self.n, self.lr, self.eps, self.wd, self.lag

    def got(self):
        return self.p.get(), self.m.get(), self.v.get()

    def twin(self, betas, t_global, other=None):
        s = other if other is not None else self
        return A.adam_twin(*self.host, lr=s.lr, betas=betas, eps=s.eps, wd=s.wd, t=t_global - s.lag)

    def check(self, betas, t_global, what, form, zeroed=False):
        """Within the bound of the twin run with this segment's own settings; sentinels and gradient intact.  Then the state the device
        holds becomes the prepared state of the next launch."""
        got = self.got()
        r = A.assert_within(got, self.twin(betas, t_global), what, form)
        for s, name in ((self.p, "p"), (self.g, "g"), (self.m, "m"), (self.v, "v")):
            s.assert_sentinels(f"{what} {name}")
        g = self.g.get()
        if zeroed:
            assert (g.view(np.uint32) == 0).all(), f"{what}: gradient not zeroed (+0) by ZERO_GRAD"
            self.g.t.copy_(torch.from_numpy(self.host[1]))           # hand the same gradient to the next launch
        else:
            assert np.array_equal(g.view(np.uint32), self.host[1].view(np.uint32)), f"{what}: the gradient was written"
        self.host = (got[0], self.host[1], got[1], got[2])
        return r


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _word(dev, *vals):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


def adam_step(lib, s, betas, step=0, step_dev=None):
    rc = lib.naruto_adam_step(s.p.ptr, s.g.ptr, s.m.ptr, s.v.ptr, s.n, s.lr, betas[0], betas[1], s.eps, s.wd, step,
                              None if step_dev is None else step_dev.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


def adam_multi(lib, segs, betas, step=0, step_dev=None, flags=0):
    arr = (_lib.NarutoAdamSeg * len(segs))()
    for sg, s in zip(arr, segs):
        s.fill(sg)
    rc = lib.naruto_adam_multi(arr, len(segs), betas[0], betas[1], step, None if step_dev is None else step_dev.data_ptr(), flags, _stream())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ rows x steps, five ways to say "step t"
WAYS = ("step host", "step step_dev", "multi host", "multi step_dev", "multi advance")


@pytest.mark.parametrize("row", list(A.ROWS))
@pytest.mark.parametrize("way", WAYS)
def test_rows_and_steps(gpu, built_lib, way, row):
    b1, b2, lr, eps, wd = A.ROWS[row]
    betas = (b1, b2)
    for t in A.STEPS:
        s = Seg(4097, t, 31 * t + ord(row), gpu, lr=lr, eps=eps, wd=wd)
        what = f"{way}, row {row}, t {t}"
        if way == "step host":
            assert adam_step(built_lib, s, betas, step=t) == 0
        elif way == "step step_dev":
            word = _word(gpu, t)
            assert adam_step(built_lib, s, betas, step_dev=word) == 0
            assert word.tolist() == [t]
        elif way == "multi host":
            assert adam_multi(built_lib, [s], betas, step=t) == 0
        elif way == "multi step_dev":
            word = _word(gpu, t, 0)
            assert adam_multi(built_lib, [s], betas, step_dev=word) == 0
            assert word.tolist() == [t, 0]
        else:
            word = _word(gpu, t - 1, 0)
            assert adam_multi(built_lib, [s], betas, step_dev=word, flags=_lib.ADAM_ADVANCE) == 0
            assert word.tolist() == [t, 0], f"{what}: the step word reads {word.tolist()}"
        s.check(betas, t, what, K_ADAM if way.startswith("step") else K_MULTI)


# ------------------------------------------------------------------------------------------------ launch edges
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048 * 256, 2048 * 256 + 1])
def test_k_adam_launch_edges(gpu, built_lib, n):
    """One block, the block boundary, 2048 blocks exactly, and one element into the grid-stride loop."""
    b1, b2, lr, eps, wd = A.ROWS["a"]
    for t, word in ((3, None), (10, _word(gpu, 10))):
        s = Seg(n, t, 500 + n % 1000 + t, gpu, lr=lr, eps=eps, wd=wd)
        assert adam_step(built_lib, s, (b1, b2), step=t if word is None else 0, step_dev=word) == 0
        s.check((b1, b2), t, f"k_adam n {n} t {t}", K_ADAM)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_k_adam_multi_launch_edges(gpu, built_lib, n):
    """One workgroup per 1024 elements: 1023 / 1024 / 1025 around the second workgroup, 2^20 + 1 one element into the stride loop (1024 workgroups)."""
    b1, b2, lr, eps, wd = A.ROWS["a"]
    s = Seg(n, 3, 600 + n % 1000, gpu, lr=lr, eps=eps, wd=wd)
    assert adam_multi(built_lib, [s], (b1, b2), step=3) == 0
    s.check((b1, b2), 3, f"k_adam_multi n {n}", K_MULTI)


# ------------------------------------------------------------------------------------------------ segments
SIZES = [1, 255, 1024, 1025, 7, 4096, 33, 1024 * 1024 + 1]
SEG_LR = [0.01, 0.02, 1.0, 2e-3, 0.05, 1e-3, 0.3, 0.004]
SEG_EPS = [1e-8, 1e-15, 1e-3, 1e-6, 1e-8, 1e-15, 1e-3, 1e-10]
SEG_WD = [1e-6, 0.0, 0.1, 0.0, 1e-2, 0.0, 0.0, 1e-6]
SEG_BETAS = (0.9, 0.999)              # beta2^1000 = 0.37: a step number that is off by one still shows at t = 1000


def _lags(t_global):
    return [0, 1, 5, 0, t_global - 1, 2, 0, 7]       # segment 4 is at ITS first step


def _segments(n_segs, t_global, dev, seed=0):
    lags = _lags(t_global)
    return [Seg(SIZES[k], t_global - lags[k], 900 + 17 * k + seed, dev, lr=SEG_LR[k], eps=SEG_EPS[k], wd=SEG_WD[k], lag=lags[k],
                zero_frac=0.25 if SIZES[k] >= 255 else 0.0) for k in range(n_segs)]


def _check_segments(segs, t_global, what, zeroed=False):
    for k, s in enumerate(segs):
        if len(segs) > 1:
            # not vacuous: under the NEXT segment's lr / eps / wd / lag this segment's result leaves the bound
            wrong = s.twin(SEG_BETAS, t_global, other=segs[(k + 1) % len(segs)])
            share = A.share_over_bound(s.p.get(), wrong)
            assert share >= 0.5, f"{what}: segment {k} cannot be told from its neighbour ({share:.2f} of the elements leave the bound)"
        s.check(SEG_BETAS, t_global, f"{what} segment {k} (n {s.n}, lag {s.lag})", K_MULTI, zeroed=zeroed)


@pytest.mark.parametrize("n_segs", [1, 2, 5, 8])
def test_segments_use_their_own_settings(gpu, built_lib, n_segs):
    T = 1000
    segs = _segments(n_segs, T, gpu)
    word = _word(gpu, T, 0)
    assert adam_multi(built_lib, segs, SEG_BETAS, step_dev=word) == 0
    assert word.tolist() == [T, 0]
    _check_segments(segs, T, f"{n_segs} segments")


def test_advance_over_many_workgroups(gpu, built_lib):
    """Three launches of the 8-segment case (2000-odd workgroups on one ticket) from {41, 0}: steps 42, 43, 44, each from the kernel's own
    previous output."""
    segs = _segments(8, 42, gpu, seed=5)
    word = _word(gpu, 41, 0)
    for T in (42, 43, 44):
        assert adam_multi(built_lib, segs, SEG_BETAS, step_dev=word, flags=_lib.ADAM_ADVANCE) == 0
        assert word.tolist() == [T, 0], word.tolist()
        _check_segments(segs, T, f"advance to {T}")


def test_zero_grad(gpu, built_lib):
    """With the flag every consumed gradient is +0 afterwards and nothing else is touched (Seg.check: sentinels, p / m / v on the twin);
    without it the gradients come back bit for bit."""
    for flags in (_lib.ADAM_ZERO_GRAD, _lib.ADAM_ZERO_GRAD | _lib.ADAM_ADVANCE, 0):
        segs = _segments(5, 1000, gpu, seed=flags)
        word = _word(gpu, 1000 - (flags & 1), 0)
        assert adam_multi(built_lib, segs, SEG_BETAS, step_dev=word, flags=flags) == 0
        assert word.tolist() == [1000, 0]
        _check_segments(segs, 1000, f"flags {flags}", zeroed=bool(flags & _lib.ADAM_ZERO_GRAD))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_unaligned_views(gpu, built_lib, off):
    """Parameter, gradient and moments 1, 2 or 3 elements past a 16-byte boundary (MappingTrainer's table_shard slice is such a view),
    all four alike and each at its own offset."""
    b1, b2, lr, eps, wd = A.ROWS["a"]
    for offs in ((off,) * 4, (off, (off + 1) % 4, (off + 2) % 4, (off + 3) % 4)):
        for n in (4097, 1024 * 3 + 1):
            s = Seg(n, 3, 70 + off, gpu, lr=lr, eps=eps, wd=wd, off=offs)
            assert adam_step(built_lib, s, (b1, b2), step=3) == 0
            s.check((b1, b2), 3, f"k_adam offsets {offs} n {n}", K_ADAM)
            s = Seg(n, 3, 80 + off, gpu, lr=lr, eps=eps, wd=wd, off=offs)
            s2 = Seg(n + 2, 3, 90 + off, gpu, lr=2 * lr, eps=eps, wd=0.0, off=offs[::-1])
            assert adam_multi(built_lib, [s, s2], (b1, b2), step=3, flags=_lib.ADAM_ZERO_GRAD) == 0
            s.check((b1, b2), 3, f"k_adam_multi offsets {offs} n {n}", K_MULTI, zeroed=True)
            s2.check((b1, b2), 3, f"k_adam_multi offsets {offs[::-1]} n {n + 2}", K_MULTI, zeroed=True)


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("row", ["b", "c"])
def test_untouched_entries_do_not_move(gpu, built_lib, row):
    """g = m = v = 0 without weight decay: the parameter keeps its bits and the moments stay +0 (a table entry no ray ever reached)."""
    b1, b2, lr, eps, wd = A.ROWS[row]
    assert wd == 0.0
    n = 4097
    p = A.make_inputs(n, 1, 11)[0]
    z = np.zeros(n, np.float32)
    for t in (1, 3, 1000):
        for form in (K_ADAM, K_MULTI):
            s = Seg(n, t, 0, gpu, lr=lr, eps=eps, wd=wd, host=(p, z, z, z))
            if form == K_ADAM:
                assert adam_step(built_lib, s, (b1, b2), step=t) == 0
            else:
                assert adam_multi(built_lib, [s], (b1, b2), step=t) == 0
            gp, gm, gv = s.got()
            assert np.array_equal(gp.view(np.uint32), p.view(np.uint32)), f"{form} row {row} t {t}: an untouched parameter moved"
            assert (gm.view(np.uint32) == 0).all() and (gv.view(np.uint32) == 0).all(), f"{form} row {row} t {t}: moments of an untouched entry are not +0"


@pytest.mark.parametrize("t", [1, 10])
def test_tiny_gradients_stay_finite_and_small(gpu, built_lib, t):
    """|g| in 10^U(-30, -20): g^2 underflows, the bound (relative in v) does not apply.  Everything stays finite and the parameter moves by
    no more than S |m1| / eps."""
    b1, b2, lr, eps, wd = A.ROWS["b"]
    rs = np.random.RandomState(40 + t)
    n = 4097
    mag = 10.0 ** rs.uniform(-30, -20, n)
    g = (rs.randn(n) * mag).astype(np.float32)
    p = (rs.randn(n) * 10.0 ** rs.uniform(-6, 0, n)).astype(np.float32)
    m = np.zeros(n, np.float32) if t == 1 else (0.3 * rs.randn(n) * mag).astype(np.float32)
    v = np.zeros(n, np.float32) if t == 1 else ((rs.rand(n) + 0.05) * mag * mag).astype(np.float32)
    tw = A.adam_twin(p, g, m, v, lr=lr, betas=(b1, b2), eps=eps, wd=wd, t=t)
    S = float(np.float32(lr)) / (1.0 - float(np.float32(b1)) ** t)
    cap = S * np.abs(tw[1]) / float(np.float32(eps)) * (1.0 + 1e-3) + np.spacing(np.abs(p)).astype(np.float64)
    for form in (K_ADAM, K_MULTI):
        s = Seg(n, t, 0, gpu, lr=lr, eps=eps, wd=wd, host=(p, g, m, v))
        if form == K_ADAM:
            assert adam_step(built_lib, s, (b1, b2), step=t) == 0
        else:
            assert adam_multi(built_lib, [s], (b1, b2), step=t) == 0
        for a, name in zip(s.got(), "pmv"):
            assert np.isfinite(a).all(), f"{form} t {t}: {name} not finite"
        moved = np.abs(s.got()[0].astype(np.float64) - p.astype(np.float64))
        assert (moved <= cap).all(), f"{form} t {t}: moved {moved.max():.3e}, worst excess {np.max(moved - cap):.3e}"


def test_argument_checks(gpu, built_lib):
    lib = built_lib
    b1, b2, lr, eps, wd = A.ROWS["a"]
    s = Seg(300, 3, 1, gpu, lr=lr, eps=eps, wd=wd)
    before = [x.big.clone() for x in (s.p, s.g, s.m, s.v)]
    arr9 = (_lib.NarutoAdamSeg * 9)()
    for sg in arr9:
        s.fill(sg)
    word = _word(gpu, 3, 0)
    st = _stream()
    assert lib.naruto_adam_multi(arr9, 0, b1, b2, 3, None, 0, st) < 0
    assert lib.naruto_adam_multi(arr9, 9, b1, b2, 3, None, 0, st) < 0
    assert lib.naruto_adam_multi(None, 1, b1, b2, 3, None, 0, st) < 0
    assert lib.naruto_adam_multi(arr9, 1, b1, b2, 3, None, _lib.ADAM_ADVANCE, st) < 0, "ADVANCE without step_dev"
    assert lib.naruto_adam_multi(arr9, 1, b1, b2, 0, None, 0, st) < 0, "step 0 without step_dev"
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        bad = (_lib.NarutoAdamSeg * 2)()
        s.fill(bad[0])
        s.fill(bad[1])
        setattr(bad[1], field, None)
        assert lib.naruto_adam_multi(bad, 2, b1, b2, 3, word.data_ptr(), 0, st) < 0, f"NULL {field} in a segment"
    ptrs = [s.p.ptr, s.g.ptr, s.m.ptr, s.v.ptr]
    for k in range(4):
        a = list(ptrs)
        a[k] = None
        assert lib.naruto_adam_step(*a, s.n, lr, b1, b2, eps, wd, 3, None, st) < 0
    assert lib.naruto_adam_step(*ptrs, s.n, lr, b1, b2, eps, wd, 0, None, st) < 0, "step 0 without step_dev"
    assert lib.naruto_adam_step(*ptrs, 0, lr, b1, b2, eps, wd, 3, None, st) == 0, "n = 0 is not an error"
    torch.cuda.synchronize()
    for x, b in zip((s.p, s.g, s.m, s.v), before):
        assert torch.equal(x.big, b), "a refused or empty call wrote something"
    assert word.tolist() == [3, 0]


# ------------------------------------------------------------------------------------------------ FusedAdam's launch paths
def _fused(groups, dev, seed, **kw):
    """FusedAdam over one parameter per group -> (optimiser, parameters)."""
    from naruto_amd.trainer import FusedAdam
    ps = []
    for k, g in enumerate(groups):
        p0 = A.make_inputs(int(np.prod(g["shape"])), 2, seed + k)[0]
        ps.append(torch.nn.Parameter(torch.from_numpy(p0).reshape(g["shape"]).to(dev)))
    opt = FusedAdam([dict(params=[p], **{k: v for k, v in g.items() if k != "shape"}) for p, g in zip(ps, groups)], **kw)
    return opt, ps


def _fused_steps(opt, ps, steps, what, make_grad=None, before_step=None, t_of=lambda k: k, **step_kw):
    """``steps`` calls of opt.step(), each compared with the twin fed the optimiser's own previous state."""
    for k in range(1, steps + 1):
        if before_step is not None:
            before_step(k)
        snap = []
        for i, p in enumerate(ps):
            g = A.make_inputs(p.numel(), 2, 1000 * k + i)[1]
            p.grad = torch.from_numpy(g).reshape(p.shape).to(p.device) if make_grad is None else make_grad(p, g)
            m, v = opt.moments(p)
            snap.append((p.detach().cpu().numpy().ravel(), g, m.cpu().numpy().ravel(), v.cpu().numpy().ravel()))
        opt.step(**step_kw)
        torch.cuda.synchronize()
        for i, (p, gp) in enumerate((p, gp) for gp in opt.param_groups for p in gp["params"]):
            m, v = opt.moments(p)
            tw = A.adam_twin(*snap[i], lr=gp["lr"], betas=gp["betas"], eps=gp["eps"], wd=gp["weight_decay"], t=t_of(k))
            A.assert_within((p.detach().cpu().numpy().ravel(), m.cpu().numpy().ravel(), v.cpu().numpy().ravel()), tw,
                            f"{what}: step {k} tensor {i}", K_MULTI)
            yield k, i, p, snap[i], gp


def test_fused_adam_two_beta_groups(gpu):
    """Two beta groups: two launches behind one step_dev[:1] += 1.  After k steps the word reads {k, 0}."""
    groups = [dict(shape=(1025,), lr=0.01, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-6),
              dict(shape=(33, 7), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
              dict(shape=(300,), lr=0.02, betas=(0.9, 0.99), eps=1e-15, weight_decay=0.0)]
    opt, ps = _fused(groups, gpu, 10)
    seen = 0
    for k, i, p, snap, gp in _fused_steps(opt, ps, 3, "two beta groups"):
        assert opt.step_dev.tolist() == [k, 0]
        seen += 1
    assert seen == 9


def test_fused_adam_eleven_tensors(gpu):
    """Eleven tensors in one beta group: two launches, 8 + 3.  The ninth tensor is segment 0 of the second launch and must run with ITS
    settings, not with those of the first launch's segment 0."""
    groups = [dict(shape=(40 + 97 * k,), lr=0.01 * (k + 1), eps=[1e-8, 1e-15, 1e-3][k % 3], weight_decay=[0.0, 1e-6, 0.1][k % 3]) for k in range(11)]
    opt, ps = _fused(groups, gpu, 30, betas=(0.9, 0.999))
    g0 = opt.param_groups[0]
    for k, i, p, snap, gp in _fused_steps(opt, ps, 3, "eleven tensors"):
        assert opt.step_dev.tolist() == [k, 0]
        if i == 8:
            wrong = A.adam_twin(*snap, lr=g0["lr"], betas=g0["betas"], eps=g0["eps"], wd=g0["weight_decay"], t=k)
            assert A.share_over_bound(p.detach().cpu().numpy().ravel(), wrong) >= 0.5, "the ninth tensor cannot be told from the first"


def test_fused_adam_external_step_word(gpu):
    """external_step: the step number is whatever the caller's word holds (500, 501, ...); step_dev stays {0, 0}."""
    groups = [dict(shape=(1025,), lr=1.0, eps=1e-8, weight_decay=0.0), dict(shape=(77,), lr=0.01, eps=1e-8, weight_decay=1e-6)]
    opt, ps = _fused(groups, gpu, 50, betas=(0.9, 0.999))
    word = _word(gpu, 0)
    opt.external_step = word

    def before(k):
        word.fill_(499 + k)

    for k, i, p, snap, gp in _fused_steps(opt, ps, 3, "external step word", before_step=before, t_of=lambda k: 499 + k):
        assert opt.step_dev.tolist() == [0, 0] and word.tolist() == [499 + k]


def test_fused_adam_noncontiguous_grad_with_zero_grad(gpu):
    """A .grad that is a transposed view: the kernel steps on (and zeroes) a contiguous copy; step(zero_grad=True) promises zeroed
    gradients, so the caller's own tensor must read zero afterwards too."""
    groups = [dict(shape=(33, 7), lr=0.01, eps=1e-8, weight_decay=1e-6), dict(shape=(129,), lr=0.02, eps=1e-15, weight_decay=0.0)]
    opt, ps = _fused(groups, gpu, 70, betas=(0.9, 0.99))
    bases = {}

    def make_grad(p, g):
        if p.dim() == 2:
            bases[0] = torch.from_numpy(g).reshape(p.shape).t().contiguous().to(p.device)        # [7, 33] storage
            view = bases[0].t()
            assert not view.is_contiguous() and view.shape == p.shape
            return view
        return torch.from_numpy(g).to(p.device)

    for k, i, p, snap, gp in _fused_steps(opt, ps, 3, "non-contiguous grad", make_grad=make_grad, zero_grad=True):
        assert float(p.grad.abs().max()) == 0.0, f"step {k} tensor {i}: zero_grad=True left the caller's .grad non-zero"
        if p.dim() == 2:
            assert p.grad.data_ptr() == bases[0].data_ptr() and float(bases[0].abs().max()) == 0.0

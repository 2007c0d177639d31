"""torch.optim.Adam (amsgrad off, L2 weight decay) restated once in fp64, with a derived per-element error bound for an fp32 implementation of
the same step -- the reference every hand-written copy of the step in this repository is compared with, ONE step at a time from prepared
state, so that nothing accumulates and no tolerance is guessed.

adam_twin     the step in fp64 on fp32 inputs.  Hyper-parameters enter as the fp32 values the C ABI receives (naruto_adam_multi(float beta1,
              ...)), widened to double.  Returns (p1, m1, v1, bound_p, bound_m, bound_v).
emulate_fp32  the kernels' formula in numpy float32 (k_adam / k_adam_multi / adam_apply): what the bound has to admit.
MUTANTS       wrong steps the bound has to reject: off-by-one step, lag ignored, a neighbour segment's settings, ...

The bound is a first-order propagation of fp32 rounding, U = 2^-24 per operation:
    g' = g + wd p              dg      = 2U (|g| + |wd p|)                                   (0 without weight decay)
    m1 = m + (g' - m)(1 - b1)  bound_m = 3U (|g'| + |m|) + dg
    v1 = b2 v + (1 - b2) g'^2  bound_v = 4U v1 + (1 - b2)(2 |g'| dg + dg^2)
    D  = sqrt(v1)/c2 + eps     dD      = bound_v / (2 sqrt(v1) c2) + 2U D                    (v1 == 0: sqrt(bound_v)/c2 + 2U D)
    u  = S m1 / D              bound_p = S bound_m / D + |u| (dD/D + U (6 + 2 b1^t/(1-b1^t) + b2^t/(1-b2^t))) + 2U |p1|
with S = lr/(1 - b1^t), c2 = sqrt(1 - b2^t).  The last bracket allows 2 ulp on each powf(b, t) (HIP's documented accuracy; halved for b2 by
the square root); an implementation that computes the bias corrections in fp64 and rounds once (pose_adam_step) is checked without them
(``fp64_bias=True``)."""
import numpy as np

U = 2.0 ** -24

# (b1, b2, lr, eps, wd)
ROWS = {
    "a": (0.9, 0.99, 0.01, 1e-8, 1e-6),       # decoder
    "b": (0.9, 0.99, 0.01, 1e-15, 0.0),       # table
    "c": (0.9, 0.999, 1.0, 1e-8, 0.0),        # uncertainty grid
    "d": (0.9, 0.999, 2e-3, 1e-8, 0.0),
    "e": (0.0, 0.0, 1e-3, 1e-8, 0.0),
}
# the host grid's extra row: a large eps and a large weight decay (what catches "wd dropped" and "neighbour's eps" on most elements)
EXTRA_ROWS = {"f": (0.5, 0.9, 0.1, 1e-3, 0.1)}
STEPS = (1, 2, 3, 10, 1000, 100000)


def row_kw(row):
    b1, b2, lr, eps, wd = row
    return dict(lr=lr, betas=(b1, b2), eps=eps, wd=wd)


def _w(x):
    """A hyper-parameter as the C ABI receives it: rounded to fp32, widened to double (scalar or per-element array)."""
    return np.asarray(x, np.float32).astype(np.float64)


def adam_twin(p, g, m, v, *, lr, betas, eps, wd, t, fp64_bias=False):
    """One step of torch.optim.Adam in fp64.  ``t``: 1-based step with the lag already subtracted.  -> (p1, m1, v1, bound_p, bound_m, bound_v)."""
    assert t >= 1
    p, g, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, g, m, v))
    b1, b2, lr, eps, wd = _w(betas[0]), _w(betas[1]), _w(lr), _w(eps), _w(wd)
    t = float(t)
    g2 = g + wd * p
    m1 = m + (g2 - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * g2 * g2
    b1t, b2t = b1 ** t, b2 ** t
    S = lr / (1.0 - b1t)
    c2 = np.sqrt(1.0 - b2t)
    D = np.sqrt(v1) / c2 + eps
    u = S * m1 / D
    p1 = p - u
    dg = 2.0 * U * (np.abs(g) + np.abs(wd * p)) if np.any(wd != 0.0) else np.zeros_like(g)
    bound_m = 3.0 * U * (np.abs(g2) + np.abs(m)) + dg
    bound_v = 4.0 * U * v1 + (1.0 - b2) * (2.0 * np.abs(g2) * dg + dg * dg)
    dD = np.where(v1 > 0.0, bound_v / (2.0 * np.sqrt(np.where(v1 > 0.0, v1, 1.0)) * c2), np.sqrt(bound_v) / c2) + 2.0 * U * D
    powers = 0.0 if fp64_bias else 2.0 * b1t / (1.0 - b1t) + b2t / (1.0 - b2t)
    bound_p = np.abs(S) * bound_m / D + np.abs(u) * (dD / D + U * (6.0 + powers)) + 2.0 * U * np.abs(p1)
    return p1, m1, v1, bound_p, bound_m, bound_v


MUTANTS = ("t+1", "t-1", "lag ignored", "wd dropped", "eps inside sqrt", "bc2 not rooted", "betas swapped", "lr not over bc1",
           "neighbour's eps", "neighbour's lr")


def emulate_fp32(p, g, m, v, *, lr, betas, eps, wd, t, mutant=None, lag=0, nb_eps=None, nb_lr=None):
    """The kernels' formula in numpy float32 -> (p1, m1, v1) as float32.  ``mutant``: one of MUTANTS, a deliberately wrong step
    (``lag``: what "lag ignored" adds back; ``nb_eps`` / ``nb_lr``: the neighbour segment's settings).  None where the mutant does not apply."""
    f = np.float32
    if mutant == "t+1":
        t = t + 1
    elif mutant == "t-1":
        if t <= 1:
            return None
        t = t - 1
    elif mutant == "lag ignored":
        if lag == 0:
            return None
        t = t + lag
    elif mutant == "wd dropped":
        if wd == 0:
            return None
        wd = 0.0
    elif mutant == "neighbour's eps":
        eps = nb_eps
    elif mutant == "neighbour's lr":
        lr = nb_lr
    elif mutant == "betas swapped":
        betas = (betas[1], betas[0])
    else:
        assert mutant in (None, "eps inside sqrt", "bc2 not rooted", "lr not over bc1"), mutant
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    b1, b2, lr, eps, wd = f(betas[0]), f(betas[1]), f(lr), f(eps), f(wd)
    with np.errstate(all="ignore"):
        gk = g + wd * p if wd != 0 else g
        mk = m + (gk - m) * (f(1) - b1)
        vk = b2 * v + (f(1) - b2) * gk * gk
        bc1 = f(1) - np.power(b1, f(t))
        bc2 = f(1) - np.power(b2, f(t))
        bc2s = bc2 if mutant == "bc2 not rooted" else np.sqrt(bc2)
        step_size = lr if mutant == "lr not over bc1" else lr / bc1
        denom = np.sqrt(vk + eps) / bc2s if mutant == "eps inside sqrt" else np.sqrt(vk) / bc2s + eps
        pk = p - step_size * (mk / denom)
    return pk.astype(f), mk.astype(f), vk.astype(f)


def make_inputs(n, t, seed, zero_frac=0.25):
    """(p, g, m, v) fp32: g = randn 10^U(-12,3) with ``zero_frac`` exact zeros and |g| >= 1e-12 otherwise (v stays a normal fp32 number: the
    bound is relative in v); p = randn 10^U(-6,0), so that the update, not ulp(p), dominates; moments zero at t = 1, else m = 0.3 randn mag,
    v = (U(0,1) + 0.05) mag^2 with 10 % of the entries zero in both."""
    rs = np.random.RandomState(seed)
    f = np.float32
    mag = 10.0 ** rs.uniform(-12, 3, n)
    g = rs.randn(n) * mag
    g = np.where(np.abs(g) < 1e-12, np.where(g < 0, -1e-12, 1e-12), g).astype(f)
    g[rs.rand(n) < zero_frac] = 0
    p = (rs.randn(n) * 10.0 ** rs.uniform(-6, 0, n)).astype(f)
    if t == 1:
        m, v = np.zeros(n, f), np.zeros(n, f)
    else:
        m = (rs.randn(n) * mag * 0.3).astype(f)
        v = ((rs.rand(n) + 0.05) * mag * mag).astype(f)
        z = rs.rand(n) < 0.1
        m[z] = 0
        v[z] = 0
    return p, g, m, v


TINY = 2.0 ** -126            # smallest normal fp32 number


def bound_applies(p, g, m, v, *, betas, wd, **_):
    """Where the bound's premise holds for gradients the test did not draw itself: every product of the step is zero or a normal fp32 number
    (the bound is relative in v; a gradient whose square underflows rounds absolutely, at 2^-149).  make_inputs keeps |g| >= 1e-12 for this."""
    p, g, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, g, m, v))
    b1, b2, wd = _w(betas[0]), _w(betas[1]), _w(wd)
    g2 = g + wd * p
    ok = lambda x: (x == 0.0) | (np.abs(x) >= TINY)
    return ok((1.0 - b2) * g2 * g2) & ok(b2 * v) & ok((1.0 - b1) * (g2 - m))


def ratios(got, twin, mask=None):
    """max |got - twin| / bound for (p, m, v) (over ``mask``); an entry whose bound is 0 must be exact (ratio 0, else inf)."""
    out = []
    for k in range(3):
        err = np.abs(np.asarray(got[k], np.float64) - twin[k])
        b = twin[3 + k]
        if mask is not None:
            err, b = err[mask], b[mask]
        with np.errstate(all="ignore"):
            r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
        out.append(float(np.max(r)) if r.size else 0.0)
    return tuple(out)


def assert_within(got, twin, what, form=None, mask=None):
    """|got - twin| <= bound per element (of ``mask``) for p, m and v.  ``form``: the name under which the worst ratio is kept (record / dump_worst)."""
    r = ratios(got, twin, mask)
    if form is not None:
        record(form, r)
    for name, x in zip("pmv", r):
        assert np.isfinite(np.asarray(got["pmv".index(name)], np.float64)).all(), f"{what}: {name} not finite"
        assert x <= 1.0, f"{what}: {name} leaves the bound, worst |error| / bound = {x:.3f} (p, m, v: {r})"
    return r


WORST = {}                 # form -> worst |error| / bound seen for (p, m, v) by the tests of this session


def record(form, r):
    old = WORST.get(form, (0.0, 0.0, 0.0))
    WORST[form] = tuple(max(a, b) for a, b in zip(old, r))


def dump_worst():
    """With NARUTO_ADAM_BOUNDS_OUT set: merge this session's worst ratios into that JSON file (how profiles/adam_bounds.json was recorded)."""
    import json
    import os
    path = os.environ.get("NARUTO_ADAM_BOUNDS_OUT")
    if not path or not WORST:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    for form, r in WORST.items():
        old = data.get(form, {"p": 0.0, "m": 0.0, "v": 0.0})
        data[form] = {k: round(max(old[k], x), 4) for k, x in zip("pmv", r)}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)


def share_over_bound(got_p, twin):
    """Share of elements whose parameter lies outside bound_p."""
    return float(np.mean(np.abs(np.asarray(got_p, np.float64) - twin[0]) > twin[3]))

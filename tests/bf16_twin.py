"""CPU side of the bf16 MLP backward's tests (test_gpu_bwd_bf16.py, test_bwd_bf16_host.py): the torch restatement of k_query_bwd_bf by both
routes, a second evaluation of the same arithmetic in another accumulation order, the filter that keeps ReLU masks away from accumulation
noise, the fixed point sets and the two tolerances.

The restatement is oracle/spec_bf16.py's: every matrix product with bf16-rounded operands, ReLU masks from the bf16 forward.  It accumulates in
fp64; the second evaluation (``rev=True``) accumulates the same products in fp32, last K entry first -- what two correct implementations may
differ by.  Routes: "raw" puts a cotangent [M,5] on raw = query_color_sdf; "geo" puts cotangents on (sdf, uncertainty) [M,2] and on the 15 geo
features, as query_sdf(return_geo=True, return_uncert=True) does -- the colour net is unused there and its weights get no gradient."""
import numpy as np
import torch

from oracle import spec_bf16 as BF
from oracle import spec_torch as S

NAMES = ("sdf_w0", "sdf_w1", "col_w0", "col_w1", "uncert_grid", "table")
ROUTES = ("raw", "geo")
FAR = (-0.95, 1.95)                  # outside the closed-form OneBlob's range (-0.93, 1.93): such a point sends its 64-entry step to the dense form
N_INSIDE, N_OUTSIDE, N_FAR = 64, 24, 8
N_ANCHOR_IN_RANGE = N_INSIDE + N_OUTSIDE
N_POOL_IN_RANGE = 577                # the anchors first; the composition cases take prefixes (257 for all but the several-steps-per-wave case)


def leaves(ora):
    return {"sdf_w0": ora.sdf_w0, "sdf_w1": ora.sdf_w1, "col_w0": ora.col_w0, "col_w1": ora.col_w1, "uncert_grid": ora.uncert_grid, "table": ora.table}


# ---------------------------------------------------------------------------------------------- the second evaluation
def _dot_rev(a, b):
    """sum_k a[:, k] b[:, k] -> [rows of a, rows of b], accumulated in fp32 from the last k to the first."""
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k in range(a.shape[1] - 1, -1, -1):
        acc = acc + a[:, k, None] * b[None, :, k]
    return acc


class RevLinear(torch.autograd.Function):
    """BF.BfLinear with every sum accumulated in fp32, in reversed order (products of two bf16 numbers are exact in fp32)."""

    @staticmethod
    def forward(ctx, x, W, exact):
        ctx.save_for_backward(x, W)
        ctx.exact = exact
        return _dot_rev(x, W) if exact else _dot_rev(BF.bf(x), BF.bf(W))

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        dx = _dot_rev(g, W.T.contiguous()) if ctx.exact else _dot_rev(BF.bf(g), BF.bf(W).T.contiguous())
        dW = _dot_rev(BF.bf(g).T.contiguous(), BF.bf(x).T.contiguous())
        return dx, dW, None


def _query_rev(ora, x):
    """BF.query_color_sdf_bf16 on RevLinear."""
    feats, pos = S.hash_encode(x, ora.table, ora.meta), S.oneblob_encode(x, ora.n_bins)
    h = RevLinear.apply(torch.cat([feats, pos], -1), ora.sdf_w0, False)
    out = RevLinear.apply(torch.relu(h), ora.sdf_w1, False)
    c = RevLinear.apply(torch.cat([pos, out[:, 1:]], -1), ora.col_w0, False)
    rgb = RevLinear.apply(torch.relu(c), ora.col_w1, True)
    unc = S.sample_uncert_grid_ref(ora.uncert_grid, x)[:, None]
    return torch.cat([rgb, out[:, :1], unc], -1), out


# ---------------------------------------------------------------------------------------------- the restatement, both routes
def restate(ora, x, cot, route, rev=False):
    """Forward outputs and the six gradients of the restatement at the points x [M,3] (numpy float32).  cot: {"raw": [M,5]} or {"su": [M,2],
    "geo": [M,15]}.  -> ({"raw"} or {"su", "geo"}, {name: gradient or None})."""
    for p in leaves(ora).values():
        p.grad = None
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    raw, out = (_query_rev if rev else BF.query_color_sdf_bf16)(ora, xt)
    if route == "raw":
        fwd = {"raw": raw}
        loss = (raw * torch.from_numpy(cot["raw"])).sum()
    else:
        fwd = {"su": torch.stack([out[:, 0], raw[:, 4]], -1), "geo": out[:, 1:]}
        loss = (fwd["su"] * torch.from_numpy(cot["su"])).sum() + (fwd["geo"] * torch.from_numpy(cot["geo"])).sum()
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in leaves(ora).items()}
    if route == "geo":               # (autograd hands the unused colour net the zeros that flow back through raw's concatenation)
        for k in ("col_w0", "col_w1"):
            assert grads[k] is None or float(grads[k].abs().max()) == 0.0
            grads[k] = None
    return {k: v.detach().clone() for k, v in fwd.items()}, grads


# ---------------------------------------------------------------------------------------------- the point filter
def away_from_relu_kinks(ora, x, margin=1e-4):
    """[M] bool: every pre-activation h, c of the restatement at least margin * sum |w| |x| away from zero.  Nearer, the ReLU mask (and with it
    a whole row of the backward) is decided by accumulation noise: the two evaluations above may disagree (H.relu_kink_distance is the same
    idea for the exact network)."""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    with torch.no_grad():
        feats, pos = S.hash_encode(xt, ora.table, ora.meta), S.oneblob_encode(xt, ora.n_bins)
        W0, W1, C0 = (BF.bf(w.detach()).double() for w in (ora.sdf_w0, ora.sdf_w1, ora.col_w0))
        in0 = BF.bf(torch.cat([feats, pos], -1)).double()
        h, sh = in0 @ W0.T, in0.abs() @ W0.abs().T
        out = (BF.bf(torch.relu(h).float()).double() @ W1.T).float()
        in1 = BF.bf(torch.cat([pos, out[:, 1:]], -1)).double()
        c, sc = in1 @ C0.T, in1.abs() @ C0.abs().T
    return ((h.abs() >= margin * sh).all(1) & (c.abs() >= margin * sc).all(1)).numpy()


# ---------------------------------------------------------------------------------------------- the point sets
def is_far(x):
    """[M] bool: a coordinate outside the closed form's range (oneblob_sparse_ok: x > -0.93f && x < 1.93f)."""
    x = np.asarray(x, dtype=np.float32)
    return ~((x > np.float32(-0.93)) & (x < np.float32(1.93))).all(axis=1)


def _candidates():
    """Candidate points by group, more than needed of each, fixed seeds: (name, points, how many to keep)."""
    rs = np.random.RandomState(701)
    groups = []
    # each coordinate in centre bin 0 and in centre bin 15 (the closed form's wraps)
    for d in range(3):
        for b in (0, 15):
            x = rs.uniform(0.05, 0.95, size=(6, 3))
            x[:, d] = (b + rs.uniform(0.05, 0.95, size=6)) / 16.0
            groups.append((f"bin {b} of coordinate {d}", x, 1))
    # every coordinate exactly on a bin edge k/16 (as test_bin_edges walks them)
    i = np.arange(17)[:, None]
    groups.append(("bin edges", ((i + 6 * np.arange(3)[None, :]) % 17) / 16.0, 8))
    groups.append(("inside", rs.uniform(0.0, 1.0, size=(80, 3)), N_INSIDE - 6 - 8))
    x = rs.uniform(-0.3, 1.3, size=(160, 3))
    groups.append(("outside", x[((x < 0.0) | (x > 1.0)).any(axis=1)][:60], N_OUTSIDE))
    x = rs.uniform(0.05, 0.95, size=(16, 3))
    x[np.arange(16), np.arange(16) % 3] = np.where(np.arange(16) % 2 == 0, FAR[0], FAR[1])
    groups.append(("far", x, N_FAR))
    return [(n, x.astype(np.float32), k) for n, x, k in groups]


class Points:
    """The fixed point sets: ``x`` [n_in + N_FAR, 3] -- first the in-range pool (its first N_ANCHOR_IN_RANGE are section 1's anchors), then the far
    points -- with one cotangent per point and route.  ``n_candidates`` / ``n_dropped``: what the filter saw of the anchor candidates."""

    def __init__(self, ora, n_in=N_POOL_IN_RANGE):
        keep_in, keep_far, self.n_candidates, self.n_dropped = [], [], 0, 0
        for name, x, k in _candidates():
            ok = away_from_relu_kinks(ora, x)
            self.n_candidates += len(x)
            self.n_dropped += int((~ok).sum())
            assert int(ok.sum()) >= k, f"{name}: {int(ok.sum())} of {len(x)} candidates pass the filter, {k} needed"
            (keep_far if name == "far" else keep_in).append(x[ok][:k])
        anchors, far = np.concatenate(keep_in), np.concatenate(keep_far)
        assert anchors.shape == (N_ANCHOR_IN_RANGE, 3) and far.shape == (N_FAR, 3)
        assert not is_far(anchors).any() and is_far(far).all()
        b = np.floor(anchors[:N_INSIDE].astype(np.float64) * 16.0).astype(np.int64)
        assert all({0, 15} <= set(b[:, d]) for d in range(3)), "anchors: a centre bin 0 / 15 is missing"
        assert ((anchors[:N_INSIDE] >= 0.0) & (anchors[:N_INSIDE] <= 1.0)).all() and ((anchors[N_INSIDE:] < 0.0) | (anchors[N_INSIDE:] > 1.0)).any(axis=1).all()
        more = np.random.RandomState(702).uniform(-0.2, 1.2, size=(n_in - N_ANCHOR_IN_RANGE, 3)).astype(np.float32)
        self.n_in = n_in
        self.x = np.ascontiguousarray(np.concatenate([anchors, more, far]))
        self.far_idx = list(range(n_in, n_in + N_FAR))
        n = self.x.shape[0]
        rs = np.random.RandomState(703)
        self.cot = {"raw": rs.normal(size=(n, 5)).astype(np.float32), "su": rs.normal(size=(n, 2)).astype(np.float32),
                    "geo": rs.normal(size=(n, 15)).astype(np.float32)}
        # the dense flavour's companion: a far point that gets an all-zero cotangent
        self.companion = np.array([[0.37, FAR[0], 0.61]], dtype=np.float32)

    def cot_of(self, idx, route):
        idx = np.asarray(idx, dtype=np.int64)
        return {"raw": self.cot["raw"][idx]} if route == "raw" else {"su": self.cot["su"][idx], "geo": self.cot["geo"][idx]}

    @property
    def anchor_idx(self):
        return list(range(N_ANCHOR_IN_RANGE)) + self.far_idx


def step_flavours(x_list):
    """Per entry of a list of points, the OneBlob form its 64-entry step takes in k_query_bwd_bf and k_query_fwd_bf ("closed" / "dense"): both
    decide by __all over the wave's 64 lanes, and the lanes past the list's end redo its last entry."""
    n = len(x_list)
    far = is_far(x_list)
    out = []
    for s0 in range(0, n, 64):
        lanes = np.minimum(np.arange(s0, s0 + 64), n - 1)
        out += ["dense" if far[lanes].any() else "closed"] * (min(s0 + 64, n) - s0)
    return out


# ---------------------------------------------------------------------------------------------- the two tolerances of section 1
CAP = 2.0 ** -6          # of the tensor's scale at that point: a bf16 ulp is at most 2^-7 relative, an entry a sum of products of two rounded operands
FWD_UNCERT = {"raw": 4, "su": 1}           # the channel that does not pass through the MLPs


def point_errors(got, want, forward):
    """One point, one tensor -> (tight, err / scale, scale).  tight: forward outputs within 2e-5 + 1e-5 |want|, gradients within 2e-5 of the scale
    (the accumulation-order accuracy the two bf16 restatement tests of test_gpu_parity ask for); scale = max |want|."""
    got, want = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(want).detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    scale = float(want.abs().max())
    tight = bool((err <= 2e-5 + 1e-5 * want.abs()).all()) if forward else bool((err <= 2e-5 * scale).all())
    worst = float(err.max())
    return tight, (worst / scale if scale > 0.0 else (0.0 if worst == 0.0 else float("inf"))), scale


def composition_bound(n_points, sum_abs, sum_signed):
    """|G(batch) - sum_i G_i| <= M 2^-23 sum_i |G_i| + 1e-9 max |sum_i G_i|: M fp32 additions of exactly represented addends (with a factor of
    two for the partial sums across tiles, waves and workgroups), and the scatter's 2^-40 fixed point."""
    return n_points * 2.0 ** -23 * sum_abs + 1e-9 * float(sum_signed.abs().max())

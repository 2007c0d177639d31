"""Depth odometry on the device (csrc/naruto_odom.hip, csrc/naruto_odom.h; include/naruto_hip.h states the layout of the maps and state
blocks): the relative motion between two consecutive depth frames by coarse-to-fine projective point-to-plane ICP.  It needs no field, so
it gives the tracker (``CoSLAMNarutoHIP(track=True, motion_prior="depth_icp")``) a start within its reach when the camera moves in a stop,
turn, go pattern that constant-speed extrapolation cannot follow.  Nothing like it is in the reference tree: PARITY UNPINNED, the contract
is this text; tests/odometry_spec.py is its numpy twin.

Convention.  Pixel (u, v) has direction ((u-cx)/fx, -(v-cy)/fy, -1); depth is measured along -z; a depth that is not a finite positive
number is missing.  The estimate ``T`` maps the current camera's coordinates to the previous camera's: ``c2w[i] = c2w[i-1] @ T``.

Frame maps (one launch per frame, kept: the current frame's maps are the next frame's previous maps), float32, every operation rounded:
  * a depth pyramid of ``levels`` levels; level l+1 has floor(h/2) x floor(w/2) pixels (an odd last row / column is not read); a pixel is the
    mean of its 2 x 2 block's valid depths d with d - m <= ``band``, m the block's smallest valid depth, summed in the order (0,0), (0,1),
    (1,0), (1,1); 0 when none is valid.  Intrinsics per level: f/2 and c' = (c + 0.5)/2 - 0.5;
  * per level the vertex map V = depth * direction and the normal map: the normalised cross product of V(u+1,v) - V(u,v) and
    V(u,v+1) - V(u,v), valid when all three vertices are valid, both differences have |dz| < ``jump`` and the length is positive; the last row
    and column have none.  Missing vertices and normals are (0,0,0).

One iteration at level l with the fp64 transform T of the device state block:
  * accumulate, per pixel of the current frame: q = T p (fp64 from the float32 vertex, ((r0*x + r1*y) + r2*z) + t); rejected when
    -q.z <= 1e-6; projected to u = floor(fx*q.x/(-q.z) + cx + 0.5), v likewise with -fy; rejected outside the image, where the previous
    frame has no normal n, or when |q - V_prev| > ``max_dist``.  Residual r = n . (q - V_prev), row J = [q x n, n]: a left perturbation
    T <- exp(xi) T, xi = (omega, t).  29 fp64 sums (the 21 upper entries of J^T J, the 6 of J^T r, sum r^2, the count) in an order that
    depends on the pixel count alone: no atomics, bitwise reproducible;
  * step, one thread: ``degenerate`` (T unchanged) when the count is below 6 or a Cholesky pivot is <= 1e-12 x the largest diagonal entry;
    else xi = -(J^T J)^-1 J^T r and T <- exp(xi) T.  A level is finished when |omega| < 1e-6 and |t| < 1e-6 (``converged``) or after its
    iteration cap (``max_iteration``); ``iters`` lists the caps from the coarsest level to the finest.
The step writes a per-level done word into the state; launches of a finished level return at once.  A whole estimate is therefore a FIXED
sequence of launches -- for each level from the coarsest, cap x (accumulate, step) -- with nothing read back: ``estimate_device`` never
waits for the host.  When every level is degenerate the state's T is still the initial one.

Limits: frame-to-frame only (drift is left to the tracker and global_BA); depth only, no photometric term; the two views must overlap.

RGB-D ODOMETRY (``RGBDOdometryHIP``, ``motion_prior="rgbd_icp"``): the same estimate with a photometric row per pixel beside the geometric
one.  A plane seen head on leaves three motions free for the depth rows (degenerate, T unchanged); the image on the plane pins them.
PARITY UNPINNED as above; tests/odometry_rgbd_spec.py is the numpy twin.  The camera convention, T, the state block, the level schedule,
the done words and the step are those of the depth odometry.

Intensity maps, float32 with contraction off like the depth maps:
  * level 0: I = (0.299 r + 0.587 g) + 0.114 b of the colour frame [H,W,3] (float32, 0 .. 1); level l+1: (((a + b) + c) + d) * 0.25 over
    the 2 x 2 block in the order (0,0), (0,1), (1,0), (1,1), an odd last row / column not read; every thread nests the means down to level 0;
  * gx(u,v) = (I(u+1,v) - I(u-1,v)) * 0.5 for 1 <= u <= w-2, else 0; gy the same in v.
RGB-D maps block: the depth maps block (same layout, same bits as ``DepthOdometryHIP.frame_maps``), then the intensity block: per level, at
3 x (the pixels of the levels before it) floats, I [h*w] | gx [h*w] | gy [h*w].  One launch per frame writes both.

One evaluation at a level, per pixel i of the current frame, fp64 without contraction:
  1. the geometric row, exactly the depth odometry's (association, rejections, J, r, order);
  2. the photometric row, only when ``photo_weight`` > 0, from the same q = T p with p.z < 0 and zc = -q.z > 1e-6:
     uc = (fx q.x)/zc + cx, vc = (-(fy q.y))/zc + cy, u0 = floor(uc), v0 = floor(vc); rejected unless 1 <= u0, u0+1 <= w-2, 1 <= v0,
     v0+1 <= h-2 (the four neighbours are interior pixels whose gradients are central differences); with j the geometric row's nearest
     pixel (floor(uc+0.5), floor(vc+0.5)), rejected unless V_prev[j].z < 0 and |q - V_prev[j]|^2 <= max_dist^2 (an occlusion test; no
     normal is needed).  I_prev, gx_prev, gy_prev are sampled bilinearly with a = uc - u0, b = vc - v0: top = s00 + a (s10 - s00),
     bot = s01 + a (s11 - s01), s = top + b (bot - top) (s10 at (u0+1, v0)).  r_I = I_prev(uc,vc) - I_cur[i]; rejected unless
     |r_I| <= ``photo_max_diff`` and both sampled gradients are finite (a NaN fails the comparison, so non-finite colours drop out here).
     With w = ``photo_weight`` (metres per unit of intensity; the float32 value as a double), A = gx fx, B = gy fy, in this order:
     g = (w (A/zc), w (-(B/zc)), w ((A q.x - B q.y)/(zc zc))), r = w r_I, J = [q x g, g]: the geometric row's form with g for n, so one
     accumulation routine serves both;
  3. 32 fp64 sums: [0..28] as above over the rows of BOTH kinds (the count too), [29] the geometric rows, [30] the photometric rows,
     [31] sum r_I^2 unweighted.  Per pixel the geometric row's terms are added first, then the photometric row's; pixels, threads, the fold
     and the finishing launch in the depth odometry's order: no atomics, bitwise reproducible;
  4. the step is the depth odometry's, unchanged, on the first 29 sums: a level's ``inliers`` and ``rmse`` then count and mix both kinds of
     rows (rmse^2 = (sum r^2 + w^2 sum r_I^2) / rows).
Defaults ``photo_weight = 0.1``, ``photo_max_diff = 0.3``.  Limits: the photometric term needs texture and overlap, and assumes that a
surface point's intensity is the same in both frames; a failed estimate is not detected unless the gate below is on.

SCORED STARTS AND A VERDICT (``OdometryGate``; ``estimate_gated``, ``estimate_gated_device``; opt-in for both classes, nothing above changes;
``CoSLAMNarutoHIP(prior_gate=...)``).  PARITY UNPINNED as above; tests/odometry_gate_spec.py is the numpy twin and
tests/test_odometry_gate_host.py the study the defaults come from.  An estimate converges only from a start inside its basin and a lost one
looks like any other, so:
  * ``score``: K <= 4 candidate transforms in one pass over a level.  Per pixel the vertex p is read once; [0] counts the pixels with
    p.z < 0 (``n_valid``).  Per candidate k the geometric row's association, rejections and residual r exactly as ``accumulate`` makes them
    (the same device function): [1+4k] the rows, [2+4k] the sum of min(r*r, trunc*trunc) (r*r < trunc*trunc ? r*r : trunc*trunc).  With
    ``photo_weight`` > 0 (RGB-D blocks) the photometric row's acceptance, gradient test included: [3+4k] the rows, [4+4k] the sum of
    r_I*r_I; else 0.  fp64, no contraction, pixels / threads / fold / finishing launch in ``accumulate``'s order: no atomics, bitwise
    reproducible.  At K = 1 with trunc = max_dist, [1], [2] are ``accumulate``'s [28], [27] bit for bit, and [1], [3], [4] the RGB-D
    ``accumulate``'s [29], [30], [31].  A candidate with a non-finite entry gets no rows and changes no other candidate's sums;
  * ``candidates`` (one thread): the identity and the last motion inv(est[i-2]) @ est[i-1] (i > 1; ``init_state``'s bits), else the identity;
  * ``choose`` (one thread): cost[k] = (s + (n_valid - n) tau^2) / (n_valid tau^2) with s = [2+4k], n = [1+4k], tau = trunc -- every valid
    pixel without a row costs as much as a truncated one -- plus the same expression of the photometric pair with tau = ``photo_max_diff``
    when the photometric term is on; 1 per term when n_valid = 0, +inf when not finite.  The lowest cost wins, ties go to the lowest index,
    index 0 when all are +inf.  The state block is written as ``init_state`` writes it with that T;
  * the level loop, untouched;
  * a K = 1 score of the state's T at level 0 with trunc = max_dist, and ``verdict`` (one thread): PASS iff level 0's status is not
    ``degenerate``, n_geo >= ``min_overlap`` n_valid, n_geo > 0 and s_geo <= ``max_rmse``^2 n_geo, |t|^2 <= ``max_trans``^2 and
    trace(R) >= 1 + 2 cos(``max_rot_deg``) (the host computes that bound).  A NaN fails its comparison.  On FAIL the state's T becomes the
    chosen start.  No second attempt, no photometric verdict (those figures are only recorded).
Record, 16 doubles per estimate: verdict (1 PASS / 0 FAIL), chosen index, four costs (-1 = unused), n_valid, n_geo, rmse, |t|, trace,
level 0's status, n_photo, photometric rmse, 0, 0; rmse, |t|, trace and the photometric rmse are -1 where not finite.  The whole gated
estimate is a fixed sequence of launches -- candidates, score, finish, choose, the level loop, score, finish, verdict: six more than
``init_state`` + the level loop -- and nothing is read back.  Defaults (the study: zero lost estimates passed, zero converged ones refused
over 80): ``max_trans`` 0.3 m, ``max_rot_deg`` 30, ``min_overlap`` 0.25, ``max_rmse`` 6 mm, ``score_trunc`` 5 cm.  Limits: views without
overlap fail from every start and are only flagged; the thresholds were chosen at 80 x 60 and 160 x 120 in a closed room.

A REFERENCE RING (``AnchorPolicy``; ``new_anchor``, ``anchor_reset``, ``estimate_anchored_device``, ``chain``; opt-in for both classes, nothing
above changes; ``CoSLAMNarutoHIP(prior_anchor=...)``).  PARITY UNPINNED as above; tests/odometry_anchor_spec.py is the numpy twin.  The
gated estimate composes every T onto the frame before it, so every estimate's bias and noise stays in the pose for good.  Here frame i
is registered to one of ``slots`` kept frames and ``est[i] = est[that frame] @ T``.  All of it lives on the device:
  * the ring: ``slots`` (1 .. 8, default 4) maps blocks of this odometry's own layout, back to back;
  * the head, int32 [12]: [0] the slot written last, [1] the count of consecutive refused estimates, [2] the slot chosen for the current
    frame, [3] the promote decision of the current frame, [4 + s] slot s's frame id (-1 = empty).  A slot's pose is not stored: it is
    ``est[frame id]`` as it stands when it is read, so the tracker's result and a ``global_BA`` write-back reach it.  A slot word that is not
    below ``slots`` reads the last slot: no word leaves the ring.
Per frame i >= 1, after ``frame_maps`` (unchanged); every step is a launch, nothing is read back, no kernel waits on a device word:
  * ``anchor_candidates`` (one thread): per slot s with frame f the two starts R = inv(est[f]) @ est[i-1] and R @ M, M the last motion
    inv(est[i-2]) @ est[i-1] (i > 1, else the identity): the pose chain's inverse and product, fp64 from the float32 matrices.  When
    f = i-1 (and for an empty slot) the pair is ``candidates``' own, bit for bit: no inverse times itself;
  * ``score_refs``: ``score`` at K = 2 for every slot in one launch and one finishing launch; slot s's nine sums equal ``score`` on that
    slot's block and pair in every bit; an empty slot's workgroups leave at once, its sums are zeros;
  * ``anchor_choose`` (one thread): ``choose``'s cost per (slot, start) of the slots that hold a frame; the lowest wins, ties go to the
    larger frame id, then to the lower start; a cost that is not finite is +inf; no such slot, or every cost +inf: the slot written last
    with start 0.  It writes head[2], the chosen slot's pair into ``cands`` (what the unchanged ``verdict`` reads), the state block and
    record [1..5] as ``choose`` does, and the anchor record's [0], [1], [2], [6], [7];
  * the level loop and the K = 1 score at level 0: the existing kernels' bodies, with the previous maps = the ring's block head[2],
    resolved at kernel entry; ``step`` and ``verdict`` unchanged;
  * ``anchor_update`` (one thread), from the verdict's record, T being relative to the chosen reference: after a PASS the frame is promoted
    when n_geo < ``min_overlap`` n_valid, |t| > ``max_trans`` or trace(R) < 1 + 2 cos(``max_rot_deg``), and the streak is 0; after a FAIL
    the streak grows, and the ``refail``-th refusal in a row promotes the frame (which is what frame-to-frame odometry does every frame)
    and clears the streak.  A promoted frame takes slot (head[0] + 1) mod ``slots``; the head records it there;
  * ``anchor_promote``: a copy of the current maps into that slot; every workgroup reads the decision word first; other slots untouched;
  * ``pose_chain.pose_predict_anchored``: est[i] = est[f] @ T, f read from the anchor record.
Anchor record, 8 doubles per frame: the chosen slot, its frame id, the slots that held a frame, promoted, the slot written (-1 = none), the
fail streak after the frame, the best cost, the runner-up among all (slot, start) pairs (-1 where +inf).  Defaults (the study of DESIGN 7o):
``slots`` 4, ``min_overlap`` 0.7, ``max_trans`` 0.10 m, ``max_rot_deg`` 10, ``refail`` 2; they must lie strictly inside the gate's, or no
passing frame could ever be promoted before the gate refuses.  Limits: no second attempt, no loop closure, eviction is the ring's.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import check
from .ops import _on_device, _stream


def _intrinsics(cam) -> tuple:
    if isinstance(cam, dict):
        return tuple(cam[k] for k in ("H", "W", "fx", "fy", "cx", "cy"))
    cam = tuple(cam)
    if len(cam) != 6:
        raise ValueError("DepthOdometryHIP: the camera is a dict with H, W, fx, fy, cx, cy or that tuple")
    return cam


@dataclass
class OdometryGate:
    """The gate of the odometry prior (module docstring): the verdict's four thresholds and the truncation of the start's cost."""
    max_trans: float = 0.3          # metres between two consecutive frames
    max_rot_deg: float = 30.0       # degrees
    min_overlap: float = 0.25       # geometric rows / valid pixels at level 0
    max_rmse: float = 0.006         # metres, over the geometric rows at level 0
    score_trunc: float = 0.05       # metres: tau of the start's cost

    def __post_init__(self):
        if not (all(math.isfinite(v) for v in (self.max_trans, self.max_rot_deg, self.min_overlap, self.max_rmse, self.score_trunc))
                and self.max_trans >= 0 and 0 <= self.max_rot_deg <= 180 and 0 <= self.min_overlap <= 1 and self.max_rmse >= 0 and self.score_trunc > 0):
            raise ValueError(f"OdometryGate: {self!r}: max_trans, max_rmse >= 0, max_rot_deg in 0 .. 180, min_overlap in 0 .. 1, score_trunc > 0")

    @staticmethod
    def of(gate) -> "OdometryGate":
        """None or True: the defaults; an OdometryGate: itself."""
        if gate is None or gate is True:
            return OdometryGate()
        if not isinstance(gate, OdometryGate):
            raise ValueError(f"the gate is None, True or an OdometryGate; got {gate!r}")
        return gate

    def abi(self):
        """The HOST struct of naruto_odom_verdict: min_trace = 1 + 2 cos(max_rot), made here so that the kernel needs no cosine."""
        return _lib.NarutoOdomGate(max_trans=float(self.max_trans), min_trace=1.0 + 2.0 * math.cos(math.radians(self.max_rot_deg)),
                                   min_overlap=float(self.min_overlap), max_rmse=float(self.max_rmse))


@dataclass
class AnchorPolicy:
    """The reference ring of the odometry prior (module docstring): its size and when a frame becomes a reference.  The three limits must
    lie strictly inside those of ``gate`` (default: ``OdometryGate()``); ``within`` checks them against another gate."""
    slots: int = 4
    min_overlap: float = 0.7        # geometric rows / valid pixels against the chosen reference: below it the frame is promoted
    max_trans: float = 0.10         # metres to the chosen reference: above it the frame is promoted
    max_rot_deg: float = 10.0       # degrees to the chosen reference: above it the frame is promoted
    refail: int = 2                 # this many refused estimates in a row promote the current frame
    gate: Optional[OdometryGate] = None

    def __post_init__(self):
        if not (isinstance(self.slots, int) and 1 <= self.slots <= _lib.ODOM_MAX_REFS and isinstance(self.refail, int) and 1 <= self.refail < 2 ** 30):
            raise ValueError(f"AnchorPolicy: slots = {self.slots!r} (1 .. {_lib.ODOM_MAX_REFS}), refail = {self.refail!r} (an int >= 1)")
        if not (all(math.isfinite(v) for v in (self.min_overlap, self.max_trans, self.max_rot_deg)) and 0 <= self.min_overlap <= 1
                and self.max_trans >= 0 and 0 <= self.max_rot_deg <= 180):
            raise ValueError(f"AnchorPolicy: {self!r}: min_overlap in 0 .. 1, max_trans >= 0, max_rot_deg in 0 .. 180")
        self.within(self.gate)

    def within(self, gate) -> "AnchorPolicy":
        """Raises ValueError unless every limit lies strictly inside ``gate``'s: otherwise the gate refuses before the ring can move on."""
        gate = OdometryGate.of(gate)
        if not (self.min_overlap > gate.min_overlap and self.max_trans < gate.max_trans and self.max_rot_deg < gate.max_rot_deg):
            raise ValueError(f"AnchorPolicy: min_overlap {self.min_overlap} / max_trans {self.max_trans} / max_rot_deg {self.max_rot_deg} must lie strictly "
                             f"inside the gate's {gate.min_overlap} / {gate.max_trans} / {gate.max_rot_deg}")
        return self

    @staticmethod
    def of(policy) -> "AnchorPolicy":
        """None or True: the defaults; an AnchorPolicy: itself."""
        if policy is None or policy is True:
            return AnchorPolicy()
        if not isinstance(policy, AnchorPolicy):
            raise ValueError(f"the anchor policy is None, True or an AnchorPolicy; got {policy!r}")
        return policy

    def abi(self):
        """The HOST struct of naruto_odom_anchor_update: min_trace = 1 + 2 cos(max_rot), as ``OdometryGate.abi``."""
        return _lib.NarutoOdomAnchor(slots=int(self.slots), refail=int(self.refail), min_overlap=float(self.min_overlap), max_trans=float(self.max_trans),
                                     min_trace=1.0 + 2.0 * math.cos(math.radians(self.max_rot_deg)))


class DepthOdometryHIP:
    def __init__(self, cam: Union[Dict, Sequence], levels: int = 3, iters: Sequence[int] = (10, 5, 4), max_dist: float = 0.25, jump: float = 0.15,
                 band: float = 0.1, device="cuda"):
        H, W, fx, fy, cx, cy = _intrinsics(cam)
        self.H, self.W, self.levels, self.iters = int(H), int(W), int(levels), tuple(int(k) for k in iters)
        if not 1 <= self.levels <= _lib.ODOM_MAX_LEVELS or len(self.iters) != self.levels or min(self.iters) < 1:
            raise ValueError(f"DepthOdometryHIP: levels = {levels} (1 .. {_lib.ODOM_MAX_LEVELS}) needs as many iteration caps >= 1, coarse to fine; got {iters!r}")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.desc = _lib.NarutoOdomDesc(H=self.H, W=self.W, levels=self.levels, iters=(C.c_uint32 * _lib.ODOM_MAX_LEVELS)(*self.iters),
                                        fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), max_dist=float(max_dist), jump=float(jump), band=float(band))
        lib = _lib.load()
        self.maps_bytes = int(lib.naruto_odom_maps_bytes(C.byref(self.desc)))
        ws = int(lib.naruto_odom_workspace_bytes(C.byref(self.desc)))
        if self.maps_bytes == 0 or ws == 0:
            raise ValueError("DepthOdometryHIP: " + lib.naruto_last_error().decode("utf-8", "replace"))
        self.workspace = _lib.workspace(ws, self.device, torch.float64)
        self.sums = torch.zeros(_lib.ODOM_SUMS, dtype=torch.float64, device=self.device)
        self.state = torch.zeros(_lib.ODOM_STATE_DOUBLES, dtype=torch.float64, device=self.device)
        # (h, w, offset in floats) of every level inside a maps block
        self.level_shapes, off, h, w = [], 0, self.H, self.W
        for _ in range(self.levels):
            self.level_shapes.append((h, w, off))
            off, h, w = off + 7 * h * w, h // 2, w // 2

    def new_maps(self) -> torch.Tensor:
        return torch.empty(self.maps_bytes // 4, dtype=torch.float32, device=self.device)

    def frame_maps(self, depth: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The maps block of the depth frame [H,W] (float32 on the device): one launch."""
        depth = depth.to(self.device, torch.float32).contiguous()
        if depth.numel() != self.H * self.W:
            raise ValueError(f"DepthOdometryHIP: a depth frame of {tuple(depth.shape)}, built for {self.H} x {self.W}")
        out = self.new_maps() if out is None else out
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() * 4 == self.maps_bytes):
            raise ValueError("DepthOdometryHIP: out must be a maps block of new_maps()")
        with _on_device(self.device):
            check(_lib.load().naruto_odom_frame_maps(C.byref(self.desc), depth.data_ptr(), out.data_ptr(), _stream()), "naruto_odom_frame_maps")
        return out

    def level_views(self, maps: torch.Tensor, level: int):
        """(depth [h,w], vertex [h,w,3], normal [h,w,3]): views into a maps block."""
        h, w, off = self.level_shapes[level]
        n = h * w
        return maps[off:off + n].view(h, w), maps[off + n:off + 4 * n].view(h, w, 3), maps[off + 4 * n:off + 7 * n].view(h, w, 3)

    def init_state(self, init=None, est: Optional[torch.Tensor] = None, i: int = 0, const_speed: bool = False, state: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The state block with T = ``init`` ([4,4], host), else the last motion inv(est[i-2]) @ est[i-1] read ON THE DEVICE when ``est`` is
        given with ``const_speed`` and i > 1, else the identity: one launch."""
        state = self.state if state is None else state
        T = None
        if init is not None:
            T = C.byref(_lib.NarutoOdomInit(T=(C.c_double * 16)(*np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init,
                                                                             dtype=np.float64).reshape(16))))
        with _on_device(self.device):
            check(_lib.load().naruto_odom_state_init(T, None if est is None else est.data_ptr(), 0 if est is None else est.shape[0], int(i),
                                                     1 if const_speed else 0, state.data_ptr(), _stream()), "naruto_odom_state_init")
        return state

    def accumulate(self, level: int, maps_prev: torch.Tensor, maps_cur: torch.Tensor, state: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
        state = self.state if state is None else state
        with _on_device(self.device):
            check(_lib.load().naruto_odom_accumulate(C.byref(self.desc), int(level), maps_prev.data_ptr(), maps_cur.data_ptr(), state.data_ptr(),
                                                     self.sums.data_ptr(), self.workspace.data_ptr(), None if rows is None else rows.data_ptr(), _stream()),
                  "naruto_odom_accumulate")
        return self.sums

    def step(self, level: int, state: Optional[torch.Tensor] = None) -> None:
        state = self.state if state is None else state
        with _on_device(self.device):
            check(_lib.load().naruto_odom_step(C.byref(self.desc), int(level), self.sums.data_ptr(), state.data_ptr(), _stream()), "naruto_odom_step")

    def run_levels(self, maps_prev: torch.Tensor, maps_cur: torch.Tensor, state: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fixed launch sequence over an initialised state: for each level from the coarsest, cap x (accumulate, step)."""
        state = self.state if state is None else state
        for k, cap in enumerate(self.iters):
            level = self.levels - 1 - k
            for _ in range(cap):
                self.accumulate(level, maps_prev, maps_cur, state)
                self.step(level, state)
        return state

    def estimate_device(self, maps_prev: torch.Tensor, maps_cur: torch.Tensor, init=None) -> torch.Tensor:
        """Launches only.  Returns the device state block (float64 [48]; its first 16 doubles are T), owned by this object."""
        return self.run_levels(maps_prev, maps_cur, self.init_state(init))

    # ------------------------------------------------------------------------------------ scored starts and a verdict (module docstring)
    _photo_on = False

    def _photo_ref(self):
        return None                                                        # the maps are depth blocks

    def _gate_buffers(self) -> None:
        if getattr(self, "cands", None) is None:
            lib = _lib.load()
            self.cands = torch.zeros(_lib.ODOM_MAX_CANDS * 16, dtype=torch.float64, device=self.device)
            self.score_sums = torch.zeros(1 + 4 * _lib.ODOM_MAX_CANDS, dtype=torch.float64, device=self.device)
            self.score_workspace = _lib.workspace(int(lib.naruto_odom_score_workspace_bytes(C.byref(self.desc), _lib.ODOM_MAX_CANDS)), self.device, torch.float64)
            self.record = torch.zeros(_lib.ODOM_GATE_WORDS, dtype=torch.float64, device=self.device)

    def _candidates(self, candidates) -> int:
        """``candidates`` ([K,4,4] on the host, or a float64 device tensor of K x 16 doubles) into ``self.cands``; returns K."""
        self._gate_buffers()
        if isinstance(candidates, torch.Tensor) and candidates.is_cuda:
            c = candidates.to(torch.float64).reshape(-1)
        else:
            c = torch.from_numpy(np.ascontiguousarray(np.asarray(candidates.cpu() if isinstance(candidates, torch.Tensor) else candidates,
                                                                 dtype=np.float64).reshape(-1)))
        K = c.numel() // 16
        if c.numel() != 16 * K or not 1 <= K <= _lib.ODOM_MAX_CANDS:
            raise ValueError(f"{type(self).__name__}: candidates are 1 .. {_lib.ODOM_MAX_CANDS} transforms [K,4,4]; got {c.numel()} numbers")
        if c.data_ptr() != self.cands.data_ptr():
            self.cands[:16 * K].copy_(c, non_blocking=True)
        return K

    def _score(self, level: int, maps_prev: torch.Tensor, maps_cur: torch.Tensor, cands: torch.Tensor, K: int, trunc: float, sums: torch.Tensor) -> None:
        check(_lib.load().naruto_odom_score(C.byref(self.desc), self._photo_ref(), int(level), maps_prev.data_ptr(), maps_cur.data_ptr(), cands.data_ptr(),
                                            int(K), float(trunc), sums.data_ptr(), self.score_workspace.data_ptr(), _stream()), "naruto_odom_score")

    def score(self, maps_prev: torch.Tensor, maps_cur: torch.Tensor, candidates, level: Optional[int] = None, trunc: Optional[float] = None) -> torch.Tensor:
        """The 1 + 4 K sums of K candidate transforms at ``level`` (default: the coarsest) with the residual truncated at ``trunc`` metres
        (default: ``OdometryGate.score_trunc``): float64 on the device, a view of ``score_sums``, owned by this object.  ``candidates``: [K,4,4] on the
        host (copied into ``self.cands``) or a contiguous float64 device tensor [K,16], read in place.  Launches only."""
        self._gate_buffers()
        if isinstance(candidates, torch.Tensor) and candidates.is_cuda:        # read in place: a state block's head is one candidate
            if candidates.dtype != torch.float64 or not candidates.is_contiguous() or candidates.numel() % 16 or not 16 <= candidates.numel() <= 16 * _lib.ODOM_MAX_CANDS:
                raise ValueError(f"{type(self).__name__}: device candidates are contiguous float64 [K,16], K = 1 .. {_lib.ODOM_MAX_CANDS}")
            cands, K = candidates, candidates.numel() // 16
        else:
            cands, K = self.cands, self._candidates(candidates)
        level = self.levels - 1 if level is None else int(level)
        with _on_device(self.device):
            self._score(level, maps_prev, maps_cur, cands, K, OdometryGate.score_trunc if trunc is None else trunc, self.score_sums)
        return self.score_sums[:1 + 4 * K]

    def candidates(self, est: torch.Tensor, i: int) -> torch.Tensor:
        """The two starts of frame ``i`` into ``self.cands``, made on the device: the identity and inv(est[i-2]) @ est[i-1] (i > 1, else the
        identity once more).  ``est``: float32 [num_frames,4,4] on the device.  Returns the view [2,16]: one launch."""
        self._gate_buffers()
        with _on_device(self.device):
            check(_lib.load().naruto_odom_candidates(est.data_ptr(), est.shape[0], int(i), self.cands.data_ptr(), _stream()), "naruto_odom_candidates")
        return self.cands[:32].view(2, 16)

    def choose(self, K: int, trunc: float, state: torch.Tensor, record: torch.Tensor) -> None:
        """``naruto_odom_choose`` on ``score_sums`` and ``cands``: the cheapest start's T into ``state``, the record's head: one launch."""
        with _on_device(self.device):
            self._choose(K, trunc, state, record)

    def verdict(self, gate=None, state: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None) -> None:
        """``naruto_odom_verdict`` on ``score_sums`` (a K = 1 score of the state's T at level 0 with trunc = max_dist): one launch."""
        gate, state, record = OdometryGate.of(gate), self.state if state is None else state, self.record if record is None else record
        with _on_device(self.device):
            check(_lib.load().naruto_odom_verdict(C.byref(self.desc), C.byref(gate.abi()), self.score_sums.data_ptr(), self.cands.data_ptr(), state.data_ptr(),
                                                  record.data_ptr(), _stream()), "naruto_odom_verdict")

    def _choose(self, K: int, trunc: float, state: torch.Tensor, record: torch.Tensor) -> None:
        check(_lib.load().naruto_odom_choose(int(K), self.score_sums.data_ptr(), self.cands.data_ptr(), 1 if self._photo_on else 0, float(trunc),
                                             float(self.photo.max_diff) if self._photo_on else 0.0, state.data_ptr(), record.data_ptr(), _stream()),
              "naruto_odom_choose")

    def costs(self, maps_prev: torch.Tensor, maps_cur: torch.Tensor, candidates, level: Optional[int] = None, trunc: Optional[float] = None) -> np.ndarray:
        """The K costs ``naruto_odom_choose`` compares (float64 on the host; synchronises).  ``self.state`` and ``self.record`` are not touched."""
        trunc = OdometryGate.score_trunc if trunc is None else trunc
        K = self._candidates(candidates)
        self.score(maps_prev, maps_cur, self.cands[:16 * K], level, trunc)
        state, record = torch.empty_like(self.state), torch.empty_like(self.record)
        self.choose(K, trunc, state, record)
        return record[2:2 + K].cpu().numpy()

    def estimate_gated_device(self, maps_prev: torch.Tensor, maps_cur: torch.Tensor, est: Optional[torch.Tensor] = None, i: int = 0, gate=None,
                              record: Optional[torch.Tensor] = None, candidates=None) -> torch.Tensor:
        """The gated estimate (module docstring): launches only.  The starts are the identity and the last motion of ``est`` at frame ``i``
        (made on the device) when ``est`` is given, else ``candidates`` (default: the identity alone).  ``record``: float64 [16] on the device
        (default ``self.record``).  Returns the state block; after a FAIL its T is the chosen start."""
        gate = OdometryGate.of(gate)
        self._gate_buffers()
        record = self.record if record is None else record
        if not (record.is_cuda and record.dtype == torch.float64 and record.is_contiguous() and record.numel() == _lib.ODOM_GATE_WORDS):
            raise ValueError(f"{type(self).__name__}: record is float64 [{_lib.ODOM_GATE_WORDS}] on the device")
        state = self.state
        if est is None:
            K = self._candidates(np.eye(4)[None] if candidates is None else candidates)
        else:
            self.candidates(est, i)
            K = 2
        with _on_device(self.device):
            self._score(self.levels - 1, maps_prev, maps_cur, self.cands, K, gate.score_trunc, self.score_sums)
            self._choose(K, gate.score_trunc, state, record)
        self.run_levels(maps_prev, maps_cur, state)
        with _on_device(self.device):
            self._score(0, maps_prev, maps_cur, state, 1, float(self.desc.max_dist), self.score_sums)
        self.verdict(gate, state, record)
        return state

    # ------------------------------------------------------------------------------------ a reference ring (module docstring)
    def new_anchor(self, policy=None) -> SimpleNamespace:
        """The device side of a reference ring: ``.ring`` float32 [slots, a maps block], ``.head`` int32 [12] (all slots empty),
        ``.cands`` float64 [slots,2,16], ``.sums`` float64 [slots,9], ``.workspace``, ``.record`` float64 [8], and ``.policy``."""
        policy = AnchorPolicy.of(policy)
        self._gate_buffers()
        ws = int(_lib.load().naruto_odom_score_refs_workspace_bytes(C.byref(self.desc), policy.slots))
        if ws == 0:
            raise ValueError(f"{type(self).__name__}: " + _lib.load().naruto_last_error().decode("utf-8", "replace"))
        head = torch.tensor([0, 0, 0, 0] + [-1] * _lib.ODOM_MAX_REFS, dtype=torch.int32).to(self.device)
        return SimpleNamespace(policy=policy, slots=policy.slots, ring=torch.zeros(policy.slots, self.maps_bytes // 4, dtype=torch.float32, device=self.device),
                               head=head, cands=torch.zeros(policy.slots, 2, 16, dtype=torch.float64, device=self.device),
                               sums=torch.zeros(policy.slots, 9, dtype=torch.float64, device=self.device),
                               workspace=_lib.workspace(ws, self.device, torch.float64),
                               record=torch.zeros(_lib.ODOM_ANCHOR_WORDS, dtype=torch.float64, device=self.device))

    def anchor_reset(self, anchor: SimpleNamespace, maps: torch.Tensor, frame: int = 0) -> None:
        """``maps`` (frame ``frame``'s block) into slot 0 and the head from the host: that slot alone holds a frame, nothing is refused."""
        if maps.numel() * 4 != self.maps_bytes:
            raise ValueError(f"{type(self).__name__}: maps must be a maps block of new_maps()")
        anchor.ring[0].copy_(maps.reshape(-1), non_blocking=True)
        anchor.head.copy_(torch.tensor([0, 0, 0, 0, int(frame)] + [-1] * (_lib.ODOM_MAX_REFS - 1), dtype=torch.int32))

    def anchor_candidates(self, anchor: SimpleNamespace, est: torch.Tensor, i: int) -> torch.Tensor:
        """Every slot's two starts of frame ``i`` into ``anchor.cands`` [slots,2,16]: one launch."""
        with _on_device(self.device):
            check(_lib.load().naruto_odom_anchor_candidates(est.data_ptr(), est.shape[0], int(i), anchor.head.data_ptr(), anchor.slots, anchor.cands.data_ptr(),
                                                            _stream()), "naruto_odom_anchor_candidates")
        return anchor.cands

    def score_refs(self, anchor: SimpleNamespace, maps_cur: torch.Tensor, level: Optional[int] = None, trunc: Optional[float] = None) -> torch.Tensor:
        """``score`` at K = 2 of every slot's pair against that slot's block into ``anchor.sums`` [slots,9]: two launches."""
        level = self.levels - 1 if level is None else int(level)
        with _on_device(self.device):
            check(_lib.load().naruto_odom_score_refs(C.byref(self.desc), self._photo_ref(), level, anchor.ring.data_ptr(), anchor.head.data_ptr(), anchor.slots,
                                                     maps_cur.data_ptr(), anchor.cands.data_ptr(), float(OdometryGate.score_trunc if trunc is None else trunc),
                                                     anchor.sums.data_ptr(), anchor.workspace.data_ptr(), _stream()), "naruto_odom_score_refs")
        return anchor.sums

    def anchor_choose(self, anchor: SimpleNamespace, trunc: float, state: torch.Tensor, record: torch.Tensor, anchor_record: Optional[torch.Tensor] = None) -> None:
        """``naruto_odom_anchor_choose`` on ``anchor.sums`` and ``anchor.cands``: the head's chosen slot, its pair into ``self.cands``, the state
        block, the record's head and the anchor record's: one launch."""
        self._gate_buffers()
        anchor_record = anchor.record if anchor_record is None else anchor_record
        with _on_device(self.device):
            check(_lib.load().naruto_odom_anchor_choose(anchor.slots, anchor.sums.data_ptr(), anchor.cands.data_ptr(), 1 if self._photo_on else 0, float(trunc),
                                                        float(self.photo.max_diff) if self._photo_on else 0.0, anchor.head.data_ptr(), self.cands.data_ptr(),
                                                        state.data_ptr(), record.data_ptr(), anchor_record.data_ptr(), _stream()), "naruto_odom_anchor_choose")

    def accumulate_anchored(self, level: int, anchor: SimpleNamespace, maps_cur: torch.Tensor, state: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``accumulate`` with the previous maps = the ring's block ``head[2]``, resolved on the device."""
        state = self.state if state is None else state
        with _on_device(self.device):
            check(_lib.load().naruto_odom_accumulate_anchored(C.byref(self.desc), self._photo_ref(), int(level), anchor.ring.data_ptr(), anchor.head.data_ptr(),
                                                              anchor.slots, maps_cur.data_ptr(), state.data_ptr(), self.sums.data_ptr(), self.workspace.data_ptr(),
                                                              _stream()), "naruto_odom_accumulate_anchored")
        return self.sums

    def score_anchored(self, anchor: SimpleNamespace, maps_cur: torch.Tensor, cands: torch.Tensor, level: int = 0, trunc: Optional[float] = None) -> torch.Tensor:
        """``score`` at K = 1 of ``cands`` (float64 [16] on the device: a state block's head) against the ring's block ``head[2]``."""
        self._gate_buffers()
        with _on_device(self.device):
            check(_lib.load().naruto_odom_score_anchored(C.byref(self.desc), self._photo_ref(), int(level), anchor.ring.data_ptr(), anchor.head.data_ptr(),
                                                         anchor.slots, maps_cur.data_ptr(), cands.data_ptr(), float(self.desc.max_dist if trunc is None else trunc),
                                                         self.score_sums.data_ptr(), self.score_workspace.data_ptr(), _stream()), "naruto_odom_score_anchored")
        return self.score_sums[:5]

    def anchor_update(self, anchor: SimpleNamespace, i: int, record: torch.Tensor, anchor_record: Optional[torch.Tensor] = None) -> None:
        """The promote decision of frame ``i`` from the verdict's ``record`` into the head and the anchor record: one launch."""
        anchor_record = anchor.record if anchor_record is None else anchor_record
        with _on_device(self.device):
            check(_lib.load().naruto_odom_anchor_update(C.byref(anchor.policy.abi()), int(i), record.data_ptr(), anchor.head.data_ptr(), anchor_record.data_ptr(),
                                                        _stream()), "naruto_odom_anchor_update")

    def anchor_promote(self, anchor: SimpleNamespace, maps_cur: torch.Tensor) -> None:
        """The current maps into the slot the update chose when the decision word is set, else nothing: one launch."""
        if maps_cur.numel() * 4 != self.maps_bytes:
            raise ValueError(f"{type(self).__name__}: maps_cur must be a maps block of new_maps()")
        with _on_device(self.device):
            check(_lib.load().naruto_odom_anchor_promote(C.byref(self.desc), self._photo_ref(), anchor.slots, anchor.head.data_ptr(), maps_cur.data_ptr(),
                                                         anchor.ring.data_ptr(), _stream()), "naruto_odom_anchor_promote")

    def estimate_anchored_device(self, anchor: SimpleNamespace, maps_cur: torch.Tensor, est: torch.Tensor, i: int, gate=None,
                                 record: Optional[torch.Tensor] = None, anchor_record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The anchored estimate of frame ``i`` (module docstring): launches only.  ``record``: float64 [16], ``anchor_record``: float64 [8], both on
        the device (defaults ``self.record``, ``anchor.record``).  Returns the state block: T relative to the reference the anchor record names,
        for ``pose_chain.pose_predict_anchored``."""
        gate = OdometryGate.of(gate)
        anchor.policy.within(gate)
        self._gate_buffers()
        record = self.record if record is None else record
        anchor_record = anchor.record if anchor_record is None else anchor_record
        if not (record.is_cuda and record.dtype == torch.float64 and record.is_contiguous() and record.numel() == _lib.ODOM_GATE_WORDS):
            raise ValueError(f"{type(self).__name__}: record is float64 [{_lib.ODOM_GATE_WORDS}] on the device")
        if not (anchor_record.is_cuda and anchor_record.dtype == torch.float64 and anchor_record.is_contiguous() and anchor_record.numel() == _lib.ODOM_ANCHOR_WORDS):
            raise ValueError(f"{type(self).__name__}: anchor_record is float64 [{_lib.ODOM_ANCHOR_WORDS}] on the device")
        state = self.state
        self.anchor_candidates(anchor, est, i)
        self.score_refs(anchor, maps_cur, self.levels - 1, gate.score_trunc)
        self.anchor_choose(anchor, gate.score_trunc, state, record, anchor_record)
        for k, cap in enumerate(self.iters):
            level = self.levels - 1 - k
            for _ in range(cap):
                self.accumulate_anchored(level, anchor, maps_cur, state)
                self.step(level, state)
        self.score_anchored(anchor, maps_cur, state, 0)
        self.verdict(gate, state, record)
        self.anchor_update(anchor, i, record, anchor_record)
        self.anchor_promote(anchor, maps_cur)
        return state

    def chain(self, frames, gate=None, anchor=None, first=None) -> SimpleNamespace:
        """A prior-only chain over ``frames`` (depth frames; for the RGB-D odometry (depth, colour) pairs): ``est[0]`` = ``first`` ([4,4], default
        the identity), every later pose from the gated estimate alone.  ``anchor`` None: frame to frame, ``estimate_gated_device`` +
        ``pose_predict_relative``; True or an ``AnchorPolicy``: the reference ring.  ``.poses`` float32 [n,4,4], ``.prior_log`` float64 [n,16],
        ``.anchor_log`` float64 [n,8] or None, on the host; the frames' launches never wait, the call synchronises once at its end."""
        from . import pose_chain
        gate, n = OdometryGate.of(gate), len(frames)
        est = torch.zeros(max(n, 2), 4, 4, dtype=torch.float32, device=self.device)
        est[0] = torch.eye(4) if first is None else torch.as_tensor(np.asarray(first, dtype=np.float32))
        prior_log = torch.zeros(n, _lib.ODOM_GATE_WORDS, dtype=torch.float64, device=self.device)
        pose6 = torch.zeros(6, dtype=torch.float32, device=self.device)
        maps = [self.new_maps(), self.new_maps()]
        ring, anchor_log = None, None
        self._frame(frames[0], maps[0])
        if anchor is not None and anchor is not False:
            ring = self.new_anchor(AnchorPolicy.of(anchor).within(gate))
            anchor_log = torch.zeros(n, _lib.ODOM_ANCHOR_WORDS, dtype=torch.float64, device=self.device)
            self.anchor_reset(ring, maps[0], 0)
        for i in range(1, n):
            cur = self._frame(frames[i], maps[i & 1])
            if ring is None:
                state = self.estimate_gated_device(maps[(i - 1) & 1], cur, est=est, i=i, gate=gate, record=prior_log[i])
                pose_chain.pose_predict_relative(est, i, state, pose6)
            else:
                state = self.estimate_anchored_device(ring, cur, est, i, gate, prior_log[i], anchor_log[i])
                pose_chain.pose_predict_anchored(est, i, anchor_log[i], state, pose6)
        return SimpleNamespace(poses=est[:n].cpu().numpy(), prior_log=prior_log.cpu().numpy(), anchor_log=None if anchor_log is None else anchor_log.cpu().numpy())

    def _frame(self, frame, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.frame_maps(*frame, out=out) if isinstance(frame, (tuple, list)) else self.frame_maps(frame, out=out)

    def estimate_gated(self, prev, cur, candidates=None, gate=None) -> SimpleNamespace:
        """The gated estimate between two frames (a depth frame; for the RGB-D odometry a (depth, colour) pair).  ``.T`` float64 [4,4] (the
        chosen start after a FAIL), ``.passed``, ``.chosen``, ``.costs`` (one per candidate), ``.overlap`` = n_geo / n_valid and ``.rmse`` at
        level 0, ``.record`` [16], and ``read_state``'s per-level ``.status``, ``.iterations``, ``.inliers``.  This call synchronises."""
        K = 1 if candidates is None else int(np.asarray(candidates.cpu() if isinstance(candidates, torch.Tensor) else candidates).size // 16)
        state = self.estimate_gated_device(self._frame(prev), self._frame(cur), gate=gate, candidates=candidates)
        out, rec = DepthOdometryHIP.read_state(self, state), self.record.cpu().numpy()
        return SimpleNamespace(T=out.transformation, passed=bool(rec[0] == 1.0), chosen=int(rec[1]), costs=[float(c) for c in rec[2:2 + K]],
                               overlap=float(rec[7] / rec[6]) if rec[6] > 0 else 0.0, rmse=float(rec[8]), record=rec, status=out.status,
                               iterations=out.iterations, inliers=out.inliers)

    def read_state(self, state: Optional[torch.Tensor] = None) -> SimpleNamespace:
        """The state block on the host (synchronises)."""
        s = (self.state if state is None else state).cpu().numpy()
        words = s[16:16 + _lib.ODOM_LEVEL_WORDS * self.levels].reshape(self.levels, _lib.ODOM_LEVEL_WORDS)
        return SimpleNamespace(transformation=s[:16].reshape(4, 4).copy(), status=[_lib.ICP_STATUS[int(w[1])] for w in words],
                               iterations=[int(w[2]) for w in words], inliers=[int(w[3]) for w in words], rmse=[float(w[4]) for w in words])

    def estimate(self, depth_prev: torch.Tensor, depth_cur: torch.Tensor, init=None) -> SimpleNamespace:
        """``.transformation`` float64 [4,4] (current camera to previous camera), and per level (index = pyramid level, 0 the finest)
        ``.status``, ``.iterations``, ``.inliers``, ``.rmse``.  This call synchronises."""
        return self.read_state(self.estimate_device(self.frame_maps(depth_prev), self.frame_maps(depth_cur), init))


class RGBDOdometryHIP(DepthOdometryHIP):
    """The depth odometry with a photometric row per pixel (module docstring).  The maps block is the depth odometry's followed by the
    intensity block; ``init_state`` and ``step`` are the parent's (the step reads the first 29 of the 32 sums)."""

    def __init__(self, cam: Union[Dict, Sequence], levels: int = 3, iters: Sequence[int] = (10, 5, 4), max_dist: float = 0.25, jump: float = 0.15,
                 band: float = 0.1, photo_weight: float = 0.1, photo_max_diff: float = 0.3, device="cuda"):
        super().__init__(cam, levels, iters, max_dist, jump, band, device=device)
        if not (math.isfinite(photo_weight) and photo_weight >= 0.0 and photo_max_diff >= 0.0):
            raise ValueError(f"RGBDOdometryHIP: photo_weight = {photo_weight!r} must be finite and >= 0, photo_max_diff = {photo_max_diff!r} >= 0")
        self.photo = _lib.NarutoOdomPhoto(weight=float(photo_weight), max_diff=float(photo_max_diff))
        lib = _lib.load()
        self.depth_maps_bytes = self.maps_bytes
        self.maps_bytes = int(lib.naruto_odom_rgbd_maps_bytes(C.byref(self.desc)))
        ws = int(lib.naruto_odom_rgbd_workspace_bytes(C.byref(self.desc)))
        if self.maps_bytes == 0 or ws == 0:
            raise ValueError("RGBDOdometryHIP: " + lib.naruto_last_error().decode("utf-8", "replace"))
        self.workspace = _lib.workspace(ws, self.device, torch.float64)
        self.sums = torch.zeros(_lib.ODOM_RGBD_SUMS, dtype=torch.float64, device=self.device)
        # offset in floats of every level's I | gx | gy inside a maps block
        self.intensity_offsets, off = [], self.depth_maps_bytes // 4
        for h, w, _ in self.level_shapes:
            self.intensity_offsets.append(off)
            off += 3 * h * w

    def frame_maps(self, depth: torch.Tensor, color: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The RGB-D maps block of the frame: depth [H,W], colour [H,W,3] (float32 on the device): one launch."""
        depth = depth.to(self.device, torch.float32).contiguous()
        color = color.to(self.device, torch.float32).contiguous()
        if depth.numel() != self.H * self.W or color.numel() != 3 * self.H * self.W:
            raise ValueError(f"RGBDOdometryHIP: a depth frame of {tuple(depth.shape)} and a colour frame of {tuple(color.shape)}, built for {self.H} x {self.W}")
        out = self.new_maps() if out is None else out
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() * 4 == self.maps_bytes):
            raise ValueError("RGBDOdometryHIP: out must be a maps block of new_maps()")
        with _on_device(self.device):
            check(_lib.load().naruto_odom_rgbd_frame_maps(C.byref(self.desc), depth.data_ptr(), color.data_ptr(), out.data_ptr(), _stream()),
                  "naruto_odom_rgbd_frame_maps")
        return out

    @property
    def _photo_on(self) -> bool:
        return float(self.photo.weight) > 0.0

    def _photo_ref(self):
        return C.byref(self.photo)                                         # the maps are RGB-D blocks

    def level_views(self, maps: torch.Tensor, level: int):
        """(depth [h,w], vertex [h,w,3], normal [h,w,3], I [h,w], gx [h,w], gy [h,w]): views into an RGB-D maps block."""
        h, w, _ = self.level_shapes[level]
        n, off = h * w, self.intensity_offsets[level]
        return super().level_views(maps, level) + tuple(maps[off + k * n:off + (k + 1) * n].view(h, w) for k in range(3))

    def accumulate(self, level: int, maps_prev: torch.Tensor, maps_cur: torch.Tensor, state: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None):
        """The 32 sums of one evaluation.  ``rows``: float64 [pixels of the level, 4] = (geometric j or -1, r, photometric j or -1, r_I)."""
        state = self.state if state is None else state
        with _on_device(self.device):
            check(_lib.load().naruto_odom_rgbd_accumulate(C.byref(self.desc), C.byref(self.photo), int(level), maps_prev.data_ptr(), maps_cur.data_ptr(),
                                                          state.data_ptr(), self.sums.data_ptr(), self.workspace.data_ptr(),
                                                          None if rows is None else rows.data_ptr(), _stream()), "naruto_odom_rgbd_accumulate")
        return self.sums

    def read_state(self, state: Optional[torch.Tensor] = None) -> SimpleNamespace:
        """The parent's, plus the last evaluation's ``geometric_rows`` and ``photometric_rows`` read from the sums (synchronises)."""
        out = super().read_state(state)
        s = self.sums.cpu().numpy()
        out.geometric_rows, out.photometric_rows = int(s[29]), int(s[30])
        return out

    def estimate(self, depth_prev: torch.Tensor, color_prev: torch.Tensor, depth_cur: torch.Tensor, color_cur: torch.Tensor, init=None) -> SimpleNamespace:
        """As ``DepthOdometryHIP.estimate`` from two RGB-D frames.  This call synchronises."""
        return self.read_state(self.estimate_device(self.frame_maps(depth_prev, color_prev), self.frame_maps(depth_cur, color_cur), init))

"""Frame-to-model alignment on the device (csrc/naruto_sdfreg.hip; include/naruto_hip.h states the ABI): a depth frame registered to the
field's own SDF.  Every motion prior of this package is frame to frame, so nothing in a chain of them refers to the map and the chain
drifts; the map is the anchor.  The frame's depth is back-projected, the points are carried into the field's frame by the predicted pose,
and the squared signed distance the field reports there is minimised: Co-SLAM's ``tracking_pc`` idea, KinectFusion's against a TSDF.  It is
an opt-in refinement between any motion prior and the tracker (``CoSLAMNarutoHIP(track=True, model_align=...)``).  Nothing like it is in the
reference tree: PARITY UNPINNED, the contract is this text; tests/field_registration_spec.py is its numpy twin.

Convention.  The odometry's (``naruto_amd.odometry``): pixel (u, v) has direction ((u-cx)/fx, -(v-cy)/fy, -1); the current frame's vertex
map at pyramid level l is ``DepthOdometryHIP.frame_maps``'s; the state block's first 48 doubles and the level words are the odometry's.
Here ``T`` is the CAMERA-TO-FIELD POSE ITSELF, not a relative motion.  The state block has 64 doubles: the start's T follows.

One iteration at level l is five launches, nothing read back:
  1. ``points`` (k_sdfreg_points), per pixel of the level's vertex map: q = T p in fp64 as ((r0*x + r1*y) + r2*z) + t, rounded once to
     float32; x = (q - bbox_min) / (bbox_max - bbox_min) per axis in float32 without contraction (``run_network``'s normalisation); the point
     is ``valid`` iff p.z < 0 and every x component is finite and in [0, 1].  x [M,3] ((0.5, 0.5, 0.5) for an invalid point, so the query
     kernels see benign input), q [M,3] float32, valid [M] bytes;
  2. ``naruto_query_fwd`` on x: ``sdf_uncert`` only, the colour net is skipped;
  3. ``naruto_query_bwd_points`` with the constant cotangent d_raw = (0,0,0,1,0) per point, d_geo = NULL, x-points form:
     d_x [M,3] = d sdf / d x, exact fp32 in both MLP modes;
  4. ``accumulate`` (k_sdfreg_accumulate + k_sdfreg_finish), fp64 without contraction, per valid point: r = trunc * sdf and
     g = (trunc * d_x) / (bbox_max - bbox_min) per axis, ``trunc`` = ``training.trunc``: the world-space gradient in the frame's length units.
     A point is rejected unless sdf and g are finite, |sdf| < ``sdf_gate`` and g.g > 0 (the field saturates towards +-1 beyond the truncation
     band and carries no direction there).  Row J = [q x g, g], residual r, left perturbation T <- exp(xi) T: plain Gauss-Newton on the
     field's own distance, g is not normalised.  30 sums: the odometry's 29 (the 21 upper entries of J^T J, the 6 of J^T r, sum r^2, the rows)
     and the count of valid points; thread t of workgroup b takes points b*2048 + t + 256 k, 256 partial vectors fold by halves in LDS, a
     second launch folds the workgroups (the odometry's routine, csrc/naruto_odom.h): no atomics, bitwise reproducible.  ``rows``
     (optional, [M,2] doubles): the accepted flag and r;
  5. ``naruto_odom_step``, unchanged, on the first 29 sums: ``degenerate`` below 6 rows or on a small pivot (T unchanged), ``converged``
     below 1e-6 / 1e-6, the iteration caps and the done words.  A points / accumulate launch of a finished level writes nothing.

``init`` (one thread): T = est[i] (float32 -> fp64), level words 0, the start kept behind the state block.  Right after it the start is
evaluated once at the finest level used (points, query, gradient, accumulate into sums of its own).  After the level loop -- for each level
from the coarsest, cap x the five launches -- the final T is evaluated the same way, and ``verdict`` (one thread) gives PASS iff
  * the finest level is not ``degenerate``;  * rows >= ``min_overlap`` n_valid;  * rows > 0;
  * sum r^2 / rows at the final T is not above its value at the start;
  * the motion from the start satisfies |t| <= ``max_trans`` (t = the difference of the translations) and
    trace(R_start^T R) >= 1 + 2 cos(``max_rot_deg``) (the host computes that bound).
A NaN fails its comparison.  On FAIL T becomes the start.  Record, 8 doubles: verdict, n_valid, rows, start rmse, final rmse, |t|, trace,
the finest level's status; -1 where a figure is not finite.  ``commit`` (one thread): est[i] = T rounded once to float32 and
pose6_out = ``naruto_pose_log`` of the stored matrix, exactly as ``pose_predict_relative`` ends.

Defaults: the two coarsest levels of a three-level pyramid (level 0 costs a field query per pixel per iteration), 6 iterations each,
``sdf_gate`` 0.9, ``min_overlap`` 0.25, ``max_trans`` = trunc (the basin is the truncation band), ``max_rot_deg`` 4 (the study of
tools/study_model_align.py: 5 passed one lost estimate that had turned by 4.7 degrees; no converged one turned by more than 3.2).

Limits: the basin is the truncation band, so this refines a prior and does not replace one; a wall seen head on is degenerate, as for
``depth_icp``; unmapped space gives no rows and the verdict refuses the estimate; geometry only (no photometric term, no weighting by the
field's uncertainty); no second attempt after a FAIL.
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
from .odometry import DepthOdometryHIP, _intrinsics
from .ops import _on_device, _params_struct, _points_struct, _stream


@dataclass
class RegistrationGate:
    """The verdict's thresholds (module docstring).  ``max_trans`` None: ``training.trunc``."""
    min_overlap: float = 0.25
    max_trans: Optional[float] = None
    max_rot_deg: float = 4.0

    def __post_init__(self):
        vals = (self.min_overlap, self.max_rot_deg) + (() if self.max_trans is None else (self.max_trans,))
        if not (all(math.isfinite(v) for v in vals) and 0 <= self.min_overlap <= 1 and 0 <= self.max_rot_deg <= 180 and (self.max_trans is None or self.max_trans >= 0)):
            raise ValueError(f"RegistrationGate: {self!r}: min_overlap in 0 .. 1, max_rot_deg in 0 .. 180, max_trans >= 0 or None")

    @staticmethod
    def of(gate) -> "RegistrationGate":
        """None or True: the defaults; a RegistrationGate: itself."""
        if gate is None or gate is True:
            return RegistrationGate()
        if not isinstance(gate, RegistrationGate):
            raise ValueError(f"the gate is None, True or a RegistrationGate; got {gate!r}")
        return gate

    def abi(self, trunc: float):
        return _lib.NarutoSdfRegGate(max_trans=float(trunc if self.max_trans is None else self.max_trans),
                                     min_trace=1.0 + 2.0 * math.cos(math.radians(self.max_rot_deg)), min_overlap=float(self.min_overlap))


class FieldRegistrationHIP:
    def __init__(self, model, config: Dict, cam: Union[Dict, Sequence], levels: Optional[Sequence[int]] = None, iters: Optional[Sequence[int]] = None,
                 sdf_gate: float = 0.9, gate=None, pyramid_levels: int = 3, jump: float = 0.15, band: float = 0.1, device=None):
        """``model``: the field (``JointEncodingHIP``); ``config``: its config (``training.trunc``); ``cam``: the frame's H, W, fx, fy, cx, cy.
        ``levels``: the pyramid levels used, from the coarsest to the finest (default: the two coarsest of ``pyramid_levels``); ``iters``: their
        caps (default 6 each).  ``pyramid_levels``, ``jump``, ``band``: the maps block's, as ``DepthOdometryHIP``'s -- an odometry's maps block of
        the same pyramid is read as it is."""
        H, W = int(_intrinsics(cam)[0]), int(_intrinsics(cam)[1])
        pyramid_levels = int(pyramid_levels)
        if levels is None:
            usable = [l for l in range(pyramid_levels) if (H >> l) > 0 and (W >> l) > 0]
            levels = sorted(usable[-2:], reverse=True)
        self.levels = tuple(int(l) for l in levels)
        self.iters = tuple(int(k) for k in (iters if iters is not None else (6,) * len(self.levels)))
        if (not self.levels or len(self.iters) != len(self.levels) or min(self.iters) < 1 or min(self.levels) < 0 or max(self.levels) >= pyramid_levels
                or any(a <= b for a, b in zip(self.levels, self.levels[1:]))):
            raise ValueError(f"FieldRegistrationHIP: levels = {levels!r} run from the coarsest to the finest inside a pyramid of {pyramid_levels}, "
                             f"each with a cap >= 1; got iters = {iters!r}")
        if not (math.isfinite(sdf_gate) and sdf_gate > 0):
            raise ValueError(f"FieldRegistrationHIP: sdf_gate = {sdf_gate!r} must be finite and positive")
        self.model, self.config = model, config
        self.trunc = float(config["training"]["trunc"])
        self.gate = RegistrationGate.of(gate)
        device = torch.device(device) if device is not None else model.bounding_box.device
        # the pyramid and the step: an odometry object whose caps are this registration's (naruto_odom_step reads them from its desc)
        caps = [1] * pyramid_levels
        for l, cap in zip(self.levels, self.iters):
            caps[pyramid_levels - 1 - l] = cap
        self.pyramid = DepthOdometryHIP(cam, levels=pyramid_levels, iters=caps, jump=jump, band=band, device=device)
        self.device, self.odesc = self.pyramid.device, self.pyramid.desc
        bb = model.bounding_box.detach().to("cpu", torch.float32)
        n = len(self.levels)
        pad = [0] * (_lib.ODOM_MAX_LEVELS - n)
        self.desc = _lib.NarutoSdfRegDesc(trunc=self.trunc, sdf_gate=float(sdf_gate), bbox_min=(C.c_float * 3)(*[float(v) for v in bb[:, 0]]),
                                          bbox_max=(C.c_float * 3)(*[float(v) for v in bb[:, 1]]), n_levels=n,
                                          levels=(C.c_uint32 * _lib.ODOM_MAX_LEVELS)(*(list(self.levels) + pad)),
                                          iters=(C.c_uint32 * _lib.ODOM_MAX_LEVELS)(*(list(self.iters) + pad)))
        lib = _lib.load()
        ws = int(lib.naruto_sdfreg_workspace_bytes(C.byref(self.odesc)))
        if ws == 0:
            raise ValueError("FieldRegistrationHIP: " + lib.naruto_last_error().decode("utf-8", "replace"))
        self.workspace = _lib.workspace(ws, self.device, torch.float64)
        M = max(self.pixels(l) for l in self.levels)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.x, self.q, self.d_x = torch.full((M, 3), 0.5, **f32), torch.zeros(M, 3, **f32), torch.zeros(M, 3, **f32)
        self.valid = torch.zeros(M, dtype=torch.uint8, device=self.device)
        self.sdf_uncert = torch.zeros(M, 2, **f32)
        self.d_raw = torch.zeros(M, 5, **f32)
        self.d_raw[:, 3] = 1.0                                                # the constant cotangent: d sdf
        f64 = dict(dtype=torch.float64, device=self.device)
        self.sums, self.sums_start, self.sums_final = (torch.zeros(_lib.SDFREG_SUMS, **f64) for _ in range(3))
        self.pyramid.sums = self.sums                                        # naruto_odom_step reads the first 29 of the 30
        self.state = torch.zeros(_lib.SDFREG_STATE_DOUBLES, **f64)
        self.record = torch.zeros(_lib.SDFREG_RECORD, **f64)
        self._est1 = torch.zeros(1, 4, 4, **f32)
        self._pose6 = torch.zeros(6, **f32)

    def pixels(self, level: int) -> int:
        h, w, _ = self.pyramid.level_shapes[level]
        return h * w

    def _fits(self, level: int) -> int:
        """The pixels of ``level``, refused when this object's buffers (sized by the levels it was built for) cannot hold them."""
        if not 0 <= int(level) < self.pyramid.levels or self.pixels(level) > self.x.shape[0]:
            raise ValueError(f"FieldRegistrationHIP: level {level} is outside the levels {self.levels} this object was built for")
        return self.pixels(level)

    def frame_maps(self, depth: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The maps block of a depth frame [H,W]: ``DepthOdometryHIP.frame_maps`` of this registration's pyramid, one launch."""
        return self.pyramid.frame_maps(depth, out=out)

    # ------------------------------------------------------------------------------------------------ the launches
    def points(self, maps: torch.Tensor, level: int, state: Optional[torch.Tensor] = None, gated: bool = True) -> None:
        state = self.state if state is None else state
        self._fits(level)
        check(_lib.load().naruto_sdfreg_points(C.byref(self.odesc), C.byref(self.desc), int(level), 1 if gated else 0, maps.data_ptr(), state.data_ptr(),
                                               self.x.data_ptr(), self.q.data_ptr(), self.valid.data_ptr(), _stream()), "naruto_sdfreg_points")

    def query(self, level: int) -> None:
        """The field's sdf and its gradient at ``self.x``: ``naruto_query_fwd`` (sdf_uncert only) and ``naruto_query_bwd_points``."""
        lib, M = _lib.load(), self._fits(level)
        handle, ps = self.model._handle(), _params_struct({k: v.detach() for k, v in self.model._params().items()})
        pts, _ = _points_struct(self.x, None, None, None)
        check(lib.naruto_query_fwd(handle.ptr, C.byref(ps), M, C.byref(pts), None, self.sdf_uncert.data_ptr(), None, None, _stream()), "naruto_query_fwd")
        check(lib.naruto_query_bwd_points(handle.ptr, C.byref(ps), M, C.byref(pts), self.d_raw.data_ptr(), None, None, None, self.d_x.data_ptr(), None, None,
                                          0, None, _stream()), "naruto_query_bwd_points")

    def accumulate(self, level: int, sums: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
                   gated: bool = True, sdf_uncert=None, d_x=None, q=None, valid=None) -> torch.Tensor:
        sums, state = self.sums if sums is None else sums, self.state if state is None else state
        a = [self.sdf_uncert if sdf_uncert is None else sdf_uncert, self.d_x if d_x is None else d_x, self.q if q is None else q,
             self.valid if valid is None else valid]
        if min(t.shape[0] for t in a) < self.pyramid.level_shapes[int(level)][0] * self.pyramid.level_shapes[int(level)][1]:
            raise ValueError(f"FieldRegistrationHIP: an array is shorter than level {level}'s pixels")
        check(_lib.load().naruto_sdfreg_accumulate(C.byref(self.odesc), C.byref(self.desc), int(level), 1 if gated else 0, *(t.data_ptr() for t in a),
                                                   state.data_ptr(), sums.data_ptr(), self.workspace.data_ptr(), None if rows is None else rows.data_ptr(),
                                                   _stream()), "naruto_sdfreg_accumulate")
        return sums

    def _evaluate(self, maps: torch.Tensor, level: int, sums: torch.Tensor, gated: bool, rows: Optional[torch.Tensor] = None) -> None:
        self.points(maps, level, gated=gated)
        self.query(level)
        self.accumulate(level, sums, rows=rows, gated=gated)

    def iterate(self, maps: torch.Tensor, level: int) -> None:
        """One iteration at ``level`` on ``self.state``: the five launches."""
        self._evaluate(maps, level, self.sums, True)
        self.pyramid.step(level, self.state)

    def init(self, est: torch.Tensor, i: int) -> None:
        check(_lib.load().naruto_sdfreg_init(est.data_ptr(), est.shape[0], int(i), self.state.data_ptr(), _stream()), "naruto_sdfreg_init")

    def verdict(self, record: Optional[torch.Tensor] = None) -> None:
        record = self.record if record is None else record
        check(_lib.load().naruto_sdfreg_verdict(C.byref(self.desc), C.byref(self.gate.abi(self.trunc)), self.sums_start.data_ptr(), self.sums_final.data_ptr(),
                                                self.state.data_ptr(), record.data_ptr(), _stream()), "naruto_sdfreg_verdict")

    def commit(self, est: torch.Tensor, i: int, pose6_out: torch.Tensor) -> None:
        check(_lib.load().naruto_sdfreg_commit(est.data_ptr(), est.shape[0], int(i), self.state.data_ptr(), pose6_out.data_ptr(), _stream()),
              "naruto_sdfreg_commit")

    # ------------------------------------------------------------------------------------------------ the estimate
    def align_device(self, maps_cur: torch.Tensor, est: torch.Tensor, i: int, pose6_out: torch.Tensor, record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The whole alignment of frame ``i`` (module docstring): launches only.  ``maps_cur``: the frame's maps block (this registration's
        ``frame_maps`` or an odometry's of the same pyramid); ``est``: float32 [num_frames,4,4] on the device, ``est[i]`` is the start and
        receives the result (the start's bits after a FAIL); ``pose6_out``: float32 [6], its (omega, t); ``record``: float64 [8] on the device
        (default ``self.record``).  Returns the state block, owned by this object."""
        record = self.record if record is None else record
        if not (est.is_cuda and est.dtype == torch.float32 and est.is_contiguous() and est.dim() == 3 and est.shape[1:] == (4, 4) and 0 <= int(i) < est.shape[0]):
            raise ValueError("FieldRegistrationHIP: est is a contiguous float32 [num_frames,4,4] on the device and i one of its frames")
        if not (pose6_out.is_cuda and pose6_out.dtype == torch.float32 and pose6_out.is_contiguous() and pose6_out.numel() == 6):
            raise ValueError("FieldRegistrationHIP: pose6_out is float32 [6] on the device")
        if not (record.is_cuda and record.dtype == torch.float64 and record.is_contiguous() and record.numel() == _lib.SDFREG_RECORD):
            raise ValueError(f"FieldRegistrationHIP: record is float64 [{_lib.SDFREG_RECORD}] on the device")
        if not (maps_cur.is_cuda and maps_cur.dtype == torch.float32 and maps_cur.is_contiguous() and maps_cur.numel() * 4 >= self.pyramid.maps_bytes):
            raise ValueError("FieldRegistrationHIP: maps_cur is a maps block of this pyramid")
        finest = self.levels[-1]
        with _on_device(self.device), torch.no_grad():
            self.init(est, i)
            self._evaluate(maps_cur, finest, self.sums_start, False)
            for level, cap in zip(self.levels, self.iters):
                for _ in range(cap):
                    self.iterate(maps_cur, level)
            self._evaluate(maps_cur, finest, self.sums_final, False)
            self.verdict(record)
            self.commit(est, i, pose6_out)
        return self.state

    def _maps(self, frame: torch.Tensor) -> torch.Tensor:
        """A maps block as it is; a depth frame [H,W] through ``frame_maps``."""
        if frame.is_cuda and frame.dim() == 1 and frame.numel() * 4 >= self.pyramid.maps_bytes:
            return frame
        return self.frame_maps(frame)

    def read_state(self) -> SimpleNamespace:
        return self.pyramid.read_state(self.state[:_lib.ODOM_STATE_DOUBLES])

    def align(self, depth: torch.Tensor, c2w_start) -> SimpleNamespace:
        """Align a depth frame [H,W] (or a maps block) from the pose ``c2w_start`` [4,4].  ``.T`` float64 [4,4] (the start after a FAIL),
        ``.passed``, ``.record`` [8], ``.pose`` float32 [4,4] as committed, ``.pose6``, and per pyramid level ``.status``, ``.iterations``,
        ``.inliers``, ``.rmse``.  This call synchronises."""
        self._est1[0].copy_(torch.as_tensor(c2w_start).to(torch.float32).reshape(4, 4))
        self.align_device(self._maps(depth), self._est1, 0, self._pose6)
        out, rec = self.read_state(), self.record.cpu().numpy()
        return SimpleNamespace(T=out.transformation, passed=bool(rec[0] == 1.0), record=rec, pose=self._est1[0].cpu().clone(), pose6=self._pose6.cpu().clone(),
                               status=out.status, iterations=out.iterations, inliers=out.inliers, rmse=out.rmse)

    def evaluate(self, maps: torch.Tensor, T, level: int):
        """One evaluation of the pose ``T`` [4,4] (fp64 on the host) at ``level``: (sums float64 [30], rows float64 [M,2]) on the host, for tests
        and the study; ``self.x``, ``self.q``, ``self.valid``, ``self.sdf_uncert``, ``self.d_x`` keep the evaluation's arrays.  Synchronises;
        ``self.state`` is not touched."""
        maps, M = self._maps(maps), self._fits(level)
        state = torch.zeros_like(self.state)
        state[:16] = torch.from_numpy(np.asarray(T, np.float64).reshape(16).copy()).to(self.device)
        rows, sums = torch.zeros(M, 2, dtype=torch.float64, device=self.device), torch.zeros_like(self.sums)
        with _on_device(self.device), torch.no_grad():
            self.points(maps, level, state, gated=False)
            self.query(level)
            self.accumulate(level, sums, state, rows, gated=False)
        return sums.cpu().numpy(), rows.cpu().numpy()

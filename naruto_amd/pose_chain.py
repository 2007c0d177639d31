"""Co-SLAM's pose chain on the device (csrc/naruto_posechain.hip; include/naruto_hip.h restates the contract): the arithmetic a tracked
run does on ``est_c2w_data`` / ``est_c2w_data_rel`` between the tracker and ``global_BA``, without a trip to the host.

``est`` / ``rel`` are the [num_frames,4,4] float32 device tensors behind ``slam.DevicePoses``.  Every function launches on torch's
current stream, allocates only the output it returns when none is given, and never synchronises.

  * ``pose_log(c2w)``                                   [P,4,4] -> (omega, t) [P,6]: ``tracking.matrices_to_pose6`` on the device
  * ``pose_predict(est, i, const_speed, pose6_out)``    ``predict_current_pose`` into ``est[i]`` and the tracker's ``pose_init``
  * ``pose_predict_relative(est, i, state_T, pose6_out)``   ``est[i] = est[i-1] @ T`` from a depth-odometry state block, and ``pose_init``
  * ``pose_predict_anchored(est, i, anchor_record, state_T, pose6_out)``   ``est[i] = est[f] @ T``, f the anchored odometry's reference frame
  * ``pose_commit(est, rel, i, keyframe_every, c2w)``   the tracked pose into ``est[i]``; ``rel[i]`` for a frame that is no keyframe
  * ``pose_scatter(est, refined, P, keyframe_every, cur_id, optim_cur)``   ``global_BA``'s write-back (coslam.py:401-407)
  * ``pose_resolve(est, rel, n, keyframe_every)``       ``convert_relative_pose``: [n,4,4], every frame relative to its refined keyframe
  * ``pose_log_host(c2w)``                              ``pose_log``'s own code run on the CPU (no GPU needed)
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import check
from .ops import _on_device, _stream


def _mats(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 2 and tuple(t.shape[-2:]) == (4, 4)):
        raise ValueError(f"pose_chain: {name} must be a contiguous float32 [..,4,4] tensor on the GPU")
    return t


def _vec6(t: torch.Tensor, name: str, rows: int) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 6 * rows):
        raise ValueError(f"pose_chain: {name} must be a contiguous float32 tensor of {rows} x 6 on the GPU")
    return t


def pose_log(c2w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(omega, t) [P,6] float32 of the camera-to-world matrices ``c2w`` [P,4,4] (or [4,4])."""
    c2w = _mats(c2w, "c2w")
    P = c2w.numel() // 16
    if out is None:
        out = torch.empty(P, 6, dtype=torch.float32, device=c2w.device)
    _vec6(out, "out", P)
    with _on_device(c2w.device):
        check(_lib.load().naruto_pose_log(P, c2w.data_ptr(), out.data_ptr(), _stream()), "naruto_pose_log")
    return out


def pose_predict(est: torch.Tensor, i: int, const_speed: bool, pose6_out: torch.Tensor) -> None:
    """``est[i]`` <- the constant-speed prediction (``est[i-1]`` for ``i == 1`` or without ``const_speed``); ``pose6_out`` [6] <- its
    (omega, t), e.g. ``TrackerHIP.pose_init``."""
    est = _mats(est, "est")
    _vec6(pose6_out, "pose6_out", 1)
    with _on_device(est.device):
        check(_lib.load().naruto_pose_predict(est.data_ptr(), est.shape[0], int(i), 1 if const_speed else 0, pose6_out.data_ptr(), _stream()),
              "naruto_pose_predict")


def pose_predict_relative(est: torch.Tensor, i: int, state_T: torch.Tensor, pose6_out: torch.Tensor) -> None:
    """``est[i]`` <- ``est[i-1] @ T`` with ``T`` the 16 float64 at the head of ``state_T`` (a ``DepthOdometryHIP`` state block on the device);
    ``pose6_out`` [6] <- its (omega, t), exactly as ``pose_predict`` ends."""
    est = _mats(est, "est")
    _vec6(pose6_out, "pose6_out", 1)
    if not (isinstance(state_T, torch.Tensor) and state_T.is_cuda and state_T.dtype == torch.float64 and state_T.is_contiguous() and state_T.numel() >= 16):
        raise ValueError("pose_chain: state_T must be a contiguous float64 tensor of at least 16 elements on the GPU")
    with _on_device(est.device):
        check(_lib.load().naruto_pose_predict_relative(est.data_ptr(), est.shape[0], int(i), state_T.data_ptr(), pose6_out.data_ptr(), _stream()),
              "naruto_pose_predict_relative")


def pose_predict_anchored(est: torch.Tensor, i: int, anchor_record: torch.Tensor, state_T: torch.Tensor, pose6_out: torch.Tensor) -> None:
    """``est[i]`` <- ``est[f] @ T`` with ``f`` the reference frame the anchored odometry chose, read ON THE DEVICE from
    ``anchor_record[1]`` (float64 [8], ``odometry.estimate_anchored_device``'s), and ``T`` the head of ``state_T``; ``pose6_out`` as
    ``pose_predict_relative`` ends."""
    est = _mats(est, "est")
    _vec6(pose6_out, "pose6_out", 1)
    for t, name, n in ((state_T, "state_T", 16), (anchor_record, "anchor_record", _lib.ODOM_ANCHOR_WORDS)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() >= n):
            raise ValueError(f"pose_chain: {name} must be a contiguous float64 tensor of at least {n} elements on the GPU")
    with _on_device(est.device):
        check(_lib.load().naruto_pose_predict_anchored(est.data_ptr(), est.shape[0], int(i), anchor_record.data_ptr(), state_T.data_ptr(),
                                                       pose6_out.data_ptr(), _stream()), "naruto_pose_predict_anchored")


def pose_commit(est: torch.Tensor, rel: torch.Tensor, i: int, keyframe_every: int, c2w: torch.Tensor) -> None:
    """``est[i]`` <- ``c2w`` [4,4]; for a frame that is no keyframe ``rel[i]`` <- ``est[i] @ inv(est[kf(i)])``."""
    est, rel, c2w = _mats(est, "est"), _mats(rel, "rel"), _mats(c2w, "c2w")
    if rel.shape != est.shape or c2w.numel() != 16:
        raise ValueError("pose_chain: rel must have est's shape and c2w be one [4,4] matrix")
    with _on_device(est.device):
        check(_lib.load().naruto_pose_commit(est.data_ptr(), rel.data_ptr(), est.shape[0], int(i), int(keyframe_every), c2w.data_ptr(), _stream()),
              "naruto_pose_commit")


def pose_scatter(est: torch.Tensor, refined: torch.Tensor, P: int, keyframe_every: int, cur_id: int, optim_cur: bool) -> None:
    """``est[k * keyframe_every]`` <- ``refined[k]`` for k = 1 .. P-2, ``est[cur_id]`` <- ``refined[P-1]`` iff ``optim_cur``."""
    est, refined = _mats(est, "est"), _mats(refined, "refined")
    if not 0 < int(P) <= refined.shape[0]:
        raise ValueError(f"pose_chain: P = {P} poses out of the {refined.shape[0]} given")
    with _on_device(est.device):
        check(_lib.load().naruto_pose_scatter(est.data_ptr(), est.shape[0], refined.data_ptr(), int(P), int(keyframe_every), int(cur_id),
                                              1 if optim_cur else 0, _stream()), "naruto_pose_scatter")


def pose_resolve(est: torch.Tensor, rel: torch.Tensor, n: int, keyframe_every: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n,4,4]: ``est[i]`` for a keyframe, ``rel[i] @ est[kf(i)]`` otherwise."""
    est, rel = _mats(est, "est"), _mats(rel, "rel")
    n = int(n)
    if not (0 < n <= est.shape[0] and rel.shape == est.shape):
        raise ValueError(f"pose_chain: n = {n} frames out of est's {est.shape[0]}; rel must have est's shape")
    if out is None:
        out = torch.empty(n, 4, 4, dtype=torch.float32, device=est.device)
    if _mats(out, "out").numel() != 16 * n:
        raise ValueError(f"pose_chain: out must be [{n},4,4]")
    with _on_device(est.device):
        check(_lib.load().naruto_pose_resolve(est.data_ptr(), rel.data_ptr(), n, int(keyframe_every), out.data_ptr(), _stream()), "naruto_pose_resolve")
    return out


def pose_log_host(c2w: torch.Tensor) -> torch.Tensor:
    """``pose_log`` by the kernel's own code on the CPU (``naruto_debug_pose_log``): [P,4,4] float32 host -> [P,6] float32."""
    a = torch.as_tensor(c2w).detach().to("cpu", torch.float32).reshape(-1, 4, 4).contiguous()
    out = torch.zeros(a.shape[0], 6, dtype=torch.float32)
    check(_lib.load().naruto_debug_pose_log(a.shape[0], a.data_ptr(), out.data_ptr()), "naruto_debug_pose_log")
    return out

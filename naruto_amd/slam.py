"""CoSLAMNarutoHIP: the object the reference's run loop drives (``CoSLAMNaruto``, reference src/slam/coslam/coslam.py), assembled from
the device pieces of this package -- ``MappingTrainer`` / ``FusedBA`` (mapping iteration and ``global_BA`` loop), ``KeyFrameStoreHIP``,
``ActiveRaySamplerHIP``, ``get_map_volumes``, ``extract_mesh`` -- with a frame going from the simulator into the mapping loop
without a detour through torch expressions or the host (``naruto_frame_ingest`` / ``naruto_keyframe_row``).  It needs neither
``mmengine`` nor the Co-SLAM third-party tree.

PARITY UNPINNED.  ``CoSLAMNaruto`` inherits from Co-SLAM's ``CoSLAM`` and uses its ``get_camera_rays``, ``KeyFrameDatabase`` and
``select_samples``, none of which is in the reference tree.  What this class does is therefore restated here:

  * Camera rays (``init_cam_rays``, coslam.py:122-144): H, W, fx, fy, cx, cy are the config's values FLOOR-divided by
    ``data.downsample`` -- the reference's ``//``, which also drops the half pixel of cx = 599.5 -- and ``rays_d`` [H,W,3] holds
    ((i - cx)/fx, -(j - cy)/fy, -1) for column i, row j: x right, y up, looking along -z, this package's convention throughout.
  * ``online_recon_step(i, color, depth, c2w)`` (coslam.py:537-633), in this order:
      1. the mesh is saved at ``mesh.voxel_eval`` when ``i % mesh.vis == 0``;
      2. frame 0: ``est_c2w_data[0] = c2w``; ``mapping.first_iters`` iterations of first-frame mapping (coslam.py:197-219:
         ``mapping.sample`` distinct pixels out of all H*W per iteration, no smoothness term, the network's Adam every iteration, the
         uncertainty grid's gradient zeroed once, stepped once at the end and kept); frame 0 becomes a keyframe; map volumes;
      3. any other frame: ``est_c2w_data[i] = c2w`` (``tracking.disable``), or the frame is tracked (``track=True``; see below);
      4. when ``i % mapping.map_every == 0``: ``global_BA`` over the keyframes stored BEFORE this frame, with the poses
         ``est_c2w_data[0, keyframe_every, ... < i]`` and the current one last (coslam.py:259-267), AND THEN the map volumes;
      5. when ``i % mapping.keyframe_every == 0``: the frame becomes a keyframe (``mapping.filter_depth`` as configured);
      6. with active rays, the cached uncertainty volume becomes the new one.
    It returns None, or [uncert_vol, sdf_vol] when step 2 or 4 made new ones.
  * The random draws (keyframe pixels, batch rays, depth jitter) are this package's keyed streams, not Python's ``random``: the drawn
    sets differ from the reference's by construction, their distribution does not (``keyframe_store``, ``ba_loop``).

What differs on purpose:

  * the volumes come back as float32 DEVICE tensors [X,Y,Z] -- views of one buffer this object owns and OVERWRITES at the next mapped
    frame (clone them to keep them).  ``NarutoPlannerHIP.main`` and ``ActiveRaySamplerHIP.set_volume`` take them as they are;
  * the keyframe store holds ``num_frames // keyframe_every + 1`` keyframes -- sized by the run, not by the dataset placeholder of
    20 000 frames the reference sizes it by (4.6 GB at 1200 x 680);
  * ``est_c2w_data`` is indexable by frame id like the reference's dict but backed by one [num_frames,4,4] device tensor, so the
    keyframe poses of a ``global_BA`` call are a strided slice of it;
  * a frame that neither maps nor becomes a keyframe launches nothing.  A mapped frame waits once for the host: the 8-byte count of
    valid-depth pixels, which sizes the current-frame draw (the reference filters on the host at the same place, coslam.py:322-325).

CAMERA TRACKING (``CoSLAMNarutoHIP(..., track=True)``; the reference's ``tracking.disable: False`` branch, coslam.py:595-602, 264-281,
378-407; Co-SLAM's ``predict_current_pose``, ``tracking_render`` and ``convert_relative_pose`` are not in the reference tree: parity
unpinned, restated in ``naruto_amd.tracking`` and ``naruto_amd.pose_chain``).  The ``c2w`` argument is used for frame 0 only.  Every
other frame i, in the reference's order:

  1. ``pose_predict``: ``est[i]`` <- the constant-speed prediction (``tracking.const_speed``), and its (omega, t) into the tracker;
  2. ``TrackerHIP.track_device``: the frame into the tracker's buffers, one replay of its captured call;
  3. ``pose_commit``: ``est[i]`` <- the tracked pose, ``rel[i] = est[i] @ inv(est[kf(i)])`` for a frame that is no keyframe;
  4. on a mapped frame: ``global_BA`` refining the keyframe poses (``FusedBA(optimize_poses=True)``, the initial (omega, t) from
     ``naruto_pose_log`` on the device), ``pose_scatter`` writing ``ba.poses`` back to ``est`` (coslam.py:401-407), the map volumes;
  5. the keyframe add.

All pose arithmetic runs on the device (csrc/naruto_posechain.hip): a tracked frame that does not map never waits for the host, a
mapped one waits once, for the same 8-byte count as without tracking.  ``resolved_poses()`` gives every frame's pose relative to its
(refined) keyframe; ``save_ckpt`` writes the raw ``pose`` / ``pose_rel`` as the reference does.  The tracker is captured once, at the end
of frame 0, and keeps its own random word (derived from ``seed``).  ``track=False`` is the object without any of this, launch for launch.

MOTION PRIOR (``motion_prior="const_speed"`` | ``"depth_icp"`` | ``"rgbd_icp"``, with ``track=True`` only).  ``"const_speed"``, the default, is step 1 as
written.  With ``"depth_icp"`` the prediction comes from the two depth frames themselves (``naruto_amd.odometry.DepthOdometryHIP``): frame
0 makes its maps; every frame i > 0 makes its maps, runs the frame-to-frame estimate from the last relative motion
``inv(est[i-2]) @ est[i-1]`` (``tracking.const_speed`` and i > 1; the identity otherwise), and ``pose_predict_relative`` stands in the place
of ``pose_predict``: ``est[i] = est[i-1] @ T``.  When every level is degenerate T is still that initial motion -- decided on the device;
the estimate is a fixed sequence of launches and adds no wait for the host.  ``odometry.state`` keeps the last estimate's state block.
``"rgbd_icp"`` is the same step with ``naruto_amd.odometry.RGBDOdometryHIP``: the frame's colour image goes into the maps as well, and every
pixel adds a photometric row, which pins the motions a bare wall leaves free for the depth rows; launch for launch the same sequence.

PRIOR GATE (``prior_gate=None`` | ``True`` | ``odometry.OdometryGate``, with an odometry prior only; ``None`` is the step above, launch for
launch).  The estimate starts from the cheaper of two starts -- the identity and the last relative motion, scored on the device at the
coarsest level -- and after the level loop four checks at level 0 give a verdict (``naruto_amd.odometry``); a FAIL hands the tracker the
chosen start instead of the lost estimate.  Frame i's record goes into ``prior_log[i]`` ([num_frames,16] float64 on the device: verdict,
chosen start, costs, overlap, rmse ...); six launches more per frame, still nothing read back.

PRIOR ANCHOR (``prior_anchor=None`` | ``True`` | ``odometry.AnchorPolicy``, with an odometry prior and ``prior_gate``; ``None`` is the step
above, launch for launch).  The gated prior composes every estimate onto the frame before, so every estimate's bias stays in the pose.
With ``prior_anchor`` the frame is registered to one of a ring of reference frames kept on the device -- the cheapest of all (slot, start)
pairs at the coarsest level -- and ``pose_predict_anchored`` writes ``est[i] = est[reference] @ T``; a reference's pose is ``est`` as it stands,
so the tracker's result and ``global_BA``'s write-back reach it.  A frame becomes a reference when it has moved away from the one it was
registered to, or after two refusals in a row (``naruto_amd.odometry``).  Frame i's anchor record goes into ``anchor_log[i]`` ([num_frames,8]
float64 on the device).  Launches only, nothing read back; ``model_align`` reads the current frame's maps as before.

MODEL ALIGNMENT (``model_align=None`` | ``True`` | ``registration.RegistrationGate``, with ``track=True`` and any ``motion_prior``; ``None`` is
the step above, launch for launch and bit for bit).  Every prior above is frame to frame, so the chain drifts; with ``model_align`` the
predicted ``est[i]`` is registered to the field's own SDF (``naruto_amd.registration.FieldRegistrationHIP.align_device``: the frame's depth
back-projected, Gauss-Newton on the signed distance the field reports) after ``pose_predict`` / ``pose_predict_relative`` and before
``track_device``; it rewrites ``est[i]`` and ``tracker.pose_init`` on the device, or leaves the prediction's bits when its verdict is FAIL.
Frame i's record goes into ``align_log[i]`` ([num_frames,8] float64 on the device).  The odometry's current maps are reused when an
odometry prior is on; otherwise the frame's maps are made here (one launch).  Launches only: a tracked frame still never waits for the host.

A config with ``tracking.disable: False`` and no ``track=True`` is refused (``NotImplementedError``) before the library is touched:
tracking is switched on by the keyword, whatever ``tracking.disable`` says.  Out of scope: ``tracking.iter_point > 0`` (``tracking_pc``),
other ``training.rot_rep`` (both refused by ``tracking.tracking_settings``), data-parallel pose refinement.
"""

from __future__ import annotations

import json
import os
from typing import Dict, Iterator, List, Optional

import torch

from .active_ray_sampler import ActiveRaySamplerHIP
from .ba_loop import FusedBA
from .capture import no_collection
from .field import _map_lattice, get_map_volumes
from .keyframe_store import KeyFrameStoreHIP, frame_ingest
from .mesh import extract_mesh
from .pose_chain import pose_commit, pose_log, pose_predict, pose_predict_anchored, pose_predict_relative, pose_resolve, pose_scatter
from .trainer import MappingTrainer


def step_schedule(i: int, config: Dict) -> Dict[str, bool]:
    """What ``online_recon_step`` does at frame ``i`` (coslam.py:571, 579, 607, 622): ``mesh`` saved, ``first`` frame mapping, ``map``
    (``global_BA`` + volumes), ``keyframe`` added, ``volumes`` returned."""
    mp = config["mapping"]
    first = i == 0
    mapped = (not first) and i % int(mp["map_every"]) == 0
    return {"mesh": i % int(config["mesh"]["vis"]) == 0, "first": first, "map": mapped,
            "keyframe": first or i % int(mp["keyframe_every"]) == 0, "volumes": first or mapped}


def camera_rays(H: int, W: int, fx: float, fy: float, cx: float, cy: float) -> torch.Tensor:
    """[H,W,3] camera-frame ray table ((i - cx)/fx, -(j - cy)/fy, -1), float32 (module docstring)."""
    i = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    j = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    return torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones(H, W)], -1).contiguous()


class DevicePoses:
    """``est_c2w_data``: frame id -> [4,4], as the reference's dict, over one [num_frames,4,4] float32 device tensor (``tensor``)."""

    def __init__(self, num_frames: int, device):
        self.tensor = torch.zeros(int(num_frames), 4, 4, dtype=torch.float32, device=device)
        self._have = [False] * int(num_frames)

    def __setitem__(self, i: int, c2w) -> None:
        self.tensor[i].copy_(torch.as_tensor(c2w).to(torch.float32).reshape(4, 4), non_blocking=True)
        self._have[i] = True

    def __getitem__(self, i: int) -> torch.Tensor:
        if not self._have[i]:
            raise KeyError(i)
        return self.tensor[i]

    def __contains__(self, i) -> bool:
        return isinstance(i, int) and 0 <= i < len(self._have) and self._have[i]

    def __len__(self) -> int:
        return sum(self._have)

    def mark(self, i: int) -> None:
        """Row ``i`` of ``tensor`` was written on the device (``naruto_amd.pose_chain``): it counts as set."""
        self._have[int(i)] = True

    def keys(self) -> Iterator[int]:
        return (i for i, h in enumerate(self._have) if h)

    def as_dict(self) -> Dict[int, torch.Tensor]:
        """frame id -> [4,4] on the host (one copy): what ``save_ckpt`` writes and ``culling.poses_from_checkpoint`` reads."""
        host = self.tensor.cpu()
        return {i: host[i].clone() for i in self.keys()}


class CoSLAMNarutoHIP:
    def __init__(self, config: Dict, voxel_size: float = 0.1, active_ray: Optional[bool] = None, act_ray_num_uncert_sample: int = 500,
                 act_ray_oversample_mul: int = 4, num_frames: int = 2000, seed: Optional[int] = 0, result_dir: Optional[str] = None, device="cuda",
                 track: bool = False, motion_prior: Optional[str] = None, prior_gate=None, model_align=None, prior_anchor=None):
        """``config``: a Co-SLAM config (``naruto_amd.config.load_config``); it is kept and, as in the reference's ``override_config``,
        ``mapping.active_ray`` is overwritten when ``active_ray`` is given.  ``num_frames``: the length of the run (sizes the keyframe store
        and the pose tensor).  ``seed``: keys the keyframe store's draws and, through ``torch.manual_seed`` (None: left alone), the
        network's initial values and the trainer's in-kernel random streams.  ``result_dir``: meshes and checkpoints go under
        ``<result_dir>/coslam`` (None: ``save_*`` need an explicit directory).  ``track``: estimate the camera poses during the run
        (module docstring) with ``tracking_settings(config)``, whatever ``tracking.disable`` says.  ``motion_prior``: where a tracked
        frame's initial pose comes from, ``"const_speed"`` (the default), ``"depth_icp"`` or ``"rgbd_icp"`` (module docstring); needs ``track=True``.
        ``prior_gate``: None (today's step, launch for launch), True or an ``odometry.OdometryGate``: the odometry prior scores its two starts
        and judges its estimate (module docstring); needs an odometry prior.  ``model_align``: None (today's step, launch for launch), True or a
        ``registration.RegistrationGate``: every tracked frame's predicted pose is registered to the field's SDF before the tracker takes it
        (module docstring); needs ``track=True``, works with every ``motion_prior``.  ``prior_anchor``: None (today's step, launch for launch),
        True or an ``odometry.AnchorPolicy``: the gated odometry prior registers every frame to one of a ring of reference frames kept on the
        device instead of the frame before (module docstring); needs an odometry prior and ``prior_gate``."""
        tk = config.get("tracking") or {}
        self.track = bool(track)
        if motion_prior is not None and motion_prior not in ("const_speed", "depth_icp", "rgbd_icp"):
            raise ValueError(f"CoSLAMNarutoHIP: motion_prior = {motion_prior!r}; 'const_speed', 'depth_icp' or 'rgbd_icp'")
        if motion_prior is not None and not self.track:
            raise ValueError("CoSLAMNarutoHIP: motion_prior is the tracker's initial pose and needs track=True")
        self.motion_prior = motion_prior or "const_speed"
        if model_align is not None and model_align is not False and not self.track:
            raise ValueError("CoSLAMNarutoHIP: model_align refines the tracker's initial pose and needs track=True")
        if prior_gate is not None and prior_gate is not False and self.motion_prior not in ("depth_icp", "rgbd_icp"):
            raise ValueError("CoSLAMNarutoHIP: prior_gate judges the odometry prior and needs motion_prior='depth_icp' or 'rgbd_icp'")
        if prior_anchor is not None and prior_anchor is not False and (self.motion_prior not in ("depth_icp", "rgbd_icp") or prior_gate is None or prior_gate is False):
            raise ValueError("CoSLAMNarutoHIP: prior_anchor keeps reference frames for the gated odometry prior and needs motion_prior='depth_icp' or "
                             "'rgbd_icp' and prior_gate")
        if not self.track and not bool(tk.get("disable", True)):
            raise NotImplementedError("CoSLAMNarutoHIP: tracking.disable: False asks for camera tracking and pose refinement during the run; they are "
                                      "switched on by the keyword track=True (naruto_amd.tracking.TrackerHIP, FusedBA(optimize_poses=True)), not by the config")
        self.tracking = None
        if self.track:
            from .tracking import tracking_settings
            self.tracking = tracking_settings(config)          # refuses iter_point > 0 and other rot_rep, before anything is built
        self.config = config
        if active_ray is not None:
            config["mapping"]["active_ray"] = bool(active_ray)
        self.device = torch.device(device)
        self.voxel_size = float(voxel_size)
        self.result_dir = result_dir
        self.step = 0
        self.num_frames = int(num_frames)
        mp, cam, ds = config["mapping"], config["cam"], config["data"]["downsample"]
        self.H, self.W = cam["H"] // ds, cam["W"] // ds
        self.fx, self.fy, self.cx, self.cy = cam["fx"] // ds, cam["fy"] // ds, cam["cx"] // ds, cam["cy"] // ds
        self.rays_d = camera_rays(self.H, self.W, self.fx, self.fy, self.cx, self.cy).to(self.device)
        self.bounding_box = torch.tensor(mp["bound"], dtype=torch.float32, device=self.device)
        self.marching_cube_bound = torch.tensor(mp["marching_cubes_bound"], dtype=torch.float32, device=self.device)
        self.est_c2w_data = DevicePoses(self.num_frames, self.device)
        self.est_c2w_data_rel = DevicePoses(self.num_frames, self.device)
        if seed is not None:
            torch.manual_seed(int(seed))
        self.trainer = MappingTrainer(config, self.bounding_box, self.device, uncert_voxel=self.voxel_size, fused_adam=True)
        self.model = self.trainer.model
        self.num_rays_to_save = int(self.H * self.W * mp["n_pixels"])
        num_kf = self.num_frames // int(mp["keyframe_every"]) + 1
        self.keyframeDatabase = KeyFrameStoreHIP(config, self.H, self.W, num_kf, self.num_rays_to_save, self.device, seed=int(seed or 0))
        self.active_ray_sampler = None
        if mp.get("active_ray", False):
            if not 0 < int(act_ray_num_uncert_sample) <= int(mp["sample"]):
                raise ValueError(f"CoSLAMNarutoHIP: act_ray_num_uncert_sample = {act_ray_num_uncert_sample} active rays do not fit a batch of "
                                 f"mapping.sample = {mp['sample']} rays")
            self.active_ray_sampler = ActiveRaySamplerHIP(config=config, num_uncert_sample=act_ray_num_uncert_sample, oversample_mul=act_ray_oversample_mul)
        self.ba = FusedBA(self.trainer, self.keyframeDatabase, self.active_ray_sampler, max_poses=num_kf + 1, optimize_poses=True if self.track else None)
        self.tracker = None
        if self.track:
            from .tracking import TrackerHIP
            # the tracker's own random word: the seed's, moved off the keyframe store's and the trainer's streams
            self.tracker = TrackerHIP(self.model, config, self.H, self.W, device=self.device, rng_seed=(int(seed or 0) * 0x9E3779B1 + 0x7F4A7C15) % (1 << 62))
        self.odometry = None
        if self.motion_prior == "depth_icp":
            from .odometry import DepthOdometryHIP
            self.odometry = DepthOdometryHIP((self.H, self.W, self.fx, self.fy, self.cx, self.cy), device=self.device)
            self._odom_maps = [self.odometry.new_maps(), self.odometry.new_maps()]          # frame i's maps live in [i & 1]
        elif self.motion_prior == "rgbd_icp":
            from .odometry import RGBDOdometryHIP
            self.odometry = RGBDOdometryHIP((self.H, self.W, self.fx, self.fy, self.cx, self.cy), device=self.device)
            self._odom_maps = [self.odometry.new_maps(), self.odometry.new_maps()]
        self.prior_gate, self.prior_log = None, None
        if prior_gate is not None and prior_gate is not False:
            from .odometry import OdometryGate
            self.prior_gate = OdometryGate.of(prior_gate)
            self.prior_log = torch.zeros(self.num_frames, 16, dtype=torch.float64, device=self.device)     # frame i's record (odometry.py)
        self.prior_anchor, self.anchor_log = None, None
        if prior_anchor is not None and prior_anchor is not False:
            from .odometry import AnchorPolicy
            self.prior_anchor = self.odometry.new_anchor(AnchorPolicy.of(prior_anchor).within(self.prior_gate))
            self.anchor_log = torch.zeros(self.num_frames, 8, dtype=torch.float64, device=self.device)     # frame i's anchor record (odometry.py)
        self.aligner, self.align_log = None, None
        if model_align is not None and model_align is not False:
            from .registration import FieldRegistrationHIP, RegistrationGate
            self.aligner = FieldRegistrationHIP(self.model, config, (self.H, self.W, self.fx, self.fy, self.cx, self.cy), gate=RegistrationGate.of(model_align),
                                                device=self.device)
            self._align_maps = None if self.odometry is not None else self.aligner.pyramid.new_maps()    # an odometry prior's maps are read as they are
            self.align_log = torch.zeros(self.num_frames, 8, dtype=torch.float64, device=self.device)      # frame i's record (registration.py)
        self.cached_uncert = None
        self.filter_depth = bool(mp.get("filter_depth", False))
        self._n_valid = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._n_valid_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self._n_valid_event = torch.cuda.Event()
        lattice = _map_lattice(self.bounding_box, self.voxel_size)
        self._vol_shape = tuple(lattice.shape[:-1])
        self._vols = torch.zeros(2, *self._vol_shape, dtype=torch.float32, device=self.device)
        if result_dir is not None:
            os.makedirs(os.path.join(result_dir, "coslam"), exist_ok=True)
            with open(os.path.join(result_dir, "coslam", "config.json"), "w", encoding="utf-8") as fh:
                fh.write(json.dumps(config, indent=4))

    # ---------------------------------------------------------------------------------------------
    def update_step(self, step: int) -> None:
        self.step = int(step)

    def _ingest(self, color: torch.Tensor, depth: torch.Tensor) -> None:
        """The frame into ``FusedBA.current`` ([H*W,7]) and its valid-depth count into the device word: one launch."""
        color = color.to(self.device, torch.float32).contiguous()
        depth = depth.to(self.device, torch.float32).contiguous()
        frame_ingest(self.rays_d, color, depth, float(self.config["cam"]["depth_trunc"]), self.ba.current, self._n_valid)

    def _read_n_valid(self) -> int:
        """The step's one wait for the host: 8 bytes through pinned memory."""
        self._n_valid_host.copy_(self._n_valid, non_blocking=True)
        self._n_valid_event.record(torch.cuda.current_stream(self.device))
        self._n_valid_event.synchronize()
        return int(self._n_valid_host[0])

    def _capture_tracker(self, color: torch.Tensor, depth: torch.Tensor) -> None:
        """End of frame 0: the tracker's call recorded as one graph, warmed up on frame 0 itself from its own pose (the warm-up and the
        capture put the tracker's random word back; ``est`` is not touched)."""
        tr = self.tracker
        with torch.no_grad():
            tr.direction.copy_(self.rays_d)
            tr.rgb.copy_(color.to(self.device, torch.float32))
            tr.depth.copy_(depth.to(self.device, torch.float32))
        pose_log(self.est_c2w_data.tensor[0], out=tr.pose_init)
        with no_collection():
            tr.capture()

    def _odom_frame_maps(self, color: torch.Tensor, depth: torch.Tensor, out: torch.Tensor) -> None:
        """The frame's odometry maps into ``out``: one launch; the RGB-D odometry takes the colour frame too."""
        if self.motion_prior == "rgbd_icp":
            self.odometry.frame_maps(depth, color, out=out)
        else:
            self.odometry.frame_maps(depth, out=out)

    def _track(self, i: int, color: torch.Tensor, depth: torch.Tensor, every: int):
        """Frame ``i > 0`` of a tracked run: predict, track, commit (module docstring) -- launches only.  Returns the frame as the
        float32 device tensors the tracker took."""
        color = color.to(self.device, torch.float32).contiguous()
        depth = depth.to(self.device, torch.float32).contiguous()
        est, rel = self.est_c2w_data, self.est_c2w_data_rel
        if (i - 1) not in est or (i % every != 0 and (i // every) * every not in est):
            raise KeyError(f"CoSLAMNarutoHIP: frame {i} is tracked from frame {i - 1} (and stored relative to keyframe {(i // every) * every}); "
                           "step the frames in order")
        if self.odometry is not None:
            od, cur = self.odometry, self._odom_maps[i & 1]
            self._odom_frame_maps(color, depth, cur)
            if self.prior_anchor is not None:
                state = od.estimate_anchored_device(self.prior_anchor, cur, est.tensor, i, self.prior_gate, self.prior_log[i], self.anchor_log[i])
                pose_predict_anchored(est.tensor, i, self.anchor_log[i], state, self.tracker.pose_init)
            elif self.prior_gate is not None:
                state = od.estimate_gated_device(self._odom_maps[(i - 1) & 1], cur, est=est.tensor, i=i, gate=self.prior_gate, record=self.prior_log[i])
            else:
                state = od.init_state(est=est.tensor, i=i, const_speed=bool(self.tracking["const_speed"]))
                od.run_levels(self._odom_maps[(i - 1) & 1], cur, state)
            if self.prior_anchor is None:
                pose_predict_relative(est.tensor, i, state, self.tracker.pose_init)
        else:
            pose_predict(est.tensor, i, bool(self.tracking["const_speed"]), self.tracker.pose_init)
        if self.aligner is not None:
            maps = self._odom_maps[i & 1] if self.odometry is not None else self.aligner.frame_maps(depth, out=self._align_maps)
            self.aligner.align_device(maps, est.tensor, i, self.tracker.pose_init, record=self.align_log[i])
        tracked = self.tracker.track_device(self.rays_d, color, depth)
        pose_commit(est.tensor, rel.tensor, i, every, tracked)
        est.mark(i)
        if i % every != 0:
            rel.mark(i)
        return color, depth

    def resolved_poses(self) -> torch.Tensor:
        """Co-SLAM's ``convert_relative_pose`` over the frames stepped so far, [n,4,4] float32 on the device: a keyframe's pose as it
        stands (refined by the ``global_BA`` calls since), any other frame's relative pose applied to its keyframe's
        (``naruto_pose_resolve``).  Without tracking: the poses given."""
        n = max((k for k in self.est_c2w_data.keys()), default=-1) + 1
        if n == 0:
            return torch.zeros(0, 4, 4, dtype=torch.float32, device=self.device)
        if not self.track:
            return self.est_c2w_data.tensor[:n].clone()
        return pose_resolve(self.est_c2w_data.tensor, self.est_c2w_data_rel.tensor, n, int(self.config["mapping"]["keyframe_every"]))

    def _volumes(self) -> List[torch.Tensor]:
        return get_map_volumes(self.model.query_sdf, self.bounding_box, self.voxel_size, to_host=False, out=self._vols)

    def online_recon_step(self, i: int, color: torch.Tensor, depth: torch.Tensor, c2w: torch.Tensor) -> Optional[List[torch.Tensor]]:
        """One step of the run loop (module docstring).  color [H,W,3], depth [H,W], c2w [4,4] camera-to-world.  Returns None or
        [uncert_vol, sdf_vol]: float32 device tensors [X,Y,Z], views of a buffer this object overwrites at the next mapped frame."""
        i = int(i)
        cfg, mp = self.config, self.config["mapping"]
        todo = step_schedule(i, cfg)
        vols = None
        with torch.cuda.device(self.device):
            if todo["mesh"]:
                self.save_mesh(i, voxel_size=cfg["mesh"]["voxel_eval"])
            if todo["first"]:
                self.est_c2w_data[0] = c2w
                self.est_c2w_data_rel[0] = c2w
                self._ingest(color, depth)
                self.ba.first_frame_mapping(self.est_c2w_data.tensor[0], int(mp["first_iters"]))
                n_valid = self._read_n_valid() if self.filter_depth else None
                self.keyframeDatabase.add_keyframe_device(self.ba.current, i, self.filter_depth, self._n_valid, n_valid_host=n_valid)
                vols = self._volumes()
                if self.track:
                    self._capture_tracker(color, depth)
                if self.odometry is not None:
                    self._odom_frame_maps(color, depth, self._odom_maps[0])
                    if self.prior_anchor is not None:
                        self.odometry.anchor_reset(self.prior_anchor, self._odom_maps[0], 0)
            else:
                every = int(mp["keyframe_every"])
                if self.track:
                    color, depth = self._track(i, color, depth, every)
                else:
                    self.est_c2w_data[i] = c2w
                if todo["map"] or todo["keyframe"]:
                    self._ingest(color, depth)
                n_valid = None
                if todo["map"]:
                    n_valid = self._read_n_valid() if self.filter_depth else None
                    poses_all = torch.cat([self.est_c2w_data.tensor[0:i:every], self.est_c2w_data.tensor[i:i + 1]], 0)
                    uncert = self.cached_uncert if self.active_ray_sampler is not None else None
                    if self.track:
                        self.ba.global_BA(None, poses_all, uncert_vol=uncert, n_valid=n_valid, optimize_poses=True, pose_init_on_device=True)
                        if self.ba._pose_on:               # coslam.py:401-407: a call that refined poses writes them back
                            pose_scatter(self.est_c2w_data.tensor, self.ba.poses, poses_all.shape[0], every, i, bool(mp.get("optim_cur", True)))
                    else:
                        self.ba.global_BA(None, poses_all, uncert_vol=uncert, n_valid=n_valid)
                    vols = self._volumes()
                if todo["keyframe"]:
                    self.keyframeDatabase.add_keyframe_device(self.ba.current, i, self.filter_depth, self._n_valid, n_valid_host=n_valid)
        if self.active_ray_sampler is not None and vols is not None:
            self.cached_uncert = vols[0]
        return vols

    # ---------------------------------------------------------------------------------------------
    def _savedir(self, kind: str, given: Optional[str]) -> str:
        if given is not None:
            return given
        if self.result_dir is None:
            raise ValueError(f"CoSLAMNarutoHIP: no result_dir was given; pass the {kind} directory")
        return os.path.join(self.result_dir, "coslam", kind)

    def save_mesh(self, i: Optional[int] = None, voxel_size: float = 0.05, suffix: str = "", mesh_savedir: Optional[str] = None):
        """coslam.py:421-458: ``mesh_<i>.ply`` (default: the current step) coloured by ``query_color``, or rendered along the vertex
        normals with ``mesh.render_color``.  Without a ``result_dir`` and a directory nothing is written; the mesh is returned."""
        path = ""
        if mesh_savedir is not None or self.result_dir is not None:
            path = os.path.join(self._savedir("mesh", mesh_savedir), f"mesh_{self.step if i is None else i:04}{suffix}.ply")
        color_func = self.model.render_surface_color if self.config["mesh"]["render_color"] else self.model.query_color
        return extract_mesh(self.model.query_sdf, self.config, self.bounding_box, color_func=color_func, marching_cube_bound=self.marching_cube_bound,
                            voxel_size=voxel_size, mesh_savepath=path)

    def save_uncert_mesh(self, i: Optional[int] = None, voxel_size: float = 0.05, suffix: str = "", mesh_savedir: Optional[str] = None):
        """coslam.py:460-492: the mesh coloured by the uncertainty."""
        path = ""
        if mesh_savedir is not None or self.result_dir is not None:
            path = os.path.join(self._savedir("uncert_mesh", mesh_savedir), f"mesh_{self.step if i is None else i:04}{suffix}.ply")
        return extract_mesh(self.model.query_sdf, self.config, self.bounding_box, color_func=None, marching_cube_bound=self.marching_cube_bound,
                            voxel_size=voxel_size, render_uncert=True, mesh_savepath=path)

    def save_ckpt(self, i: Optional[int] = None, suffix: str = "", ckpt_savedir: Optional[str] = None) -> str:
        """coslam.py:494-517: {'pose', 'pose_rel', 'model'}; the poses as frame id -> [4,4] dicts (``culling.poses_from_checkpoint``)."""
        savedir = self._savedir("checkpoint", ckpt_savedir)
        os.makedirs(savedir, exist_ok=True)
        path = os.path.join(savedir, f"ckpt_{self.step if i is None else i:04}{suffix}.pt")
        model = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        torch.save({"pose": self.est_c2w_data.as_dict(), "pose_rel": self.est_c2w_data_rel.as_dict(), "model": model}, path)
        return path

    def load_ckpt(self, path: str) -> None:
        """The inverse of ``save_ckpt``: the model's ``state_dict`` (``render.load_field_state``) and both pose dicts."""
        from .render import load_checkpoint, load_field_state
        ckpt = load_checkpoint(path)
        for name, store in (("pose", self.est_c2w_data), ("pose_rel", self.est_c2w_data_rel)):
            poses = ckpt.get(name)
            if not isinstance(poses, dict):
                raise ValueError(f"{path}: no '{name}' dict of frame id -> [4,4] in the checkpoint")
            if poses and max(poses) >= self.num_frames:
                raise ValueError(f"{path}: frame {max(poses)} in '{name}', this run holds {self.num_frames} frames")
        load_field_state(self.model, ckpt["model"])
        for name, store in (("pose", self.est_c2w_data), ("pose_rel", self.est_c2w_data_rel)):
            store.tensor.zero_()
            store._have = [False] * self.num_frames
            for k, v in ckpt[name].items():
                store[int(k)] = v

    def render_view(self, c2w, **kw) -> Dict[str, torch.Tensor]:
        """Images of the map from the pose(s) ``c2w`` through this run's camera (``render.FieldViewRendererHIP.render``)."""
        from .render import FieldViewRendererHIP
        cam = {k: getattr(self, k) for k in ("H", "W", "fx", "fy", "cx", "cy")}
        cam.update(near=self.config["cam"]["near"], far=self.config["cam"]["far"])
        return FieldViewRendererHIP(self.model, self.config, cam).render(c2w, **kw)

    @torch.no_grad()
    def predict_sdf(self, points: torch.Tensor) -> torch.Tensor:
        """coslam.py:519-535 / coslam_utils.py:35-56: points [N,K,3] in field coordinates -> sdf [N,K] (units of ``training.trunc``)."""
        bb = self.bounding_box
        q = (points.to(self.device, torch.float32) - bb[:, 0]) / (bb[:, 1] - bb[:, 0])
        return self.model.query_sdf(q, embed=False, return_uncert=True)[..., 0]

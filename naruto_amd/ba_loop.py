"""One mapping (bundle-adjustment) iteration end to end on the device: what the reference's ``CoSLAMNaruto.global_BA`` does per
iteration (reference src/slam/coslam/coslam.py:310-399) --

    rays, ids = keyframeDatabase.sample_global_rays(sample_num)                :325        Co-SLAM KeyFrameDatabase [not in tree]
    idx_cur   = random.sample(valid pixels of the current frame, n_cur)         :332-340
    rays_o, rays_d = poses_all[ids] applied to the camera-frame directions      :342-347
    rays_* = active_ray_sampler.sample_rays(...)        (mapping.active_ray)     :349-359    src/slam/coslam/active_ray_sampler.py:77-149
    ret = model.forward(...); loss = get_loss_from_ret(ret, smooth=True); loss.backward(); Adam     :361-399

-- as ONE stream of launches: ``naruto_assemble_rays`` (N2) -> ``naruto_active_ray_select`` (N1) -> the fused training iteration
(``MappingTrainer``), the first two writing straight into the iteration's input buffers, all of it recorded in one hipGraph.  What
changes between replays lives in device memory: the draws are keyed by the trainer's {seed, iteration counter} (advanced by every
forward), the keyframe / pose / valid-pixel counts sit in a three-word tensor the host refreshes once per ``global_BA`` call, the
planner's uncertainty volume is refreshed in place.  The graph is re-captured only when the ray COUNT changes (n_cur = max(sample_num
// n_kf, min_pixels_cur): constant once n_kf exceeds sample_num / min_pixels_cur, i.e. for all but the first ~20 keyframes).

The reference draws with Python's ``random`` on the host and round-trips through numpy for the active rays; the drawn sets differ by
construction (tests: same distribution properties, and the chained launches equal the three operators run one by one).

POSE REFINEMENT (``optimize_poses``; the reference turns it on with ``tracking.disable: False``).  ``get_pose_param_optim`` and
``matrix_from_tensor`` are Co-SLAM functions that are not in the reference tree: what follows restates the loop around them
(coslam.py:256-281, 342-344, 378-407) with the pose parametrisation of ``naruto_amd.tracking`` -- parity unpinned.  Per ``global_BA``
call with P poses (``poses_all``, the current frame's last; ray id -1 means the last):

1. Pose optimisation is OFF for the call when fewer than 2 keyframes are stored or the caller does not ask for it (coslam.py:264): the
   call is then the plain call, launch for launch and bit for bit.
2. Otherwise pose 0 is fixed, poses 1 .. P-2 are parameters, pose P-1 (the current frame) is one iff ``mapping.optim_cur``
   (coslam.py:273-281).  A parameter pose starts from ``(matrix_to_axis_angle(R), t)`` of the caller's matrix -- converted in fp64 and
   rounded to fp32, on the host or, with ``pose_init_on_device`` (the run loop: ``CoSLAMNarutoHIP(track=True)``), by ``naruto_pose_log`` on
   the device without waiting for the host -- and from the first iteration on its rays are formed from ``R(omega)`` (Rodrigues, evaluated on the
   device for the initial matrices and after every step alike), not from the caller's matrix.  Fixed poses keep the caller's bits.
3. Every iteration is the ordinary mapping iteration (forward, losses incl. smoothness, backward, Adam on the network, uncertainty grid
   every 5th) AND the gradient of the same total loss w.r.t. every parameter pose, taken at the parameters the forward used,
   accumulated over the iterations since the last pose step (``naruto_train_backward_poses``).
4. After the iterations with ``(i + 1) % mapping.pose_accum_step == 0``: one ``torch.optim.Adam`` step (betas 0.9 / 0.999, eps 1e-8,
   ``mapping.lr_rot`` / ``mapping.lr_trans``) on all parameter poses with one shared step count (a pose that drew no ray has gradient
   0 and is still stepped), the accumulated gradient is zeroed, and all later batches of the call -- the prefetched one included -- are
   formed from the new poses (coslam.py:378-395).  Fresh moments and step count at every call.
5. ``refined_poses()`` returns the P poses [P,4,4] float32 on the device; the caller writes them to ``est_c2w_data`` (coslam.py:401-407).

Whether a pose step is due is decided ON THE DEVICE from the call's iteration count, so the per-iteration graphs and the call graph are
the plain ones plus five launches per iteration; ``prepare`` adds one launch per call (the reset, outside the graphs).  The graphs are
re-captured when the switch changes, not when P grows."""

from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import _lib
from .active_ray_sampler import ActiveRaySamplerHIP
from .capture import no_collection, parked, preserved, release_parked
from .keyframe_store import KeyFrameStoreHIP
from .trainer import MappingTrainer, unpack_rays


class FusedBA:
    def __init__(self, trainer: MappingTrainer, store: KeyFrameStoreHIP, sampler: Optional[ActiveRaySamplerHIP] = None,
                 max_poses: int = 4096, use_graph: bool = True, one_launch_prologue: Optional[bool] = None, prefetch: Optional[bool] = None,
                 optimize_poses: Optional[bool] = None):
        assert trainer.direct and trainer.group is None, "FusedBA drives the single-process fused trainer (MappingTrainer(fused_adam=True))"
        self.trainer, self.store, self.sampler = trainer, store, sampler
        self.config = trainer.config
        self.device = trainer.device
        self.use_graph = use_graph
        # assembly + selection as ONE launch (naruto_assemble_select) instead of two.  Measured (round 5, profiles/r05_ba_prologue_ab.txt): the
        # one launch takes 43 us against 20 + 7.5 -- the selecting workgroup has to draw all 6 444 candidates itself (Feistel walks: integer
        # multiplies on ONE CU) where k_assemble_rays spreads them over 34 -- 0.210 against 0.193 ms per iteration: OFF by default
        # (NARUTO_BA_ONE_LAUNCH_PROLOGUE=1 or the argument switch it on; same rays either way, tested)
        self.one_launch_prologue = (os.environ.get("NARUTO_BA_ONE_LAUNCH_PROLOGUE", "0") == "1") if one_launch_prologue is None else bool(one_launch_prologue)
        # PREFETCH (round 5, on by default; NARUTO_BA_PREFETCH=0 or the argument switch it off): the ray assembly of iteration i + 1 rides in the
        # LAST launch of iteration i (k_bwd_finish_next: NarutoFusedAdam.next_batch) -- by then nothing reads the ray buffers any more and the
        # iteration counter that keys the draw has been advanced -- so only the FIRST iteration of a global_BA call launches k_assemble_rays
        # itself.  Same batches, same trajectory (tests: the graph twin prefetches, the eager twin does not).
        self.prefetch = (os.environ.get("NARUTO_BA_PREFETCH", "1") != "0") if prefetch is None else bool(prefetch)
        # ... and with active rays that assembly also looks the candidates' keys up (NarutoRayBatch.keys_out): the selection in front of the
        # next forward starts from the keys (naruto_active_ray_select_keyed) instead of two dependent trips to memory per candidate.
        # NARUTO_BA_KEYED_SELECT=0 switches it off.
        self.keyed = sampler is not None and os.environ.get("NARUTO_BA_KEYED_SELECT", "1") != "0"
        self._keys = None
        # the TrainStep this object last hung its riders on (TrainStep.attach: the next-batch draw, the pose refinement); the step holds
        # them and knows whose they are
        self._armed = None
        # CALL GRAPH (round 5; NARUTO_BA_CALL_GRAPH=0 switches it off): the mapping.iters iterations of a global_BA call recorded as ONE graph
        # next to the per-iteration graphs -- a call of the configured length is one graph launch
        self.call_graph = use_graph and os.environ.get("NARUTO_BA_CALL_GRAPH", "1") != "0"
        mp = self.config['mapping']
        self.active = sampler is not None
        self.sample_num = sampler.oversample_num if self.active else int(mp['sample'])
        self.min_pixels_cur = sampler.min_pixels_cur if self.active else int(mp['min_pixels_cur'])
        self.filter_depth = bool(mp.get('filter_depth', False))
        dev = self.device
        self.current = torch.zeros(store.total_pixels, 7, dtype=torch.float32, device=dev)        # the current frame's rays, refreshed per call
        self.poses = torch.zeros(int(max_poses), 4, 4, dtype=torch.float32, device=dev)
        self.dyn = torch.zeros(3, dtype=torch.int64, device=dev)                                   # {n_kf, n_poses, n_cur_pop}
        # pinned staging for the asynchronous refresh of ``dyn``: TWO buffers used in turn, each guarded by the event recorded behind
        # its last copy -- a second prepare() must not overwrite a buffer whose host-to-device copy is still queued behind replays
        self._dyn_host = [torch.zeros(3, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._dyn_done = [None, None]
        self._dyn_turn = 0
        self._n_cur_pop = 1
        self._vol_ptr = None          # data_ptr of the sampler's volume the graph was captured with
        self._shape = None            # (n_cur, n_train) the graph was captured for
        self._stage = None            # the oversampled batch between assembly and selection (active ray only)
        self._ws = None
        self.bbox = [[float(v) for v in row] for row in self.config['mapping']['bound']]
        # pose refinement (see the module docstring): the default follows the reference's switch, tracking.disable
        tk = self.config.get('tracking') or {}
        self.optimize_poses = (not bool(tk.get('disable', True))) if optimize_poses is None else bool(optimize_poses)
        self._pose = None             # the per-pose device buffers (allocated on first use)
        self._bap = None              # the NarutoBAPoses of the current shape
        self._pose_on = False         # this call refines poses
        self._n_poses = 0
        self._init_c2w = None

    # ---------------------------------------------------------------------------------------------
    def sizes(self, n_kf: int, n_valid_cur: int):
        """(n_cur, n_train): current-frame rays drawn (coslam.py:332-340) and rays the training step sees."""
        n_cur = max(self.sample_num // n_kf, self.min_pixels_cur)
        if self.filter_depth:
            n_cur = min(n_valid_cur, n_cur)
        n_train = self.sampler.n_out(n_cur) if self.active else self.sample_num + n_cur
        return n_cur, n_train

    def _keyed(self, n_cur: int) -> bool:
        return self.keyed and self.sample_num + n_cur - self.sampler.n_out(n_cur) <= 8192

    def _assemble(self, out, n_cur: int, keyed: bool = False, call=None, frame_only: bool = False):
        """The batch draw into ``out``, its argument list stated once: launched (``assemble_batch``) or, with
        ``call=self.store.next_batch_struct``, described for the fused optimiser's next_batch.  ``keyed``: the assembly looks the
        candidates' keys up while the rows are in registers (NarutoRayBatch.keys_out).  ``frame_only``: first-frame mapping -- no stored
        ray, every pixel of the frame a candidate."""
        sample_num, filter_depth = (0, False) if frame_only else (self.sample_num, self.filter_depth)
        keys = self.sampler.key_lookup(self.sample_num + n_cur, n_cur, self.bbox, self._keys) if keyed else None
        return (call or self.store.assemble_batch)(sample_num, self.current, self.poses, self.min_pixels_cur, out=out, filter_depth=filter_depth,
                                                   rng=self.trainer.iter_state, dyn=self.dyn, n_cur=n_cur, n_cur_pop=self._n_cur_pop, keys=keys,
                                                   ids_out=self._ids())

    def _select(self, bufs, n_cur: int, keyed: bool):
        """The active ray selection from the stage into ``bufs`` (``keyed``: starting from the keys the assembly looked up)."""
        self.sampler.sample_rays(*self._stage, n_cur, None, self.bbox, out=bufs, workspace=self._ws, keys=self._keys if keyed else None,
                                 src_rows=self._src_rows())

    def _prologue(self, n_cur: int):
        def prologue(*bufs):
            if not self.active:
                self._assemble(bufs, n_cur)
            elif self.one_launch_prologue and self.sample_num + n_cur - self.sampler.n_out(n_cur) <= 8192:
                # assembly + selection in one launch (naruto_assemble_select): the oversampled batch is never written
                assert not self._pose_on
                self.store.assemble_select(self.sampler, self.sample_num, self.current, self.poses, self.min_pixels_cur, self.bbox, out=bufs,
                                           filter_depth=self.filter_depth, rng=self.trainer.iter_state, dyn=self.dyn, n_cur=n_cur, n_cur_pop=self._n_cur_pop)
            else:
                keyed = self._keyed(n_cur)
                self._assemble(self._stage, n_cur, keyed)
                self._select(bufs, n_cur, keyed)
        return prologue

    def _later_prologue(self, n_cur: int):
        """With prefetch: what an iteration that finds its batch assembled still has to launch (the selection; the candidates' keys were
        looked up by the assembly that rode in the previous iteration's finishing launch), or None."""
        return (lambda *bufs: self._select(bufs, n_cur, self._keyed(n_cur))) if self.active else None

    def _attach(self, train_step, next_batch=None):
        """This object's riders onto ``train_step`` -- the pose refinement while a call refines poses, ``next_batch`` -- and off the step
        they rode on before."""
        if self._armed is not None and self._armed is not train_step:
            self._armed.detach(self)
        ba_poses = self._bap if self._pose_on else None
        train_step.attach(self, next_batch=next_batch, ba_poses=ba_poses)
        self._armed = train_step if (next_batch is not None or ba_poses is not None) else None

    def _arm(self, n_cur: int, bufs, train_step):
        """``_attach`` with the draw of the NEXT iteration as the fused optimiser's next_batch when this object prefetches (into the stage
        when active rays select from it, else straight into the iteration's own input buffers).  The struct and everything it points
        into live ON the TrainStep whose backward reads them (the trainer's cache and a captured graph's _static['ts'] outlive this
        object): the host pointer in opt.next_batch can never dangle."""
        self._attach(train_step, self._assemble(self._stage if self.active else bufs, n_cur, self.active and self._keyed(n_cur),
                                                call=self.store.next_batch_struct) if self.prefetch else None)

    def _detach(self):
        """Take this object's riders off the TrainStep they ride on: its backward no longer assembles anything (and no longer overwrites
        the stage / ray buffers of this object) nor refines poses.  Somebody else's riders on that step stay."""
        ts, self._armed = getattr(self, "_armed", None), None
        return ts is not None and ts.detach(self)

    def close(self):
        """Detach from the trainer: the TrainStep this object rode on keeps working as a plain training step (trainer.step,
        first_frame_mapping).  Graphs captured with this object's riders inside are dropped (their finishing launch would go on drawing
        batches) -- not the graphs another FusedBA has captured on the same TrainStep since."""
        st = getattr(self.trainer, "_static", None)
        captured = getattr(self, "_armed", None) is not None and st is not None and st.get('ts') is self._armed
        if self._detach() and captured and self.use_graph:
            self._drop_graphs()
        self._shape = None

    def _drop_graphs(self):
        """Forget the trainer's graphs (they hold this object's prefetch / pose launches).  Inside a stream capture -- this object's
        finaliser can run in somebody else's -- the graph objects are parked instead of destroyed."""
        tr = self.trainer
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            parked((tr._graphs, getattr(tr, "_static", None)))
        tr._graphs = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --------------------------------------------------------------------------------------------- pose refinement
    def _ids(self):
        return self._pose["ids"] if self._pose_on else None

    def _src_rows(self):
        return self._pose["src_rows"] if (self._pose_on and self.active) else None

    def _check_pose_refinement(self):
        """The refusals, before anything is launched."""
        mp, tr = self.config['mapping'], self.config['training']
        rot_rep = tr.get('rot_rep', 'axis_angle')
        if rot_rep != 'axis_angle':
            raise NotImplementedError(f"FusedBA refines axis-angle poses: training.rot_rep = {rot_rep!r} is not implemented")
        if self.trainer.group is not None:
            raise NotImplementedError("FusedBA(optimize_poses=True): pose gradients are not all-reduced across data-parallel ranks")
        if self.active and self.one_launch_prologue:
            raise NotImplementedError("FusedBA(optimize_poses=True) with one_launch_prologue=True: naruto_assemble_select never writes the oversampled "
                                      "batch the pose ids follow; use the two-launch prologue (the default)")
        if int(mp.get('map_accum_step', 1)) != 1 or int(mp.get('map_wait_step', 0)) != 0:
            raise NotImplementedError("FusedBA(optimize_poses=True): mapping.map_accum_step must be 1 and mapping.map_wait_step 0")
        if int(mp.get('pose_accum_step', 5)) <= 0:
            raise ValueError("mapping.pose_accum_step must be positive")

    def _pose_buffers(self):
        if self._pose is None:
            dev, n = self.device, self.poses.shape[0]
            f32 = dict(dtype=torch.float32, device=dev)
            mp = self.config['mapping']
            accum = max(int(mp.get('pose_accum_step', 5)), 1)
            max_trace = max(-(-int(mp['iters']) // accum), 1)
            self._pose = {"pose_init": torch.zeros(n, 6, **f32), "pose6": torch.zeros(n, 6, **f32), "exp_avg": torch.zeros(n, 6, **f32),
                          "exp_avg_sq": torch.zeros(n, 6, **f32), "accum": torch.zeros(n, 12, dtype=torch.float64, device=dev),
                          "state": torch.zeros(4, dtype=torch.int32, device=dev), "trace_pose": torch.zeros(max_trace, n, 6, **f32),
                          "trace_grad": torch.zeros(max_trace, n, 6, **f32), "max_trace": max_trace}
        return self._pose

    def _build_bap(self, n_cur: int, n_train: int):
        """The NarutoBAPoses of this shape (ids / source rows / ray-gradient buffers are per shape, the per-pose buffers are not)."""
        pb = self._pose_buffers()
        dev = self.device
        mp, tr = self.config['mapping'], self.config['training']
        n_stage = self.sample_num + n_cur
        S = int(tr['n_samples_d']) + int(tr['n_range_d'])
        pb["ids"] = torch.zeros(n_stage, dtype=torch.int64, device=dev)
        pb["src_rows"] = torch.zeros(n_train, dtype=torch.int32, device=dev) if self.active else None
        pb["d_rays_o"], pb["d_rays_d"] = torch.zeros(n_train, 3, device=dev), torch.zeros(n_train, 3, device=dev)
        pb["ws"] = _lib.workspace(_lib.load().naruto_ba_poses_workspace(self.trainer.model._handle().ptr, n_train, S), dev, zero=True)
        b = _lib.NarutoBAPoses()
        b.max_poses, b.optim_cur, b.pose_accum_step = self.poses.shape[0], 1 if mp.get('optim_cur', True) else 0, int(mp.get('pose_accum_step', 5))
        b.dyn, b.poses = self.dyn.data_ptr(), self.poses.data_ptr()
        b.pose_init, b.pose6, b.exp_avg, b.exp_avg_sq = (pb[k].data_ptr() for k in ("pose_init", "pose6", "exp_avg", "exp_avg_sq"))
        b.accum, b.state = pb["accum"].data_ptr(), pb["state"].data_ptr()
        b.ids, b.n_ids = pb["ids"].data_ptr(), n_stage
        b.src_rows = pb["src_rows"].data_ptr() if self.active else None
        b.d_rays_o, b.d_rays_d = pb["d_rays_o"].data_ptr(), pb["d_rays_d"].data_ptr()
        b.lr_rot, b.lr_trans, b.beta1, b.beta2, b.eps = float(mp['lr_rot']), float(mp['lr_trans']), 0.9, 0.999, 1e-8
        b.trace_pose, b.trace_grad, b.max_trace = pb["trace_pose"].data_ptr(), pb["trace_grad"].data_ptr(), pb["max_trace"]
        b.workspace = pb["ws"].data_ptr()
        self._bap = b

    def refined_poses(self) -> torch.Tensor:
        """The P poses of the last ``prepare`` / ``global_BA`` as they stand now, [P,4,4] float32 on the device: refined where the call
        optimised them, the caller's bits otherwise.  The caller writes them back to ``est_c2w_data`` (coslam.py:401-407)."""
        return self.poses[:self._n_poses].clone()

    def last_pose_trace(self) -> Dict:
        """The last refining call, read when asked: ``n_steps`` pose steps taken; per step ``pose`` [n_steps,P,6] the (omega, t) BEFORE the
        step and ``grad`` [n_steps,P,6] the accumulated gradient (fixed poses: their (omega, t) and zeros); ``init_c2w`` [P,4,4] the
        matrices the call started from (R(omega) for the parameter poses); ``iterations`` of the call so far."""
        if not self._pose_on or self._pose is None:
            raise RuntimeError("last_pose_trace: the last call did not optimise poses")
        pb, P = self._pose, self._n_poses
        state = pb["state"].cpu()
        n = min(int(state[0]), pb["max_trace"])
        return {"n_steps": int(state[0]), "iterations": int(state[1]), "pose": pb["trace_pose"][:n, :P].cpu().clone(),
                "grad": pb["trace_grad"][:n, :P].cpu().clone(), "init_c2w": self._init_c2w.clone(), "pose6": pb["pose6"][:P].cpu().clone()}

    def prepare(self, current_rays: Optional[torch.Tensor], poses_all: torch.Tensor, uncert_vol=None, smooth: bool = True, optimize_poses: Optional[bool] = None,
                n_valid: Optional[int] = None, pose_init_on_device: bool = False):
        """Per ``global_BA`` call: the current frame's rays [H*W,7], all poses [P,4,4] (the current frame's LAST), optionally the
        planner's refreshed uncertainty volume.  One count of the valid-depth pixels is read back (the reference does the same
        filtering on the host, coslam.py:332-337); everything else is asynchronous.  ``optimize_poses`` (default: the constructor's):
        refine the keyframe poses during the call (module docstring); the matrices are converted to (omega, t) on the host.
        ``current_rays=None``: ``self.current`` has been filled by the caller (``keyframe_store.frame_ingest(..., out=ba.current, ...)``) and
        ``n_valid`` is that launch's count of valid-depth pixels (needed with ``mapping.filter_depth``): the copy and the count are skipped.
        ``pose_init_on_device``: the (omega, t) of the P poses come from ``naruto_pose_log`` over ``self.poses[:P]`` on the device instead
        of the host conversion -- same branches and formulas, no wait for the host (the run loop's tracked frames)."""
        dev = self.device
        release_parked()
        want_poses = self.optimize_poses if optimize_poses is None else bool(optimize_poses)
        if want_poses:
            self._check_pose_refinement()
        if current_rays is None:
            assert n_valid is not None or not self.filter_depth, "current_rays=None with mapping.filter_depth: pass the ingest's n_valid"
            cur = self.current
        else:
            assert n_valid is None, "n_valid belongs to current_rays=None (the count is taken from the rays given)"
            cur = current_rays.to(dev, torch.float32).reshape(-1, 7)
            assert cur.shape[0] == self.current.shape[0], "current_rays: one row per pixel of the frame the store was built for"
            self.current.copy_(cur, non_blocking=True)
        P = poses_all.shape[0]
        assert P <= self.poses.shape[0], "more poses than FusedBA(max_poses=...)"
        self.poses[:P].copy_(poses_all.to(dev, torch.float32), non_blocking=True)
        n_kf = len(self.store)
        assert n_kf > 0, "no keyframe stored yet"
        self._n_poses = P
        pose_on = bool(want_poses and n_kf >= 2 and P >= 2)            # coslam.py:264
        if pose_on:
            # (omega, t) of every pose: on the device from the rows just copied (naruto_pose_log), or fp64 on the host, through pinned
            # memory (the caching host allocator keeps the block until the copy ran)
            if pose_init_on_device:
                from .pose_chain import pose_log
                pose_log(self.poses[:P], out=self._pose_buffers()["pose_init"][:P])
            else:
                from .tracking import matrices_to_pose6
                host6 = matrices_to_pose6(poses_all).float().pin_memory()
                self._pose_buffers()["pose_init"][:P].copy_(host6, non_blocking=True)
        if current_rays is None:
            n_valid = int(n_valid) if self.filter_depth else cur.shape[0]
        elif not self.filter_depth:
            n_valid = cur.shape[0]
        else:
            n_valid = int(((cur[:, -1] > 0.0) & (cur[:, -1] <= self.config["cam"]["depth_trunc"])).sum().item())
        turn = self._dyn_turn
        self._dyn_turn ^= 1
        if self._dyn_done[turn] is not None:
            self._dyn_done[turn].synchronize()            # the copy that last read this staging buffer has landed (two calls back: normally long ago)
        host = self._dyn_host[turn]
        host[0], host[1], host[2] = n_kf, P, max(n_valid, 1)
        self._n_cur_pop = max(n_valid, 1)
        self.dyn.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._dyn_done[turn] = ev
        vol_moved = False
        if self.active and uncert_vol is not None:
            vol = self.sampler.set_volume(uncert_vol, dev)
            vol_moved = self._vol_ptr is not None and vol.data_ptr() != self._vol_ptr      # a new tensor (other shape): the captured launch reads the old one
            self._vol_ptr = vol.data_ptr()
        n_cur, n_train = self.sizes(n_kf, n_valid)
        if self._shape != (n_cur, n_train, smooth, pose_on) or (vol_moved and (self.use_graph or self.keyed)):
            self._detach()
            self._pose_on = pose_on
            if pose_on:
                self._build_bap(n_cur, n_train)
            f32 = dict(dtype=torch.float32, device=dev)
            n_stage = self.sample_num + n_cur
            if self.active:
                self._stage = (torch.empty(n_stage, 3, **f32), torch.empty(n_stage, 3, **f32), torch.empty(n_stage, 3, **f32), torch.empty(n_stage, 1, **f32))
                self._ws = _lib.workspace(4 * self.sampler.workspace_elems(n_stage), dev, torch.int32)
                self._keys = torch.zeros(n_stage, dtype=torch.int32, device=dev)
            pro = self._prologue(n_cur)
            chain = [(i + 1) % 5 == 0 for i in range(int(self.config['mapping']['iters']))] if self.call_graph else None
            self._drive(n_train, smooth, pro, self._later_prologue(n_cur) if self.prefetch else pro, lambda bufs, ts: self._arm(n_cur, bufs, ts), chain)
            self._shape = (n_cur, n_train, smooth, pose_on)
        if pose_on:
            # the call's reset: (omega, t) <- the upload, moments / sums / counts zeroed, the parameter poses' matrices from R(omega) -- after
            # a capture's warm-up iterations (they step the poses like any other iteration) and in front of the call's first assembly
            import ctypes as C
            from .ops import _on_device, _stream
            with _on_device(dev):
                _lib.check(_lib.load().naruto_ba_poses_init(C.byref(self._bap), _stream()), "naruto_ba_poses_init")
            self._init_c2w = self.poses[:P].clone()
        return n_cur, n_train

    def _drive(self, n_train: int, smooth: bool, first_prologue, later_prologue, arm, chain=None):
        """Set the trainer up for this object's iterations of ``n_train`` rays.  Graph mode: capture them, ``later_prologue`` in front of
        every iteration and, with prefetch, ``first_prologue`` in front of a call's first (the later ones find their batch drawn by the
        preceding iteration's last launch; without prefetch the two are the same), ``chain`` as ``MappingTrainer.capture`` takes it.
        Eager mode: the iterations' own ray buffers.  Either way ``arm(bufs, train_step)`` hangs this object's riders on the step."""
        self._pro, self._pro_later, self._driven = first_prologue, later_prologue, (n_train, smooth, arm, chain)
        tr = self.trainer
        if self.use_graph:
            with no_collection():
                tr.capture(n_train, smooth=smooth, prologue=later_prologue, first_prologue=first_prologue if self.prefetch else None, chain=chain,
                           on_buffers=lambda *a: arm(a[:4], a[4]))
        else:
            self._eager_bufs = unpack_rays(torch.zeros(n_train * 10, dtype=torch.float32, device=self.device), n_train)
            tr._graphs = None
            arm(self._eager_bufs, tr.train_step_for(n_train, smooth))

    def _iterate(self, i: int, smooth: bool, uncert_step: bool):
        tr = self.trainer
        n_train, _, arm, chain = self._driven
        if self.use_graph:
            dropped = tr.ray_buffers() is None
            if dropped:
                # somebody took the trainer's graphs away (another FusedBA on the same trainer, trainer._graphs = None): capture again,
                # the poses being refined put back like the rest of the training state, and assemble this iteration's batch here -- nothing
                # prefetched it (the draw is keyed by the iteration counter: assembling twice is idempotent)
                pose_state = [self.poses] + [v for v in self._pose.values() if torch.is_tensor(v)] if self._pose_on else []
                with preserved(pose_state):
                    self._drive(n_train, smooth, self._pro, self._pro_later, arm, chain)
            bufs = tr.ray_buffers()
            if dropped:
                self._pro(*bufs)
            return tr.step(*bufs, smooth=smooth, uncert_step=uncert_step, first=(i == 0))           # the replay starts with the prologue's launches
        bufs = self._eager_bufs
        full = i == 0 or not self.prefetch
        # the TrainStep this iteration WILL run on (the trainer's cache is keyed on (n_rays, smooth, n_rays_total) and evicts, and another
        # FusedBA may have taken it over): if this object's riders are not on it, nothing drew this iteration's batch and nothing would draw
        # the next one -- arm it and assemble this batch with the full prologue
        ts = tr.train_step_for(n_train, smooth)
        drawn, refined = ts.riders_of(self)
        if (self.prefetch and drawn is None) or refined is not (self._bap if self._pose_on else None):
            arm(bufs, ts)
            full = True
        pro = self._pro if full else self._pro_later
        if pro is not None:
            pro(*bufs)
        return tr.step(*bufs, smooth=smooth, uncert_step=uncert_step)

    def iteration(self, i: int, smooth: bool = True):
        """Iteration ``i`` (0-based) of the current ``global_BA`` call: the uncertainty grid's Adam steps after iterations 5, 10, ...
        (coslam.py:397-399)."""
        return self._iterate(i, smooth, (i + 1) % 5 == 0)

    def global_BA(self, current_rays: Optional[torch.Tensor], poses_all: torch.Tensor, n_iters: Optional[int] = None, uncert_vol=None, smooth: bool = True,
                  optimize_poses: Optional[bool] = None, n_valid: Optional[int] = None, pose_init_on_device: bool = False):
        """The optimisation loop of one ``global_BA`` call (coslam.py:293-399).  ``optimize_poses`` (default: the constructor's, which
        follows ``tracking.disable``; off in every shipped config): refine the keyframe poses during the call as the reference's pose
        optimiser does (module docstring); read them with ``refined_poses()`` afterwards.  ``current_rays=None`` with ``n_valid``, ``pose_init_on_device``: see ``prepare``."""
        self.prepare(current_rays, poses_all, uncert_vol, smooth, optimize_poses, n_valid=n_valid, pose_init_on_device=pose_init_on_device)
        return self.call_iterations(n_iters, smooth)

    def first_frame_mapping(self, pose: torch.Tensor, n_iters: Optional[int] = None):
        """The optimisation loop of the reference's ``first_frame_mapping`` (coslam.py:197-219) on the device, over the frame in
        ``self.current`` (``keyframe_store.frame_ingest(..., out=ba.current, ...)``): every iteration draws ``mapping.sample`` distinct
        pixels out of ALL H*W (``select_samples`` does not filter by depth; no keyframe is stored yet, no active rays) -- the batch assembly
        with ``n_global = 0``, keyed by the trainer's {seed, iteration counter} and prefetched by the preceding iteration's last launch like a
        ``global_BA`` batch --, forms the rays with the single ``pose`` [4,4], and takes a training step without the smoothness term.  The
        network's Adam steps every iteration; the uncertainty grid's gradient is zeroed once, accumulates over all iterations, is stepped
        once at the end and is NOT zeroed afterwards (``MappingTrainer.first_frame_mapping``'s contract).  ``n_iters`` defaults to
        ``mapping.first_iters``.  Replayed as per-iteration graphs; the next ``prepare`` captures the ``global_BA`` graphs afresh."""
        dev, tr = self.device, self.trainer
        mp = self.config['mapping']
        n_iters = int(mp['first_iters']) if n_iters is None else int(n_iters)
        n = int(mp['sample'])
        n_pix = self.current.shape[0]
        assert n <= n_pix, "mapping.sample exceeds the frame's pixel count"
        release_parked()
        self._detach()
        self._pose_on = False
        self._shape = None                     # the graphs below replace a global_BA call's
        self.poses[:1].copy_(pose.to(dev, torch.float32).reshape(1, 4, 4), non_blocking=True)
        self._n_poses = 1
        self.dyn.copy_(torch.tensor([0, 1, n_pix], dtype=torch.int64), non_blocking=False)
        self._n_cur_pop = n_pix

        def prologue(*bufs):
            self._assemble(bufs, n, frame_only=True)

        def arm(bufs, ts):
            self._attach(ts, self._assemble(bufs, n, call=self.store.next_batch_struct, frame_only=True) if self.prefetch else None)

        with torch.no_grad():
            tr.model.uncert_grid.grad.zero_()
        self._drive(n, False, prologue, None if self.prefetch else prologue, arm)
        out = None
        for i in range(n_iters):
            out = self._iterate(i, False, False)
        with torch.no_grad():
            tr.uncert_optim.step()
        # the finishing launch of the last iteration drew one more batch into buffers nobody reads; take the draw off the training step
        # so that a plain trainer.step on it afterwards assembles nothing
        if self.use_graph:
            self._drop_graphs()
        self._detach()
        return out

    def call_iterations(self, n_iters: Optional[int] = None, smooth: bool = True):
        """The iterations of the current ``global_BA`` call (after ``prepare``): one launch of the call graph when the call has the
        configured length, iteration by iteration otherwise.  Returns the last iteration's (ret, loss)."""
        n_iters = int(self.config['mapping']['iters']) if n_iters is None else int(n_iters)
        if self.use_graph and self.trainer.chain_length() == n_iters and self._shape is not None and self._shape[2] == smooth:
            return self.trainer.step_chain()
        out = None
        for i in range(n_iters):
            out = self.iteration(i, smooth)
        return out

"""Mesh subdivision on the device: ``subdivide_to_size``, the step the evaluation protocol's culling tool runs before the vertex test.

``third_parties/neural_slam_eval/cull_mesh.py`` (scripts/evaluation/eval_replica.sh:55-72) subdivides the mesh with
``trimesh.remesh.subdivide_to_size`` before it decides, per vertex, what the cameras saw -- to the author's recollection by default, at
1.5 cm; that cannot be verified on this stack (the tool is an empty submodule of the reference tree and ``trimesh`` is not installed),
so the step is OFF unless ``max_edge`` is given.  PARITY UNPINNED, as the cull itself is.  This is the contract, restated from the
published algorithm, not from that code:

  Inputs: vertices [V,3] float32 or float64 (kept in their own dtype), faces [F,3], optional RGBA8 colours [V,4], ``max_edge`` > 0,
  ``max_iter`` = 10, ``max_faces`` = 2**27.

  A generation
  1. A face is *long* iff, for one of its edges (a, b), ((dx*dx + dy*dy) + dz*dz) > max_edge*max_edge with d = v[b] - v[a]: everything in
     the vertices' dtype, products and sums rounded, no contraction, ``max_edge`` converted to that dtype once.  The comparison is strict
     (an edge of exactly ``max_edge`` is not split), there is no square root (so the numpy twin makes the same bits), and NaN compares
     false: such a face is never split.
  2. No face long, or ``max_iter`` generations done: stop, and report the number of generations and of faces that are still long.  A
     positive remainder is not an error: the result carries it and the command line prints it.
  3. The next face count is F + 3 n_long and the vertex count at most V + 3 n_long.  If the first exceeds ``max_faces`` or the second
     reaches 2^31 (indices stay int32): ValueError, before anything is allocated or launched for that generation.
  4. One midpoint per UNDIRECTED edge of the long faces, shared by the long faces that meet in it (welded): (v[lo] + v[hi]) * 0.5 in
     the vertices' dtype, colour (c[lo] + c[hi] + 1) >> 1 per channel.  Midpoints are appended behind the existing vertices in order of
     first appearance in the long faces' edge list, which is face-major in face order with the slots (v0v1), (v1v2), (v2v0).  Existing
     vertices keep their indices and values in every generation: the input's vertices are a prefix of the output's.
  5. The new face list: the faces that are not long first, in their order and unchanged; then four children per long face, in the long
     faces' order: (v0,m0,m2) (m0,v1,m1) (m2,m1,v2) (m0,m1,m2), m_k the midpoint of slot k (the winding is preserved).  An edge between
     a long and a short face gets a midpoint only the long side uses: that T-junction is the published function's behaviour and leaves
     the surface unchanged.

  What differs from trimesh's function is the indexing only: it sets finished faces aside with copies of their vertices per generation,
  here there is one welded vertex array.  Generation by generation the same faces are split into the same triangles.

Stages of a generation (csrc/naruto_subdiv.hip): mark -> torch.cumsum -> edge table (64-bit compare-and-swap on the key, integer minimum
on the slot ordinal: the numbering depends on the mesh alone) -> torch.cumsum -> emit.  The host reads two small copies per generation
(n_long; n_mid with the error word).  tests/subdivide_spec.py restates the contract in numpy and the kernels equal it in every bit.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import check
from . import mesh as M

DEFAULT_MAX_ITER = 10
DEFAULT_MAX_FACES = 2 ** 27
MIN_TABLE_SLOTS = 64


@dataclass
class SubdividePlan:
    """Cells of the edge table per slot of a long face (>= 2: the table is at most half full); the result does not depend on it."""
    table_factor: float = 2.0


@dataclass
class SubdivideResult:
    generations: int
    remaining_long: int                  # faces that still have an edge longer than max_edge (> 0 only when max_iter stopped it)


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check_arguments(max_edge, max_iter, max_faces) -> None:
    if isinstance(max_edge, bool) or not isinstance(max_edge, (int, float)) or not math.isfinite(max_edge) or not max_edge > 0:
        raise ValueError(f"subdivide: max_edge must be a finite number > 0, got {max_edge!r}")
    if int(max_iter) != max_iter or max_iter < 0:
        raise ValueError(f"subdivide: max_iter must be an integer >= 0, got {max_iter!r}")
    if int(max_faces) != max_faces or max_faces < 1:
        raise ValueError(f"subdivide: max_faces must be an integer >= 1, got {max_faces!r}")


def check_growth(n_faces: int, n_vertices: int, n_long: int, max_faces: int) -> None:
    """Step 3: the predicted sizes of the next generation, before anything is allocated or launched for it."""
    nf, nv = n_faces + 3 * n_long, n_vertices + 3 * n_long
    if nf > max_faces:
        raise ValueError(f"subdivide: the next generation would have {nf} faces, more than max_faces = {max_faces}")
    if nv >= 2 ** 31:
        raise ValueError(f"subdivide: the next generation could have {nv} vertices; indices are int32")


def table_slots(n_long: int, plan=None) -> int:
    factor = 2.0 if plan is None else float(plan.table_factor if isinstance(plan, SubdividePlan) else plan["table_factor"])
    if not (math.isfinite(factor) and factor >= 2.0):
        raise ValueError("subdivide: the edge table has at least 2 cells per slot")
    return max(MIN_TABLE_SLOTS, math.ceil(factor * 3 * n_long))


def colors_tensor(colors, n_vertices: int, device) -> Optional[torch.Tensor]:
    """RGBA8 [V,4] on the device, checked on the host side first: one colour per vertex."""
    if colors is None:
        return None
    c = torch.as_tensor(colors)
    if c.numel() != 4 * n_vertices:
        raise ValueError("subdivide: one RGBA colour per vertex")
    return c.to(device=device, dtype=torch.uint8).reshape(-1, 4).contiguous()


def subdivide_on_device(v: torch.Tensor, f: torch.Tensor, col: Optional[torch.Tensor], max_edge: float, max_iter: int = DEFAULT_MAX_ITER,
                        max_faces: int = DEFAULT_MAX_FACES, plan=None, timings: Optional[list] = None):
    """The generations, on checked device tensors (v [V,3] float32/float64, f int32 [F,3], col uint8 [V,4] or None, all contiguous) ->
    (v, f, col, SubdivideResult).  ``timings``: a list that receives one dict per generation with the faces in and out and the seconds of
    each stage between device synchronisations (tools/time_subdivide.py); timing adds the synchronisations, nothing else."""
    lib = _lib.load()
    f64 = int(v.dtype == torch.float64)
    generations = 0

    def lap(row, name, t0):
        if timings is None:
            return t0
        import time
        torch.cuda.synchronize(v.device)
        t1 = time.perf_counter()
        if name is not None:
            row[name] = row.get(name, 0.0) + (t1 - t0)
        return t1

    with torch.cuda.device(v.device):
        while True:
            n_f, n_v = len(f), len(v)
            row = {"faces_in": n_f, "vertices_in": n_v}
            t = lap(row, None, 0.0)
            flags = torch.empty(n_f, dtype=torch.uint8, device=v.device)
            check(lib.naruto_subdivide_mark(n_f, n_v, f.data_ptr(), v.data_ptr(), f64, float(max_edge), flags.data_ptr(), _stream()), "naruto_subdivide_mark")
            t = lap(row, "mark_s", t)
            rank = torch.cumsum(flags, 0, dtype=torch.int32)
            n_long = int(rank[-1])                                            # host read 1 of the generation
            t = lap(row, "scan_s", t)
            if n_long == 0 or generations >= max_iter:
                if timings is not None:
                    row.update(n_long=n_long, faces_out=n_f, vertices_out=n_v)
                    timings.append(row)
                return v, f, col, SubdivideResult(generations, n_long)
            check_growth(n_f, n_v, n_long, max_faces)
            slots = table_slots(n_long, plan)
            n_bytes = lib.naruto_subdivide_workspace(n_long, slots)
            if n_bytes == 0:
                raise ValueError(f"subdivide: {n_long} long faces with an edge table of {slots} cells are beyond the supported sizes")
            ws = _lib.workspace(n_bytes, v.device, torch.int32)
            own = torch.empty(3 * n_long, dtype=torch.uint8, device=v.device)
            check(lib.naruto_subdivide_edges(n_f, n_v, f.data_ptr(), flags.data_ptr(), rank.data_ptr(), n_long, slots, ws.data_ptr(), own.data_ptr(), _stream()),
                  "naruto_subdivide_edges")
            t = lap(row, "edges_s", t)
            mid_rank = torch.cumsum(own, 0, dtype=torch.int32)
            n_mid, err = (int(x) for x in torch.stack([mid_rank[-1], ws[0]]).cpu())                  # host read 2: the midpoints and the error word
            t = lap(row, "scan_s", t)
            if err != 0 or not 0 < n_mid <= 3 * n_long:
                raise _lib.NarutoError(f"naruto_subdivide_edges: error word {err}, {n_mid} midpoints for {n_long} long faces")
            new_v = torch.empty(n_v + n_mid, 3, dtype=v.dtype, device=v.device)
            new_v[:n_v] = v
            new_c = None
            if col is not None:
                new_c = torch.empty(n_v + n_mid, 4, dtype=torch.uint8, device=v.device)
                new_c[:n_v] = col
            new_f = torch.empty(n_f + 3 * n_long, 3, dtype=torch.int32, device=v.device)
            t = lap(row, "copy_s", t)
            check(lib.naruto_subdivide_emit(n_f, n_v, f.data_ptr(), flags.data_ptr(), rank.data_ptr(), n_long, slots, ws.data_ptr(), mid_rank.data_ptr(), n_mid,
                                            new_v.data_ptr(), f64, new_c.data_ptr() if new_c is not None else None, new_f.data_ptr(), _stream()), "naruto_subdivide_emit")
            t = lap(row, "emit_s", t)
            if timings is not None:
                row.update(n_long=n_long, n_mid=n_mid, table_slots=slots, faces_out=len(new_f), vertices_out=len(new_v))
                timings.append(row)
            v, f, col = new_v, new_f, new_c
            generations += 1


def subdivide_to_size(mesh, max_edge: float, max_iter: int = DEFAULT_MAX_ITER, max_faces: int = DEFAULT_MAX_FACES, plan=None):
    """(subdivided mesh, :class:`SubdivideResult`) -- the module docstring's contract.  ``mesh`` is what :func:`naruto_amd.culling.cull_mesh`
    takes and the result is of the same kind: a :class:`naruto_amd.mesh.Mesh` or the path of a ``.ply`` -> a Mesh (float64 vertices, int64
    faces); a tuple (vertices, faces[, colors RGBA8 [V,4]]) of arrays or device tensors -> the same tuple as device tensors (vertices in
    their own dtype, faces int32).  ``plan``: a :class:`SubdividePlan`; no bit of the result depends on it.  Arguments are checked before
    any launch."""
    from . import culling as CU
    check_arguments(max_edge, max_iter, max_faces)
    table_slots(1, plan)                                                      # (the plan is checked here, before any launch)
    vertices, faces, colors, kind = CU._as_mesh(mesh)
    if colors is not None and torch.as_tensor(colors).numel() != 4 * (torch.as_tensor(vertices).numel() // 3):
        raise ValueError("subdivide: one RGBA colour per vertex")
    v, f = CU._geometry(vertices, faces)
    col = colors_tensor(colors, len(v), v.device)
    v, f, col, res = subdivide_on_device(v, f, col, float(max_edge), int(max_iter), int(max_faces), plan)
    if kind == "mesh":
        return M.Mesh(v.to(torch.float64).cpu().numpy(), f.to(torch.int64).cpu().numpy(), col.cpu().numpy() if col is not None else None), res
    return ((v, f, col) if colors is not None else (v, f)), res

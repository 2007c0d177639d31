"""numpy restatement of the subdivision contract (naruto_amd/remesh.py, csrc/naruto_subdiv.hip): generations of 1 -> 4 splits of the faces
that have an edge longer than max_edge, one welded midpoint per undirected edge, numbered in order of first appearance.  Every operation
is a numpy operation in the vertices' own dtype in the order the contract writes it (no square root), so the device results are
compared with ``==`` on the bits.  Plain vectorised numpy: the room at max_edge 0.1 (156 292 faces) takes a fraction of a second."""
import numpy as np


def long_faces(vertices, faces, max_edge):
    """bool [F]: the face has an edge (a, b) with ((dx*dx + dy*dy) + dz*dz) > max_edge*max_edge in the vertices' dtype; NaN is False."""
    v = np.asarray(vertices)
    limit = v.dtype.type(max_edge)
    limit2 = limit * limit
    out = np.zeros(len(faces), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            d = v[faces[:, b]] - v[faces[:, a]]
            out |= ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > limit2
    return out


def generation(vertices, faces, colors, is_long):
    """One generation for the faces flagged long -> (vertices, faces, colors)."""
    n_v = len(vertices)
    lf = faces[is_long].astype(np.int64)                                       # the long faces, in their order
    a, b = lf.reshape(-1), lf[:, [1, 2, 0]].reshape(-1)                        # face-major slots (v0v1), (v1v2), (v2v0)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = (lo << 32) | hi
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                                   # unique keys in order of first appearance
    number = np.empty(len(uniq), dtype=np.int64)
    number[order] = np.arange(len(uniq))
    owner = first[order]                                                       # the slot that owns midpoint 0, 1, ...
    with np.errstate(invalid="ignore", over="ignore"):
        mid = (vertices[lo[owner]] + vertices[hi[owner]]) * vertices.dtype.type(0.5)
    new_v = np.concatenate([vertices, mid])
    new_c = None
    if colors is not None:
        mc = (colors[lo[owner]].astype(np.uint32) + colors[hi[owner]].astype(np.uint32) + 1) >> 1
        new_c = np.concatenate([colors, mc.astype(np.uint8)])
    m = (n_v + number[inverse.reshape(-1)]).reshape(-1, 3)
    v0, v1, v2 = lf[:, 0], lf[:, 1], lf[:, 2]
    m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
    children = np.stack([v0, m0, m2, m0, v1, m1, m2, m1, v2, m0, m1, m2], 1).reshape(-1, 3)
    return new_v, np.concatenate([faces[~is_long], children.astype(faces.dtype)]), new_c


def check_growth(n_faces, n_vertices, n_long, max_faces):
    nf, nv = n_faces + 3 * n_long, n_vertices + 3 * n_long
    if nf > max_faces:
        raise ValueError(f"subdivide: the next generation would have {nf} faces, more than max_faces = {max_faces}")
    if nv >= 2 ** 31:
        raise ValueError(f"subdivide: the next generation could have {nv} vertices; indices are int32")


def subdivide_to_size(vertices, faces, max_edge, colors=None, max_iter=10, max_faces=2 ** 27):
    """-> (vertices in their dtype, faces int32 [F',3], colors or None, generations, remaining_long)."""
    v = np.ascontiguousarray(vertices).reshape(-1, 3)
    assert v.dtype in (np.float32, np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int32)
    c = None if colors is None else np.asarray(colors, dtype=np.uint8).reshape(-1, 4)
    generations = 0
    while True:
        is_long = long_faces(v, f, max_edge)
        n_long = int(is_long.sum())
        if n_long == 0 or generations >= max_iter:
            return v, f, c, generations, n_long
        check_growth(len(f), len(v), n_long, max_faces)
        v, f, c = generation(v, f, c, is_long)
        generations += 1


def cull_subdivided(vertices, faces, poses, cam, max_edge, colors=None, bounds=None, remove_occlusion=True, occluder=None, eps=0.03, near=0.01, far=10.0,
                    max_iter=10):
    """cull_mesh(max_edge=...) restated: the depth maps of the ORIGINAL mesh (its faces that survive the bounds, or the occluder), the
    vertex test, keep rule and compaction on the subdivided mesh -> ((vertices, faces, colors), depth or None, generations, remaining)."""
    import cull_spec as CS
    faces = np.asarray(faces).reshape(-1, 3)
    depth = None
    if remove_occlusion:
        if occluder is not None:
            depth = CS.render_depth(occluder[0], occluder[1], poses, cam, near, far)
        else:
            alive0 = None if bounds is None else CS.inside_bounds(vertices, bounds)[faces].any(1)
            depth = CS.render_depth(vertices, faces, poses, cam, near, far, face_mask=alive0)
    sv, sf, sc, generations, remaining = subdivide_to_size(vertices, faces, max_edge, colors, max_iter)
    alive = np.ones(len(sf), dtype=bool) if bounds is None else CS.inside_bounds(sv, bounds)[sf].any(1)
    _, seen = CS.vertex_tests(sv, poses, cam, depth, eps)
    keep = alive & seen.any(0)[sf].any(1)
    return CS.compact(sv, sf, keep, sc), depth, generations, remaining

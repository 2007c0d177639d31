"""CPU tests of the subdivision's numpy restatement (tests/subdivide_spec.py), of the host side of naruto_amd/remesh.py (argument
validation and the max_faces refusal, neither of which reaches the library) and of the new C ABI symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from naruto_amd import _lib
from naruto_amd import remesh as RM

import cull_spec as CS
import subdivide_spec as SD


def _area(v, f):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()


def _edges(v, f):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([np.linalg.norm(v[f[:, b]] - v[f[:, a]], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))])


def square():
    """Two triangles that share the diagonal of the unit square."""
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def long_short_pair():
    """A(0,0,0) B(0.5,0,0) C(0,3,0), long at 0.6, next to A B D(0.25,-0.4,0), short at 0.6 (its edges: 0.5, 0.4717, 0.4717)."""
    return np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 3.0, 0.0], [0.25, -0.4, 0.0]]), np.array([[1, 0, 3], [0, 1, 2]], dtype=np.int32)


def nan_pair():
    """A(0,0,0) B(0.1,0,0) with a NaN vertex, and A B E(0,2,0)."""
    return np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [np.nan, 5.0, 0.0], [0.0, 2.0, 0.0]]), np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32)


@pytest.fixture(scope="module")
def room():
    v, f = CS.room_mesh()
    return v, f


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_room_area_edges_prefix_and_counts(room, dtype):
    """The room at 0.25: the issue's counts; area unchanged to 1e-12 relative (float64 vertices; the float32 run is held to the float32
    rounding of its midpoints, 1e-6); every edge <= max_edge; the input's vertices are a prefix; the sphere's faces are untouched."""
    v, f = room[0].astype(dtype), room[1]
    sv, sf, sc, gens, rem = SD.subdivide_to_size(v, f, 0.25)
    assert (gens, rem, len(sf), len(sv)) == (5, 0, 14497, 7252) and sc is None and sv.dtype == dtype and sf.dtype == np.int32
    assert np.array_equal(sv[:len(v)].view(np.uint8), v.view(np.uint8))
    rel = abs(_area(sv, sf) - _area(v, f)) / _area(v, f)
    print("relative area change", rel)
    assert rel <= (1e-12 if dtype is np.float64 else 1e-6)
    assert _edges(sv, sf).max() <=0.25 * (1 + (1e-12 if dtype is np.float64 else 1e-6))
    short0 = ~SD.long_faces(v, f, 0.25)
    assert short0.sum() == len(f) - 12 and np.array_equal(sf[:short0.sum()], f[short0])          # the sphere: first, in order, unchanged
    # every face references existing vertices and every vertex is referenced
    assert sf.min() == 0 and sf.max() == len(sv) - 1 and len(np.unique(sf)) == len(sv)


def test_room_at_other_sizes(room):
    v, f = room
    sv, sf, _, gens, rem = SD.subdivide_to_size(v, f, 0.1)
    assert (gens, rem, len(sf), len(sv)) == (7, 0, 156292, 78405)
    first = SD.long_faces(v, f, 0.12)[12:-1]
    assert first.any() and not first.all()                                    # split and unsplit sphere faces: T-junctions


def test_shared_edge_is_welded():
    v, f = square()
    col = np.array([[0, 10, 255, 255], [1, 20, 255, 0], [3, 31, 254, 255], [200, 0, 0, 1]], dtype=np.uint8)
    sv, sf, sc, gens, rem = SD.subdivide_to_size(v, f, 0.8, col, max_iter=1)
    assert gens == 1 and len(sv) == 9 and len(sf) == 8 and rem == 0           # (children's edges: 0.5 and 0.7071)
    # first appearance: (0,1) (1,2) (2,0) of face 0, then (2,3) (3,0) of face 1 -- its (0,2) is face 0's (2,0)
    assert np.array_equal(sv[4:], [[0.5, 0, 0], [1, 0.5, 0], [0.5, 0.5, 0], [0.5, 1, 0], [0, 0.5, 0]])
    assert np.array_equal(sf, [[0, 4, 6], [4, 1, 5], [6, 5, 2], [4, 5, 6], [0, 6, 8], [6, 2, 7], [8, 7, 3], [6, 7, 8]])
    assert np.array_equal(sc[4:], [[1, 15, 255, 128], [2, 26, 255, 128], [2, 21, 255, 255], [102, 16, 127, 128], [100, 5, 128, 128]])
    assert abs(_area(sv, sf) - 1.0) <= 1e-12
    n = np.cross(sv[sf[:, 1]] - sv[sf[:, 0]], sv[sf[:, 2]] - sv[sf[:, 0]])
    assert (n[:, 2] > 0).all()                                                # the winding is preserved


def test_an_edge_of_exactly_max_edge_is_not_split():
    """A 3-4-5 triangle with sides 0.75, 1 and 1.25, all exact in both types: at max_edge = 1.25 nothing is split, one unit in the last
    place of the type below it the face is."""
    v, f = np.array([[0.0, 0.0, 0.0], [0.75, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]], dtype=np.int32)
    for dtype in (np.float32, np.float64):
        sv, sf, _, gens, rem = SD.subdivide_to_size(v.astype(dtype), f, 1.25)
        assert (gens, rem) == (0, 0) and np.array_equal(sf, f) and np.array_equal(sv, v), dtype
        below = float(np.nextafter(dtype(1.25), dtype(0)))
        sv, sf, _, gens, rem = SD.subdivide_to_size(v.astype(dtype), f, below)
        assert (gens, rem, len(sf), len(sv)) == (1, 0, 4, 6), dtype
    # max_edge is converted to the vertices' type once: the float64 neighbour of 1.25 is 1.25 in float32
    assert SD.subdivide_to_size(v.astype(np.float32), f, float(np.nextafter(1.25, 0.0)))[3] == 0


def test_max_iter_zero_returns_the_input(room):
    v, f = room
    sv, sf, _, gens, rem = SD.subdivide_to_size(v, f, 0.25, max_iter=0)
    assert gens == 0 and rem == 12 and np.array_equal(sv, v) and np.array_equal(sf, f)
    _, sf1, _, gens, rem = SD.subdivide_to_size(v, f, 0.25, max_iter=1)
    assert gens == 1 and rem == 48 and len(sf1) == len(f) + 36


def test_long_face_next_to_a_short_one():
    v, f = long_short_pair()
    assert SD.long_faces(v, f, 0.6).tolist() == [False, True]
    sv, sf, _, gens, rem = SD.subdivide_to_size(v, f, 0.6, max_iter=1)
    assert gens == 1 and np.array_equal(sf[0], f[0]) and np.array_equal(sv[:4], v)
    assert np.array_equal(sv[4], [0.25, 0.0, 0.0])                            # the midpoint of AB, slot 0 of the long face
    assert (sf[1:] == 4).any(1).sum() == 3 and not (sf[0] == 4).any()         # used by the long side only: a T-junction
    sv, sf, _, gens, rem = SD.subdivide_to_size(v, f, 0.6)
    assert rem == 0 and np.array_equal(sf[0], f[0]) and _edges(sv, sf).max() <= 0.6
    assert abs(_area(sv, sf) - _area(v, f)) <= 1e-12 * _area(v, f)


def test_nan_vertices_are_never_split():
    """A face whose only finite edge is short has no edge that compares longer: it is never split, whatever its neighbour does."""
    v, f = nan_pair()
    assert SD.long_faces(v, f, 0.8).tolist() == [False, True]
    sv, sf, _, gens, rem = SD.subdivide_to_size(v, f, 0.8)
    assert rem == 0 and gens == 2 and np.array_equal(sf[0], f[0]) and len(sf) == 1 + 16
    inf = square()[0].copy()
    inf[:, 0] = np.inf                                                        # inf - inf = NaN
    assert not SD.long_faces(inf, f, 0.8).any()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def test_max_faces_refusal_names_the_count_and_calls_nothing(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: _NoLibrary())
    with pytest.raises(ValueError, match="5 faces.*max_faces = 4"):
        RM.check_growth(2, 4, 1, 4)
    RM.check_growth(2, 4, 1, 5)
    with pytest.raises(ValueError, match="2147483648 vertices"):
        RM.check_growth(10, 2 ** 31 - 3, 1, 2 ** 40)
    v, f = square()
    with pytest.raises(ValueError, match="8 faces.*max_faces = 7"):
        SD.subdivide_to_size(v, f, 0.8, max_faces=7)
    assert len(SD.subdivide_to_size(v, f, 0.8, max_faces=8)[1]) == 8


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    """Nothing below reaches a device or the library: the test runs without a GPU and the library is replaced by one that refuses every call."""
    from naruto_amd import culling as CU
    monkeypatch.setattr(_lib, "load", lambda: _NoLibrary())
    v, f = square()
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="max_edge"):
            RM.subdivide_to_size((v, f), bad)
    with pytest.raises(ValueError, match="max_iter"):
        RM.subdivide_to_size((v, f), 0.5, max_iter=-1)
    with pytest.raises(ValueError, match="max_iter"):
        RM.subdivide_to_size((v, f), 0.5, max_iter=1.5)
    with pytest.raises(ValueError, match="max_faces"):
        RM.subdivide_to_size((v, f), 0.5, max_faces=0)
    with pytest.raises(ValueError, match="2 cells"):
        RM.subdivide_to_size((v, f), 0.5, plan=RM.SubdividePlan(1.5))
    with pytest.raises(ValueError, match="out of range"):
        RM.subdivide_to_size((v, np.array([[0, 1, 4]])), 0.5)
    with pytest.raises(ValueError, match="out of range"):
        RM.subdivide_to_size((v, np.array([[0, -1, 2]])), 0.5)
    with pytest.raises(ValueError, match="without faces"):
        RM.subdivide_to_size((v, np.zeros((0, 3), dtype=np.int32)), 0.5)
    with pytest.raises(ValueError, match="colour per vertex"):
        RM.subdivide_to_size((v, f, np.zeros((3, 4), dtype=np.uint8)), 0.5)
    with pytest.raises(ValueError, match="a mesh is"):
        RM.subdivide_to_size(v, 0.5)
    poses, cam = np.eye(4, dtype=np.float32)[None], CS.camera()
    with pytest.raises(ValueError, match="max_edge"):
        CU.cull_mesh((v, f), poses, cam, max_edge=0.0)
    with pytest.raises(ValueError, match="max_iter"):
        CU.cull_mesh((v, f), poses, cam, max_edge=0.5, max_iter=-2)
    assert RM.table_slots(1) == RM.MIN_TABLE_SLOTS and RM.table_slots(1000) == 6000 and RM.table_slots(1000, {"table_factor": 3}) == 9000


def test_new_abi_symbols_are_declared_and_exported(built_lib):
    header = open(_lib.HEADER).read()
    want = {
        "naruto_subdivide_workspace": (C.c_size_t, 2),
        "naruto_subdivide_mark": (C.c_int, 8),
        "naruto_subdivide_edges": (C.c_int, 10),
        "naruto_subdivide_emit": (C.c_int, 15),
    }
    for name, (res, n_args) in want.items():
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert _lib.SIGNATURES[name][0] is res and len(_lib.SIGNATURES[name][1]) == n_args, name
        fn = getattr(built_lib, name)
        assert fn.restype is res and len(fn.argtypes) == n_args
        decl = header[header.index(name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args, name
    assert "naruto_subdiv.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "naruto_subdiv.hip"))
    ws = built_lib.naruto_subdivide_workspace
    assert ws(0, 64) == 0 and ws(10, 59) == 0 and ws(10, 2 ** 31 + 1) == 0 and ws((2 ** 31 - 1) // 3 + 1, 2 ** 31) == 0
    assert ws(10, 60) >= 4 + 60 * 12 + 30 * 4 and ws(10, 120) > ws(10, 60) and ws(1, 2 ** 31) >= 12 * 2 ** 31


def test_abi_argument_checks_return_errors_without_a_launch(built_lib):
    one = C.c_void_p(8)                                                        # never dereferenced: every call below fails its checks first
    big = 2 ** 31
    assert built_lib.naruto_subdivide_mark(1, 3, None, one, 0, 0.5, one, None) != 0
    assert built_lib.naruto_subdivide_mark(1, 3, one, one, 0, 0.0, one, None) != 0
    assert built_lib.naruto_subdivide_mark(1, 3, one, one, 1, float("nan"), one, None) != 0
    assert built_lib.naruto_subdivide_mark(big, 3, one, one, 0, 0.5, one, None) != 0
    assert b"subdivide_mark" in built_lib.naruto_last_error()
    assert built_lib.naruto_subdivide_edges(4, 6, one, one, one, 2, 11, one, one, None) != 0          # a table more than half full
    assert built_lib.naruto_subdivide_edges(4, 6, one, one, one, 5, 64, one, one, None) != 0          # more long faces than faces
    assert built_lib.naruto_subdivide_edges(4, 6, one, one, one, 0, 64, one, one, None) != 0
    assert built_lib.naruto_subdivide_edges(4, 6, one, one, one, 2, 64, None, one, None) != 0
    assert built_lib.naruto_subdivide_edges(big, 6, one, one, one, 2, 64, one, one, None) != 0
    assert b"subdivide_edges" in built_lib.naruto_last_error()
    assert built_lib.naruto_subdivide_emit(4, 6, one, one, one, 2, 64, one, one, 7, one, 0, None, one, None) != 0       # more midpoints than slots
    assert built_lib.naruto_subdivide_emit(4, 6, one, one, one, 2, 64, one, one, 0, one, 0, None, one, None) != 0
    assert built_lib.naruto_subdivide_emit(4, big - 3, one, one, one, 2, 64, one, one, 5, one, 0, None, one, None) != 0 # vertices reach 2^31
    assert built_lib.naruto_subdivide_emit(4, 6, one, one, one, 2, 64, one, one, 5, None, 0, None, one, None) != 0
    assert built_lib.naruto_subdivide_emit(4, 6, one, one, one, 2, 64, one, one, 5, one, 0, None, None, None) != 0
    assert b"subdivide_emit" in built_lib.naruto_last_error()

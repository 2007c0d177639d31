"""The glTF loader (naruto_amd/gltf.py) and the texture restatement's own properties, without a GPU: a scene this file writes as .glb and
as .gltf with data URIs comes back as exactly the arrays it was made from; the PNG decoder over every row filter and colour type; every
refusal; the command lines' gates."""
import copy
import json
import struct

import numpy as np
import pytest

import gltf_scene as GS
import sim_texture_spec as TS
from naruto_amd import gltf as G
from naruto_amd.mesh import Material, Mesh, TexturedMesh


@pytest.fixture(scope="module")
def scene():
    return GS.loader_scene()


def _check(mesh, expect, frame="gltf"):
    assert isinstance(mesh, TexturedMesh) and isinstance(mesh, Mesh)
    want_v = expect["vertices"]
    if frame == "mp3d":
        want_v = np.stack([want_v[:, 0], -want_v[:, 2], want_v[:, 1]], -1)
    assert mesh.vertices.dtype == np.float64 and np.array_equal(mesh.vertices, want_v)
    assert mesh.faces.dtype == np.int64 and np.array_equal(mesh.faces, expect["faces"])
    assert mesh.uv.dtype == np.float32 and np.array_equal(mesh.uv, expect["uv"])
    assert mesh.vertex_colors.dtype == np.uint8 and np.array_equal(mesh.vertex_colors, expect["colors"])
    assert mesh.face_material.dtype == np.int32 and np.array_equal(mesh.face_material, expect["face_material"])
    assert [(m.texture, m.wrap_s, m.wrap_t, tuple(m.factor)) for m in mesh.materials] == expect["materials"]
    assert len(mesh.textures) == len(expect["textures"])
    for got, want in zip(mesh.textures, expect["textures"]):
        assert got.dtype == np.uint8 and np.array_equal(got, want)


@pytest.mark.parametrize("kind", ["glb", "gltf"])
def test_the_scene_comes_back_exactly(tmp_path, scene, kind):
    doc, blob, expect = scene
    path = GS.write_glb(tmp_path / "s.glb", doc, blob) if kind == "glb" else GS.write_gltf(tmp_path / "s.gltf", doc, blob)
    if kind == "gltf":
        text = json.load(open(path))
        assert text["buffers"][0]["uri"].startswith("data:") and all(i["uri"].startswith("data:") for i in text["images"])
    _check(G.load_gltf(path), expect)
    _check(G.load_gltf(path, frame="mp3d"), expect, "mp3d")
    _check(Mesh.load(path), expect)                                            # the dispatch on the extension
    with pytest.raises(ValueError, match="frame"):
        G.load_gltf(path, frame="habitat")


def test_external_files_and_no_default_scene(tmp_path, scene):
    """A .gltf that points to a .bin and an image file beside it; without `scene` and `scenes` every root node is walked."""
    doc, blob, expect = scene
    doc = copy.deepcopy(doc)
    (tmp_path / "data.bin").write_bytes(blob)
    doc["buffers"][0]["uri"] = "data.bin"
    v = doc["bufferViews"][doc["images"][0].pop("bufferView")]
    (tmp_path / "image 0.png").write_bytes(blob[v["byteOffset"]:v["byteOffset"] + v["byteLength"]])
    doc["images"][0]["uri"] = "image%200.png"
    del doc["scene"], doc["scenes"]
    (tmp_path / "s.gltf").write_text(json.dumps(doc))
    _check(G.load_gltf(tmp_path / "s.gltf"), expect)


def test_mesh_load_still_reads_ply_and_culling_takes_the_geometry(tmp_path, scene):
    from naruto_amd import culling as CU
    doc, blob, expect = scene
    path = GS.write_glb(tmp_path / "s.glb", doc, blob)
    v, f, col, kind = CU._as_mesh(path)
    assert kind == "mesh" and np.array_equal(v, expect["vertices"]) and np.array_equal(f, expect["faces"]) and np.array_equal(col, expect["colors"])
    Mesh(expect["vertices"], expect["faces"]).export(str(tmp_path / "m.ply"))
    back = Mesh.load(str(tmp_path / "m.ply"))
    assert type(back) is Mesh and np.array_equal(back.faces, expect["faces"])


# ---- PNG ---------------------------------------------------------------------------------------------------------------------------------
def _as_rgba(samples, ctype, palette=None, palette_alpha=None):
    s = samples
    h, w = s.shape[:2]
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    if ctype == 0:
        out[..., :3] = s
    elif ctype == 4:
        out[..., :3], out[..., 3] = s[..., :1], s[..., 1]
    elif ctype == 2:
        out[..., :3] = s
    elif ctype == 6:
        out[...] = s
    else:
        out[..., :3] = palette[s[..., 0]]
        if palette_alpha is not None:
            a = np.full(len(palette), 255, dtype=np.uint8)
            a[:len(palette_alpha)] = palette_alpha
            out[..., 3] = a[s[..., 0]]
    return out


PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


@pytest.mark.parametrize("ctype", [0, 2, 3, 4, 6])
@pytest.mark.parametrize("row_filter", [0, 1, 2, 3, 4, "mixed"])
def test_png_decoder_returns_the_source(ctype, row_filter):
    rng = np.random.default_rng(ctype * 10 + (5 if row_filter == "mixed" else row_filter))
    h, w = 7, 9
    palette = rng.integers(0, 256, (6, 3), dtype=np.uint8) if ctype == 3 else None
    alpha = np.array([0, 128, 7], dtype=np.uint8) if ctype == 3 else None
    s = rng.integers(0, 6 if ctype == 3 else 256, (h, w, PNG_CHANNELS[ctype]), dtype=np.uint8)
    kinds = [(r * 3 + 1) % 5 for r in range(h)] if row_filter == "mixed" else row_filter
    data = GS.encode_png(s, ctype, kinds, palette=palette, palette_alpha=alpha)
    want = _as_rgba(s, ctype, palette, alpha)
    assert G.png_decodable(data)
    got = G.decode_png(data)
    assert got.dtype == np.uint8 and got.shape == (h, w, 4) and np.array_equal(got, want)
    assert np.array_equal(G.decode_image(data), want)


@pytest.mark.parametrize("ctype", [0, 2, 3, 4, 6])
def test_png_decoder_equals_pil(ctype):
    """Skipped where PIL cannot be imported."""
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(100 + ctype)
    palette = rng.integers(0, 256, (6, 3), dtype=np.uint8) if ctype == 3 else None
    alpha = np.array([0, 128, 7], dtype=np.uint8) if ctype == 3 else None
    s = rng.integers(0, 6 if ctype == 3 else 256, (7, 9, PNG_CHANNELS[ctype]), dtype=np.uint8)
    data = GS.encode_png(s, ctype, [(r * 3 + 1) % 5 for r in range(7)], palette=palette, palette_alpha=alpha)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGBA")), G.decode_png(data))


def test_png_refusals(monkeypatch):
    s = np.zeros((2, 2, 4), dtype=np.uint8)
    good = GS.png_rgba(s)
    with pytest.raises(ValueError, match="truncated"):
        G.decode_png(good[:40])
    with pytest.raises(ValueError, match="truncated"):
        G.decode_png(good[:-12])                                               # no IEND
    with pytest.raises(ValueError, match="not a PNG"):
        G.decode_png(b"GIF89a" + good)
    bad_filter = GS.encode_png(s, 6, 0)
    with pytest.raises(ValueError, match="row filter"):
        import zlib
        raw = bytearray(b"\x07" + bytes(8) + b"\x00" + bytes(8))
        z = zlib.compress(bytes(raw))
        head = bad_filter[:33]
        G.decode_png(head + GS._chunk(b"IDAT", z) + GS._chunk(b"IEND", b""))
    # what the decoder does not read goes to PIL; without PIL it is an error that says so
    interlaced = GS.encode_png(s, 6, 0, interlace=1)
    sixteen = GS.encode_png(np.zeros((2, 4, 4), dtype=np.uint8), 6, 0, bit_depth=16)
    assert not G.png_decodable(interlaced) and not G.png_decodable(sixteen)
    monkeypatch.setattr(G, "_pil", lambda: None)
    for data in (interlaced, sixteen, b"\xff\xd8\xff\xe0" + bytes(20)):
        with pytest.raises(ValueError, match="PIL"):
            G.decode_image(data, "images[0]")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _load(tmp_path, doc, blob, name="bad.glb"):
    return G.load_gltf(GS.write_glb(tmp_path / name, doc, blob))


@pytest.mark.parametrize("ext", ["KHR_draco_mesh_compression", "KHR_texture_basisu", "KHR_texture_transform"])
def test_required_extensions_are_refused(tmp_path, scene, ext):
    doc = copy.deepcopy(scene[0])
    doc["extensionsRequired"] = ["KHR_materials_unlit", ext]
    with pytest.raises(ValueError, match=ext):
        _load(tmp_path, doc, scene[1])


def test_refusals_name_the_item(tmp_path, scene, monkeypatch):
    doc0, blob0, _ = scene
    pos_a = doc0["meshes"][1]["primitives"][0]["attributes"]["POSITION"]
    uv_a = doc0["meshes"][1]["primitives"][0]["attributes"]["TEXCOORD_1"]
    idx_a = doc0["meshes"][1]["primitives"][0]["indices"]

    def offset(doc, accessor):
        a = doc["accessors"][accessor]
        return doc["bufferViews"][a["bufferView"]]["byteOffset"] + a.get("byteOffset", 0)

    # a sparse accessor
    doc = copy.deepcopy(doc0)
    doc["accessors"][pos_a]["sparse"] = {"count": 1, "indices": {"bufferView": 0, "componentType": 5123}, "values": {"bufferView": 0}}
    with pytest.raises(ValueError, match=rf"accessors\[{pos_a}\].*sparse"):
        _load(tmp_path, doc, blob0)
    # a primitive of lines
    doc = copy.deepcopy(doc0)
    doc["meshes"][1]["primitives"][1]["mode"] = 1
    with pytest.raises(ValueError, match=r"meshes\[1\]\.primitives\[1\] has mode 1"):
        _load(tmp_path, doc, blob0)
    # an index out of range
    blob = bytearray(blob0)
    struct.pack_into("<I", blob, offset(doc0, idx_a) + 8, 4)
    with pytest.raises(ValueError, match=r"meshes\[1\]\.primitives\[0\]: index 4 out of range for 4"):
        _load(tmp_path, doc0, bytes(blob))
    # a position that is not finite
    for bad in (float("nan"), float("inf")):
        blob = bytearray(blob0)
        struct.pack_into("<f", blob, offset(doc0, pos_a) + 16, bad)
        with pytest.raises(ValueError, match=r"meshes\[1\]\.primitives\[0\]: non-finite position"):
            _load(tmp_path, doc0, bytes(blob))
    # |uv| > 1024
    blob = bytearray(blob0)
    struct.pack_into("<f", blob, offset(doc0, uv_a) + 4, -1024.5)
    with pytest.raises(ValueError, match=r"TEXCOORD_1.*1024"):
        _load(tmp_path, doc0, bytes(blob))
    struct.pack_into("<f", blob, offset(doc0, uv_a) + 4, -1024.0)              # the bound itself is read
    _load(tmp_path, doc0, bytes(blob))
    # an accessor that runs past its view; a view past its buffer; a buffer shorter than it says
    doc = copy.deepcopy(doc0)
    doc["accessors"][pos_a]["count"] = 5
    with pytest.raises(ValueError, match=rf"accessors\[{pos_a}\].*truncated"):
        _load(tmp_path, doc, blob0)
    doc = copy.deepcopy(doc0)
    doc["bufferViews"][-1]["byteLength"] += 64
    with pytest.raises(ValueError, match=rf"bufferViews\[{len(doc['bufferViews']) - 1}\] is truncated"):
        _load(tmp_path, doc, blob0)
    doc = copy.deepcopy(doc0)
    doc["buffers"][0]["byteLength"] += 64
    with pytest.raises(ValueError, match=r"buffers\[0\] is truncated"):
        _load(tmp_path, doc, blob0)
    # an image with a side above 16384: refused on its header, before anything is decoded
    big = GS.encode_png(np.zeros((1, 1, 4), dtype=np.uint8), 6, 0)
    big = big[:16] + struct.pack(">II", 16385, 1) + big[24:]
    doc = copy.deepcopy(doc0)
    b2 = bytearray(blob0) + b"\0" * (-len(blob0) % 4)
    doc["bufferViews"].append({"buffer": 0, "byteOffset": len(b2), "byteLength": len(big)})
    doc["images"][0] = {"bufferView": len(doc["bufferViews"]) - 1, "mimeType": "image/png"}
    doc["buffers"][0]["byteLength"] = len(b2) + len(big)
    with pytest.raises(ValueError, match=r"images\[0\].*16385 x 1"):
        _load(tmp_path, doc, bytes(b2) + big)
    # a JPEG where PIL cannot be imported
    jpeg = b"\xff\xd8\xff\xe0" + bytes(32)
    doc = copy.deepcopy(doc0)
    doc["bufferViews"].append({"buffer": 0, "byteOffset": len(b2), "byteLength": len(jpeg)})
    doc["images"][1] = {"bufferView": len(doc["bufferViews"]) - 1, "mimeType": "image/jpeg"}
    doc["buffers"][0]["byteLength"] = len(b2) + len(jpeg)
    monkeypatch.setattr(G, "_pil", lambda: None)
    with pytest.raises(ValueError, match=r"images\[1\].*JPEG needs PIL"):
        _load(tmp_path, doc, bytes(b2) + jpeg)


def test_truncated_containers(tmp_path, scene):
    doc, blob, _ = scene
    data = GS.glb_bytes(doc, blob)
    for cut, what in ((8, "truncated GLB header"), (16, "truncated GLB"), (len(data) - 40, "truncated GLB"), (len(data) - 1, "truncated GLB")):
        p = tmp_path / f"cut{cut}.glb"
        p.write_bytes(data[:cut])
        with pytest.raises(ValueError, match=what):
            G.load_gltf(p)
    # the file is whole, a chunk says it is longer than the file
    js_len = struct.unpack("<I", data[12:16])[0]
    bad = bytearray(data)
    struct.pack_into("<I", bad, 12 + 8 + js_len, len(blob) + 400)
    (tmp_path / "long.glb").write_bytes(bytes(bad))
    with pytest.raises(ValueError, match="truncated GLB chunk"):
        G.load_gltf(tmp_path / "long.glb")
    (tmp_path / "v1.glb").write_bytes(data[:4] + struct.pack("<I", 1) + data[8:])
    with pytest.raises(ValueError, match="version 1"):
        G.load_gltf(tmp_path / "v1.glb")
    (tmp_path / "text.gltf").write_text("{ not json")
    with pytest.raises(ValueError, match="neither"):
        G.load_gltf(tmp_path / "text.gltf")


def test_command_lines_take_gltf_and_still_refuse_obj():
    from naruto_amd import culling as CU
    from naruto_amd import evaluation as E
    from naruto_amd import render as RD
    from naruto_amd import run as R
    run = ["--config", "c.yaml", "--num_iter", "3", "--result_dir", "out", "--mesh"]
    view = ["--config", "c.yaml", "--ckpt", "k.pt", "--poses", "--out_dir", "o", "--mesh"]
    for name in ("scene.glb", "scene.GLTF"):
        a = R.parse_args(run + [name])
        assert a.mesh == name and a.mesh_frame == "gltf"
        assert R.parse_args(run + [name, "--dataset", "MP3D"]).mesh_frame == "mp3d"
        assert R.parse_args(run + [name, "--dataset", "MP3D", "--mesh_frame", "gltf"]).mesh_frame == "gltf"
        assert RD.parse_args(view + [name]).mesh == name
    assert R.parse_args(run + ["scene.ply", "--dataset", "MP3D"]).mesh_frame == "gltf"
    for parse, args in ((R.parse_args, run), (RD.parse_args, view)):
        with pytest.raises(SystemExit):
            parse(args + ["scene.obj"])
    with pytest.raises(ValueError, match="obj"):
        E.main(["--rec_mesh", "a.ply", "--gt_mesh", "scene.obj"])
    with pytest.raises(ValueError, match="only"):
        CU.main(["--config", "c.yaml", "--input_mesh", "scene.obj", "--ckpt_path", "c.pt"])


# ---- the restatement's own properties ---------------------------------------------------------------------------------------------------------
def test_twin_pyramid_of_a_constant_image_is_constant():
    for h, w in ((1, 1), (5, 3), (64, 16), (16, 64), (7, 1)):
        im = np.tile(np.array([3, 128, 255, 77], dtype=np.uint8), (h, w, 1))
        chain = TS.pyramid(im)
        assert len(chain) == TS.n_levels(w, h) == 1 + int(np.floor(np.log2(max(w, h))))
        size = (h, w)
        for lv in chain:
            assert lv.shape == size + (4,) and (lv == im[0, 0]).all()
            size = (max(1, size[0] >> 1), max(1, size[1] >> 1))
    words, desc = TS.pyramid_buffer([TS.hashed_image(5, 3, 1), TS.hashed_image(1, 1, 2)])
    assert desc.tolist() == [[0, 3, 5, 3], [15 + 2 + 1, 1, 1, 1]] and len(words) == 4 * 19
    # rounding half up, per channel: (0 + 0 + 1 + 1 + 2) >> 2 = 1, (255 * 4 + 2) >> 2 = 255
    im = np.array([[[0, 255, 1, 2]], [[1, 255, 2, 3]]], dtype=np.uint8)
    assert TS.pyramid(im)[1].tolist() == [[[1, 255, 2, 3]]]


def test_twin_level_is_monotone_and_exact_at_the_powers():
    rho2 = np.concatenate([[0.0, np.nan], np.float32(2.0) ** np.arange(-4, 40, dtype=np.float32), [np.inf]]).astype(np.float32)
    for levels in (1, 2, 5, 12, 15):
        lv = TS.level(rho2, levels)
        assert lv[1] == 0 and lv[0] == 0 and lv[-1] == levels - 1
        assert (np.diff(lv[2:]) >= 0).all() and lv.min() == 0 and lv.max() == levels - 1
        for k in range(levels - 1):
            p = np.float32(4.0) ** k
            assert TS.level(p, levels) == k and TS.level(np.nextafter(p, np.float32(np.inf)), levels) == k + 1     # the comparison is strict


@pytest.mark.parametrize("w", [1, 2, 5, 8])
def test_twin_wraps_land_inside(w):
    i = np.arange(-2 * w - 1, 2 * w + 2)
    rep, mir, cl = (TS.wrap(i, w, m) for m in TS.WRAPS)
    for got in (rep, mir, cl):
        assert got.min() >= 0 and got.max() < w
    assert np.array_equal(rep, [k % w for k in i])
    assert np.array_equal(cl, [min(max(k, 0), w - 1) for k in i])
    period = list(range(w)) + list(range(w - 1, -1, -1))
    assert np.array_equal(mir, [period[k % (2 * w)] for k in i])


def test_twin_tap_at_texel_centres_and_beyond():
    im = TS.hashed_image(4, 8, 3)
    jj, ii = np.meshgrid(np.arange(4), np.arange(8), indexing="ij")
    u, v = ((ii + 0.5) / 8).astype(np.float32), ((jj + 0.5) / 4).astype(np.float32)
    got = TS.tap(im, u, v, GS.REPEAT, GS.REPEAT)
    assert np.array_equal(got, im[..., :3].astype(np.float32) / np.float32(255))                # (0.5 / 8 etc. are exact: a = b = 0)
    far = np.array([np.nan, np.inf, 3e9, -3e9], dtype=np.float32)
    assert (TS.tap(im, far, np.zeros(4, dtype=np.float32), GS.REPEAT, GS.CLAMP_TO_EDGE) == 0).all()
    seen = set()
    TS.tap(im, np.float32([-0.3]), np.float32([0.5]), GS.MIRRORED_REPEAT, GS.CLAMP_TO_EDGE, seen)
    assert seen == {("s", GS.MIRRORED_REPEAT)}


def test_textured_mesh_is_built_from_arrays():
    m = TexturedMesh(np.zeros((3, 3)), np.array([[0, 1, 2]]), None, uv=np.zeros((3, 2), dtype=np.float32), face_material=np.array([0], dtype=np.int32),
                     materials=[Material(texture=0)], textures=[np.zeros((1, 1, 4), dtype=np.uint8)])
    assert m.materials[0].wrap_s == GS.REPEAT and m.materials[0].factor == (1.0, 1.0, 1.0, 1.0) and m.vertex_colors is None
    assert TexturedMesh(np.zeros((3, 3)), np.array([[0, 1, 2]])).materials == []

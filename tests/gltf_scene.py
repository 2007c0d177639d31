"""glTF files written with struct, json and zlib alone, for tests/test_gltf_host.py and tests/test_gpu_sim_textured.py: a PNG encoder with a
chosen row filter and colour type, a GLB / .gltf writer, and a small scene that uses every feature naruto_amd/gltf.py reads."""
import base64
import json
import struct
import zlib

import numpy as np

REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = 10497, 33648, 33071


# ---- PNG -------------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _filter_row(kind, row, prev, bpp):
    out = bytearray(len(row))
    for k in range(len(row)):
        a = row[k - bpp] if k >= bpp else 0
        b = prev[k]
        c = prev[k - bpp] if k >= bpp else 0
        pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[kind]
        out[k] = (row[k] - pred) & 255
    return bytes(out)


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode_png(samples, colour_type, row_filter=0, palette=None, palette_alpha=None, interlace=0, bit_depth=8):
    """samples uint8 [H,W,C] with C the colour type's channels (0 grey: 1, 2 RGB: 3, 3 palette: 1, 4 grey + alpha: 2, 6 RGBA: 4);
    ``row_filter`` 0 .. 4 on every row, or a list with one filter per row."""
    s = np.asarray(samples, dtype=np.uint8)
    h, w, ch = s.shape
    kinds = [row_filter] * h if isinstance(row_filter, int) else list(row_filter)
    raw, prev = b"", bytes(w * ch)
    for r in range(h):
        row = s[r].tobytes()
        raw += bytes([kinds[r]]) + _filter_row(kinds[r], row, prev, ch)
        prev = row
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, colour_type, 0, 0, interlace))
    if palette is not None:
        out += _chunk(b"PLTE", np.asarray(palette, dtype=np.uint8).tobytes())
    if palette_alpha is not None:
        out += _chunk(b"tRNS", np.asarray(palette_alpha, dtype=np.uint8).tobytes())
    z = zlib.compress(raw)
    half = len(z) // 2                                            # two IDAT chunks: the decoder joins them
    return out + _chunk(b"IDAT", z[:half]) + _chunk(b"IDAT", z[half:]) + _chunk(b"IEND", b"")


def png_rgba(image, row_filter=4):
    return encode_png(np.asarray(image, dtype=np.uint8), 6, row_filter)


# ---- containers ------------------------------------------------------------------------------------------------------------------------
def glb_bytes(doc, blob=None):
    js = json.dumps(doc).encode("utf-8")
    js += b" " * (-len(js) % 4)
    chunks = struct.pack("<II", len(js), 0x4E4F534A) + js
    if blob is not None:
        blob = bytes(blob) + b"\0" * (-len(blob) % 4)
        chunks += struct.pack("<II", len(blob), 0x004E4942) + blob
    return struct.pack("<4sII", b"glTF", 2, 12 + len(chunks)) + chunks


def write_glb(path, doc, blob=None):
    with open(path, "wb") as f:
        f.write(glb_bytes(doc, blob))
    return str(path)


def data_uri(data, mime="application/octet-stream"):
    return f"data:{mime};base64," + base64.b64encode(bytes(data)).decode("ascii")


def write_gltf(path, doc, blob):
    """The same document as text: the buffer and every image that sits in a bufferView of it become base64 data URIs."""
    doc = json.loads(json.dumps(doc))
    doc["buffers"][0]["uri"] = data_uri(blob)
    for img in doc.get("images", []):
        if "bufferView" in img:
            v = doc["bufferViews"][img.pop("bufferView")]
            off = v.get("byteOffset", 0)
            img["uri"] = data_uri(blob[off:off + v["byteLength"]], img.get("mimeType", "image/png"))
    with open(path, "w") as f:
        json.dump(doc, f)
    return str(path)


class Builder:
    """Collects bufferViews and accessors over one growing buffer."""

    def __init__(self):
        self.blob, self.views, self.accessors = bytearray(), [], []

    def view(self, data, stride=None):
        self.blob += b"\0" * (-len(self.blob) % 4)
        v = {"buffer": 0, "byteOffset": len(self.blob), "byteLength": len(data)}
        if stride:
            v["byteStride"] = stride
        self.blob += bytes(data)
        self.views.append(v)
        return len(self.views) - 1

    def accessor(self, view, component, kind, count, offset=0, normalized=False, **more):
        a = {"bufferView": view, "componentType": component, "type": kind, "count": count, "byteOffset": offset}
        if normalized:
            a["normalized"] = True
        a.update(more)
        self.accessors.append(a)
        return len(self.accessors) - 1

    def array(self, arr, component, kind, normalized=False):
        arr = np.ascontiguousarray(arr)
        return self.accessor(self.view(arr.tobytes()), component, kind, len(arr), normalized=normalized)

    def document(self, **rest):
        doc = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(self.blob)}], "bufferViews": self.views, "accessors": self.accessors}
        doc.update(rest)
        return doc, bytes(self.blob)


# ---- the loader's scene ----------------------------------------------------------------------------------------------------------------------
QUAD = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32)
QUAD_UV16 = np.array([[0, 0], [65535, 0], [65535, 32768], [0, 32768]], dtype=np.uint16)
QUAD_IDX = np.array([0, 1, 2, 0, 2, 3])
NODE0_T, NODE0_S = [0.5, -1.0, 2.0], [2.0, 1.0, 0.5]            # with the rotation (0, 1, 0, 0): half a turn about y, exact in binary
NODE2_T = [0.0, 0.25, 0.0]
NODE1_M = np.array([[1, 0, 0, -3], [0, 0, -1, 0.5], [0, 1, 0, 1], [0, 0, 0, 1]], dtype=np.float64)


def loader_scene():
    """-> (document, buffer, expectation).  Two root nodes -- one TRS with a child, one with a matrix -- over two meshes, the first used
    twice: u16, u32 and u8 indices and a non-indexed primitive; interleaved attributes with a byteStride; normalised-u16 and float texture
    coordinates (the latter TEXCOORD_1); a textured, a factor-only and a specular-glossiness material and a primitive without one;
    COLOR_0 as normalised bytes; an RGBA and a palette PNG; a sampler with two wrap modes."""
    b = Builder()
    # mesh 0: one quad, position (12 bytes) and normalised-u16 uv (4 bytes) interleaved, u16 indices, material 0
    inter = b"".join(QUAD[i].tobytes() + QUAD_UV16[i].tobytes() for i in range(4))
    vi = b.view(inter, stride=16)
    a_pos0 = b.accessor(vi, 5126, "VEC3", 4, 0, min=[0, 0, 0], max=[1, 1, 0])
    a_uv0 = b.accessor(vi, 5123, "VEC2", 4, 12, normalized=True)
    a_idx0 = b.array(QUAD_IDX.astype(np.uint16), 5123, "SCALAR")
    # mesh 1: three primitives
    tri_a = np.array([[0, 0, 1], [2, 0, 1], [0, 2, 1], [2, 2, 1]], dtype=np.float32)
    uv_a = np.array([[-0.5, 0.25], [1.5, 0.25], [-0.5, 3.0], [1.5, 3.0]], dtype=np.float32)
    idx_a = np.array([0, 1, 2, 2, 1, 3])
    tri_b = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2]], dtype=np.float32)      # not indexed
    tri_c = np.array([[0, 0, 3], [1, 0, 3], [0, 1, 3]], dtype=np.float32)
    col_c = np.array([[255, 0, 0, 255], [0, 128, 0, 200], [10, 20, 30, 40]], dtype=np.uint8)
    a_pos_a, a_uv_a, a_idx_a = b.array(tri_a, 5126, "VEC3"), b.array(uv_a, 5126, "VEC2"), b.array(idx_a.astype(np.uint32), 5125, "SCALAR")
    a_pos_b = b.array(tri_b, 5126, "VEC3")
    a_pos_c, a_col_c, a_idx_c = b.array(tri_c, 5126, "VEC3"), b.array(col_c, 5121, "VEC4", normalized=True), b.array(np.array([2, 1, 0], dtype=np.uint8), 5121, "SCALAR")
    rng = np.random.default_rng(5)
    image0 = rng.integers(0, 256, (2, 4, 4), dtype=np.uint8)
    palette = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    index1 = rng.integers(0, 5, (3, 3, 1), dtype=np.uint8)
    image1 = np.concatenate([palette[index1[..., 0]], np.full((3, 3, 1), 255, dtype=np.uint8)], -1)
    v_img0, v_img1 = b.view(png_rgba(image0)), b.view(encode_png(index1, 3, 2, palette=palette))
    doc, blob = b.document(
        scene=0, scenes=[{"nodes": [0, 1]}],
        nodes=[{"mesh": 0, "translation": NODE0_T, "rotation": [0, 1, 0, 0], "scale": NODE0_S, "children": [2]},
               {"mesh": 1, "matrix": NODE1_M.T.reshape(-1).tolist()},
               {"mesh": 0, "translation": NODE2_T}],
        meshes=[{"primitives": [{"attributes": {"POSITION": a_pos0, "TEXCOORD_0": a_uv0}, "indices": a_idx0, "material": 0}]},
                {"primitives": [{"attributes": {"POSITION": a_pos_a, "TEXCOORD_1": a_uv_a}, "indices": a_idx_a, "material": 2},
                                {"attributes": {"POSITION": a_pos_b}, "material": 1, "mode": 4},
                                {"attributes": {"POSITION": a_pos_c, "COLOR_0": a_col_c}, "indices": a_idx_c}]}],
        materials=[{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "baseColorFactor": [1.0, 0.5, 0.25, 1.0]}, "extensions": {"KHR_materials_unlit": {}}},
                   {"pbrMetallicRoughness": {"baseColorFactor": [0.25, 0.5, 0.75, 1.0]}},
                   {"extensions": {"KHR_materials_pbrSpecularGlossiness": {"diffuseTexture": {"index": 1, "texCoord": 1}, "diffuseFactor": [0.5, 1.0, 1.0, 0.5]}}}],
        textures=[{"source": 0, "sampler": 0}, {"source": 1}],
        samplers=[{"wrapS": CLAMP_TO_EDGE, "wrapT": MIRRORED_REPEAT, "magFilter": 9728}],
        images=[{"bufferView": v_img0, "mimeType": "image/png"}, {"bufferView": v_img1, "mimeType": "image/png"}],
        extensionsUsed=["KHR_materials_unlit", "KHR_materials_pbrSpecularGlossiness"], extensionsRequired=["KHR_materials_unlit"])
    # the expectation, in the order of the walk: node 0 (mesh 0), its child node 2 (mesh 0), node 1 (mesh 1: three primitives)
    m0 = np.eye(4)
    m0[:3, :3] = np.diag([-1.0, 1.0, -1.0]) * np.array(NODE0_S)[None]
    m0[:3, 3] = NODE0_T
    m2 = m0.copy()
    m2[:3, 3] = m0[:3, :3] @ np.array(NODE2_T) + m0[:3, 3]
    world = lambda m, p: p.astype(np.float64) @ m[:3, :3].T + m[:3, 3]                                          # noqa: E731
    uv0 = QUAD_UV16.astype(np.float32) / np.float32(65535)
    zero = lambda n: np.zeros((n, 2), dtype=np.float32)                                                          # noqa: E731
    white = lambda n: np.full((n, 4), 255, dtype=np.uint8)                                                       # noqa: E731
    expect = {
        "vertices": np.concatenate([world(m0, QUAD), world(m2, QUAD), world(NODE1_M, tri_a), world(NODE1_M, tri_b), world(NODE1_M, tri_c)]),
        "faces": np.concatenate([QUAD_IDX.reshape(-1, 3), QUAD_IDX.reshape(-1, 3) + 4, idx_a.reshape(-1, 3) + 8, np.arange(6).reshape(-1, 3) + 12, np.array([[2, 1, 0]]) + 18]),
        "uv": np.concatenate([uv0, uv0, uv_a, zero(6), zero(3)]),
        "colors": np.concatenate([white(18), col_c]),
        "face_material": np.array([0, 0, 0, 0, 2, 2, 1, 1, -1], dtype=np.int32),
        "materials": [(0, CLAMP_TO_EDGE, MIRRORED_REPEAT, (1.0, 0.5, 0.25, 1.0)), (-1, REPEAT, REPEAT, (0.25, 0.5, 0.75, 1.0)), (1, REPEAT, REPEAT, (0.5, 1.0, 1.0, 0.5))],
        "textures": [image0, image1],
    }
    return doc, blob, expect


def room_glb(path, room, image):
    """A box over ``room`` [[x0,x1],[y0,y1],[z0,z1]] as a .glb: sim_spec.box_scene()'s 12 triangles under a node that scales and moves
    them, one texture (``image`` uint8 [H,W,4]) on every wall with uv in [-1, 3] and a mirrored sampler."""
    import sim_spec as SS
    v, f, _, _ = SS.box_scene()
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float32)
    uv = np.tile(corner * 4 - 1, (6, 1)).astype(np.float32)
    b = Builder()
    a_pos, a_uv, a_idx = b.array(v, 5126, "VEC3"), b.array(uv, 5126, "VEC2"), b.array(f.reshape(-1).astype(np.uint16), 5123, "SCALAR")
    v_img = b.view(png_rgba(image, row_filter=[r % 5 for r in range(len(image))]))
    room = np.asarray(room, dtype=np.float64)
    scale = (room[:, 1] - room[:, 0]) / (SS.BOX_HI - SS.BOX_LO)
    doc, blob = b.document(scenes=[{"nodes": [0]}], nodes=[{"mesh": 0, "scale": scale.tolist(), "translation": (room[:, 0] - SS.BOX_LO * scale).tolist()}],
                           meshes=[{"primitives": [{"attributes": {"POSITION": a_pos, "TEXCOORD_0": a_uv}, "indices": a_idx, "material": 0}]}],
                           materials=[{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}}}], textures=[{"source": 0, "sampler": 0}],
                           samplers=[{"wrapS": MIRRORED_REPEAT, "wrapT": MIRRORED_REPEAT}], images=[{"bufferView": v_img, "mimeType": "image/png"}])
    return write_glb(path, doc, blob)

"""glTF 2.0 scenes for the mesh simulator: ``.glb`` and ``.gltf`` -> :class:`naruto_amd.mesh.TexturedMesh`.

Half of the reference's scenes -- the MP3D and the NARUTO ones (``configs/MP3D/*/mp3d.stage_config.json``,
``configs/NARUTO/*/naruto.stage_config.json``) -- are textured ``.glb`` files that Habitat-Sim loads there.  This module reads them with the
standard library and numpy alone: the container (a ``.glb``'s JSON and BIN chunks; a ``.gltf`` with external files or base64 data URIs),
the default scene's node tree, triangle primitives, the texture coordinates the base-colour texture names, vertex colours, base-colour
materials with their samplers' wrap modes, and the images.

Read:
  * nodes       the default scene (``scene``, else scene 0, else every root node); ``matrix`` or TRS, composed in float64; a mesh that two
                nodes use appears twice
  * primitives  mode 4 (triangles); indices u8 / u16 / u32 or none; ``POSITION``; ``byteStride`` and accessor offsets honoured
  * uv          ``TEXCOORD_n`` with n the material's ``baseColorTexture.texCoord``; float, or normalised u8 / u16 (c / 255, c / 65535 in
                float32); a primitive whose material has no texture gets uv 0
  * colours     ``COLOR_0`` -> ``vertex_colors`` RGBA8 (vertices of primitives without it: opaque white)
  * materials   ``pbrMetallicRoughness.baseColorFactor`` / ``baseColorTexture``; without a base-colour texture, the ``diffuseFactor`` /
                ``diffuseTexture`` of ``KHR_materials_pbrSpecularGlossiness`` in their place; ``KHR_materials_unlit`` is accepted (nothing
                here is lit); the sampler's ``wrapS`` / ``wrapT`` (its filters are ignored: the simulator has one filter)
  * images      PNG by the decoder below (8-bit grey, grey + alpha, RGB, RGBA and palette, non-interlaced, all five row filters); JPEG and
                every other PNG through PIL when PIL can be imported; every image becomes uint8 [H,W,4]

Refused, with a ``ValueError`` that names the item: any other ``extensionsRequired`` (Draco, Basis, ``KHR_texture_transform`` ...), sparse
accessors, primitives of other modes, truncated chunks and buffers, indices out of range, non-finite positions, |uv| > 1024, an image with
a side above 16384.  Not read: normals, tangents, skins, animations, cameras, lights, alpha modes (everything renders opaque), texture
transforms.
"""

from __future__ import annotations

import base64
import json
import os
import struct
import zlib
from typing import Dict, List, Optional, Tuple

import numpy as np

from .mesh import Material, TexturedMesh

MAX_IMAGE_SIDE = 16384
MAX_UV = 1024.0
REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = 10497, 33648, 33071
_ACCEPTED_EXTENSIONS = ("KHR_materials_pbrSpecularGlossiness", "KHR_materials_unlit")
_COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT2": 4, "MAT3": 9, "MAT4": 16}
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


# ---- images --------------------------------------------------------------------------------------------------------------------------
def _png_header(data: bytes, what: str) -> Tuple[int, int, int, int, int]:
    """(W, H, bit depth, colour type, interlace) of a PNG's IHDR."""
    if len(data) < 33 or data[12:16] != b"IHDR":
        raise ValueError(f"{what}: truncated PNG")
    w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", data[16:29])
    return w, h, depth, ctype, interlace


def _check_side(w: int, h: int, what: str) -> None:
    if w < 1 or h < 1 or w > MAX_IMAGE_SIDE or h > MAX_IMAGE_SIDE:
        raise ValueError(f"{what}: an image of {w} x {h} (sides 1 .. {MAX_IMAGE_SIDE})")


def png_decodable(data: bytes) -> bool:
    """Whether :func:`decode_png` reads this PNG: 8 bits per sample, not interlaced, no colour-key transparency."""
    if not data.startswith(_PNG_MAGIC) or len(data) < 33 or data[12:16] != b"IHDR":
        return False
    _, _, depth, ctype, interlace = _png_header(data, "png")
    if depth != 8 or ctype not in _PNG_CHANNELS or interlace != 0:
        return False
    return ctype == 3 or b"tRNS" not in data        # (a false alarm on the four letters inside other data only sends the image to PIL)


def _unfilter(raw: bytes, h: int, stride: int, bpp: int, what: str) -> np.ndarray:
    """The PNG row filters undone: raw = h rows of (filter byte, stride bytes) -> uint8 [h, stride].  None, Sub and Up rows are numpy
    operations; an Average or Paeth row is a Python loop over its bytes (each needs the byte to its left): seconds for a 2048 x 2048
    image that uses them throughout."""
    if len(raw) < h * (stride + 1):
        raise ValueError(f"{what}: truncated PNG (image data of {len(raw)} bytes, {h * (stride + 1)} needed)")
    rows = np.frombuffer(raw, dtype=np.uint8, count=h * (stride + 1)).reshape(h, stride + 1)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    for r in range(h):
        kind, line = int(rows[r, 0]), rows[r, 1:]
        if kind == 0:
            cur = line
        elif kind == 1:                                                     # Sub: a running sum per channel, modulo 256
            cur = np.cumsum(line.reshape(-1, bpp), axis=0, dtype=np.uint64).astype(np.uint8).reshape(-1)
        elif kind == 2:                                                     # Up
            cur = line + prev
        elif kind in (3, 4):                                                # Average, Paeth: each byte needs the one to its left
            src, up, dst = line.tolist(), prev.tolist(), [0] * stride
            for k in range(stride):
                a = dst[k - bpp] if k >= bpp else 0
                b = up[k]
                if kind == 3:
                    pred = (a + b) >> 1
                else:
                    c = up[k - bpp] if k >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                dst[k] = (src[k] + pred) & 255
            cur = np.array(dst, dtype=np.uint8)
        else:
            raise ValueError(f"{what}: PNG row filter {kind}")
        out[r] = cur
        prev = out[r]
    return out


def decode_png(data: bytes, what: str = "png") -> np.ndarray:
    """An 8-bit, non-interlaced PNG (grey, grey + alpha, RGB, RGBA or palette, the palette's ``tRNS`` alpha included) -> uint8 [H,W,4]."""
    if not data.startswith(_PNG_MAGIC):
        raise ValueError(f"{what}: not a PNG")
    w, h, depth, ctype, interlace = _png_header(data, what)
    _check_side(w, h, what)
    if depth != 8 or ctype not in _PNG_CHANNELS or interlace != 0:
        raise ValueError(f"{what}: PNG of bit depth {depth}, colour type {ctype}, interlace {interlace} is not decoded here")
    pos, idat, palette, alpha, ended = 8, [], None, None, False
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise ValueError(f"{what}: truncated PNG (chunk {kind!r})")
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IDAT":
            idat.append(body)
        elif kind == b"PLTE":
            palette = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
        elif kind == b"tRNS":
            alpha = np.frombuffer(body, dtype=np.uint8)
        elif kind == b"IEND":
            ended = True
            break
        pos += 12 + n
    if not ended or not idat:
        raise ValueError(f"{what}: truncated PNG (no IEND or no image data)")
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"{what}: PNG image data: {e}") from None
    ch = _PNG_CHANNELS[ctype]
    px = _unfilter(raw, h, w * ch, ch, what).reshape(h, w, ch)
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    if ctype == 0:
        out[..., :3] = px
    elif ctype == 4:
        out[..., :3], out[..., 3] = px[..., :1], px[..., 1]
    elif ctype == 2:
        out[..., :3] = px
    elif ctype == 6:
        out[...] = px
    else:
        if palette is None or int(px.max()) >= len(palette):
            raise ValueError(f"{what}: PNG palette missing or index out of range")
        out[..., :3] = palette[px[..., 0]]
        if alpha is not None:
            table = np.full(len(palette), 255, dtype=np.uint8)
            table[:min(len(alpha), len(palette))] = alpha[:len(palette)]
            out[..., 3] = table[px[..., 0]]
    return out


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def decode_image(data: bytes, what: str = "image") -> np.ndarray:
    """Image bytes -> uint8 [H,W,4]: :func:`decode_png` where it applies, PIL otherwise."""
    if png_decodable(data):
        return decode_png(data, what)
    if data.startswith(_PNG_MAGIC):
        w, h = _png_header(data, what)[:2]
        _check_side(w, h, what)
    Image = _pil()
    if Image is None:
        kind = "PNG of this kind" if data.startswith(_PNG_MAGIC) else ("JPEG" if data[:2] == b"\xff\xd8" else "image format")
        raise ValueError(f"{what}: a {kind} needs PIL to be decoded, and PIL cannot be imported")
    import io
    try:
        img = Image.open(io.BytesIO(data))
        _check_side(img.size[0], img.size[1], what)
        return np.ascontiguousarray(np.asarray(img.convert("RGBA"), dtype=np.uint8))
    except ValueError:
        raise
    except Exception as e:                                                   # PIL's own errors: one kind of error for the caller
        raise ValueError(f"{what}: {e}") from None


# ---- container -----------------------------------------------------------------------------------------------------------------------
def _read_container(path: str) -> Tuple[dict, Optional[bytes]]:
    """-> (the JSON document, the BIN chunk or None)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"glTF":
        try:
            return json.loads(data.decode("utf-8")), None
        except (UnicodeDecodeError, json.JSONDecodeError) as e:
            raise ValueError(f"{path}: neither a GLB container nor glTF JSON ({e})") from None
    if len(data) < 12:
        raise ValueError(f"{path}: truncated GLB header")
    _, version, length = struct.unpack("<4sII", data[:12])
    if version != 2:
        raise ValueError(f"{path}: GLB version {version} (2 is read)")
    if length > len(data):
        raise ValueError(f"{path}: truncated GLB ({len(data)} bytes of {length})")
    pos, doc, blob = 12, None, None
    while pos < length:
        if pos + 8 > length:
            raise ValueError(f"{path}: truncated GLB chunk header at byte {pos}")
        n, kind = struct.unpack("<II", data[pos:pos + 8])
        if pos + 8 + n > length:
            raise ValueError(f"{path}: truncated GLB chunk at byte {pos} ({n} bytes declared)")
        body = data[pos + 8:pos + 8 + n]
        if kind == 0x4E4F534A and doc is None:
            try:
                doc = json.loads(body.decode("utf-8"))
            except (UnicodeDecodeError, json.JSONDecodeError) as e:
                raise ValueError(f"{path}: the GLB's JSON chunk: {e}") from None
        elif kind == 0x004E4942 and blob is None:
            blob = body
        pos += 8 + n + (-n % 4)
    if doc is None:
        raise ValueError(f"{path}: GLB without a JSON chunk")
    return doc, blob


def _uri_bytes(uri: str, base: str, what: str) -> bytes:
    if uri.startswith("data:"):
        head, _, payload = uri.partition(",")
        if not head.endswith(";base64"):
            raise ValueError(f"{what}: a data URI that is not base64")
        try:
            return base64.b64decode(payload)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
    from urllib.parse import unquote
    try:
        with open(os.path.join(base, unquote(uri)), "rb") as f:
            return f.read()
    except OSError as e:
        raise ValueError(f"{what}: {e}") from None


class _Document:
    def __init__(self, path: str):
        self.path = os.fspath(path)
        self.doc, self.blob = _read_container(self.path)
        self.base = os.path.dirname(os.path.abspath(self.path))
        if not isinstance(self.doc, dict) or str(self.doc.get("asset", {}).get("version", "")).split(".")[0] != "2":
            raise ValueError(f"{self.path}: not a glTF 2.x document")
        for ext in self.doc.get("extensionsRequired", []):
            if ext not in _ACCEPTED_EXTENSIONS:
                raise ValueError(f"{self.path}: required extension {ext} is not read")
        self._buffers: Dict[int, bytes] = {}
        self._images: Dict[int, int] = {}
        self.textures: List[np.ndarray] = []

    def _item(self, kind: str, index, what: str) -> dict:
        items = self.doc.get(kind, [])
        if not isinstance(index, int) or not 0 <= index < len(items):
            raise ValueError(f"{self.path}: {what} names {kind}[{index}] of {len(items)}")
        return items[index]

    def buffer(self, index: int, what: str) -> bytes:
        if index not in self._buffers:
            b = self._item("buffers", index, what)
            if "uri" in b:
                data = _uri_bytes(b["uri"], self.base, f"{self.path}: buffers[{index}]")
            elif index == 0 and self.blob is not None:
                data = self.blob
            else:
                raise ValueError(f"{self.path}: buffers[{index}] has no uri and there is no BIN chunk for it")
            if len(data) < int(b.get("byteLength", 0)):
                raise ValueError(f"{self.path}: buffers[{index}] is truncated ({len(data)} bytes of {b.get('byteLength')})")
            self._buffers[index] = data
        return self._buffers[index]

    def view(self, index: int, what: str) -> Tuple[bytes, int, int, int]:
        """-> (buffer, first byte, byte length, byteStride or 0)."""
        v = self._item("bufferViews", index, what)
        data = self.buffer(v.get("buffer"), f"bufferViews[{index}]")
        off, n = int(v.get("byteOffset", 0)), int(v.get("byteLength", 0))
        if off < 0 or n < 0 or off + n > len(data):
            raise ValueError(f"{self.path}: bufferViews[{index}] is truncated (bytes {off} .. {off + n} of {len(data)})")
        return data, off, n, int(v.get("byteStride", 0))

    def accessor(self, index: int, what: str) -> Tuple[np.ndarray, bool]:
        """-> (array [count, width] in the stored component type, normalized)."""
        a = self._item("accessors", index, what)
        name = f"accessors[{index}] ({what})"
        if "sparse" in a:
            raise ValueError(f"{self.path}: {name} is sparse: not read")
        if a.get("componentType") not in _COMPONENT or a.get("type") not in _WIDTH:
            raise ValueError(f"{self.path}: {name} has component type {a.get('componentType')} and type {a.get('type')}")
        dt, width, count = np.dtype(_COMPONENT[a["componentType"]]).newbyteorder("<"), _WIDTH[a["type"]], int(a.get("count", 0))
        if count < 0:
            raise ValueError(f"{self.path}: {name} has count {count}")
        if "bufferView" not in a:
            return np.zeros((count, width), dtype=dt), bool(a.get("normalized", False))
        data, off, n, stride = self.view(a["bufferView"], name)
        size = dt.itemsize * width
        stride = stride or size
        first = int(a.get("byteOffset", 0))
        if first < 0 or stride < size or (count and first + (count - 1) * stride + size > n):
            raise ValueError(f"{self.path}: {name} is truncated: {count} elements of {size} bytes, stride {stride}, from byte {first} of a view of {n}")
        arr = np.ndarray((count, width), dtype=dt, buffer=data, offset=off + first, strides=(stride, dt.itemsize))
        return np.array(arr), bool(a.get("normalized", False))

    def texture(self, index, what: str) -> Tuple[int, int, int]:
        """glTF texture -> (index into ``self.textures``, wrap_s, wrap_t); an image is decoded once."""
        t = self._item("textures", index, what)
        wrap_s = wrap_t = REPEAT
        if "sampler" in t:
            s = self._item("samplers", t["sampler"], f"textures[{index}]")
            wrap_s, wrap_t = int(s.get("wrapS", REPEAT)), int(s.get("wrapT", REPEAT))
            for w in (wrap_s, wrap_t):
                if w not in (REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE):
                    raise ValueError(f"{self.path}: samplers[{t['sampler']}] has wrap mode {w}")
        if "source" not in t:
            raise ValueError(f"{self.path}: textures[{index}] has no source image (its extensions are not read)")
        src = t["source"]
        if src not in self._images:
            img = self._item("images", src, f"textures[{index}]")
            name = f"{self.path}: images[{src}]"
            if "bufferView" in img:
                data, off, n, _ = self.view(img["bufferView"], f"images[{src}]")
                raw = data[off:off + n]
            elif "uri" in img:
                raw = _uri_bytes(img["uri"], self.base, name)
            else:
                raise ValueError(f"{name} has neither a uri nor a bufferView")
            self._images[src] = len(self.textures)
            self.textures.append(decode_image(raw, name))
        return self._images[src], wrap_s, wrap_t

    def material(self, index: int) -> Tuple[Material, int]:
        """-> (Material, the TEXCOORD set its texture reads)."""
        m = self._item("materials", index, "a primitive")
        pbr = m.get("pbrMetallicRoughness", {})
        factor, info = pbr.get("baseColorFactor", [1.0, 1.0, 1.0, 1.0]), pbr.get("baseColorTexture")
        sg = m.get("extensions", {}).get("KHR_materials_pbrSpecularGlossiness")
        if info is None and sg is not None:
            factor, info = sg.get("diffuseFactor", [1.0, 1.0, 1.0, 1.0]), sg.get("diffuseTexture")
        factor = tuple(float(x) for x in factor)
        if len(factor) != 4 or not all(np.isfinite(factor)):
            raise ValueError(f"{self.path}: materials[{index}] has the colour factor {factor}")
        if info is None:
            return Material(-1, REPEAT, REPEAT, factor), 0
        tex, wrap_s, wrap_t = self.texture(info.get("index"), f"materials[{index}]")
        return Material(tex, wrap_s, wrap_t, factor), int(info.get("texCoord", 0))


def _node_matrix(node: dict, what: str) -> np.ndarray:
    if "matrix" in node:
        m = np.asarray(node["matrix"], dtype=np.float64)
        if m.shape != (16,):
            raise ValueError(f"{what}: matrix of {m.size} numbers")
        return m.reshape(4, 4).T                                             # stored column-major
    t = np.asarray(node.get("translation", [0.0, 0.0, 0.0]), dtype=np.float64)
    x, y, z, w = (float(c) for c in node.get("rotation", [0.0, 0.0, 0.0, 1.0]))
    s = np.asarray(node.get("scale", [1.0, 1.0, 1.0]), dtype=np.float64)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.float64)
    m = np.eye(4)
    m[:3, :3] = r * s[None, :]
    m[:3, 3] = t
    return m


def _unit_float(a: np.ndarray, normalized: bool, what: str) -> np.ndarray:
    """float32 of a float accessor, or c / max of a normalised unsigned one."""
    if a.dtype == np.float32:
        return a.astype(np.float32)
    if normalized and a.dtype in (np.uint8, np.uint16):
        return a.astype(np.float32) / np.float32(np.iinfo(a.dtype).max)
    raise ValueError(f"{what}: float, or normalised unsigned byte / short, not {a.dtype}{' normalised' if normalized else ''}")


def load_gltf(path, frame: str = "gltf") -> TexturedMesh:
    """``.glb`` / ``.gltf`` -> :class:`TexturedMesh` (module docstring).  ``frame``: ``"gltf"`` keeps the stored coordinates; ``"mp3d"``
    maps (x, y, z) -> (x, -z, y), the inverse of the reference's ``coslam_mp3d2habitat`` (src/data/pose_loader.py:203-220): the scene then
    lies in the world the MP3D ``coslam.yaml`` bounds describe."""
    if frame not in ("gltf", "mp3d"):
        raise ValueError(f"load_gltf: frame {frame!r} (gltf or mp3d)")
    d = _Document(path)
    doc = d.doc
    nodes = doc.get("nodes", [])
    if doc.get("scenes"):
        roots = d._item("scenes", doc.get("scene", 0), "scene").get("nodes", [])
    else:
        children = {c for n in nodes for c in n.get("children", [])}
        roots = [i for i in range(len(nodes)) if i not in children]
    materials, tex_coord = [], []
    for i in range(len(doc.get("materials", []))):
        m, tc = d.material(i)
        materials.append(m)
        tex_coord.append(tc)
    verts, faces, uvs, cols, face_mat, n_vertices, any_colour = [], [], [], [], [], 0, False

    def primitive(mesh_i: int, prim_i: int, prim: dict, world: np.ndarray):
        nonlocal n_vertices, any_colour
        what = f"{d.path}: meshes[{mesh_i}].primitives[{prim_i}]"
        if prim.get("mode", 4) != 4:
            raise ValueError(f"{what} has mode {prim.get('mode')}: triangles (4) only")
        for ext in prim.get("extensions", {}):
            if ext not in _ACCEPTED_EXTENSIONS and ext in doc.get("extensionsRequired", []):
                raise ValueError(f"{what} needs extension {ext}")
        attrs = prim.get("attributes", {})
        if "POSITION" not in attrs:
            raise ValueError(f"{what} has no POSITION")
        pos, _ = d.accessor(attrs["POSITION"], f"{what} POSITION")
        if pos.dtype != np.float32 or pos.shape[1] != 3:
            raise ValueError(f"{what}: POSITION is float VEC3")
        if not np.isfinite(pos).all():
            raise ValueError(f"{what}: non-finite position")
        n = len(pos)
        if "indices" in prim:
            idx, _ = d.accessor(prim["indices"], f"{what} indices")
            if idx.dtype not in (np.uint8, np.uint16, np.uint32) or idx.shape[1] != 1:
                raise ValueError(f"{what}: indices are unsigned scalars")
            idx = idx.reshape(-1).astype(np.int64)
        else:
            idx = np.arange(n, dtype=np.int64)
        if len(idx) % 3:
            raise ValueError(f"{what}: {len(idx)} indices are not triangles")
        if len(idx) and int(idx.max()) >= n:
            raise ValueError(f"{what}: index {int(idx.max())} out of range for {n} vertices")
        mat = prim.get("material", -1)
        if mat != -1 and not (isinstance(mat, int) and 0 <= mat < len(materials)):
            raise ValueError(f"{what} names materials[{mat}] of {len(materials)}")
        uv = np.zeros((n, 2), dtype=np.float32)
        if mat >= 0 and materials[mat].texture >= 0:
            key = f"TEXCOORD_{tex_coord[mat]}"
            if key not in attrs:
                raise ValueError(f"{what}: its material's texture reads {key}, which the primitive does not have")
            raw, normalized = d.accessor(attrs[key], f"{what} {key}")
            if raw.shape != (n, 2):
                raise ValueError(f"{what}: {key} is a VEC2 per vertex")
            uv = _unit_float(raw, normalized, f"{what} {key}")
            if not np.isfinite(uv).all() or float(np.abs(uv).max(initial=0.0)) > MAX_UV:
                raise ValueError(f"{what}: {key} is not finite or beyond |uv| <= {MAX_UV:g}")
        col = np.full((n, 4), 255, dtype=np.uint8)
        if "COLOR_0" in attrs:
            raw, normalized = d.accessor(attrs["COLOR_0"], f"{what} COLOR_0")
            if raw.shape[0] != n or raw.shape[1] not in (3, 4):
                raise ValueError(f"{what}: COLOR_0 is a VEC3 or VEC4 per vertex")
            c = _unit_float(raw, normalized, f"{what} COLOR_0").astype(np.float64)
            col[:, :raw.shape[1]] = np.rint(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0).astype(np.uint8)
            any_colour = True
        p = pos.astype(np.float64)
        verts.append(p @ world[:3, :3].T + world[:3, 3])
        faces.append(idx.reshape(-1, 3) + n_vertices)
        uvs.append(uv)
        cols.append(col)
        face_mat.append(np.full(len(idx) // 3, mat, dtype=np.int32))
        n_vertices += n

    def walk(index, parent: np.ndarray, seen: Tuple[int, ...]):
        node = d._item("nodes", index, "the node tree")
        if index in seen:
            raise ValueError(f"{d.path}: nodes[{index}] is its own ancestor")
        world = parent @ _node_matrix(node, f"{d.path}: nodes[{index}]")
        if "mesh" in node:
            mesh = d._item("meshes", node["mesh"], f"nodes[{index}]")
            for k, prim in enumerate(mesh.get("primitives", [])):
                primitive(node["mesh"], k, prim, world)
        for c in node.get("children", []):
            walk(c, world, seen + (index,))

    for r in roots:
        walk(r, np.eye(4), ())
    if not verts:
        raise ValueError(f"{d.path}: no mesh in the scene")
    v = np.concatenate(verts)
    if frame == "mp3d":
        v = np.stack([v[:, 0], -v[:, 2], v[:, 1]], -1)
    return TexturedMesh(np.ascontiguousarray(v), np.concatenate(faces).astype(np.int64), np.concatenate(cols) if any_colour else None,
                        uv=np.concatenate(uvs), face_material=np.concatenate(face_mat), materials=materials, textures=d.textures)

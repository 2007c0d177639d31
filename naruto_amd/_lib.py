"""ctypes binding of libnaruto_hip.so (C ABI: include/naruto_hip.h).

This is the ONLY compute backend of the package: if the shared library has not been built the import
fails loudly -- there is no PyTorch / CPU fallback for the hot path.

The header is the one statement of the ABI.  It is read once at import, and the ``ctypes.Structure`` classes, the constants (each
``#define NARUTO_X`` is ``_lib.X``) and ``SIGNATURES`` below are derived from its declarations; ``ABI`` keeps what was read.  A new entry
point, struct field or constant is added to the header (and to the library) and nowhere else.  Pointers become ``c_void_p`` -- an address,
which is what a tensor's ``data_ptr()`` is -- except pointers to the header's own structs (``POINTER(Struct)``) and parameters the header
marks ``NARUTO_HOST``: those point to host memory and become ``POINTER(<scalar>)``, so that ctypes takes an array or passes a bare
``c_uint32()`` by reference.  The parser refuses what it does not understand (``HeaderError`` names the declaration) rather than guess:
a wrong width or order here is a wild pointer in a kernel, not a Python error.
"""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from typing import List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NARUTO_HIP_LIB") or os.path.join(_HERE, "libnaruto_hip.so")      # override: kernel experiments only
CSRC = os.path.join(_HERE, "csrc")
SOURCES = sorted(s for s in os.listdir(CSRC) if s.endswith((".hip", ".h", ".inc")))          # whatever the build can read
HEADER = os.path.join(os.path.dirname(_HERE), "include", "naruto_hip.h")


class HeaderError(ValueError):
    pass


_SCALARS = {"uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "int64_t": C.c_int64,
            "int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_QUALIFIERS = r"\b(?:const|struct|NARUTO_HOST)\b"
_DECLARATOR = r"(\**)\s*(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)"


class Header:
    """The declarations of a naruto_hip.h: ``structs`` {name: Structure class}, ``opaque`` {names of handle types}, ``defines`` {NARUTO_X: int},
    ``macros`` [names of the function-like macros: C expressions, not constants], ``functions`` {name: (restype, [argtypes])} and
    ``host_args`` {name: indices of its NARUTO_HOST parameters}, all in declaration order."""

    def __init__(self, text: str, path: str = "naruto_hip.h"):
        self.path, self.structs, self.opaque, self.defines, self.macros, self.functions, self.host_args = path, {}, set(), {}, [], {}, {}
        self._guard, self._in_cplusplus = None, False
        # comments and, below, preprocessor lines are blanked in place so that offsets keep giving line numbers
        self.text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: re.sub(r"[^\n]", " ", m.group()), text, flags=re.S)
        self.text = "\n".join(self._preprocessor(n + 1, line) for n, line in enumerate(self.text.split("\n")))
        for at, decl in self._statements(0, len(self.text)):
            self._declaration(at, decl)

    def _fail(self, at: int, why: str, decl: str, line: int = None):
        raise HeaderError(f"{self.path}:{line or self.text.count(chr(10), 0, at) + 1}: {why}: {' '.join(decl.split())!r}")

    def _preprocessor(self, n: int, line: str) -> str:
        """Line n: a directive is recorded and blanked, as are the two lines of the extern "C" wrapper; any other line passes."""
        s = line.strip()
        if not s.startswith("#"):
            if self._in_cplusplus and s not in ('extern "C" {', "}", ""):
                self._fail(0, 'only the extern "C" wrapper may stand under #ifdef __cplusplus', s, n)
            return "" if self._in_cplusplus else line
        m = re.fullmatch(r"#\s*define\s+(NARUTO_\w+)(\([^)]*\))?\s*(.*)", s)
        other = re.fullmatch(r"#\s*(ifndef\s+(\w+)|ifdef\s+__cplusplus|endif|include\s*<[\w./]+>)", s)
        if s.endswith("\\") or not (m or other):
            self._fail(0, "unsupported preprocessor line", s, n)
        if other:
            self._in_cplusplus = other.group(1).startswith("ifdef")
            self._guard = other.group(2) or self._guard
            return ""
        name, params, value = m.groups()
        literal = re.fullmatch(r"\(?\s*(-?(?:0[xX][0-9a-fA-F]+|0|[1-9]\d*))[uU]?[lL]{0,2}\s*\)?", value)
        if name in self.defines or name in self.macros:
            self._fail(0, "#define repeated", s, n)
        if params is not None:
            self.macros.append(name)
        elif literal:
            self.defines[name] = int(literal.group(1), 0)
        elif value or name not in ("NARUTO_HOST", self._guard):           # the two defines without a value: the marker and the include guard
            self._fail(0, "#define whose value is not one integer literal", s, n)
        return ""

    def _statements(self, start: int, end: int):
        """(offset, text) of every `;`-terminated declaration of text[start:end] outside braces; what follows the last `;` must be blank."""
        depth, at = 0, start
        for i in range(start, end):
            c = self.text[i]
            depth += (c == "{") - (c == "}")
            if c == ";" and depth == 0:
                decl = self.text[at:i]
                if decl.strip():
                    yield at + len(decl) - len(decl.lstrip()), decl.strip()
                at = i + 1
        rest = self.text[at:end]
        if rest.strip():
            self._fail(at + len(rest) - len(rest.lstrip()), "declaration without its ';'", rest)

    def _base(self, at, word: str, decl: str):
        """The type a declaration starts with: a ctypes scalar, a Structure class, or None for void and the opaque handles."""
        if word in _SCALARS or word in self.structs:
            return _SCALARS.get(word) or self.structs[word]
        if word not in ("void", "char") and word not in self.opaque:
            self._fail(at, f"unknown type {word!r}", decl)
        return None

    def _dims(self, at, dims: str, decl: str) -> List[int]:
        out = []
        for d in re.findall(r"\[\s*(\w*)\s*\]", dims):
            if not (d.isdigit() or d in self.defines) or int(self.defines.get(d, d)) <= 0:
                self._fail(at, f"array dimension {d!r} is neither a positive integer nor a #define", decl)
            out.append(int(self.defines.get(d, d)))
        return out

    def _declaration(self, at: int, decl: str):
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s+(\w+)", decl)
        if m and m.group(1) == m.group(2):
            self.opaque.add(m.group(1))
            return
        m = re.fullmatch(r"typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)", decl, flags=re.S)
        if m and m.group(1) == m.group(3) and m.group(1) not in self.structs:
            body = at + m.start(2)
            fields = [f for f_at, f_decl in self._statements(body, body + len(m.group(2))) for f in self._fields(f_at, f_decl)]
            self.structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
            return
        m = re.fullmatch(r"(.*?)\b(naruto_\w+)\s*\((.*)\)", decl, flags=re.S)
        if not m or m.group(2) in self.functions or re.search(r"[(){}]", m.group(3)):
            self._fail(at, "neither a struct typedef nor one prototype of a new naruto_* function", decl)
        ret, name, params = " ".join(re.sub(_QUALIFIERS, " ", m.group(1)).split()), m.group(2), m.group(3).strip()
        if ret not in ("void", "char*", "char *"):
            restype = self._base(at, ret, decl)
            if restype is None or ret in self.structs:
                self._fail(at, f"unsupported return type {ret!r}", decl)
        else:
            restype = None if ret == "void" else C.c_char_p
        args = [] if params in ("void", "") else [self._parameter(at, p, decl) for p in params.split(",")]
        self.functions[name] = (restype, [t for t, _ in args])
        self.host_args[name] = tuple(i for i, (_, host) in enumerate(args) if host)

    def _fields(self, at: int, decl: str):
        """`const float *a, *b` / `float* p[5]` / `double r[3][2], q[3][2]`: one (name, ctype) per declarator; a pointer is an address."""
        m = re.fullmatch(r"(\w+)\b\s*(.*)", re.sub(r"\b(?:const|struct)\b", " ", decl).strip(), flags=re.S)
        if not m:
            self._fail(at, "not a field declaration", decl)
        base = self._base(at, m.group(1), decl)
        for part in m.group(2).split(","):
            d = re.fullmatch(_DECLARATOR, part.strip())
            if not d or (base is None and not d.group(1)) or (m.group(1) in self.structs and not d.group(1)):
                self._fail(at, "not a field declaration (scalars, pointers and arrays of them)", decl)
            t = C.c_void_p if d.group(1) else base
            for n in reversed(self._dims(at, d.group(3), decl)):              # x[3][2] is three rows of two
                t = t * n
            yield d.group(2), t

    def _parameter(self, at: int, param: str, decl: str):
        """(ctype, is NARUTO_HOST) of one parameter; `T x[n]` is `T* x`."""
        host = re.search(r"\bNARUTO_HOST\b", param) is not None
        m = re.fullmatch(r"(\w+)\b\s*(\**)\s*(\w*)\s*((?:\[\s*\w*\s*\]\s*)*)", re.sub(_QUALIFIERS, " ", param).strip())
        if not m:
            self._fail(at, f"parameter {' '.join(param.split())!r} not understood", decl)
        base, depth = self._base(at, m.group(1), decl), len(m.group(2)) + bool(m.group(4))
        if depth == 0:
            if host or base is None or m.group(1) in self.structs:
                self._fail(at, f"parameter {' '.join(param.split())!r}: by value only scalars, and NARUTO_HOST only on pointers", decl)
            return base, False
        if depth == 1 and m.group(1) in self.structs:
            return C.POINTER(base), host
        if not host:
            return C.c_void_p, False
        if depth == 1 and base is None:
            self._fail(at, f"parameter {' '.join(param.split())!r}: NARUTO_HOST needs a pointer to a scalar, a struct or a pointer", decl)
        return C.POINTER(base if depth == 1 else C.c_void_p), True


ICP_STATUS = ("running", "converged", "degenerate", "max_iteration")           # indexed by NARUTO_ICP_RUNNING ... NARUTO_ICP_MAX_ITERATION

with open(HEADER) as _f:
    ABI = Header(_f.read(), HEADER)
SIGNATURES = ABI.functions                      # name -> (restype, argtypes); every symbol include/naruto_hip.h declares
# the struct classes under their own names, every `#define NARUTO_X n` as X
for _name, _value in list(ABI.structs.items()) + [(_n[len("NARUTO_"):], _v) for _n, _v in ABI.defines.items()]:
    if _name in globals():
        raise HeaderError(f"{HEADER}: {_name} would shadow a name of the binding")
    globals()[_name] = _value


def build_command(out: str = LIB_PATH) -> List[str]:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics",
            os.path.join(CSRC, "naruto_api.hip"), "-o", out]


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in [os.path.join(CSRC, s) for s in SOURCES] + [HEADER])


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or needs_build():
        tmp = f"{LIB_PATH}.{os.getpid()}.tmp"               # never a half-written library under the final name
        cmd = build_command(tmp)
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.run(cmd, check=True)
            os.replace(tmp, LIB_PATH)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return LIB_PATH


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no fallback path.")
        # The device pointers and streams handed to the library are PyTorch's, so both must talk to ONE HIP runtime: the
        # one PyTorch-ROCm brings along.  Loaded first, libnaruto_hip.so would pull in /opt/rocm's libamdhip64 and the
        # process would end up with two runtimes (the second one reports "no ROCm-capable device").  Import torch first.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class NarutoError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().naruto_last_error().decode("utf-8", "replace")
        raise NarutoError(f"{what or 'libnaruto_hip'} failed ({rc}): {msg}")


def workspace(n_bytes: int, device, dtype=None, zero: bool = False):
    """The one place a ``naruto_*_workspace()`` byte count becomes a tensor: ``ceil(n_bytes / itemsize)`` elements of ``dtype`` (float32 unless given)."""
    import torch
    dtype = dtype or torch.float32
    return (torch.zeros if zero else torch.empty)(-(-int(n_bytes) // dtype.itemsize), dtype=dtype, device=device)


def kernel_resources(lib_path: str = None):
    """Per kernel of the device code object embedded in the built library: the AMDGPU metadata notes the loader reads
    (``.vgpr_count``, ``.agpr_count``, ``.vgpr_spill_count``, ``.sgpr_spill_count``, ``.private_segment_fixed_size`` = scratch bytes per
    lane, ``.group_segment_fixed_size`` = static LDS).  Uses the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf);
    returns {demangled-ish kernel name: {field: int}}.  tests/test_host.py holds the hot kernels to zero scratch with it."""
    import tempfile
    llvm = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
    lib_path = lib_path or LIB_PATH
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib_path], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "agpr_count":                      # first field of a kernel's record (fields are sorted by name)
            cur = {"agpr_count": int(val)}
        elif cur is not None and key == "name":
            name = re.sub(r"^_ZN6naruto\d+", "", val)
            m2 = re.match(r"(\w+?)(?:I((?:L[bi]\d+E)+)E)?E", name)          # Itanium: name [I <Lb0E | Li128E ...> E] E <signature>
            if m2:
                name = m2.group(1)
                if m2.group(2):
                    args = re.findall(r"L([bi])(\d+)E", m2.group(2))
                    name += "<" + ",".join(("true" if v == "1" else "false") if k == "b" else v for k, v in args) + ">"
            out[name] = cur
        elif cur is not None and key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "sgpr_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size"):
            cur[key] = int(val)
    return out

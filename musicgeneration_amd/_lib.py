"""ctypes binding of libmgx.so (include/mgx.h).  No fallback: if the library is missing or a call
fails, the product path raises -- there is no CPU/eager substitute (the oracle lives in oracle/ and
is never imported from here)."""
from __future__ import annotations

import ctypes as C
import os
import re

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGX_LIB_PATH") or os.path.join(PKG, "libmgx.so")      # override: A/B two builds in one run

HEADER = os.path.join(os.path.dirname(PKG), "include", "mgx.h")


class MgxError(RuntimeError):
    pass


_BY_VALUE = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32,
             "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}


def _decl(decl: str, where: str):
    """`[const] type [*..] name` -> (name, ctypes type); any pointer crosses as void* (callers pass data_ptr() integers and None)"""
    m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*", decl)
    if m is None or not (m.group(2) or m.group(1) in _BY_VALUE):
        raise MgxError(f"include/mgx.h: no binding for `{' '.join(decl.split())}` in `{where}`")
    return m.group(3), C.c_void_p if m.group(2) else _BY_VALUE[m.group(1)]


def parse_header(text: str):
    """-> (defines, structs, functions) of include/mgx.h: {MGX_NAME: int}, {name: ctypes.Structure subclass},
    {name: (restype, argtypes)}.  The header is strict C99 over a closed set of types (tests/test_cabi.py compiles it that
    way), so three regular expressions read it; whatever they do not account for is refused, never bound by guesswork."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MGX_\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M)
               if re.fullmatch(r"-?(\d+|0[xX][0-9a-fA-F]+)", v)}
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|^\}\s*$', "", text, flags=re.M)          # the __cplusplus guard's two lines
    text = re.sub(r"typedef\s+enum\s*\w*\s*\{[^}]*\}\s*\w+\s*;", "", text)      # mgx_status crosses as int
    structs, functions = {}, {}

    def struct(m):
        fields = []
        for decl in filter(str.strip, m.group(1).split(";")):
            first, *more = decl.split(",")                               # `int N, K;`
            name, ct = _decl(first, "struct " + m.group(2))
            if more and (ct is C.c_void_p or not all(re.fullmatch(r"\s*\w+\s*", d) for d in more)):
                raise MgxError(f"include/mgx.h: no binding for `{' '.join(decl.split())}` in `struct {m.group(2)}`")
            fields += [(n.strip(), ct) for n in [name] + more]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return ""

    def function(m):
        ret, name, params = re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise MgxError(f"include/mgx.h: no binding for the return type `{ret}` of `{name}`")
        functions[name] = (_RETURNS[ret], [] if params == "void" else [_decl(p, name)[1] for p in params.split(",")])
        return ""

    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"([\w \t*]+?)\b(mgx_\w+)\s*\(([^()]*)\)\s*;", function, text)
    if text.strip():
        raise MgxError("include/mgx.h: not understood (a declaration that is neither a struct nor a plain function?): "
                       + " ".join(text.split())[:120])
    return defines, structs, functions


# The binding IS the header: a second copy kept by hand could shift every argument after an `int` written for a `size_t`.
with open(HEADER) as _f:
    DEFINES, STRUCTS, FUNCTIONS = parse_header(_f.read())
# A left-over libmgx.so of another ABI still exports the same names: calling it with this header's types would shift arguments.
EXPECTED_ABI = DEFINES["MGX_ABI_VERSION"]

_lib = None


def load() -> C.CDLL:
    """Load libmgx.so (building it first if hipcc is available and the .so is absent/stale)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must load ITS libamdhip64 first: libmgx.so then binds to the same HIP runtime instance
    # (loading libmgx first would pull in /opt/rocm's copy and leave two runtimes in one process).
    import torch  # noqa: F401
    own = os.path.abspath(LIB_PATH) == os.path.join(PKG, "libmgx.so")
    if own:
        from . import _build
        force = os.environ.get("MGX_REBUILD") == "1"
        if force or not os.path.exists(LIB_PATH) or (_build.have_hipcc() and _build._stale()):
            # absent or older than a source / the header: rebuild when a compiler is here (the GPU box has one too)
            if _build.have_hipcc():
                _build.build(force=force)
    if not os.path.exists(LIB_PATH):
        raise MgxError(f"{LIB_PATH} is missing: run `python -m musicgeneration_amd._build` (needs hipcc)")
    lib = C.CDLL(LIB_PATH)

    def bind(name):
        fn = getattr(lib, name)      # AttributeError here = header/library mismatch: fail loudly
        fn.restype, fn.argtypes = FUNCTIONS[name]
        return fn

    abi = bind("mgx_abi_version")()
    if abi != EXPECTED_ABI:
        raise MgxError(f"{LIB_PATH} has ABI version {abi}, this package binds ABI {EXPECTED_ABI} (include/mgx.h): "
                       "stale build -- rebuild with `python -m musicgeneration_amd._build --force`")
    for name in FUNCTIONS:
        bind(name)
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mgx_last_error().decode("utf-8", "replace")
        raise MgxError(f"{what} failed (status {rc}): {msg}")


def ptr(t) -> int:
    """device pointer of a torch tensor (or None -> NULL)"""
    return None if t is None else t.data_ptr()


_raw_stream = None


def stream_ptr() -> int:
    """raw hipStream_t of torch's current stream on the current device.  Through torch's C entry point: the Python-level
    ``torch.cuda.current_stream().cuda_stream`` costs ~8 us per call (device-index bookkeeping, a Stream object), i.e. 0.4 ms of
    a training step's ~150 launches -- nothing at the bench shape, a fifth of the host's time per step where the step is a few
    milliseconds (d_model 256, batch 2-6: round 6, profiles/r06_host_overhead.txt)."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        raw, dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
        _raw_stream = (lambda: raw(dev())) if (raw is not None and dev is not None) else (lambda: torch.cuda.current_stream().cuda_stream)
    return _raw_stream()

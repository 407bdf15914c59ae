"""CPU-side checks of the C-ABI boundary: libmgx.so builds/loads, exports every symbol declared in
include/mgx.h, the ctypes binding is read from the header, and the product path fails loudly without a GPU."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "mgx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mgx_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from musicgeneration_amd import _build, _lib
    path = _build.build()
    lib = ctypes.CDLL(path)
    names = _header_functions()
    assert len(names) >= 16
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mgx.h but not exported by libmgx.so"
    # the binding, the header (by this file's own regex) and the library's exports are one set of names
    bound = _lib.load()
    assert set(_lib.FUNCTIONS) == set(names) and all(getattr(bound, n).argtypes is not None for n in names)
    if shutil.which("nm") is not None:      # nothing named mgx_* is exported beside them
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("mgx_")} == set(names)


def test_no_torch_types_in_the_abi():
    src = open(os.path.join(ROOT, "include", "mgx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)          # declarations only (comments cite torch ops)
    assert "torch" not in code.lower() and "at::" not in code and "#include <hip" not in code
    assert "hipStream_t" not in code                            # the stream crosses the ABI as void*


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-box behaviour")
def test_fails_loudly_without_gpu():
    from musicgeneration_amd import _lib, ops
    from musicgeneration_amd.network import MusicTransformer
    lib = _lib.load()
    assert lib.mgx_abi_version() == _lib.EXPECTED_ABI
    assert lib.mgx_device_count() < 0 and b"hipGetDeviceCount" in lib.mgx_last_error()
    with pytest.raises(_lib.MgxError):
        ops.pad_bitmap(torch.zeros(2, 32, dtype=torch.int32), 5)          # CPU tensor: no fallback
    mt = MusicTransformer(embedding_dim=128, vocab_size=309, num_layer=1, max_seq=32)
    with pytest.raises(_lib.MgxError):
        mt(torch.zeros(1, 32, dtype=torch.int32))


def test_shape_errors_have_messages():
    """argument validation happens on the host before any launch, so it is testable without a GPU"""
    from musicgeneration_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    aligned = ctypes.c_void_p(4096)
    rc = lib.mgx_rel_attn_fwd(one, one, None, one, one, aligned, 1 << 20, 1, 33, 64, 64, None)
    assert rc == -1 and b"L%32==0" in lib.mgx_last_error()
    rc = lib.mgx_rel_attn_fwd(None, one, None, one, one, aligned, 1 << 20, 1, 32, 64, 64, None)
    assert rc == -2
    assert lib.mgx_rel_attn_fwd_workspace(2048) == 2048 * 128
    rc = lib.mgx_rel_attn_fwd(one, one, None, one, one, aligned, 64, 1, 32, 64, 64, None)      # workspace too small
    assert rc == -1 and b"workspace" in lib.mgx_last_error()
    rc = lib.mgx_linear_fwd(one, one, None, one, 4, 4, 48, 0, None)
    assert rc == -1 and b"K%64==0" in lib.mgx_last_error()
    rc = lib.mgx_add_ln_fwd(one, one, one, one, one, one, one, 4, 4100, 1e-6, 0.0, 0, None)
    assert rc == -1
    # three f32 [B,h,L] statistics (delta, -lse log2e, -delta) + two fragment-ordered bf16 copies of E [L,64] + the causal half
    # of dS by (query tile, key tile): 64*65/2 tiles of 32x32 bf16 per (b,h)
    assert lib.mgx_rel_attn_bwd_workspace(8, 2048, 512) == 3 * 8 * 8 * 2048 * 4 + 2 * 64 * 2048 * 2 + 8 * 8 * (64 * 65 // 2) * 2048
    # deterministic mode: argument validation (no GPU needed)
    assert lib.mgx_deterministic() == 0
    assert lib.mgx_set_deterministic(ctypes.c_void_p(12), 1 << 20) == -1 and b"aligned" in lib.mgx_last_error()
    assert lib.mgx_set_deterministic(ctypes.c_void_p(64 << 20), 1 << 20) == -1 and b"32 MiB" in lib.mgx_last_error()   # aligned, too small
    assert lib.mgx_set_deterministic_stream(ctypes.c_void_p(1), ctypes.c_void_p(64 << 20), 32 << 20) == -1 and b"first" in lib.mgx_last_error()
    assert lib.mgx_set_deterministic(None, 0) == 0 and lib.mgx_deterministic() == 0
    # stream registry (no stream is created or touched: the library only remembers the number)
    assert lib.mgx_stream_set_cus(ctypes.c_void_p(0x1000), 64) == 0 and lib.mgx_stream_cus(ctypes.c_void_p(0x1000)) == 64
    assert lib.mgx_stream_set_cus(ctypes.c_void_p(0x1000), 0) == 0
    assert lib.mgx_add_ln_bwd_workspace(100, 512) == 512 * 3 * 512 * 4       # 512 blocks of column partials
    rc = lib.mgx_add_ln_bwd(one, one, one, one, one, one, one, one, one, one, None, one, 16, 8, 512, 0.0, 0, None)
    assert rc == -1 and b"workspace" in lib.mgx_last_error()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "musicgeneration_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn


def test_header_is_plain_c_and_library_links_from_c(tmp_path):
    """The boundary is a C ABI: include/mgx.h must compile as strict C99 (no C++/torch types) and a C program must link
    against libmgx.so and get the documented error codes back -- no Python, no GPU needed for argument validation."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    from musicgeneration_amd import _lib
    _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "abi.c"
    src.write_text(
        '#include "mgx.h"\n#include <stdio.h>\n'
        'int main(void) {\n'
        '    mgx_dw_problem p = {0};\n'
        '    int rc = mgx_linear_dw_grouped(&p, 1, 128, NULL, 0, NULL);\n'
        '    printf("%d %d %s\\n", mgx_abi_version(), rc, mgx_last_error());\n'
        '    return 0;\n}\n')
    exe = str(tmp_path / "abi")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), str(src),
                    "-o", exe, "-L", libdir, "-l:libmgx.so", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split(None, 2)
    assert int(out[0]) >= 8 and int(out[1]) == -2 and "NULL pointer" in out[2]


def test_stale_library_abi_is_rejected(monkeypatch):
    """a left-over libmgx.so of another ABI exports the same names: load() must refuse it instead of calling it with
    shifted arguments"""
    from musicgeneration_amd import _lib
    _lib.load()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXPECTED_ABI", _lib.EXPECTED_ABI + 1)
    with pytest.raises(_lib.MgxError, match="ABI version"):
        _lib.load()
    monkeypatch.setattr(_lib, "EXPECTED_ABI", _lib.EXPECTED_ABI - 1)
    monkeypatch.setattr(_lib, "_lib", None)
    assert _lib.load().mgx_abi_version() == _lib.EXPECTED_ABI
    # the header's constant, the library and the binding agree
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert f"#define MGX_ABI_VERSION {_lib.EXPECTED_ABI}" in hdr


def test_bench_refuses_a_world_size_mismatch():
    """`bench.py --gpus N` must never print a line for another N: launched with a WORLD_SIZE that differs from --gpus it
    exits non-zero before touching the GPU; without a launcher and without N devices the self-launch refuses too."""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout) and '"metric"' not in r.stdout
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    import torch
    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and '"metric"' not in r.stdout and "HIP device" in r.stderr


def test_dw_grouped_workspace_says_which_weights_take_the_ring_path():
    """mgx_linear_dw_grouped_workspace is host logic (the split-then-fix-up plan): > 0 exactly for the groups the ring kernel takes --
    many rows, weights that fill their 256 x 256 tiles to 60 % (ragged last tile row / column allowed) -- and it sizes one fp32
    partial tile per (tile, M-split).  Without a GPU the plan assumes 256 CUs."""
    from musicgeneration_amd import _lib, ops
    lib = _lib.load()

    def need(shapes, M):
        arr = (ops._DwProblem * len(shapes))()
        for i, (N, K) in enumerate(shapes):
            arr[i] = ops._DwProblem(16, 16, 16, None, N, K)
        return lib.mgx_linear_dw_grouped_workspace(ctypes.cast(arr, ctypes.c_void_p), len(shapes), M)

    block = [(1536, 512), (512, 512), (256, 512), (512, 256)]           # cfg2's encoder block: 20 tiles
    n = need(block, 131072)
    assert n > 0 and n % (20 * 65536 * 4) == 0 and 1 <= n // (20 * 65536 * 4) <= 256 // 20
    n128 = need(block, 262144)                                           # the benchmark's rows (cfg2 at batch 128): as many M-splits, twice as long
    assert n128 > 0 and n128 % (20 * 65536 * 4) == 0 and 1 <= n128 // (20 * 65536 * 4) <= 256 // 20
    assert need([(448, 512)], 262144) > 0 and need(block, 262144 + 8) == 0 and need(block + [(128, 768)], 262144) == n128
    assert need([(448, 512)], 131072) > 0                                # the vocabulary projection: second tile row 192 of 256
    assert need([(384, 768), (768, 384)], 16384) > 0                     # cfg4's FFN weights: 75 % of their tiles
    assert need([(128, 768)], 16384) == 0                                # half a tile row: the 128 x 128 kernel
    assert need(block, 1024) == 0 and need(block, 131072 + 8) == 0       # few rows / M % 32 != 0: the 128 x 128 kernels
    # a mixed group is sized for its ring-shaped weights only
    assert need(block + [(128, 768)], 131072) == n


def _header_defines():
    return {n: int(v) for n, v in re.findall(r"^#define (MGX_\w+) (\d+)", open(os.path.join(ROOT, "include", "mgx.h")).read(), re.M)}


def test_binding_matches_pinned_signatures():
    """load() binds from include/mgx.h; these literal signatures cover every type class the header uses"""
    from musicgeneration_amd import _lib
    lib = _lib.load()
    vp, i, f, sz, u32, u64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint32,
                              ctypes.c_uint64)
    pinned = {
        "mgx_rel_attn_fwd_workspace": (sz, [i]),
        "mgx_rel_attn_decode_splits": (i, [i, i, i]),
        "mgx_last_error": (ctypes.c_char_p, []),
        "mgx_stream_create_cu_mask": (i, [vp, vp, i]),                                       # void**, const uint32_t*
        "mgx_adam_step": (i, [vp, vp, vp, vp, vp, sz, f, f, f, f, i, f, vp]),
        "mgx_dropout_bf16_at": (i, [vp, vp, sz, sz, f, vp, vp]),                             # const uint64_t*
        "mgx_gru_next_event": (i, [vp, i, i, vp, vp, f, vp, u32, vp, i, vp, vp, vp, i, vp]),
        "mgx_sample_topk_topp": (i, [vp, i, i, f, i, f, u64, vp, vp, i, vp, vp, i, vp, i, i, i, vp, vp]),
        "mgx_linear_dw_grouped": (i, [vp, i, i, vp, sz, vp]),                                # const mgx_dw_problem*
        "mgx_grad_norm": (i, [vp, sz, f, f, vp, vp, vp]),                                    # double*, mgx_clip_state*
    }
    assert len(pinned["mgx_sample_topk_topp"][1]) == 19
    for name, (res, args) in pinned.items():
        fn = getattr(lib, name)
        assert fn.restype is res, name
        assert list(fn.argtypes or []) == args and all(a is b for a, b in zip(fn.argtypes or [], args)), name


@pytest.mark.parametrize("text, names", [
    ("int mgx_x(long n);", ("mgx_x", "long n")),
    ("typedef struct { double a; short s; } mgx_s;", ("mgx_s", "short s")),
    ("int mgx_x(void (*cb)(int), void* stream);", ("mgx_x",)),
    ("int mgx_x(int a[4]);", ("mgx_x",)),
    ("long mgx_x(void);", ("mgx_x", "long")),
    ("int mgx_ok(int n);\nint mgx_x(unsigned int n);", ("mgx_x", "unsigned int n")),
])
def test_parser_refuses_what_it_does_not_understand(text, names):
    from musicgeneration_amd import _lib
    with pytest.raises(_lib.MgxError) as e:
        _lib.parse_header(text)
    assert all(n in str(e.value) for n in names)


def test_parser_reads_a_small_header():
    from musicgeneration_amd import _lib
    defines, structs, functions = _lib.parse_header(
        "#ifndef X_H\n#define X_H\n#define MGX_N 7 /* seven */\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
        "typedef enum { MGX_A = 0, MGX_B = -1 } mgx_e;\n"
        "typedef struct mgx_t { const float* p; /* ; */ uint32_t a, b;\n uint64_t c; } mgx_t;\n"
        "// int mgx_gone(long x);\n"
        "size_t mgx_f(const mgx_t* t,\n   double x, int32_t y, void** out);\nconst char *mgx_g(void);\n"
        "#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert defines == {"MGX_N": 7}
    assert functions == {"mgx_f": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p]),
                         "mgx_g": (ctypes.c_char_p, [])}
    assert list(structs) == ["mgx_t"] and structs["mgx_t"]._fields_ == [
        ("p", ctypes.c_void_p), ("a", ctypes.c_uint32), ("b", ctypes.c_uint32), ("c", ctypes.c_uint64)]


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof and every offsetof of the header's structs, as gcc lays them out, against the ctypes classes parsed from it"""
    import shutil
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    from musicgeneration_amd import _lib
    fields = {"mgx_dw_problem": ["dY", "X", "gW", "gb", "N", "K"],
              "mgx_clip_state": ["norm", "scale", "skipped_last", "n_clipped", "n_skipped"]}
    assert set(_lib.STRUCTS) == set(fields)
    body = "".join(f'    printf("{s} %zu' + " %zu" * len(fs) + f'\\n", sizeof({s})'
                   + "".join(f", offsetof({s}, {f})" for f in fs) + ");\n" for s, fs in fields.items())
    src = tmp_path / "layout.c"
    src.write_text('#include "mgx.h"\n#include <stdio.h>\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(fields)
    for line in lines:
        name, size, *offsets = line.split()
        cls = _lib.STRUCTS[name]
        assert [n for n, _ in cls._fields_] == fields[name]
        assert ctypes.sizeof(cls) == int(size)
        assert [getattr(cls, f).offset for f in fields[name]] == [int(o) for o in offsets], name


def test_read_clip_state_decodes_the_struct():
    from musicgeneration_amd import ops
    import math
    for norm, scale, last, clipped, skipped in [(3.5, 0.25, 0, 7, 2), (float("nan"), 0.0, 1, (1 << 32) + 5, (1 << 40) + 1),
                                                (float("inf"), 0.0, 1, 0, (1 << 64) - 1)]:
        raw = struct.pack("<dfIQQ", norm, scale, last, clipped, skipped)
        assert len(raw) == 32 == ops.CLIP_STATE_BYTES
        got = ops.read_clip_state(torch.frombuffer(bytearray(raw), dtype=torch.int64))
        assert list(got) == ["norm", "scale", "skipped_last", "clipped", "skipped"]
        assert type(got["norm"]) is float and type(got["scale"]) is float
        assert all(type(got[k]) is int for k in ("skipped_last", "clipped", "skipped"))
        assert got["norm"] == norm or (math.isnan(norm) and math.isnan(got["norm"]))
        assert (got["scale"], got["skipped_last"], got["clipped"], got["skipped"]) == (scale, last, clipped, skipped)


def test_constants_come_from_the_header():
    from musicgeneration_amd import _lib, ops
    d = _header_defines()
    assert _lib.EXPECTED_ABI == d["MGX_ABI_VERSION"]
    assert ops.GRAD_NORM_PARTS == d["MGX_GRAD_NORM_PARTS"]
    assert ops._DET_BYTES == d["MGX_DET_SCRATCH_BYTES"] == 32 << 20
    assert ops.CLIP_STATE_BYTES == 32
    assert ops._DwProblem is _lib.STRUCTS["mgx_dw_problem"]
    for name in ("MGX_DW_MAX_GROUP", "MGX_GEMM_SKINNY", "MGX_GEMM_TILE128", "MGX_GEMM_RING8", "MGX_GEMM_RING4"):
        assert _lib.DEFINES[name] == d[name]
    lib = _lib.load()
    aligned = ctypes.c_void_p(64 << 20)
    assert lib.mgx_set_deterministic(aligned, d["MGX_DET_SCRATCH_BYTES"] - 1) == -1 and b"32 MiB" in lib.mgx_last_error()
    assert lib.mgx_deterministic() == 0

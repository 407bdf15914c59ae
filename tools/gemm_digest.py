"""Digests of the GEMM entry points: a fixed, seeded list of small calls, one per route through linear.hip (skinny, 128 x 128 with
both buffer variants, the eight- and the four-wave ring; every epilogue operand; the weight-gradient plans), one SHA-256 per case
over the output bytes (contiguous CPU copy), then what mgx_linear_kernel_id answers for the boundary shapes of
tests/test_gpu_ring.py::test_linear_kernel_id_boundaries.  Two libraries (MGX_LIB_PATH) compute the same thing bit for bit and
route alike when their lists agree line for line.  The routes named in the comments are those of a 256-CU device.  The weight
gradients run in deterministic mode: otherwise they add with fp32 atomics and no two runs agree."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import _lib, ops

g = torch.Generator().manual_seed(2024)


def bf(*s, scale=0.5):
    return (torch.randn(*s, generator=g) * scale).cuda().bfloat16()


def f32(*s):
    return torch.randn(*s, generator=g).cuda()


def show(name, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for x in outs:
        h.update(x.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    print(f"{name:34s} {h.hexdigest()}", flush=True)


# ---- forward: (name, M, N, K, bias, act) ----
for name, M, N, K, use_b, act in [
        ("fwd skinny bias relu", 17, 200, 192, True, 1), ("fwd skinny", 32, 64, 1024, False, 0),
        ("fwd tile128 dbuf", 300, 264, 128, True, 1), ("fwd tile128 dbuf N%8", 300, 260, 64, True, 0),
        ("fwd tile128 sbuf", 4000, 3072, 64, False, 1),               # 32 x 24 = 768 workgroups: the single-buffer variant
        ("fwd ring8 bias relu", 49152, 256, 128, True, 1), ("fwd ring8", 49152, 256, 576, False, 0),
        ("fwd ring4 bias", 24576, 512, 512, True, 0), ("fwd ring4 relu", 24576, 512, 640, False, 1)]:
    a, w = bf(M, K), bf(N, K, scale=K ** -0.5)
    show(name, ops.linear_fwd(a, w, f32(N) if use_b else None, act))

# ---- dX [M,K] = dY [M,N] . W [N,K]: (name, M, N, K, mask, addend) ----
for name, M, N, K, use_y, use_add in [
        ("dx tile128 dbuf exact", 300, 128, 264, False, False), ("dx tile128 dbuf ragged N", 300, 72, 264, True, False),
        ("dx tile128 sbuf exact", 4000, 64, 3072, False, True), ("dx tile128 sbuf ragged N", 4000, 40, 3072, False, False),
        ("dx tile128 mask+addend", 24576, 512, 512, True, True),      # both operands: never a ring
        ("dx ring8", 49152, 128, 256, False, False), ("dx ring8 mask", 49152, 128, 256, True, False),
        ("dx ring8 addend", 49152, 512, 256, False, True),
        ("dx ring4", 24576, 512, 512, False, False), ("dx ring4 mask", 24576, 512, 512, True, False),
        ("dx ring4 addend", 24576, 640, 512, False, True)]:
    dy, w = bf(M, N), bf(N, K, scale=N ** -0.5)
    show(name, ops.linear_dx(dy, w, bf(M, K) if use_y else None, bf(M, K) if use_add else None))

# ---- weight gradients, deterministic mode: (name, M, [(N, K, bias)], grouped) ----
ops.set_deterministic(True)
for name, M, shapes, grouped in [
        ("dw tile128", 1000, [(264, 136, True)], False), ("dw ring (ragged tiles)", 4096, [(448, 512, True)], False),
        ("dw grouped ring", 4096, [(768, 256, True), (256, 256, False), (512, 256, True), (256, 512, False)], True),
        ("dw grouped mixed", 4096, [(768, 768, True), (128, 768, True), (768, 384, False)], True),
        ("dw grouped tile128 fallback", 1024, [(256, 256, True), (128, 384, False)], True)]:
    probs = [(bf(M, N), bf(M, K), f32(N, K), f32(N) if b else None) for N, K, b in shapes]
    if grouped:
        ops.linear_dw_grouped(probs)
    else:
        ops.linear_dw(*probs[0])
    show(name, *[t for p in probs for t in p[2:] if t is not None])
ops.set_deterministic(False)

# ---- decode path: LayerNorm prologue and fused embedding, row-major and fragment-order weights ----
M, N, K = 5, 200, 256
x, res, gam, bet, w, b = bf(M, K), bf(M, K), f32(K), f32(K), bf(N, K, scale=K ** -0.5), f32(N)
for name, wt in (("rowmajor", w), ("frag", ops.FragWeight(w))):
    show("linear_ln_fwd " + name, *ops.linear_ln_fwd(x, res, gam, bet, wt, b, 1))
    show("linear_fwd M<=32 " + name, ops.linear_fwd(x, wt, b, 0))
B, V, d, N = 7, 337, 128, 392
tok = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).cuda()
table, pe, w, b = f32(V, d), f32(64, d), bf(N, d, scale=d ** -0.5), f32(N)
for wname, wt in (("rowmajor", w), ("frag", ops.FragWeight(w))):
    for pname, pos, ragged in (("shared", torch.tensor([9], dtype=torch.int32), False),
                               ("per-row", torch.arange(3, 3 + 5 * B, 5, dtype=torch.int32), True)):
        hout = torch.empty(B, d, dtype=torch.bfloat16, device="cuda")
        show(f"decode_embed_linear {wname} {pname}", *ops.decode_embed_linear(tok, table, pe, pos.cuda(), wt, b, hout, ragged=ragged))

# ---- routing: kind 0 forward, 1 / 2 / 3 dX without operand / with a ReLU mask / with an addend ----
lib = _lib.load()
FWD = [(32, 512, 512), (33, 512, 512), (24576, 512, 512), (24320, 512, 512), (24704, 512, 512), (24576, 520, 512), (24576, 512, 64),
       (24576, 512, 256), (24576, 512, 384), (24576, 512, 576), (24576, 512, 640), (24576, 256, 512), (49152, 256, 512),
       (2097152, 1024, 512)]
DX = [(24576, 512, 512), (49152, 512, 256), (24320, 512, 512)]
for kind, M, N, K in [(0,) + s for s in FWD] + [(k,) + s for s in DX for k in (1, 2, 3)]:
    print(f"kernel_id kind {kind} ({M}, {N}, {K}) -> {lib.mgx_linear_kernel_id(kind, M, N, K, None)}", flush=True)

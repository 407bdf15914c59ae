"""Digests of the attention backward: a fixed, seeded list of small calls of mgx_rel_attn_bwd_parts, one per path through its
kernels -- one tile; one 64-key block; the 32-key fallback with a wave past the end of the sequence; trailing, interior and
whole-tile padding; 1 and 3 heads; E longer than L; dE groups laid out in sequence (B = 3) and dealt (B = 8); the stored-dS path
(parts 15), the 32-key kernel forced (1|64|2|8) and the recompute dQ (1|32) -- and one large call whose batch group is smaller
than B.  Per case one SHA-256 over the bytes of dqkv, the dS region of the workspace and dE (contiguous CPU copies).  Two
libraries (MGX_LIB_PATH) compute the same thing bit for bit when their lists agree line for line.  dE is taken in deterministic
mode: otherwise it is summed with fp32 atomics and no two runs agree.  (parts bit 16, dE by recomputation, has no deterministic
mode and stays out: tests/test_gpu_kernels.py checks it against a tolerance.)
    python tools/attn_bwd_digest.py [--no-big]"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import _lib, ops

PAD = 7


def up256(n):
    return (n + 255) // 256 * 256


def run(name, B, L, heads, M, pads, parts):
    d = 64 * heads
    g = torch.Generator().manual_seed(1000 + 7 * L + heads + B)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.8).to(torch.bfloat16).cuda()
    E = (torch.randn(M, 64, generator=g) * 0.5).to(torch.bfloat16).cuda()
    dctx = torch.randn(B, L, d, generator=g).to(torch.bfloat16).cuda()
    tok = torch.randint(0, PAD, (B, L), generator=g, dtype=torch.int32)
    if "trail" in pads:
        tok[0, L - 5:] = PAD
    if "interior" in pads:
        tok[-1, L // 2] = PAD
    if "tile" in pads:
        tok[B // 2, 64:96] = PAD                              # a whole key tile, not the first: no fully masked query
    bits = ops.pad_bitmap(tok.cuda(), PAD) if pads else None
    ctx, lse = ops.rel_attn_fwd(qkv, E, bits)
    dE = torch.zeros(M, 64, device="cuda")
    dqkv = torch.zeros_like(qkv)                              # zeroed: a part that is not run leaves its outputs untouched
    ws = torch.zeros(_lib.load().mgx_rel_attn_bwd_workspace(B, L, d), dtype=torch.uint8, device="cuda")
    ops.rel_attn_bwd(qkv, E, bits, ctx, dctx, lse, dE, parts, dqkv, ws)
    torch.cuda.synchronize()
    ds_off = 3 * up256(B * heads * L * 4) + 2 * up256(L * 64 * 2)      # delta, -lse log2e, -delta | EfA, EfT | dS tiles (rel_attn_bwd.hip: bwd_workspace)
    h = hashlib.sha256()
    for x in (dqkv, ws[ds_off:], dE):
        h.update(x.cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    print(f"{name:44s} parts {parts:3d}  {h.hexdigest()}", flush=True)


SHAPES = [  # name, B, L, heads, M, pads
    ("one tile", 1, 32, 1, 32, ""),
    ("one 64-key block, nT = 4", 2, 128, 1, 160, ""),
    ("32-key fallback, 3 heads, M > L", 1, 160, 3, 192, ""),
    ("32-key fallback L = 416, trailing pads", 2, 416, 1, 416, "trail"),
    ("L = 384 trail + interior + tile pads", 2, 384, 3, 400, "trail interior tile"),
    ("B = 3: dE groups in sequence", 3, 96, 1, 96, ""),
    ("B = 8: dE groups dealt, interior pad", 8, 160, 1, 192, "interior"),
]

ops.set_deterministic(True)
for parts in (15, 1 | 64 | 2 | 8, 1 | 32):
    for name, B, L, heads, M, pads in SHAPES:
        run(name, B, L, heads, M, pads, parts)
if "--no-big" not in sys.argv:
    # 16 rows x 10.5 MB x 5 tensors pass the batch group's 110 MB: groups of 8.  Workspace 0.6 GB.
    run("batch group 8 of B = 16", 16, 2048, 8, 2048, "", 1 | 4 | 2)
ops.set_deterministic(False)

"""Micro-benchmark of the embedding gradient kernel at cfg2, batch 64 -- the bench default of rounds 3-5, bench.py's batch64 block (64 x 2048 tokens, V = 337, d = 512, dropout 0.2)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops
dev = torch.device("cuda")
B, L, V, d = 64, 2048, 337, 512
g = torch.Generator().manual_seed(1)
tok = torch.randint(0, V - 1, (B, L), generator=g, dtype=torch.int32).to(dev)
dout = torch.randn(B, L, d, generator=g).to(torch.bfloat16).to(dev)
dt = torch.zeros(V, d, device=dev)
ops.embed_bwd(tok, dout, dt, 0.2, 3)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20): ops.embed_bwd(tok, dout, dt, 0.2, 3)
e1.record(); torch.cuda.synchronize()
print(f"embed_bwd {1e3 * e0.elapsed_time(e1) / 20:8.1f} us")

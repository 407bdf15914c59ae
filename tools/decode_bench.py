"""cfg5: autoregressive sampling, seq_len 8192, batch 32, top-p 0.9, graph-captured KV-cache decode."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd.network import MusicTransformer
ap = argparse.ArgumentParser()
ap.add_argument("--L", type=int, default=8192); ap.add_argument("--B", type=int, default=32)
ap.add_argument("--d", type=int, default=512); ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--V", type=int, default=337); ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--groups", type=int, default=None, help="independent sub-batches on separate streams (default: generate_cached's own choice)")
ap.add_argument("--masked", action="store_true", help="each group's stream on its own 1/G of the CUs (round 6 experiment)")
ap.add_argument("--kv", choices=["bf16", "fp8"], default="bf16", help="K/V cache: bf16 (default) or the 8-bit e4m3fn cache")
a = ap.parse_args()
torch.manual_seed(0)
mt = MusicTransformer(embedding_dim=a.d, vocab_size=a.V, num_layer=a.layers, max_seq=a.L, dropout=0.0).cuda().eval()
prior = torch.randint(0, a.V - 1, (a.B, 1), device="cuda")
mt.generate_cached(prior, 64, top_p=0.9, seed=1, use_graph=not a.no_graph, groups=a.groups, masked_groups=a.masked, kv_cache=a.kv)      # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
out = mt.generate_cached(prior, a.L - 1, top_p=0.9, seed=0, use_graph=not a.no_graph, groups=a.groups, masked_groups=a.masked,
                         kv_cache=a.kv)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
steps = a.L - 1
row_bytes = 2 * a.d * 2 if a.kv == "bf16" else 2 * (a.d + 4 * a.d // 64)     # K and V row of every head: bf16, or codes + scales
kv_bytes = a.layers * a.B * row_bytes * (steps * (steps + 1) / 2)              # K and V rows read over the whole run
w_bytes = steps * 2 * sum(p.numel() for p in mt.parameters())
tag = (" masked" if a.masked else "") + (", kv fp8" if a.kv == "fp8" else "")
print(f"cfg5 decode (groups={a.groups}{tag}): B={a.B} L={a.L} d={a.d} layers={a.layers}: {dt:.2f} s, {a.B*steps/dt:,.0f} tokens/s, "
      f"{1e3*dt/steps:.3f} ms/step avg; algorithmic KV traffic {kv_bytes/dt/1e9:,.0f} GB/s (+weights {w_bytes/dt/1e9:,.0f} GB/s)")
assert out.shape == (a.B, a.L) and int(out.max()) < a.V

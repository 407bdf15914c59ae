"""Ragged KV-cache decode: B prompts whose lengths spread uniformly over 1 .. Pmax, each continued by N tokens in one lockstep
batch (generate_cached(prior_lengths=...), graph on), against a uniform batch whose prompts all have the longest length.
Both runs prefill Pmax - 1 rows in one batched pass; a 1-token run of each measures that prefill, which is subtracted to
give the per-step decode time."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd.network import MusicTransformer
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=32); ap.add_argument("--Pmax", type=int, default=4096)
ap.add_argument("--new", type=int, default=4096); ap.add_argument("--d", type=int, default=512)
ap.add_argument("--layers", type=int, default=6); ap.add_argument("--V", type=int, default=337)
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
torch.manual_seed(0)
mt = MusicTransformer(embedding_dim=a.d, vocab_size=a.V, num_layer=a.layers, max_seq=a.Pmax + a.new, dropout=0.0).cuda().eval()
prior = torch.randint(0, a.V - 1, (a.B, a.Pmax), device="cuda")
ragged = torch.linspace(1, a.Pmax, a.B).round().long().tolist()         # uniform over 1 .. Pmax, the longest = Pmax
uniform = [a.Pmax] * a.B


def timed(lens, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched", prior_lengths=lens)
    torch.cuda.synchronize()
    assert out.shape == (a.B, a.Pmax + n)
    return time.perf_counter() - t0


res = {}
for name, lens in (("ragged", ragged), ("uniform", uniform)):
    timed(lens, 64)                                                       # warm-up (graph capture path)
    full = min(timed(lens, a.new) for _ in range(a.reps))
    pre = min(timed(lens, 1) for _ in range(a.reps))
    step = (full - pre) / (a.new - 1)
    res[name] = dict(seconds=round(full, 3), prefill_s=round(pre, 3), ms_per_step=round(1e3 * step, 4),
                     tokens_per_s=round(a.B * a.new / full), decode_tokens_per_s=round(a.B / step))
    print(f"{name:8s}: B={a.B} prompts {min(lens)}..{max(lens)}, {a.new} new tokens: {full:.2f} s ({pre:.2f} s prefill + 1 step), "
          f"{1e3 * step:.3f} ms/step, {a.B * a.new / full:,.0f} tokens/s ({a.B / step:,.0f} tokens/s decode only)")
res["ragged_over_uniform_step"] = round(res["ragged"]["ms_per_step"] / res["uniform"]["ms_per_step"], 4)
res["config"] = vars(a)
print(json.dumps(res))

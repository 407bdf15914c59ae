"""One MusicTransformer.score call through each logit path at cfg2's shape (REMI V = 337, d = 512, 6 layers, L = 2048), and its
parts on the same tensors: the forward up to the last LayerNorm (_hidden), the vocabulary projection alone (mgx_linear_fwd: what
the bf16 path stores and the fused kernel does not), mgx_token_logprob on the stored logits, mgx_linear_logprob on the hidden
states.  Device events around each call, every variant warmed up at its own shape, then timed --reps times in turn (so a drift
of the box hits all alike); the median, the best and the worst are printed.  Informative: no gate hangs on these figures."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops
from musicgeneration_amd.network import MusicTransformer
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seq-len", type=int, default=2048)
ap.add_argument("--d-model", type=int, default=512)
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--vocab", type=int, default=337)
a = ap.parse_args()
B, L, d, V = a.batch, a.seq_len, a.d_model, a.vocab
torch.manual_seed(0)
mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=a.layers, max_seq=L, dropout=0.0).cuda().eval()
x = torch.randint(0, V - 1, (B, L), device="cuda")
with torch.no_grad():
    h = mt._hidden(x)
    st, Vp = mt.store(), mt.vocab_padded
    w, bias = st.padded_view("fc.weight", Vp, d), st.padded_view("fc.bias", Vp, None, "param")
    logits = ops.linear_fwd(h, w, bias, 0)
tgt = torch.cat([x[:, 1:], torch.full((B, 1), -1, device="cuda")], 1).to(torch.int32).contiguous().view(-1)
variants = {
    "score fp32": lambda: mt.score(x, logits="fp32"),
    "score bf16": lambda: mt.score(x, logits="bf16"),
    "_hidden": lambda: mt._hidden(x),
    "vocabulary projection (mgx_linear_fwd)": lambda: ops.linear_fwd(h, w, bias, 0),
    "mgx_token_logprob": lambda: ops.token_logprob(logits[:, :, :V], tgt),
    "mgx_linear_logprob": lambda: ops.linear_logprob(h.view(B * L, d), w[:V], bias[:V], tgt),
}


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        e0.record()
        f()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


for f in variants.values():
    timed(f), timed(f)
times = {v: [] for v in variants}
for _ in range(a.reps):
    for v, f in variants.items():
        times[v].append(timed(f))
res = {"config": vars(a)}
for v, ts in times.items():
    res[v] = dict(median_ms=round(statistics.median(ts), 3), best_ms=round(min(ts), 3), worst_ms=round(max(ts), 3))
    print(f"{v:42s} median {res[v]['median_ms']:9.3f} ms   best {res[v]['best_ms']:9.3f}   worst {res[v]['worst_ms']:9.3f}   ({a.reps} runs)")
lp32, lp16 = mt.score(x, logits="fp32")["logp"], mt.score(x, logits="bf16")["logp"]
diff = (lp32 - lp16)[:, 1:].double()
print(f"per-event |logp fp32 path - logp bf16 path|: rms {diff.pow(2).mean().sqrt().item():.5f}, max {diff.abs().max().item():.5f}, "
      f"mean {diff.mean().item():.2e} (B = {B}, L = {L}, random weights)")
print(json.dumps(res))

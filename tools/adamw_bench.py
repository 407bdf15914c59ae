"""What weight decay, parameter groups and the weight EMA add to the optimiser sweep (GPU box, repo root):
    python tools/adamw_bench.py [--reps 50] [--rounds 7]
On cfg2's flat buffers (the model is built for its layout and its names) it times, with device events and in alternation,
mgx_adam_step alone and mgx_adam_step_groups with (1) one group (1, 0) and no EMA, (2) the default decay split of FusedAdam,
(3) the default split plus the EMA, and prints microseconds and bytes/s against the algorithmic bytes (30 B per parameter with
the shadow, 38 B with the EMA, 1/64 B for the group byte), then the median and the spread over the rounds and each variant
against plain Adam beside plain Adam's own run-to-run spread."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops
from musicgeneration_amd.network import MusicTransformer
from musicgeneration_amd.optim import build_groups
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()
dev = torch.device("cuda")
mt = MusicTransformer(embedding_dim=512, vocab_size=337, num_layer=6, max_seq=2048, dropout=0.2).to(dev)      # bench.py: CFG2
st = mt.store()
n = st.param.numel()
group_of_name, pairs, _ = build_groups(list(mt.named_parameters()), 0.01)
def tables(table, pairs):
    return (torch.tensor(table, dtype=torch.uint8, device=dev), torch.tensor([s for s, _ in pairs], dtype=torch.float32, device=dev),
            torch.tensor([w for _, w in pairs], dtype=torch.float32, device=dev))
split = tables(ops.adam_group_chunks(st.offsets, st.names, group_of_name, n), pairs)
one = tables([0] * ((n + 63) // 64), [(1.0, 0.0)])
decayed = sum(st.offsets[k][1] for k, i in group_of_name.items() if pairs[i][1] > 0)
g = torch.Generator().manual_seed(0)
p = torch.randn(n, generator=g).to(dev); grad = (0.01 * torch.randn(n, generator=g)).to(dev)
m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
ema = p.clone()
del mt, st
H = (1e-4, 0.9, 0.98, 1e-9)
step = [0]
def adam():
    step[0] += 1; ops.adam_step(p, grad, m, v, shadow, *H, step[0], 1.0)
def groups1():
    step[0] += 1; ops.adam_step_groups(p, grad, m, v, shadow, None, *H, step[0], 1.0, None, *one)
def decay():
    step[0] += 1; ops.adam_step_groups(p, grad, m, v, shadow, None, *H, step[0], 1.0, None, *split)
def decay_ema():
    step[0] += 1; ops.adam_step_groups(p, grad, m, v, shadow, ema, *H, step[0], 1.0, None, *split, 0.999)
def timed(fn):
    for _ in range(5): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps * 1e3          # us
print(f"n = {n} parameters, {len(pairs)} groups {pairs}, {decayed} parameters ({decayed / n * 100:.1f} %) decayed; "
      f"{a.rounds} rounds of {a.reps} calls each, alternating")
CASES = (("adam", adam, 30.0), ("groups1", groups1, 30.0 + 1 / 64), ("decay", decay, 30.0 + 1 / 64), ("decay+ema", decay_ema, 38.0 + 1 / 64))
T = {k: [] for k, _, _ in CASES}
for r in range(a.rounds):
    line = []
    for k, fn, bytes_per in CASES:
        t = timed(fn); T[k].append(t)
        line.append(f"{k} {t:7.1f} us {bytes_per * n / t / 1e6:5.2f} TB/s")
    print(f"round {r}: " + " | ".join(line))
med = {k: statistics.median(x) for k, x in T.items()}
for k, x in T.items():
    print(f"{k:9s} median {med[k]:7.1f} us  min {min(x):7.1f}  max {max(x):7.1f}  spread {(max(x) - min(x)) / med[k] * 100:4.1f} %")
for k in ("groups1", "decay", "decay+ema"):
    print(f"{k} against plain Adam: {(med[k] - med['adam']) / med['adam'] * 100:+.1f} % (by bytes: {'+26.7' if k == 'decay+ema' else '+0.1'} %; "
          f"run-to-run spread of plain Adam {(max(T['adam']) - min(T['adam'])) / med['adam'] * 100:.1f} %)")

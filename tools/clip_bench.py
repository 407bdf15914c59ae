"""What gradient clipping adds to the optimiser step (GPU box, repo root):
    python tools/clip_bench.py [--n N] [--reps 50] [--rounds 7]
At cfg2's flat parameter count (the model is built to read store.param.numel(); --n overrides it) it times, with device events and
in alternation on the same buffers, mgx_adam_step alone, mgx_adam_step_clipped alone (on the state one mgx_grad_norm call left),
mgx_grad_norm alone and the pair mgx_grad_norm + mgx_adam_step_clipped as FusedAdam.step issues it, and prints microseconds and
bytes/s against the algorithmic bytes of DESIGN.md 2.4 (Adam 30 B per parameter with the shadow, the norm pass 4 B), then the
median and the spread over the rounds and the two comparisons that matter: the added time (pair - Adam alone) against the Adam
pass, and clipped Adam against plain Adam beside plain Adam's own run-to-run spread."""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=0, help="elements; 0 = cfg2's store.param.numel()")
ap.add_argument("--reps", type=int, default=50); ap.add_argument("--rounds", type=int, default=7)
a = ap.parse_args()
dev = torch.device("cuda")
n = a.n
if not n:
    from musicgeneration_amd.network import MusicTransformer
    mt = MusicTransformer(embedding_dim=512, vocab_size=337, num_layer=6, max_seq=2048, dropout=0.2).to(dev)      # bench.py: CFG2
    n = mt.store().param.numel()
    del mt
g = torch.Generator().manual_seed(0)
p = torch.randn(n, generator=g).to(dev); grad = (0.01 * torch.randn(n, generator=g)).to(dev)
m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
workspace, state = ops.clip_buffers(dev)
H = (1e-4, 0.9, 0.98, 1e-9)
step = [0]
def adam():
    step[0] += 1; ops.adam_step(p, grad, m, v, shadow, *H, step[0], 1.0)
def clipped():
    step[0] += 1; ops.adam_step_clipped(p, grad, m, v, shadow, *H, step[0], state)
def norm():
    ops.grad_norm(grad, 1.0, 1.0, workspace, state)
def pair():
    step[0] += 1; ops.grad_norm(grad, 1.0, 1.0, workspace, state); ops.adam_step_clipped(p, grad, m, v, shadow, *H, step[0], state)
def timed(fn):
    for _ in range(5): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps * 1e3          # us
print(f"n = {n} parameters ({4 * n / 2**20:.1f} MiB of gradients); {a.rounds} rounds of {a.reps} calls each, alternating")
T = {"adam": [], "clipped": [], "norm": [], "pair": []}
norm()                                                 # a state for the clipped kernel alone
for r in range(a.rounds):
    ta, tc, tn, tp = timed(adam), timed(clipped), timed(norm), timed(pair)
    T["adam"].append(ta); T["clipped"].append(tc); T["norm"].append(tn); T["pair"].append(tp)
    print(f"round {r}: adam_step {ta:7.1f} us {30 * n / ta / 1e6:5.2f} TB/s | adam_step_clipped {tc:7.1f} us {30 * n / tc / 1e6:5.2f} TB/s | "
          f"grad_norm {tn:6.1f} us {4 * n / tn / 1e6:5.2f} TB/s | grad_norm + adam_step_clipped {tp:7.1f} us {34 * n / tp / 1e6:5.2f} TB/s")
med = {k: statistics.median(x) for k, x in T.items()}
for k, x in T.items():
    print(f"{k:7s} median {med[k]:7.1f} us  min {min(x):7.1f}  max {max(x):7.1f}  spread {(max(x) - min(x)) / med[k] * 100:4.1f} %")
added = med["pair"] - med["adam"]
print(f"added by clipping (pair - adam): {added:.1f} us = {added / med['adam'] * 100:.1f} % of the Adam pass (the pass moves 7.5x fewer bytes: it must stay below 100 %)")
print(f"clipped Adam {med['clipped']:.1f} us against plain Adam {med['adam']:.1f} us ({(med['clipped'] - med['adam']) / med['adam'] * 100:+.1f} %; "
      f"run-to-run spread of plain Adam {(max(T['adam']) - min(T['adam'])) / med['adam'] * 100:.1f} %); the pair is "
      f"{med['pair'] - med['norm'] - med['clipped']:+.1f} us against the sum of its parts run alone")
cs = ops.read_clip_state(state)
print(f"state: norm {cs['norm']:.6g} scale {cs['scale']:.6g} clipped {cs['clipped']} skipped {cs['skipped']}")

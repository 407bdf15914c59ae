"""Event_Melody_RNN training step through the scheduled-sampling route (``generate(..., events, output_type='logit')`` +
cross-entropy + backward: the step-major forward, one hipGraph) next to ``Train`` (layer-major: batched input GEMMs) at the
reference's configuration (Event_MelodyRNN/config.py: hidden 512, 3 layers, batch 100, window 200).  The three variants are
timed alternately, several rounds, so that a drift of the box shows as spread and not as a difference."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd.melody_rnn import Event_Melody_RNN
B, T, V, H, NL = 100, 200, 308, 512, 3
torch.manual_seed(0)
net = Event_Melody_RNN(init_dim=32, event_dim=V, hidden_dim=H, rnn_layers=NL, dropout=0.3).cuda().train()
events = torch.randint(0, V, (T, B), device="cuda")
init = torch.randn(B, 32, device="cuda")
lossf = torch.nn.CrossEntropyLoss()
calls = [0]
def train():
    out = net.Train(init, events[:-1])
    lossf(out.view(-1, V), events.view(-1)).backward()
def sched(ratio):
    def fn():
        calls[0] += 1
        out = net.generate(init, T, events=events[:-1], teacher_forcing_ratio=ratio, output_type='logit', seed=calls[0])
        lossf(out.reshape(-1, V), events.view(-1)).backward()
    return fn
variants = [("Train", train), ("generate -T 1.0", sched(1.0)), ("generate -T 0.5", sched(0.5))]
def timed(fn, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps
for _, fn in variants:                                  # capture + warm-up of every shape the timed window uses
    for _ in range(3): fn()
rounds = {name: [] for name, _ in variants}
for _ in range(5):
    for name, fn in variants:
        rounds[name].append(timed(fn, 20) * 1e3)
for name, ts in rounds.items():
    print(f"GRU train step B={B} T={T} H={H} layers={NL} {name}: median {sorted(ts)[len(ts) // 2]:.2f} ms "
          f"(min {min(ts):.2f}, max {max(ts):.2f} over {len(ts)} rounds of 20 steps; {B * T / (sorted(ts)[len(ts) // 2] * 1e-3):,.0f} events/s)")

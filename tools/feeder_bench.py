"""What feeding costs a training step, and what the device feeder changes (GPU box, repo root):
    python tools/feeder_bench.py [--batches 128,8] [--rounds 5] [--steps 10]
train.py's step (feeder, leading-pads check and H2D copy on the host path, forward, smoothed cross-entropy, backward, Noam
schedule + Adam) at cfg2 (d 512, six layers, max_seq 2048, dropout 0.2; the MIDI-like vocabulary of 309 ids, so that the stretch
applies) on a synthetic MIDI-like corpus, fed three ways in alternation:
    host      Data.slide_seq2seq_batch + utils.check_no_leading_pads + the H2D copy         (train.py without a new flag)
    device    DeviceData, no augmentation                                                  (--device-feeder)
    device+   DeviceData, transposition -3 .. 3 and stretch 0.95 / 1.0 / 1.05              (--transpose 3 --stretch 0.95,1.0,1.05)
Wall-clock per step over `steps` steps ending in a synchronize (the host's feeding is what is being measured), per round; then
the median and the spread over the rounds.  Last, the kernel alone at both shapes with device events."""
import argparse, os, random, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from musicgeneration_amd import ops, utils
from musicgeneration_amd.criterion import CustomSchedule, SmoothCrossEntropyLoss
from musicgeneration_amd.data import Data, DeviceData
from musicgeneration_amd.network import MusicTransformer
from musicgeneration_amd.optim import FusedAdam
ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="128,8"); ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10); ap.add_argument("--files", type=int, default=200)
a = ap.parse_args()
dev = torch.device("cuda:0")
V, PAD, L = 309, 308, 2048
root = tempfile.mkdtemp(prefix="feeder_bench_")
rng = np.random.default_rng(0)
for i in range(a.files):                                   # a third time shifts, the rest notes and velocities: a performance's mix
    n = 6000 + 37 * i
    ids = np.where(rng.random(n) < 0.33, rng.integers(208, 308, n), rng.integers(0, 208, n)).astype(np.uint16)
    torch.save(ids, os.path.join(root, f"p{i:03d}.data"))
mt = MusicTransformer(embedding_dim=512, vocab_size=V, num_layer=6, max_seq=L, dropout=0.2).to(dev)      # bench.py: CFG2's model
mt.train()
opt = FusedAdam(mt, lr=0, betas=(0.9, 0.98), eps=1e-9)
sch = CustomSchedule(512, optimizer=opt)
lossf = SmoothCrossEntropyLoss(0.1, V, PAD)
host = Data(root, L, rng=random.Random(1))
feeders = {"host": host,
           "device": DeviceData(Data(root, L, rng=random.Random(1)), dev, PAD),
           "device+": DeviceData(Data(root, L, rng=random.Random(1)), dev, PAD, transpose=list(range(-3, 4)), stretch=[0.95, 1.0, 1.05],
                                 aug_rng=random.Random(2))}
print(f"corpus: {len(host.file_dict['train'])} training files, {feeders['device'].corpus.numel()} events on the device; model cfg2 with V = {V}")


def step(name, B):
    f = feeders[name]
    x, y = f.slide_seq2seq_batch(B, L)
    if name == "host":
        utils.check_no_leading_pads(x, PAD)
        x, y = (torch.from_numpy(t).contiguous().to(dev, non_blocking=True, dtype=torch.int) for t in (x, y))
    loss = lossf(mt(x), y)
    loss.backward()
    sch.step()
    opt.zero_grad()


def timed(name, B, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(name, B)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3       # ms per step


opt.zero_grad()
for B in [int(b) for b in a.batches.split(",")]:
    steps = a.steps if B >= 64 else 4 * a.steps
    for name in feeders:
        timed(name, B, 3)                                  # warm-up: allocations, code objects
    T = {name: [] for name in feeders}
    for r in range(a.rounds):
        for name in feeders:
            T[name].append(timed(name, B, steps))
        print(f"batch {B:3d} round {r}: " + " | ".join(f"{name} {T[name][-1]:8.3f} ms" for name in feeders))
    med = {k: statistics.median(v) for k, v in T.items()}
    for k, v in T.items():
        print(f"batch {B:3d} {k:8s} median {med[k]:8.3f} ms/step  min {min(v):8.3f}  max {max(v):8.3f}  spread {(max(v) - min(v)) / med[k] * 100:4.1f} %"
              f"  {B * L / med[k] / 1e3:6.2f} M events/s")
    spread = max(T["host"]) - min(T["host"])
    for k in ("device", "device+"):
        print(f"batch {B:3d} {k:8s} against host: {med[k] - med['host']:+.3f} ms/step ({(med[k] - med['host']) / med['host'] * 100:+.2f} %); "
              f"the host-fed step's own spread over the rounds is {spread:.3f} ms")

    # the kernel alone, device events
    for name in ("device", "device+"):
        f = feeders[name]
        files, starts = f.plan(B, L)
        shift, q = f.draw_augmentation(B)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
        start = torch.from_numpy(f.offsets_host[files] + starts).to(dev)
        avail = torch.from_numpy((f.lengths_host[files] - starts).astype(np.int32)).to(dev)
        x = torch.empty(B, L, dtype=torch.int32, device=dev); y = torch.empty_like(x)
        kw = dict(perm=f.perm, shift_row=None if shift is None else i32(shift), stretch_q=None if q is None else i32(q), ts0=f.ts0, n_ts=f.n_ts)
        for _ in range(5):
            ops.crop_augment(f.corpus, start, avail, x, y, PAD, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            ops.crop_augment(f.corpus, start, avail, x, y, PAD, **kw)
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 100 * 1e3
        print(f"batch {B:3d} mgx_crop_augment alone ({name}): {us:7.1f} us per call, back to back ({B * L * 8 / us / 1e3:6.1f} GB/s of x and y written)")
mt.check_no_leading_pads()
shutil.rmtree(root)

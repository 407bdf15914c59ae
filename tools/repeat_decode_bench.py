"""What repetition control costs a step: generate_cached with ``repetition`` (one more launch per step, captured with it) against
the same call without the keyword, on the same prompts, graph on.  Two settings: "realistic" (window 64, ngram 8 over the whole
sequence) and "worst" (window 4096, ngram 64 over the whole sequence).  The calls run in alternation, off / realistic / worst,
``--reps`` times each (three at least); a 1-token run of each measures its prefill, which is subtracted to give the per-step
time.  Also the kernel alone, back to back on one stream, on the last column of a full history: a random one (an n-gram
comparison ends at its first column) and a constant one (every comparison runs all its columns: the true worst case).

    python tools/repeat_decode_bench.py > profiles/r27_repeat_control.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from musicgeneration_amd import ops
from musicgeneration_amd.decode import Repetition
from musicgeneration_amd.network import MusicTransformer

SHAPES = {                                                               # d, layers, V, B, P, new
    "reference": (256, 6, 337, 8, 500, 2000),                            # generate.py -c prompt.mid -b 8
    "cfg5": (512, 6, 337, 32, 4096, 512),
}
SETTINGS = {"off": None, "realistic": dict(window=64, ngram=8, span=0), "worst": dict(window=4096, ngram=64, span=0)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def timed(mt, prior, n, rep):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched", repetition=rep)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(vs, digits):
    return dict(min=round(min(vs), digits), median=round(statistics.median(vs), digits), max=round(max(vs), digits))


def kernel_alone(B, V, total, hist, kw, iters=400):
    """us per launch, back to back, at the history's last column"""
    logits = torch.randn(B, (V + 63) // 64 * 64, device="cuda").to(torch.bfloat16)
    pos = torch.tensor([total - 1], dtype=torch.int32, device="cuda")
    subject = torch.ones(V, dtype=torch.int32, device="cuda")
    pen = torch.full((kw["window"] + 1,), 1e-3, dtype=torch.float32, device="cuda")
    for _ in range(20):
        ops.repeat_penalty(logits, V, hist, pos, subject, pen, kw["window"], kw["ngram"], kw["span"], 1e-3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.repeat_penalty(logits, V, hist, pos, subject, pen, kw["window"], kw["ngram"], kw["span"], 1e-3)
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / iters, 2)


for name in a.shapes.split(","):
    d, layers, V, B, P, new = SHAPES[name]
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
    prior = torch.randint(0, V - 1, (B, P), device="cuda")
    subject = np.ones(V, dtype=np.int32)
    subject[V - 1] = 0
    reps = {k: None if kw is None else Repetition(subject, presence=0.1, frequency=0.05, **kw) for k, kw in SETTINGS.items()}
    runs = {k: [] for k in SETTINGS}
    for k in SETTINGS:
        timed(mt, prior, 64, reps[k])                                   # warm-up (graph capture path)
    for _ in range(a.reps):
        for k in SETTINGS:                                              # off / realistic / worst, in alternation
            full, _ = timed(mt, prior, new, reps[k])
            pre, _ = timed(mt, prior, 1, reps[k])
            runs[k].append(dict(full=full, pre=pre, step=1e3 * (full - pre) / (new - 1)))
    res = dict(shape=name, config=dict(d=d, layers=layers, V=V, B=B, P=P, new=new, reps=a.reps))
    for k, rs in runs.items():
        res[k] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                      tokens_per_s=spread([B * new / r["full"] for r in rs], 0))
    off = res["off"]["ms_per_step"]
    for k in ("realistic", "worst"):
        t = res[k]["ms_per_step"]
        res[k]["minus_off_us_per_step"] = round(1e3 * (t["median"] - off["median"]), 2)
        res[k]["verdict"] = "slower" if t["min"] > off["max"] else "faster" if t["max"] < off["min"] else \
            "no difference: inside the run-to-run spread of the call without the keyword"
        total = P + new
        rand = torch.randint(0, V - 1, (B, total), dtype=torch.int32, device="cuda")
        res[k]["kernel_alone_us"] = dict(random_history=kernel_alone(B, V, total, rand, SETTINGS[k]),
                                         constant_history=kernel_alone(B, V, total, torch.zeros_like(rand), SETTINGS[k]))
    for k in SETTINGS:
        v = res[k]
        print(f"{name:10s} {k:9s}: B={B} P={P} +{new}: {v['ms_per_step']['median']:.4f} ms/step "
              f"({v['ms_per_step']['min']:.4f} .. {v['ms_per_step']['max']:.4f}), prefill {v['prefill_s']['median']:.3f} s, "
              f"{v['tokens_per_s']['median']:,.0f} tokens/s"
              + ("" if k == "off" else f"; - off: {v['minus_off_us_per_step']} us/step ({v['verdict']}); kernel alone "
                 f"{v['kernel_alone_us']['random_history']} us (random history), {v['kernel_alone_us']['constant_history']} us "
                 f"(constant history)"))
    print(json.dumps(res), flush=True)
    del mt
    torch.cuda.empty_cache()

"""What the per-row length budgets cost a step: generate_timed with every budget None (no row ever ends, the mask never bites,
so the call makes the steps and draws the tokens of generate_cached, plus two launches per step and one read of ``done`` per
``--poll`` steps) against generate_cached on the same prompts, graph on.  The two calls run in alternation, A/B/A/B, ``--reps``
times each (three at least); a 1-token run of each measures its prefill, which is subtracted to give the per-step time.  The
tokens of the two calls are compared.  Also: the wall time of one poll read (``Budget.finished``) on an idle device.

    python tools/budget_decode_bench.py > profiles/r24_budget_decode.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from musicgeneration_amd.network import MusicTransformer

SHAPES = {                                                               # d, layers, V, B, P, new
    "reference": (256, 6, 337, 8, 500, 2000),                            # generate.py -c prompt.mid -b 8
    "cfg5": (512, 6, 337, 32, 4096, 512),
}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--poll", type=int, default=32)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def timed(mt, prior, n, budgeted, cost):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if budgeted:
        out, lengths, info = mt.generate_timed(prior, None, cost, n, poll=a.poll, top_p=0.9, seed=0)
        assert info["steps_run"] == n and int(lengths.min()) == n
    else:
        out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched")
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(vs, digits):
    return dict(min=round(min(vs), digits), median=round(statistics.median(vs), digits), max=round(max(vs), digits))


for name in a.shapes.split(","):
    d, layers, V, B, P, new = SHAPES[name]
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
    prior = torch.randint(0, V - 1, (B, P), device="cuda")
    cost = np.zeros(V, dtype=np.int32)
    cost[195] = 1                                                       # REMI's bar
    runs = {True: [], False: []}
    for budgeted in (True, False):
        timed(mt, prior, 64, budgeted, cost)                            # warm-up (graph capture path)
    outs = {}
    for _ in range(a.reps):
        for budgeted in (True, False):                                  # A/B/A/B
            full, outs[budgeted] = timed(mt, prior, new, budgeted, cost)
            pre, _ = timed(mt, prior, 1, budgeted, cost)
            runs[budgeted].append(dict(full=full, pre=pre, step=1e3 * (full - pre) / (new - 1)))
    res = dict(shape=name, config=dict(d=d, layers=layers, V=V, B=B, P=P, new=new, reps=a.reps, poll=a.poll),
               same_tokens=bool(torch.equal(outs[True], outs[False])))
    for budgeted, key in ((True, "timed"), (False, "cached")):
        rs = runs[budgeted]
        res[key] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                        tokens_per_s=spread([B * new / r["full"] for r in rs], 0))
    t, c = res["timed"]["ms_per_step"], res["cached"]["ms_per_step"]
    res["timed_minus_cached_us_per_step"] = round(1e3 * (t["median"] - c["median"]), 2)
    res["verdict"] = "timed slower" if t["min"] > c["max"] else "timed faster" if t["max"] < c["min"] else \
        "no difference: inside generate_cached's run-to-run spread"
    # one poll read on an idle device: the reduction's launch, the copy of its one value and the synchronise
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    reads = []
    for i in range(220):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bool(done.min().item())
        if i >= 20:
            reads.append(1e6 * (time.perf_counter() - t0))
    res["poll_read_us"] = spread(reads, 1)
    res["poll_read_in_steps"] = round(res["poll_read_us"]["median"] / (1e3 * c["median"]), 3)
    for key in ("timed", "cached"):
        v = res[key]
        print(f"{name:10s} {key:7s}: B={B} P={P} +{new}: {v['ms_per_step']['median']:.4f} ms/step "
              f"({v['ms_per_step']['min']:.4f} .. {v['ms_per_step']['max']:.4f}), prefill {v['prefill_s']['median']:.3f} s, "
              f"{v['tokens_per_s']['median']:,.0f} tokens/s")
    print(f"{name:10s} timed - cached: {res['timed_minus_cached_us_per_step']} us/step ({res['verdict']}); same tokens: "
          f"{res['same_tokens']}; one poll read {res['poll_read_us']['median']} us = {res['poll_read_in_steps']} steps (poll {a.poll})")
    print(json.dumps(res), flush=True)
    del mt
    torch.cuda.empty_cache()

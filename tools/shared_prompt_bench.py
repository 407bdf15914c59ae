"""N samples per prompt: generate_cached(samples_per_prompt=N) over one shared prompt cache against the same call on the prompts
repeated N times (repeat_interleave + prior_lengths), graph on.  The two calls run in alternation, A/B/A/B, ``--reps`` times each
(three at least); a 1-token run of each measures its prefill, which is subtracted to give the per-step decode time.  Reports, per
call, ms/step, prefill seconds, tokens/s and torch.cuda.max_memory_allocated, each time as min / median / max over the reps, and
whether the difference in ms/step lies outside the repeated call's own run-to-run spread.

    python tools/shared_prompt_bench.py > profiles/r20_shared_prompt_decode.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd.network import MusicTransformer

SHAPES = {                                                               # d, layers, V, Bp, N, P, new
    "cfg5-4x8": (512, 6, 337, 4, 8, 4096, 512),
    "cfg5-2x16": (512, 6, 337, 2, 16, 4096, 512),
    "reference": (256, 6, 337, 1, 8, 500, 2000),                        # generate.py -c prompt.mid -b 8: one prompt, eight rows
}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def timed(mt, prior, lens, N, n, shared):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    if shared:
        out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prior_lengths=lens, samples_per_prompt=N)
    else:
        out = mt.generate_cached(prior.repeat_interleave(N, 0), n, top_p=0.9, seed=0, prefill="batched",
                                 prior_lengths=[v for v in lens for _ in range(N)])
    torch.cuda.synchronize()
    assert out.shape == (prior.shape[0] * N, prior.shape[1] + n)
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated()


def spread(vs, digits):
    return dict(min=round(min(vs), digits), median=round(statistics.median(vs), digits), max=round(max(vs), digits))


for name in a.shapes.split(","):
    d, layers, V, Bp, N, P, new = SHAPES[name]
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
    prior = torch.randint(0, V - 1, (Bp, P), device="cuda")
    lens = [P] * Bp                                                     # equal lengths: the repeated call takes its uniform chain
    runs = {True: [], False: []}
    for shared in (True, False):
        timed(mt, prior, lens, N, 64, shared)                           # warm-up (graph capture path)
    for _ in range(a.reps):
        for shared in (True, False):                                    # A/B/A/B
            full, mem = timed(mt, prior, lens, N, new, shared)
            pre, _ = timed(mt, prior, lens, N, 1, shared)
            runs[shared].append(dict(full=full, pre=pre, step=1e3 * (full - pre) / (new - 1), mem=mem))
    res = dict(shape=name, config=dict(d=d, layers=layers, V=V, Bp=Bp, N=N, P=P, new=new, reps=a.reps))
    for shared, key in ((True, "shared"), (False, "repeated")):
        rs = runs[shared]
        res[key] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                        tokens_per_s=spread([Bp * N * new / r["full"] for r in rs], 0),
                        max_memory_MiB=round(max(r["mem"] for r in rs) / 2 ** 20, 1))
    s, r = res["shared"]["ms_per_step"], res["repeated"]["ms_per_step"]
    res["repeated_over_shared_step"] = round(r["median"] / s["median"], 3)
    # a gain counts only when the two calls' ranges do not overlap
    res["verdict"] = "shared faster" if s["max"] < r["min"] else "shared slower" if s["min"] > r["max"] else \
        "no gain: inside the repeated call's run-to-run spread"
    for key in ("shared", "repeated"):
        v = res[key]
        print(f"{name:10s} {key:8s}: Bp={Bp} N={N} P={P} +{new}: {v['ms_per_step']['median']:.3f} ms/step "
              f"({v['ms_per_step']['min']:.3f} .. {v['ms_per_step']['max']:.3f}), prefill {v['prefill_s']['median']:.3f} s, "
              f"{v['tokens_per_s']['median']:,.0f} tokens/s, peak {v['max_memory_MiB']:,.0f} MiB")
    print(f"{name:10s} repeated / shared ms per step {res['repeated_over_shared_step']}: {res['verdict']}")
    print(json.dumps(res), flush=True)
    del mt
    torch.cuda.empty_cache()

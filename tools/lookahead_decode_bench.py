"""What a draft-and-verify step costs and what it buys: generate_cached(lookahead=T) at T = 2, 4, 8 against the same call without
the keyword (the one-token call, untouched by the feature), on the same prompts, graph on.  Two ends of the acceptance: "guide", the
draft is the call's own sample for the seed -- what the history call at the same T returned -- (acceptance near 1: T tokens per step),
and "history" on the random-init model (acceptance near 0: the pure overhead of a step).  The one-token call's sample is no such
guide on this model: random-init logits are near ties, the two chains differ in the last bit, and after the first flipped draw the
two samples have nothing in common (the share of rows identical to the one-token call's is printed).  The calls run in
alternation, ``--reps`` times each (three at least); a 1-token run of each measures its prefill and first step, which is subtracted
to give the per-step time.  Break-even acceptance: ms per lookahead step over ms per one-token step, minus one -- the extra tokens a
step must accept, on average, to pay for itself.

    python tools/lookahead_decode_bench.py > profiles/r29_lookahead_decode.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd.network import MusicTransformer

SHAPES = {                                                               # d, layers, V, B, P, new
    "reference": (256, 6, 337, 8, 500, 2000),                            # generate.py -c prompt.mid -b 8
    "cfg5": (512, 6, 337, 32, 4096, 512),
}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--lookahead", default="2,4,8")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def timed(mt, prior, n, **kw):
    st = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched", **(dict(kw, stats=st) if kw else {}))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out, st


def spread(vs, digits):
    return dict(min=round(min(vs), digits), median=round(statistics.median(vs), digits), max=round(max(vs), digits))


for name in a.shapes.split(","):
    d, layers, V, B, P, new = SHAPES[name]
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
    prior = torch.randint(0, V - 1, (B, P), device="cuda")
    _, one, _ = timed(mt, prior, new)                                    # the one-token call's sample
    calls = {"off": {}}
    for T in (int(v) for v in a.lookahead.split(",")):
        calls[f"T={T} history"] = dict(lookahead=T)
        calls[f"T={T} guide"] = dict(lookahead=T, draft=timed(mt, prior, new, lookahead=T)[1])      # the call's own sample
    for kw in calls.values():
        timed(mt, prior, 64, **kw)                                       # warm-up (graph capture path)
    runs = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, kw in calls.items():                                      # in alternation
            full, out, st = timed(mt, prior, new, **kw)
            pre, _, _ = timed(mt, prior, 1, **kw)
            steps = st.get("steps_run", new)
            runs[k].append(dict(full=full, pre=pre, steps=steps, step=1e3 * (full - pre) / max(1, steps - 1),
                                per_step=B * new / (B * steps) if not kw else sum(st["tokens"]) / max(1, sum(st["steps"])),
                                same=1.0 if not kw else (out == one).all(1).float().mean().item(),
                                # the tokens every row shares with the one-token call's row before the first that differs
                                agree=[new] * B if not kw else ((out != one)[:, P:].int().cumsum(1) == 0).sum(1).tolist()))
    res = dict(shape=name, config=dict(d=d, layers=layers, V=V, B=B, P=P, new=new, reps=a.reps))
    for k, rs in runs.items():
        res[k] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                      steps=rs[0]["steps"], tokens_per_step=round(rs[0]["per_step"], 3), rows_identical=round(rs[0]["same"], 3),
                      tokens_before_first_difference=rs[0]["agree"],
                      tokens_per_s=spread([B * new / r["full"] for r in rs], 0))
    off = res["off"]["ms_per_step"]["median"]
    for k in calls:
        v = res[k]
        if k != "off":
            v["break_even_acceptance"] = round(v["ms_per_step"]["median"] / off - 1.0, 3)
        print(f"{name:10s} {k:12s}: B={B} P={P} +{new}: {v['ms_per_step']['median']:.4f} ms/step "
              f"({v['ms_per_step']['min']:.4f} .. {v['ms_per_step']['max']:.4f}), {v['steps']} steps, "
              f"{v['tokens_per_step']:.2f} tokens/step and row, {v['tokens_per_s']['median']:,.0f} tokens/s"
              + ("" if k == "off" else f"; rows identical to the one-token call's {100 * v['rows_identical']:.0f} % (first difference after "
                 f"{min(v['tokens_before_first_difference'])} .. {max(v['tokens_before_first_difference'])} tokens); break-even "
                 f"{v['break_even_acceptance']:+.2f} extra tokens/step"))
    print(json.dumps(res), flush=True)
    del mt
    torch.cuda.empty_cache()

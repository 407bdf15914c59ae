"""What the held-note state costs a step: generate_cached with ``note_rules`` (four more launches per step: the first draw and
mgx_notes_mask before the sampler, mgx_notes_keep and mgx_notes_account after it) against the same call without, on the same
prompts, graph on.  The unconstrained call is the code path of before the feature.  The two calls run in alternation, A/B/A/B, ``--reps`` times each (three at least) in one
process; a 1-token run of each measures its prefill, which is subtracted to give the per-step time.  The rule table is
EventSeq.note_rules over the first 308 ids of the vocabulary, so the mask bites and the two calls draw different tokens; the
share of the constrained rows that are well-formed is reported (it must be 1).

    python tools/note_state_decode_bench.py > profiles/r25_note_state_decode.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from musicgeneration_amd.network import MusicTransformer
from musicgeneration_amd.sequence import EventSeq, held_bits

SHAPES = {                                                               # d, layers, V, B, P, new
    "reference": (256, 6, 337, 8, 500, 2000),                            # generate.py -c prompt.mid -b 8
    "cfg5": (512, 6, 337, 32, 4096, 512),
}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-polyphony", type=int, default=None)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def timed(mt, prior, n, rules):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched", note_rules=rules,
                             max_polyphony=a.max_polyphony if rules is not None else None)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(vs, digits):
    return dict(min=round(min(vs), digits), median=round(statistics.median(vs), digits), max=round(max(vs), digits))


def well_formed(rule, row, P):
    """does the continuation of ``row`` break no rule, from its prompt's state?"""
    held = set(held_bits(rule, row[:P]).tolist())
    for t in row[P:]:
        r = int(rule[t])
        if r > 0 and (r - 1 in held or (a.max_polyphony is not None and len(held) >= a.max_polyphony)):
            return False
        if r < 0 and -r - 1 not in held:
            return False
        held = held | {r - 1} if r > 0 else held - {-r - 1} if r < 0 else held
    return True


for name in a.shapes.split(","):
    d, layers, V, B, P, new = SHAPES[name]
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
    prior = torch.randint(0, V - 1, (B, P), device="cuda")
    rules = EventSeq.note_rules(V)
    runs = {True: [], False: []}
    for constrained in (True, False):
        timed(mt, prior, 64, rules if constrained else None)            # warm-up (graph capture path)
    outs = {}
    for _ in range(a.reps):
        for constrained in (True, False):                               # A/B/A/B
            full, outs[constrained] = timed(mt, prior, new, rules if constrained else None)
            pre, _ = timed(mt, prior, 1, rules if constrained else None)
            runs[constrained].append(dict(full=full, pre=pre, step=1e3 * (full - pre) / (new - 1)))
    rows = {k: v.cpu().numpy() for k, v in outs.items()}
    res = dict(shape=name, config=dict(d=d, layers=layers, V=V, B=B, P=P, new=new, reps=a.reps, max_polyphony=a.max_polyphony),
               well_formed_rows={("notes" if k else "plain"): float(np.mean([well_formed(rules, r, P) for r in rows[k]])) for k in rows})
    for constrained, key in ((True, "notes"), (False, "plain")):
        rs = runs[constrained]
        res[key] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                        tokens_per_s=spread([B * new / r["full"] for r in rs], 0))
    t, c = res["notes"]["ms_per_step"], res["plain"]["ms_per_step"]
    res["notes_minus_plain_us_per_step"] = round(1e3 * (t["median"] - c["median"]), 2)
    res["notes_over_plain"] = round(t["median"] / c["median"], 4)
    res["verdict"] = "notes slower" if t["min"] > c["max"] else "notes faster" if t["max"] < c["min"] else \
        "no difference: inside the unconstrained call's run-to-run spread"
    for key in ("notes", "plain"):
        v = res[key]
        print(f"{name:10s} {key:6s}: B={B} P={P} +{new}: {v['ms_per_step']['median']:.4f} ms/step "
              f"({v['ms_per_step']['min']:.4f} .. {v['ms_per_step']['max']:.4f}), prefill {v['prefill_s']['median']:.3f} s, "
              f"{v['tokens_per_s']['median']:,.0f} tokens/s")
    print(f"{name:10s} notes - plain: {res['notes_minus_plain_us_per_step']} us/step, ratio {res['notes_over_plain']} "
          f"({res['verdict']}); well-formed rows: {res['well_formed_rows']}")
    print(json.dumps(res), flush=True)
    del mt
    torch.cuda.empty_cache()

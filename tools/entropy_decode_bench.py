"""What entropy-aware sampling costs a step: generate_cached with ``entropy_sampling`` against the same call without the keyword,
on the same prompts, graph on, on a model of the MIDI-like vocabulary (V = 309).  Three settings, each against "off": min-p alone
(one more launch per step, two comparisons per id), typical alone (the same launch with its bisection: 31 rounds of a masked sum
over the row), and Mirostat with the trace (the mask and the account: two more launches).  The four calls run in alternation
``--reps`` times each (three at least); a 1-token run of each measures its prefill, which is subtracted to give the per-step time.
Also the two kernels alone, back to back on one stream, beside mgx_sample_topk_topp alone (top-p on: one bisection of its own) on
the same logits.

    python tools/entropy_decode_bench.py > profiles/r31_entropy_sampling.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops
from musicgeneration_amd.decode import EntropySampling
from musicgeneration_amd.network import MusicTransformer
from musicgeneration_amd.sequence import EventSeq

SHAPES = {                                                               # d, layers, B, P, new
    "reference": (256, 6, 8, 500, 2000),                                 # generate.py -c prompt.mid -b 8
    "cfg5": (512, 6, 32, 4096, 512),
}
SETTINGS = {"off": None, "min_p": dict(min_p=0.05), "typical": dict(typical_p=0.9),
            "mirostat+trace": dict(tau=3.0, eta=0.1, trace=True)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def timed(mt, prior, n, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched", entropy_sampling=None if kw is None else EntropySampling(**kw))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(vs, digits):
    return dict(min=round(min(vs), digits), median=round(statistics.median(vs), digits), max=round(max(vs), digits))


def back_to_back(call, iters=400):
    """us per launch, back to back on one stream"""
    for _ in range(20):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / iters, 2)


def kernels_alone(B, V):
    """the mask (min-p alone, typical alone, all three stages), the account and the sampler (top-p 0.9) on the same random logits
    ~ N(0, 3^2).  The mask rewrites its input, so a device copy restores it before every launch; the copy is timed alone and
    taken off"""
    logits = (torch.randn(B, (V + 63) // 64 * 64, device="cuda") * 3).to(torch.bfloat16)
    keep = logits.clone()
    pos, tok = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    mu, lse = torch.full((B,), 6.0, device="cuda"), torch.zeros(B, device="cuda")
    trace = torch.zeros(B, 8, device="cuda")
    res = dict(sampler_us=back_to_back(lambda: ops.sample_topk_topp(keep, V, pos, tok, temperature=1.0, top_p=0.9, advance=False)))
    res["copy_us"] = back_to_back(lambda: logits.copy_(keep))
    for name, kw in (("mask_min_p_us", dict(min_p=0.05)), ("mask_typical_us", dict(typical_p=0.9)),
                     ("mask_all_us", dict(min_p=0.05, typical_p=0.9, mu=mu))):
        res[name] = round(back_to_back(lambda: ops.entropy_mask(logits.copy_(keep), V, 1.0, lse_out=lse, **kw)) - res["copy_us"], 2)
    res["account_us"] = back_to_back(lambda: ops.entropy_account(tok, keep, V, 1.0, lse, pos, mu=mu, tau=3.0, eta=0.0, surprise_out=trace))
    return res


for name in a.shapes.split(","):
    d, layers, B, P, new = SHAPES[name]
    V = EventSeq.dim() + 1
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
    prior = torch.randint(0, V - 1, (B, P), device="cuda")
    runs = {k: [] for k in SETTINGS}
    for k in SETTINGS:
        timed(mt, prior, 64, SETTINGS[k])                               # warm-up (graph capture path)
    for _ in range(a.reps):
        for k in SETTINGS:                                              # off / min-p / typical / Mirostat, in alternation
            full, _ = timed(mt, prior, new, SETTINGS[k])
            pre, _ = timed(mt, prior, 1, SETTINGS[k])
            runs[k].append(dict(full=full, pre=pre, step=1e3 * (full - pre) / (new - 1)))
    res = dict(shape=name, config=dict(d=d, layers=layers, V=V, B=B, P=P, new=new, reps=a.reps))
    for k, rs in runs.items():
        res[k] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                      tokens_per_s=spread([B * new / r["full"] for r in rs], 0))
    off = res["off"]["ms_per_step"]
    for k in SETTINGS:
        if k == "off":
            continue
        on = res[k]["ms_per_step"]
        res[k]["minus_off_us_per_step"] = round(1e3 * (on["median"] - off["median"]), 2)
        res[k]["verdict"] = "slower" if on["min"] > off["max"] else "faster" if on["max"] < off["min"] else \
            "no difference: inside the run-to-run spread of the call without the keyword"
    res["kernels_alone"] = kernels_alone(B, V)
    for k in SETTINGS:
        v = res[k]
        print(f"{name:10s} {k:14s}: B={B} P={P} +{new}: {v['ms_per_step']['median']:.4f} ms/step "
              f"({v['ms_per_step']['min']:.4f} .. {v['ms_per_step']['max']:.4f}), prefill {v['prefill_s']['median']:.3f} s, "
              f"{v['tokens_per_s']['median']:,.0f} tokens/s"
              + ("" if k == "off" else f"; - off: {v['minus_off_us_per_step']} us/step ({v['verdict']})"))
    ka = res["kernels_alone"]
    print(f"{name:10s} kernels alone, B={B} V={V}: mgx_entropy_mask {ka['mask_min_p_us']} us (min-p) / {ka['mask_typical_us']} us "
          f"(typical) / {ka['mask_all_us']} us (all three stages), a device copy of {ka['copy_us']} us that restores its input taken "
          f"off; mgx_entropy_account {ka['account_us']} us; mgx_sample_topk_topp {ka['sampler_us']} us")
    print(json.dumps(res), flush=True)
    del mt
    torch.cuda.empty_cache()

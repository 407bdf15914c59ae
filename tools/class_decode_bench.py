"""What per-class sampling costs a step: generate_cached with ``class_sampling`` (one more launch per step, captured with it) against
the same call without the keyword, on the same prompts, graph on.  Two class sets, each on a model of its codec's vocabulary and
with EVERY class filtered (a temperature, a top-k and a top-p of its own: the most the kernel can be asked): the MIDI-like
classes (C = 5, V = 309) and MuMIDI's (C = 11, V = 486).  The two calls run in alternation ``--reps`` times each (three at
least); a 1-token run of each measures its prefill, which is subtracted to give the per-step time.  Also the kernel alone, back
to back on one stream, beside mgx_sample_topk_topp alone (top-k and top-p on) on the same logits: a launch that cost more than
the sampler's time times the number of filtered classes would be walking the classes one after the other.

    python tools/class_decode_bench.py > profiles/r30_class_sampling.txt"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops
from musicgeneration_amd.decode import ClassSampling
from musicgeneration_amd.MuMIDI import MuMIDI_EventSeq
from musicgeneration_amd.network import MusicTransformer
from musicgeneration_amd.sequence import EventSeq

SHAPES = {                                                               # d, layers, B, P, new
    "reference": (256, 6, 8, 500, 2000),                                 # generate.py -c prompt.mid -b 8
    "cfg5": (512, 6, 32, 4096, 512),
}
CODECS = {"midi_like": EventSeq, "mumidi": MuMIDI_EventSeq}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
assert a.reps >= 3, "three runs of each call at least: the spread is part of the result"


def every_class_filtered(classes, C):
    return ClassSampling(classes, [0.7 + 0.05 * c for c in range(C)], [3 + c for c in range(C)], [0.9] * C)


def timed(mt, prior, n, cs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mt.generate_cached(prior, n, top_p=0.9, seed=0, prefill="batched", class_sampling=cs)
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


def kernels_alone(B, V, classes, C):
    """the class kernel (every class filtered) and the sampler (top-k 40, top-p 0.9) on the same random logits ~ N(0, 3^2).  The
    class kernel rewrites its input, so a device copy restores it before every launch; the copy is timed alone and taken off"""
    logits = (torch.randn(B, (V + 63) // 64 * 64, device="cuda") * 3).to(torch.bfloat16)
    cs = every_class_filtered(classes, C)
    cs.call_temperature = 1.0
    cs.stage("cuda")
    pos, tok = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    keep = logits.clone()
    sampler = back_to_back(lambda: ops.sample_topk_topp(keep, V, pos, tok, temperature=1.0, top_k=40, top_p=0.9, advance=False))
    first = back_to_back(lambda: ops.class_logits(logits.copy_(keep), V, cs.cls, cs.inv_temp, cs.k, cs.p, 1.0))
    copy = back_to_back(lambda: logits.copy_(keep))
    return dict(sampler_us=sampler, class_logits_us=round(first - copy, 2), copy_us=copy)


for name in a.shapes.split(","):
    d, layers, B, P, new = SHAPES[name]
    for codec, Codec in CODECS.items():
        V = Codec.dim() + 1
        names, classes = Codec.event_classes(V)
        C = len(names)
        torch.manual_seed(0)
        mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=layers, max_seq=P + new, dropout=0.0).cuda().eval()
        prior = torch.randint(0, V - 1, (B, P), device="cuda")
        settings = {"off": None, "on": every_class_filtered(classes, C)}
        runs = {k: [] for k in settings}
        for k in settings:
            timed(mt, prior, 64, settings[k])                           # warm-up (graph capture path)
        for _ in range(a.reps):
            for k in settings:                                          # off / on, in alternation
                full, _ = timed(mt, prior, new, settings[k])
                pre, _ = timed(mt, prior, 1, settings[k])
                runs[k].append(dict(full=full, pre=pre, step=1e3 * (full - pre) / (new - 1)))
        res = dict(shape=name, classes=codec, config=dict(d=d, layers=layers, V=V, C=C, B=B, P=P, new=new, reps=a.reps))
        for k, rs in runs.items():
            res[k] = dict(ms_per_step=spread([r["step"] for r in rs], 4), prefill_s=spread([r["pre"] for r in rs], 3),
                          tokens_per_s=spread([B * new / r["full"] for r in rs], 0))
        off, on = res["off"]["ms_per_step"], res["on"]["ms_per_step"]
        res["on"]["minus_off_us_per_step"] = round(1e3 * (on["median"] - off["median"]), 2)
        res["on"]["verdict"] = "slower" if on["min"] > off["max"] else "faster" if on["max"] < off["min"] else \
            "no difference: inside the run-to-run spread of the call without the keyword"
        res["kernels_alone"] = kernels_alone(B, V, classes, C)
        for k in settings:
            v = res[k]
            print(f"{name:10s} {codec:9s} C={C:2d} {k:3s}: B={B} P={P} +{new}: {v['ms_per_step']['median']:.4f} ms/step "
                  f"({v['ms_per_step']['min']:.4f} .. {v['ms_per_step']['max']:.4f}), prefill {v['prefill_s']['median']:.3f} s, "
                  f"{v['tokens_per_s']['median']:,.0f} tokens/s"
                  + ("" if k == "off" else f"; - off: {v['minus_off_us_per_step']} us/step ({v['verdict']})"))
        ka = res["kernels_alone"]
        print(f"{name:10s} {codec:9s} C={C:2d} kernels alone, B={B} V={V}: mgx_class_logits {ka['class_logits_us']} us (every class "
              f"filtered; a device copy of {ka['copy_us']} us that restores its input taken off), mgx_sample_topk_topp "
              f"{ka['sampler_us']} us; {C} x the sampler = {round(C * ka['sampler_us'], 1)} us")
        print(json.dumps(res), flush=True)
        del mt
        torch.cuda.empty_cache()

"""Digests of the kernels that read a logits row as the sampler does (csrc/logit_row.hpp): a fixed, seeded list of direct ops
calls -- sample_topk_topp, class_logits, entropy_mask, lookahead_accept, beam_select, token_logprob -- one SHA-256 per case over
the output bytes (contiguous CPU copy).  Every vocabulary size runs 10 rows: 8 whose previous tokens 0..7 pick all four kinds of
grammar row (a random half, three ids, one id, nothing), one with a third of its logits at -inf and one with ties across the
k-th value; with and without the grammar table, and -- where the call has them -- top_k in 0, 5, V and top_p in 1, 0.9, 1e-6.
Two libraries (MGX_LIB_PATH) compute the same thing bit for bit when their lists agree line for line."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicgeneration_amd import ops

ROWS, T, OUT_LD, TEMP, SEED = 10, 2, 16, 0.9, 7
VS = [1, 63, 64, 65, 337, 1023, 1024]                      # one id, the lane-slot boundary, the vocabulary, the last slot, the limit
I32, F32 = torch.int32, torch.float32


def show(name, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for x in outs:
        h.update(x.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    print(f"{name:58s} {h.hexdigest()}", flush=True)


def grammar(V, g):
    """bit v of row t: v may follow t.  t % 4 == 0: a random half, 1: three ids, 2: exactly one, 3: nothing"""
    allow = torch.zeros(V, V, dtype=torch.bool)
    for t in range(V):
        if t % 4 == 0:
            allow[t] = torch.rand(V, generator=g) < 0.5
        elif t % 4 < 3:
            allow[t, torch.randperm(V, generator=g)[:3 if t % 4 == 1 else 1]] = True
    bits = torch.zeros(V, (V + 31) // 32 * 32, dtype=torch.int64)
    bits[:, :V] = allow
    words = (bits.view(V, -1, 32) << torch.arange(32)).sum(2)                  # < 2^32
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(I32).cuda()


def logits_rows(V, g, rows=ROWS):
    """bf16 [rows, ld], NaN in the padding columns; the last row but one has a third of its ids at -inf, the last one the values
    ranked 3rd .. 8th equal: a tie across the k-th value of top_k = 5"""
    ld = (V + 7) // 8 * 8 + 8
    x = 2 * torch.randn(rows, V, generator=g)
    x[rows - 2, torch.randperm(V, generator=g)[:V // 3]] = float("-inf")
    order = x[rows - 1].argsort(descending=True)
    x[rows - 1, order[2:8]] = float(x[rows - 1, order[min(4, V - 1)]])
    full = torch.full((rows, ld), float("nan"))
    full[:, :V] = x
    return full.bfloat16().cuda()


def i32(*shape, value=0):
    return torch.full(shape, value, dtype=I32, device="cuda")


for V in VS:
    g = torch.Generator().manual_seed(1000 + V)
    table, lg = grammar(V, g), logits_rows(V, g)
    prev = (torch.arange(ROWS) % V).to(I32).cuda()                             # rows 0..7: every kind of grammar row, twice
    cls = (torch.arange(V) % 3).to(I32).cuda()
    guess = torch.randint(0, V, (ROWS // T,), generator=g).to(I32).cuda()
    target = torch.randint(0, V, (ROWS,), generator=g).to(I32).cuda()
    K = min(2, V)                                                              # beams per prompt
    for tab, tname in ((None, "no table"), (table, "table")):
        for k in (0, 5, V):
            for p in (1.0, 0.9, 1e-6):
                case = f"V={V} {tname} top_k={k} top_p={p:g}"
                tok, out, probs = prev.clone(), i32(ROWS, OUT_LD, value=-1), torch.zeros(ROWS, V, device="cuda")
                ops.sample_topk_topp(lg, V, i32(1, value=3), tok, out, probs, TEMP, k, p, SEED, allow_table=tab)
                show("sample_topk_topp " + case, tok, out, probs)
                x = lg.clone()
                ops.class_logits(x, V, cls, torch.tensor([1.0, 1.25, 0.7], device="cuda"), torch.tensor([k, k, 0], dtype=I32).cuda(),
                                 torch.tensor([p, 1.0, p], device="cuda"), TEMP, None if tab is None else prev, tab)
                show("class_logits " + case, x.view(torch.int16))
                B = ROWS // T                                                  # row b * T + i of lg: position i of row b
                draft = torch.stack([prev[:B], guess], 1).contiguous()
                tok, pos, done = prev[:B].clone(), i32(B, value=3), i32(B)
                out, stats, probs = i32(B, OUT_LD, value=-1), i32(B, 2), torch.zeros(B, OUT_LD, V, device="cuda")
                ops.lookahead_accept(lg, V, pos, draft, i32(B, value=12), tok, out, done, probs_all=probs, stats=stats,
                                     temperature=TEMP, top_k=k, top_p=p, seed=SEED, allow_table=tab)
                show("lookahead_accept " + case, tok, pos, out, done, stats, probs)
        case = f"V={V} {tname}"
        for name, kw in (("min_p typical", dict(min_p=0.05, typical_p=0.9)), ("mirostat", dict(mu=torch.linspace(1, 9, ROWS).cuda()))):
            x, lse = lg.clone(), torch.zeros(ROWS, device="cuda")
            ops.entropy_mask(x, V, TEMP, lse_out=lse, tok=None if tab is None else prev, allow_table=tab, **kw)
            show(f"entropy_mask {name} {case}", x.view(torch.int16), lse)
        for stochastic in (False, True):
            score = torch.zeros(ROWS // K, K, device="cuda")
            score[0, K - 1] = float("-inf")                                    # a dead beam
            tok, parent, hist = prev.clone(), i32(ROWS), (i32(ROWS, OUT_LD, value=-1), i32(ROWS, OUT_LD, value=-1))
            ops.beam_select(lg, V, score, tok, parent, i32(ROWS, value=3), *hist, TEMP, tab, stochastic, SEED)
            show(f"beam_select {'stochastic ' if stochastic else ''}{case}", tok, parent, score)
        show("token_logprob " + case, *ops.token_logprob(lg[:, :V], target, TEMP, None if tab is None else prev, tab))

"""The tensor contracts of the decode-path wrappers of ops.py (from _step_pos to score_reduce), on the host: every wrapper checks
its tensors before it asks for device memory, so on CPU tensors a well-formed call gets as far as the refusal of CPU memory
(MgxError, "CUDA/HIP") and nothing is launched, and a malformed one is refused before that with a ValueError that names the
wrapper and the argument.  Table-driven, after _wrappers() of test_ragged_args.py; no GPU.

The table holds the arguments that HAVE a host contract.  The oldest wrappers check their positions, caches and grammar table
on the host and leave the rest to the library's own refusals; those arguments are fixed inside the case's call and are not
perturbed here: decode_embed's and decode_embed_linear's tok, table, pe, w, bias and out / hout; rel_attn_decode's qkv_new, E and
ctx; sample_topk_topp's logits, next_tok, out_tokens and probs_out; the workspace of the three attention wrappers."""
import inspect

import pytest

torch = pytest.importorskip("torch")

B, V, D = 3, 20, 64
T, K, C, N = 2, 2, 2, 2                                    # guesses per step, beams, classes, samples per prompt
W = (V + 31) // 32
_BF, _I32, _F32 = torch.bfloat16, torch.int32, torch.float32


def _z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


class Case:
    """one wrapper: ``args`` name -> value of a well-formed call, ``call`` the wrapper on them, ``tensors`` the arguments that
    have a contract -- name -> what a refusal of each perturbation names in its message (default: the argument's own name;
    False under "short": every length is within the argument's contract, so a shorter one is accepted) -- and ``optional``
    name -> the arguments that become None with it (an argument that goes together with another leaves together with it)"""

    def __init__(self, call, args, tensors, optional=None):
        self.call, self.args, self.tensors, self.optional = call, args, tensors, optional or {}

    def run(self, **changed):
        return self.call({**self.args, **changed})


def _cache(rows=B, L=8, dtype=_BF):
    return _z(dtype, rows, 1, L, 64)


POS = dict.fromkeys(("dtype", "short", "strided"), "positions?")         # _step_pos's own wording (the blames are patterns)
OTHER = lambda name: dict(short=name)                                  # the argument sets a size: the next one is found short


def _cases():
    from musicgeneration_amd import ops
    table, pe, E = _z(_F32, V, D), _z(_F32, 8, D), _z(_BF, 8, 64)
    gram = dict(tok=_z(_I32, B), allow_table=_z(_I32, V, W))
    c = {}
    c["decode_embed"] = Case(lambda a: ops.decode_embed(gram["tok"], table, pe, a["pos_dev"], _z(_BF, B, D), ragged=True),
                             dict(pos_dev=_z(_I32, B)), dict(pos_dev=POS))
    c["decode_embed_linear"] = Case(
        lambda a: ops.decode_embed_linear(gram["tok"], table, pe, a["pos_dev"], _z(_BF, 32, D), None, _z(_BF, B, D), ragged=True),
        dict(pos_dev=_z(_I32, B)), dict(pos_dev=POS))
    c["kv_store_fp8"] = Case(
        lambda a: ops.kv_store_fp8(a["qkv"], 2, a["kcache"], a["vcache"], a["kscale"], a["vscale"]),
        dict(qkv=_z(_BF, B, 4, 3 * D), kcache=_cache(dtype=torch.uint8), vcache=_cache(dtype=torch.uint8), kscale=_z(_F32, B, 1, 8),
             vscale=_z(_F32, B, 1, 8)),
        dict(qkv={}, kcache=OTHER("vcache"), vcache=dict(dtype="8-bit caches must both"), kscale={}, vscale={}))
    c["rel_attn_decode"] = Case(
        lambda a: ops.rel_attn_decode(_z(_BF, B, 3 * D), a["kcache"], a["vcache"], E, a["pos_dev"], _z(_BF, B, D), ragged=True),
        dict(kcache=_cache(), vcache=_cache(), pos_dev=_z(_I32, B)), dict(kcache=OTHER("vcache"), vcache={}, pos_dev=POS))
    R = B * N
    c["rel_attn_decode_shared"] = Case(
        lambda a: ops.rel_attn_decode_shared(a["qkv_new"], a["kpre"], a["vpre"], a["kown"], a["vown"], a["E"], a["pos_rows"],
                                             a["pre_rows"], a["ctx"], None, N),
        dict(qkv_new=_z(_BF, R, 3 * D), kpre=_cache(), vpre=_cache(), kown=_cache(R), vown=_cache(R), E=E, pos_rows=_z(_I32, R),
             pre_rows=_z(_I32, B), ctx=_z(_BF, R, D)),
        dict(qkv_new={}, kpre=OTHER("vpre"), vpre={}, kown=OTHER("vown"), vown={}, E=dict(short=False), pos_rows=POS, pre_rows={},
             ctx={}))
    c["sample_topk_topp"] = Case(
        lambda a: ops.sample_topk_topp(_z(_BF, B, 32), V, a["pos_dev"], _z(_I32, B), _z(_I32, B, 16), allow_table=a["allow_table"],
                                       ragged=True, base=a["base"]),
        dict(pos_dev=_z(_I32, B), base=_z(_I32, B), allow_table=gram["allow_table"]), dict(pos_dev=POS, base={}, allow_table={}),
        dict(base=["base"], allow_table=["allow_table"]))
    c["decode_reanchor"] = Case(
        lambda a: ops.decode_reanchor(a["pos_dev"], a["base"], a["out_tokens"], a["seq"], 2, 0, ragged=True),
        dict(pos_dev=_z(_I32, B), base=_z(_I32, B), out_tokens=_z(_I32, B, 16), seq=_z(_I32, B, 32)),
        dict(pos_dev=POS, base={}, out_tokens={}, seq=OTHER("positions?")))
    c["budget_mask"] = Case(
        lambda a: ops.budget_mask(a["logits"], V, a["cost"], a["remaining"], a["done"]),
        dict(logits=_z(_BF, B, 32), cost=_z(_I32, V), remaining=_z(_I32, B), done=_z(_I32, B)),
        dict(logits={}, cost={}, remaining=OTHER("logits"), done={}))
    c["budget_account"] = Case(
        lambda a: ops.budget_account(a["next_tok"], a["out_tokens"], a["pos_dev"], a["cost"], a["remaining"], a["done"], a["count"], 0,
                                     ragged=True, base=a["base"]),
        dict(next_tok=_z(_I32, B), out_tokens=_z(_I32, B, 16), pos_dev=_z(_I32, B), cost=_z(_I32, V), remaining=_z(_I32, B),
             done=_z(_I32, B), count=_z(_I32, B), base=_z(_I32, B)),
        dict(next_tok={}, out_tokens={}, pos_dev=POS, cost=dict(short=False), remaining=OTHER("positions?"), done={}, count={}, base={}),
        dict(base=["base"]))
    c["repeat_penalty"] = Case(
        lambda a: ops.repeat_penalty(a["logits"], V, a["out_tokens"], a["pos_dev"], a["subject"], a["pen"], a["window"], ragged=True,
                                     base=a["base"]),
        dict(logits=_z(_BF, B, 32), out_tokens=_z(_I32, B, 16), pos_dev=_z(_I32, B), subject=_z(_I32, V), pen=_z(_F32, 5), window=4,
             base=_z(_I32, B)),
        dict(logits=OTHER("positions?"), out_tokens={}, pos_dev=POS, subject={}, pen={}, base={}),
        dict(base=["base"], subject=["subject", "pen", "window"]))
    c["class_logits"] = Case(
        lambda a: ops.class_logits(a["logits"], V, a["cls"], a["inv_temp"], a["top_k"], a["top_p"], 1.0, a["tok"], a["allow_table"]),
        dict(logits=_z(_BF, B, 32), cls=_z(_I32, V), inv_temp=_z(_F32, C), top_k=_z(_I32, C), top_p=_z(_F32, C), **gram),
        dict(logits=OTHER("tok"), cls={}, inv_temp=OTHER("top_k"), top_k={}, top_p={}, tok={}, allow_table={}),
        dict(tok=["tok", "allow_table"]))
    c["entropy_mask"] = Case(
        lambda a: ops.entropy_mask(a["logits"], V, 1.0, mu=a["mu"], lse_out=a["lse_out"], tok=a["tok"], allow_table=a["allow_table"]),
        dict(logits=_z(_BF, B, 32), mu=_z(_F32, B), lse_out=_z(_F32, B), **gram),
        dict(logits=OTHER("mu"), mu={}, lse_out={}, tok={}, allow_table={}),
        dict(mu=["mu"], lse_out=["lse_out"], tok=["tok", "allow_table"]))
    c["entropy_account"] = Case(
        lambda a: ops.entropy_account(a["next_tok"], a["logits"], V, 1.0, a["lse"], a["pos_dev"], a["mu"], 3.0, 0.1, a["surprise_out"],
                                      ragged=True, base=a["base"]),
        dict(next_tok=_z(_I32, B), logits=_z(_BF, B, 32), lse=_z(_F32, B), pos_dev=_z(_I32, B), mu=_z(_F32, B),
             surprise_out=_z(_F32, B, 16), base=_z(_I32, B)),
        dict(next_tok={}, logits=OTHER("positions?"), lse={}, pos_dev=POS, mu={}, surprise_out={}, base={}),
        dict(mu=["mu"], surprise_out=["surprise_out"], base=["base"]))
    c["lookahead_draft"] = Case(
        lambda a: ops.lookahead_draft(a["tok"], a["out_tokens"], a["pos_dev"], a["draft"], a["pos_rows"], 8, 0, guide=a["guide"],
                                      base=a["base"]),
        dict(tok=_z(_I32, B), out_tokens=_z(_I32, B, 16), pos_dev=_z(_I32, B), draft=_z(_I32, B, T), pos_rows=_z(_I32, B * T),
             guide=_z(_I32, B, 16), base=_z(_I32, B)),
        dict(tok=OTHER("draft"), out_tokens={}, pos_dev=POS, draft={}, pos_rows={}, guide={}, base={}),
        dict(guide=["guide"], base=["base"]))
    c["rel_attn_decode_multi"] = Case(
        lambda a: ops.rel_attn_decode_multi(a["qkv_new"], a["kcache"], a["vcache"], a["E"], a["pos_dev"], a["ctx"], None, T),
        dict(qkv_new=_z(_BF, B * T, 3 * D), kcache=_cache(), vcache=_cache(), E=E, pos_dev=_z(_I32, B), ctx=_z(_BF, B * T, D)),
        dict(qkv_new={}, kcache=OTHER("vcache"), vcache={}, E=dict(short=False), pos_dev=POS, ctx={}))
    c["lookahead_accept"] = Case(
        lambda a: ops.lookahead_accept(a["logits"], V, a["pos_dev"], a["draft"], a["limit"], a["tok"], a["out_tokens"], a["done"],
                                       probs_all=a["probs_all"], stats=a["stats"], allow_table=a["allow_table"], base=a["base"]),
        dict(logits=_z(_BF, B * T, 32), pos_dev=_z(_I32, B), draft=_z(_I32, B, T), limit=_z(_I32, B), tok=_z(_I32, B),
             out_tokens=_z(_I32, B, 16), done=_z(_I32, B), probs_all=_z(_F32, B, 16, V), stats=_z(_I32, B, 2),
             allow_table=gram["allow_table"], base=_z(_I32, B)),
        dict(logits={}, pos_dev=POS, draft={}, limit={}, tok=OTHER("draft"), out_tokens={}, done={}, probs_all={}, stats={},
             allow_table={}, base={}),
        dict(probs_all=["probs_all"], stats=["stats"], allow_table=["allow_table"], base=["base"]))
    notes = dict(rule=_z(_I32, V), state=_z(_I32, B, ops.NOTE_WORDS))
    c["notes_mask"] = Case(lambda a: ops.notes_mask(a["logits"], V, a["rule"], a["state"]), dict(logits=_z(_BF, B, 32), **notes),
                           dict(logits={}, rule={}, state=OTHER("logits")))
    c["notes_account"] = Case(lambda a: ops.notes_account(a["next_tok"], a["rule"], a["state"], V), dict(next_tok=_z(_I32, B), **notes),
                              dict(next_tok={}, rule={}, state=OTHER("next_tok")))
    c["notes_keep"] = Case(
        lambda a: ops.notes_keep(a["first_tok"], a["next_tok"], a["out_tokens"], a["pos_dev"], a["rule"], a["state"], V=V, ragged=True,
                                 base=a["base"]),
        dict(first_tok=_z(_I32, B), next_tok=_z(_I32, B), out_tokens=_z(_I32, B, 16), pos_dev=_z(_I32, B), base=_z(_I32, B), **notes),
        dict(first_tok={}, next_tok={}, out_tokens={}, pos_dev=POS, rule={}, state=OTHER("positions?"), base={}),
        dict(out_tokens=["out_tokens"], base=["base"]))
    c["crop_augment"] = Case(
        lambda a: ops.crop_augment(a["corpus"], a["start"], a["avail"], a["x"], a["y"], 0, perm=a["perm"], shift_row=a["shift_row"],
                                   stretch_q=a["stretch_q"], ts0=0, n_ts=4, n_out=a["n_out"]),
        dict(corpus=_z(torch.uint16, 64), start=_z(torch.int64, B), avail=_z(_I32, B), x=_z(_I32, B, 4), y=_z(_I32, B, 4),
             perm=_z(_I32, 2, V), shift_row=_z(_I32, B), stretch_q=_z(_I32, B), n_out=_z(_I32, B)),
        dict(corpus=dict(short=False), start={}, avail={}, x=OTHER("y"), y={}, perm=dict(short=False), shift_row={}, stretch_q={},
             n_out={}),
        dict(y=["y"], perm=["perm", "shift_row"], stretch_q=["stretch_q"], n_out=["n_out"]))
    R = B * K
    c["beam_select"] = Case(
        lambda a: ops.beam_select(a["logits"], V, a["score"], a["tok"], a["parent"], a["pos_rows"], a["hist_tok"], a["hist_parent"],
                                  allow_table=a["allow_table"]),
        dict(logits=_z(_BF, R, 32), score=_z(_F32, B, K), tok=_z(_I32, R), parent=_z(_I32, R), pos_rows=_z(_I32, R),
             hist_tok=_z(_I32, R, 16), hist_parent=_z(_I32, R, 16), allow_table=gram["allow_table"]),
        dict(logits={}, score=OTHER("logits"), tok={}, parent={}, pos_rows={}, hist_tok={}, hist_parent={}, allow_table={}),
        dict(allow_table=["allow_table"]))
    c["kv_beam_reorder"] = Case(
        lambda a: ops.kv_beam_reorder(a["dst"], a["src"], a["parent"], a["pos_rows"], K),
        dict(dst=_cache(R), src=_cache(R), parent=_z(_I32, R), pos_rows=_z(_I32, R)),
        dict(dst=dict(dtype="src", short="src"), src={}, parent={}, pos_rows={}))
    c["beam_backtrack"] = Case(
        lambda a: ops.beam_backtrack(a["hist_tok"], a["hist_parent"], a["c0_rows"], a["out"], K, 4),
        dict(hist_tok=_z(_I32, R, 16), hist_parent=_z(_I32, R, 16), c0_rows=_z(_I32, R), out=_z(_I32, R, 16)),
        dict(hist_tok={}, hist_parent={}, c0_rows={}, out=OTHER("hist_tok")))
    c["token_logprob"] = Case(
        lambda a: ops.token_logprob(a["logits"], a["target"], prev=a["prev"], allow_table=a["allow_table"]),
        dict(logits=_z(_BF, B, V), target=_z(_I32, B), prev=_z(_I32, B), allow_table=gram["allow_table"]),
        dict(logits=OTHER("target"), target={}, prev={}, allow_table={}), dict(prev=["prev", "allow_table"]))
    c["linear_logprob"] = Case(
        lambda a: ops.linear_logprob(a["a"], a["w"], a["bias"], a["target"]),
        dict(a=_z(_BF, B, D), w=_z(_BF, V, D), bias=_z(_F32, V), target=_z(_I32, B)),
        dict(a=OTHER("target"), w=OTHER("bias"), bias={}, target={}), dict(bias=["bias"]))
    c["score_reduce"] = Case(lambda a: ops.score_reduce(a["logp"], a["hit"]), dict(logp=_z(_F32, B, 4), hit=_z(_I32, B, 4)),
                             dict(logp=OTHER("hit"), hit={}))
    return c


WRAPPERS = ["decode_embed", "decode_embed_linear", "kv_store_fp8", "rel_attn_decode", "rel_attn_decode_shared", "sample_topk_topp",
            "decode_reanchor", "budget_mask", "budget_account", "repeat_penalty", "class_logits", "entropy_mask", "entropy_account",
            "lookahead_draft", "rel_attn_decode_multi", "lookahead_accept", "notes_mask", "notes_account", "notes_keep",
            "crop_augment", "beam_select", "kv_beam_reorder", "beam_backtrack", "token_logprob", "linear_logprob", "score_reduce"]
# public functions of the range that take no tensor to check: sizes of scratch buffers and the grammar's conversion
NO_TENSOR_CONTRACT = ["rel_attn_decode_splits", "rel_attn_decode_workspace", "rel_attn_decode_shared_splits",
                      "rel_attn_decode_shared_workspace", "rel_attn_decode_multi_splits", "rel_attn_decode_multi_workspace",
                      "grammar_table"]
_WRONG_DTYPE = {_I32: torch.int64, torch.int64: _I32, _F32: torch.float64, _BF: _F32, torch.uint16: _I32, torch.uint8: _I32}


def test_the_wrapper_lists_cover_every_wrapper():
    from musicgeneration_amd import ops
    assert sorted(_cases()) == sorted(WRAPPERS)
    first, last = (inspect.getsourcelines(f)[1] for f in (ops._step_pos, ops.score_reduce))
    public = [n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")
              and first <= inspect.getsourcelines(f)[1] <= last]
    assert sorted(public) == sorted(WRAPPERS + NO_TENSOR_CONTRACT)
    for case in _cases().values():                                        # every tensor the table hands a call is perturbed
        assert sorted(n for n, v in case.args.items() if torch.is_tensor(v)) == sorted(case.tensors)


@pytest.mark.parametrize("name", WRAPPERS)
def test_a_well_formed_call_passes_every_host_check(name):
    from musicgeneration_amd._lib import MgxError
    case = _cases()[name]
    with pytest.raises(MgxError, match="CUDA/HIP"):
        case.run()
    for leave in case.optional.values():                                  # every optional argument is accepted as None
        with pytest.raises(MgxError, match="CUDA/HIP"):
            case.run(**{n: (0 if n == "window" else None) for n in leave})


def _perturbed(kind, t):
    if kind == "dtype":
        return t.to(_WRONG_DTYPE[t.dtype])
    if kind == "short":
        return t[:-1]                                                     # one entry, or one row, too few
    return torch.stack([t, t], dim=-1)[..., 0]                            # the same shape and values, every stride doubled


@pytest.mark.parametrize("kind", ["dtype", "short", "strided"])
@pytest.mark.parametrize("name", WRAPPERS)
def test_a_malformed_tensor_is_refused_by_name(name, kind):
    from musicgeneration_amd._lib import MgxError
    case = _cases()[name]
    for arg, blame in case.tensors.items():
        bad = _perturbed(kind, case.args[arg])
        assert kind != "strided" or (bad.shape == case.args[arg].shape and not bad.is_contiguous())
        who = blame.get(kind, arg)
        if who is False:                                                  # any length is well-formed
            with pytest.raises(MgxError, match="CUDA/HIP"):
                case.run(**{arg: bad})
            continue
        with pytest.raises(ValueError, match=rf"^{name}: .*\b{who}\b"):
            case.run(**{arg: bad})

"""Argument checks of the ragged-prompt decode (generate_cached(prior_lengths=...), generate.py --condition-files): they
run on the host before any device work, so they are tested without a GPU."""
import pytest
import torch

from decode_fixtures import host_model


@pytest.mark.parametrize("lens,length,kw,msg", [
    ([0, 5, 40], 10, {}, "1 .. 40"),                               # an empty prompt
    ([41, 5, 40], 10, {}, "1 .. 40"),                              # longer than prior is wide
    ([1, 5], 10, {}, "2 entries"),                                 # one length per row
    ([1, 5, 40], 57, {}, "max_seq"),                               # Pmax + length > max_seq
    ([1, 5, 40], 10, dict(prefill="token"), "prefill"),            # no token-by-token prefill of ragged prompts
    ([1, 5, 40], 10, dict(prefill="bogus"), "prefill"),
])
def test_prior_lengths_are_refused(lens, length, kw, msg):
    x = torch.randint(0, 300, (3, 40))
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, length, prior_lengths=lens, **kw)


def test_ragged_batched_prefill_that_pads_past_max_seq_is_refused():
    x = torch.randint(0, 300, (2, 90))                             # 89 prefill rows pad to 96 > max_seq 92
    with pytest.raises(ValueError, match="max_seq=92"):
        host_model(L=92).generate_cached(x, 2, prior_lengths=[90, 3])


def _midi(path, n):
    from musicgeneration_amd import smf
    smf.write_notes(path, [(80, 60 + i % 12, 0.5 * i, 0.5 * i + 0.25) for i in range(n)])
    return path


def test_condition_files_cli_refusals(tmp_path):
    from musicgeneration_amd import generate
    a, b = _midi(str(tmp_path / "a.mid"), 3), _midi(str(tmp_path / "b.mid"), 30)
    base = ["-o", str(tmp_path / "out"), "-d", "", "--condition-files", f"{a},{b}"]
    for extra in (["-c", a], ["--grammar"], ["--reference-mask"]):
        with pytest.raises(SystemExit, match="cannot be combined"):
            generate.main(base + extra)
    with pytest.raises(SystemExit) as e:
        generate.main(base + ["-l", "100", "-M", "128"])
    msg = str(e.value)
    from musicgeneration_amd.sequence import EventSeq, NoteSeq
    longest = len(EventSeq.from_note_seq(NoteSeq.from_midi_file(b)).to_array())
    assert f"({longest} events)" in msg and "-l 100" in msg and "-M 128" in msg


# ---- the step-position arguments of the ops wrappers (ops._step_pos): refused on the host, before any device work --------
_B, _D, _V = 3, 64, 20
_BF = torch.bfloat16


def _i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _wrappers():
    """name -> (call(pos, ragged, base), takes a base): every ops wrapper that takes a position, on CPU tensors that are
    otherwise well-formed, so that the position check is the only one that can refuse"""
    from musicgeneration_amd import ops
    tok, table, pe = _i32(_B), torch.zeros(_V, _D), torch.zeros(8, _D)
    hid, out = torch.zeros(_B, _D, dtype=_BF), _i32(_B, 16)
    cache, E = torch.zeros(_B, 1, 8, 64, dtype=_BF), torch.zeros(8, 64, dtype=_BF)
    rule, state = _i32(_V), _i32(_B, ops.NOTE_WORDS)
    return {
        "decode_embed": (lambda p, r, b: ops.decode_embed(tok, table, pe, p, hid, ragged=r), False),
        "decode_embed_linear": (lambda p, r, b: ops.decode_embed_linear(tok, table, pe, p, torch.zeros(32, _D, dtype=_BF), None, hid,
                                                                        ragged=r), False),
        "rel_attn_decode": (lambda p, r, b: ops.rel_attn_decode(torch.zeros(_B, 3 * _D, dtype=_BF), cache, cache.clone(), E, p, hid,
                                                                ragged=r), False),
        "sample_topk_topp": (lambda p, r, b: ops.sample_topk_topp(torch.zeros(_B, 32, dtype=_BF), _V, p, _i32(_B), out, ragged=r,
                                                                  base=b), True),
        "decode_reanchor": (lambda p, r, b: ops.decode_reanchor(p, _i32(p.numel()) if b is None else b, out, _i32(_B, 32), 2, 0,
                                                                ragged=r), True),
        "budget_account": (lambda p, r, b: ops.budget_account(_i32(_B), out, p, _i32(_V), _i32(_B), _i32(_B), _i32(_B), 0, ragged=r,
                                                              base=b), True),
        "notes_keep": (lambda p, r, b: ops.notes_keep(_i32(_B), _i32(_B), out, p, rule, state, ragged=r, base=b), True),
    }


WRAPPERS = ["decode_embed", "decode_embed_linear", "rel_attn_decode", "sample_topk_topp", "decode_reanchor", "budget_account",
            "notes_keep"]
WITH_BASE = ["sample_topk_topp", "decode_reanchor", "budget_account", "notes_keep"]


def test_the_wrapper_lists_cover_every_wrapper():
    table = _wrappers()
    assert sorted(table) == sorted(WRAPPERS) and sorted(n for n, (_, b) in table.items() if b) == sorted(WITH_BASE)


@pytest.mark.parametrize("name", WRAPPERS)
def test_positions_of_the_wrong_kind_are_refused(name):
    call, _ = _wrappers()[name]
    for ragged, n in ((False, 1), (True, _B)):
        with pytest.raises(ValueError, match="int32"):                     # wrong dtype
            call(torch.zeros(n, dtype=torch.int64), ragged, None)
        with pytest.raises(ValueError, match="int32"):
            call(torch.zeros(n, dtype=torch.float32), ragged, None)
    with pytest.raises(ValueError, match="contiguous"):                    # a strided view (one entry is always contiguous)
        call(_i32(2 * _B)[::2], True, None)
    for n in (1, _B - 1, _B + 1):                                          # ragged: one entry per row
        with pytest.raises(ValueError, match=f"{_B} entries"):
            call(_i32(n), True, None)
    for n in (0, 2, _B):                                                   # a shared counter is one entry
        with pytest.raises(ValueError, match="shared position"):
            call(_i32(n), False, None)


@pytest.mark.parametrize("name", WITH_BASE)
def test_a_base_of_another_shape_is_refused(name):
    call, _ = _wrappers()[name]
    for ragged, n, bad in ((False, 1, (0, 2, _B)), (True, _B, (1, _B - 1, _B + 1))):
        for m in bad:
            with pytest.raises(ValueError, match="base"):
                call(_i32(n), ragged, _i32(m))
        with pytest.raises(ValueError, match="base"):
            call(_i32(n), ragged, torch.zeros(n, dtype=torch.int64))


@pytest.mark.parametrize("name", WRAPPERS)
def test_well_formed_positions_pass_the_host_check(name):
    """what the helper lets through reaches the next check, which on CPU tensors is the one for device memory -- also for a
    ragged batch of one row, which a check on the entry count alone could not tell from a shared counter"""
    from musicgeneration_amd._lib import MgxError
    call, has_base = _wrappers()[name]
    for ragged, n in ((False, 1), (True, _B)):
        for base in ([None, _i32(n)] if has_base else [None]):
            with pytest.raises(MgxError, match="CUDA/HIP tensors"):
                call(_i32(n), ragged, base)

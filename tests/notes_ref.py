"""numpy references of the three held-note contracts of include/mgx.h (ABI 28), written from the header, and the fold they share:
what a row holds after a stream of tokens, and where a stream breaks a rule.  Imported by basename, like budget_ref / beam_ref.
A state is a Python set of bits here; ``words`` / ``bits_of`` convert to and from the device's int32 [NOTE_WORDS]."""
import numpy as np

NEG_INF_BF16 = np.uint16(0xFF80)
NOTE_WORDS = 4
NOTE_BITS = 32 * NOTE_WORDS


def words(bits):
    """a set of bits -> int32 [NOTE_WORDS]: bit k in word k >> 5 at bit k & 31"""
    w = [0] * NOTE_WORDS
    for k in bits:
        assert 0 <= k < NOTE_BITS
        w[k >> 5] |= 1 << (k & 31)
    return np.array(w, dtype=np.uint32).view(np.int32)


def bits_of(state_words):
    """int32 [NOTE_WORDS] -> the set of bits"""
    w = np.asarray(state_words, dtype=np.int32).view(np.uint32)
    return {k for k in range(NOTE_BITS) if (int(w[k >> 5]) >> (k & 31)) & 1}


def _rule(rule, v):
    """(kind, bit) of id v: kind +1 sets, -1 clears, 0 touches nothing (also a value outside -128 .. 128)"""
    r = int(rule[v])
    if r == 0 or abs(r) > NOTE_BITS:
        return 0, None
    return (1 if r > 0 else -1), abs(r) - 1


def banned_id(rule, v, held, max_on):
    """does mgx_notes_mask ban id v for a row holding the set ``held``?"""
    kind, k = _rule(rule, v)
    if kind > 0:
        return k in held or len(held) >= max_on
    return kind < 0 and k not in held


def banned(rule, V, held, max_on):
    """the ids v < V that mgx_notes_mask bans for a row holding the set ``held``: bool [V]"""
    return np.array([banned_id(rule, v, held, max_on) for v in range(V)], dtype=bool)


def mask(logit_bits, V, rule, state, max_on):
    """mgx_notes_mask: logit_bits uint16 [B, ld] (the bf16 bit patterns), state int32 [B, NOTE_WORDS] -> a new array of the bits
    the kernel must leave"""
    out = np.array(logit_bits, dtype=np.uint16, copy=True)
    for b in range(out.shape[0]):
        out[b, :V][banned(rule, V, bits_of(state[b]), max_on)] = NEG_INF_BF16
    return out


def apply(rule, V, held, tok):
    """one token applied to the set ``held`` (a new set): no validity check; a token outside 0 .. V-1 touches nothing"""
    held = set(held)
    if 0 <= tok < V:
        kind, k = _rule(rule, tok)
        if kind > 0:
            held.add(k)
        elif kind < 0:
            held.discard(k)
    return held


def account(next_tok, rule, state, V):
    """mgx_notes_account on a copy of state int32 [B, NOTE_WORDS]"""
    return np.stack([words(apply(rule, V, bits_of(state[b]), int(next_tok[b]))) for b in range(len(next_tok))])


def keep(first_tok, next_tok, out_tokens, pos, base, per_row, rule, state, max_on, V):
    """mgx_notes_keep on copies: -> (next_tok, out_tokens); out_tokens may be None, base None is 0"""
    next_tok = np.array(next_tok, dtype=np.int64, copy=True)
    out_tokens = None if out_tokens is None else np.array(out_tokens, dtype=np.int64, copy=True)
    for b in range(len(next_tok)):
        t = int(first_tok[b])
        if not 0 <= t < V or banned_id(rule, t, bits_of(state[b]), max_on):
            continue
        next_tok[b] = t
        at = b if per_row else 0
        col = (0 if base is None else int(base[at])) + int(pos[at])
        if out_tokens is not None and 0 <= col < out_tokens.shape[1]:
            out_tokens[b, col] = t
    return next_tok, out_tokens


def fold(rule, V, ids, held=()):
    """the set held after ``ids``, starting from ``held``"""
    held = set(held)
    for t in ids:
        held = apply(rule, V, held, int(t))
    return held


def first_break(rule, V, ids, held=(), max_on=NOTE_BITS):
    """the index of the first id of ``ids`` that the mask would have banned, walking the fold from ``held`` (None: the stream
    is well-formed and never turns a note on at or above the cap)"""
    held = set(held)
    for i, t in enumerate(ids):
        t = int(t)
        if 0 <= t < V and banned_id(rule, t, held, max_on):
            return i
        held = apply(rule, V, held, t)
    return None

"""numpy references of the two length-budget contracts of include/mgx.h (ABI 27), written from the header, and ``truncate``: what
a budgeted row must be, given the unbudgeted row it would otherwise have been.  Imported by basename, like beam_ref / score_ref."""
import numpy as np

NEG_INF_BF16 = np.uint16(0xFF80)
NO_BUDGET = 2 ** 31 - 1


def mask(logit_bits, V, cost, remaining, done):
    """mgx_budget_mask: logit_bits uint16 [B, ld] (the bf16 bit patterns) -> a new array of the bits the kernel must leave"""
    out = np.array(logit_bits, dtype=np.uint16, copy=True)
    for b in range(out.shape[0]):
        if done[b] != 0:
            continue
        for v in range(V):
            if int(cost[v]) > int(remaining[b]):
                out[b, v] = NEG_INF_BF16
    return out


def account(next_tok, out_tokens, pos, base, per_row, cost, remaining, done, count, pad_token, inclusive):
    """mgx_budget_account on copies: -> (next_tok, out_tokens, remaining, done, count); pos / base are read only (base None: 0)"""
    next_tok, out_tokens, remaining, done, count = (np.array(a, dtype=np.int64, copy=True)
                                                    for a in (next_tok, out_tokens, remaining, done, count))
    for b in range(len(remaining)):
        at = b if per_row else 0
        col = (0 if base is None else int(base[at])) + int(pos[at])
        drop = True
        if done[b] == 0:
            remaining[b] -= int(cost[next_tok[b]])
            drop = False
            if remaining[b] > 0:
                count[b] += 1
            else:
                done[b] = 1
                if inclusive:
                    count[b] += 1
                else:
                    drop = True
        if drop:
            next_tok[b] = pad_token
            if 0 <= col < out_tokens.shape[1]:
                out_tokens[b, col] = pad_token
    return next_tok, out_tokens, remaining, done, count


def truncate(tokens, start, cost, budget, inclusive, pad_token, steps=None):
    """the row a budget makes of the unbudgeted row ``tokens`` (1-d; its continuation begins at column ``start``), provided the
    mask never bit -- no token of the row costs more than what was left when it was drawn: -> (row, length, spent, end), the
    row with pad_token from its end on, the events kept, their cost, and the 1-based step at which the row ended (0: a budget of
    0 ends it before the first step; None: it never ended).  ``steps``: the steps the run made, where ``tokens`` is wider than
    start + steps (the columns a shorter prompt leaves at the end of a ragged batch)"""
    row = np.array(tokens, dtype=np.int64, copy=True)
    left, length, spent, end = int(budget), 0, 0, None
    if left == 0:
        end = 0
    else:
        for s, col in enumerate(range(start, len(row) if steps is None else min(len(row), start + steps))):
            c = int(cost[row[col]])
            assert c <= left, "the mask would have changed this row: truncate does not apply"
            left -= c
            if left > 0 or inclusive:
                length, spent = length + 1, spent + c
            if left <= 0:
                end = s + 1
                break
    row[start + length:] = pad_token
    return row, length, spent, end

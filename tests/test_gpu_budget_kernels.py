"""The two length-budget kernels (ABI 27) against the numpy restatement of their header contracts (tests/budget_ref.py).  Both
are integer work, so every check is exact: the logits' BITS after mgx_budget_mask -- the columns at and beyond V and the guard
bands included -- and all of mgx_budget_account's state.  The chained test plays six steps of a scripted token stream, the host
doing the sampler's writes and its advance between the calls, and must arrive at budget_ref.truncate's rows."""
import numpy as np
import pytest
import torch

import budget_ref
import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
POISON = -77777
PAD = 1000
# zeros, the largest time_shift (100), values on both sides of every `remaining` below, and one no budget could pay
COSTS = [0, 100, 1, 2, 49, 50, 51, 98, 99, 101, INT32_MAX, 0, 3]
ROW_SETS = [([1, 50, 50], [0, 0, 1]), ([99, 100, INT32_MAX], [0, 0, 0])]     # (remaining, done): B = 3, the third row of set 0 is done


def banded(a, dtype=torch.int32):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


@pytest.mark.parametrize("V", [1, 63, 64, 65, 337, 1024])
def test_mask(V):
    ld = (V + 63) // 64 * 64                                                  # V = 64 and 1024 leave no column beyond V: the band follows
    B = 3
    for si, (remaining, done) in enumerate(ROW_SETS):
        for shift in (0, 1, 5):
            rng = np.random.default_rng(1000 * V + 10 * si + shift)
            cost = np.array([COSTS[(v + shift) % len(COSTS)] for v in range(V)], dtype=np.int32)
            x = torch.from_numpy(rng.normal(size=(B, ld)) * 4.0).to(torch.bfloat16)
            x[:, V:] = float("nan")
            x[torch.from_numpy(rng.random((B, ld)) < 0.1)] = float("-inf")     # logits that already hold -inf (the grammar's)
            bits = x.view(torch.int16).numpy().view(np.uint16)
            lg, c, r, d = banded(x, torch.bfloat16), banded(cost), banded(remaining), banded(done)
            KC.ops().budget_mask(lg.t, V, c.t, r.t, d.t)
            torch.cuda.synchronize()
            want = budget_ref.mask(bits, V, cost, remaining, done)
            case = f"V={V} ld={ld} rows={remaining} done={done} shift={shift}"
            KC.check_equal("mask", KC.bits16(lg.t).to(torch.int32), torch.from_numpy(want.view(np.int16).astype(np.int32)), case)
            assert (want[:, V:] == bits[:, V:]).all()                          # the reference itself: columns >= V stay,
            if si == 0:
                assert (want[2] == bits[2]).all()                              # and so does the done row
            assert (want != bits).any() or V == 1                              # the case masks something
            for b in (lg, c, r, d):
                assert b.bands_intact(), case
            for b, a in ((c, cost), (r, remaining), (d, done)):                # the state is read only
                assert b.t.cpu().tolist() == list(map(int, a)), case


def account_case(B, per_row, with_base, seed, out_ld=16):
    """rows cycle through: live and staying live; ending exactly; already done; a cost-0 token; overshooting (no mask ran);
    no budget; done with its column outside the row.  Ragged rows sit at different positions"""
    rng = np.random.default_rng(seed)
    Vc = 12
    cost = rng.integers(1, 9, Vc).astype(np.int32)
    cost[3] = 0
    tok = rng.integers(0, Vc, B).astype(np.int32)
    tok[tok == 3] = 4
    kind = np.arange(B) % 7
    remaining = np.where(kind == 0, cost[tok] + 1 + rng.integers(0, 50, B), 0)
    remaining = np.where(kind == 1, cost[tok], remaining)
    remaining = np.where(kind == 2, rng.integers(0, 5, B), remaining)
    tok = np.where(kind == 3, 3, tok).astype(np.int32)
    remaining = np.where(kind == 3, 1 + rng.integers(0, 3, B), remaining)
    remaining = np.where(kind == 4, np.maximum(cost[tok] - 1, 1), remaining)
    remaining = np.where(kind == 5, INT32_MAX, remaining)
    remaining = np.where(kind == 6, 7, remaining)
    done = ((kind == 2) | (kind == 6)).astype(np.int32)
    count = rng.integers(0, 30, B).astype(np.int32)
    n = B if per_row else 1
    base = rng.integers(0, 4, n).astype(np.int32) if with_base else None
    pos = rng.integers(1, out_ld - 4, n).astype(np.int32)
    if per_row:                                                               # the done rows of kind 6: column out_ld, outside the row
        pos = np.where(kind == 6, out_ld - (base if with_base else 0), pos).astype(np.int32)
    out = rng.integers(0, Vc, (B, out_ld)).astype(np.int32)
    return dict(next_tok=tok, out=out, pos=pos, base=base, cost=cost, remaining=remaining.astype(np.int32), done=done, count=count)


@pytest.mark.parametrize("inclusive", [1, 0])
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_account(B, per_row, with_base, inclusive):
    c = account_case(B, per_row, with_base, seed=B * 8 + per_row * 4 + with_base * 2 + inclusive)
    dev = {k: None if v is None else banded(v) for k, v in c.items()}
    KC.ops().budget_account(dev["next_tok"].t, dev["out"].t, dev["pos"].t, dev["cost"].t, dev["remaining"].t, dev["done"].t,
                            dev["count"].t, PAD, bool(inclusive), ragged=bool(per_row), base=None if not with_base else dev["base"].t)
    torch.cuda.synchronize()
    tok, out, rem, done, count = budget_ref.account(c["next_tok"], c["out"], c["pos"], c["base"], per_row, c["cost"], c["remaining"],
                                                    c["done"], c["count"], PAD, inclusive)
    case = f"B={B} per_row={per_row} base={with_base} inclusive={inclusive}"
    for name, want in (("next_tok", tok), ("out", out), ("remaining", rem), ("done", done), ("count", count), ("pos", c["pos"]),
                       ("cost", c["cost"])) + ((("base", c["base"]),) if with_base else ()):
        KC.check_equal("account " + name, dev[name].t, torch.from_numpy(np.asarray(want, dtype=np.int64)), case)
        assert dev[name].bands_intact(), (case, name)
    if B >= 5:                                                                # the case holds every kind of row
        assert (done != c["done"]).any() and (rem != c["remaining"]).any() and (out != c["out"]).any()
        assert ((done == 0) & (count == c["count"] + 1)).any()


@pytest.mark.parametrize("inclusive", [1, 0])
@pytest.mark.parametrize("per_row", [0, 1])
def test_six_chained_steps_arrive_at_truncate(per_row, inclusive):
    """a scripted stream of six tokens per row; the host writes each where the sampler would and advances the position, the
    kernel charges it.  Budgets: the cost of a row's first 1, 3 and 6 tokens (it lands exactly there, or earlier where a token
    is free), 0, more than the row costs, and none"""
    steps, out_ld = 6, 12
    rng = np.random.default_rng(7 + per_row)
    cost = np.array([0, 1, 2, 3, 5, 0], dtype=np.int32)
    pad = 5
    script = rng.integers(0, 5, (6, steps)).astype(np.int32)
    script[:, 0] = np.maximum(script[:, 0], 1)                                # the first token costs something
    sums = np.cumsum(cost[script], 1)
    budgets = np.array([sums[0, 0], sums[1, 2], sums[2, 5], 0, sums[4, 5] + 5, INT32_MAX], dtype=np.int64)
    B = len(budgets)
    pos0 = (rng.integers(0, 4, B) if per_row else np.array([2])).astype(np.int32)
    start = (pos0 + 1) if per_row else np.repeat(pos0 + 1, B)
    out0 = np.full((B, out_ld), pad, dtype=np.int32)
    for b in range(B):
        out0[b, :start[b]] = 1 + b % 4                                        # a prompt
    full = out0.copy()                                                        # the unbudgeted rows
    for b in range(B):
        full[b, start[b]:start[b] + steps] = script[b]
    out, pos = banded(out0), banded(pos0)
    tok = banded(np.zeros(B, dtype=np.int32))
    c, rem = banded(cost), banded(budgets.astype(np.int32))
    done, count = banded((budgets == 0).astype(np.int32)), banded(np.zeros(B, dtype=np.int32))
    rows = torch.arange(B, device="cuda:0")
    for s in range(steps):
        t = torch.from_numpy(script[:, s].copy()).cuda()
        cols = (pos.t.long() + 1) if per_row else (pos.t.long() + 1).expand(B)
        out.t[rows, cols] = t                                                 # the sampler: column pos + 1, next_tok, advance
        tok.t.copy_(t)
        pos.t.add_(1)
        KC.ops().budget_account(tok.t, out.t, pos.t, c.t, rem.t, done.t, count.t, pad, bool(inclusive), ragged=bool(per_row))
    torch.cuda.synchronize()
    case = f"per_row={per_row} inclusive={inclusive}"
    ends = []
    for b in range(B):
        row, length, spent, end = budget_ref.truncate(full[b], start[b], cost, budgets[b], inclusive, pad, steps)
        ends.append(end)
        KC.check_equal("chain out", out.t[b], torch.from_numpy(row), f"{case} row {b}")
        assert int(count.t[b]) == length and int(done.t[b]) == (end is not None), (case, b)
        assert int(cost[out.t[b, start[b]:start[b] + length].cpu().numpy()].sum()) == spent
        assert int(tok.t[b]) == (pad if end is not None and (end < steps or not inclusive) else script[b, -1])
    assert ends[3] == 0 and ends[4] is None and ends[5] is None and ends[0] == 1 and 1 <= ends[1] <= 3 and ends[2] is not None
    assert int(pos.t[0]) == pos0[0] + steps                                   # the positions only ever advance
    for t_ in (out, pos, tok, c, rem, done, count):
        assert t_.bands_intact(), case

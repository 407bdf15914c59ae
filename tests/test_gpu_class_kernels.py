"""mgx_class_logits (ABI 33) against the fp64 restatement of its header contract (tests/class_ref.py), element by element.

The bound, for an id the reference keeps at ln p' = r:  |got - r| <= |r| 2^-8 + 3e-4.  The first term is half a bf16 spacing, the
one rounding of the result.  The second is the f32 evaluation: three log-sum-exps over <= 1024 terms at <= 1024 * 2^-24 = 6.1e-5
each, plus the rounding of the scaled exponent (|x - m| * inv_temp <= ~100 at 2^-24 relative: 6e-6) -- 1.9e-4, rounded up.  The
-inf set must be identical; the filter inputs are redrawn until every margin the reference reports for its own cuts is >= 1e-3
(asserted on the inputs alone, on the CPU), far above f32 error, so the two cannot disagree about a kept set there.  Exact ties
at a cut have a case of their own.  Buffers sit inside guard bands; everything the call only reads is compared afterwards."""
import numpy as np
import pytest
import torch

import class_ref
import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

SEEN = {}
_report = KC.report_fixture(SEEN, "largest |got - r| - |r| 2^-8 = {:.3g} (allowed 3e-4)")
F32_TERM = 3e-4
MARGIN = 1e-3
T_CALL = 0.9


def banded(a, dtype):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


def classes_for(V, C, layout):
    """contiguous runs (class 1 left without a member where there are four or more) or v % C"""
    if layout == "interleaved":
        return (np.arange(V) % C).astype(np.int32)
    use = [c for c in range(C) if not (C >= 4 and c == 1)]
    return np.asarray([use[min(v * len(use) // V, len(use) - 1)] for v in range(V)], dtype=np.int32)


def params_for(C, filtered=True):
    """every class with a temperature of its own and, with ``filtered``, the filters cycling through top-k, top-p, both, neither"""
    # 2.0 for class 0, the one that is cut by top-p alone however many ids it has: a nucleus over a thousand ids at a flat
    # temperature ends among probabilities of 1e-4, where no cut has a relative margin of 1e-3
    inv_temp = np.asarray([0.5 + 1.5 * ((7 * c + 15) % 16) / 15 for c in range(C)], dtype=np.float32)
    if not filtered:
        return inv_temp, np.zeros(C, dtype=np.int32), np.ones(C, dtype=np.float32)
    top_k = np.asarray([(0, 1, 3, 0)[c % 4] for c in range(C)], dtype=np.int32)
    top_p = np.asarray([(0.9, 1.0, 0.6, 1.0)[c % 4] for c in range(C)], dtype=np.float32)
    return inv_temp, top_k, top_p


def table_for(rng, V, tok):
    """a random grammar table (bit v of row t, ~70 % set) whose row of tok[3] -- where there is one -- allows nothing"""
    W = (V + 31) // 32
    bits = rng.random((V, W * 32)) < 0.7
    bits[:, V:] = False
    if len(tok) > 3:
        bits[min(max(tok[3], 0), V - 1)] = False
    words = (bits.reshape(V, W, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(-1).astype(np.uint32)
    return words


def draw_rows(rng, B, V, ld, cls, inv_temp, top_k, top_p, tok, table):
    """bf16-valued logits ~ N(0, 3^2) with ~10 % -inf, float64 [B, ld] (NaN beyond V), every row redrawn until the reference's
    margins on it are >= MARGIN.  In a batch of five, row 1 is all -inf, row 2 has class cls[0] all -inf, row 3's grammar row is
    empty (table_for) and row 4's grammar row allows only ids that are -inf"""
    x = np.full((B, ld), np.nan)
    for b in range(B):
        allowed = None if table is None else class_ref.allowed_bits(table, tok[b], V)
        for _ in range(500):
            r = class_ref.bf16_values(rng.normal(size=V) * 3.0)
            r[rng.random(V) < 0.1] = -np.inf
            if B == 5 and b == 1:
                r[:] = -np.inf
            if B == 5 and b == 2:
                r[cls == cls[0]] = -np.inf
            if B == 5 and b == 4 and allowed is not None:
                r[allowed] = -np.inf
            _, margins = class_ref.warp_row(r, cls, inv_temp, top_k, top_p, T_CALL, allowed)
            if all(m >= MARGIN for m in margins):
                break
        else:
            raise AssertionError("no row with wide margins in 500 draws")
        x[b, :V] = r
    return x


def run(x, V, cls, inv_temp, top_k, top_p, tok, table, case, temperature=T_CALL):
    """one call; -> the logits after it, float64 [B, ld] (their bf16 values), checked against the reference"""
    B, ld = x.shape
    ref, touched, margins = class_ref.warp(x, V, cls, inv_temp, top_k, top_p, temperature, tok, table)
    assert all(m >= MARGIN for m in margins), (case, min(margins))            # on the inputs alone
    before = torch.from_numpy(x).to(torch.bfloat16)
    lg, cl = banded(before, torch.bfloat16), banded(cls, torch.int32)
    it, tk, tp = banded(inv_temp, torch.float32), banded(top_k, torch.int32), banded(top_p, torch.float32)
    tb = None if table is None else banded(table.view(np.int32), torch.int32)
    to = None if table is None else banded(np.asarray(tok, dtype=np.int32), torch.int32)
    KC.ops().class_logits(lg.t, V, cl.t, it.t, tk.t, tp.t, temperature, tok=None if to is None else to.t,
                          allow_table=None if tb is None else tb.t)
    torch.cuda.synchronize()
    for b_ in (lg, cl, it, tk, tp, tb, to):
        assert b_ is None or b_.bands_intact(), case
    for b_, a in ((cl, cls), (it, inv_temp), (tk, top_k), (tp, top_p), (to, None if table is None else np.asarray(tok, dtype=np.int32)),
                  (tb, None if table is None else table.view(np.int32))):
        assert b_ is None or (b_.t.cpu().numpy() == a).all(), case           # what the call only reads
    bits0, bits1 = KC.bits16(before).numpy(), KC.bits16(lg.t).numpy()
    assert (bits1[:, V:] == bits0[:, V:]).all(), case                         # columns >= V
    assert (bits1[~touched] == bits0[~touched]).all(), case                   # a row with nothing to draw from: bit for bit
    got = lg.t.cpu().to(torch.float64).numpy()
    g, r = got[touched][:, :V], ref[touched]
    assert not np.isnan(g).any(), case
    assert ((g == -np.inf) == (r == -np.inf)).all(), (case, "the -inf sets differ", np.argwhere((g == -np.inf) != (r == -np.inf))[:4].tolist())
    fin = r > -np.inf
    if fin.any():
        excess = (np.abs(g[fin] - r[fin]) - np.abs(r[fin]) * 2.0 ** -8).max()
        if excess > SEEN.get("class_logits", (-np.inf, None))[0]:
            SEEN["class_logits"] = (excess, case)
        print(f"[class_logits] {case}: excess {excess:.3g}")
        assert excess <= F32_TERM, (case, excess)
    return got


@pytest.mark.parametrize("C", [1, 4, 16])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 337, 1024])
def test_against_the_reference(V, C):
    cases = rewritten = 0
    for B in (1, 5):
        for ld in (V, V + 7):
            for layout in ("contiguous", "interleaved"):
                for grammar in (False, True):
                    seed = (((V * 17 + C) * 2 + (B == 5)) * 2 + (ld > V)) * 4 + (layout == "interleaved") * 2 + grammar
                    rng = np.random.default_rng(seed)
                    cls = classes_for(V, C, layout)
                    inv_temp, top_k, top_p = params_for(C)
                    tok = rng.integers(0, V, B).tolist()
                    if B == 5:
                        tok[0] = V + 5                                         # clamped to the last row of the table
                    table = table_for(rng, V, tok) if grammar else None
                    x = draw_rows(rng, B, V, ld, cls, inv_temp, top_k, top_p, tok, table)
                    case = f"V={V} C={C} B={B} ld={ld} {layout} grammar={grammar}"
                    got = run(x, V, cls, inv_temp, top_k, top_p, tok, table, case)
                    cases += 1
                    rewritten += int((got[:, :V] != x[:, :V]).sum())
    assert cases == 16 and rewritten > 0


def test_unfiltered_classes_and_other_temperatures():
    """no filter anywhere (every finite id stays finite), and the call's temperature away from 1 in both directions"""
    V, C = 337, 5
    cls = classes_for(V, C, "contiguous")
    inv_temp, top_k, top_p = params_for(C, filtered=False)
    for T in (0.5, 1.0, 2.0):
        rng = np.random.default_rng(int(T * 10))
        x = draw_rows(rng, 5, V, V + 7, cls, inv_temp, top_k, top_p, [0] * 5, None)
        got = run(x, V, cls, inv_temp, top_k, top_p, None, None, f"unfiltered T={T}", temperature=T)
        for b in (0, 3, 4):
            assert ((got[b, :V] > -np.inf) == (x[b, :V] > -np.inf)).all()
        assert (got[2, :V][cls == cls[0]] == -np.inf).all()


def test_exact_ties_straddling_the_cuts():
    """equal bf16 logits on both sides of a top-k cut (class 0) and of a top-p cut (class 1): every tied id is kept"""
    V = 70
    x = np.full((1, V), -np.inf)
    cls = (np.arange(V) >= 35).astype(np.int32)
    cls[64] = 0                                                               # lane 0's second slot belongs to class 0
    x[0, [0, 64, 3, 33, 34]] = [2.0, 1.0, 1.0, 1.0, 0.5]                     # the tie spans two of a lane's slots and two lanes
    x[0, [35, 40, 65, 69, 66]] = [2.0, 1.0, 1.0, 1.0, 0.5]
    q = np.exp(x[0, [35, 40, 65, 69, 66]])
    q /= q.sum()
    inv_temp, top_k = np.ones(2, dtype=np.float32), np.asarray([2, 0], dtype=np.int32)
    top_p = np.asarray([1.0, q[0] + 0.5 * q[1]], dtype=np.float32)            # the nucleus ends inside the tie
    got = run(x, V, cls, inv_temp, top_k, top_p, None, None, "ties", temperature=1.0)
    assert np.flatnonzero(got[0] > -np.inf).tolist() == [0, 3, 33, 35, 40, 64, 65, 69]
    top_k, top_p = np.asarray([1, 0], dtype=np.int32), np.asarray([1.0, 0.99 * q[0]], dtype=np.float32)
    got = run(x, V, cls, inv_temp, top_k, top_p, None, None, "ties dropped together", temperature=1.0)
    assert np.flatnonzero(got[0] > -np.inf).tolist() == [0, 35]


def test_every_error_of_the_contract():
    lib, _, ptr, _ = KC.raw()
    V, ld, C, B = 65, 72, 4, 2
    lg = banded(torch.zeros(B, ld), torch.bfloat16)
    cl, it = banded(classes_for(V, C, "interleaved"), torch.int32), banded(np.ones(C), torch.float32)
    tk, tp = banded(np.zeros(C), torch.int32), banded(np.ones(C), torch.float32)
    tok, tb = banded(np.zeros(B), torch.int32), banded(np.zeros((V, 3)), torch.int32)
    before = KC.bits16(lg.t).clone()

    def call(**kw):
        a = dict(dict(logits=ptr(lg.t), V=V, ld=ld, cls=ptr(cl.t), C=C, it=ptr(it.t), k=ptr(tk.t), p=ptr(tp.t), t=1.0, tok=None,
                      table=None, B=B), **kw)
        return lib.mgx_class_logits(a["logits"], a["V"], a["ld"], a["cls"], a["C"], a["it"], a["k"], a["p"], a["t"], a["tok"],
                                    a["table"], a["B"], None)
    for kw in (dict(logits=None), dict(cls=None), dict(it=None), dict(k=None), dict(p=None), dict(tok=ptr(tok.t)), dict(table=ptr(tb.t))):
        assert call(**kw) == -2, kw                                           # MGX_ERR_NULL
    for kw in (dict(B=0), dict(B=-1), dict(V=0), dict(V=1025, ld=1025), dict(ld=V - 1), dict(C=0), dict(C=17), dict(t=0.0),
               dict(t=-0.5), dict(t=float("inf")), dict(t=float("nan"))):
        assert call(**kw) == -1, kw                                           # MGX_ERR_SHAPE
    torch.cuda.synchronize()
    assert torch.equal(KC.bits16(lg.t), before) and lg.bands_intact()         # a refused call launches nothing
    assert call() == 0 and call(tok=ptr(tok.t), table=ptr(tb.t)) == 0
    ops = KC.ops()
    with pytest.raises(ValueError, match="together"):
        ops.class_logits(lg.t, V, cl.t, it.t, tk.t, tp.t, 1.0, tok=tok.t)
    with pytest.raises(ValueError, match="bf16"):
        ops.class_logits(lg.t.float(), V, cl.t, it.t, tk.t, tp.t, 1.0)
    with pytest.raises(ValueError, match="top_k"):
        ops.class_logits(lg.t, V, cl.t, it.t, tk.t.float(), tp.t, 1.0)
    with pytest.raises(ValueError, match="cls"):
        ops.class_logits(lg.t, V, cl.t[:V - 1], it.t, tk.t, tp.t, 1.0)
    with pytest.raises(Exception, match="CUDA/HIP"):
        ops.class_logits(lg.t, V, cl.t.cpu(), it.t, tk.t, tp.t, 1.0)


def test_the_sampler_files_the_softmax_of_the_warped_row():
    """warp, then mgx_sample_topk_topp at temperature 1: probs_out is softmax of the rewritten row, the drawn token is a kept id,
    and with top_k[c] = 1 everywhere exactly one id per live class is nonzero"""
    V, C, B, ld = 337, 5, 4, 344
    cls = classes_for(V, C, "interleaved")
    ops = KC.ops()
    for name, (inv_temp, top_k, top_p) in (("filters", params_for(C)),
                                            ("top-k 1", (params_for(C)[0], np.ones(C, dtype=np.int32), np.ones(C, dtype=np.float32)))):
        rng = np.random.default_rng(len(name))
        x = draw_rows(rng, B, V, ld, cls, inv_temp, top_k, top_p, [0] * B, None)
        ref, _, margins = class_ref.warp(x, V, cls, inv_temp, top_k, top_p, T_CALL)
        assert all(m >= MARGIN for m in margins)
        lg = torch.from_numpy(x).to(torch.bfloat16).cuda()
        dev = lambda a, dt: torch.as_tensor(a).to(dt).cuda()                  # noqa: E731
        ops.class_logits(lg, V, dev(cls, torch.int32), dev(inv_temp, torch.float32), dev(top_k, torch.int32), dev(top_p, torch.float32),
                         T_CALL)
        probs = torch.zeros(B, V, device="cuda")
        tok = torch.zeros(B, dtype=torch.int32, device="cuda")
        ops.sample_topk_topp(lg, V, torch.zeros(1, dtype=torch.int32, device="cuda"), tok, probs_out=probs, temperature=1.0, seed=3,
                             advance=False)
        torch.cuda.synchronize()
        warped = lg.cpu().to(torch.float64)[:, :V]
        want = torch.softmax(warped, -1)
        KC.check_bound("sampler after warp", probs, want, torch.full_like(want, 2e-6), name, seen={})
        got = probs.cpu().numpy()
        for b in range(B):
            assert ((got[b] > 0) == (ref[b] > -np.inf)).all(), (name, b)
            assert got[b, int(tok[b])] > 0
            over = np.abs(got[b] - class_ref.filed(ref[b])) - class_ref.prob_bound(ref[b], F32_TERM) - 2e-6
            assert over.max() <= 0, (name, b, over.max())                     # and what the reference says is filed
            if name == "top-k 1":
                for c in range(C):
                    live = (x[b, :V][cls == c] > -np.inf).any()
                    assert (got[b][cls == c] > 0).sum() == (1 if live else 0), (name, b, c)

"""mgx_rel_attn_decode_shared (ABI 26), the decode attention of N samples per prompt over one shared prompt cache, against the
fp64 reference of the header contract (oracle/decode_ref.rel_attn_decode on K and V assembled as the prompt's rows, the row's own
rows and the step's new row), element by element.

Bound: that of tests/test_gpu_decode_kernels.py, |ctx - ref| <= 2^-8 |ref| + 16 F per element -- 2^-8 |ref| the bf16 rounding of
the output, F the fp32 noise floor of the reference formula (decode_ref.attn_noise_floor).  The kernel evaluates the formula of
mgx_rel_attn_decode with the same exp2 and the same merge tree, so the margin 16 is taken over, not calibrated here.
MEASURED on one MI355X over all cases of this module: the largest (|ctx - ref| - 2^-8 |ref|) / F was 3.46 (every logit near
-200, eight splits; 1.12 on Gaussian data) -- and wherever the repeated call takes the same split count the two agree bitwise.

Shapes: Bp = 2 prompts, d = 128 (two heads); (Lpre, Lown) so that mgx_rel_attn_decode_shared_splits returns 1, 2, 4, 8 and 16,
every value it has; N in {1, 2, 3, NQ, NQ + 1, 16} (NQ = MGX_SHARED_NQ queries per workgroup: a partial chunk, a full one, a full
one and a spare, many).  Positions: p in {0, 1, 63, 64, 65, Lpre} with t - p in {0, 1, 7, 8, 9, 63, 64, Lown - 1}, both
sides of every share boundary of the key ranges, and p inside a range (mid-iteration and on a multiple of 8); the two prompts of
a call hold different (p, t), p = 0 next to p = Lpre.  Everything the call must not read is poisoned, everything it must not
write is compared bit for bit."""
import pytest
import torch

import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import decode_ref as D

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
NAN16 = 0x7FC0
C_ATTN = 16.0
SEEN = {"c": 0.0}
BP, DM, H = 2, 128, 2

# name: (Lpre, Lown, M - (Lpre + Lown), key splits)
CONFIGS = {
    "one": (200, 100, 16, 1),
    "two": (1000, 500, 16, 2),                      # Lpre + Lown not a multiple of 64
    "four": (1600, 448, 0, 4),
    "eight": (4000, 200, 16, 8),
    "sixteen": (8000, 300, 0, 16),
}


def sample_counts():
    nq = KC.ops().SHARED_NQ
    return sorted({1, 2, 3, nq, nq + 1, 16})


def fit(t, p, Lpre, Lown):
    """p moved into the contract for this t: max(0, t - Lown + 1) <= p <= min(t, Lpre)"""
    return max(max(0, t - Lown + 1), min(p, t, Lpre))


def position_pairs(Lpre, Lown, n):
    """(p, t) pairs: the cross product of the two sets of the module docstring, both sides of every share boundary of
    dec_key_range (t + 1 a multiple of 64 n) for k = 1, 2 and the largest k, and p inside a key range"""
    ps = [0, 1, 63, 64, 65, Lpre]
    qs = [0, 1, 7, 8, 9, 63, 64, Lown - 1]
    pairs = {(p, p + q) for p in ps for q in qs if p <= Lpre and q < Lown}
    L = Lpre + Lown
    kmax = (L - 1) // (64 * n)
    for k in {1, 2, kmax}:
        for i, t in enumerate((64 * n * k - 1, 64 * n * k, 64 * n * k + 1)):
            if 0 <= t < L:
                pairs.add((fit(t, t - (1, 9, 64)[i], Lpre, Lown), t))
    half = Lown // 2
    pairs.add((Lpre - 3, Lpre - 3 + half))            # p inside a range and inside a wave's 8 keys
    pairs.add((Lpre // 8 * 8 - 8, Lpre // 8 * 8 - 8 + half))
    pairs.add((Lpre, Lpre))                           # p = t = Lpre: the own cache holds the new key only
    if len(pairs) % 2:
        pairs.add((63, 65))                           # an even count: the calls take them two by two
    for p, t in pairs:
        assert 0 <= p <= min(t, Lpre) and t - p < Lown
    return sorted(pairs)


def calls(pairs):
    """the pairs two by two, first against last: one call holds p = 0 next to p = Lpre"""
    assert len(pairs) % 2 == 0
    return [(pairs[i], pairs[-1 - i]) for i in range(len(pairs) // 2)]


class SharedData:
    """both caches, q/k/v of the step and E for one configuration and N, on the device and (the same values) on the CPU"""

    def __init__(self, cfg, N, kind="gauss", seed=0):
        self.Lpre, self.Lown, extra, self.nsplit = cfg
        self.N, self.R, self.kind = N, BP * N, kind
        self.M = self.Lpre + self.Lown + extra
        Lpre, Lown, R, d = self.Lpre, self.Lown, self.R, DM
        g = torch.Generator(device=DEV).manual_seed(1000 * seed + Lpre + 31 * N)
        rn = lambda *s: torch.randn(*s, device=DEV, generator=g)                                    # noqa: E731
        Kp = rn(BP, H, Lpre, 64) * torch.exp(0.5 * rn(BP, H, Lpre, 1))               # rows of different magnitude
        Vp = rn(BP, H, Lpre, 64) * torch.exp(0.5 * rn(BP, H, Lpre, 1))
        Ko = rn(R, H, Lown, 64) * torch.exp(0.5 * rn(R, H, Lown, 1))
        Vo = rn(R, H, Lown, 64) * torch.exp(0.5 * rn(R, H, Lown, 1))
        qkv = rn(R, 3 * d)
        if kind.startswith("dom"):
            # the N queries of a prompt point one way (a prompt key can only dominate all of them then), at different lengths
            u = rn(BP, 1, H, 64).expand(BP, N, H, 64)
            c = 1.0 + 0.25 * torch.rand(BP, N, H, 1, device=DEV, generator=g)
            qkv[:, :d] = (c * u + 0.1 * rn(BP, N, H, 64)).reshape(R, d)
            u_b = u[:, 0]                                                           # [BP, H, 64]
            beta = 8.0 / (u_b * u_b).sum(-1, keepdim=True)                          # (x beta u).q_r / 8 = x c_r, about
        q = qkv[:, :d].reshape(R, H, 64)
        alpha = 8.0 * 90.0 / (q * q).sum(-1, keepdim=True)                          # (alpha q).q / 8 = 90
        if kind == "q0":
            qkv[:, :d] = 0
        elif kind == "dom-t":                                                       # the new key dominates
            qkv[:, d:2 * d] = (alpha * q).reshape(R, d)
        elif kind == "dom-pre":                                                     # a prompt key dominates every sample
            Kp[:, :, 0] = 100.0 * beta * u_b                                        # 100 .. 125 for the N samples
        elif kind == "dom-own":                                                     # a key of the row's own cache
            Ko[:, :, 0] = alpha * q
        elif kind == "dom-last":                                                    # the last split holds the winner (an own
            Ko[:, :, Lown - 2] = (100.0 / 90.0) * alpha * q                         # row), split 0 the runner-up (a prompt row:
            Kp[:, :, 0] = 48.0 * beta * u_b                                         # 48 .. 60 for the N samples)
        elif kind == "neg200":                                                      # every logit near -200
            qkv[:, :d] = 4.0
            qkv[:, d:2 * d] = -6.25 + 0.05 * rn(R, d)
            Kp = -6.25 + 0.05 * rn(BP, H, Lpre, 64)
            Ko = -6.25 + 0.05 * rn(R, H, Lown, 64)
        self.qkv, self.E = qkv.to(BF), (0.3 * rn(self.M, 64)).to(BF)
        self.kpre, self.vpre, self.kown, self.vown = Kp.to(BF), Vp.to(BF), Ko.to(BF), Vo.to(BF)
        self.cpu = [t.cpu() for t in (self.kpre, self.vpre, self.kown, self.vown)]
        self.qkv_cpu, self.E_cpu = self.qkv.cpu(), self.E.cpu()
        ops = KC.ops()
        got = ops.rel_attn_decode_shared_splits(BP, N, Lpre, Lown, d)
        assert got == self.nsplit, (cfg, N, got)
        self.ws = ops.rel_attn_decode_shared_workspace(BP, N, Lpre, Lown, d, DEV)
        assert (self.ws is None) == (self.nsplit == 1)
        assert self.ws is None or self.ws.numel() == R * H * self.nsplit * 68 * 4

    def rows64(self, r, p, t):
        """K, V of row r as the step sees them: fp64 [h, t+1, 64] -- p prompt rows, t - p own rows, the new row"""
        b, d = r // self.N, DM
        out = []
        for pre, own, col in ((self.cpu[0], self.cpu[2], 1), (self.cpu[1], self.cpu[3], 2)):
            new = self.qkv_cpu[r, col * d:(col + 1) * d].reshape(H, 1, 64)
            out.append(torch.cat([pre[b, :, :p], own[r, :, :t - p], new], 1).double())
        return out

    def run(self, pts):
        """one call with every poison in place; ``pts``: (p, t) per prompt.  Returns ctx on the CPU after checking what the call
        wrote and what it left alone"""
        ops = KC.ops()
        N, R, Lpre, Lown, d = self.N, self.R, self.Lpre, self.Lown, DM
        p_b = torch.tensor([p for p, _ in pts], device=DEV)
        t_b = torch.tensor([t for _, t in pts], device=DEV)
        q_r = (t_b - p_b).repeat_interleave(N)                                                  # the own row every row appends
        kpre, vpre = (c.view(torch.int16).masked_fill((torch.arange(Lpre, device=DEV)[None] >= p_b[:, None])[:, None, :, None],
                                                      NAN16).view(BF) for c in (self.kpre, self.vpre))
        stale = (torch.arange(Lown, device=DEV)[None] >= q_r[:, None])[:, None, :, None]        # [R, 1, Lown, 1]
        kown, vown = (c.view(torch.int16).masked_fill(stale, NAN16).view(BF) for c in (self.kown, self.vown))
        kpre0, vpre0 = kpre.clone(), vpre.clone()
        want_k, want_v = kown.clone(), vown.clone()
        ridx = torch.arange(R, device=DEV)
        want_k[ridx, :, q_r] = self.qkv[:, d:2 * d].reshape(R, H, 64)
        want_v[ridx, :, q_r] = self.qkv[:, 2 * d:].reshape(R, H, 64)
        E = self.E.clone()
        E.view(torch.int16)[:self.M - 1 - int(t_b.max())] = NAN16                               # rows no key of this call maps to
        if self.ws is not None:
            self.ws.fill_(0xFF)                                                                 # every stale partial is NaN
        ctx = torch.full((R, d), float("nan"), dtype=BF, device=DEV)
        pos = t_b.repeat_interleave(N).to(torch.int32).contiguous()
        ops.rel_attn_decode_shared(self.qkv, kpre, vpre, kown, vown, E, pos, p_b.to(torch.int32), ctx, self.ws, N)
        torch.cuda.synchronize()
        what = (self.kind, "N", N, pts)
        i16 = lambda x: x.view(torch.int16)                                                                 # noqa: E731
        assert torch.equal(i16(kpre), i16(kpre0)) and torch.equal(i16(vpre), i16(vpre0)), what  # the prompt cache: never written
        assert torch.equal(i16(kown), i16(want_k)) and torch.equal(i16(vown), i16(want_v)), what
        return ctx.float().cpu()

    def check(self, pts):
        ctx = self.run(pts).double().reshape(self.R, H, 64)
        what = (self.kind, "N", self.N, "Lpre, Lown", self.Lpre, self.Lown)
        assert torch.isfinite(ctx).all(), (what, pts)
        q = self.qkv_cpu[:, :DM].reshape(self.R, H, 64)
        for r in range(self.R):
            p, t = pts[r // self.N]
            K, V = self.rows64(r, p, t)
            ref = D.rel_attn_decode(q[r], K, V, self.E_cpu, t)
            F = D.attn_noise_floor(q[r], K, V, self.E_cpu, t, ref)[:, None]
            err = (ctx[r] - ref).abs()
            over = (err - 2.0 ** -8 * ref.abs()).clamp(min=0)
            if (F > 0).any():
                SEEN["c"] = max(SEEN["c"], float((over / F)[(F > 0).expand_as(over)].max()))
            bad = err > 2.0 ** -8 * ref.abs() + C_ATTN * F
            assert not bad.any(), (what, "row", r, "p, t", (p, t), "head, dim", bad.nonzero()[:4].tolist(), "err",
                                   err[bad][:4].tolist(), "ref", ref[bad][:4].tolist(), "F", F.flatten().tolist())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_shared_attention_at_every_split_count_position_and_sample_count(name):
    """Gaussian data; the sample counts take the calls in turn, so each meets each configuration several times"""
    cfg = CONFIGS[name]
    Lpre, Lown, _, n = cfg
    pairs = position_pairs(Lpre, Lown, n)
    assert {(0, 0), (Lpre, Lpre), (Lpre, Lpre + Lown - 1), (0, Lown - 1), (64, 64 + 63)} <= set(pairs)
    assert any(t + 1 == 64 * n for _, t in pairs) and any(0 < p < Lpre and p % 8 for p, _ in pairs)
    ns = sample_counts()
    data = {N: SharedData(cfg, N) for N in ns}
    todo = calls(pairs)
    assert todo[0][0][0] == 0 and todo[0][1][0] == Lpre and len(todo) >= 2 * len(ns)
    for i, pts in enumerate(todo):
        assert pts[0] != pts[1]
        data[ns[i % len(ns)]].check(pts)
    print(f"\n{name}: {len(pairs)} (p, t) pairs in {len(todo)} calls, largest (err - 2^-8|ref|) / F so far {SEEN['c']:.3f}")


@pytest.mark.parametrize("kind", ["q0", "dom-pre", "dom-own", "dom-t", "dom-last", "neg200"])
@pytest.mark.parametrize("name", ["one", "two", "eight", "sixteen"])
def test_shared_attention_value_cases(name, kind):
    """q = 0 (the plain mean of v_0..v_t); one key 60 or more above all others in the prompt part, in the own part, at j = t,
    and in the last split with the runner-up in split 0; every logit near -200"""
    cfg = CONFIGS[name]
    Lpre, Lown, _, n = cfg
    nq = KC.ops().SHARED_NQ
    full = (Lpre, Lpre + Lown - 1)
    todo = [(3, (full, (1, Lown))), (nq + 1, ((65, 74), full)), (16, ((0, Lown - 1), (Lpre, Lpre + 1)))]
    for N, pts in todo:
        data = SharedData(cfg, N, kind, seed=1)
        if pts[0] == full:                             # the case is what it claims to be, from the reference's own logits
            q = data.qkv_cpu[:, :DM].reshape(data.R, H, 64).double()
            p, t = full
            for r in range(N):
                K, V = data.rows64(r, p, t)
                s = (torch.einsum("hjd,hd->hj", K, q[r]) + torch.einsum("jd,hd->hj", data.E_cpu.double()[data.M - 1 - t:], q[r])) / 8
                top = s.topk(3, -1)
                if kind == "q0":
                    assert (s == 0).all() and (D.rel_attn_decode(q[r], K, V, data.E_cpu, t) - V.mean(1)).abs().max() <= 1e-12
                elif kind == "neg200":
                    assert s.max() < -150 and s.min() > -250
                else:
                    want = {"dom-t": t, "dom-pre": 0, "dom-own": p, "dom-last": t - 1}[kind]
                    assert (top.indices[:, 0] == want).all() and (top.values[:, 0] - top.values[:, 2] >= 60).all(), (r, top)
                    if kind == "dom-last":             # the runner-up sits in split 0, well above the rest
                        assert (top.indices[:, 1] == 0).all() and (top.values[:, 0] - top.values[:, 1] >= 30).all()
                        assert (top.values[:, 1] - top.values[:, 2] >= 20).all()
                    else:
                        assert (top.values[:, 0] - top.values[:, 1] >= 60).all()
        data.check(pts)
    print(f"\n{name} {kind}: largest (err - 2^-8|ref|) / F so far {SEEN['c']:.3f}")


def test_a_single_key_returns_its_value_for_every_sample_count():
    """p = t = 0: the softmax has one term, ctx is v_0 exactly"""
    for N in sample_counts():
        data = SharedData(CONFIGS["one"], N, seed=2)
        ctx = data.run([(0, 0), (0, 0)])
        assert torch.equal(ctx, data.qkv_cpu[:, 2 * DM:].float()), N


def test_positions_outside_the_contract_touch_nothing():
    """the positions cannot be checked on the host: a prompt whose (t, p) break the contract leaves both caches as they were
    (its ctx rows are unspecified), and the prompt beside it is computed as always"""
    ops = KC.ops()
    N = 3
    data = SharedData(CONFIGS["two"], N, seed=3)
    Lpre, Lown, M, d = data.Lpre, data.Lown, data.M, DM
    good = (65, 74)
    for p, t in ((Lpre + 1, Lpre + 5), (10, 10 + Lown), (12, 11), (-1, 5), (Lpre, M), (3, -2)):
        kpre, vpre, kown, vown = (c.clone() for c in (data.kpre, data.vpre, data.kown, data.vown))
        ctx = torch.zeros(data.R, d, dtype=BF, device=DEV)
        pos = torch.tensor([t] * N + [good[1]] * N, dtype=torch.int32, device=DEV)
        pre = torch.tensor([p, good[0]], dtype=torch.int32, device=DEV)
        ops.rel_attn_decode_shared(data.qkv, kpre, vpre, kown, vown, data.E, pos, pre, ctx, data.ws, N)
        torch.cuda.synchronize()
        assert torch.equal(kpre, data.kpre) and torch.equal(vpre, data.vpre), (p, t)
        assert torch.equal(kown[:N], data.kown[:N]) and torch.equal(vown[:N], data.vown[:N]), (p, t)
        assert not torch.equal(kown[N:], data.kown[N:]) and torch.isfinite(ctx[N:].float()).all(), (p, t)


def test_shared_call_beside_the_ragged_call_on_repeated_caches():
    """information, not an assertion beyond the bound both meet: mgx_rel_attn_decode with per-row positions on R rows whose caches are the
    prompt rows followed by the own rows (the repeated call's layout) computes the same logical attention; whether the two
    agree bitwise is printed (their split counts differ where decode_splits and the shared policy do)"""
    ops = KC.ops()
    for name, N, pts in (("one", 3, ((65, 74), (200, 263))), ("two", ops.SHARED_NQ + 1, ((1000, 1499), (0, 63))),
                         ("eight", 16, ((4000, 4199), (63, 70)))):
        data = SharedData(CONFIGS[name], N, seed=4)
        ctx = data.run(list(pts))
        Lmax, R = data.Lpre + data.Lown, data.R
        kc, vc = (torch.zeros(R, H, Lmax, 64, dtype=BF, device=DEV) for _ in range(2))
        for r in range(R):
            p, t = pts[r // N]
            for c, pre, own in ((kc, data.kpre, data.kown), (vc, data.vpre, data.vown)):
                c[r, :, :p] = pre[r // N, :, :p]
                c[r, :, p:t] = own[r, :, :t - p]
        pos = torch.tensor([pts[r // N][1] for r in range(R)], dtype=torch.int32, device=DEV)
        rep = ops.rel_attn_decode(data.qkv, kc, vc, data.E, pos, torch.empty(R, DM, dtype=BF, device=DEV),
                                  ops.rel_attn_decode_workspace(R, Lmax, DM, DEV), ragged=True).float().cpu()
        same = torch.equal(rep, ctx)
        print(f"\n{name} N={N}: shared splits {data.nsplit}, repeated splits {ops.rel_attn_decode_splits(R, Lmax, DM)}: "
              f"bitwise equal {same}, largest difference {(rep - ctx).abs().max().item():.3e}")
        assert (rep - ctx).abs().max().item() <= 2.0 ** -6 * ctx.abs().max().item()     # two roundings of one value, loosely


def test_shape_violations_are_refused_with_a_message():
    ops = KC.ops()
    from musicgeneration_amd._lib import MgxError
    data = SharedData(CONFIGS["one"], 2, seed=5)
    pos = torch.zeros(data.R, dtype=torch.int32, device=DEV)
    pre = torch.zeros(BP, dtype=torch.int32, device=DEV)
    ctx = torch.empty(data.R, DM, dtype=BF, device=DEV)
    args = (data.qkv, data.kpre, data.vpre, data.kown, data.vown, data.E, pos, pre, ctx, None)
    for N in (0, 17):
        with pytest.raises(ValueError, match="1 .. 16"):
            ops.rel_attn_decode_shared(*args, N)
    with pytest.raises(ValueError, match="Bp \\* N"):
        ops.rel_attn_decode_shared(*args, 3)
    with pytest.raises(ValueError, match="pre_rows"):
        ops.rel_attn_decode_shared(*args[:7], pre[:1], ctx, None, 2)
    big = SharedData(CONFIGS["two"], 2, seed=5)
    with pytest.raises(MgxError, match="workspace"):
        ops.rel_attn_decode_shared(big.qkv, big.kpre, big.vpre, big.kown, big.vown, big.E, pos, pre, ctx, None, 2)
    torch.cuda.synchronize()

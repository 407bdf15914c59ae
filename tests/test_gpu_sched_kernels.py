"""The three kernels of scheduled sampling for Event_Melody_RNN (mgx.h, ABI 23) against references written from their header
contracts: fp64 projections (oracle/train_ref.py), the integer twin of the sampler's uniform (oracle/decode_ref.py).

  mgx_gru_step_x_fwd_save  h_next / y bit-equal to mgx_gru_step_x_fwd; gi_out / gh_out within the bound the fused steps' projections
                           have in tests/test_gpu_gru_kernels.py: |got - ref| <= 2^-8 |ref| + C_STEP F, C_STEP = 0.25, F = proj_floor
  mgx_dropout_bf16_at      slices that tile a buffer are bit-equal to one mgx_dropout_bf16 call over it
  mgx_gru_next_event       forced rows = events; greedy rows = the smallest id at the maximum, exactly; drawn rows = the id of the
                           fp64 CDF, a row excused only when u * mass lies within V * 2^-22 * mass of a CDF boundary (the fp32
                           summation bound in any order, doubled), at most 1 % of the rows
Every output buffer is longer than the kernel may write and holds a sentinel there."""
import numpy as np
import pytest
import torch

import kernel_checks as KC
from kernel_checks import bits16, gen, nothing_more_after_a_gpu_error, weights  # noqa: F401 (the fixture is used by name)
from oracle import decode_ref as D
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
F64 = torch.float64
C_STEP = 0.25


# =====================================================================================================================
# 1. the step that saves its projections
# =====================================================================================================================
@pytest.mark.parametrize("B,H,Kx", [(1, 64, 64), (33, 64, 128), (5, 320, 64), (33, 704, 576)])     # the last: the K > 512 tail loop
def test_save_step_is_the_sampling_step_plus_its_two_projections(B, H, Kx):
    ops = KC.ops()
    wih, bih = weights(3 * H, Kx, 2)
    whh, bhh = weights(3 * H, H, 3)
    g = gen(B, H, Kx)
    h_prev = torch.randn(B, H, generator=g)
    x = torch.randn(B, Kx, generator=g).to(BF)
    hp_bf = h_prev.to(BF)
    args = (x.to(DEV), ops.pack_frag(wih.to(DEV)), bih.to(DEV), hp_bf.to(DEV), h_prev.to(DEV), ops.pack_frag(whh.to(DEV)), bhh.to(DEV))
    h_ref, y_ref = torch.empty(B, H, device=DEV), torch.empty(B, H, dtype=BF, device=DEV)
    ops.gru_step_x_fwd(*args, h_ref, y_ref)
    PAD = 3                                                  # sentinel rows after the B real ones
    h_next = torch.full((B + PAD, H), -7.0, device=DEV)
    y = torch.full((B + PAD, H), -7.0, dtype=BF, device=DEV)
    gi_out = torch.full((B + PAD, 3 * H), -7.0, dtype=BF, device=DEV)
    gh_out = torch.full((B + PAD, 3 * H), -7.0, dtype=BF, device=DEV)
    ops.gru_step_x_fwd_save(*args, h_next[:B], y[:B], gi_out[:B], gh_out[:B])
    torch.cuda.synchronize()
    assert h_next[:B].cpu().view(torch.int32).equal(h_ref.cpu().view(torch.int32)), "h_next differs from mgx_gru_step_x_fwd"
    assert bits16(y[:B]).equal(bits16(y_ref)), "y differs from mgx_gru_step_x_fwd"
    for name, buf in (("h_next", h_next), ("y", y), ("gi_out", gi_out), ("gh_out", gh_out)):
        assert (buf[B:].float().cpu() == -7.0).all(), f"{name}: a row >= B was written"
    for name, got, (a, w, b) in (("gi_out", gi_out, (x, wih, bih)), ("gh_out", gh_out, (hp_bf, whh, bhh))):
        ref, S = T.proj(a, w, b)
        F = T.proj_floor(a, w, b, ref, S)
        got = got[:B].cpu().to(F64)
        assert torch.isfinite(got).all()
        ratio = ((got - ref).abs() - 2.0 ** -8 * ref.abs()) / F
        print(f"[save step] B={B} H={H} Kx={Kx} {name}: ratio {ratio.max().item():.3f}")
        assert ratio.max().item() <= C_STEP, f"{name}: ratio {ratio.max().item():.3f} > {C_STEP}"


# =====================================================================================================================
# 2. dropout on slices
# =====================================================================================================================
@pytest.mark.parametrize("p_drop", (0.0, 0.1))
def test_dropout_slices_tile_the_whole_buffer_call_bit_for_bit(p_drop):
    lib, chk, ptr, stream_ptr = KC.raw()
    ops = KC.ops()
    n = 8 * (2 ** 16 + 5)
    seed = (1 << 40) + 12345
    x = torch.randn(n, generator=gen(n)).to(BF).to(DEV)
    whole = torch.full((n + 8,), 1.0, dtype=BF, device=DEV)
    chk(lib.mgx_dropout_bf16(ptr(x), ptr(whole), n, float(p_drop), seed, stream_ptr()), "mgx_dropout_bf16")
    seed_dev = torch.tensor([seed], dtype=torch.int64, device=DEV)
    out = torch.full((n + 8,), 1.0, dtype=BF, device=DEV)
    cuts = [0, 8, 8 * 1000, 8 * 1257, 8 * 40000, 8 * (2 ** 16 - 1), n]            # unequal multiples of 8; the last slice is 6 groups
    for a, b in zip(cuts, cuts[1:]):
        ops.dropout_bf16_at(x[a:b], out[a:b], a, p_drop, seed_dev)
    torch.cuda.synchronize()
    assert bits16(out).equal(bits16(whole))
    assert (out[n:].float().cpu() == 1.0).all()
    if p_drop > 0:
        assert (whole[:n].float() == 0).any().item() and not bits16(whole[:n]).equal(bits16(x))
        # the seed is read when the kernel runs: another seed in the same device word gives another mask
        seed_dev.fill_(seed + 1)
        other = torch.empty(8 * 1000, dtype=BF, device=DEV)
        ops.dropout_bf16_at(x[:8 * 1000], other, 0, p_drop, seed_dev)
        assert not bits16(other).equal(bits16(whole[:8 * 1000]))
    else:
        assert bits16(whole[:n]).equal(bits16(x))


# =====================================================================================================================
# 3. the next event
# =====================================================================================================================
HUGE = 3.0e38                                                # columns >= V hold this: reading one wins every maximum


def next_event(logits, V, flag, events, temperature, seed, step, emb):
    """-> tok, used_out int32 [B], x_out [B,Ep] (cpu), after checking the sentinels past every output"""
    ops = KC.ops()
    B, Ep = logits.shape[0], emb.shape[1]
    PAD = 5
    tok = torch.full((B + PAD,), -9, dtype=torch.int32, device=DEV)
    used = torch.full((B + PAD,), -9, dtype=torch.int32, device=DEV)
    x_out = torch.full((B + 1, Ep), -7.0, dtype=BF, device=DEV)
    ops.gru_next_event(logits.to(DEV), V, torch.tensor([flag], dtype=torch.int32, device=DEV),
                       None if events is None else events.to(torch.int32).to(DEV), temperature,
                       torch.tensor([seed], dtype=torch.int64, device=DEV), step, emb.to(DEV), tok[:B], used[:B], x_out[:B])
    torch.cuda.synchronize()
    assert (tok[B:].cpu() == -9).all() and (used[B:].cpu() == -9).all() and (x_out[B:].float().cpu() == -7.0).all()
    tok, used, x_out = tok[:B].cpu(), used[:B].cpu(), x_out[:B].cpu()
    assert tok.equal(used), "used_out != tok"
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    assert bits16(x_out).equal(bits16(emb[tok.long()])), "x_out is not emb[tok] bit for bit"
    return tok


def make_logits(B, V, scale=3.0, seed=0):
    ld = (V + 8) // 8 * 8 + 8                                # ld > V
    g = gen(B, V, seed)
    lg = torch.full((B, ld), HUGE)
    lg[:, :V] = scale * torch.randn(B, V, generator=g)
    return lg.to(BF)


def make_emb(V, seed=1):
    Ep = (V + 63) // 64 * 64
    return torch.randn(V, Ep, generator=gen(V, seed)).to(BF)


def greedy_ref(lg, V):
    """the smallest id at the maximum of the non-NaN logits; 0 for a row without a finite logit"""
    v = lg[:, :V].float().numpy().astype(np.float64)
    out = np.zeros(v.shape[0], dtype=np.int64)
    for b in range(v.shape[0]):
        ok = ~np.isnan(v[b])
        if not np.isfinite(v[b]).any():
            continue
        out[b] = int(np.nonzero(ok & (v[b] == v[b][ok].max()))[0][0])
    return out


@pytest.mark.parametrize("B", (1, 4096))
@pytest.mark.parametrize("V", (5, 52, 337, 1024))
def test_next_event_forced_and_greedy_rows(V, B):
    lg = make_logits(B, V)
    emb = make_emb(V)
    g = gen(V, B, 9)
    nat_ties = (lg[:, :V].float() == lg[:, :V].float().max(-1, keepdim=True).values).sum(-1) > 1
    rows = torch.arange(B)
    # planted exact ties at the maximum, at two or three ids of every fourth row
    tie_rows = rows[rows % 4 == 0]
    for b in tie_rows.tolist():
        ids = torch.randperm(V, generator=g)[: min(3, V - 1)]
        lg[b, ids] = lg[b, :V].float().max().item() + 1.0
    if B > 8:
        nan, inf = float("nan"), float("inf")
        lg[1, :V] = -inf                                     # no finite logit: id 0
        lg[2, :V] = nan                                      # nothing but NaN: id 0
        lg[3, :V] = -inf
        lg[3, V - 1] = -2.0                                  # one finite logit among -inf
        lg[5, 0] = nan                                       # a NaN never wins, wherever it stands
        lg[5, V // 2] = nan
        lg[6, :V] = nan
        lg[6, V - 2] = -inf
        lg[6, V - 1] = -5.0                                  # NaN, -inf and one finite value: the finite one
        lg[7, :V] = -inf
        lg[7, 1] = nan                                       # -inf and NaN only: id 0
    events = torch.randint(0, V, (B,), generator=g)
    if B > 8:
        events[9], events[10] = -4, V + 3                    # clamped to 0 .. V-1
    want_forced = events.clamp(0, V - 1)
    for flag in (1, 3):                                      # forced wins over greedy
        assert next_event(lg, V, flag, events, 1.0, 11, 2, emb).long().equal(want_forced), f"flag {flag}"
    want = greedy_ref(lg, V)
    got = next_event(lg, V, 2, events, 1.0, 11, 2, emb).long().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"greedy rows {bad[:8].tolist()}: got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"
    assert (next_event(lg, V, 2, None, 1.0, 11, 2, emb).long().numpy() == want).all()     # events = NULL
    assert (next_event(lg, V, 3, None, 1.0, 11, 2, emb).long().numpy() == want).all()     # ... no step is forced
    print(f"V={V} B={B}: {100 * nat_ties.float().mean().item():.1f} % of the random rows tie at the maximum, "
          f"{tie_rows.numel()} planted")
    if B > 8:
        assert got[1] == 0 and got[2] == 0 and got[3] == V - 1 and got[6] == V - 1 and got[7] == 0


def cdf_ref(lg, V, temperature, seed, step):
    """fp64: expected id per row, and whether u * mass lies within V * 2^-22 * mass of a CDF boundary"""
    x = lg[:, :V].float().numpy().astype(np.float64) * (1.0 / temperature)
    p = np.exp(x - x.max(-1, keepdims=True))
    cdf = np.cumsum(p, -1)
    mass = cdf[:, -1]
    u = D.u01(seed, step, np.arange(lg.shape[0]))
    target = u * mass
    want = np.array([D.draw(p[b], u[b]) for b in range(lg.shape[0])])
    near = np.abs(cdf - target[:, None]).min(-1) <= V * 2.0 ** -22 * mass
    return want, near, p / mass[:, None]


@pytest.mark.parametrize("temperature", (1.0, 0.5))
@pytest.mark.parametrize("V", (5, 52))
def test_next_event_categorical_draw_against_the_fp64_cdf(V, temperature):
    B, seed, step = 4096, (5 << 33) + 77, 11
    lg = make_logits(B, V, seed=3)
    emb = make_emb(V)
    want, near, _ = cdf_ref(lg, V, temperature, seed, step)
    for flag, events in ((0, torch.zeros(B, dtype=torch.int64)), (1, None)):       # not forced; "forced" without events
        got = next_event(lg, V, flag, events, temperature, seed, step, emb).long().numpy()
        print(f"V={V} T={temperature}: {100 * near.mean():.2f} % of {B} rows excused, {(got != want).sum()} rows differ")
        assert near.mean() <= 0.01
        bad = np.nonzero((got != want) & ~near)[0]
        assert bad.size == 0, f"rows {bad[:8].tolist()}: got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"
    # the draw is a function of (seed, step, row)
    again = next_event(lg, V, 0, None, temperature, seed, step, emb)
    assert again.long().numpy().tolist() == got.tolist()
    assert (next_event(lg, V, 0, None, temperature, seed, step + 1, emb).long().numpy() != got).any()
    assert (next_event(lg, V, 0, None, temperature, seed + 1, step, emb).long().numpy() != got).any()


def test_next_event_frequencies_follow_the_softmax():
    """V = 5, one distribution in all 4096 rows: every id's count within 5 binomial standard deviations"""
    V, B, seed, step = 5, 4096, 99, 3
    lg = make_logits(1, V, scale=1.5, seed=4).repeat(B, 1)
    _, _, prob = cdf_ref(lg, V, 1.0, seed, step)
    got = next_event(lg, V, 0, None, 1.0, seed, step, make_emb(V)).long().numpy()
    for v in range(V):
        pv = prob[0, v]
        n, sd = (got == v).sum(), np.sqrt(B * pv * (1 - pv))
        print(f"id {v}: p {pv:.4f} count {n} expected {B * pv:.1f} sd {sd:.1f}")
        assert abs(n - B * pv) <= 5 * sd

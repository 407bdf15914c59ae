"""Every entry point of csrc/gru_train.hip (GRU cell forward / backward, the fused time steps, the bf16 dropout, the row scatter)
against the fp64 reference of its header contract (oracle/train_ref.py), element by element.  Until now the fused steps were
compared only with the two-kernel path and the cell kernels with nothing: a shared misreading of the cell formula passed.

No bound here is a max-norm bound and none was calibrated against another kernel.
  bf16 output   |got - ref| <= 2^-8 |ref| + C * F      2^-8 |ref| is the output's rounding (half an ulp is 2^-9)
  fp32 output   |got - ref| <= C * F
  the dropout's output and every one-hot projection: exact
F is the family's noise floor (train_ref: the same formula in fp32, its sums reversed, against fp64, plus one fp32 ulp).

The fused steps are checked in stages, so that a flipped bf16 rounding upstream needs no slack downstream:
  forward    gh_out against the fp64 product + bias; h_next and y against the fp64 cell evaluated on the kernel's OWN gh_out
  backward   every output is dh times a coefficient and dh = dh_direct + bf16(d_rec) + dy, so the bound is
             (2^-8 |d_rec| + C_STEP F_drec) |coef| + the output's own rounding + C_CELL F_cell, with d_rec taken in fp64
  final      dh_out against dh_direct + d_rec within 2^-8 |d_rec| + C_STEP F
  x_fwd      gi and gh are not outputs: with one-hot rows of x and h they are known exactly (a weight column plus bias) and
             h_next gets the cell bound alone; on random data an output whose six pre-activations all lie further than
             C_STEP F from a bf16 rounding boundary gets the cell bound on the rounded fp64 projections, the others (at
             most 2 %) twice the first-order effect of one bf16 ulp of each doubtful pre-activation
With one-hot rows in h_prev (or x, or dgh_next) a projection's result is the weight's column plus bias EXACTLY: that checks
pack_frag's fragment order for every k-step of every chunk.

The constants absorb the summation order and the fast exp / tanh, nothing else.  Each is MEASURED on one MI355X as the largest
(|err| - rounding term) / F over all cases of this module and set to twice that, rounded up to a power of two
(profiles/r11_rowwise_gru_kernel_tests.txt has the figures and the cases):
  C_CELL  the cell, forward and backward      4    measured 1.107 (h_next of the fused forward step, H 128, B 33)
  C_STEP  the projections of the fused steps  0.25 measured 0.111 (gh_out, H 704, B 100; the floor holds the classical 2^-24 sum |a w|)
  C_SCAT  the row scatter (fp32 atomics)      2    measured 0.594 (n 5000, cols 64, V 300; 0.507 .. 0.594 over three runs)
Every test prints its largest ratio before it asserts (pytest -s shows them).
"""
import pytest
import torch

import kernel_checks as KC
from kernel_checks import bits16, gen, nothing_more_after_a_gpu_error, weights  # noqa: F401 (the fixture is used by name)
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
F64 = torch.float64
C = {"CELL": 4.0, "STEP": 0.25, "SCAT": 2.0}
SEEN = {}
_report = KC.report_fixture(SEEN, "largest ratio {:.3f}")


def check(fam, got, ref, F, case, rounding, extra=None):
    KC.check_floor(fam, got, ref, F, case, C=C[fam], seen=SEEN, rounding=rounding, extra=extra)


# =====================================================================================================================
# 1. the cell kernels on given bf16 gi / gh
# =====================================================================================================================
CELL_SHAPES = ((1, 7), (3, 100), (33, 129), (100, 512))                    # B * H not a multiple of 256 (but the last)


def cell_inputs(B, H, scale=2.0):
    g = gen(B, H)
    return ((scale * torch.randn(B, 3 * H, generator=g)).to(BF), (scale * torch.randn(B, 3 * H, generator=g)).to(BF),
            torch.randn(B, H, generator=g))


def check_cell_fwd(gi, gh, h_prev, h_next, y, case):
    ref = T.gru_cell_fwd(gi, gh, h_prev)
    check("CELL", h_next, ref, T.gru_cell_fwd_floor(gi, gh, h_prev, ref), case + " h_next", 0.0)
    assert h_next.dtype == torch.float32 and bits16(y).equal(bits16(h_next.to(BF))), case + ": y is not the bf16 rounding of h_next"


def check_cell_bwd(gi, gh, h_prev, dh, dgi, dgh, dhp, case, extra=None):
    """extra: dict coefficient name -> additional slack per element (the fused step's d_rec term)"""
    ref = T.gru_cell_bwd(gi, gh, h_prev, dh)
    F = T.gru_cell_bwd_floor(gi, gh, h_prev, dh, ref)
    ex = (lambda *names: None) if extra is None else (lambda *names: torch.cat([extra[n] for n in names], 1))
    check("CELL", dgi, ref[0], F, case + " dgi", 2.0 ** -8, ex("r", "z", "n"))
    check("CELL", dgh, ref[1], F, case + " dgh", 2.0 ** -8, ex("r", "z", "nr"))
    assert dhp.dtype == torch.float32
    check("CELL", dhp, ref[2], F, case + " dh_out", 0.0, ex("h"))


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_forward_against_fp64(B, H):
    ops = KC.ops()
    gi, gh, h_prev = cell_inputs(B, H)
    h_next, y = torch.empty(B, H, device=DEV), torch.empty(B, H, dtype=BF, device=DEV)
    ops.gru_cell_fwd(gi.to(DEV), gh.to(DEV), h_prev.to(DEV), h_next, y)
    check_cell_fwd(gi, gh, h_prev, h_next, y, f"cell fwd B={B} H={H}")


@pytest.mark.parametrize("B,H", CELL_SHAPES)
def test_cell_backward_against_fp64_for_every_combination_of_its_optional_inputs(B, H):
    ops = KC.ops()
    gi, gh, h_prev = cell_inputs(B, H)
    g = gen(B, H, 1)
    parts = (torch.randn(B, H, generator=g), torch.randn(B, H, generator=g).to(BF), torch.randn(B, H, generator=g).to(BF))
    for mask in range(8):
        use = [p if mask >> i & 1 else None for i, p in enumerate(parts)]
        dh = sum((p.double() for p in use if p is not None), torch.zeros(B, H, dtype=F64))
        dgi, dgh = (torch.full((B, 3 * H), float("nan"), dtype=BF, device=DEV) for _ in range(2))
        dhp = torch.full((B, H), float("nan"), device=DEV)
        ops.gru_cell_bwd(gi.to(DEV), gh.to(DEV), h_prev.to(DEV), *(None if p is None else p.to(DEV) for p in use), dgi, dgh, dhp)
        check_cell_bwd(gi, gh, h_prev, dh, dgi, dgh, dhp, f"cell bwd B={B} H={H} inputs={mask:03b}")
        if mask == 0:
            assert (bits16(dgi) & 0x7FFF).eq(0).all() and (dhp == 0).all()


@pytest.mark.parametrize("a", (30.0, 100.0))
def test_cell_with_saturated_gates_is_finite_and_exact(a):
    """pre-activations of +-30 and +-100: sigmoid(+a) is exactly 1 in fp32, sigmoid(-100) exactly 0"""
    ops = KC.ops()
    B, H = 4, 36
    g = gen(int(a))
    gi, gh, h_prev = cell_inputs(B, H, 1.0)
    gi, gh = gi.float(), gh.float()
    gh[:, :2 * H] = 0
    sign = torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0)
    gi[0, H:2 * H] = a                    # row 0: z = 1            -> h' = h, no gradient to the gates, dh_prev = dh
    gi[1, H:2 * H] = -a                   # row 1: z = 0 (a = 100)  -> h' = n, dh_prev = 0
    gi[2, :H] = -a                        # row 2: r = 0 (a = 100)  -> n = tanh(gi_n): gh_n has no effect
    gi[3] = (a * sign).repeat(3)          # row 3: everything saturated, both signs
    gh[3, 2 * H:] = a * sign
    gi, gh = gi.to(BF), gh.to(BF)
    h_next, y = torch.empty(B, H, device=DEV), torch.empty(B, H, dtype=BF, device=DEV)
    ops.gru_cell_fwd(gi.to(DEV), gh.to(DEV), h_prev.to(DEV), h_next, y)
    check_cell_fwd(gi, gh, h_prev, h_next, y, f"cell fwd saturated a={a}")
    hn = h_next.cpu()
    assert hn[0].view(torch.int32).equal(h_prev[0].view(torch.int32)), "z = 1: h_next is not h_prev bit for bit"
    assert (hn.abs() <= torch.maximum(h_prev.abs(), torch.ones(())) * (1 + 2.0 ** -22)).all()
    dh = torch.randn(B, H, generator=g)
    dgi, dgh = (torch.full((B, 3 * H), float("nan"), dtype=BF, device=DEV) for _ in range(2))
    dhp = torch.full((B, H), float("nan"), device=DEV)
    ops.gru_cell_bwd(gi.to(DEV), gh.to(DEV), h_prev.to(DEV), dh.to(DEV), None, None, dgi, dgh, dhp)
    check_cell_bwd(gi, gh, h_prev, dh.double(), dgi, dgh, dhp, f"cell bwd saturated a={a}")
    assert dhp.cpu()[0].view(torch.int32).equal(dh[0].view(torch.int32)) and (dgi.cpu()[0].float() == 0).all() and (dgh.cpu()[0].float() == 0).all()
    if a == 100.0:
        assert (dhp.cpu()[1] == 0).all() and (dgi.cpu()[1, H:2 * H].float() == 0).all()
        assert (dgi.cpu()[2, :H].float() == 0).all() and (dgh.cpu()[2, 2 * H:].float() == 0).all()
        gh2 = gh.clone()
        gh2[2, 2 * H:] = 7.0              # r = 0: gh_n is multiplied by an exact zero
        h2, y2 = torch.empty(B, H, device=DEV), torch.empty(B, H, dtype=BF, device=DEV)
        ops.gru_cell_fwd(gi.to(DEV), gh2.to(DEV), h_prev.to(DEV), h2, y2)
        assert h2.cpu()[2].view(torch.int32).equal(hn[2].view(torch.int32))


# =====================================================================================================================
# 2. dropout and scatter
# =====================================================================================================================
@pytest.mark.parametrize("p_drop", (0.0, 0.1, 0.99999))
@pytest.mark.parametrize("n", (8, 8 * 1000, 8 * (2 ** 16 + 5)))
def test_dropout_is_the_integer_twin_bit_for_bit(n, p_drop):
    """n / 8 not a multiple of 256; kept elements are the bf16 rounding of value * scale in fp32, dropped ones 0"""
    lib, chk, ptr, stream_ptr = KC.raw()
    seed = (1 << 40) + 12345
    x = torch.randn(n, generator=gen(n)).to(BF)
    xg, out = x.to(DEV), torch.full((n + 8,), 1.0, dtype=BF, device=DEV)
    chk(lib.mgx_dropout_bf16(ptr(xg), ptr(out), n, float(p_drop), seed, stream_ptr()), "mgx_dropout_bf16")
    mult = T.drop_mult(p_drop, seed, n)
    want = (x.float() * mult).to(BF)
    assert bits16(out[:n]).equal(bits16(want))
    assert (out[n:].cpu().float() == 1.0).all()               # nothing past the end
    if p_drop > 0:
        assert (out[:n].cpu().float()[mult == 0] == 0).all() and (n < 8000 or ((mult == 0).any() and (mult != 0).any()))
        assert KC.ops().dropout_bf16(xg, p_drop, seed).cpu().view(torch.int16).equal(bits16(want))


@pytest.mark.parametrize("n,ld,cols,V", ((7, 16, 12, 11), (1000, 72, 65, 9), (5000, 64, 64, 300)))
def test_scatter_add_rows_against_fp64(n, ld, cols, V):
    """repeated indices, indices outside [0, V) (ignored), ld > cols, dst starting nonzero"""
    ops = KC.ops()
    g = gen(n, V)
    idx = torch.randint(-2, V + 2, (n,), generator=g).to(torch.int32)
    idx[:3] = torch.tensor([3, 3, 3], dtype=torch.int32)
    idx[idx == 5] = 4                                         # row 5 receives nothing
    src = torch.randn(n, ld, generator=g).to(BF)
    init = torch.randn(V, cols, generator=g)
    dst = init.clone().to(DEV)
    ops.scatter_add_rows(idx.to(DEV), src.to(DEV), dst)
    upd, S = T.scatter_add_rows(idx, src, V, cols)
    tot = init.double() + upd
    check("SCAT", dst, tot, T.EPS32 * (S + init.double().abs()) + T.ulp32(torch.maximum(init.double().abs(), tot.abs())),
          f"scatter n={n} ld={ld} cols={cols} V={V}", 0.0)
    assert dst.cpu()[5].view(torch.int32).equal(init[5].view(torch.int32))


# =====================================================================================================================
# 3. the fused steps
# =====================================================================================================================
STEP_H = (64, 128, 192, 320, 512, 704, 1024)        # k per wave 16 .. 256: one chunk, partial and whole second chunks
STEP_B = (1, 31, 32, 33, 100)
STEP_KX = (64, 192, 320, 576, 1024)


def one_hot_rows(B, K):
    """row b is 1 at one column of k-step b % (K / 16), 0 elsewhere"""
    hot = torch.tensor([16 * (b % (K // 16)) + (5 * b + b // (K // 16)) % 16 for b in range(B)])
    x = torch.zeros(B, K)
    x[torch.arange(B), hot] = 1.0
    return x, hot


def step_fwd(gi, h_prev, hp_bf, whh, bhh):
    ops = KC.ops()
    B, H = h_prev.shape
    h_next, y = torch.full((B, H), float("nan"), device=DEV), torch.zeros(B, H, dtype=BF, device=DEV)
    gh_out = torch.zeros(B, 3 * H, dtype=BF, device=DEV)
    ops.gru_step_fwd(gi.to(DEV), hp_bf.to(DEV), h_prev.to(DEV), ops.pack_frag(whh.to(DEV)), bhh.to(DEV), h_next, y, gh_out)
    return h_next, y, gh_out


@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("H", STEP_H)
def test_fused_forward_step_in_stages_against_fp64(H, B):
    whh, bhh = weights(3 * H, H, 0)
    gi, _, h_prev = cell_inputs(B, H)
    hp_bf = h_prev.to(BF)
    h_next, y, gh_out = step_fwd(gi, h_prev, hp_bf, whh, bhh)
    ref, S = T.proj(hp_bf, whh, bhh)
    case = f"step fwd H={H} B={B}"
    check("STEP", gh_out, ref, T.proj_floor(hp_bf, whh, bhh, ref, S), case + " gh_out", 2.0 ** -8)
    check_cell_fwd(gi, gh_out.cpu(), h_prev, h_next, y, case)


@pytest.mark.parametrize("H", STEP_H)
def test_fused_forward_step_with_one_hot_rows_returns_the_weight_column_plus_bias_exactly(H):
    B = max(33, H // 16 + 3)
    whh, bhh = weights(3 * H, H, 1)
    gi, _, h_prev = cell_inputs(B, H)
    hp, hot = one_hot_rows(B, H)
    h_next, y, gh_out = step_fwd(gi, h_prev, hp.to(BF), whh, bhh)
    want = (whh.float()[:, hot].T + bhh).to(BF)
    bad = torch.nonzero(bits16(gh_out) != bits16(want))
    assert bad.numel() == 0, f"H={H}: gh_out differs at (row, gate column) {bad[:6].tolist()}"
    check_cell_fwd(gi, want, h_prev, h_next, y, f"step fwd one-hot H={H}")


def doubtful(v, F):
    """bf16 rounding of fp64 v, and where v lies within C_STEP F of a rounding boundary (-> rounded, mask, bf16 ulp)"""
    r = T.bf16_round(v)
    ulp = 2.0 ** (torch.floor(torch.log2(r.abs().clamp(min=2.0 ** -126))) - 7)
    return r, (ulp / 2 - (v - r).abs()) <= C["STEP"] * F, ulp


@pytest.mark.parametrize("H,Kx,B", [(H, Kx, B) for H in (64, 320, 704) for Kx in STEP_KX for B in (1, 33)] +
                         [(H, Kx, 100) for H, Kx in ((128, 64), (192, 576), (512, 512), (1024, 1024), (1024, 320), (512, 1024))])
def test_fused_sampling_step_against_fp64(H, Kx, B):
    ops = KC.ops()
    wih, bih = weights(3 * H, Kx, 2)
    whh, bhh = weights(3 * H, H, 3)
    _, _, h_prev = cell_inputs(B, H)
    x = torch.randn(B, Kx, generator=gen(B, Kx, 4)).to(BF)
    hp_bf = h_prev.to(BF)
    h_next, y = torch.full((B, H), float("nan"), device=DEV), torch.zeros(B, H, dtype=BF, device=DEV)
    ops.gru_step_x_fwd(x.to(DEV), ops.pack_frag(wih.to(DEV)), bih.to(DEV), hp_bf.to(DEV), h_prev.to(DEV), ops.pack_frag(whh.to(DEV)),
                       bhh.to(DEV), h_next, y)
    (gi64, Si), (gh64, Sh) = T.proj(x, wih, bih), T.proj(hp_bf, whh, bhh)
    gi, di, ui = doubtful(gi64, T.proj_floor(x, wih, bih, gi64, Si))
    gh, dh_, uh = doubtful(gh64, T.proj_floor(hp_bf, whh, bhh, gh64, Sh))
    c = T.gru_cell_coef(gi, gh, h_prev)
    # first-order effect on h' of one bf16 ulp of each doubtful pre-activation: dh'/dg = (c_r, c_z, c_n) for gi, (c_r, c_z, c_n r) for gh
    ci, ch = torch.cat([c["r"], c["z"], c["n"]], 1).abs(), torch.cat([c["r"], c["z"], c["nr"]], 1).abs()
    slack = (2 * (ci * ui * di + ch * uh * dh_)).reshape(B, 3, H).sum(1)
    frac = (slack > 0).double().mean().item()
    print(f"x_fwd H={H} Kx={Kx} B={B}: {100 * frac:.2f} % of the outputs have a doubtful pre-activation")
    assert frac <= 0.02
    ref = T.gru_cell_fwd(gi, gh, h_prev)
    check("CELL", h_next, ref, T.gru_cell_fwd_floor(gi, gh, h_prev, ref), f"x_fwd H={H} Kx={Kx} B={B} h_next", 0.0, slack)
    assert bits16(y).equal(bits16(h_next.to(BF)))


@pytest.mark.parametrize("H,Kx", [(H, Kx) for H in (64, 704) for Kx in STEP_KX] + [(1024, 1024), (512, 576), (320, 64), (192, 192), (128, 320)])
def test_fused_sampling_step_with_one_hot_rows_of_x_and_h_is_the_cell_on_exact_weight_columns(H, Kx):
    ops = KC.ops()
    B = max(33, H // 16 + 3, Kx // 16 + 3)
    wih, bih = weights(3 * H, Kx, 5)
    whh, bhh = weights(3 * H, H, 6)
    _, _, h_prev = cell_inputs(B, H)
    (x, hx), (hp, hh) = one_hot_rows(B, Kx), one_hot_rows(B, H)
    h_next, y = torch.full((B, H), float("nan"), device=DEV), torch.zeros(B, H, dtype=BF, device=DEV)
    ops.gru_step_x_fwd(x.to(BF).to(DEV), ops.pack_frag(wih.to(DEV)), bih.to(DEV), hp.to(BF).to(DEV), h_prev.to(DEV),
                       ops.pack_frag(whh.to(DEV)), bhh.to(DEV), h_next, y)
    gi, gh = (wih.float()[:, hx].T + bih).to(BF), (whh.float()[:, hh].T + bhh).to(BF)
    check_cell_fwd(gi, gh, h_prev, h_next, y, f"x_fwd one-hot H={H} Kx={Kx}")


def step_bwd(gi, gh, h_prev, dh_direct, dgh_next, whh, dy, final, B, H):
    ops = KC.ops()
    dv = lambda t: None if t is None else t.to(DEV)                                                 # noqa: E731
    dgi, dgh = (torch.full((B, 3 * H), float("nan"), dtype=BF, device=DEV) for _ in range(2))
    dh_out = torch.full((B, H), float("nan"), device=DEV)
    whh_t = ops.pack_frag(whh.T.contiguous().to(DEV))                                               # W_hh^T [H, 3H]
    if final:
        ops.gru_step_bwd(None, None, None, dv(dh_direct), dv(dgh_next), whh_t, None, None, None, dh_out, final=True)
    else:
        ops.gru_step_bwd(dv(gi), dv(gh), dv(h_prev), dv(dh_direct), dv(dgh_next), whh_t, dv(dy), dgi, dgh, dh_out)
    return dgi, dgh, dh_out


@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("H", STEP_H)
def test_fused_backward_step_middle_first_and_final_against_fp64(H, B):
    """H = 128, 512, 1024: eight waves split the 3H gates; the others four.  3H / NS > 192: a second round of loads"""
    whh, _ = weights(3 * H, H, 7)
    gi, gh, h_prev = cell_inputs(B, H)
    g = gen(B, H, 8)
    dh_direct, dy = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g).to(BF)
    dgh_next = torch.randn(B, 3 * H, generator=g).to(BF)
    d_rec, S = T.proj(dgh_next, whh.T)                                        # [B, H] = dgh_next @ W_hh
    Fd = T.proj_floor(dgh_next, whh.T, None, d_rec, S)
    slack = 2.0 ** -8 * d_rec.abs() + C["STEP"] * Fd                          # of the bf16 d_rec inside dh
    coef = T.gru_cell_coef(gi, gh, h_prev)
    case = f"step bwd H={H} B={B}"
    # a middle step: all three parts of dh
    dgi, dgh, dh_out = step_bwd(gi, gh, h_prev, dh_direct, dgh_next, whh, dy, False, B, H)
    check_cell_bwd(gi, gh, h_prev, dh_direct.double() + d_rec + dy.double(), dgi, dgh, dh_out, case + " middle",
                   {k: slack * v.abs() for k, v in coef.items()})
    # the step run first (the sequence's last): no dgh_next, no dh_direct
    dgi, dgh, dh_out = step_bwd(gi, gh, h_prev, None, None, whh, dy, False, B, H)
    check_cell_bwd(gi, gh, h_prev, dy.double(), dgi, dgh, dh_out, case + " first")
    # final: no cell
    _, _, dh_out = step_bwd(None, None, None, dh_direct, dgh_next, whh, None, True, B, H)
    tot = dh_direct.double() + d_rec
    check("STEP", dh_out, tot, Fd + T.ulp32(torch.maximum(dh_direct.double().abs(), d_rec.abs())), case + " final", 0.0, 2.0 ** -8 * d_rec.abs())
    _, _, dh_out = step_bwd(None, None, None, None, dgh_next, whh, None, True, B, H)
    check("STEP", dh_out, d_rec, Fd, case + " final without dh_direct", 2.0 ** -8)


@pytest.mark.parametrize("H", STEP_H)
def test_fused_backward_step_with_one_hot_rows_of_dgh_next_returns_the_weight_row_exactly(H):
    B = 3 * H // 16 + 3
    whh, _ = weights(3 * H, H, 9)
    dgh_next, hot = one_hot_rows(B, 3 * H)
    dh_direct = torch.randn(B, H, generator=gen(H, 10))
    _, _, dh_out = step_bwd(None, None, None, None, dgh_next.to(BF), whh, None, True, B, H)
    bad = torch.nonzero(dh_out.cpu() != whh.float()[hot])
    assert bad.numel() == 0, f"H={H}: d_rec differs at (row, unit) {bad[:6].tolist()}"
    _, _, dh_out = step_bwd(None, None, None, dh_direct, dgh_next.to(BF), whh, None, True, B, H)
    assert dh_out.cpu().view(torch.int32).equal((dh_direct + whh.float()[hot]).view(torch.int32))


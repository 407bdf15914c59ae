"""The training GEMMs of the product library -- the 128 x 128 kernels (csrc/linear_tile128.hip: forward, dX, dW, grouped dW), the
eight-wave and four-wave 256 x 256 ring kernels (csrc/linear_ring.hip: forward, dX) and the ring weight gradient with its fix-up
pass -- against the fp64 references of oracle/train_ref.py (linear_fwd / linear_dx / linear_dw), element by element, inside guard
bands.  Until now every check of these kernels was a max-norm or whole-tensor bound against an fp32 product of Gaussian data: an
element near zero could be wrong by its whole value, and nothing looked at the memory beyond row M or column N.

No bound here is a max-norm bound and none was measured on a kernel.
  exact data    operands are integers of magnitude <= 7, bias <= 2000, addend <= 128, gW0 / gb0 <= 1000: exact in bf16 / fp32, and
                every partial sum in any order is an integer of magnitude <= S = sum |terms|, which each case asserts to lie below
                2^24 FROM THE REFERENCE.  fp32 accumulation is then exact whatever its order, so
                  forward  == bf16_round(act(sum + bias))                  (mgx.h: bias and ReLU in fp32, one RNE rounding)
                  dX       == bf16_round(mask(bf16_round(sum)) + addend)   (mgx.h: round, mask, add in fp32, round)
                  gW, gb   == the fp64 value, also in deterministic mode (2^30 fixed point holds integers below 2^31 exactly)
                with NO tolerance (values compared, so -0 == +0).  Each bf16 case asserts, from the reference, that outputs >= 256
                and outputs exactly on a bf16 tie occur: truncation, a wrong tie and a bias added after the rounding all fail.
  Gaussian data |got - ref| <= 2^-8 |ref| + R 2^-23 S          bf16 output: 2^-8 |ref| is its rounding (half an ulp is at most
                                                               2^-9 |ref|); R 2^-23 S the classical bound of an fp32 sum of R
                                                               terms in any order (R = reduction length, + 1 with a bias);
                                                               check_c of tests/test_gpu_decode_kernels.py
                dX + addend: 2^-8 |ref| + (1 + 2^-8) (2^-8 |p| + R 2^-23 S)    two roundings: p the masked product, ref = p + addend
                gW, gb:      (M + 1) 2^-23 S                   fp32 outputs: M terms and the slot's start value, any order
                elements under a false mask: exactly 0 (exactly the addend when there is one)
                kind "far" has rows far from zero whose offsets cancel in the sum: S >> |ref|, the rounding term is no help.
  guard bands   every operand and every output lies inside a larger allocation, 512 bytes (a multiple of 256: alignment is
                unchanged) before and after it.  Operand bands hold NaN: a read outside the operand poisons the result.  Output
                bands (C, dX, gW, gb) hold the bit pattern 0x5A..: they must come back bit for bit, and so must the interior
                elements the call does not own (the parts of gW next to a ragged ring tile are exact-compared like the rest).
  which kernel  every forward / dX case asserts mgx_linear_kernel_id for the family it names ON THE STREAM IT LAUNCHES ON; every dW
                case asserts whether mgx_linear_dw_grouped_workspace is > 0 (ring + fix-up) or 0 (128 x 128 kernels).  The ring
                kernels are reached at small shapes through a CU-masked stream of 8 CUs (ops.masked_stream(8)): 6 tiles or more.
The product library only: no experiment build, no environment variable.  Every test prints its largest (error / bound) ratio per
family before it asserts (pytest -s; profiles/r15_gemm_kernel_tests.txt has the figures).
"""
import ctypes
import functools

import pytest
import torch

import kernel_checks as KC
from kernel_checks import Det, P, Stream, check_equal, nothing_more_after_a_gpu_error, operand, output  # noqa: F401 (the fixture is used by name)
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

BF, F64 = torch.bfloat16, torch.float64
SKINNY, TILE128, RING8, RING4 = 0, 1, 2, 3
SEEN = {}
_report = KC.report_fixture(SEEN, "largest error / bound {:.3g}")
_raw = functools.partial(KC.raw, product_only=True)


def check_bound(fam, got, ref, bound, case):
    KC.check_bound(fam, got, ref, bound, case, seen=SEEN)


def rounding_is_exercised(pre, case):
    """from the reference alone: some outputs are >= 256 and some lie exactly on a bf16 tie"""
    assert (pre.abs() >= 256).any() and T.on_bf16_tie(pre).any(), f"{case}: the data does not exercise the rounding"


# ---- forward --------------------------------------------------------------------------------------------------------------------
def run_fwd(fam, M, N, K, use_bias, act, kind, cus=0, seed=0):
    lib, chk, _, sp = _raw()
    case = f"fwd {kind} M={M} N={N} K={K} bias={int(use_bias)} act={act} cus={cus}"
    a, w = T.gemm_operands(kind, M, N, K, seed)
    bias = T.gemm_bias(kind, N, seed) if use_bias else None
    A, W, B, C = operand(a), operand(w), operand(bias), output((M, N), BF)
    with Stream(cus):
        assert lib.mgx_linear_kernel_id(0, M, N, K, sp()) == fam, case
        chk(lib.mgx_linear_fwd(P(A), P(W), P(B), P(C), M, N, K, act, sp()), case)
    assert C.bands_intact(), case + ": the call wrote outside C"
    pre, S = T.linear_fwd(a, w, bias, act)
    name = ("SKINNY", "TILE128", "RING8", "RING4")[fam] + " fwd"
    if kind == "exact":
        assert S.max() < 2 ** 24, case
        if K >= 6 and M * N >= 64:
            rounding_is_exercised(pre, case)
        check_equal(name, C.t, T.bf16_round(pre), case)
    else:
        check_bound(name, C.t, pre, KC.gemm_fwd_bound(pre, S, K + (1 if use_bias else 0)), case)


TILE_M = (33, 127, 128, 129, 257)                   # one partial tile; one row short of / exactly / one row past a tile; three tile rows
TILE_N = (4, 12, 124, 132, 340)                     # all N % 8 == 4: the direct epilogue store_tileT; below, at and past a tile, three tile columns
TILE_N8 = (8, 120, 136, 520)                        # N % 8 == 0: the epilogue through LDS (store_tile_lds); also the dX output widths
TILE_K = (64, 128, 192, 512)                        # 1, 2, 3, 8 reduction tiles: none, an even and an odd count of loop trips


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("M", TILE_M)
def test_tile_forward(M, kind):
    """every N and K of the tables with this M; bias / act cycle so that each of the four combinations meets every N, every K"""
    for i_n, N in enumerate(TILE_N + TILE_N8):
        for i_k, K in enumerate(TILE_K):
            combo = (TILE_M.index(M) + i_n + i_k) % 4
            run_fwd(TILE128, M, N, K, bool(combo & 1), combo >> 1, kind)


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("N,use_bias,act", ((2044, True, 1), (2048, False, 1), (2048, True, 0)))
def test_tile_forward_single_lds_buffer(N, use_bias, act, kind):
    """49 x 16 = 784 workgroups >= 768: linear_fwd_kernel<false> (one LDS buffer, two barriers per step); M % 256 != 0 keeps the
    call off the ring.  N = 2044: the direct epilogue; 2048: through LDS.  K = 192: the loop runs (two trips)"""
    assert ((6145 + 127) // 128) * ((N + 127) // 128) >= 768
    run_fwd(TILE128, 6145, N, 192, use_bias, act, kind)


# 8-CU stream: a ring needs >= 6 whole tiles.  19 tiles: the eight workgroups walk three and two tiles, the ring runs across tile
# boundaries (four-wave kernel: its outputs are 512 or 768 wide, so 18 or 20 tiles stand in for 19)
RING8_CASES = [(1536, 256, 128), (2048, 256, 160), (4864, 256, 256), (768, 512, 384), (1536, 256, 576), (4864, 256, 512), (512, 768, 128)]
RING4_CASES = [(768, 512, 512), (1024, 512, 640), (2560, 512, 1024), (512, 768, 512), (1536, 768, 640), (768, 768, 1024)]


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("fam,cases", ((RING8, RING8_CASES), (RING4, RING4_CASES)), ids=("ring8", "ring4"))
def test_ring_forward_on_eight_cus(fam, cases, kind):
    """(the forward needs K % 64 == 0: the reduction of 160, five 32-column steps, is the dX's alone; here it is 192, six steps)"""
    for i, (M, NO, R) in enumerate(cases):
        R = 192 if R == 160 else R
        run_fwd(fam, M, NO, R, bool(i & 1), (i >> 1) & 1, kind, cus=8)
        run_fwd(fam, M, NO, R, not (i & 1), 1 - ((i >> 1) & 1), kind, cus=8, seed=1)


@pytest.mark.parametrize("kind", ("exact", "gauss"))
@pytest.mark.parametrize("fam,R", ((RING8, 256), (RING4, 512)), ids=("ring8", "ring4"))
def test_ring_forward_on_the_whole_device(fam, R, kind):
    """300 tiles on 256 CUs: some workgroups walk two tiles"""
    run_fwd(fam, 38400, 512, R, True, 1, kind)


# ---- dX -------------------------------------------------------------------------------------------------------------------------
EPI = ("none", "mask", "addend", "both")


def run_dx(fam, M, N, K, epi, kind, cus=0, seed=0):
    """dX [M, K] = dY [M, N] . W [N, K]: reduction N, output width K"""
    lib, chk, _, sp = _raw()
    case = f"dx {kind} M={M} N={N} K={K} {epi} cus={cus}"
    dy, wt = T.gemm_operands(kind, M, K, N, seed)                        # wt [K, N]: reduction-contiguous
    w = wt.T.contiguous()
    y = T.relu_mask(M, K, seed) if epi in ("mask", "both") else None
    add = T.gemm_addend(kind, M, K, seed) if epi in ("addend", "both") else None
    DY, W, Y, ADD, DX = operand(dy), operand(w), operand(y), operand(add), output((M, K), BF)
    with Stream(cus):
        assert lib.mgx_linear_kernel_id(1 + EPI.index(epi), M, N, K, sp()) == fam, case
        chk(lib.mgx_linear_dx(P(DY), P(W), P(Y), P(ADD), P(DX), M, N, K, sp()), case)
    assert DX.bands_intact(), case + ": the call wrote outside dX"
    p, S, final = T.linear_dx(dy, w, y, add)
    got = DX.t.cpu().to(F64)
    name = ("SKINNY", "TILE128", "RING8", "RING4")[fam] + " dX"
    keep = torch.ones(M, K, dtype=torch.bool) if y is None else (y.double() > 0)
    if y is not None:
        assert keep.any() and (~keep).any() and (y.double() < 0).any(), case + ": the mask needs values on both sides of zero"
        if K >= 16:
            assert keep[0, 1:1 + len(T.MASK_KEPT)].tolist() == list(T.MASK_KEPT)
        under = got[~keep] if add is None else (got - add.double())[~keep]
        assert (under == 0).all(), case + ": an element under a false mask is not exactly zero (+ addend)"
    if kind == "exact":
        assert S.max() + T.EXACT_ADDEND < 2 ** 24, case
        if N >= 6 and M * K >= 64:
            rounding_is_exercised(p, case)
            if add is not None:
                assert T.on_bf16_tie(torch.where(keep, T.bf16_round(p), torch.zeros((), dtype=F64)) + add.double()).any(), case
        check_equal(name, DX.t, final, case)
    else:
        pm = torch.where(keep, p, torch.zeros((), dtype=F64))
        check_bound(name, DX.t, *KC.gemm_dx_bound(pm, S, N, add), case)


DX_N_GUARDED, DX_N_EXACT = (8, 72, 200), (64, 192, 512)      # N % 64 != 0: zero-filled reduction tail (linear_dx_kernel<., false>)


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("M", TILE_M)
def test_tile_dx(M, kind):
    """every reduction length and output width with this M; the four epilogues cycle so that each meets every N and every K"""
    for i_n, N in enumerate(DX_N_GUARDED + DX_N_EXACT):
        for i_k, K in enumerate(TILE_N8):
            run_dx(TILE128, M, N, K, EPI[(TILE_M.index(M) + i_n + i_k) % 4], kind)


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("N,epi", ((192, "mask"), (200, "addend")))
def test_tile_dx_single_lds_buffer(N, epi, kind):
    """784 workgroups: linear_dx_kernel<false, .>, exact (N = 192) and guarded (N = 200) loads"""
    run_dx(TILE128, 6145, N, 2048, epi, kind)


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
def test_dx_with_mask_and_addend_takes_the_tile_kernel_at_a_ring_shape(kind):
    """the ring kernels have one epilogue per operand: with both, the shape that rides the ring with either goes to 128 x 128"""
    lib, _, _, sp = _raw()
    for M, N, K, fam in ((1536, 128, 256, RING8), (768, 512, 512, RING4)):
        with Stream(8):
            assert lib.mgx_linear_kernel_id(2, M, N, K, sp()) == fam and lib.mgx_linear_kernel_id(3, M, N, K, sp()) == fam
        run_dx(TILE128, M, N, K, "both", kind, cus=8)


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("fam,cases", ((RING8, RING8_CASES), (RING4, RING4_CASES)), ids=("ring8", "ring4"))
def test_ring_dx_on_eight_cus(fam, cases, kind):
    """(M, NO, R) as in the forward: output width NO = K, reduction R = N; none / mask / addend cycle, each case runs two of them"""
    for i, (M, NO, R) in enumerate(cases):
        run_dx(fam, M, R, NO, EPI[i % 3], kind, cus=8)
        run_dx(fam, M, R, NO, EPI[(i + 1) % 3], kind, cus=8, seed=1)


@pytest.mark.parametrize("epi", ("mask", "addend"))
@pytest.mark.parametrize("fam,R", ((RING8, 256), (RING4, 512)), ids=("ring8", "ring4"))
def test_ring_dx_on_the_whole_device(fam, R, epi):
    run_dx(fam, 38400, R, 512, epi, "exact" if epi == "mask" else "gauss")


# ---- dW -------------------------------------------------------------------------------------------------------------------------
def run_dw(M, shapes, kind, *, path, with_gb=True, det=False, cus=0, calls=1, seed=0):
    """path "tile": one mgx_linear_dw per weight (ops.linear_dw would reroute); "tile-grouped" / "ring": mgx_linear_dw_grouped (through
    ops.linear_dw_grouped: it owns the workspace), whose plan must be the 128 x 128 grouped kernel (workspace 0) / the ring kernel
    + fix-up (workspace > 0).  `calls` > 1: the same call again into the same slots (they accumulate)"""
    lib, chk, _, sp = _raw()
    ops = KC.ops()
    case = f"dw {path} {kind} M={M} {shapes} gb={int(with_gb)} det={int(det)} cus={cus} calls={calls}"
    data, bufs = [], []
    for j, (N, K) in enumerate(shapes):
        dyT, xT = T.gemm_operands(kind, N, K, M, seed + 10 * j)           # [N, M], [K, M]: the reduction runs over the rows m
        dy, x = dyT.T.contiguous(), xT.T.contiguous()
        has_b = with_gb and (j % 2 == 0 or len(shapes) == 1)
        gw0, gb0 = T.gemm_grad0(kind, N, K, seed=seed), (T.gemm_grad0(kind, N, seed=seed) if has_b else None)
        data.append((dy, x, gw0, gb0))
        bufs.append((operand(dy), operand(x), output(None, torch.float32, gw0), None if gb0 is None else output(None, torch.float32, gb0)))
    arr = (ops._DwProblem * len(shapes))()
    for j, ((N, K), (DY, X, GW, GB)) in enumerate(zip(shapes, bufs)):
        arr[j] = ops._DwProblem(P(DY), P(X), P(GW), P(GB), N, K)
    need = lib.mgx_linear_dw_grouped_workspace(ctypes.cast(arr, ctypes.c_void_p), len(shapes), M)
    assert (need > 0) == (path == "ring"), case + f": workspace {need}"
    stream = Stream(cus)
    with Det(det, stream.ms), stream:
        for _ in range(calls):
            if path == "tile":
                for (N, K), (DY, X, GW, GB) in zip(shapes, bufs):
                    chk(lib.mgx_linear_dw(P(DY), P(X), P(GW), P(GB), M, N, K, sp()), case)
            else:
                ops.linear_dw_grouped([(DY.t, X.t, GW.t, None if GB is None else GB.t) for DY, X, GW, GB in bufs])
        torch.cuda.synchronize()
    name = {"tile": "TILE128 dW", "tile-grouped": "TILE128 dW grouped", "ring": "RING dW"}[path]
    for (N, K), (dy, x, gw0, gb0), (DY, X, GW, GB) in zip(shapes, data, bufs):
        assert GW.bands_intact() and (GB is None or GB.bands_intact()), case + ": the call wrote outside gW / gb"
        dW, db, SW, Sb = T.linear_dw(dy, x)
        gW, SW = gw0.double() + calls * dW, gw0.double().abs() + calls * SW
        c2 = f"{case} [{N}x{K}]"
        if kind == "exact":
            assert SW.max() < 2 ** 24 and calls * Sb.max() + T.EXACT_GRAD < 2 ** 24, c2
            check_equal(name, GW.t, gW, c2 + " gW")
            if GB is not None:
                check_equal(name, GB.t, gb0.double() + calls * db, c2 + " gb")
        else:
            check_bound(name, GW.t, gW, KC.gemm_dw_bound(SW, calls * M), c2 + " gW")
            if GB is not None:
                check_bound(name, GB.t, gb0.double() + calls * db, KC.gemm_dw_bound(gb0.double().abs() + calls * Sb, calls * M), c2 + " gb")


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "deterministic"))
@pytest.mark.parametrize("nm", range(1, 8))
def test_tile_dw_pipeline_remainders(nm, det):
    """N = K = 128 is one tile, so dw_mchunk makes 256 M-splits of 64 nm rows at M = 16384 nm: nm reduction tiles per split, every
    remainder of the three-register-set pipeline of dw_tile<true> (nm = 1, 2, 3: its prologue alone; 4 .. 7: the loop and its
    tails); M - 8 is not a multiple of the split: dw_tile<false>"""
    M = 16384 * nm
    assert T.dw_tile_plan(M, [(128, 128)], False) == (64 * nm, True, nm) and T.dw_tile_plan(M - 8, [(128, 128)], False)[1:] == (False, nm)
    run_dw(M, [(128, 128)], "exact", path="tile", det=det, with_gb=bool(nm & 1))
    run_dw(M - 8, [(128, 128)], "exact", path="tile", det=det, with_gb=not (nm & 1))
    if not det:
        run_dw(M, [(128, 128)], "gauss", path="tile")
        run_dw(M - 8, [(128, 128)], "far", path="tile")


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("M", (1, 63, 64, 65))
def test_tile_dw_ragged_weights_and_short_batches(M, kind):
    """fewer rows than a reduction tile, one tile, one row more; weights narrower than a tile, not a multiple of a tile, and of two
    tile rows; with and without gb; a second call into the same slots"""
    for i, N in enumerate((8, 72, 136)):
        for j, K in enumerate((8, 200)):
            run_dw(M, [(N, K)], kind, path="tile", with_gb=bool((i + j) & 1), calls=1 + ((i + j + M) & 1), det=(kind == "exact" and j == 1))


GROUP = [(8, 8), (72, 200), (136, 8), (128, 128), (64, 64), (256, 128), (8, 200), (136, 200)]     # none fills a 256 x 256 tile to 60 %


@pytest.mark.parametrize("kind", T.GEMM_KINDS)
@pytest.mark.parametrize("count", (1, 4, 8))
def test_tile_dw_grouped(count, kind):
    """the grouped 128 x 128 kernel: M a whole number of splits (dw_tile<true>, three reduction tiles each), M % 32 != 0 below 4096
    and above it (dw_tile<false>)"""
    shapes = GROUP[3:4] if count == 1 else GROUP[:count]
    tiles = sum(((N + 127) // 128) * ((K + 127) // 128) for N, K in shapes)
    m_exact = 192 * ((480 + tiles - 1) // tiles)
    assert T.dw_tile_plan(m_exact, shapes, True) == (192, True, 3)
    for M in (m_exact, 1000, 4104):
        assert M == m_exact or not T.dw_tile_plan(M, shapes, True)[1]
        run_dw(M, shapes, kind, path="tile-grouped", calls=2 if M == 1000 else 1)
    run_dw(1000, shapes, kind, path="tile-grouped", with_gb=False, det=(kind == "exact"))


@pytest.mark.parametrize("det", (False, True), ids=("plain", "deterministic"))
@pytest.mark.parametrize("kind", ("exact", "gauss"))
@pytest.mark.parametrize("M,shapes,path", (
    (4096, [(256, 256)], "ring"),                                         # one tile, 128 splits of ONE 32-row step
    (4096, [(448, 512)], "ring"), (4096, [(456, 520)], "ring"),           # ragged last tile row / column; odd multiples of 8
    (4096, [(768, 768), (128, 768), (768, 384)], "ring"),                 # mixed: 128 x 768 goes to the 128 x 128 grouped kernel
    (4096 + 8, [(256, 256)], "tile-grouped"), (2048, [(256, 256)], "tile-grouped"),      # M % 32 != 0, M < 4096: no ring
))
def test_ring_dw_on_the_whole_device(M, shapes, path, kind, det):
    run_dw(M, shapes, kind, path=path, det=det)
    if not det:
        run_dw(M, shapes, kind, path=path, with_gb=False, calls=2, seed=1)


@pytest.mark.parametrize("det", (False, True), ids=("plain", "deterministic"))
@pytest.mark.parametrize("kind", ("exact", "gauss"))
@pytest.mark.parametrize("M", (4096, 4096 + 160))
def test_ring_dw_on_eight_cus(M, kind, det):
    """512 x 256 is two tiles: four long M-splits on eight CUs (32 or 34 steps of 32 rows; at 4096 + 160 the last split is ragged);
    in deterministic mode the plan is the whole device's"""
    run_dw(M, [(512, 256)], kind, path="ring", cus=8, det=det)
    run_dw(M, [(512, 256)], kind, path="ring", cus=8, det=det, with_gb=False, seed=1)


# ---- special values -------------------------------------------------------------------------------------------------------------
FWD_SPECIAL = ((SKINNY, 8, 64, 128, 0), (TILE128, 129, 132, 128, 0), (TILE128, 129, 136, 128, 0), (RING8, 1536, 256, 128, 8), (RING4, 768, 512, 512, 8))


@pytest.mark.parametrize("use_bias", (False, True))
@pytest.mark.parametrize("act", (0, 1))
@pytest.mark.parametrize("fam,M,N,K,cus", FWD_SPECIAL, ids=("skinny", "tile-direct", "tile-lds", "ring8", "ring4"))
def test_forward_special_values(fam, M, N, K, cus, act, use_bias):
    """mgx.h: the ReLU propagates NaN.  Pre-activations that are NaN -- from a NaN input of either sign (rows 1, 2), from +inf and
    -inf meeting in one row (row 3), from 0 * inf (row 4) -- stay NaN; +inf stays +inf and -inf becomes 0 (row 5, even / odd
    columns); without the ReLU every one of them passes through.  All other rows are integer data and exact."""
    lib, chk, _, sp = _raw()
    case = f"fwd special fam={fam} M={M} N={N} K={K} act={act} bias={int(use_bias)}"
    a, w = T.gemm_operands("exact", M, N, K)
    bias = T.gemm_bias("exact", N) if use_bias else None
    a, w = a.float(), w.float()
    w[:, 0], w[:, 1], w[:, 2] = 1.0, -1.0, 0.0
    w[:, 3] = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    a[1:6, :4] = 0.0
    a[1, 0], a[2, 0] = float("nan"), float("nan")
    a[3, 0], a[3, 1] = float("inf"), float("inf")
    a[4, 2] = float("inf")
    a[5, 3] = float("inf")
    a, w = a.to(BF), w.to(BF)
    a.view(torch.int16)[1, 0], a.view(torch.int16)[2, 0] = 0x7FC0, 0xFFC0 - 0x10000         # NaN with the sign bit clear / set
    assert torch.isnan(a[1:3, 0]).all()
    A, W, B, C = operand(a), operand(w), operand(bias), output((M, N), BF)
    with Stream(cus):
        assert lib.mgx_linear_kernel_id(0, M, N, K, sp()) == fam, case
        chk(lib.mgx_linear_fwd(P(A), P(W), P(B), P(C), M, N, K, act, sp()), case)
    assert C.bands_intact(), case
    lin, _ = T.linear_fwd(a, w, bias, 0)
    even = torch.arange(N) % 2 == 0
    # the case is what it claims to be, from the reference alone
    assert torch.isnan(lin[1:5]).all() and (lin[5, even] == float("inf")).all() and (lin[5, ~even] == -float("inf")).all()
    assert torch.isfinite(lin[0]).all() and torch.isfinite(lin[6:]).all()
    want = T.bf16_round(T.relu(lin) if act else lin)
    got = C.t.cpu().to(F64)
    bad = torch.nonzero(~((got == want) | (torch.isnan(got) & torch.isnan(want))))
    assert bad.numel() == 0, (case, bad[:6].tolist(), [got[tuple(i)].item() for i in bad[:6]], [want[tuple(i)].item() for i in bad[:6]])

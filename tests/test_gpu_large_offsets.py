"""The kernels that are indexed by row x width, at the smallest shapes whose byte offsets pass 2^31 and 2^32 -- bench.py's own
shape (cfg2, batch 128: a 4.36 GB dS workspace) among them.  The per-kernel modules check every element against fp64 at every
tile and chunk edge, at sizes whose offsets fit in 31 bits; what they cannot see is an offset that wraps modulo 2^32 or is
sign-extended between 2^31 and 2^32 (the four-wave GEMM epilogue, the ring kernels' lane tables and every attention sweep address
with "64-bit base + 32-bit lane offset").  Through the raw C ABI of the product library, outputs inside 0x5A guard bands.

Three checks per case:
  (a) fp64 on sampled row blocks of the big call's own output: the first block, the block around the 2^31-byte and the 2^32-byte
      mark of every operand and output that has one, the last block (large_offsets.sample_blocks; for attention a block is one
      (b, h) pair, the marks those of its dS tiles), with the references, floors and constants of the kernel's own module:
      test_gpu_gemm_kernels (Gaussian bounds), test_gpu_rowwise_kernels (C_LNF 8, C_LNB 4, C_CE 8, C_EMB 4), test_gpu_attn_kernels
      (attn_*_bounds), test_gpu_decode_kernels (C_ATTN 16).  No new tolerance.
  (b) every row, bit for bit: the big call equals calls on row chunks that stay below 2^31 bytes in every operand
      (large_offsets.row_chunks, compare_rows).  Rows that alias -- the writer and both readers of a wrapped dS tile land on an
      earlier pair alike, the last writer wins -- differ from their chunk call, which (a) need not have sampled.  The chunk shapes
      are ones the fp64 modules cover per row; a chunk may take another GEMM family or another attention batch group, whose
      bit-identity tests/test_gpu_ring.py and tests/test_gpu_kernels.py assert.  Where a chunk call cannot compute the same thing
      (dropout: the mask is a function of the element index from the call's base) every row goes through (a)'s floors instead,
      evaluated on the device in fp64; the LayerNorm cases do that for p = 0 as well.
  (c) the guard bands of every output and workspace come back intact.
Cross-row reductions (dW / db, dgamma / dbeta / dxsum, the CE statistics, the embedding gradient) are checked against an fp64 sum
accumulated on the device in row chunks, inside the floor formula of their own module evaluated on the same chunks; the CE counts
with ==.  dE: the whole call against the sum of the chunk calls, each into a zeroed dE, within the 2e-5 that
test_full_size_dE_and_dQ_two_ways allows between two implementations, on both of its routes.

Data: seeded device draws of at most 2^26 elements written straight into the operands -- one stream, no period (rows tiled from a
small block would map a wrap onto equal values).  Every test holds less than 24 GB and releases it; each prints its peak.
profiles/r28_large_offset_tests.txt has the reading of the address arithmetic per family and the measured figures.
tests/test_large_offset_helpers.py shows on the CPU that (b) fails on a wrap, an unwritten row and two swapped rows."""
import ctypes
import functools
import gc
import math

import pytest
import torch

import kernel_checks as KC
import large_offsets as LO
from kernel_checks import P, nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import decode_ref as D
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
SKINNY, TILE128, RING8, RING4 = 0, 1, 2, 3
FAMILY = ("SKINNY", "TILE128", "RING8", "RING4")
C = {"LNF": 8.0, "LNB": 4.0, "CE": 8.0, "EMB": 4.0, "DEC": 16.0}     # the constants of test_gpu_rowwise_kernels / test_gpu_decode_kernels
MEM_LIMIT = 24e9
SEEN = {}
_report = KC.report_fixture(SEEN, "largest ratio {:.3g}")
_raw = functools.partial(KC.raw, product_only=True)


@pytest.fixture(autouse=True)
def memory_is_bounded_and_released(request):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    print(f"\nPEAK {request.node.name}: {peak / 1e9:.2f} GB")
    gc.collect()
    torch.cuda.empty_cache()
    assert peak <= MEM_LIMIT, f"{request.node.name} held {peak / 1e9:.2f} GB"
    assert torch.cuda.memory_allocated() < 1e9, f"{request.node.name} left {torch.cuda.memory_allocated() / 1e9:.2f} GB allocated"


def whole_device():
    return torch.cuda.get_device_properties(0).multi_processor_count == 256       # the routing table is written for 256 CUs


def sync():
    torch.cuda.synchronize()


def check_bound(fam, got, ref, bound, case):
    KC.check_bound(fam, got, ref, bound, case, seen=SEEN)


def check_floor(fam, key, got, ref, F, case, rounding=0.0):
    KC.check_floor(fam, got, ref, F, case, C=C[key], seen=SEEN, rounding=rounding)


class Worst:
    """(a)'s floor check on the device, over the chunks of one output: the largest (|got - ref| - rounding |ref|) / F"""

    def __init__(self, fam, key, case, rounding=0.0):
        self.fam, self.key, self.case, self.rounding, self.worst = fam, key, case, rounding, -float("inf")

    def add(self, got, ref, F):
        got = got.to(F64).reshape(ref.shape)
        assert torch.isfinite(got).all(), (self.fam, self.case, "non-finite output")
        F = F.to(F64)
        while F.dim() < ref.dim():
            F = F.unsqueeze(-1)
        assert (F > 0).all(), (self.fam, self.case, "a floor is not positive")
        self.worst = max(self.worst, (((got - ref).abs() - self.rounding * ref.abs()) / F).max().item())

    def done(self):
        KC._note(SEEN, self.fam, self.worst, self.case, f"[{self.fam}] {self.case}: ratio {self.worst:.3f} (every row, on the device)")
        assert self.worst <= C[self.key], f"{self.fam} {self.case}: ratio {self.worst:.2f} > {C[self.key]}"


# =====================================================================================================================
# 1. GEMMs.  Read: csrc/linear.hip routes on (M, output width, reduction); the four-wave ring kernel is refused at out_elems * 2
#    >= 2^32 because store_wave_block4 forms uint32 byte offsets from the matrix base (zero-extended when added to the pointer:
#    legal up to 2^32 - 16); its tile bases a_base / b_base, the eight-wave kernel's row pointers and every address of the
#    128 x 128 kernels are size_t products; the lane tables hold offsets inside one 256-row tile.  The ring weight gradient takes
#    64-bit stage bases per M-split and 32-bit bytes per stage.
# =====================================================================================================================
GEMM_M = ((1 << 21) - 256, (1 << 21) + 256, (1 << 21) + 264)
GEMM_BLOCK = 256                                    # rows of a sampled block: one ring tile


def small_weights(N, K, seed):
    g = KC.gen(N, K, seed)
    return (torch.randn(N, K, generator=g) / K ** 0.5).to(BF), torch.randn(N, generator=g)


@pytest.mark.parametrize("M,N,K,fam", ((GEMM_M[0], 1024, 512, RING4), (GEMM_M[1], 1024, 512, RING8), (GEMM_M[2], 1024, 64, TILE128)),
                         ids=("ring4-below-2^32", "ring8-past-2^32", "tile128-past-2^32"))
def test_linear_forward(M, N, K, fam):
    lib, chk, _, sp = _raw()
    act = 1 if fam == TILE128 else 0
    case = f"fwd M={M} N={N} K={K} act={act}"
    if whole_device():
        assert lib.mgx_linear_kernel_id(0, M, N, K, None) == fam, case
    assert (M * N * 2 >= 1 << 32) == (fam != RING4) and M * N * 2 > 1 << 31
    w, bias = small_weights(N, K, 1)
    A, W, B, Cout = LO.big_operand((M, K), BF), KC.operand(w), KC.operand(bias), LO.big_output((M, N), BF)
    LO.fill_normal(A.t, LO.device_gen(M + N + K), 0.5)
    chk(lib.mgx_linear_fwd(P(A), P(W), P(B), P(Cout), M, N, K, act, sp()), case)
    sync()
    assert Cout.bands_intact(), case + ": the call wrote outside C"
    name = FAMILY[fam] + " fwd" if whole_device() else "fwd"
    for lo, hi in LO.sample_blocks(M, GEMM_BLOCK, (2 * K, 2 * N)):
        pre, S = T.linear_fwd(A.t[lo:hi].cpu(), w, bias, act)
        check_bound(name, Cout.t[lo:hi], pre, 2.0 ** -8 * pre.abs() + (K + 1) * 2.0 ** -23 * S, f"{case} rows {lo}:{hi}")
    chunks = LO.row_chunks(M, (2 * K, 2 * N), align=256)
    Cc = LO.big_output((chunks[0][1], N), BF)

    def chunk(lo, hi):
        Cc.refill()
        chk(lib.mgx_linear_fwd(A.t[lo:hi].data_ptr(), P(W), P(B), P(Cc), hi - lo, N, K, act, sp()), case)
        return Cc.t[:hi - lo]
    LO.compare_rows(name, Cout.t, chunk, chunks, case)
    assert Cc.bands_intact() and Cout.bands_intact(), case
    del A, Cout, Cc


EPI = ("none", "mask", "addend")


@pytest.mark.parametrize("epi", EPI)
@pytest.mark.parametrize("M,fam", tuple(zip(GEMM_M, (RING4, RING8, TILE128))), ids=("ring4-below-2^32", "ring8-past-2^32", "tile128-past-2^32"))
def test_linear_dx(M, fam, epi):
    """dX [M, 1024] = dY [M, 512] . W [512, 1024]: the output, the mask and the addend are the operands past the marks"""
    lib, chk, _, sp = _raw()
    N, K = 512, 1024
    case = f"dx M={M} N={N} K={K} {epi}"
    if whole_device():
        assert lib.mgx_linear_kernel_id(1 + EPI.index(epi), M, N, K, None) == fam, case
    w = small_weights(K, N, 2)[0].T.contiguous()                       # [N, K]
    g = LO.device_gen(M + EPI.index(epi))
    DY, W, DX = LO.big_operand((M, N), BF), KC.operand(w), LO.big_output((M, K), BF)
    LO.fill_normal(DY.t, g, 0.5)
    Y = LO.fill_normal(LO.big_operand((M, K), BF).t, g) if epi == "mask" else None
    ADD = LO.fill_normal(LO.big_operand((M, K), BF).t, g) if epi == "addend" else None
    yp = lambda t, lo: None if t is None else t[lo:].data_ptr()                                         # noqa: E731
    chk(lib.mgx_linear_dx(P(DY), P(W), yp(Y, 0), yp(ADD, 0), P(DX), M, N, K, sp()), case)
    sync()
    assert DX.bands_intact(), case + ": the call wrote outside dX"
    name = FAMILY[fam] + " dX" if whole_device() else "dX"
    for lo, hi in LO.sample_blocks(M, GEMM_BLOCK, (2 * N, 2 * K)):
        y, add = (None if t is None else t[lo:hi].cpu() for t in (Y, ADD))
        p, S, _ = T.linear_dx(DY.t[lo:hi].cpu(), w, y, add)
        keep = torch.ones(hi - lo, K, dtype=torch.bool) if y is None else (y.double() > 0)
        got = DX.t[lo:hi].cpu().to(F64)
        if y is not None:
            assert keep.any() and (~keep).any() and (got[~keep] == 0).all(), case + ": an element under a false mask is not exactly zero"
        pm = torch.where(keep, p, torch.zeros((), dtype=F64))
        first = 2.0 ** -8 * pm.abs() + N * 2.0 ** -23 * S
        if add is None:
            check_bound(name, DX.t[lo:hi], pm, first, f"{case} rows {lo}:{hi}")
        else:
            ref = pm + add.double()
            check_bound(name, DX.t[lo:hi], ref, 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * first, f"{case} rows {lo}:{hi}")
    chunks = LO.row_chunks(M, (2 * N, 2 * K), align=256)
    Dc = LO.big_output((chunks[0][1], K), BF)

    def chunk(lo, hi):
        Dc.refill()
        chk(lib.mgx_linear_dx(DY.t[lo:hi].data_ptr(), P(W), yp(Y, lo), yp(ADD, lo), P(Dc), hi - lo, N, K, sp()), case)
        return Dc.t[:hi - lo]
    LO.compare_rows(name, DX.t, chunk, chunks, case)
    assert Dc.bands_intact() and DX.bands_intact(), case
    del DY, DX, Dc, Y, ADD


@pytest.mark.parametrize("grouped", (False, True), ids=("tile128", "ring-grouped"))
def test_linear_dw(grouped):
    """gW [1024, 512] += dY [M, 1024]^T X [M, 512], gb += column sums of dY, M = 2^21 + 256: dY passes 2^32 bytes, X 2^31.  The
    grouped call plans the ring kernel at 8 tiles x 32 M-splits.  Reference: fp64 products accumulated on the device in row
    chunks; bound of test_gpu_gemm_kernels' Gaussian data, (M + 1) 2^-23 sum |terms|, from the same chunks"""
    lib, chk, _, sp = _raw()
    ops = KC.ops()
    M, N, K = GEMM_M[1], 1024, 512
    case = f"dw {'grouped' if grouped else 'single'} M={M} N={N} K={K}"
    g = LO.device_gen(M + int(grouped))
    DY, X = LO.big_operand((M, N), BF), LO.big_operand((M, K), BF)
    LO.fill_normal(DY.t, g, 0.5), LO.fill_normal(X.t, g, 0.5)
    GW, GB = KC.output(None, F32, torch.zeros(N, K)), KC.output(None, F32, torch.zeros(N))
    if grouped:
        arr = (ops._DwProblem * 1)(ops._DwProblem(P(DY), P(X), P(GW), P(GB), N, K))
        parr = ctypes.cast(arr, ctypes.c_void_p)
        need = lib.mgx_linear_dw_grouped_workspace(parr, 1, M)
        if whole_device():
            assert need == 8 * 32 * 65536 * 4, (case, need)            # 8 tiles x 32 splits of one 256 x 256 fp32 tile
        assert need > 0, case + ": the group must take the ring kernel"
        WS = LO.big_output((need,), torch.uint8)
        chk(lib.mgx_linear_dw_grouped(parr, 1, M, P(WS), need, sp()), case)
    else:
        WS = None
        chk(lib.mgx_linear_dw(P(DY), P(X), P(GW), P(GB), M, N, K, sp()), case)
    sync()
    assert GW.bands_intact() and GB.bands_intact() and (WS is None or WS.bands_intact()), case + ": the call wrote outside gW / gb / its workspace"
    gW, SW = torch.zeros(N, K, dtype=F64, device=DEV), torch.zeros(N, K, dtype=F64, device=DEV)
    gb, Sb = torch.zeros(N, dtype=F64, device=DEV), torch.zeros(N, dtype=F64, device=DEV)
    for lo in range(0, M, 1 << 16):
        dy, x = DY.t[lo:lo + (1 << 16)].double(), X.t[lo:lo + (1 << 16)].double()
        gW += dy.T @ x
        SW += dy.abs().T @ x.abs()
        gb += dy.sum(0)
        Sb += dy.abs().sum(0)
        del dy, x
    name = "RING dW" if grouped else "TILE128 dW"
    check_bound(name, GW.t, gW.cpu(), ((M + 1) * 2.0 ** -23 * SW).cpu(), case + " gW")
    check_bound(name, GB.t, gb.cpu(), ((M + 1) * 2.0 ** -23 * Sb).cpu(), case + " gb")
    # that bound grows with M; rows lost or read twice are what this module is after: the whole call against calls on row chunks
    # below 2^31 bytes that accumulate into one second slot, within the 1e-5 test_full_size_grouped_dW allows between two launches
    G2, B2 = KC.output(None, F32, torch.zeros(N, K)), KC.output(None, F32, torch.zeros(N))
    for lo, hi in LO.row_chunks(M, (2 * N, 2 * K), align=256):
        if grouped:
            arr = (ops._DwProblem * 1)(ops._DwProblem(DY.t[lo:hi].data_ptr(), X.t[lo:hi].data_ptr(), P(G2), P(B2), N, K))
            parr = ctypes.cast(arr, ctypes.c_void_p)
            assert lib.mgx_linear_dw_grouped_workspace(parr, 1, hi - lo) <= need
            chk(lib.mgx_linear_dw_grouped(parr, 1, hi - lo, P(WS), need, sp()), case)
        else:
            chk(lib.mgx_linear_dw(DY.t[lo:hi].data_ptr(), X.t[lo:hi].data_ptr(), P(G2), P(B2), hi - lo, N, K, sp()), case)
    sync()
    assert G2.bands_intact() and B2.bands_intact() and (WS is None or WS.bands_intact()), case
    rw, rb = LO.rel(GW.t, G2.t), LO.rel(GB.t, B2.t)
    print(f"[{name}] {case}: whole call vs chunk calls rel gW {rw:.3g} gb {rb:.3g}; vs fp64 rel gW {LO.rel(GW.t, gW):.3g} gb {LO.rel(GB.t, gb):.3g}")
    assert rw < 1e-5 and rb < 1e-5, (case, rw, rb)
    del DY, X, WS


# =====================================================================================================================
# 2. residual + LayerNorm.  Read (csrc/rowwise_ops.hip): one wave per row, every address (size_t) r * d + col; the forward's grid is
#    capped at 2^20 workgroups (rows 2^22 + 3: the waves loop once), the backward's at 512 (the waves loop 2049 times; r + nwave
#    stays far below 2^31); the dropout group index (uint32_t) (r * d / 8 + col / 8) reaches 2^28.
# =====================================================================================================================
LN_PIECE = 1 << 22                                  # elements per fp64 piece of the device reference


def ln_mult_cpu(cfg, lo, hi, d):
    if cfg[0] == 0:
        return None
    g = (torch.arange(lo, hi, dtype=torch.int64)[:, None] * (d // 8) + torch.arange(d // 8)[None, :]).reshape(-1).numpy()
    return torch.from_numpy(T.drop_mult8(cfg, g)).reshape(hi - lo, d)


@pytest.mark.parametrize("p_drop", (0.0, 0.1))
@pytest.mark.parametrize("rows,d", (((1 << 22) + 3, 512), ((1 << 20) + 1, 2048)))
def test_layernorm(rows, d, p_drop):
    lib, chk, _, sp = _raw()
    seed, eps = (1 << 32) + 9, 1e-6
    case = f"ln rows={rows} d={d} p={p_drop}"
    assert rows * d > 1 << 31
    cfg = T.make_drop(p_drop, seed)
    g = LO.device_gen(rows + d)
    gc_ = KC.gen(d, 5)
    gamma, beta = 1 + 0.5 * torch.randn(d, generator=gc_), torch.randn(d, generator=gc_)
    GA, BE = KC.operand(gamma), KC.operand(beta)
    X, R = LO.big_operand((rows, d), BF), LO.big_operand((rows, d), BF)
    LO.fill_normal(X.t, g), LO.fill_normal(R.t, g, 1.0, 0.25)
    OUT, MEAN, RSTD = LO.big_output((rows, d), BF), LO.big_output((rows,), F32), LO.big_output((rows,), F32)
    chk(lib.mgx_add_ln_fwd(P(X), P(R), P(GA), P(BE), P(OUT), P(MEAN), P(RSTD), rows, d, eps, float(p_drop), seed, sp()), case)
    sync()
    assert OUT.bands_intact() and MEAN.bands_intact() and RSTD.bands_intact(), case + ": the forward wrote outside out / mean / rstd"
    blocks = LO.sample_blocks(rows, 4, (2 * d,))
    assert LO.marks_inside(rows * 2 * d) == list(LO.MARKS) and len(blocks) >= 3          # (the 2^32 block may be the last block)
    for lo, hi in blocks:                                                   # (a), as run_ln of test_gpu_rowwise_kernels
        x, res, mult, c2 = X.t[lo:hi].cpu(), R.t[lo:hi].cpu(), ln_mult_cpu(cfg, lo, hi, d), f"{case} rows {lo}:{hi}"
        ref = T.add_ln_fwd(x, res, gamma, beta, eps, mult)
        Fm, Fr = T.add_ln_fwd_floor(x, res, gamma, beta, eps, mult, ref)
        mk, rk = MEAN.t[lo:hi].cpu(), RSTD.t[lo:hi].cpu()
        check_floor("LN fwd", "LNF", mk, ref[0], Fm, c2 + " mean")
        check_floor("LN fwd", "LNF", rk, ref[1], Fr, c2 + " rstd")
        staged = T.add_ln_out(x, res, gamma, beta, mk, rk, mult)
        check_floor("LN fwd", "LNF", OUT.t[lo:hi], staged, T.add_ln_out_floor(x, res, gamma, beta, mk, rk, mult, staged), c2 + " out", 2.0 ** -8)
        if mult is not None:
            assert (mult == 0).any() and (mult != 0).any()
    chunks = LO.row_chunks(rows, (2 * d,), max_rows=(1 << 28) // d)
    if p_drop == 0:                                                         # (b): 0.5 GB chunks
        Oc, Mc, Rc = LO.big_output((chunks[0][1], d), BF), LO.big_output((chunks[0][1],), F32), LO.big_output((chunks[0][1],), F32)
        mean_c, rstd_c = torch.empty_like(MEAN.t), torch.empty_like(RSTD.t)

        def fwd_chunk(lo, hi):
            for b in (Oc, Mc, Rc):
                b.refill()
            chk(lib.mgx_add_ln_fwd(X.t[lo:hi].data_ptr(), R.t[lo:hi].data_ptr(), P(GA), P(BE), P(Oc), P(Mc), P(Rc), hi - lo, d, eps, 0.0, seed,
                                   sp()), case)
            mean_c[lo:hi], rstd_c[lo:hi] = Mc.t[:hi - lo], Rc.t[:hi - lo]
            return Oc.t[:hi - lo]
        LO.compare_rows("LN fwd", OUT.t, fwd_chunk, chunks, case + " out")
        LO.compare_rows("LN fwd", MEAN.t, lambda lo, hi: mean_c[lo:hi], chunks, case + " mean")
        LO.compare_rows("LN fwd", RSTD.t, lambda lo, hi: rstd_c[lo:hi], chunks, case + " rstd")
        assert Oc.bands_intact() and Mc.bands_intact() and Rc.bands_intact(), case
        del Oc, Mc, Rc, mean_c, rstd_c
    # every row of the forward on the device, and nothing of `out` is needed after it
    ga, be = gamma.to(DEV), beta.to(DEV)
    piece = LN_PIECE // d
    wm, wr, wo = Worst("LN fwd", "LNF", case + " mean"), Worst("LN fwd", "LNF", case + " rstd"), Worst("LN fwd", "LNF", case + " out", 2.0 ** -8)
    for lo in range(0, rows, piece):
        hi = min(rows, lo + piece)
        x, res, mult = X.t[lo:hi], R.t[lo:hi], (LO.drop_mult_rows(cfg, lo, hi, d, DEV) if p_drop > 0 else None)
        ref = T.add_ln_fwd(x, res, ga, be, eps, mult)
        Fm, Fr = T.add_ln_fwd_floor(x, res, ga, be, eps, mult, ref)
        wm.add(MEAN.t[lo:hi], ref[0], Fm), wr.add(RSTD.t[lo:hi], ref[1], Fr)
        staged = T.add_ln_out(x, res, ga, be, MEAN.t[lo:hi], RSTD.t[lo:hi], mult)
        wo.add(OUT.t[lo:hi], staged, T.add_ln_out_floor(x, res, ga, be, MEAN.t[lo:hi], RSTD.t[lo:hi], mult, staged))
        del ref, staged, mult, Fm, Fr
    for w_ in (wm, wr, wo):
        w_.done()
    del OUT
    torch.cuda.empty_cache()
    # ---- backward, from the mean / rstd the forward kernel saved ----
    DO = LO.big_operand((rows, d), BF)
    LO.fill_normal(DO.t, g)
    DRES = LO.big_output((rows, d), BF)
    DX = LO.big_output((rows, d), BF) if p_drop > 0 else DRES               # p = 0: dx may alias dres, as ops.add_ln_bwd calls it
    DG, DB, DS = (KC.output(None, F32, torch.zeros(d)) for _ in range(3))
    need = lib.mgx_add_ln_bwd_workspace(rows, d)
    WS = LO.big_output((need,), torch.uint8)

    def bwd(dout, x, res, mean, rstd, dx, dres, dg, db, ds, n):
        chk(lib.mgx_add_ln_bwd(dout, x, res, P(GA), mean, rstd, dx, dres, dg, db, ds, P(WS), need, n, d, float(p_drop), seed, sp()), case)
    bwd(P(DO), P(X), P(R), P(MEAN), P(RSTD), P(DX), P(DRES), P(DG), P(DB), P(DS), rows)
    sync()
    assert all(b.bands_intact() for b in (DRES, DX, DG, DB, DS, WS)), case + ": the backward wrote outside an output or its workspace"
    for lo, hi in blocks:
        x, res, dout, mult, c2 = X.t[lo:hi].cpu(), R.t[lo:hi].cpu(), DO.t[lo:hi].cpu(), ln_mult_cpu(cfg, lo, hi, d), f"{case} rows {lo}:{hi}"
        mk, rk = MEAN.t[lo:hi].cpu(), RSTD.t[lo:hi].cpu()
        rb = T.add_ln_bwd(dout, x, res, gamma, mk, rk, mult)
        Frow, _, _ = T.add_ln_bwd_floor(dout, x, res, gamma, mk, rk, mult, rb)
        check_floor("LN bwd", "LNB", DRES.t[lo:hi], rb[0], Frow, c2 + " dres", 2.0 ** -8)
        check_floor("LN bwd", "LNB", DX.t[lo:hi], rb[1], Frow, c2 + " dx", 2.0 ** -8)
    if p_drop == 0:
        Dc = LO.big_output((chunks[0][1], d), BF)
        sg, sb, ss = (torch.zeros(d, device=DEV) for _ in range(3))

        def bwd_chunk(lo, hi):
            Dc.refill()
            bwd(DO.t[lo:hi].data_ptr(), X.t[lo:hi].data_ptr(), R.t[lo:hi].data_ptr(), MEAN.t[lo:hi].data_ptr(), RSTD.t[lo:hi].data_ptr(), P(Dc), P(Dc),
                sg.data_ptr(), sb.data_ptr(), ss.data_ptr(), hi - lo)
            return Dc.t[:hi - lo]
        LO.compare_rows("LN bwd", DRES.t, bwd_chunk, chunks, case)
        assert Dc.bands_intact() and WS.bands_intact(), case
        del Dc
    wres, wdx = Worst("LN bwd", "LNB", case + " dres", 2.0 ** -8), Worst("LN bwd", "LNB", case + " dx", 2.0 ** -8)
    acc = {k: torch.zeros(d, dtype=F64, device=DEV) for k in ("g", "ga", "b", "ba", "s", "sa")}
    for lo in range(0, rows, piece):
        hi = min(rows, lo + piece)
        x, res, dout, mult = X.t[lo:hi], R.t[lo:hi], DO.t[lo:hi], (LO.drop_mult_rows(cfg, lo, hi, d, DEV) if p_drop > 0 else None)
        mk, rk = MEAN.t[lo:hi], RSTD.t[lo:hi]
        rb = T.add_ln_bwd(dout, x, res, ga, mk, rk, mult)
        Frow, _, _ = T.add_ln_bwd_floor(dout, x, res, ga, mk, rk, mult, rb)
        wres.add(DRES.t[lo:hi], rb[0], Frow), wdx.add(DX.t[lo:hi], rb[1], Frow)
        if mult is not None:
            assert (DX.t[lo:hi][mult == 0] == 0).all(), case + ": a dropped element of dx is not 0"
        xh = (x.double() * (1.0 if mult is None else mult) + res.double() - mk.double()[:, None]) * rk.double()[:, None]
        terms, dxk = dout.double() * xh, DX.t[lo:hi].double()              # dxsum: the kernel sums what the consumer reads, its own bf16 dx
        for k, v in (("g", terms), ("b", dout.double()), ("s", dxk)):
            acc[k] += v.sum(0)
            acc[k + "a"] += v.abs().sum(0)
        del rb, Frow, xh, terms, dxk, mult
    wres.done(), wdx.done()
    for name, got, k in (("dgamma", DG, "g"), ("dbeta", DB, "b"), ("dxsum", DS, "s")):
        tot = acc[k].cpu()
        F = T.EPS32 * acc[k + "a"].cpu() + T.ulp32(tot)                    # train_ref.sum_floor over the pieces; + the start value's term of run_ln
        F = F + (T.ulp32(torch.zeros(d, dtype=F64)) if name == "dxsum" else T.ulp32(tot))
        check_floor("LN bwd", "LNB", got.t, tot, F, f"{case} {name}")
    del X, R, DO, DRES, DX, MEAN, RSTD, WS


# =====================================================================================================================
# 3. smoothed cross entropy.  Read: one wave per row, lp = logits + (size_t) r * ld, the same for dlogits; 512 x 16 waves loop over
#    the rows (r += nwave stays below 2^31); the four statistics are fp32 sums of per-block partials: the counts are integers
#    below 2^24 and stay exact.
# =====================================================================================================================
def test_cross_entropy():
    lib, chk, _, sp = _raw()
    rows, V, ld, eps_ls = (1 << 22) + 3, 337, 512, 0.1
    pad = V - 1
    case = f"ce rows={rows} V={V} ld={ld}"
    assert rows * ld > 1 << 31 and rows < 1 << 24
    g = LO.device_gen(rows + V)
    LG, TG = LO.big_operand((rows, ld), BF), LO.big_operand((rows,), I32)
    LO.fill_normal(LG.t, g, 2.0)
    LG.t[:, V:] = float("nan")                                              # the padding columns are never read
    LO.fill_randint(TG.t, g, 0, V)
    ST = KC.output(None, F32, torch.zeros(4))
    AM, LSE = LO.big_output((rows,), I32), LO.big_output((rows,), F32)
    chk(lib.mgx_smooth_ce_fwd(P(LG), P(TG), P(ST), P(AM), P(LSE), rows, V, ld, eps_ls, pad, sp()), case)
    sync()
    assert ST.bands_intact() and AM.bands_intact() and LSE.bands_intact(), case + ": the forward wrote outside stats / argmax / lse"
    blocks = LO.sample_blocks(rows, 8, (2 * ld,))
    assert LO.marks_inside(rows * 2 * ld) == list(LO.MARKS) and len(blocks) >= 3
    for lo, hi in blocks:
        lg, tg, c2 = LG.t[lo:hi].cpu(), TG.t[lo:hi].cpu(), f"{case} rows {lo}:{hi}"
        ref = T.smooth_ce_fwd(lg, tg, V, eps_ls, pad)
        Fl, _ = T.smooth_ce_fwd_floor(lg, tg, V, eps_ls, pad, ref)
        assert (AM.t[lo:hi].cpu().long() == ref[1]).all(), c2 + ": arg-max differs"
        check_floor("CE fwd", "CE", LSE.t[lo:hi], ref[0], Fl, c2 + " lse")
    chunks = LO.row_chunks(rows, (2 * ld,))
    n0 = chunks[0][1]
    Ac, Lc, sc = LO.big_output((n0,), I32), LO.big_output((n0,), F32), torch.zeros(4, device=DEV)
    lse_c = torch.empty_like(LSE.t)

    def fwd_chunk(lo, hi):
        Ac.refill(), Lc.refill()
        chk(lib.mgx_smooth_ce_fwd(LG.t[lo:hi].data_ptr(), TG.t[lo:hi].data_ptr(), sc.data_ptr(), P(Ac), P(Lc), hi - lo, V, ld, eps_ls, pad, sp()), case)
        lse_c[lo:hi] = Lc.t[:hi - lo]
        return Ac.t[:hi - lo]
    LO.compare_rows("CE fwd", AM.t, fwd_chunk, chunks, case + " argmax")
    LO.compare_rows("CE fwd", LSE.t, lambda lo, hi: lse_c[lo:hi], chunks, case + " lse")
    assert Ac.bands_intact() and Lc.bands_intact(), case
    del Ac, Lc, lse_c
    # the statistics: fp64 on the device over all rows, the floor of smooth_ce_fwd_floor on the same pieces
    e = T._f32(eps_ls)
    tot, terms, cnt, hits = (torch.zeros((), dtype=F64, device=DEV) for _ in range(4))
    cols = torch.arange(V, device=DEV)
    for lo in range(0, rows, 1 << 16):
        x, t = LG.t[lo:lo + (1 << 16), :V].double(), TG.t[lo:lo + (1 << 16)].long()
        mx = x.amax(-1)
        lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(-1))
        xt = x.gather(1, t[:, None])[:, 0]
        keep = t != pad
        tot += (lse - (1.0 - e) * xt - (e / V) * x.sum(-1))[keep].sum()
        terms += (lse.abs() + (1.0 - e) * xt.abs() + (e / V) * x.abs().sum(-1))[keep].sum()
        first = torch.where(x == mx[:, None], cols[None, :], V).amin(-1)   # the FIRST index of the maximum
        assert torch.equal(first, AM.t[lo:lo + (1 << 16)].long()), f"{case}: arg-max differs in rows {lo}.."
        cnt += keep.sum()
        hits += (first == t).sum()
    sk = ST.t.cpu()
    print(f"[CE] {case}: stats {sk.tolist()} reference loss sum {tot.item():.6f}")
    assert sk[1].item() == cnt.item() and sk[2].item() == hits.item() and sk[3].item() == rows, (case, sk.tolist(), cnt.item(), hits.item())
    tot = tot.cpu()
    check_floor("CE fwd", "CE", sk[:1], tot.reshape(1), (T.EPS32 * terms.cpu() + 2 * T.ulp32(tot)).reshape(1), case + " stats[0]")
    # ---- backward, from the lse and the count the forward kernel left ----
    DL = LO.big_output((rows, ld), BF)
    chk(lib.mgx_smooth_ce_bwd(P(LG), P(TG), P(ST), P(LSE), P(DL), rows, V, ld, eps_ls, pad, 1.0, None, sp()), case)
    sync()
    assert DL.bands_intact() and ST.bands_intact(), case + ": the backward wrote outside dlogits"
    for lo, hi in blocks:
        lg, tg, lk, c2 = LG.t[lo:hi].cpu(), TG.t[lo:hi].cpu(), LSE.t[lo:hi].cpu(), f"{case} rows {lo}:{hi}"
        rb = T.smooth_ce_bwd(lg, tg, float(sk[1]), lk, V, ld, eps_ls, pad, 1.0)
        check_floor("CE bwd", "CE", DL.t[lo:hi], rb, T.smooth_ce_bwd_floor(lg, tg, float(sk[1]), lk, V, ld, eps_ls, pad, 1.0, rb), c2 + " dlogits", 2.0 ** -8)
    for lo in range(0, rows, 1 << 20):
        dl = DL.t[lo:lo + (1 << 20)]
        assert (dl[:, V:] == 0).all() and (dl[TG.t[lo:lo + (1 << 20)] == pad] == 0).all(), case + ": padding columns / pad rows of dlogits are not 0"
    Dc = LO.big_output((n0, ld), BF)

    def bwd_chunk(lo, hi):
        Dc.refill()
        chk(lib.mgx_smooth_ce_bwd(LG.t[lo:hi].data_ptr(), TG.t[lo:hi].data_ptr(), P(ST), LSE.t[lo:hi].data_ptr(), P(Dc), hi - lo, V, ld, eps_ls, pad,
                                  1.0, None, sp()), case)
        return Dc.t[:hi - lo]
    LO.compare_rows("CE bwd", DL.t, bwd_chunk, chunks, case)
    assert Dc.bands_intact() and DL.bands_intact(), case
    del LG, TG, AM, LSE, DL, Dc


# =====================================================================================================================
# 4. embedding + PE and its gradient.  Read: the forward walks 8-element groups with a long index g, r = g / (d / 8), every address
#    (size_t) r * d + c; the backward's blocks scan token ranges r_lo .. r_hi (int, rows = 4.2e6) and gather dout + (size_t) r * d.
# =====================================================================================================================
def test_embedding():
    lib, chk, _, sp = _raw()
    from oracle import ref_cpu
    B, L, d, V = 2049, 2048, 512, 337
    rows, seed = B * L, 77
    case = f"embed B={B} L={L} d={d} V={V}"
    assert rows * d > 1 << 31
    g = LO.device_gen(rows)
    gc_ = KC.gen(V, d)
    table, pe = torch.randn(V, d, generator=gc_), ref_cpu.sinusoid_table(L, d).float()
    TB, PE = KC.operand(table), KC.operand(pe)
    TOK = LO.big_operand((rows,), I32)
    LO.fill_randint(TOK.t, g, 0, V - 1)                                     # token V - 1 never occurs
    OUT = LO.big_output((rows, d), BF)
    blocks = LO.sample_blocks(rows, 8, (2 * d,))
    assert LO.marks_inside(rows * 2 * d) == list(LO.MARKS) and len(blocks) == 4

    def sampled(p_drop):
        cfg = T.make_drop(p_drop, seed)
        for lo, hi in blocks:
            tok, mult = TOK.t[lo:hi].cpu(), ln_mult_cpu(cfg, lo, hi, d)
            per = pe[torch.arange(lo, hi) % L]                              # the block's own PE rows: train_ref indexes them from 0
            ref = T.embed_pe_fwd(tok, table, per, hi - lo, mult)
            check_floor("EMB fwd", "EMB", OUT.t[lo:hi], ref, T.embed_pe_fwd_floor(tok, table, per, hi - lo, mult, ref), f"{case} p={p_drop} rows {lo}:{hi}", 2.0 ** -8)
    chk(lib.mgx_embed_pe_fwd(P(TOK), P(TB), P(PE), P(OUT), B, L, d, V, 0.0, seed, sp()), case)
    sync()
    assert OUT.bands_intact(), case + ": the forward wrote outside out"
    sampled(0.0)
    chunks = LO.row_chunks(rows, (2 * d,), align=L)
    Oc = LO.big_output((chunks[0][1], d), BF)

    def chunk(lo, hi):
        Oc.refill()
        chk(lib.mgx_embed_pe_fwd(TOK.t[lo:hi].data_ptr(), P(TB), P(PE), P(Oc), (hi - lo) // L, L, d, V, 0.0, seed, sp()), case)
        return Oc.t[:hi - lo]
    LO.compare_rows("EMB fwd", OUT.t, chunk, chunks, case)
    assert Oc.bands_intact() and OUT.bands_intact(), case
    del Oc
    OUT.refill()                                                            # with dropout: the sampled blocks at the rows' own group indices
    chk(lib.mgx_embed_pe_fwd(P(TOK), P(TB), P(PE), P(OUT), B, L, d, V, 0.1, seed, sp()), case)
    sync()
    assert OUT.bands_intact(), case
    sampled(0.1)
    # ---- backward: dtable [V, d] += sqrt(d) sum_{r: tok[r] = v} mult[r] dout[r]; OUT's buffer serves as dout ----
    LO.fill_normal(OUT.t, g)
    for p_drop in (0.0, 0.1):
        cfg = T.make_drop(p_drop, seed)
        DT = KC.output(None, F32, torch.zeros(V, d))
        chk(lib.mgx_embed_bwd(P(TOK), P(OUT), P(DT), B, L, d, V, float(p_drop), seed, sp()), case)
        sync()
        assert DT.bands_intact(), case + ": the backward wrote outside dtable"
        upd, S = torch.zeros(V, d, dtype=F64, device=DEV), torch.zeros(V, d, dtype=F64, device=DEV)
        for lo in range(0, rows, 1 << 15):
            hi = min(rows, lo + (1 << 15))
            src = OUT.t[lo:hi].double()
            if p_drop > 0:
                src = src * LO.drop_mult_rows(cfg, lo, hi, d, DEV)
            upd.index_add_(0, TOK.t[lo:hi].long(), src)
            S.index_add_(0, TOK.t[lo:hi].long(), src.abs())
        tot, S = (upd * math.sqrt(d)).cpu(), (S * math.sqrt(d)).cpu()
        check_floor("EMB bwd", "EMB", DT.t, tot, T.EPS32 * S + T.ulp32(tot), f"{case} p={p_drop} dtable")
        assert (DT.t[V - 1] == 0).all() and (tot[V - 1] == 0).all(), "the row of a token that never occurs was touched"
    del TOK, OUT


# =====================================================================================================================
# 5. attention.  Read: every kernel takes (b, h) from blockIdx and forms its bases in size_t -- qkv_b = qkv + (size_t) b * L * 3d, the
#    statistics at ((size_t) b * heads + hd) * L, the dS tiles of a pair at ((size_t) b * heads + hd) * ntri * 1024 elements
#    (rel_attn_dkv32 / dkv64 / dq_lite / de_tiles) -- and adds 32-bit lane offsets that stay inside one pair (4.3 MB at L = 2048,
#    16.9 MB at L = 4096) or one batch row of qkv.  bwd_workspace() and batch_group() are size_t / double on the host; the plan
#    refuses grids past 65535 in y (16 x 127 = 2032 here).
# =====================================================================================================================
PROD, RECOMPUTE = 1 | 4 | 2 | 8, 1 | 4 | 32 | 16
ATTN_SHAPES = ((127, 2048, 512), (128, 2048, 512), (64, 4096, 256))
REF_L = 2048                                        # the fp64 reference holds Eg [L, L, 64]: 2.1 GB at L = 2048, 8.6 GB at L = 4096


def head_slice(t, b, hd, d, parts):
    """columns of head hd of batch row b of a [B, L, parts * d] tensor -> [1, L, parts * 64]"""
    return torch.cat([t[b:b + 1, :, p * d + hd * 64:p * d + (hd + 1) * 64] for p in range(parts)], -1)


class Attn:
    """one attention call through the raw ABI, inside bands; the workspace is exactly the size its query returns"""

    def __init__(self, B, L, d, M):
        self.lib, self.chk, _, self.sp = _raw()
        self.B, self.L, self.d, self.M, self.h = B, L, d, M, d // 64
        self.CTX, self.LSE, self.DQKV = LO.big_output((B, L, d), BF), LO.big_output((B, self.h, L), F32), LO.big_output((B, L, 3 * d), BF)
        self.nf, self.nb = self.lib.mgx_rel_attn_fwd_workspace(L), self.lib.mgx_rel_attn_bwd_workspace(B, L, d)
        self.WF, self.WB = LO.big_output((self.nf,), torch.uint8), LO.big_output((self.nb,), torch.uint8)
        self.DE = KC.output(None, F32, torch.zeros(M, 64))

    def fwd(self, qkv, E, n, case):
        self.CTX.refill(), self.LSE.refill()
        self.chk(self.lib.mgx_rel_attn_fwd(qkv.data_ptr(), P(E), None, P(self.CTX), P(self.LSE), P(self.WF), self.nf, n, self.L, self.d, self.M,
                                           self.sp()), case)
        sync()
        assert self.CTX.bands_intact() and self.LSE.bands_intact() and self.WF.bands_intact(), case + ": the forward wrote outside ctx / lse / its workspace"
        return self.CTX.t[:n], self.LSE.t[:n]

    def bwd(self, qkv, E, ctx, dctx, lse, n, parts, case):
        """-> dqkv of the n rows, dE [M, 64] fp64 of this call alone (accumulated into zeros)"""
        self.DQKV.refill()
        self.DE.t.zero_()
        need = self.lib.mgx_rel_attn_bwd_workspace(n, self.L, self.d)
        assert need <= self.nb
        self.chk(self.lib.mgx_rel_attn_bwd_parts(qkv.data_ptr(), P(E), None, ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), P(self.DQKV), P(self.DE),
                                                 P(self.WB), need, n, self.L, self.d, self.M, parts, self.sp()), case)
        sync()
        assert self.DQKV.bands_intact() and self.DE.bands_intact() and self.WB.bands_intact(), case + ": the backward wrote outside dqkv / dE / its workspace"
        return self.DQKV.t[:n], self.DE.t.double()


@pytest.mark.parametrize("B,L,d", ATTN_SHAPES, ids=("B127-groups-of-1", "B128-bench", "L4096"))
def test_attention(B, L, d):
    M, h = L, d // 64
    T_tiles = (L // 32) * (L // 32 + 1) // 2
    pair_bytes = T_tiles * 2048
    case = f"attn B={B} L={L} d={d}"
    assert B * h * pair_bytes > 1 << 32
    g = LO.device_gen(B + L + d)
    QKV, E, DCTX = LO.big_operand((B, L, 3 * d), BF), LO.big_operand((M, 64), BF), LO.big_operand((B, L, d), BF)
    LO.fill_normal(QKV.t, g, 0.8), LO.fill_normal(E.t, g, 0.5), LO.fill_normal(DCTX.t, g)
    big = Attn(B, L, d, M)
    assert big.nb > 1 << 32
    ctx, lse = big.fwd(QKV.t, E, B, case)
    ctx, lse = ctx.clone(), lse.clone()                                     # the backward is chained: it reads the kernel's own ctx and lse
    dq_prod, dE_prod = big.bwd(QKV.t, E, ctx, DCTX.t, lse, B, PROD, case)
    dq_prod = dq_prod.clone()
    pairs = [lo for lo, _ in LO.sample_blocks(B * h, 1, (pair_bytes,))]
    assert len(pairs) == 4 and pairs[1] * pair_bytes <= 1 << 31 < (pairs[1] + 1) * pair_bytes and pairs[2] * pair_bytes <= 1 << 32 < (pairs[2] + 1) * pair_bytes
    if L <= REF_L:                                                          # (a): train_ref's formulas as they stand, evaluated on the device
        for pair in pairs:
            b, hd = divmod(pair, h)
            c2 = f"{case} pair (b={b}, h={hd})"
            q1, c1, l1 = head_slice(QKV.t, b, hd, d, 3), head_slice(ctx, b, hd, d, 1), lse[b:b + 1, hd:hd + 1]
            with torch.device(DEV):                                         # (train_ref builds its index tensors where the default device is)
                ref = T.rel_attn_fwd(q1, E.t, None, 1, M)
                cb, lb, _ = T.attn_fwd_bounds(ref)
                fwd_ref = [t.cpu() for t in (ref.ctx, cb, ref.lse, lb)]
                del ref, cb, lb
                r = T.rel_attn_bwd(q1, E.t, None, c1, l1, head_slice(DCTX.t, b, hd, d, 1), 1, M)
                bd, _ = T.attn_bwd_bounds(r, B)
                want, bd = r.dqkv.cpu(), bd.cpu()
                del r
            check_bound("attn fwd ctx", c1, fwd_ref[0], fwd_ref[1], c2)
            check_bound("attn fwd lse", l1, fwd_ref[2], fwd_ref[3], c2)
            got = head_slice(dq_prod, b, hd, d, 3)
            for o, name in enumerate(("dq", "dk", "dv")):
                check_bound(f"attn bwd {name}", got[..., 64 * o:64 * o + 64], want[..., 64 * o:64 * o + 64], bd[..., 64 * o:64 * o + 64], c2)
        torch.cuda.empty_cache()
    dq_rec, dE_rec = big.bwd(QKV.t, E, ctx, DCTX.t, lse, B, RECOMPUTE, case)
    dq_rec = dq_rec.clone()
    assert torch.equal(LO.ibits(dq_prod[..., d:]), LO.ibits(dq_rec[..., d:])), case + ": the same dK/dV kernel on the same inputs"
    print(f"[attn] {case}: dE tiles vs recompute rel {LO.rel(dE_prod, dE_rec):.3g}, dq rel {LO.rel(dq_prod[..., :d], dq_rec[..., :d]):.3g}")
    assert dE_prod.abs().max() > 0 and LO.rel(dq_prod[..., :d], dq_rec[..., :d]) < 4e-3     # (tiles against recompute dE: test_gpu_fullsize's check, printed here)
    big_ws = big.nb
    del big
    torch.cuda.empty_cache()
    # (b): chunks of batch rows whose whole workspace (the dS tiles and the statistics before them) stays below 2^31 bytes
    lib = _raw()[0]
    chunks = LO.row_chunks(B, (lib.mgx_rel_attn_bwd_workspace(1, L, d), L * 3 * d * 2))
    assert len(chunks) >= 3
    small = Attn(chunks[0][1], L, d, M)
    assert small.nb < 1 << 31 and big_ws > 1 << 32
    ctx_c, lse_c = torch.empty_like(ctx), torch.empty_like(lse)
    dE_sum = {PROD: torch.zeros(M, 64, dtype=F64, device=DEV), RECOMPUTE: torch.zeros(M, 64, dtype=F64, device=DEV)}
    outs = {PROD: torch.empty_like(dq_prod), RECOMPUTE: torch.empty_like(dq_prod)}
    for lo, hi in chunks:
        c, l_ = small.fwd(QKV.t[lo:hi], E, hi - lo, case)
        ctx_c[lo:hi], lse_c[lo:hi] = c, l_
        for parts in (PROD, RECOMPUTE):
            dq, dE = small.bwd(QKV.t[lo:hi], E, ctx[lo:hi], DCTX.t[lo:hi], lse[lo:hi], hi - lo, parts, case)
            outs[parts][lo:hi] = dq
            dE_sum[parts] += dE
    LO.compare_rows("attn fwd", ctx, lambda lo, hi: ctx_c[lo:hi], chunks, case + " ctx")
    LO.compare_rows("attn fwd", lse, lambda lo, hi: lse_c[lo:hi], chunks, case + " lse")
    LO.compare_rows("attn bwd", dq_prod, lambda lo, hi: outs[PROD][lo:hi], chunks, case + " production parts")
    LO.compare_rows("attn bwd", dq_rec, lambda lo, hi: outs[RECOMPUTE][lo:hi], chunks, case + " recompute parts")
    for parts, dE_big in ((PROD, dE_prod), (RECOMPUTE, dE_rec)):
        r = LO.rel(dE_big, dE_sum[parts])
        KC._note(SEEN, "attn dE whole / chunks (bound 2e-5)", r / 2e-5, f"{case} parts={parts}", f"[attn dE] {case} parts={parts}: whole call vs sum of {len(chunks)} chunk calls rel {r:.3g}")
        assert r < 2e-5, (case, parts, r)
    del small, QKV, DCTX, E


def test_attention_weights():
    """mgx_rel_attn_weights, fp32 [B, h, L, L] = 4.43 GB into a zero-filled buffer; chunks are single batch rows"""
    lib, chk, _, sp = _raw()
    B, L, d = 33, 2048, 512
    M, h = L, d // 64
    case = f"weights B={B} L={L} d={d}"
    assert B * h * L * L * 4 > 1 << 32 and (B - 1) * h * L * L * 4 <= 1 << 32
    g = LO.device_gen(B + L)
    QKV, E = LO.big_operand((B, L, 3 * d), BF), LO.big_operand((M, 64), BF)
    LO.fill_normal(QKV.t, g, 0.8), LO.fill_normal(E.t, g, 0.5)
    a = Attn(B, L, d, M)
    _, lse = a.fwd(QKV.t, E, B, case)
    lse = lse.clone()
    nf = a.nf
    del a
    W, WS = LO.big_output((B, h, L, L), F32), LO.big_output((nf,), torch.uint8)
    W.t.zero_()
    chk(lib.mgx_rel_attn_weights(P(QKV), P(E), None, lse.data_ptr(), P(W), P(WS), nf, B, L, d, M, sp()), case)
    sync()
    assert W.bands_intact() and WS.bands_intact(), case + ": the call wrote outside weights / its workspace"
    pairs = [lo for lo, _ in LO.sample_blocks(B * h, 1, (L * L * 4,))]
    assert pairs == [0, 128, 256, B * h - 1]
    with torch.device(DEV):
        for pair in pairs:
            b, hd = divmod(pair, h)
            ref = T.rel_attn_fwd(head_slice(QKV.t, b, hd, d, 3), E.t.clone(), None, 1, M)
            lin = lse[b:b + 1, hd:hd + 1]
            want = T.attn_weights(ref, lin)
            check_bound("weights", W.t[b:b + 1, hd:hd + 1], want.cpu(), T.attn_weights_bound(ref, lin, want).cpu(), f"{case} pair (b={b}, h={hd})")
            del ref, want
    torch.cuda.empty_cache()
    Wc = LO.big_output((1, h, L, L), F32)

    def chunk(lo, hi):
        Wc.refill()
        Wc.t.zero_()
        chk(lib.mgx_rel_attn_weights(QKV.t[lo:hi].data_ptr(), P(E), None, lse[lo:hi].data_ptr(), P(Wc), P(WS), nf, 1, L, d, M, sp()), case)
        return Wc.t
    LO.compare_rows("weights", W.t, chunk, [(b, b + 1) for b in range(B)], case)
    assert Wc.bands_intact() and W.bands_intact(), case
    del W, Wc, QKV, E


# =====================================================================================================================
# 6. the decode cache.  Read (csrc/decode.hip, beam.hip): workgroup (b, h) streams kcache + ((size_t) b * heads + hd) * Lmax * 64,
#    rows at (size_t) j * 64; the reorder copies runs at ((size_t) r * heads + hd) * run_units 16-byte units.  520 x 8 workgroups and
#    128 x 8 both take one key split (decode_splits: >= 1024 workgroups), so a 128-row call computes a row exactly as the big one.
# =====================================================================================================================
def test_decode_cache_attention_and_beam_reorder():
    lib, chk, _, sp = _raw()
    B, Lmax, d, K = 520, 8192, 512, 8
    h, M = d // 64, Lmax
    row_bytes = h * Lmax * 128
    case = f"decode B={B} Lmax={Lmax} d={d}"
    assert B * row_bytes > 1 << 32 and lib.mgx_rel_attn_decode_splits(B, Lmax, d) == 1 == lib.mgx_rel_attn_decode_splits(128, Lmax, d)
    g = LO.device_gen(B + Lmax)
    KCA, VCA = LO.big_operand((B, h, Lmax, 64), BF), LO.big_operand((B, h, Lmax, 64), BF)
    LO.fill_normal(KCA.t, g), LO.fill_normal(VCA.t, g)
    QN, E = LO.big_operand((B, 3 * d), BF), LO.big_operand((M, 64), BF)
    LO.fill_normal(QN.t, g), LO.fill_normal(E.t, g, 0.3)
    pos = (Lmax - 1 - torch.arange(B, dtype=I32) % 61).to(DEV)              # per-row positions near Lmax
    k0 = KCA.t.clone()                                                      # the K cache before the call: rows other than t must not change
    CTX = LO.big_output((B, d), BF)
    chk(lib.mgx_rel_attn_decode(P(QN), P(KCA), P(VCA), P(E), pos.data_ptr(), 1, P(CTX), None, 0, B, Lmax, d, M, sp()), case)
    sync()
    assert CTX.bands_intact() and KCA.bands_intact() and VCA.bands_intact(), case + ": the call wrote outside ctx or a cache"
    bi = torch.arange(B, device=DEV)
    want_k = k0
    want_k[bi, :, pos.long()] = QN.t[:, d:2 * d].reshape(B, h, 64)
    assert torch.equal(LO.ibits(KCA.t), LO.ibits(want_k)), case + ": the K cache is not its old rows + k_t at row t"
    assert torch.equal(LO.ibits(VCA.t[bi, :, pos.long()]), LO.ibits(QN.t[:, 2 * d:].reshape(B, h, 64))), case + ": row t of the V cache is not v_t"
    del k0, want_k
    torch.cuda.empty_cache()
    blocks = LO.sample_blocks(B, 2, (row_bytes,))
    assert blocks == [(0, 2), (255, 257), (511, 513), (B - 2, B)]
    Ec = E.t.cpu()
    for lo, hi in blocks:
        for b in range(lo, hi):
            t = int(pos[b])
            q, Kb, Vb = QN.t[b, :d].reshape(h, 64).cpu(), KCA.t[b, :, :t + 1].cpu().double(), VCA.t[b, :, :t + 1].cpu().double()
            ref = D.rel_attn_decode(q, Kb, Vb, Ec, t)
            check_floor("decode attn", "DEC", CTX.t[b].reshape(h, 64), ref, D.attn_noise_floor(q, Kb, Vb, Ec, t, ref), f"{case} row {b} t={t}", 2.0 ** -8)
    # (b): caches of 128 rows copied out of the big ones (the last 8 rows as the tail of rows 392 .. 519: eight rows alone would take
    # eight key splits)
    Cc = LO.big_output((128, d), BF)

    def chunk(lo, hi):
        s = hi - 128
        kc, vc = KCA.t[s:hi].clone(), VCA.t[s:hi].clone()
        Cc.refill()
        chk(lib.mgx_rel_attn_decode(QN.t[s:hi].data_ptr(), kc.data_ptr(), vc.data_ptr(), P(E), pos[s:hi].data_ptr(), 1, P(Cc), None, 0, 128, Lmax, d, M,
                                    sp()), case)
        sync()
        return Cc.t[lo - s:]
    LO.compare_rows("decode attn", CTX.t, chunk, [(0, 128), (128, 256), (256, 384), (384, 512), (512, B)], case)
    assert Cc.bands_intact(), case
    # ---- beam reorder: slot r takes rows < n_r of its parent's cache, bit for bit; rows >= n_r of dst are not written ----
    R = B
    parent = torch.randint(0, K, (R,), generator=torch.Generator().manual_seed(3), dtype=I32).to(DEV)
    n_rows = (pos + 1 - (torch.arange(R, device=DEV) % 7 == 0).to(I32) * 3).contiguous()      # some slots a little shorter
    src_row = (torch.arange(R, device=DEV) // K * K + parent).long()
    DST = LO.big_output((R, h, Lmax, 64), BF)
    below = torch.arange(Lmax, device=DEV)[None, None, :, None]
    for name, SRC in (("K", KCA), ("V", VCA)):
        DST.refill()
        chk(lib.mgx_kv_beam_reorder(P(DST), P(SRC), parent.data_ptr(), n_rows.data_ptr(), R, K, h, Lmax, 128, sp()), case)
        sync()
        assert DST.bands_intact() and SRC.bands_intact(), case + ": the reorder wrote outside dst"
        for lo in range(0, R, 40):
            hi = min(R, lo + 40)
            want = torch.where(below < n_rows[lo:hi, None, None, None], LO.ibits(torch.index_select(SRC.t, 0, src_row[lo:hi])), 0x5A5A)
            assert torch.equal(LO.ibits(DST.t[lo:hi]), want.to(torch.int16)), f"{case}: reorder of the {name} cache, slots {lo}:{hi}"
        print(f"[reorder] {case} {name} cache: exact on all {R} slots")
    del KCA, VCA, DST, CTX, Cc

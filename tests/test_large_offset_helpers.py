"""The helpers of tests/test_gpu_large_offsets.py on small CPU tensors, with the marks scaled down to 256 and 512 bytes: the block
sampler, the chunker, and the comparison of a big call with its chunk calls, fed a reference output and the three faults a wrapped
or sign-extended offset would produce.  This is the evidence that the GPU tests would notice the bug they are written for; no kernel
is made to produce it."""
import pytest
import torch

import kernel_checks as KC
import large_offsets as LO
from oracle import train_ref as T

BF = torch.bfloat16
MARKS = (256, 512)


# ---- block sampler --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,block,row_bytes", ((100, 4, (8,)), (100, 4, (8, 16)), (40, 2, (16, 4)), (33, 8, (16,)), (64, 1, (8,)),
                                                  (65, 1, (8,)), (7, 16, (100,)), (1, 4, (1000,))))
def test_sampler_returns_first_last_and_one_block_per_mark_inside(rows, block, row_bytes):
    blocks = LO.sample_blocks(rows, block, row_bytes, MARKS)
    b = min(block, rows)
    assert blocks == sorted(set(blocks)) and all(hi - lo == b and 0 <= lo and hi <= rows for lo, hi in blocks)
    assert (0, b) in blocks and (rows - b, rows) in blocks
    inside = [(rb, m) for rb in row_bytes for m in MARKS if 0 < m < rows * rb]
    for rb, m in inside:
        holds = [(lo, hi) for lo, hi in blocks if lo * rb <= m < hi * rb]
        assert holds, (rb, m, blocks)
        if b >= 2:                                  # bytes of the tensor on both sides of the mark
            assert any(lo * rb < m for lo, hi in holds)
    assert len(blocks) <= 2 + len(inside)           # nothing for a mark outside the tensor


def test_sampler_returns_nothing_for_marks_outside_the_tensor():
    assert LO.sample_blocks(31, 4, (8,), MARKS) == [(0, 4), (27, 31)]            # 248 bytes: below both marks
    assert LO.sample_blocks(32, 4, (8,), MARKS) == [(0, 4), (28, 32)]            # 256 bytes: the mark is the end, not inside
    assert LO.sample_blocks(33, 4, (8,), MARKS) == [(0, 4), (29, 33)]            # the block that holds byte 256 is the last one
    assert LO.sample_blocks(64, 4, (8,), MARKS) == [(0, 4), (30, 34), (60, 64)]  # 512 bytes: only the first mark is inside
    assert LO.sample_blocks(100, 4, (8,), MARKS) == [(0, 4), (30, 34), (62, 66), (96, 100)]
    assert LO.marks_inside(1 << 32) == [1 << 31] and LO.marks_inside((1 << 32) + 1) == [1 << 31, 1 << 32] and LO.marks_inside(1 << 31) == []


def test_sampler_names_the_attention_pairs_of_the_gpu_cases():
    """one (b,h) pair per block: the pair whose dS tiles hold byte 2^31 and the one that holds byte 2^32"""
    pair = 2080 * 2048                              # L = 2048: 64 * 65 / 2 tiles of 2 KB
    assert LO.sample_blocks(127 * 8, 1, (pair,)) == [(0, 1), (504, 505), (1008, 1009), (1015, 1016)]
    assert LO.sample_blocks(128 * 8, 1, (pair,)) == [(0, 1), (504, 505), (1008, 1009), (1023, 1024)]
    assert LO.sample_blocks(64 * 4, 1, (8256 * 2048,)) == [(0, 1), (127, 128), (254, 255), (255, 256)]
    assert LO.sample_blocks(126 * 8, 1, (pair,)) == [(0, 1), (504, 505), (1007, 1008)]      # B = 126: 4.29e9 bytes, below 2^32


# ---- chunker --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,row_bytes,align,max_rows", ((100, (8,), 1, None), (100, (8, 16), 1, None), (100, (8, 16), 4, None),
                                                           (1000, (2, 6), 8, 16), (5, (8,), 1, None), (96, (8,), 16, None)))
def test_chunks_tile_the_rows_and_stay_below_the_first_mark(rows, row_bytes, align, max_rows):
    chunks = LO.row_chunks(rows, row_bytes, MARKS[0], align, max_rows)
    assert chunks[0][0] == 0 and chunks[-1][1] == rows
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(hi > lo for lo, hi in chunks)
    for lo, hi in chunks:
        assert all((hi - lo) * rb < MARKS[0] for rb in row_bytes)
        assert max_rows is None or hi - lo <= max_rows
    assert all((hi - lo) % align == 0 for lo, hi in chunks[:-1]) and all(lo % align == 0 for lo, _ in chunks)


def test_chunks_of_the_gemm_case_are_whole_tiles_below_2_31_bytes():
    chunks = LO.row_chunks((1 << 21) + 256, (1024, 2048), align=256)
    assert chunks == [(0, 1048320), (1048320, 2096640), (2096640, 2097408)]
    with pytest.raises(AssertionError):
        LO.row_chunks(10, (300,), MARKS[0], align=1)


# ---- comparer -------------------------------------------------------------------------------------------------------------------
ROWS, COLS = 96, 8                                  # bf16 rows of 16 bytes: the marks are at rows 16 and 32


def reference_output():
    a, w = T.gemm_operands("gauss", ROWS, COLS, 64, seed=3)
    return T.bf16_round(T.linear_fwd(a, w)[0]).to(BF)


def compare(big, ref):
    chunks = LO.row_chunks(ROWS, (2 * COLS,), MARKS[0])
    assert len(chunks) > 6 and all((hi - lo) * 2 * COLS < MARKS[0] for lo, hi in chunks)
    LO.compare_rows("helper", big, lambda lo, hi: ref[lo:hi], chunks, "cpu")


def test_comparer_passes_on_the_reference():
    ref = reference_output()
    assert len({tuple(r.tolist()) for r in KC.bits16(ref)}) == ROWS          # no two rows alike: the data has no period
    compare(ref.clone(), ref)


@pytest.mark.parametrize("mark", MARKS)
def test_comparer_fails_on_the_wrap(mark):
    """the rows past a mark hold what belongs at (offset mod mark): a store whose offset lost its upper bits landed on the earlier
    row, and a load read it"""
    ref = reference_output()
    big = ref.clone()
    first = mark // (2 * COLS)
    idx = torch.arange(first, ROWS)
    big[idx] = ref[(idx * 2 * COLS % mark) // (2 * COLS)]
    with pytest.raises(AssertionError, match=rf"rows \[{first}, "):
        compare(big, ref)


def test_comparer_fails_on_one_unwritten_row_the_sampler_did_not_pick():
    ref = reference_output()
    sampled = LO.sample_blocks(ROWS, 4, (2 * COLS,), MARKS)
    row = 50
    assert not any(lo <= row < hi for lo, hi in sampled)
    out = LO.big_output((ROWS, COLS), BF, device="cpu")
    assert LO.pattern_rows(out.t).numel() == ROWS and out.t.float().abs().min() > 1e16
    out.t.copy_(ref)
    out.t[row].view(torch.uint8).fill_(KC.PATTERN[0])
    assert LO.pattern_rows(out.t).tolist() == [row] and out.bands_intact()
    for lo, hi in sampled:                          # check (a) alone passes: this is what check (b) is for
        KC.check_equal("helper", out.t[lo:hi], ref[lo:hi].double(), "sampled block")
    with pytest.raises(AssertionError, match=r"rows \[50\]"):
        compare(out.t, ref)


@pytest.mark.parametrize("mark", MARKS)
def test_comparer_fails_on_two_rows_swapped_across_a_mark(mark):
    ref = reference_output()
    big = ref.clone()
    r = mark // (2 * COLS)
    big[[r - 1, r]] = ref[[r, r - 1]]
    with pytest.raises(AssertionError, match=rf"rows \[{r - 1}"):
        compare(big, ref)


def test_comparer_insists_that_the_chunks_cover_every_row():
    ref = reference_output()
    with pytest.raises(AssertionError, match="cover"):
        LO.compare_rows("helper", ref, lambda lo, hi: ref[lo:hi], [(0, 40), (40, 80)], "cpu")
    with pytest.raises(AssertionError, match="tile"):
        LO.compare_rows("helper", ref, lambda lo, hi: ref[lo:hi], [(0, 40), (48, 96)], "cpu")


# ---- buffers and data -----------------------------------------------------------------------------------------------------------
def test_banded_buffers_on_the_device_match_kernel_checks_banded():
    out = LO.big_output((5, 8), torch.float32, device="cpu")
    assert out.t.shape == (5, 8) and out.buf.numel() == 40 + 2 * KC.BAND // 4 and out.bands_intact()
    assert (out.buf.view(torch.uint8) == 0x5A).all()
    out.buf[0] = 1.0
    assert not out.bands_intact()
    op = LO.big_operand((3, 8), BF, device="cpu")
    assert torch.isnan(op.buf.float()).all() and (LO.big_operand((4,), torch.int32, device="cpu").buf == -1).all()
    op.t.zero_()
    assert op.bands_intact() and torch.isnan(op.buf[:KC.BAND // 2].float()).all()


def test_fills_draw_one_stream_in_pieces(monkeypatch):
    monkeypatch.setattr(LO, "DRAW", 7)
    g = LO.device_gen(5, "cpu")
    a = LO.fill_normal(torch.empty(4, 5, dtype=BF), g, 0.5, 1.0)
    assert torch.isfinite(a.float()).all() and len(set(a.flatten().tolist())) > 10
    g2 = LO.device_gen(5, "cpu")
    pieces = torch.cat([torch.randn(n, generator=g2) for n in (7, 7, 6)])
    assert torch.equal(a.flatten(), (pieces * 0.5 + 1.0).to(BF))
    t = LO.fill_randint(torch.empty(30, dtype=torch.int32), LO.device_gen(1, "cpu"), 3, 9)
    assert t.min() >= 3 and t.max() < 9 and len(set(t.tolist())) > 3


@pytest.mark.parametrize("p,seed", ((0.1, 7), (0.5, (1 << 33) + 9), (0.0, 3)))
def test_device_dropout_multipliers_are_the_oracles(p, seed):
    rows, d = 40, 24
    want = T.drop_mult(p, seed, rows * d).reshape(rows, d).double()
    cfg = T.make_drop(p, seed)
    assert torch.equal(LO.drop_mult_rows(cfg, 0, rows, d, "cpu"), want)
    assert torch.equal(LO.drop_mult_rows(cfg, 11, 29, d, "cpu"), want[11:29])
    if p > 0:                                       # group indices are taken mod 2^32, as the kernels' uint32 cast does
        far = (1 << 32) // (d // 8)
        assert torch.equal(LO.drop_mult_rows(cfg, far * 3 + 11, far * 3 + 29, d, "cpu")[:, :8],
                           torch.from_numpy(T.drop_mult8(cfg, [(r * 3) & 0xFFFFFFFF for r in range(far * 3 + 11, far * 3 + 29)])).double())


def test_ulp_and_rel_match_their_cpu_twins():
    x = torch.tensor([0.0, 1.0, -3.5, 1e-30, 2.5e7, 1e39], dtype=torch.float64)
    assert torch.equal(LO.ulp32(x), T.ulp32(x))
    a, b = torch.randn(50, generator=KC.gen(1)), torch.randn(50, generator=KC.gen(2))
    assert abs(LO.rel(a, b) - KC.rel(a, b)) < 1e-6

"""Helpers of tests/test_gpu_large_offsets.py, which runs the kernels at shapes whose byte offsets pass 2^31 and 2^32: which row
blocks to check against fp64 (sample_blocks), how to cut the rows into calls that stay below the first mark (row_chunks), the
row-by-row comparison of the big call with those calls (compare_rows), buffers inside guard bands that are built on the device
(BigBanded; kernel_checks.Banded copies a CPU tensor of the whole size), and seeded device fills without a period.  The marks are
parameters, so tests/test_large_offset_helpers.py runs all of it on small CPU tensors.  Imported by basename, like kernel_checks."""
import math

import torch

import kernel_checks as KC

MARKS = (1 << 31, 1 << 32)                          # byte offsets: the largest positive int32 + 1, the largest uint32 + 1
DRAW = 1 << 26                                      # elements per random draw
M32 = 0xFFFFFFFF


# ---- which rows -----------------------------------------------------------------------------------------------------------------
def marks_inside(nbytes, marks=MARKS):
    """the marks that lie strictly inside a tensor of nbytes bytes"""
    return [m for m in marks if 0 < m < nbytes]


def sample_blocks(rows, block, row_bytes, marks=MARKS):
    """the blocks of `block` consecutive rows to check against fp64: the first, the last, and for every operand or output (one
    entry of row_bytes each: its bytes per row) and every mark inside it one block that holds the byte at the mark -- with bytes
    of the tensor before and after the mark when block >= 2.  A mark outside a tensor gives no block.  -> sorted [(lo, hi)]"""
    assert rows > 0 and block > 0
    block = min(block, rows)
    out = {(0, block), (rows - block, rows)}
    for rb in row_bytes:
        for m in marks_inside(rows * rb, marks):
            r = m // rb                             # the row that holds byte m
            lo = min(max(r - block // 2, 0), rows - block)
            assert lo * rb <= m < (lo + block) * rb and (block < 2 or rows < 2 or lo * rb < m)
            out.add((lo, lo + block))
    return sorted(out)


def row_chunks(rows, row_bytes, mark=MARKS[0], align=1, max_rows=None):
    """[(lo, hi)] that tile 0..rows exactly, every chunk below `mark` bytes in every operand (row_bytes: bytes per row of each) and a
    multiple of `align` rows (the last one aside); max_rows caps a chunk further (memory)"""
    per = (mark - 1) // max(row_bytes)
    if max_rows is not None:
        per = min(per, max_rows)
    per = per // align * align
    assert per > 0, "one aligned group of rows does not fit below the mark"
    return [(lo, min(lo + per, rows)) for lo in range(0, rows, per)]


# ---- every row, bit for bit -----------------------------------------------------------------------------------------------------
def ibits(t):
    """the tensor's bits as integers of its width, on the device it lives on (kernel_checks.bits moves them to the CPU)"""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def compare_rows(fam, big, chunk_out, chunks, case):
    """rows lo..hi of `big` equal chunk_out(lo, hi) -- the output of the call on those rows alone -- bit for bit, for every chunk,
    and the chunks tile the rows of `big`.  The comparison runs where the tensors live; the rows that differ go through
    kernel_checks.check_equal, which names the elements"""
    at = 0
    for lo, hi in chunks:
        assert lo == at and hi > lo, (fam, case, "the chunks do not tile the rows", lo, hi, at)
        at = hi
        got, want = ibits(big[lo:hi]), ibits(chunk_out(lo, hi))
        assert got.shape == want.shape, (fam, case, got.shape, want.shape)
        if torch.equal(got, want):
            continue
        bad = torch.nonzero((got != want).reshape(hi - lo, -1).any(1)).reshape(-1)[:4]
        KC.check_equal(fam, got[bad].cpu(), want[bad].cpu().to(torch.float64), f"{case} rows {[lo + int(i) for i in bad]} of the big call against chunk {lo}:{hi}")
        raise AssertionError((fam, case, "rows differ", lo, hi))
    assert at == big.shape[0], (fam, case, "the chunks do not cover every row", at, big.shape[0])
    print(f"[{fam}] {case}: every row equals its chunk call, {len(chunks)} chunks")


# ---- buffers --------------------------------------------------------------------------------------------------------------------
class BigBanded(KC.Banded):
    """kernel_checks.Banded without the CPU tensor: an uninitialised interior of `shape` between two bands, the whole allocation
    filled with one byte -- 0x5A for an output (an unwritten element fails: 1.5e16 in bf16, 1.5e16 in fp32), 0xFF for an operand
    (NaN in bf16 and fp32, -1 in int32) whose interior the test then fills"""

    def __init__(self, shape, dtype, fill=KC.PATTERN, band=KC.BAND, device="cuda:0"):
        es = torch.empty((), dtype=dtype).element_size()
        assert band % es == 0
        self.band, self.lead, self.n, self.fill = band, band // es, math.prod(shape), fill
        self.buf = torch.empty(self.n + 2 * self.lead, dtype=dtype, device=device)
        self.refill()
        self.t = self.buf[self.lead:self.lead + self.n].view(shape)
        assert self.t.data_ptr() - self.buf.data_ptr() == band
        self.bands = self._bands()

    def refill(self):
        self.buf.view(torch.uint8).fill_(self.fill[0])


def big_output(shape, dtype, device="cuda:0"):
    return BigBanded(shape, dtype, KC.PATTERN, device=device)


def big_operand(shape, dtype, device="cuda:0"):
    return BigBanded(shape, dtype, b"\xff", device=device)


def pattern_rows(t):
    """rows of t that still hold the 0x5A pattern in every element (an output row no workgroup wrote)"""
    b = t.reshape(t.shape[0], -1).contiguous().view(torch.uint8)
    return torch.nonzero((b == KC.PATTERN[0]).all(1)).reshape(-1)


# ---- data -----------------------------------------------------------------------------------------------------------------------
def fill_normal(t, g, scale=1.0, shift=0.0):
    """t (contiguous, any float type) <- shift + scale * N(0, 1) from the generator g of t's device, at most DRAW elements per draw,
    written straight into slices of t: one stream of numbers, no period"""
    flat = t.view(-1)
    for lo in range(0, flat.numel(), DRAW):
        n = min(DRAW, flat.numel() - lo)
        r = torch.randn(n, generator=g, device=t.device, dtype=torch.float32)
        flat[lo:lo + n] = r * scale + shift if (scale != 1.0 or shift != 0.0) else r
    return t


def fill_randint(t, g, lo, hi):
    """t (contiguous, integer) <- uniform integers of [lo, hi), in draws of at most DRAW"""
    flat = t.view(-1)
    for at in range(0, flat.numel(), DRAW):
        n = min(DRAW, flat.numel() - at)
        flat[at:at + n] = torch.randint(lo, hi, (n,), generator=g, device=t.device, dtype=torch.int64)
    return t


def device_gen(seed, device="cuda:0"):
    return torch.Generator(device=device).manual_seed(seed)


# ---- the dropout multipliers on the device: twin of oracle/train_ref.py hash32 / drop_mult8 ---------------------------------------
def _hash32(x):
    x = x & M32                                     # int64 holding a uint32; products wrap modulo 2^64, the low 32 bits are right
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def drop_mult_rows(cfg, lo, hi, d, device, dtype=torch.float64):
    """multipliers of rows lo..hi of a [rows, d] buffer (element index = r d + c, groups of 8, taken mod 2^32) -> [hi - lo, d];
    cfg = train_ref.make_drop(p, seed); all ones for p = 0"""
    thr, mix, scale = cfg
    if thr == 0:
        return torch.ones(hi - lo, d, dtype=dtype, device=device)
    g = (torch.arange(lo * (d // 8), hi * (d // 8), dtype=torch.int64, device=device)) & M32
    out = torch.empty(g.numel(), 8, dtype=dtype, device=device)
    for k in range(4):
        r = _hash32(((g * 4 + k) & M32) ^ int(mix))
        out[:, 2 * k] = torch.where((r & 0xFFFF) < thr, 0.0, float(scale))
        out[:, 2 * k + 1] = torch.where((r >> 16) < thr, 0.0, float(scale))
    return out.reshape(hi - lo, d)


def ulp32(x):
    """train_ref.ulp32 on the tensor's own device"""
    a = torch.clamp(x.to(torch.float64).abs(), max=1e38).to(torch.float32)
    return torch.nextafter(a, torch.full_like(a, float("inf"))).to(torch.float64) - a.to(torch.float64)


def rel(a, b):
    """|a - b| / |b| in fp64 on the tensors' device (kernel_checks.rel computes on the CPU in fp32)"""
    a, b = a.to(torch.float64).flatten(), b.to(torch.float64).flatten()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()

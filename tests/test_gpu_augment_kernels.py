"""mgx_crop_augment (ABI 29) against the sequential numpy restatement of its header contract (tests/augment_ref.py).  All of it
is integer work, so every comparison is exact; every operand and output sits in guard bands, and every input is compared with
what was uploaded after the call.

T = 1024 is the kernel's source tile (256 threads x 4 tokens each, csrc/augment.hip): n runs over 1, 2, T - 1, T, T + 1 and
2 T + 3, so that without a stretch the source ends just before, at and just after a tile boundary and spans three tiles, and
with one (2 n source tokens) both scans carry across up to five tiles.  (n = 1 with y given leaves x and y without a column; it
is run with y NULL only.)"""
import numpy as np
import pytest
import torch

import augment_ref
import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

T = 1024
V, TS0, N_TS, PAD = 309, 208, 100, 308                       # the MIDI-like vocabulary with its pad id
QS = [500, 777, 950, 1000, 1005, 1050, 1999, 2000]
KINDS = ["random", "time only", "1-unit shifts at q=500", "n_ts-unit shifts at q=2000", "n_ts-unit shifts at q=1005"]
INT32_MAX = 2 ** 31 - 1


def banded(a, dtype):
    t = torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


def piece(kind, length, rng):
    """-> (ids, q) of one row's piece"""
    if kind == 0:                                             # every kind of id, some at and beyond V (the table leaves them)
        return rng.integers(0, V + 4, length), int(rng.choice(QS))
    if kind == 1:
        return rng.integers(TS0, TS0 + N_TS, length), int(rng.choice([777, 1337]))
    if kind == 2:
        return np.full(length, TS0), 500                       # two tokens per emitted id: the tight case of the 2 n bound
    if kind == 3:
        return np.full(length, TS0 + N_TS - 1), 2000           # every id doubles
    return np.full(length, TS0 + N_TS - 1), 1005               # ids that split in two: n_ts units and a remainder


def run(corpus, start, avail, n, *, perm=None, shift=None, q=None, ts0=TS0, n_ts=N_TS, time_major=False, with_y=True, case=""):
    """one launch inside guard bands against the reference; returns (x, n_out) of the reference"""
    B = len(start)
    cols = n - 1 if with_y else n
    shape = (cols, B) if time_major else (B, cols)
    c = banded(np.asarray(corpus).astype(np.uint16).view(np.int16), torch.int16)
    ins = {"start": banded(start, torch.int64), "avail": banded(avail, torch.int32)}
    if perm is not None:
        ins["perm"], ins["shift"] = banded(perm, torch.int32), banded(shift, torch.int32)
    if q is not None:
        ins["q"] = banded(q, torch.int32)
    x, y = KC.output(shape, torch.int32), KC.output(shape, torch.int32) if with_y else None
    n_out = KC.output((B,), torch.int32)
    before = {k: v.t.cpu().clone() for k, v in ins.items()}
    KC.ops().crop_augment(c.t, ins["start"].t, ins["avail"].t, x.t, None if y is None else y.t, PAD,
                          perm=None if perm is None else ins["perm"].t, shift_row=None if perm is None else ins["shift"].t,
                          stretch_q=None if q is None else ins["q"].t, ts0=ts0, n_ts=n_ts, n_out=n_out.t, time_major=time_major)
    torch.cuda.synchronize()
    rx, ry, rn = augment_ref.crop_augment(corpus, start, avail, n, PAD, perm=None if perm is None else np.asarray(perm),
                                          shift_row=shift, stretch_q=q, ts0=ts0, n_ts=n_ts, with_y=with_y)
    lay = (lambda a: a.T) if time_major else (lambda a: a)
    KC.check_equal("crop x", x.t, torch.from_numpy(np.ascontiguousarray(lay(rx))), case)
    if with_y:
        KC.check_equal("crop y", y.t, torch.from_numpy(np.ascontiguousarray(lay(ry))), case)
    KC.check_equal("crop n_out", n_out.t, torch.from_numpy(rn), case)
    for name, b in list(ins.items()) + [("corpus", c), ("x", x), ("n_out", n_out)] + ([("y", y)] if with_y else []):
        assert b.bands_intact(), (case, name)
    for name, b in ins.items():                               # the inputs are read only
        assert torch.equal(b.t.cpu(), before[name]), (case, name)
    assert torch.equal(c.t.cpu().view(torch.int16), torch.from_numpy(np.asarray(corpus).astype(np.uint16).view(np.int16))), case
    return rx, rn


def rows_of(kinds, n, rng):
    """a corpus of one piece per row, long enough for 2 n source tokens after a random start"""
    pieces, qs, start, avail, at = [], [], [], [], 0
    for kind in kinds:
        off = int(rng.integers(0, 7))
        ids, q = piece(kind, 2 * n + off + int(rng.integers(0, 5)), rng)
        pieces.append(ids)
        qs.append(q)
        start.append(at + off)
        avail.append(len(ids) - off)
        at += len(ids)
    return np.concatenate(pieces), np.array(start), np.array(avail), np.array(qs)


SHAPES = [(n, B, tm, wy) for n in (1, 2, T - 1, T, T + 1, 2 * T + 3) for B in (1, 5) for tm in (False, True) for wy in (True, False)
          if not (n == 1 and wy)]


@pytest.mark.parametrize("n,B,time_major,with_y", SHAPES)
def test_against_the_reference(n, B, time_major, with_y):
    """B = 5: one row of every kind in one launch; B = 1: every kind in a launch of its own.  Each with and without the stretch
    and the table"""
    rng = np.random.default_rng(n * 100 + B * 10 + time_major * 2 + with_y)
    perm = rng.integers(0, V + 50, (3, V))                    # any values: the kernel looks up, it does not interpret
    for kinds in ([list(range(5))] if B == 5 else [[k] for k in range(5)]):
        corpus, start, avail, qs = rows_of(kinds, n, rng)
        shift = rng.integers(0, 3, B)
        for stretch in (True, False):
            for table in (True, False):
                case = f"n={n} B={B} time_major={time_major} y={with_y} kinds={kinds} stretch={stretch} table={table}"
                rx, rn = run(corpus, start, avail, n, perm=perm if table else None, shift=shift if table else None,
                             q=qs if stretch else None, time_major=time_major, with_y=with_y, case=case)
                assert (rn == n).all(), case                  # 2 n source tokens always suffice (q >= 500)


@pytest.mark.parametrize("n", [2, T + 1])
def test_without_augmentation_the_output_is_the_corpus_slice(n):
    rng = np.random.default_rng(n)
    corpus = rng.integers(0, 65536, 4 * n + 9)                # all 16 bits
    start = np.array([0, 5, 3 * n + 9, n + 1])
    avail = len(corpus) - start
    c = torch.from_numpy(corpus.astype(np.uint16).view(np.int16)).cuda()
    x = torch.empty(4, n - 1, dtype=torch.int32, device="cuda:0")
    y = torch.empty_like(x)
    KC.ops().crop_augment(c, torch.from_numpy(start).cuda(), torch.from_numpy(avail).int().cuda(), x, y, PAD)
    torch.cuda.synchronize()
    want = np.stack([corpus[s:s + n] for s in start])
    KC.check_equal("plain x", x, torch.from_numpy(want[:, :-1]), f"n={n}")
    KC.check_equal("plain y", y, torch.from_numpy(want[:, 1:]), f"n={n}")


@pytest.mark.parametrize("stretch", [False, True])
@pytest.mark.parametrize("n", [5, T + 1])
def test_short_and_clamped_sources(n, stretch):
    """rows whose source ends early -- by avail, by the end of the corpus (avail claims more: the clamp is what protects the
    read), empty ones (negative start, negative avail, start at and beyond corpus_len) -- end in pad_token, n_out says where; a
    shift_row outside the table and a q outside 500 .. 2000 leave the ids and the time as they are"""
    rng = np.random.default_rng(n + stretch)
    N = 3 * n + 2
    tail = min(40, N // 2)                                    # the corpus ends in time ids: the short rows at its end stretch
    corpus = np.concatenate([rng.integers(0, V + 4, N - tail), rng.integers(TS0, TS0 + N_TS, tail)])
    start = np.array([0, 3, N - 3, N - 1, N - n, -1, 4, N, N + 5, 2 ** 40, 1, 2, 7, 8, 9, 6])
    avail = np.array([n // 2, 1, INT32_MAX, INT32_MAX, 2 * n, 10, -1, 5, 5, 5, 0, N, N, N, N, N])
    B = len(start)
    shift = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, -1, 3, INT32_MAX, -INT32_MAX - 1, 2])
    q = np.array([500, 2000, 1005, 500, 600, 700, 800, 900, 1000, 1100, 1200, 0, 499, 2001, -5, INT32_MAX])
    perm = rng.integers(0, V, (3, V))
    for time_major in (False, True):
        case = f"n={n} stretch={stretch} time_major={time_major}"
        rx, rn = run(corpus, start, avail, n, perm=perm, shift=shift, q=q if stretch else None, time_major=time_major, case=case)
        assert rn[5:11].tolist() == [0] * 6 and (rx[5:11] == PAD).all(), case
        assert rn[1] >= 1 and rn[2] <= 3 * 2 and rn[3] <= 2 and rn[0] < n, case
        assert (rx[0, rn[0]:] == PAD).all() and (rn[11:] == n).all(), case
    # the rows with a q outside the range are the rows of q = 1000, the rows with a shift outside the table those without one
    if stretch:
        rx2, _, _ = augment_ref.crop_augment(corpus, start, avail, n, PAD, perm=perm, shift_row=shift, stretch_q=np.full(B, 1000),
                                          ts0=TS0, n_ts=N_TS)
        assert (rx2[11:] == rx[11:]).all()
    else:
        assert (rx[12] == corpus[7:7 + n - 1]).all() and (rx[13] == corpus[8:8 + n - 1]).all()


def test_other_time_runs():
    """a run of 7 ids from id 3 (deltas up to 14 units split into ids of 7 and a remainder), and a run of one id"""
    rng = np.random.default_rng(5)
    n = 300
    for ts0, n_ts in ((3, 7), (0, 1), (65535, 1)):
        lo = 65520 if ts0 > 1000 else 0
        corpus = rng.integers(lo, lo + 16, 5 * 2 * n)
        start = np.arange(5) * 2 * n
        avail = np.full(5, 2 * n)
        run(corpus, start, avail, n, q=np.array([500, 999, 1001, 1500, 2000]), ts0=ts0, n_ts=n_ts, case=f"run ({ts0}, {n_ts})")


def test_from_a_captured_graph():
    """the launch is captured once and replayed twice, the per-row arrays rewritten in between: it follows them"""
    rng = np.random.default_rng(11)
    n, B = T + 1, 5
    corpus, start, avail, qs = rows_of([0, 1, 2, 3, 4], n, rng)
    perm = rng.integers(0, V, (3, V))
    dev = lambda a, dt: torch.as_tensor(np.asarray(a)).to(dt).cuda()  # noqa: E731
    c = dev(corpus.astype(np.uint16).view(np.int16), torch.int16)
    st, av, sh, q, pm = dev(start, torch.int64), dev(avail, torch.int32), dev(np.zeros(B), torch.int32), dev(qs, torch.int32), dev(perm, torch.int32)
    x = torch.zeros(B, n - 1, dtype=torch.int32, device="cuda:0")
    y, n_out = torch.zeros_like(x), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # a first launch outside the capture (module load)
        KC.ops().crop_augment(c, st, av, x, y, PAD, perm=pm, shift_row=sh, stretch_q=q, ts0=TS0, n_ts=N_TS, n_out=n_out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        KC.ops().crop_augment(c, st, av, x, y, PAD, perm=pm, shift_row=sh, stretch_q=q, ts0=TS0, n_ts=N_TS, n_out=n_out)
    for rep in range(2):
        shift = rng.integers(0, 3, B)
        q_now = rng.permutation(qs)
        start_now = start + rng.integers(0, 3, B)
        sh.copy_(dev(shift, torch.int32)); q.copy_(dev(q_now, torch.int32)); st.copy_(dev(start_now, torch.int64))
        x.fill_(-1); y.fill_(-1); n_out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        rx, ry, rn = augment_ref.crop_augment(corpus, start_now, avail, n, PAD, perm=perm, shift_row=shift, stretch_q=q_now,
                                              ts0=TS0, n_ts=N_TS)
        KC.check_equal("graph x", x, torch.from_numpy(rx), f"replay {rep}")
        KC.check_equal("graph y", y, torch.from_numpy(ry), f"replay {rep}")
        KC.check_equal("graph n_out", n_out, torch.from_numpy(rn), f"replay {rep}")


def test_refusals():
    o = KC.ops()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda:0")  # noqa: E731
    c = torch.zeros(64, dtype=torch.int16, device="cuda:0")
    st = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError, match="corpus"):
        o.crop_augment(i32(64), st, i32(2), i32(2, 4), None, PAD)
    with pytest.raises(ValueError, match="start"):
        o.crop_augment(c, i32(2), i32(2), i32(2, 4), None, PAD)
    with pytest.raises(ValueError, match="avail"):
        o.crop_augment(c, st, i32(3), i32(2, 4), None, PAD)
    with pytest.raises(ValueError, match="y must be"):
        o.crop_augment(c, st, i32(2), i32(2, 4), i32(2, 5), PAD)
    with pytest.raises(ValueError, match="go together"):
        o.crop_augment(c, st, i32(2), i32(2, 4), None, PAD, perm=i32(1, 8))
    with pytest.raises(ValueError, match="time run"):
        o.crop_augment(c, st, i32(2), i32(2, 4), None, PAD, stretch_q=i32(2), ts0=0, n_ts=0)
    with pytest.raises(ValueError, match="x must"):
        o.crop_augment(c, st, i32(2), torch.zeros(2, 4, device="cuda:0"), None, PAD)
    lib, check, ptr, stream = KC.raw()
    x = i32(2, 4)
    a = i32(2)
    assert lib.mgx_crop_augment(ptr(c), 64, ptr(st), ptr(a), None, 0, 1, None, None, 0, 0, ptr(x), None, 4, 1, None, PAD, 0, 4, stream()) == -1
    assert lib.mgx_crop_augment(ptr(c), 64, ptr(st), ptr(a), None, 0, 1, None, None, 0, 0, ptr(x), None, 4, 1, None, PAD, 2, 0, stream()) == -1
    assert lib.mgx_crop_augment(ptr(c), 64, ptr(st), ptr(a), None, 0, 0, None, None, 0, 0, ptr(x), None, 4, 1, None, PAD, 2, 4, stream()) == -1
    assert lib.mgx_crop_augment(ptr(c), 64, ptr(st), ptr(a), ptr(a), 1, 1, None, None, 0, 0, ptr(x), None, 4, 1, None, PAD, 2, 4, stream()) == -2
    assert lib.mgx_crop_augment(None, 64, ptr(st), ptr(a), None, 0, 1, None, None, 0, 0, ptr(x), None, 4, 1, None, PAD, 2, 4, stream()) == -2

"""Gradient clipping through the model's layers: FusedAdam(max_norm=...) on the flat buffers of a 1-layer model (d 64, L 32,
batch 2), the skip of a non-finite step, the untouched max_norm=None path, and train.py --clip-norm.

The clipped step is checked like the kernel (tests/test_gpu_clip_kernels.py): the norm within n 2^-52 of the fp64 reference, the
scale bit for bit where the host finds it decidable, p / m / v within C_ADAM = 16 noise floors of oracle.train_ref's Adam at that
scale.  Where a floor is zero -- the zero padding of the flat buffers, rows of the embedding no token selected -- the update must
be exact."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

import clip_ref
import kernel_checks as KC
from kernel_checks import bits
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

V, D, L, B = 90, 64, 32, 2
SEEN = {}
F64 = torch.float64


def _net(seed=0):
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(seed)
    return MusicTransformer(embedding_dim=D, vocab_size=V, num_layer=1, max_seq=L, dropout=0.0).cuda().train()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    xf = torch.randint(0, V - 1, (B, L + 1), generator=g)
    return xf[:, :-1].to(torch.int32).cuda(), xf[:, 1:].to(torch.int32).cuda()


def _backward(mt, seed):
    from musicgeneration_amd.criterion import SmoothCrossEntropyLoss
    x, y = _batch(seed)
    loss = SmoothCrossEntropyLoss(0.1, V, V - 1)(mt(x), y)
    loss.backward()
    return loss.item()


def check_f32(got, ref, F, case):
    """|got - ref| <= C_ADAM * F element by element; F = 0 demands equality"""
    assert got.dtype == torch.float32
    KC.check_bound("ADAM", got, ref, KC.C_ADAM * torch.as_tensor(F, dtype=F64), case, seen=SEEN)


def test_clipped_step_is_the_fp64_references_clipped_adam_on_the_flat_buffers():
    from musicgeneration_amd.optim import FusedAdam
    mt = _net()
    st = mt.store()
    _backward(mt, 1)
    grad = st.grad.detach().cpu()
    n = grad.numel()
    nrm = clip_ref.norm(grad.numpy(), 1.0)
    assert math.isfinite(nrm) and nrm > 0
    margin = n * 2.0 ** -51
    for k in range(64):                                         # a tenth of the norm; nudged until the fp32 rounding of scale is decidable
        max_norm = clip_ref.f32(0.1 * nrm * (1 + k * 2.0 ** -10))
        ref = clip_ref.step(grad.numpy(), 1.0, max_norm, nrm)
        if clip_ref.f32_boundary_distance(ref["coef"]) > margin:
            break
    else:
        raise AssertionError("no decidable max_norm")
    lr, b1, b2, eps = 1e-3, 0.9, 0.98, 1e-9
    opt = FusedAdam(mt, lr=lr, betas=(b1, b2), eps=eps, max_norm=max_norm)
    p0, m0, v0 = st.param.detach().cpu(), opt.m.cpu(), opt.v.cpu()
    opt.step()
    cs = opt.clip_stats()
    print(f"[MODEL] n={n} norm {cs['norm']!r} ref {nrm!r} max_norm {max_norm!r} scale {cs['scale']!r} ref {ref['scale']!r}")
    assert abs(cs["norm"] - nrm) <= n * 2.0 ** -52 * nrm
    assert cs["clipped"] == 1 and cs["skipped"] == 0 and cs["skipped_last"] == 0 and ref["clipped"]
    assert np.float32(cs["scale"]).tobytes() == ref["scale"].tobytes()
    scale = float(ref["scale"])
    r = T.adam_step(p0, grad, m0, v0, lr, b1, b2, eps, 1, scale)
    F = T.adam_floor(p0, grad, m0, v0, lr, b1, b2, eps, 1, scale, r)
    check_f32(st.param, r[0], F[0], "p")
    check_f32(opt.m, r[1], F[1], "m")
    check_f32(opt.v, r[2], F[2], "v")
    assert bits(st.shadow).equal(bits(st.param.to(torch.bfloat16)))
    assert not bits(st.param).equal(bits(p0))


def _three_steps(max_norm):
    from musicgeneration_amd.criterion import CustomSchedule
    from musicgeneration_amd.optim import FusedAdam
    mt = _net(seed=3)
    opt = FusedAdam(mt, lr=0.0, betas=(0.9, 0.98), eps=1e-9, max_norm=max_norm)
    sch = CustomSchedule(D, warmup_steps=20, optimizer=opt)
    opt.zero_grad()
    for k in range(3):
        _backward(mt, 10 + k)
        sch.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    return mt, opt


def test_infinite_max_norm_trains_bit_for_bit_like_no_clipping():
    from musicgeneration_amd import ops
    ops.set_deterministic(True)
    try:
        a, oa = _three_steps(None)
        b, ob = _three_steps(math.inf)
    finally:
        ops.set_deterministic(False)
    assert bits(a.store().param).equal(bits(b.store().param)) and bits(a.store().shadow).equal(bits(b.store().shadow))
    assert bits(oa.m).equal(bits(ob.m)) and bits(oa.v).equal(bits(ob.v))
    cs = ob.clip_stats()
    assert cs["clipped"] == 0 and cs["skipped"] == 0 and cs["scale"] == 1.0 and cs["norm"] > 0
    assert oa.clip_stats() is None


def test_a_poisoned_gradient_skips_the_step_and_training_recovers():
    from musicgeneration_amd.optim import FusedAdam
    mt = _net(seed=4)
    st = mt.store()
    opt = FusedAdam(mt, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, max_norm=1.0)
    opt.zero_grad()
    _backward(mt, 20)
    opt.step()                                                   # a clean step first: the moments are not zero
    opt.zero_grad()
    _backward(mt, 21)
    st.grad[st.grad.numel() // 2] = float("nan")
    before = [bits(t).clone() for t in (st.param, opt.m, opt.v, st.shadow)]
    opt.step()
    cs = opt.clip_stats()
    assert cs["skipped"] == 1 and cs["skipped_last"] == 1 and cs["scale"] == 0.0 and math.isnan(cs["norm"])
    for t, was, name in zip((st.param, opt.m, opt.v, st.shadow), before, ("param", "m", "v", "shadow")):
        assert bits(t).equal(was), f"{name} changed in a skipped step"
    opt.zero_grad()
    _backward(mt, 22)
    old = {n: p.detach().clone() for n, p in mt.named_parameters()}
    opt.step()
    cs = opt.clip_stats()
    assert cs["skipped"] == 1 and cs["skipped_last"] == 0 and math.isfinite(cs["norm"])
    for n, p in mt.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), old[n]), f"{n} did not move after the recovery"
    assert opt._t == 3                                           # optimiser calls, the skipped one included


def test_max_norm_none_allocates_nothing_and_never_measures(monkeypatch):
    from musicgeneration_amd import ops
    from musicgeneration_amd.optim import FusedAdam
    mt = _net(seed=5)
    st = mt.store()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    moments = [torch.zeros_like(st.param), torch.zeros_like(st.param)]
    two_moments = torch.cuda.memory_allocated() - base
    del moments
    opt = FusedAdam(mt, lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    assert torch.cuda.memory_allocated() - base == two_moments   # m and v, nothing else
    assert opt.max_norm is None and opt.clip_stats() is None

    def boom(*a, **k):
        raise AssertionError("ops.grad_norm called with max_norm=None")
    monkeypatch.setattr(ops, "grad_norm", boom)
    monkeypatch.setattr(ops, "adam_step_clipped", boom)
    opt.zero_grad()
    _backward(mt, 30)
    p0 = bits(st.param).clone()
    opt.step()
    assert not bits(st.param).equal(p0)
    with pytest.raises(ValueError, match="max_norm"):
        FusedAdam(mt, max_norm=0.0)


def _dataset(root, n=24, length=120, vocab=308):
    os.makedirs(root, exist_ok=True)
    for i in range(n):
        arr = ((np.arange(length) * (1 + i % 3) + i) % vocab).astype(np.uint16)
        torch.save(arr, os.path.join(root, f"piece{i:02d}-deadbeef.data"))


def test_train_cli_clip_norm_logs_the_norm_and_its_checkpoint_resumes_either_way(tmp_path, capsys):
    from musicgeneration_amd import train
    data, out = str(tmp_path / "data"), str(tmp_path / "ckpt") + "/"
    _dataset(data)
    common = ["-d", data, "-s", out, "-b", "2", "-M", "32", "--num-layers", "1", "--d-model", "64", "--accum-grad", "1",
              "--dropout", "0.0", "-i", "1", "--max-batches", "2"]
    line = re.compile(r"Grad norm >>>> last: (\S+), clipped: (\d+)/(\d+) steps, skipped: (\d+)")
    train.main(common + ["-e", "1", "--clip-norm", "0.5"])
    log = capsys.readouterr().out
    m = line.search(log)
    assert m, log
    assert math.isfinite(float(m.group(1))) and float(m.group(1)) > 0
    assert 0 <= int(m.group(2)) <= 2 and int(m.group(3)) == 2 and int(m.group(4)) == 0
    cks = sorted(glob.glob(out + "train-*.pth"))
    assert cks, "no checkpoint written"
    ck = torch.load(cks[-1], map_location="cpu", weights_only=False)
    assert set(ck) == {"net", "optimizer", "epoch", "sched_step"}                 # unchanged: the counters are not saved
    assert set(ck["optimizer"]) == {"state", "param_groups", "param_names"}
    # resume with the flag (the guard-only form) and without it
    train.main(common + ["-e", str(ck["epoch"] + 2), "-m", cks[-1], "--clip-norm", "inf"])
    log = capsys.readouterr().out
    m = line.search(log)
    assert "Success load" in log and m and int(m.group(2)) == 0 and int(m.group(3)) == 2, log
    train.main(common + ["-e", str(ck["epoch"] + 2), "-m", cks[-1]])
    log = capsys.readouterr().out
    assert "Success load" in log and "Train >>>> Loss:" in log and "Grad norm" not in log

"""The transformer fixtures of tests/test_gpu_dropout_model.py, their oracle and their bounds: CPU only, so that
tests/test_train_ref.py can check the fixtures against the reference alone.  Imported by basename, like kernel_checks."""
import functools

import torch

from kernel_checks import cos as _cos
from test_gpu_model import _params_from_oracle_init

#        V    d   nl   L  B    p
CASES = ((60, 128, 2, 64, 3, 0.2),
         (60, 128, 2, 40, 3, 0.5),              # Lp = 64: the masks run over padded rows; max_seq = 40 < Lp as well
         (309, 192, 1, 32, 2, 0.1))             # FFN width 96, padded to 128 in the flat buffers; vocabulary padded to 320
# seed of a case's parameters and tokens: of 0 .. 11 the one at which the reference itself is least ambiguous (module docstring of
# tests/test_gpu_dropout_model.py)
FIXTURE_SEED = {CASES[0]: 2, CASES[1]: 8, CASES[2]: 4}
MODEL_SEED = 17                                 # torch.manual_seed before the model is built: call k draws (17 * 1000003 + 64 k) & (2^63 - 1)
EPS_LS = 0.1
ULP_BF16 = 2.0 ** -8

_memo = {}


def once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def fixture(case):
    """-> (parameters, two micro-batches (x, y)): oracle.init_params tamed by 0.25, trailing pad tokens in row 1"""
    def make():
        V, d, nl, L, B, _ = case
        p0, _ = _params_from_oracle_init((V, d, nl, L, B), seed=FIXTURE_SEED[case], scale=0.25)
        g = torch.Generator().manual_seed(FIXTURE_SEED[case])
        batches = []
        for _ in range(2):
            xf = torch.randint(0, V - 1, (B, L + 1), generator=g)
            xf[1, L - 4:] = V - 1                                                # trailing pads (inputs L-4.., targets L-5..)
            batches.append((xf[:, :-1].contiguous(), xf[:, 1:].contiguous()))
        return p0, batches
    return once(("fixture", case), make)


def oracle(case, call, drop, round_p=False):
    """logits, loss and gradients of micro-batch `call` under the multipliers `drop` (None: no dropout), bf16 emulated;
    round_p: the second emulation, the softmax rounded to bf16 too (oracle.ref_cpu.rga_forward)"""
    from oracle import ref_cpu as R
    V = case[0]
    p0, batches = fixture(case)
    x, y = batches[call]
    pr = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    plain = R.rga_forward
    R.EMULATE_BF16 = True
    if round_p:
        R.rga_forward = functools.partial(plain, round_p=True)
    try:
        logits, _ = R.model_forward(pr, x, V - 1, drop=drop)
        loss = R.smooth_ce(logits, y, EPS_LS, V, V - 1)
        loss.backward()
    finally:
        R.EMULATE_BF16, R.rga_forward = False, plain
    return {"logits": logits.detach(), "loss": loss.item(), "grads": {k: v.grad for k, v in pr.items()}}


def masks(case, seed, **kw):
    from oracle import ref_cpu as R
    V, d, nl, L, B, p = case
    return R.model_drop(p, seed, nl, B, L, d, **kw)


def logits_ratio(got, ref):
    return (got["logits"] - ref["logits"]).abs().max().item() / (2 * ULP_BF16 * ref["logits"].abs().max().item())


def grad_ratios(got_grads, ref_grads):
    """name -> error / bound of every parameter's gradient: 1 - cosine over 1 - 0.999 (1 - 0.995 up to 1024 elements)"""
    out = {}
    for name, ref_g in ref_grads.items():
        got = got_grads[name]
        assert got.shape == ref_g.shape and torch.isfinite(got).all(), name
        if name.endswith("Wk.bias"):                    # exactly-zero true gradient (softmax shift invariance): noise level
            out[name] = got.abs().max().item() / (2e-2 * ref_grads[name.replace("Wk", "Wq")].abs().max().item())
            continue
        out[name] = (1.0 - _cos(got, ref_g)) / (1.0 - (0.995 if ref_g.numel() <= 1024 else 0.999))
    return out


def measure(got, ref, ref_grads=None):
    """-> {"logits": r, "loss": r, "grads": {name: r}}, each an error over its bound"""
    return {"logits": logits_ratio(got, ref), "loss": abs(got["loss"] - ref["loss"]) / (2e-3 * abs(ref["loss"])),
            "grads": grad_ratios(got["grads"], ref["grads"] if ref_grads is None else ref_grads)}


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def ambiguity(case):
    """the largest move, over its bound, of any gradient between the two emulations (softmax rounded to bf16 or not), over every
    comparison the GPU module makes: p = 0 and p > 0; first call, second call, their sum -> (name, ratio)"""
    worst = ("", 0.0)
    for p_drop in (0.0, case[5]):
        pairs = []
        for call in (0, 1):
            seed = (MODEL_SEED * 1000003 + 64 * (call + 1)) & 0x7FFFFFFFFFFFFFFF
            drop = None if p_drop == 0 else masks(case, seed)
            pairs.append((oracle(case, call, drop), oracle(case, call, drop, round_p=True)))
        for a, b in pairs + [tuple({"grads": add(pairs[0][k]["grads"], pairs[1][k]["grads"])} for k in (0, 1))]:
            r = grad_ratios(b["grads"], a["grads"])
            worst = max(worst, max(r.items(), key=lambda kv: kv[1]), key=lambda kv: kv[1])
    return worst

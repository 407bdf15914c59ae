"""Fused Adam over the model's flat buffers (replaces torch.optim.Adam of train.py:143).

One kernel launch updates every parameter, both moments and the bf16 shadow.  With ``max_norm`` the global gradient norm is
clipped first -- measured by one pass over the flat gradient buffer and applied inside the Adam kernel as a scale read from
device memory -- and a step whose gradient holds an inf or a NaN is skipped instead of being written into p, m, v and the shadow.
``state_dict`` / ``load_state_dict`` use torch.optim.Adam's layout (per-parameter ``step``, ``exp_avg``,
``exp_avg_sq``) so the reference's checkpoints (train.py:201-207) round-trip.

Opt-in, in the same sweep (mgx_adam_step_groups): decoupled weight decay (AdamW) on the matrices, per-parameter learning-rate
multipliers with 0 = frozen, and an exponential moving average of the weights.  With none of them asked for, the kernels, the
allocations and the checkpoint are those of plain Adam."""
from __future__ import annotations

import contextlib
import math
import numbers

import torch

from . import ops


def check_clip_args(max_norm) -> float:
    """max_norm of FusedAdam / --clip-norm: a number > 0; inf = measure the norm and guard against non-finite gradients,
    never clip.  -> float(max_norm); ValueError otherwise (needs no GPU)"""
    if isinstance(max_norm, bool) or not isinstance(max_norm, numbers.Real):
        raise ValueError(f"max_norm must be a number > 0 (inf = guard only), got {max_norm!r}")
    max_norm = float(max_norm)
    if math.isnan(max_norm) or max_norm <= 0.0:
        raise ValueError(f"max_norm must be > 0 (inf = guard only), got {max_norm!r}")
    return max_norm


MAX_GROUPS = ops.ADAM_MAX_GROUPS
EMA_WARMUP = (1.0, 10.0)                                  # decay at update u is min(ema_decay, (1 + u) / (10 + u))


def _number(x, what) -> float:
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or math.isnan(float(x)):
        raise ValueError(f"{what}, got {x!r}")
    return float(x)


def check_weight_decay(weight_decay) -> float:
    """weight_decay of FusedAdam / --weight-decay: a finite number >= 0 (0 = off).  -> float; ValueError otherwise (needs no GPU)"""
    w = _number(weight_decay, "weight_decay must be a number >= 0")
    if w < 0.0 or math.isinf(w):
        raise ValueError(f"weight_decay must be a finite number >= 0, got {weight_decay!r}")
    return w


def check_ema_decay(ema_decay):
    """ema_decay of FusedAdam / --ema-decay: None (off) or a number in (0, 1).  -> None or float; ValueError otherwise"""
    if ema_decay is None:
        return None
    d = _number(ema_decay, "ema_decay must be a number in (0, 1)")
    if not 0.0 < d < 1.0:
        raise ValueError(f"ema_decay must be in (0, 1), got {ema_decay!r}")
    return d


def ema_warmup(ema_decay: float, u: int) -> float:
    """the decay of EMA update number u (from 0): min(ema_decay, (1 + u) / (10 + u)) -- early averages follow the weights"""
    return min(ema_decay, (EMA_WARMUP[0] + u) / (EMA_WARMUP[1] + u))


def default_no_decay(name: str, param) -> bool:
    """parameters AdamW leaves undecayed by default: everything with fewer than 2 dimensions (biases, LayerNorm weight and bias),
    the token embedding and every layer's relative embedding rga.E -- decay falls on the projection matrices only"""
    return param.dim() < 2 or ".embedding." in "." + name or name.endswith("rga.E")


def resolve_lr_scale(lr_scale, names) -> dict:
    """lr_scale {name prefix: number >= 0} -> {name: multiplier} over ``names`` (1.0 where no prefix matches; the longest matching
    prefix wins; 0 freezes).  ValueError for a value that is no finite number >= 0 and for a prefix that matches no name"""
    if lr_scale is None:
        return {n: 1.0 for n in names}
    if not isinstance(lr_scale, dict):
        raise ValueError(f"lr_scale must be a dict from name prefix to a number >= 0, got {lr_scale!r}")
    vals = {}
    for pre, x in lr_scale.items():
        x = _number(x, f"lr_scale[{pre!r}] must be a number >= 0")
        if x < 0.0 or math.isinf(x):
            raise ValueError(f"lr_scale[{pre!r}] must be a finite number >= 0, got {x!r}")
        if not isinstance(pre, str) or not any(n.startswith(pre) for n in names):
            raise ValueError(f"lr_scale prefix {pre!r} matches no parameter; the names are: {', '.join(names)}")
        vals[pre] = x
    out = {}
    for n in names:
        hit = max((pre for pre in vals if n.startswith(pre)), key=len, default=None)
        out[n] = 1.0 if hit is None else vals[hit]
    return out


def build_groups(named, weight_decay=0.0, no_decay=None, lr_scale=None):
    """named: [(name, parameter)] -> (group_of_name {name: k}, groups [(lr multiplier, weight decay)], no_decay names): the
    groups are the distinct pairs, in order of first use.  ValueError for bad arguments or more than MAX_GROUPS groups"""
    w = check_weight_decay(weight_decay)
    if no_decay is not None and not callable(no_decay):
        raise ValueError(f"no_decay must be a predicate (name, parameter) -> bool, got {no_decay!r}")
    names = [n for n, _ in named]
    scale = resolve_lr_scale(lr_scale, names)
    exempt = [n for n, p in named if (no_decay or default_no_decay)(n, p)]
    groups, group_of_name = [], {}
    for n in names:
        pair = (scale[n], 0.0 if n in exempt else w)
        if pair not in groups:
            groups.append(pair)
        group_of_name[n] = groups.index(pair)
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"{len(groups)} distinct (lr_scale, weight_decay) pairs: the kernel takes at most {MAX_GROUPS} groups")
    return group_of_name, groups, exempt


class FusedAdam(torch.optim.Optimizer):
    """weight_decay: AdamW's decoupled decay on every parameter ``no_decay(name, parameter)`` does not exempt (default_no_decay).
    lr_scale: {name prefix: multiplier of lr}, the longest matching prefix wins, 0 freezes the parameter -- its values, moments,
    shadow and EMA are never written; its gradient is still computed and all-reduced (pruning the backward pass is out of
    scope).  ema_decay: keep an exponential moving average of the weights (``averaged``, ``ema_state_dict``, ``load_ema``)."""

    def __init__(self, model, lr=0.0, betas=(0.9, 0.98), eps=1e-9, grad_scale: float = 1.0, max_norm=None, weight_decay=0.0,
                 no_decay=None, lr_scale=None, ema_decay=None):
        self.max_norm = None if max_norm is None else check_clip_args(max_norm)
        weight_decay, self.ema_decay = check_weight_decay(weight_decay), check_ema_decay(ema_decay)
        grouped = weight_decay > 0.0 or no_decay is not None or lr_scale is not None or self.ema_decay is not None
        plan = build_groups(list(model.named_parameters()), weight_decay, no_decay, lr_scale) if grouped else None
        self.model = model
        store = model.store()
        self.store = store
        params = [store.params[n] for n in store.names]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.m = torch.zeros_like(store.param)
        self.v = torch.zeros_like(store.param)
        self._t = 0
        self.grad_scale = grad_scale
        # max_norm=None allocates nothing and keeps the unclipped kernel
        self._clip = ops.clip_buffers(store.param.device) if self.max_norm is not None else None
        # none of weight_decay / no_decay / lr_scale / ema_decay given: nothing more is allocated and step() runs the kernels above
        self._groups = None
        self.weight_decay, self.ema, self._ema_updates, self._averaged = weight_decay, None, 0, False
        if plan is not None:
            dev = store.param.device
            group_of_name, pairs, exempt = plan
            table = ops.adam_group_chunks(store.offsets, store.names, group_of_name, store.numel)
            self._groups = (torch.tensor(table, dtype=torch.uint8, device=dev),
                            torch.tensor([s for s, _ in pairs], dtype=torch.float32, device=dev),
                            torch.tensor([w for _, w in pairs], dtype=torch.float32, device=dev))
            self.no_decay_names, self._pairs = exempt, pairs
            self.lr_scale_of = {n: pairs[k][0] for n, k in group_of_name.items()}
            if self.ema_decay is not None:
                self.ema = store.param.detach().clone()

    def zero_grad(self, set_to_none: bool = False):
        self.store.grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        if self._averaged:
            raise RuntimeError("FusedAdam.step() inside averaged(): the model holds the EMA, not the trained weights")
        g = self.param_groups[0]
        self._t += 1
        dp = getattr(self.model, "_dp", None)
        ops.join_side_stream(self.store.param.device)      # weight gradients / dE issued on the CU-masked side stream (ops.configure_streams)
        if dp is not None:
            dp.wait_all()                 # gradients of every bucket reduced (sum) before the update
        st = self.store
        if self._groups is not None:
            state = None
            if self._clip is not None:
                workspace, state = self._clip
                ops.grad_norm(st.grad, self.grad_scale, self.max_norm, workspace, state)
            # like _t, the EMA's update counter counts optimiser calls, skipped ones included
            decay = 0.0 if self.ema is None else ema_warmup(self.ema_decay, self._ema_updates)
            self._ema_updates += 1
            ops.adam_step_groups(st.param, st.grad, self.m, self.v, st.shadow, self.ema, g["lr"], g["betas"][0], g["betas"][1],
                                 g["eps"], self._t, self.grad_scale, state, *self._groups, decay)
            return
        if self._clip is None:
            ops.adam_step(st.param, st.grad, self.m, self.v, st.shadow, g["lr"], g["betas"][0], g["betas"][1], g["eps"], self._t,
                          self.grad_scale)
            return
        # after the all-reduce, over the same bytes on every rank, by an order-fixed kernel: every rank gets the same scale.
        # _t counts optimiser calls, skipped ones included (a device-side counter would need a host read for state_dict)
        workspace, state = self._clip
        ops.grad_norm(st.grad, self.grad_scale, self.max_norm, workspace, state)
        ops.adam_step_clipped(st.param, st.grad, self.m, self.v, st.shadow, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                              self._t, state)

    def clip_stats(self):
        """{"norm", "scale", "skipped_last", "clipped", "skipped"}: norm, applied gradient scale and skip flag of the last step, and
        the number of steps clipped / skipped since construction (not saved in checkpoints).  SYNCHRONISES -- the only place of
        the clipping path that does.  None when max_norm is None."""
        return None if self._clip is None else ops.read_clip_state(self._clip[1])

    # ---- the EMA as a model --------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("this FusedAdam keeps no EMA: build it with ema_decay")

    @contextlib.contextmanager
    def averaged(self):
        """inside, the model computes with the EMA of its weights; on exit the trained weights and their bf16 shadow are back,
        bit for bit.  step() inside raises"""
        self._need_ema()
        if self._averaged:
            raise RuntimeError("averaged() is not re-entrant")
        st = self.store
        with torch.no_grad():
            stash = st.param.clone()
            self._averaged = True
            try:
                st.param.copy_(self.ema)                  # bumps the version: sync_shadow re-rounds the shadow on the next forward
                yield self.model
            finally:
                st.param.copy_(stash)
                st.sync_shadow(force=True)                # the shadow is always the rounding of the parameters: the same bits as before
                self._averaged = False

    def ema_state_dict(self):
        """the model's state_dict() with the EMA's values: same keys and shapes, clones"""
        self._need_ema()
        return {k: (self.store.view(self.ema, k) if k in self.store.params else t).clone() for k, t in self.model.state_dict().items()}

    @torch.no_grad()
    def load_ema(self, state_dict):
        """the inverse of ema_state_dict(): resume the EMA from a checkpoint's ``net_ema``"""
        self._need_ema()
        for n in self.store.names:
            if n not in state_dict or tuple(state_dict[n].shape) != self.store.shapes[n]:
                raise ValueError(f"EMA state_dict does not match this model at {n!r}")
        for n in self.store.names:
            self.store.view(self.ema, n).copy_(state_dict[n])

    # ---- torch.optim.Adam-compatible checkpoint format --------------------------------------------
    # torch (and the reference's ``Adam(mt.parameters())``, train.py:143) number the per-parameter state by
    # ``model.parameters()`` order (Wq.weight, Wq.bias, Wk.weight, ...), NOT by the flat store's order
    # (Wq.weight, Wk.weight, Wv.weight, Wq.bias, ...): emit and read that numbering, so a checkpoint written here loads
    # into ``torch.optim.Adam(mt.parameters())`` and vice versa.  ``param_names`` (extra key) records the order used.
    def _decay_of(self, name):
        return 0.0 if name in self.no_decay_names else self.weight_decay

    def _torch_order(self):
        return [n for n, _ in self.model.named_parameters()]

    def state_dict(self):
        st = self.store
        names = self._torch_order()
        state = {}
        for i, n in enumerate(names):
            state[i] = {"step": torch.tensor(float(self._t)), "exp_avg": st.view(self.m, n).clone(),
                        "exp_avg_sq": st.view(self.v, n).clone()}
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(names)))}
        sd = {"state": state, "param_groups": [group], "param_names": names}
        if self._groups is not None:
            # one torch param group per kernel group, in the kernel's order (first use along model.named_parameters()), each with
            # its members in that order: the dict loads into a torch.optim.AdamW built over the same split.  lr is the group's
            # effective rate; base_lr (extra key) the optimiser's own
            sd["param_groups"] = []
            for s, w in self._pairs:
                members = [i for i, n in enumerate(names) if (self.lr_scale_of[n], self._decay_of(n)) == (s, w)]
                sd["param_groups"].append(dict(group, lr=g["lr"] * s, base_lr=g["lr"], weight_decay=w if w > 0.0 else 0,
                                               decoupled_weight_decay=w > 0.0, params=members))
            sd["no_decay"] = list(self.no_decay_names)
            sd["lr_scale"] = dict(self.lr_scale_of)
            sd["ema_updates"] = self._ema_updates
        return sd

    def load_state_dict(self, sd):
        st = self.store
        names = sd.get("param_names")
        if names is None:
            names = self._torch_order()        # a torch.optim.Adam checkpoint
        if len(names) != len(st.names) or set(names) != set(st.names):
            raise ValueError("optimizer state_dict does not match this model's parameters")
        for i, n in enumerate(names):
            s = sd["state"].get(i)
            if s is None:
                continue
            k = st.offsets[n][1]
            if s["exp_avg"].numel() != k:
                raise ValueError(f"optimizer state {i} has {s['exp_avg'].numel()} elements, parameter {n} has {k}")
            st.view(self.m, n).copy_(s["exp_avg"].reshape(st.shapes[n]))
            st.view(self.v, n).copy_(s["exp_avg_sq"].reshape(st.shapes[n]))
            self._t = int(float(s["step"]))
        g = sd["param_groups"][0]
        self.param_groups[0]["lr"] = g.get("base_lr", g["lr"])
        # the decay, the exemptions and the multipliers are this optimiser's arguments, not the checkpoint's; an old or a
        # torch.optim.Adam / AdamW checkpoint has no ema_updates: the EMA's warm-up then starts over
        self._ema_updates = int(sd.get("ema_updates", 0))

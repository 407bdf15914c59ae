#!/usr/bin/env python3
"""Shared machinery of the generated gfx950 main loops (gen_dkv_asm.py, gen_gemm_asm.py, tools/experiments/gen_fwd_asm.py):

* the operand parser: the TEXT of an instruction is the only source of the registers it reads and writes (parse), with the roles of
  the operands taken from an explicit mnemonic table -- an instruction outside the table cannot be scheduled;
* instruction emission with the bookkeeping hipcc does not do inside an asm statement (Gen): counted s_waitcnt from the in-order
  LDS / VMEM queues, the wait states between an MFMA and the readers of its result (and the other hazards of such loops) padded
  with s_nop;
* the list scheduler that assigns the non-MFMA instructions of a loop body ("fillers") to the shadows of its MFMAs;
* the writer of the generated *.inc files."""
from __future__ import annotations

import functools
import re
import sys

MFMA_TO_VALU = 13      # wait states between an MFMA and any other instruction touching its result (hipcc pads s_nop 11)
VALU_TO_MFMA = 3       # a VALU-written register as an MFMA operand
TRANS_TO_VALU = 2


def v(i, n=1):
    return f"v{i}" if n == 1 else f"v[{i}:{i + n - 1}]"


def a(i, n=1):
    return f"a{i}" if n == 1 else f"a[{i}:{i + n - 1}]"


def s(i, n=1):
    return f"s{i}" if n == 1 else f"s[{i}:{i + n - 1}]"


def regs(prefix, i, n=1):
    return {f"{prefix}{k}" for k in range(i, i + n)}


# ---- operand parser ---------------------------------------------------------------------------------------------------------------
# mnemonic -> (kind, role, implicit reads, implicit writes).  kind: mfma | valu | trans | salu | lds | vmem | store (what the hazard
# rules of Gen distinguish).  role: "d" = the first operand is the destination, the others are sources; "dr" = ... and the destination
# is a source too; "-" = no destination, every operand is a source.  SCC is modelled where an instruction exists FOR it (compare ->
# select / carry / branch), not as the side effect of SALU arithmetic: nothing here waits on it.
MNEMONICS = {}


def _classify(kind, role, names, reads=(), writes=()):
    for name in names.split():
        MNEMONICS[name] = (kind, role, frozenset(reads), frozenset(writes))


_classify("mfma", "d", "v_mfma_f32_32x32x16_bf16")                 # (C = D: D appears among the sources)
_classify("valu", "d", "v_mov_b32_e32 v_add_u32_e32 v_sub_u32_e32 v_and_b32_e32 v_xor_b32_e32 v_lshlrev_b32_e32 v_lshrrev_b32_e32 v_lshrrev_b32_e64 "
          "v_lshl_add_u32 v_mbcnt_lo_u32_b32 v_mbcnt_hi_u32_b32 v_cndmask_b32_e64 v_fma_f32 v_mul_f32_e32 v_mul_f32_e64 v_add_f32_e32 v_sub_f32_e32 "
          "v_min_f32_e32 v_max_f32_e32 v_cvt_pk_bf16_f32 v_accvgpr_read_b32 v_accvgpr_write_b32 "
          "v_readfirstlane_b32 v_cmp_ne_u32_e64 v_cmp_le_u32_e64 v_cmp_ge_i32_e64 v_cmp_nle_f32_e64")      # (the last five: SGPR / VCC destination)
_classify("valu", "dr", "v_dot2c_f32_bf16_e32")
_classify("trans", "d", "v_exp_f32_e32")
_classify("salu", "d", "s_mov_b32 s_mov_b64 s_add_u32 s_sub_u32 s_mul_i32 s_min_u32 s_min_i32 s_max_i32 s_lshl_b32 s_lshr_b32 s_or_b32 s_or_b64 s_andn2_b64 "
          "s_memtime")                                             # (s_memtime returns through lgkmcnt: only stamp() emits it, with its wait)
_classify("salu", "d", "s_addc_u32 s_cselect_b32 s_cselect_b64", reads={"scc"})
_classify("salu", "-", "s_cmp_eq_u32 s_cmp_lg_u32 s_cmp_ge_u32 s_cmp_lt_u32 s_cmp_ge_i32 s_cmp_gt_i32 s_cmp_lt_i32 s_cmp_eq_u64 s_bitcmp1_b32", writes={"scc"})
_classify("salu", "-", "s_cbranch_scc1", reads={"scc"})
_classify("salu", "-", "s_cbranch_vccnz", reads={"vcc"})
_classify("salu", "-", "s_branch s_barrier s_waitcnt s_nop s_trap")
_classify("lds", "d", "ds_read_b32 ds_read_b128 ds_read_b64_tr_b16 ds_bpermute_b32")
_classify("lds", "-", "ds_write_b32 ds_write_b128")
_classify("vmem", "d", "global_load_dwordx4")
_classify("vmem", "-", "global_load_lds_dword global_load_lds_dwordx4", reads={"m0"})      # LDS-DMA: destination = LDS at M0
_classify("store", "-", "global_store_dwordx4")

_REGISTER = re.compile(r"-?(?:([vsa])(\d+)|([vsa])\[(\d+):(\d+)\]|(m0|exec|vcc|scc))$")      # (-vN: a negated source)
_NOT_A_REGISTER = re.compile(r"(?:-?\d+|0x[0-9a-f]+|\w+_%=|(?:vmcnt|lgkmcnt)\(\d+\))$")         # immediates, labels, s_waitcnt counters
_MODIFIER = re.compile(r"(?:offset:\d+|nt|sc0|sc1)$")


@functools.lru_cache(maxsize=None)
def parse(text, asm_operands=False):
    """instruction text -> (kind, reads, writes).  Registers: vN, sN, aN, ranges x[a:b], m0, exec, vcc, scc.  A compiler-allocated asm
    operand %N is not tracked (nothing in the block but the instructions that name it can touch it) unless asm_operands is set:
    then it counts as the one register "%N"."""
    mnemonic, _, rest = text.partition(" ")
    if mnemonic not in MNEMONICS:
        raise ValueError(f"asm_sched: mnemonic `{mnemonic}` is not in MNEMONICS: classify it (kind, operand roles) before scheduling `{text}`")
    kind, role, reads, writes = MNEMONICS[mnemonic]
    operands = [o.strip() for o in rest.split(",")] if rest.strip() else []
    if operands:                                         # modifiers follow the last operand (s_waitcnt: space-separated counters)
        last, *mods = operands[-1].split()
        if mnemonic == "s_waitcnt":
            operands[-1:] = [last] + mods
        else:
            operands[-1] = last
            bad = [m for m in mods if not _MODIFIER.match(m)]
            if bad:
                raise ValueError(f"asm_sched: modifier {bad} of `{text}` not understood")
    sets = []
    for o in operands:
        m = _REGISTER.match(o)
        if m:
            p1, i, p2, lo, hi, special = m.groups()
            sets.append({special} if special else regs(p1, int(i)) if p1 else regs(p2, int(lo), int(hi) - int(lo) + 1))
        elif re.match(r"%\d+$", o):
            sets.append({o} if asm_operands else set())
        elif _NOT_A_REGISTER.match(o):
            sets.append(set())
        else:
            raise ValueError(f"asm_sched: operand `{o}` of `{text}` not understood")
    if role != "-":
        writes = writes | sets[0]
        sets = sets[role == "d":]
    return kind, reads.union(*sets), frozenset(writes)


class Gen:
    def __init__(self):
        self.out = []                 # text lines
        self.pos = 0                  # wait-state clock (instructions issued; s_nop N counts N+1)
        self.lgkm = []                # outstanding LDS operations: sets of destination registers, oldest first
        self.vm = []                  # every VMEM operation issued so far: (tag, destination registers)
        self.vm_done = 0              # operations [0, vm_done) are known complete
        self.mfma_d = {}              # register -> clock of the last MFMA that wrote it
        self.mfma_c = {}              # register -> clock of the last MFMA that read it as srcC / A / B (WAR)
        self.valu_w = {}              # register -> clock of the last VALU write
        self.trans_w = {}             # register -> clock of the last transcendental write
        self.store_r = {}             # register -> clock of the last VMEM store that reads it
        self.nops = 0
        self.m0_w = None
        self.stats = {}
        self.s_stamp, self.v_stamp = 10, 246      # stamp builds: SGPRs s_stamp..+3, cycle sums in VGPRs v_stamp..

    # ---- low level -------------------------------------------------------------------------------------------------
    def raw(self, text, ws=1):
        self.out.append(text)
        self.pos += ws

    def comment(self, text):
        self.out.append(f"; {text}")

    def nop(self, states):
        while states > 0:
            k = min(states, 8)
            self.raw(f"s_nop {k - 1}", k)
            self.nops += k
            states -= k

    def _wait_lgkm(self, touched):
        idx = -1
        for i, d in enumerate(self.lgkm):
            if d & touched:
                idx = i
        if idx >= 0:
            k = len(self.lgkm) - 1 - idx
            self.raw(f"s_waitcnt lgkmcnt({min(k, 15)})")
            self.lgkm = self.lgkm[len(self.lgkm) - min(k, 15):] if k > 0 else []

    def _wait_vm(self, touched):
        idx = -1
        for i in range(self.vm_done, len(self.vm)):
            if self.vm[i][1] & touched:
                idx = i
        if idx >= 0:
            self.wait_vm_index(idx)

    def wait_vm_index(self, idx):
        k = len(self.vm) - 1 - idx
        self.raw(f"s_waitcnt vmcnt({min(k, 63)})")
        self.vm_done = max(self.vm_done, idx + 1)

    def wait_vm_tag(self, tag):
        idx = max((i for i in range(len(self.vm)) if self.vm[i][0] == tag), default=-1)
        if idx >= self.vm_done:
            self.wait_vm_index(idx)

    def stamp(self, k):
        """diagnostic builds: add the cycles since the previous stamp to sum k (v246 + k; every lane holds the same value).  Reading
        the clock waits for lgkmcnt(0): a stamped build is slower, read its SHARES"""
        self.raw(f"s_memtime {s(self.s_stamp, 2)}")
        self.raw("s_waitcnt lgkmcnt(0)")
        self.lgkm = []
        self.raw(f"s_sub_u32 {s(self.s_stamp + 3)}, {s(self.s_stamp)}, {s(self.s_stamp + 2)}")
        self.raw(f"s_mov_b32 {s(self.s_stamp + 2)}, {s(self.s_stamp)}")
        if k is not None:
            self.raw(f"v_add_u32_e32 {v(self.v_stamp + k)}, {s(self.s_stamp + 3)}, {v(self.v_stamp + k)}")

    def drain(self):
        self.raw("s_waitcnt vmcnt(0) lgkmcnt(0)")
        self.lgkm = []
        self.vm_done = len(self.vm)

    def _hazards(self, kind, reads, writes):
        need = 0
        touched = reads | writes
        for r in touched:
            if r in self.mfma_d and kind != "mfma_acc_same":
                need = max(need, self.mfma_d[r] + MFMA_TO_VALU - self.pos)
        if kind.startswith("mfma"):
            for r in reads:
                if r in self.valu_w:
                    need = max(need, self.valu_w[r] + VALU_TO_MFMA - self.pos)
        else:
            for r in writes:
                if r in self.mfma_c:                       # WAR on an operand of an MFMA in flight
                    need = max(need, self.mfma_c[r] + 6 - self.pos)
                if r in self.store_r:
                    need = max(need, self.store_r[r] + 3 - self.pos)
        if kind == "valu":
            for r in reads:
                if r in self.trans_w:
                    need = max(need, self.trans_w[r] + TRANS_TO_VALU - self.pos)
        if "m0" in reads and kind == "vmem" and self.m0_w is not None:
            need = max(need, self.m0_w + 2 - self.pos)      # SALU write of M0 -> LDS-DMA: one wait state
        if need > 0:
            self.nop(need)

    def emit(self, kind, text, reads=(), writes=()):
        reads, writes = set(reads), set(writes)
        self._wait_lgkm(reads | writes)
        self._wait_vm(reads | writes)
        self._hazards(kind, reads, writes)
        self.raw(text)
        self.stats[kind] = self.stats.get(kind, 0) + 1
        at = self.pos - 1
        if kind.startswith("mfma"):
            for r in writes:
                self.mfma_d[r] = at
            for r in reads:
                self.mfma_c[r] = at
        else:
            for r in writes:
                self.mfma_d.pop(r, None)
                if kind in ("valu", "trans"):
                    self.valu_w[r] = at
                if kind == "trans":
                    self.trans_w[r] = at
                elif r in self.trans_w:
                    del self.trans_w[r]
        if "m0" in writes:
            self.m0_w = at
        if kind == "lds":
            self.lgkm.append(writes)
        if kind == "store":
            for r in reads:
                self.store_r[r] = at

    def prewait(self, touched):
        """wait now for every outstanding load that writes a register of `touched` (the operands of a whole MFMA chain): one
        s_waitcnt pair instead of a descending ladder in front of every MFMA of the chain"""
        self._wait_lgkm(set(touched))
        self._wait_vm(set(touched))

    # ---- instructions ----------------------------------------------------------------------------------------------
    def ins(self, text, tag=None, reads=None, writes=None):
        """emit one instruction; what it reads and writes is what its text says (parse).  tag: the name of the VMEM queue entry of a
        global load, LDS-DMA or store (wait_vm_tag), required for those and only for those.  reads / writes replace the derived sets
        where the text is not the truth: every use carries a comment saying why."""
        kind, r, w = parse(text)
        r, w = (r if reads is None else set(reads)), (w if writes is None else set(writes))
        assert (tag is not None) == (kind in ("vmem", "store")), f"`{text}`: a VMEM instruction, and only a VMEM instruction, takes a queue tag"
        if tag is None:
            self.emit(kind, text, r, w)
        else:
            # the destination of a load belongs to its queue entry -- whoever touches it waits for vmcnt -- and is not checked against
            # the hazards of the load's own issue: its data lands long after an MFMA in flight has read that register as an operand
            self.emit(kind, text, r, set())
            self.vm.append((tag, set(w)))

    def mfma(self, d, a_, b_, c=None, dn=16):
        """d (+)= a_ * b_; registers given as (prefix, index), or ("%", "%N") for a whole asm operand (compiler-allocated tuple).
        Tracking: every operand counts, an asm operand as the one register "%N"; an accumulate step (c is None: C = D) whose D was last
        written by an MFMA continues that MFMA's chain and needs no wait states after it"""
        def opnd(x, n):
            return x[1] if x[0] == "%" else f"{x[0]}[{x[1]}:{x[1] + n - 1}]"
        dt = opnd(d, dn)
        text = f"v_mfma_f32_32x32x16_bf16 {dt}, {opnd(a_, 4)}, {opnd(b_, 4)}, {0 if c == 0 else dt}"
        _, reads, writes = parse(text, asm_operands=True)
        same = c != 0 and all(r in self.mfma_d for r in writes)
        self.emit("mfma_acc_same" if same else "mfma", text, reads, writes)

    def mfma_op(self, opnd, a_, b_, c0=False, cv=None):
        """accumulator given as an asm operand (%N, compiler-allocated AGPRs); c0: C = 0; cv: C = the 16 VGPRs from cv on (D = C + A B
        written to the operand).  Tracking: the accumulator operand is owned by the block's MFMAs and is NOT tracked -- an accumulate
        chain on it needs no wait states, and nothing else in the block touches it (the code behind the block does: the generators end
        with s_nop 16); A, B and a VGPR C are tracked"""
        ct = f"v[{cv}:{cv + 15}]" if cv is not None else ("0" if c0 else opnd)
        self.ins(f"v_mfma_f32_32x32x16_bf16 {opnd}, {a_[0]}[{a_[1]}:{a_[1] + 3}], {b_[0]}[{b_[1]}:{b_[1] + 3}], {ct}")


def crow(r, hh=0):
    return (r & 3) + 8 * (r >> 2) + 4 * hh


def salu_items(g, ops):
    """ops: instruction texts.  One item per SALU instruction, except that an s_addc_u32 stays glued to the s_add_u32 whose carry (SCC) it consumes:
    the scheduler interleaves items of different chains, and nearly every SALU instruction rewrites SCC"""
    out = []
    i = 0
    while i < len(ops):
        grp = [ops[i]]
        while i + 1 < len(ops) and ops[i + 1].startswith("s_addc_u32"):
            i += 1
            grp.append(ops[i])
        out.append(lambda grp=grp: [g.ins(o) for o in grp])
        i += 1
    return out


class Item:
    """one filler (a function that emits one or a few instructions) with its scheduling constraints: it may be placed in the
    shadow of MFMA `earliest` .. `deadline` (gap g = after MFMA g, before MFMA g+1), after every item in `deps`"""

    def __init__(self, fn, cost, earliest=1, deadline=44, deps=(), pin=None, name=""):
        self.fn, self.cost, self.earliest, self.deadline, self.deps, self.pin, self.name = fn, cost, earliest, deadline, list(deps), pin, name
        self.gap = None


COST = {"valu": 4, "trans": 8, "lds": 4, "lds128": 8, "salu": 3, "vmem": 8, "store": 24, "sync": 4}
GAP_BUDGET = 22        # issue cycles of fillers an MFMA (32 cycles, 8 of them its own issue) is asked to hide


def chain(items):
    """items must keep their order"""
    for x, y in zip(items, items[1:]):
        y.deps.append(x)
    return items


def try_schedule(items, ngaps, budget):
    for it in items:
        it.gap = None
    table = {g: [] for g in range(1, ngaps + 1)}
    todo = list(items)
    over = 0
    for g in range(1, ngaps + 1):
        used = 0
        progress = True
        while progress:
            progress = False
            ready = [it for it in todo if it.earliest <= g and all(d.gap is not None for d in it.deps) and (it.pin is None or it.pin == g)]
            ready.sort(key=lambda it: (it.deadline, it.earliest))
            for it in ready:
                must = it.deadline <= g or it.pin == g
                if must or used + it.cost <= budget:
                    it.gap = g
                    table[g].append(it)
                    todo.remove(it)
                    used += it.cost
                    progress = True
                    break
        over = max(over, used - budget)
    return table, todo, over


def schedule(items, ngaps=44, budget0=None):
    """earliest-deadline-first list scheduling with the smallest uniform per-gap issue budget that places every filler inside its
    window (the fillers of a step cost more than 44 MFMA shadows hide: spread the excess evenly instead of piling it up)"""
    budget = GAP_BUDGET if budget0 is None else budget0
    while True:
        table, todo, over = try_schedule(items, ngaps, budget)
        if not todo and over <= 8:
            break
        budget += 1
        assert budget < 200, f"unschedulable: {[it.name for it in todo][:8]}"
    late = [it for g in table for it in table[g] if g > it.deadline]
    assert not late, f"fillers placed after their deadline: {[(it.name, it.gap, it.deadline) for it in late][:8]}"
    return table, budget


def add_items(items, fns, cost=None, spread=0, **kw):
    """one Item per function of fns (or per (function, cost) pair), appended to `items`; spread: the k-th of the n items not before
    gap earliest + k * spread // n (an even trickle instead of a burst)"""
    out = []
    for k, f in enumerate(fns):
        f, c = f if isinstance(f, tuple) else (f, cost)
        out.append(Item(f, c, **{**kw, "earliest": kw.get("earliest", 1) + k * spread // len(fns)}))
    items.extend(out)
    return out


def fixed_point(g, emit_round, check=True):
    """a loop is generated from its own loop-carried state: three rounds of emit_round(), of which the second reaches the state of
    the wait / hazard trackers at the loop's back edge; the third must repeat it and is the one kept"""
    texts = []
    for _ in range(3):
        g.out = []
        emit_round()
        texts.append(list(g.out))
    assert not check or texts[1] == texts[2], "the loop body is not a fixed point of the wait-count / hazard trackers"
    return texts[2]


def summary(path, lines, g, label="", counts=True):
    n = sum(1 for ln in lines if not ln.startswith(";") and not ln.endswith(":"))
    print(f"wrote {path}{label}: {n} instructions, s_nop wait states inserted: {g.nops}" + (f"; counts {g.stats}" if counts else ""), file=sys.stderr)


def write_inc(path, header, macros, clobbers, tail=""):
    """a generated file: `header` comment lines, one string-literal macro per (name, lines) of `macros` (a "; ..." line becomes a
    C comment), the clobber list (macro name, registers), `tail`"""
    text = "".join(f"// {h}\n" for h in header)
    for name, lines in macros:
        text += f"#define {name} \\\n"
        for ln in lines:
            text += f"    /* {ln[1:].strip()} */ \\\n" if ln.startswith(";") else f'    "{ln}\\n\\t" \\\n'
        text += '    ""\n'
    text += f"#define {clobbers[0]} " + ", ".join(f'"{c}"' for c in clobbers[1]) + "\n" + tail
    write_if_changed(path, text)


def write_if_changed(path, text):
    """write a generated file only when its content differs: an unchanged schedule keeps its mtime, so a variant build (which
    runs the generators too) does not make the product library look stale (musicgeneration_amd/_build.py: _stale)"""
    try:
        with open(path) as f:
            if f.read() == text:
                return False
    except OSError:
        pass
    with open(path, "w") as f:
        f.write(text)
    return True

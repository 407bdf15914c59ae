"""csrc/asm_sched.py: the operand parser that derives an instruction's register sets from its text, and the wait-count / hazard
tracker of the generated main loops (the tracker cases are pinned to what the tracker emitted when every call site still passed
hand-kept register sets).  No GPU needed."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "musicgeneration_amd", "csrc")
sys.path.insert(0, CSRC)
from asm_sched import MNEMONICS, Gen, parse, regs, salu_items  # noqa: E402

V, S, A = (lambda i, n=1: regs("v", i, n)), (lambda i, n=1: regs("s", i, n)), (lambda i, n=1: regs("a", i, n))

PARSER_CASES = [
    # ---- role classes
    ("v_add_u32_e32 v3, v1, v2", "valu", V(1, 2), V(3)),                                            # destination first
    ("global_store_dwordx4 v16, v[4:7], s[34:35]", "store", V(16) | V(4, 4) | S(34, 2), set()),     # no destination: store
    ("ds_write_b32 v32, v64 offset:272", "lds", V(32) | V(64), set()),                              # ... LDS write
    ("s_cmp_ge_u32 s80, s81", "salu", S(80, 2), {"scc"}),                                           # ... compare: writes SCC
    ("s_bitcmp1_b32 s83, 12", "salu", S(83), {"scc"}),
    ("s_cbranch_scc1 L_dkv_end_%=", "salu", {"scc"}, set()),                                        # ... branch: reads SCC, %= label
    ("s_addc_u32 s93, s79, 0", "salu", S(79) | {"scc"}, S(93)),                                     # reads SCC
    ("s_cselect_b32 s50, s40, 0", "salu", S(40) | {"scc"}, S(50)),
    ("global_load_lds_dwordx4 v23, s[92:93]", "vmem", V(23) | S(92, 2) | {"m0"}, set()),            # reads M0, no register destination
    ("v_dot2c_f32_bf16_e32 v5, v33, v29", "valu", V(5) | V(33) | V(29), V(5)),                      # destination also read
    ("v_mfma_f32_32x32x16_bf16 v[78:93], v[46:49], a[144:147], v[78:93]", "mfma", V(78, 16) | V(46, 4) | A(144, 4), V(78, 16)),   # C = D
    ("v_mfma_f32_32x32x16_bf16 v[78:93], v[46:49], a[144:147], 0", "mfma", V(46, 4) | A(144, 4), V(78, 16)),
    ("ds_bpermute_b32 v78, v30, v78", "lds", V(30) | V(78), V(78)),
    ("v_readfirstlane_b32 s68, v78", "valu", V(78), S(68)),                                         # SGPR destination of a VALU instruction
    ("v_cmp_le_u32_e64 s[36:37], v241, v244", "valu", V(241) | V(244), S(36, 2)),                   # SGPR-pair destination
    ("v_exp_f32_e32 v78, v78", "trans", V(78), V(78)),
    ("v_accvgpr_write_b32 a128, v233", "valu", V(233), A(128)),
    # ---- operand forms
    ("s_mov_b32 s80, s81", "salu", S(81), S(80)),                                                   # single registers
    ("ds_read_b128 v[62:65], v17 offset:12288", "lds", V(17), V(62, 4)),                            # range, offset:
    ("s_add_u32 m0, s99, 2048", "salu", S(99), {"m0"}),                                             # m0
    ("s_cselect_b64 exec, -1, 0", "salu", {"scc"}, {"exec"}),                                       # exec, negative immediate
    ("s_mov_b64 exec, s[18:19]", "salu", S(18, 2), {"exec"}),
    ("v_cmp_nle_f32_e64 vcc, v230, s80", "valu", V(230) | S(80), {"vcc"}),                          # vcc
    ("v_mul_f32_e64 v224, -v226, s79", "valu", V(226) | S(79), V(224)),                             # negated source
    ("global_store_dwordx4 v16, v[174:177], s[34:35] offset:1024 nt", "store", V(16) | V(174, 4) | S(34, 2), set()),      # cache policies
    ("global_store_dwordx4 v16, v[174:177], s[34:35] offset:1024 sc0 sc1", "store", V(16) | V(174, 4) | S(34, 2), set()),
    ("global_load_dwordx4 a[208:211], v16, s[34:35] offset:3072", "vmem", V(16) | S(34, 2), A(208, 4)),
    ("v_mfma_f32_32x32x16_bf16 %2, v[206:209], v[78:81], %2", "mfma", V(206, 4) | V(78, 4), set()),   # %N: not tracked
    ("v_mov_b32_e32 v239, %8", "valu", set(), V(239)),
    ("s_mov_b32 s89, 0x3e38aa3b", "salu", set(), S(89)),                                            # hex immediate
    ("v_lshl_add_u32 v240, v238, 2, v239", "valu", V(238, 2), V(240)),                              # decimal immediate between registers
    ("s_waitcnt vmcnt(0) lgkmcnt(0)", "salu", set(), set()),
    ("s_barrier", "salu", set(), set()),
]


@pytest.mark.parametrize("text,kind,reads,writes", PARSER_CASES, ids=[c[0] for c in PARSER_CASES])
def test_parser_derives_kind_reads_writes_from_the_text(text, kind, reads, writes):
    assert parse(text) == (kind, reads, writes)


def test_asm_operands_are_tracked_on_request_only():
    text = "v_mfma_f32_32x32x16_bf16 v[64:79], %8, a[192:195], v[64:79]"
    assert parse(text) == ("mfma", V(64, 16) | A(192, 4), V(64, 16))
    assert parse(text, asm_operands=True) == ("mfma", V(64, 16) | A(192, 4) | {"%8"}, V(64, 16))


def test_an_unknown_mnemonic_raises_and_is_named():
    assert "v_pk_add_f32" not in MNEMONICS
    with pytest.raises(ValueError, match="v_pk_add_f32"):
        parse("v_pk_add_f32 v[0:1], v[2:3], v[4:5]")
    with pytest.raises(ValueError, match="v_pk_add_f32"):
        Gen().ins("v_pk_add_f32 v[0:1], v[2:3], v[4:5]")
    with pytest.raises(ValueError, match="glc"):           # ... and so does an operand or modifier the parser does not know
        parse("global_load_dwordx4 a[0:3], v16, s[2:3] glc")


def test_every_line_of_the_tracked_loops_parses_to_the_registers_it_names():
    """two implementations against every instruction line of the tracked files: the parser, and the regular expressions of
    test_generated_asm.py (test_every_register_the_asm_statements_name_is_in_their_clobber_lists)"""
    n_lines = 0
    for name in ("rel_attn_dkv64_loop.inc", "linear_dw_ring4_loop.inc", "linear_ring4_loop.inc"):
        for line in open(os.path.join(CSRC, name)):
            m = re.match(r'\s*"([^"]*?)(?:\\n\\t)?" \\?$', line)
            if not m:
                continue
            ins = m.group(1).split(";")[0]
            if not ins or ins.endswith(":"):
                continue
            n_lines += 1
            used = set()
            for kind, lo, hi in re.findall(r"\b([vsa])\[(\d+):(\d+)\]", ins):
                used |= {f"{kind}{i}" for i in range(int(lo), int(hi) + 1)}
            ins_wo_ranges = re.sub(r"\b[vsa]\[\d+:\d+\]", "", ins)
            used |= set(re.findall(r"(?<![\w.])([vsa]\d+)(?![\w\[])", ins_wo_ranges.split(None, 1)[1] if " " in ins_wo_ranges else ""))
            _, reads, writes = parse(ins)
            assert (reads | writes) - {"scc", "m0", "exec", "vcc"} == used, f"{name}: {ins}"
    assert n_lines > 10000


# ---- the tracker: smallest sequences, expectations from the tracker as it was driven by hand-kept sets ---------------------------
MFMA0 = "v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], v[20:23], 0"


def test_a_consumer_of_the_first_of_two_lds_reads_waits_with_a_count():
    g = Gen()
    g.ins("ds_read_b32 v1, v0")
    g.ins("ds_read_b32 v2, v0 offset:4")
    g.ins("v_mov_b32_e32 v3, v1")
    assert g.out == ["ds_read_b32 v1, v0", "ds_read_b32 v2, v0 offset:4", "s_waitcnt lgkmcnt(1)", "v_mov_b32_e32 v3, v1"]


def test_a_valu_reader_of_an_mfma_result_issues_13_slots_behind_it():
    g = Gen()
    g.mfma(("v", 0), ("v", 16), ("v", 20), c=0)
    g.ins("v_mov_b32_e32 v40, v0")
    assert g.out == [MFMA0, "s_nop 7", "s_nop 3", "v_mov_b32_e32 v40, v0"] and g.nops == 12


def test_an_mfma_operand_written_by_a_valu_instruction_issues_3_slots_behind_it():
    g = Gen()
    g.ins("v_mov_b32_e32 v16, v50")
    g.mfma(("v", 0), ("v", 16), ("v", 20), c=0)
    assert g.out == ["v_mov_b32_e32 v16, v50", "s_nop 1", MFMA0] and g.nops == 2


def test_a_valu_reader_of_a_transcendental_issues_2_slots_behind_it():
    g = Gen()
    g.ins("v_exp_f32_e32 v1, v0")
    g.ins("v_mov_b32_e32 v2, v1")
    assert g.out == ["v_exp_f32_e32 v1, v0", "s_nop 0", "v_mov_b32_e32 v2, v1"] and g.nops == 1


def test_an_lds_dma_behind_a_salu_write_of_m0_gets_its_wait_state():
    g = Gen()
    g.ins("s_add_u32 m0, s10, 0")
    g.ins("global_load_lds_dword v1, s[2:3]", "dma")
    assert g.out == ["s_add_u32 m0, s10, 0", "s_nop 0", "global_load_lds_dword v1, s[2:3]"] and g.vm == [("dma", set())]


def test_overwriting_the_source_of_a_store_issues_3_slots_behind_it():
    g = Gen()
    g.ins("global_store_dwordx4 v0, v[4:7], s[2:3] nt", "st")
    g.ins("v_mov_b32_e32 v4, v9")
    assert g.out == ["global_store_dwordx4 v0, v[4:7], s[2:3] nt", "s_nop 1", "v_mov_b32_e32 v4, v9"] and g.nops == 2


def test_an_accumulate_chain_of_mfmas_needs_no_wait_states():
    g = Gen()
    g.mfma(("v", 0), ("v", 16), ("v", 20), c=0)
    g.mfma(("v", 0), ("v", 24), ("v", 28))
    assert g.out == [MFMA0, "v_mfma_f32_32x32x16_bf16 v[0:15], v[24:27], v[28:31], v[0:15]"]
    assert g.stats == {"mfma": 1, "mfma_acc_same": 1}


def test_the_accumulator_operand_of_mfma_op_is_not_tracked():
    g = Gen()
    g.mfma_op("%0", ("v", 16), ("v", 20))
    g.mfma_op("%0", ("v", 24), ("v", 28))
    assert g.out == ["v_mfma_f32_32x32x16_bf16 %0, v[16:19], v[20:23], %0", "v_mfma_f32_32x32x16_bf16 %0, v[24:27], v[28:31], %0"]
    assert g.mfma_d == {} and g.nops == 0


def test_wait_vm_tag_counts_the_younger_queue_entries():
    g = Gen()
    g.ins("global_load_dwordx4 a[0:3], v16, s[2:3]", "e")
    g.ins("global_load_lds_dwordx4 v17, s[4:5]", "dma")
    g.ins("global_store_dwordx4 v0, v[4:7], s[6:7]", "st")
    g.wait_vm_tag("e")
    g.wait_vm_tag("e")                                     # (known complete: no second wait)
    assert g.out[3:] == ["s_waitcnt vmcnt(2)"]
    assert g.vm == [("e", A(0, 4)), ("dma", set()), ("st", set())]


def test_a_reader_of_a_load_destination_waits_for_its_queue_entry():
    g = Gen()
    g.ins("global_load_dwordx4 a[0:3], v16, s[2:3]", "e")
    g.ins("global_load_dwordx4 a[4:7], v16, s[2:3] offset:1024", "e")
    g.mfma(("v", 0), ("v", 16), ("a", 0), c=0)
    assert g.out[2:] == ["s_waitcnt vmcnt(1)", "v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], a[0:3], 0"]


def test_an_override_replaces_the_derived_sets_and_a_queue_tag_is_for_vmem_only():
    g = Gen()
    g.ins("ds_read_b32 v1, v0")
    g.ins("v_mov_b32_e32 v3, v1", reads=set())             # (test: the override, not the text, decides)
    assert g.out == ["ds_read_b32 v1, v0", "v_mov_b32_e32 v3, v1"]
    with pytest.raises(AssertionError):
        g.ins("global_load_dwordx4 a[0:3], v16, s[2:3]")
    with pytest.raises(AssertionError):
        g.ins("v_mov_b32_e32 v3, v1", "tag")


def test_salu_items_keeps_an_addc_glued_to_its_add():
    g = Gen()
    items = salu_items(g, ["s_add_u32 s4, s2, s1", "s_addc_u32 s5, s3, 0", "s_lshl_b32 s6, s1, 2"])
    assert len(items) == 2
    items[0]()
    assert g.out == ["s_add_u32 s4, s2, s1", "s_addc_u32 s5, s3, 0"]
    items[1]()
    assert g.out[2:] == ["s_lshl_b32 s6, s1, 2"]

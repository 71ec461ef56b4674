"""The hot kernels' ISA keeps the store phases free of loads (tools/isa_audit.py; CPU only: hipcc cross-compiles).

On gfx950 vmcnt counts loads and stores in one in-order queue, so a load issued behind a store makes its wait cover the
store's acknowledgement as well.  The audit compiles gemm.hip, gemm_ln.hip and attention.hip with the Makefile's flags and
checks the hot instantiations; the parser tests below run on small assembly snippets and need no compiler.
"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


A = _load()

_TAIL = "\n; NumVgprs: 100\n; ScratchSize: 0\n; Occupancy: 3\n"


def _kernel(body: str, name: str = "_ZN4rald6kernelILi1ELb0EEEvv") -> str:
    return f"{name}: ; @{name}\n" + "\n".join("\t" + l if not l.startswith(".") else l for l in body.strip().split("\n")) + _TAIL


def test_split_kernels_reads_template_arguments():
    asm = _kernel("s_endpgm", "_ZN4rald19gemm_nt_glds_kernelILi256ELi256ELi4ELi2ELi2ELi3EEEvNS_8GemmArgsE") + "\t.section\t.rodata\n" + \
          _kernel("s_endpgm", "_ZN4rald20attention_d64_kernelILb1ELb0ELb0EEEvNS_8AttnArgsE")
    ks = A.split_kernels(asm)
    assert set(ks) == {("gemm_nt_glds_kernel", (256, 256, 4, 2, 2, 3)), ("attention_d64_kernel", (1, 0, 0))}


def test_load_behind_a_store_is_found():
    clean = _kernel("global_load_dwordx4 v[0:3], v[4:5], off\ns_waitcnt vmcnt(0)\nglobal_store_dwordx4 v[4:5], v[0:3], off\n"
                    "global_store_dwordx4 v[4:5], v[0:3], off offset:16\ns_endpgm")
    assert A.audit_kernel(clean, 2, A.GEMM) == []
    late = _kernel("global_store_dwordx4 v[4:5], v[0:3], off sc0 sc1 nt\nglobal_load_dwordx4 v[0:3], v[4:5], off\ns_waitcnt vmcnt(0)\n"
                   "global_store_dwordx4 v[4:5], v[0:3], off\ns_endpgm")
    f = A.audit_kernel(late, 2, A.GEMM)
    assert len(f) == 1 and "1 VMEM load(s) behind the first store" in f[0]
    assert any("VMEM load" in x for x in A.audit_kernel(late.replace("global_load_dwordx4", "flat_load_dwordx4"), 2, A.GEMM))


def test_wait_behind_a_store_is_found_without_a_load():
    k = _kernel("global_store_dwordx4 v[4:5], v[0:3], off\ns_waitcnt vmcnt(0)\nglobal_store_dwordx4 v[4:5], v[0:3], off offset:16\ns_endpgm")
    f = A.audit_kernel(k, 2, A.GEMM)
    assert len(f) == 1 and "1 vmcnt wait(s) behind the first store" in f[0]
    assert A.audit_kernel(k.replace("s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(0)"), 2, A.GEMM) == []


def test_scratch_and_occupancy_are_checked():
    k = _kernel("s_endpgm")
    assert A.audit_kernel(k, 3, A.GEMM) == []
    assert any("occupancy" in x for x in A.audit_kernel(k, 4, A.GEMM))
    assert any("ScratchSize" in x for x in A.audit_kernel(k.replace("ScratchSize: 0", "ScratchSize: 16"), 3, A.GEMM))


_LOOP_TWO_STAGE = """
.LBB0_1:
s_waitcnt vmcnt(0)
s_barrier
global_load_lds_dwordx4 v[2:3], off
v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], v[20:23], v[0:15]
s_waitcnt vmcnt(0)
ds_read_b64_tr_b16 v[4:5], v76
ds_read_b64_tr_b16 v[6:7], v76 offset:1024
s_cbranch_scc1 .LBB0_1
s_endpgm
"""
_LOOP_THREE_STAGE = """
.LBB0_1:
s_cbranch_vccz .LBB0_2
s_waitcnt vmcnt(0)
.LBB0_2:
s_waitcnt vmcnt(4)
s_barrier
v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], v[20:23], v[0:15]
s_waitcnt vmcnt(0)
ds_read_b64_tr_b16 v[4:5], v76
ds_read_b64_tr_b16 v[6:7], v76 offset:1024
global_load_lds_dwordx4 v[2:3], off
s_cbranch_scc1 .LBB0_1
s_endpgm
"""
_LOOP_VT = """
.LBB0_1:
s_waitcnt vmcnt(0)
s_barrier
global_load_lds_dwordx4 v[2:3], off
ds_read_b64 v[4:5], v76
s_waitcnt lgkmcnt(0)
v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], v[20:23], v[0:15]
s_cbranch_scc1 .LBB0_1
s_endpgm
"""


def test_key_loop_patterns():
    two = A.audit_kernel(_kernel(_LOOP_TWO_STAGE), 3, A.KEYLOOP)
    assert any("behind the iteration's DMA issue" in x for x in two) and any("in front of the tile's last" in x for x in two)
    assert A.audit_kernel(_kernel(_LOOP_THREE_STAGE), 3, A.KEYLOOP) == []
    assert A.audit_kernel(_kernel(_LOOP_VT), 3, A.KEYLOOP) == []
    assert A.audit_kernel(_kernel("s_endpgm"), 3, A.KEYLOOP) == ["no key loop with a barrier found"]
    # near misses of the three-stage pattern: a vmcnt wait behind the DMA issue; the DMA in front of the last tr-read; no DMA in the loop
    late_wait = _LOOP_THREE_STAGE.replace("global_load_lds_dwordx4 v[2:3], off\n", "global_load_lds_dwordx4 v[2:3], off\ns_waitcnt vmcnt(0)\n")
    f = A.audit_kernel(_kernel(late_wait), 3, A.KEYLOOP)
    assert len(f) == 1 and "behind the iteration's DMA issue" in f[0]
    early_dma = _LOOP_THREE_STAGE.replace("ds_read_b64_tr_b16 v[6:7], v76 offset:1024\nglobal_load_lds_dwordx4 v[2:3], off\n",
                                          "global_load_lds_dwordx4 v[2:3], off\nds_read_b64_tr_b16 v[6:7], v76 offset:1024\n")
    assert early_dma != _LOOP_THREE_STAGE
    f = A.audit_kernel(_kernel(early_dma), 3, A.KEYLOOP)
    assert len(f) == 1 and "in front of the tile's last" in f[0]
    no_dma = _LOOP_THREE_STAGE.replace("global_load_lds_dwordx4 v[2:3], off\n", "")
    assert any("no LDS-DMA issue" in x for x in A.audit_kernel(_kernel(no_dma), 3, A.KEYLOOP))
    # resources-only entries (the unprescaled forms) are not held to the loop pattern, only to scratch and occupancy
    assert A.audit_kernel(_kernel(_LOOP_TWO_STAGE), 3, A.RESOURCES) == []
    assert any("occupancy" in x for x in A.audit_kernel(_kernel(_LOOP_TWO_STAGE), 4, A.RESOURCES))


_MFMA_KERNEL = """
s_load_dwordx2 s[0:1], s[4:5], 0x0
v_lshlrev_b32_e32 v1, 4, v0
.LBB0_1:
ds_read_b128 v[4:7], v1 offset:1024
s_waitcnt lgkmcnt(0)
v_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], v[8:11]
s_cmp_eq_u32 s2, s3
s_cbranch_scc1 .LBB0_2
s_branch .LBB0_1
.LBB0_2:
global_store_dwordx4 v[2:3], v[8:11], off
s_endpgm
"""


def test_comparison_against_another_tree(capsys):
    old = _kernel(_MFMA_KERNEL).replace("; Occupancy", "; LDSByteSize: 4096 bytes/workgroup (compile time only)\n; Occupancy")
    assert A.resources(old) == {"NumVgprs": "100", "ScratchSize": "0", "Occupancy": "3", "LDSByteSize": "4096"}
    assert [len(b) for b in A.mfma_blocks(old)] == [5]              # the loop body: label to branch
    # other registers and block numbers, one more set-up instruction: the MFMA block is the same, the delta is counted outside it
    renamed = old.replace("v[4:7]", "v[12:15]").replace("v1", "v20").replace("s2, s3", "s6, s7").replace(".LBB0_", ".LBB7_")
    renamed = renamed.replace("v_lshlrev_b32_e32 v20, 4, v0", "v_lshlrev_b32_e32 v20, 4, v0\n\ts_mov_b32 s9, 0")
    findings, notes = A.compare_kernel(old, renamed, True)
    assert findings == [] and notes == ["1 MFMA block(s) identical, +1 instruction(s) outside them"]
    # an instruction changed inside the block: a finding for a hot kernel, a note for any other
    flipped = old.replace("s_cmp_eq_u32", "s_cmp_lg_u32").replace("s_cbranch_scc1 .LBB0_2", "s_cbranch_scc0 .LBB0_2")
    findings, notes = A.compare_kernel(old, flipped, True)
    assert len(findings) == 1 and "first at instruction 3: `s_cmp_eq_u32 s#, s#` -> `s_cmp_lg_u32 s#, s#`" in findings[0] and "DIFFER" in notes[0]
    findings, notes = A.compare_kernel(old, flipped, False)
    assert findings == [] and len(notes) == 2
    # an offset is not a register name; a changed register count is a finding for every kernel
    assert A.compare_kernel(old, old.replace("offset:1024", "offset:2048"), True)[0]
    assert A.compare_kernel(old, old.replace("NumVgprs: 100", "NumVgprs: 104"), False)[0] == ["NumVgprs 100 -> 104"]
    # a barrier lost outside the MFMA blocks (the hand-over of the staging buffers to the epilogue) is a finding for every kernel
    with_barrier = old.replace("global_store_dwordx4", "s_barrier\n\tglobal_store_dwordx4")
    assert A.compare_kernel(with_barrier, old, False)[0] == ["s_barrier count 1 -> 0"] and A.compare_kernel(with_barrier, with_barrier, True)[0] == []
    # the hot set: the GEMM entries of HOT and every epilogue of the other shipped tile shapes
    assert A.is_compare_hot(("gemm_mx8_kernel", (128, 128, 2, 2, 3))) and A.is_compare_hot(("gemm_resid_ln_kernel", (64, 1, 8, 1, 1)))
    assert A.is_compare_hot(("gemm_nt_glds_kernel", (256, 256, 4, 2, 2, 3))) and not A.is_compare_hot(("gemm_nt_glds_kernel", (256, 256, 4, 2, 2, 1)))
    assert not A.is_compare_hot(("gemm_resid_ln_kernel", (64, 1, 8, 1, 0))) and not A.is_compare_hot(None)
    # all engine files of a tree go into one symbol table, so a kernel that moved from radar.hip to conv3d.hip is still compared with the
    # other tree's - a changed instruction in it is found - and a file that one tree does not have is simply absent from that tree
    conv, gn = "_ZN4rald19conv3d_igemm_kernelENS_8ConvArgsE", "_ZN4rald15gn_stats_kernelEPKfPdiii"
    sec = "\t.section\t.rodata\n"
    _kernel_lds = lambda body, name: _kernel(body, name).replace("; Occupancy", "; LDSByteSize: 4096 bytes/workgroup (compile time only)\n; Occupancy")
    old = A.engine_kernels({"radar.hip": _kernel_lds(_MFMA_KERNEL, conv) + sec + _kernel_lds("s_endpgm", gn)})
    new = A.engine_kernels({"conv3d.hip": _kernel_lds(_MFMA_KERNEL, conv), "radar.hip": _kernel_lds("s_endpgm", gn)})
    assert set(old) == set(new) == {conv, gn} and A.is_compare_hot_symbol(conv) and A.is_compare_hot_symbol(gn)
    assert A.compare_kernels(old, new) == 0
    assert "2 kernel symbols" in capsys.readouterr().out
    flipped = _MFMA_KERNEL.replace("s_cmp_eq_u32", "s_cmp_lg_u32")
    moved_and_changed = A.engine_kernels({"conv3d.hip": _kernel_lds(flipped, conv), "radar.hip": _kernel_lds("s_endpgm", gn)})
    assert A.compare_kernels(old, moved_and_changed) == 1
    out = capsys.readouterr().out
    assert "FAIL  hot " + conv in out and "ok    hot " + gn in out
    # a kernel that one tree lacks is one finding (the symbol sets differ); the same symbol in two files of one tree is an error
    assert A.compare_kernels(old, A.engine_kernels({"radar.hip": _kernel_lds("s_endpgm", gn)})) == 1
    assert "ONLY against: ['" + conv + "']" in capsys.readouterr().out
    with pytest.raises(RuntimeError, match="two engine files"):
        A.engine_kernels({"conv3d.hip": _kernel_lds("s_endpgm", gn), "radar.hip": _kernel_lds("s_endpgm", gn)})
    assert "conv3d.hip" in A.ENGINE_FILES and "radar.hip" in A.ENGINE_FILES


def test_makefile_flags_are_the_library_s():
    hipcc, flags = A.makefile_flags(A.CSRC)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags and "-amdgpu-mfma-vgpr-form=1" in flags


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None, reason="hipcc is not installed")
def test_hot_kernels_pass_the_isa_audit(tmp_path):
    report = A.audit(keep=str(tmp_path))
    assert len(report) == len(A.HOT)
    bad = {k: v for k, v in report.items() if v}
    assert not bad, "\n".join(f"{k}: {'; '.join(v)}" for k, v in bad.items())

#!/usr/bin/env python3
"""ISA audit of the hot kernels: compiles gemm.hip, gemm_ln.hip and attention.hip to gfx950 assembly with the Makefile's
flags (no GPU needed) and checks what the source cannot show.

On gfx950 `vmcnt` is ONE in-order counter for loads and stores: the `s_waitcnt vmcnt(N)` of a load issued behind a store
also waits for that store to be acknowledged.  An epilogue that loads a bias or modulation vector per m-tile therefore
serialises its m-tiles on a store round trip each, and a wait for a young LDS-DMA in the middle of an attention key tile
leaves the prefetch a fraction of a tile to land.  Rule (head of rald_amd/csrc/gemm_epilogue.h): in an epilogue every
VMEM load goes before the first store; per-column vectors come from LDS; no generic-pointer reads.

Checked per hot instantiation:
  * no global_load / buffer_load / flat_load behind the kernel's first global / buffer / flat store, and for the GEMMs no
    `s_waitcnt vmcnt` behind it either (so `bias == nullptr` leaves nothing between the m-tiles);
  * attention key loop (the Vt form; with --keyloop-all every attention form): the hand-over wait (directly in front of the loop's s_barrier) aside, every `s_waitcnt vmcnt`
    stands in front of the iteration's first LDS-DMA issue, and that issue stands behind the iteration's last
    ds_read_b64_tr_b16 - so the wait the compiler adds in front of the transposing reads covers only DMAs issued behind
    the PREVIOUS tile's last transposing read (what a three-stage ring of the row-major-V forms gives; the Vt forms have
    no such wait at all).  The shipped row-major-V forms do NOT meet this and are held to scratch and occupancy only;
  * persistent GEMM (wave roles: DMA waves load, store waves store, chosen by a wave-uniform branch): no VMEM load other than the LDS-DMA
    pieces; no basic block that holds both an LDS-DMA issue and a store; every `s_waitcnt vmcnt` alone in a block of its own behind a
    conditional branch (the DMA waves' side of the hand-over) - so the path the store waves take through the tile loop has no vmcnt wait;
    static LDS within 160 KiB (the dynamic part is PERSIST_LDS_BYTES in gemm.hip, held to the LDS plan by the kernel's static_assert);
  * ScratchSize 0 and the compiler's occupancy not below the recorded floor (2 for the GEMMs, 3 for attention, 4 for the
    unprescaled row-major-V attention form).

This is a lint on the assembly TEXT, not on control flow: "behind the first store" and "in front of the DMA issue" mean
later / earlier lines of the kernel, which matches execution order for these kernels because hipcc lays the k-loop, the
epilogue and the key loop's blocks out in program order.  A key loop whose shape it does not recognise (no s_barrier, or
no LDS-DMA issue behind the barrier) is reported, not passed.

    python tools/isa_audit.py [--csrc DIR] [--keep DIR] [--keyloop-all]      exit status 0 = clean, 1 = findings
    python tools/isa_audit.py --against DIR      compare gemm.hip, gemm_fp8.hip, gemm_ln.hip, conv3d.hip and radar.hip with another tree's (see compare)
"""
from __future__ import annotations

import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rald_amd", "csrc")
FILES = ("gemm.hip", "gemm_ln.hip", "attention.hip")
GEMM, KEYLOOP, RESOURCES, PERSIST = "gemm", "keyloop", "resources", "persist"
EPI = {"EPI_BF16": 0, "EPI_GEGLU": 3, "EPI_SOFTMAX64": 4}          # kernels.h

# (file, kernel, template arguments, label, minimum occupancy, kind).  kind: GEMM = loads and waits behind the first store; KEYLOOP = loads
# behind the first store and the key loop; RESOURCES = scratch and occupancy only.  The row-major-V attention forms are RESOURCES: their
# two-stage loop still has the compiler's mid-tile `vmcnt(0)` (a three-stage ring passes KEYLOOP but is not
# shipped without a timing); `--keyloop-all` reports it.
HOT = (
    ("gemm.hip", "gemm_nt_glds_kernel", (256, 256, 4, 2, 2, EPI["EPI_GEGLU"]), "FF1 (EPI_GEGLU)", 2, GEMM),
    ("gemm.hip", "gemm_nt_glds_kernel", (256, 256, 4, 2, 2, EPI["EPI_BF16"]), "q|k|v (EPI_BF16)", 2, GEMM),
    ("gemm.hip", "gemm_nt_glds_kernel", (256, 256, 4, 2, 2, EPI["EPI_SOFTMAX64"]), "folded cross-attention (EPI_SOFTMAX64)", 2, GEMM),
    ("gemm.hip", "gemm_nt_persist_kernel", (EPI["EPI_GEGLU"],), "FF1, persistent tile loop (EPI_GEGLU)", 2, PERSIST),
    ("gemm.hip", "gemm_nt_persist_kernel", (EPI["EPI_BF16"],), "q|k|v, persistent tile loop (EPI_BF16)", 2, PERSIST),
    ("gemm.hip", "gemm_nt_persist_kernel", (EPI["EPI_SOFTMAX64"],), "folded cross-attention, persistent tile loop, batched (EPI_SOFTMAX64)", 2, PERSIST),
    ("gemm_ln.hip", "gemm_resid_ln_kernel", (128, 2, 4, 0, 1), "residual + LN, 128 rows, bf16, group-uniform", 2, GEMM),
    ("gemm_ln.hip", "gemm_resid_ln_kernel", (128, 2, 4, 1, 1), "residual + LN, 128 rows, MXFP8, group-uniform", 2, GEMM),
    ("gemm_ln.hip", "gemm_resid_ln_kernel", (64, 1, 8, 0, 1), "residual + LN, 64 rows, bf16, group-uniform", 2, GEMM),
    ("gemm_ln.hip", "gemm_resid_ln_kernel", (64, 1, 8, 1, 1), "residual + LN, 64 rows, MXFP8, group-uniform", 2, GEMM),
    ("attention.hip", "attention_d64_kernel", (1, 1, 0), "self-attention (prescaled, row-major V)", 3, RESOURCES),
    ("attention.hip", "attention_d64_kernel", (1, 0, 0), "cross-attention (prescaled, Vt)", 3, KEYLOOP),
    ("attention.hip", "attention_d64_kernel", (1, 1, 1), "set-encoder attention (prescaled, row-major V, fp16)", 3, RESOURCES),
    ("attention.hip", "attention_d64_kernel", (0, 1, 0), "attention (unprescaled, row-major V)", 4, RESOURCES),
    ("attention.hip", "attention_d64_kernel", (0, 0, 0), "attention (unprescaled, Vt)", 3, RESOURCES),
)

_VMEM_LOAD = re.compile(r"(global|buffer|flat)_load")
_VMEM_STORE = re.compile(r"(global|buffer|flat)_(store|atomic)")
_VMWAIT = re.compile(r"s_waitcnt\b.*\bvmcnt\(")


def makefile_flags(csrc: str):
    """(compiler, flags) as rald_amd/csrc/Makefile builds the library."""
    text = open(os.path.join(csrc, "Makefile"), encoding="utf-8").read()
    var = {}
    for m in re.finditer(r"^(\w+)\s*[?:]?=\s*(.*)$", text, flags=re.M):
        var.setdefault(m.group(1), m.group(2).strip())
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["CXXFLAGS"])
    return os.environ.get("HIPCC", var.get("HIPCC", "hipcc")), flags.split()


def compile_to_asm(csrc: str, name: str, out_dir: str) -> str:
    hipcc, flags = makefile_flags(csrc)
    out = os.path.join(out_dir, name.replace(".hip", ".s"))
    cmd = [hipcc, *flags, "--offload-device-only", "-S", name, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stderr[-4000:]}")
    return open(out, encoding="utf-8").read()


def kernel_texts(asm: str) -> dict:
    """mangled symbol -> the kernel's text, from its label to its resource comment block."""
    out = {}
    for m in re.finditer(r"^(_ZN4rald\w+):\s*; @", asm, flags=re.M):        # (a function label; device variables carry no `; @`)
        end = asm.find("\n\t.section", m.end())
        tail = asm.find("; Occupancy:", m.end())
        stop = asm.find("\n", tail) if tail != -1 else end
        out[m.group(1)] = asm[m.start():stop if stop != -1 else len(asm)]
    return out


def template_id(symbol: str):
    """(kernel name, template argument tuple) of a kernel whose template arguments are all integers or bools, else None."""
    m = re.match(r"_ZN4rald\d+(\w+?)I((?:L[ib]\d+E)+)E\w*$", symbol)
    return (m.group(1), tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2)))) if m else None


def split_kernels(asm: str) -> dict:
    """(kernel name, template argument tuple) -> the kernel's text."""
    return {template_id(sym): text for sym, text in kernel_texts(asm).items() if template_id(sym)}


def _instructions(text: str) -> list:
    """Instruction and basic-block-label lines of a kernel, in text order (directives and comment lines dropped)."""
    out = []
    for line in text.split("\n"):
        s = line.split(";")[0].strip()
        if s and (re.match(r"\.LBB\d+_\d+:$", s) or not s.startswith((".", "//"))):
            out.append(s)
    return out


def audit_kernel(text: str, min_occupancy: int, kind: str) -> list:
    findings = []
    ins = _instructions(text)
    # ---- no VMEM load behind the first store
    first_store = next((i for i, s in enumerate(ins) if _VMEM_STORE.match(s)), None)
    if first_store is not None and kind != RESOURCES:
        late = [s for s in ins[first_store + 1:] if _VMEM_LOAD.match(s)]
        waits = [s for s in ins[first_store + 1:] if _VMWAIT.match(s)]
        if late:
            findings.append(f"{len(late)} VMEM load(s) behind the first store (first: `{late[0]}`), {len(waits)} vmcnt wait(s) behind it")
        elif waits and kind == GEMM:            # (attention: the key-split and the whole-row exits are two store sites of one kernel)
            findings.append(f"{len(waits)} vmcnt wait(s) behind the first store (first: `{waits[0]}`)")
    # ---- resources
    m = re.search(r"; ScratchSize: (\d+)", text)
    if m is None or int(m.group(1)) != 0:
        findings.append(f"ScratchSize {m.group(1) if m else '?'} (must be 0)")
    m = re.search(r"; Occupancy: (\d+)", text)
    if m is None or int(m.group(1)) < min_occupancy:
        findings.append(f"occupancy {m.group(1) if m else '?'} below {min_occupancy}")
    if kind == KEYLOOP:
        findings += audit_key_loop(ins)
    if kind == PERSIST:
        findings += audit_persistent(ins, text)
    return findings


def audit_persistent(ins: list, text: str) -> list:
    """Wave roles of the persistent GEMM, as far as the text shows them (see the module docstring)."""
    findings = []
    plain = [s for s in ins if _VMEM_LOAD.match(s) and not s.startswith("global_load_lds")]
    if plain:
        findings.append(f"{len(plain)} VMEM load(s) that are not LDS-DMA pieces (first: `{plain[0]}`)")
    blocks, cur = [], []
    for s in ins:
        if re.match(r"\.LBB\d+_\d+:$", s):
            blocks.append(cur)
            cur = []
            continue
        cur.append(s)
        if _BLOCK_END.match(s):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    blocks = [b for b in blocks if b]
    for i, b in enumerate(blocks):
        if any(s.startswith("global_load_lds") for s in b) and any(_VMEM_STORE.match(s) for s in b):
            findings.append("a basic block issues LDS-DMA pieces and stores: the roles are not separated")
        if any(_VMWAIT.match(s) for s in b):
            alone = all(s.startswith(("s_waitcnt", "s_branch", "s_nop", "s_mov_b")) for s in b)      # (s_mov: the structurizer's flags)
            guarded = i > 0 and blocks[i - 1][-1].startswith("s_cbranch")
            if not (alone and guarded):
                findings.append(f"`{next(s for s in b if _VMWAIT.match(s))}` is not alone behind a conditional branch: the store waves would run it")
    # the output stores are inline assembly, so the compiler's hazard recogniser does not see them: a VALU write to the data registers of
    # a store of more than 8 bytes needs two wait states behind the store
    for i, s in enumerate(ins):
        m = re.match(r"global_store_dwordx[34] \S+ v\[(\d+):(\d+)\]", s)
        for t in ins[i + 1:i + 3] if m else ():
            if t.startswith("s_nop"):
                break
            w = re.match(r"v_\S+ v(?:\[(\d+):(\d+)\]|(\d+))", t)
            if w and not (int(w.group(2) or w.group(3)) < int(m.group(1)) or int(w.group(1) or w.group(3)) > int(m.group(2))):
                findings.append(f"`{t}` writes the data registers of `{s}` within two wait states")
    m = re.search(r"; LDSByteSize: (\d+)", text)
    if m is None or int(m.group(1)) > 160 * 1024:
        findings.append(f"LDSByteSize {m.group(1) if m else '?'} above 160 KiB")
    return findings


def audit_key_loop(ins: list) -> list:
    """The key loop = the innermost loop that holds an s_barrier: from its header label to its last backward branch."""
    labels = {s[:-1]: i for i, s in enumerate(ins) if re.match(r"\.LBB\d+_\d+:$", s)}
    loops = []
    for i, s in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", s)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    loops = [(a, b) for a, b in loops if "s_barrier" in ins[a:b]]
    if not loops:
        return ["no key loop with a barrier found"]
    a, b = min(loops, key=lambda ab: ab[1] - ab[0])
    body = ins[a:b]
    barrier = body.index("s_barrier")
    dma = [i for i, s in enumerate(body) if s.startswith("global_load_lds") and i > barrier]
    tr = [i for i, s in enumerate(body) if s.startswith("ds_read_b64_tr_b16")]
    waits = [i for i, s in enumerate(body) if _VMWAIT.match(s) and i > barrier]     # (those in front of the barrier are the hand-over)
    findings = []
    if not dma:
        return ["key loop: no LDS-DMA issue behind the loop's barrier (loop shape not recognised)"]
    if waits:
        young = [i for i in waits if i > dma[0]]
        if young:
            findings.append(f"key loop: {len(young)} vmcnt wait(s) behind the iteration's DMA issue (first: `{body[young[0]]}`): "
                            "the prefetch just issued is drained in mid-tile")
        if tr and dma[0] < tr[-1]:
            findings.append("key loop: the next stage's DMA is issued in front of the tile's last ds_read_b64_tr_b16")
    return findings


def audit(csrc: str = CSRC, keep: str | None = None, keyloop_all: bool = False) -> dict:
    """label -> list of findings (empty = clean) for every hot instantiation."""
    tmp = keep or tempfile.mkdtemp(prefix="isa_audit_")
    os.makedirs(tmp, exist_ok=True)
    try:
        kernels = {name: split_kernels(compile_to_asm(csrc, name, tmp)) for name in FILES}
    finally:
        if keep is None:
            shutil.rmtree(tmp, ignore_errors=True)
    report = {}
    for fname, kernel, args, label, occ, kind in HOT:
        text = kernels[fname].get((kernel, args))
        if keyloop_all and fname == "attention.hip":
            kind = KEYLOOP
        title = f"{kernel}<{','.join(map(str, args))}>  {label}"
        report[title] = ["this instantiation is not in the build"] if text is None else audit_kernel(text, occ, kind)
    return report


# ---- comparison against another source tree (a refactor must leave the hot loops as they were) -----------------------------------
ENGINE_FILES = ("gemm.hip", "gemm_fp8.hip", "gemm_ln.hip", "conv3d.hip", "radar.hip")
# kernels whose MFMA blocks must not change (None = every value of that template argument): the GEMM entries of HOT and the other
# shipped tile shapes of the two LDS-DMA GEMMs
COMPARE_HOT = tuple((k, a) for f, k, a, *_ in HOT if f in ENGINE_FILES) + (
    ("gemm_mx8_kernel", (256, 256, 4, 2, None)), ("gemm_mx8_kernel", (128, 128, 2, 2, None)),
    ("gemm_nt_glds_kernel", (128, 128, 2, 2, 2, None)), ("gemm_nt_glds_kernel", (64, 128, 2, 2, 3, None)),
    ("gemm_nt_glds_kernel", (64, 64, 2, 2, 8, None)),
)
# plain (non-template) kernels held to the same rule, by name: the radar encoder's convolution engines, split-K reduce and GroupNorm
COMPARE_HOT_PLAIN = ("conv3d_igemm_kernel", "conv3d_line_kernel", "conv3d_plane_kernel", "conv3d_pplane_kernel", "conv_split_reduce_kernel",
                     "gn_stats_kernel", "gn_finish_kernel", "gn_apply_kernel")
_RESOURCES = ("NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")
_REG = re.compile(r"\b[vsa](\d+|\[\d+:\d+\])|\bttmp\d+")
_BLOCK_END = re.compile(r"s_c?branch|s_endpgm|s_setpc")


def is_compare_hot(tid) -> bool:
    return tid is not None and any(tid[0] == k and len(tid[1]) == len(a) and all(y is None or x == y for x, y in zip(tid[1], a))
                                   for k, a in COMPARE_HOT)


def is_compare_hot_symbol(symbol: str) -> bool:
    """a plain kernel of COMPARE_HOT_PLAIN, by its mangled symbol (_ZN4rald<len><name>E...)"""
    m = re.match(r"_ZN4rald(\d+)", symbol)
    return bool(m) and symbol[m.end():m.end() + int(m.group(1))] in COMPARE_HOT_PLAIN


def resources(text: str) -> dict:
    return {k: (m.group(1) if (m := re.search(rf"; {k}: (\d+)", text)) else "?") for k in _RESOURCES}


def mfma_blocks(text: str) -> list:
    """The basic blocks (label or branch to branch) that hold an MFMA, registers and block labels replaced by placeholders."""
    blocks, cur = [], []
    for s in _instructions(text):
        label = re.match(r"\.LBB\d+_\d+:$", s)
        if label and cur:
            blocks.append(cur)
            cur = []
        if not label:
            cur.append(re.sub(r"\.LBB\d+_\d+", ".LBB", _REG.sub(lambda m: m.group(0)[0] + "#", s)))
            if _BLOCK_END.match(s):
                blocks.append(cur)
                cur = []
    blocks.append(cur)
    return [b for b in blocks if any(i.startswith("v_mfma") for i in b)]


def compare_kernel(old: str, new: str, hot: bool):
    """(findings, notes) for one kernel present in both trees.  Findings: a resource or the number of barriers that changed and, for a hot kernel, every MFMA
    block that is not instruction for instruction the same; the same differences of a kernel that is not hot are notes."""
    findings = [f"{k} {a} -> {b}" for k, a, b in ((k, resources(old)[k], resources(new)[k]) for k in _RESOURCES) if a != b or a == "?"]
    barriers = [sum(i == "s_barrier" for i in _instructions(t)) for t in (old, new)]
    if barriers[0] != barriers[1]:
        findings.append(f"s_barrier count {barriers[0]} -> {barriers[1]}")
    bo, bn = mfma_blocks(old), mfma_blocks(new)
    diffs = [f"{len(bo)} -> {len(bn)} MFMA blocks"] if len(bo) != len(bn) else []
    for i, (x, y) in enumerate(zip(bo, bn)):
        if x != y:
            d = next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            changed = sum(1 for t in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes() if t[0] != "equal")
            diffs.append(f"MFMA block {i} ({len(x)} -> {len(y)} instructions) differs in {changed} place(s), first at instruction {d}: "
                         f"`{x[d] if d < len(x) else '<end>'}` -> `{y[d] if d < len(y) else '<end>'}`")
    count = lambda text, blocks: len([s for s in _instructions(text) if not s.endswith(":")]) - sum(map(len, blocks))
    delta = count(new, bn) - count(old, bo)
    notes = [f"{len(bn)} MFMA block(s) {'identical' if not diffs else 'DIFFER'}, {delta:+d} instruction(s) outside them"]
    return findings + (diffs if hot else []), notes + ([] if hot else diffs)


def engine_kernels(asm_by_file: dict) -> dict:
    """mangled symbol -> the kernel's text over the assembly of all of one tree's engine files ({file name: assembly}).  Symbols are unique in
    `namespace rald`, so a kernel keeps its key whichever file holds it."""
    out = {}
    for name, asm in asm_by_file.items():
        for sym, text in kernel_texts(asm).items():
            if sym in out:
                raise RuntimeError(f"{name}: kernel symbol {sym} is defined in two engine files")
            out[sym] = text
    return out


def compare_kernels(old: dict, new: dict) -> int:
    """Prints the comparison of two trees' symbol tables (engine_kernels); returns the number of findings (kernels, and one for a symbol set that differs)."""
    print(f"{len(new)} kernel symbols" + ("" if set(old) == set(new) else
          f"; ONLY against: {sorted(set(old) - set(new))}; ONLY tree: {sorted(set(new) - set(old))}"))
    bad = int(set(old) != set(new))
    for sym in sorted(set(old) & set(new)):
        tid = template_id(sym)
        hot = is_compare_hot(tid) or is_compare_hot_symbol(sym)
        findings, notes = compare_kernel(old[sym], new[sym], hot)
        title = f"{tid[0]}<{','.join(map(str, tid[1]))}>" if tid else sym
        r = resources(new[sym])
        print(f"{'FAIL' if findings else 'ok  '}  {'hot ' if hot else '    '}{title}  vgpr {r['NumVgprs']} occ {r['Occupancy']} lds {r['LDSByteSize']}: {notes[0]}")
        for f in findings + notes[1:]:
            print("        " + f)
        bad += bool(findings)
    return bad


def compare(csrc: str, against: str, keep: str | None = None) -> int:
    """Prints the comparison of the engine files' kernels (LDS-DMA GEMMs, conv3d.hip, radar.hip) of `csrc` with those of `against`; returns the number of
    findings.  All of a tree's engine files go into one symbol table first (a file that a tree does not have is skipped for that tree), so a
    kernel that moved between files is still compared."""
    tmp = keep or tempfile.mkdtemp(prefix="isa_audit_")
    try:
        sides = []
        for tag, d in (("against", against), ("tree", csrc)):
            os.makedirs(os.path.join(tmp, tag), exist_ok=True)
            names = [n for n in ENGINE_FILES if os.path.exists(os.path.join(d, n))]
            print(f"{tag}: {', '.join(names)}")
            sides.append(engine_kernels({n: compile_to_asm(d, n, os.path.join(tmp, tag)) for n in names}))
        bad = compare_kernels(*sides)
    finally:
        if keep is None:
            shutil.rmtree(tmp, ignore_errors=True)
    print("identical resources and hot MFMA blocks" if not bad else f"{bad} kernel(s) or symbol set(s) with findings")
    return bad


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=CSRC, help="directory with the .hip sources and the Makefile")
    ap.add_argument("--keep", default=None, help="keep the assembly files in this directory")
    ap.add_argument("--keyloop-all", action="store_true", help="hold every attention form to the key-loop rule (reports the row-major-V forms' mid-tile drain)")
    ap.add_argument("--against", default=None, metavar="DIR", help="compare the engine files' kernels with those of another csrc directory "
                    "(symbols, registers, scratch, occupancy, LDS; the hot kernels' MFMA blocks instruction for instruction) instead of auditing")
    o = ap.parse_args()
    if o.against:
        return 1 if compare(o.csrc, o.against, o.keep) else 0
    report = audit(o.csrc, o.keep, o.keyloop_all)
    bad = 0
    for title, findings in report.items():
        print(("FAIL  " if findings else "ok    ") + title)
        for f in findings:
            print("        " + f)
        bad += bool(findings)
    print(f"{len(report) - bad} of {len(report)} hot kernels clean")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

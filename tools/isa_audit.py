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
  * ScratchSize 0 and the compiler's occupancy not below the recorded floor (2 for the GEMMs, 3 for attention, 4 for the
    unprescaled row-major-V attention form).

This is a lint on the assembly TEXT, not on control flow: "behind the first store" and "in front of the DMA issue" mean
later / earlier lines of the kernel, which matches execution order for these kernels because hipcc lays the k-loop, the
epilogue and the key loop's blocks out in program order.  A key loop whose shape it does not recognise (no s_barrier, or
no LDS-DMA issue behind the barrier) is reported, not passed.

    python tools/isa_audit.py [--csrc DIR] [--keep DIR] [--keyloop-all]      exit status 0 = clean, 1 = findings
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rald_amd", "csrc")
FILES = ("gemm.hip", "gemm_ln.hip", "attention.hip")
GEMM, KEYLOOP, RESOURCES = "gemm", "keyloop", "resources"
EPI = {"EPI_BF16": 0, "EPI_GEGLU": 3, "EPI_SOFTMAX64": 4}          # kernels.h

# (file, kernel, template arguments, label, minimum occupancy, kind).  kind: GEMM = loads and waits behind the first store; KEYLOOP = loads
# behind the first store and the key loop; RESOURCES = scratch and occupancy only.  The row-major-V attention forms are RESOURCES: their
# two-stage loop still has the compiler's mid-tile `vmcnt(0)` (a three-stage ring passes KEYLOOP but is not
# shipped without a timing); `--keyloop-all` reports it.
HOT = (
    ("gemm.hip", "gemm_nt_glds_kernel", (256, 256, 4, 2, 2, EPI["EPI_GEGLU"]), "FF1 (EPI_GEGLU)", 2, GEMM),
    ("gemm.hip", "gemm_nt_glds_kernel", (256, 256, 4, 2, 2, EPI["EPI_BF16"]), "q|k|v (EPI_BF16)", 2, GEMM),
    ("gemm.hip", "gemm_nt_glds_kernel", (256, 256, 4, 2, 2, EPI["EPI_SOFTMAX64"]), "folded cross-attention (EPI_SOFTMAX64)", 2, GEMM),
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


def split_kernels(asm: str) -> dict:
    """(kernel name, template argument tuple) -> the kernel's text, from its label to its resource comment block."""
    out = {}
    for m in re.finditer(r"^(_ZN4rald\d+(\w+?)I((?:L[ib]\d+E)+)E\w*):", asm, flags=re.M):
        end = asm.find("\n\t.section", m.end())
        tail = asm.find("; Occupancy:", m.end())
        stop = asm.find("\n", tail) if tail != -1 else end
        args = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(3)))
        out[(m.group(2), args)] = asm[m.start():stop if stop != -1 else len(asm)]
    return out


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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=CSRC, help="directory with the .hip sources and the Makefile")
    ap.add_argument("--keep", default=None, help="keep the assembly files in this directory")
    ap.add_argument("--keyloop-all", action="store_true", help="hold every attention form to the key-loop rule (reports the row-major-V forms' mid-tile drain)")
    o = ap.parse_args()
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

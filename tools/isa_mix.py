#!/usr/bin/env python
"""Instruction-class mix of the chain kernels' loops from the SHIPPED code object (no GPU needed):

    python tools/isa_mix.py [smcpp_amd/libsmcpp_engine.so] > profiles/r06_isa_mix.json
    python tools/isa_mix.py --loops [k_chain_ssILi1ELb0ELb1ELb0E] [smcpp_amd/libsmcpp_engine.so]     (a table, see row_loops; the
                                                            symbol is a regular expression on the MANGLED name: NPL, HYB, ALLLDS, H32)

Why: a SIMD of gfx950 issues a plain 32-bit VALU instruction of a wave64 in 2 cycles and a DPP, 64-bit (fp64 / cvt / 64-bit
integer) or cross-lane (v_readlane ...) instruction in 4 (tools/dpp_lab.hip on the box: v_add_f32 982 - 1002 G/s, v_fmac_f32_dpp /
v_mov_b32_dpp 587, v_fma_f64 583, eight wavefronts per SIMD; MI355X_MICROARCH.md: 157.3 TFLOP/s FP32 vector = 2-cycle issue).
bench.py's issue roofline therefore prices the kernel's instructions per CLASS: peak = 1024 SIMDs x 2.4 GHz / mean cycles per
instruction of the mix.  The mix is STATIC: every VALU instruction inside a loop of the kernel that contains DPP instructions (the
row / position loops of the chains), each loop weighted by its length - the loops are what executes ~all of the kernel's dynamic
instructions, and their mixes differ little from each other.  Transcendentals (v_rcp_f32: quarter rate) are listed separately.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def disassemble(so):
    d = tempfile.mkdtemp()
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}", "--unbundle"])
    return subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", co], text=True)


def classify(mn, ops):
    """-> class of one VALU instruction: 'dpp' | 'w64' | 'lane' | 'trans' | 'plain32'"""
    if "_dpp" in mn or "row_" in ops or "wave_sh" in ops or "quad_perm" in ops:
        return "dpp"
    if mn.startswith(("v_readlane", "v_writelane", "v_readfirstlane", "v_permlane")):
        return "lane"
    if re.match(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_", mn):
        return "trans"
    if re.search(r"(f64|_u64|_i64|_b64)", mn):
        return "w64"
    return "plain32"


CYCLES = {"dpp": 4, "w64": 4, "lane": 4, "trans": 8, "plain32": 2}


def kernel_mix(text, symbol_re):
    out = {}
    cur = None
    body = {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", line)
        if m:
            body[cur].append((int(m.group(3), 16), m.group(1), m.group(2)))
    for sym, ins in body.items():
        if not re.search(symbol_re, sym) or not ins:
            continue
        addr_index = {a: i for i, (a, _, _) in enumerate(ins)}
        loops = []
        for i, (a, mn, ops) in enumerate(ins):
            if mn.startswith(("s_cbranch", "s_branch")):
                try:
                    off = int(ops.split()[0])
                except (ValueError, IndexError):
                    continue
                if off >= 32768:                       # backward branch: simm16, in dwords from the next instruction
                    tgt = a + 4 + 4 * (off - 65536)
                    if tgt in addr_index:
                        loops.append((addr_index[tgt], i))
        # innermost first; count each instruction once (in the innermost loop that holds it)
        loops.sort(key=lambda l: l[1] - l[0])
        owner = [None] * len(ins)
        for k, (lo, hi) in enumerate(loops):
            for j in range(lo, hi + 1):
                if owner[j] is None:
                    owner[j] = k
        tot = {c: 0 for c in CYCLES}
        salu = 0
        nloop = 0
        for k, (lo, hi) in enumerate(loops):
            mine = [ins[j] for j in range(lo, hi + 1) if owner[j] == k]
            # the chain loops: an outer row loop holds the inner position loop, so a loop counts when IT or any loop inside it has DPP
            span = [ins[j] for j in range(lo, hi + 1)]
            if not any("_dpp" in mn for _, mn, _ in span):
                continue
            nloop += 1
            for _, mn, ops in mine:
                if mn.startswith("v_") and not mn.startswith("v_cmpx_nop"):
                    tot[classify(mn, ops)] += 1
                elif mn.startswith("s_"):
                    salu += 1
        n = sum(tot.values())
        if n == 0:
            continue
        cyc = sum(tot[c] * CYCLES[c] for c in tot) / n
        out[sym] = {"loops_with_dpp": nloop, "valu_in_those_loops": n, "salu_in_those_loops": salu, "by_class": tot,
                    "mean_issue_cycles_per_valu": cyc, "peak_ginstr_per_s": 1024 * 2.4 / cyc}
    return out


def parse(text):
    """objdump -d text -> {symbol: [(address, mnemonic, operands)]}"""
    cur, body = None, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            body[cur] = []
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", line) if cur is not None else None
        if m:
            body[cur].append((int(m.group(3), 16), m.group(1), m.group(2)))
    return body


def row_loops(ins):
    """The depth-1 loops of one kernel that hold DPP instructions - the row loops of the chains, one per direction, number format and
    jump / halo variant - as rows of a table: where the loop lies, its code bytes (what has to stay in the instruction cache while it
    runs), its VALU and SALU instructions, its branch instructions and how many of those are unconditional, and the same for the loops
    nested in it (the position loops).  A taken branch costs a lone wavefront the refetch in full, and an unconditional
    one is always taken: the table is what a change to the loops' control flow is read against.  Static counts - which branches a row
    of a given span takes is read from the listing by hand."""
    addr_index = {a: i for i, (a, _, _) in enumerate(ins)}
    loops = set()
    for i, (a, mn, ops) in enumerate(ins):
        if mn.startswith(("s_cbranch", "s_branch")):
            try:
                off = int(ops.split()[0])
            except (ValueError, IndexError):
                continue
            if off >= 32768 and a + 4 + 4 * (off - 65536) in addr_index:
                loops.add((addr_index[a + 4 + 4 * (off - 65536)], i))
    # A row loop is not one interval of addresses: what a row rarely does lies BEHIND the loop's back-edge and returns with a backward
    # branch of its own, which is no loop.  So the backward branches are merged into regions - intervals that overlap or nest are one
    # region, from its first head to its last backward branch - and the loops nested in a region are its minimal intervals.
    loops = sorted(loops)
    regions = []
    for lo, hi in loops:
        if regions and lo <= regions[-1][1]:
            regions[-1][1] = max(regions[-1][1], hi)
            regions[-1][2].append((lo, hi))
        else:
            regions.append([lo, hi, [(lo, hi)]])
    rows = []
    for lo, hi, parts in regions:
        body = ins[lo:hi + 1]
        if not any("_dpp" in mn for _, mn, _ in body):
            continue
        inner = [(l2, h2) for l2, h2 in parts if (l2, h2) != (lo, hi) and not any((l3, h3) != (l2, h2) and l2 <= l3 and h3 <= h2 for l3, h3 in parts)
                 and any("_dpp" in mn for _, mn, _ in ins[l2:h2 + 1])]
        if len(parts) == 1:
            inner = []
        in_inner = lambda j: any(l2 <= j <= h2 for l2, h2 in inner)
        br = [mn for _, mn, _ in body if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc"))]
        end = ins[hi + 1][0] if hi + 1 < len(ins) else ins[hi][0] + 4
        rows.append({"head": "%x" % ins[lo][0], "bytes": end - ins[lo][0],
                     "valu": sum(mn.startswith("v_") for _, mn, _ in body),
                     "valu_outside_inner": sum(mn.startswith("v_") and not in_inner(lo + j) for j, (_, mn, _) in enumerate(body)),
                     "salu": sum(mn.startswith("s_") and not mn.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_load", "s_buffer_load")) for _, mn, _ in body),
                     "smem": sum(mn.startswith(("s_load", "s_buffer_load")) for _, mn, _ in body),
                     "waitcnt": sum(mn.startswith("s_waitcnt") for _, mn, _ in body),
                     "vmcnt": sum(mn.startswith("s_waitcnt") and "vmcnt" in ops for _, mn, ops in body),
                     "readlane": sum(mn.startswith("v_readlane") for _, mn, _ in body),
                     "branches": len(br), "unconditional": sum(mn.startswith(("s_branch", "s_setpc", "s_swappc")) for mn in br),
                     "inner_loops": len(inner), "inner_bytes": [ins[h2 + 1][0] - ins[l2][0] for l2, h2 in inner]})
    return rows


def loops_table(so, symbol_re):
    body = parse(disassemble(so))
    for sym, ins in body.items():
        if not ins or not re.search(symbol_re, sym):
            continue
        print(sym)
        print("  %-8s %6s %5s %9s %5s %5s %5s %5s %8s %8s %6s  %s" % ("head", "bytes", "VALU", "(outside)", "SALU", "SMEM", "waits", "vmcnt", "readlane", "branches", "uncond",
                                                                  "inner loops (bytes)"))
        for r in row_loops(ins):
            print("  %-8s %6d %5d %9d %5d %5d %5d %5d %8d %8d %6d  %s" % (r["head"], r["bytes"], r["valu"], r["valu_outside_inner"], r["salu"], r["smem"], r["waitcnt"], r["vmcnt"],
                                                                          r["readlane"], r["branches"], r["unconditional"], r["inner_bytes"]))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--loops":
        rest = sys.argv[2:]
        so = rest.pop() if rest and rest[-1].endswith(".so") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smcpp_amd", "libsmcpp_engine.so")
        loops_table(so, rest[0] if rest else "k_chain_ssILi1ELb0ELb1ELb0E")
        return
    so = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smcpp_amd", "libsmcpp_engine.so")
    text = disassemble(so)
    res = {"note": "static VALU class mix of the loops that contain DPP instructions, from the shipped gfx950 code object "
                   "(tools/isa_mix.py); issue cycles per wave64 instruction: " + json.dumps(CYCLES) +
                   " (tools/dpp_lab.hip; MI355X_MICROARCH.md); peak = 1024 SIMDs x 2.4 GHz / mean cycles",
           "kernels": kernel_mix(text, r"k_chain_ss|k_span_scan")}
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()

"""Device code of every kernel translation unit of two builds, compared function by function.

    python tools/isa_vs_parent.py <parent object dir> <this tree's object dir> [--title "..."] > profiles/rNN_isa_vs_parent.txt

Both directories hold the objects build_library leaves (hydromodel_amd/csrc/_obj of each tree, same hipcc, same flags).
For each hc_inst_*.o present in both, the gfx950 code object is taken out of the bundle (llvm-objdump --offloading),
disassembled (llvm-objdump -d) and split at the function labels; a function's instruction text is its lines without
addresses, encodings and comments, and without the literal of the s_add_u32 that follows an s_getpc_b64: the low word of
the displacement to a constant table, an address that moves with the size of whatever else the code object holds.  (The
s_addc_u32 that follows carries the high word and is compared as it is: two builds whose displacements differ in it,
which takes a code object of 4 GiB, would be reported as different.)  One line per kernel: unit | kernel | instruction
counts | whether the streams differ.
The exit status is 1 when a monitoring-mode step kernel (PREDICT = false) or an RHS hook differs.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def functions(obj):
    """{demangled kernel name: [instruction text]} of the gfx950 code object bundled in `obj`"""
    with tempfile.TemporaryDirectory() as tmp:
        # the fat binary sits in a section of the host object: llvm-objdump --offloading writes its bundles next to the
        # file it is given, so it is given a copy
        host = os.path.join(tmp, "unit.o")
        shutil.copy(obj, host)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", host], check=True, capture_output=True, cwd=tmp)
        co = f"{host}.0.{TARGET}"
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "-C", co], check=True,
                              capture_output=True, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if re.fullmatch(r"L\d+|\.L\S*", m.group(1)):      # a local label inside a function
                continue
            name = m.group(1)
            out[name] = []
            pcrel = False
            continue
        if name is None or not line.startswith(("\t", " ")):
            continue
        ins = re.sub(r"//.*|;.*", "", line).strip()
        ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
        ins = re.sub(r"<[^>]*>", "", ins).strip()          # branch-target labels
        # the displacement from s_getpc_b64 to a constant table (GAMMA_TAB ...) is an address: it moves with the size of
        # whatever else the code object holds
        if pcrel and re.match(r"s_add_u32 s\d+, s\d+, 0x[0-9a-f]+$", ins):
            ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
        pcrel = ins.startswith("s_getpc_b64")
        if ins and not ins.startswith("s_code_end"):
            out[name].append(ins)
    return {re.sub(r"^void |\(.*$", "", k): v for k, v in out.items() if v and "kernel" in k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    units = sorted(f for f in os.listdir(a.this) if f.startswith("hc_inst_") and f.endswith(".o")
                   and os.path.exists(os.path.join(a.parent, f)))
    rows, moved = [], []
    for u in units:
        fa, fb = functions(os.path.join(a.parent, u)), functions(os.path.join(a.this, u))
        for k in sorted(set(fa) | set(fb)):
            ia, ib = fa.get(k), fb.get(k)
            if ia is None or ib is None:
                diff = "(only in one build)"
            elif ia == ib:
                diff = "none"
            else:
                diff = "(another instruction stream)"
            rows.append(f"{u[:-2]} | {k} | {len(ia or [])} -> {len(ib or [])} | {diff}")
            t = re.search(r"step_kernel<\d+, \w+, \d+, (\w+)", k)
            if diff != "none" and (t is None or t.group(1) == "false"):
                moved.append(k)
    if a.title:
        print(a.title)
    print("# unit | kernel | instructions parent -> this tree | instructions that differ")
    print("\n".join(rows))
    if moved:
        print(f"{len(moved)} monitoring-mode step kernels / hooks differ", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

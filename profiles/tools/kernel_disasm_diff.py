#!/usr/bin/env python3
"""Which functions of the gfx950 code object have other instructions in one build than in another.

    python profiles/tools/kernel_disasm_diff.py parent/csrc/p3d_capi.o this/csrc/p3d_capi.o

Extracts the code object of each (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle), disassembles it
(llvm-objdump -d) and compares the text per function label with addresses, branch targets and pc-relative literals
masked: what is left differs only where the instructions do.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def disassemble(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.co")
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(d, "copy.o")])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        return subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)


def functions(text):
    out, cur, after_getpc = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip() or line.strip() == "...":  # (... : the zero padding behind the last function of a section)
            continue
        line = re.sub(r"//.*$", "", line).strip()                      # address comments
        line = re.sub(r"<[^>]+>", "<label>", line)                     # branch targets by label
        line = re.sub(r"^(s_c?branch\S*|s_call\S*)\s.*$", r"\1 <target>", line)
        if after_getpc and re.match(r"s_addc?_u32 ", line):            # the pc-relative literal behind s_getpc_b64
            line = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<lit>", line)
        after_getpc = 2 if line.startswith("s_getpc_b64") else max(0, after_getpc - 1)
        cur.append(line)
    return out


def main():
    a, b = functions(disassemble(sys.argv[1])), functions(disassemble(sys.argv[2]))
    print("%d functions in %s, %d in %s" % (len(a), sys.argv[1], len(b), sys.argv[2]))
    same = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s (%d instructions)" % (sys.argv[1] if name in a else sys.argv[2], name, len(a.get(name) or b.get(name))))
        elif a[name] != b[name]:
            print("differs: %s (%d / %d instructions)" % (name, len(a[name]), len(b[name])))
        else:
            same += 1
    print("%d functions identical after masking, %d instructions" % (same, sum(len(a[n]) for n in a if n in b and a[n] == b[n])))


if __name__ == "__main__":
    main()

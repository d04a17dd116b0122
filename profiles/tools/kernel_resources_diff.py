#!/usr/bin/env python3
"""Which kernels of the device translation unit report other resources in one build than in another.

    make -C p3d-raytracer_amd -B csrc/p3d_capi.o EXTRA=-Rpass-analysis=kernel-resource-usage 2> this.log     (in each checkout)
    python profiles/tools/kernel_resources_diff.py parent.log this.log

Reads the compiler's remarks (Function Name, TotalSGPRs, VGPRs, AGPRs, ScratchSize, Dynamic Stack, Occupancy, spills, LDS)
and prints every function whose fields differ, or that only one of the two builds has.
"""
import re
import sys


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, value = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = value
            out.setdefault(cur, [])
        elif cur:
            out[cur].append((key, value))
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    print("%d functions in %s, %d in %s" % (len(a), sys.argv[1], len(b), sys.argv[2]))
    for name in sorted(set(a) | set(b)):
        if a.get(name) != b.get(name):
            print(name)
            print("  ", a.get(name))
            print("  ", b.get(name))


if __name__ == "__main__":
    main()

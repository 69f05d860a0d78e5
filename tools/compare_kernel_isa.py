#!/usr/bin/env python3
"""Which kernels of two `hipcc -O3 -std=c++17 -S --cuda-device-only --offload-arch=gfx950` listings of
softrod_capi.hip differ: per kernel symbol the instruction list (hot_path_isa.function_body, local labels
renumbered) and the resource block (kernel descriptor, "Kernel info" comments, spill counts).

  python tools/compare_kernel_isa.py before.s after.s
"""
import re
import sys

import hot_path_isa


def kernels(asm: str):
    asm = re.sub(r"^(?=softrod_\w+:)", "_ZN7", asm, flags=re.M)      # C-linkage kernels, for function_body's pattern
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, flags=re.M):
        ins, labels = hot_path_isa.function_body(asm, name + ":")
        order = {l: f"L{k}" for k, l in enumerate(sorted(labels, key=labels.get))}
        ins = [re.sub(r"\.LBB\d+_\d+", lambda m: order[m.group(0)], x) for x in ins]
        desc = re.search(rf"\.amdhsa_kernel {re.escape(name)}\n(.*?)\.end_amdhsa_kernel.*?; Kernel info:\n((?:;[^\n]*\n)+)",
                         asm, flags=re.S)
        meta = re.search(rf"\.name:\s+{re.escape(name)}\n.*?\.sgpr_spill_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)",
                         asm, flags=re.S)
        out[name] = (ins, sorted(labels.values()), desc.groups(), meta.groups())
    return out


def summary(k):
    info = dict(re.findall(r"; (\w+): (\d+)", k[2][1]))
    return {x: int(info[x]) for x in ("NumVgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize")} | {"spills": k[3]}


if __name__ == "__main__":
    a, b = (kernels(open(p).read()) for p in sys.argv[1:3])
    differ = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
    print(f"{len(set(a) | set(b))} kernel symbols compared, {len(differ)} differ")
    for n in differ:
        print(" ", n, summary(a[n]) if n in a else "absent", "->", summary(b[n]) if n in b else "absent")

#!/usr/bin/env python
"""Per-kernel fp32 arithmetic of csrc/*.hip as the compiler emits it for gfx950: how many separate multiplies, adds and fused
multiply-adds every kernel holds, and which of them take a scalar the kernel loaded (an argument such as beta, or a per-row value
read through the scalar cache) -- the instructions that show whether a source-level product was fused into the sum that follows
it (DESIGN.md "What is rounded once").  CPU only (hipcc cross-compiles).

    python tools/float_ops.py neighborretr_amd/csrc/nr_sinknorm.hip [...]      # or .s files compiled earlier

Two builds whose rows agree compute the same roundings.  Rows may differ and the roundings still agree: a value computed once
where the other build computes it twice, another unrolling of a loop (the integer division of a grid-stride loop is float code)."""
import os
import re
import subprocess
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (("mul", r"v_(pk_)?mul_f(32|64)"), ("add", r"v_(pk_)?(add|sub|subrev)_f(32|64)"),
         ("fma", r"v_(pk_)?(fma|fmac|fmamk|fmaak)_f(32|64)"))


def assembly(src):
    if src.endswith(".s"):
        return open(src).read()
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "-S",
           "--cuda-device-only", src, "-o", "-"] + os.environ.get("NR_EXTRA_FLAGS", "").split()
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def demangle(name):
    out = subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip() or name
    return re.sub(r"^void ", "", out)


def sgprs(operands):
    """The scalar registers an operand string names: s7, and every register of a range s[4:7]."""
    ranges = {int(i) for lo, hi in re.findall(r"s\[(\d+):(\d+)\]", operands) for i in range(int(lo), int(hi) + 1)}
    return ranges | {int(i) for i in re.findall(r"\bs(\d+)\b", operands)}


def kernels(text):
    """name -> (counts of mul / add / fma, counts of those of them that read a loaded scalar, by opcode)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", text, re.S | re.M):
        total, scalar, loaded = Counter(), Counter(), set()
        for line in m.group(2).splitlines():
            ins = line.split(";")[0].split()
            if not ins:
                continue
            op, args = ins[0], " ".join(ins[1:])
            dst = args.split(",")[0].strip()
            if op.startswith("s_load_") or op.startswith("s_buffer_load_"):
                loaded |= sgprs(dst)
            elif op in ("s_mov_b32", "s_mov_b64") and sgprs(args.split(",", 1)[1]) and sgprs(args.split(",", 1)[1]) <= loaded:
                loaded |= sgprs(dst)                           # a copy of a loaded scalar (a pair for a packed operation)
            elif op.startswith("s_"):
                loaded -= sgprs(dst)                           # overwritten by a constant or an integer result
            for kind, pat in KINDS:
                if re.fullmatch(pat + r"(_e32|_e64)?", op):
                    total[kind] += 2 if "_pk_" in op else 1       # a packed instruction is two operations
                    if sgprs(args.split(",", 1)[1] if "," in args else "") & loaded:
                        scalar[re.sub(r"_e(32|64)$", "", op)] += 1
        out[demangle(m.group(1))] = (total, scalar)
    return out


def main():
    for src in sys.argv[1:]:
        print(f"{os.path.basename(src)}")
        for name, (total, scalar) in sorted(kernels(assembly(src)).items()):
            with_scalar = ", ".join(f"{n} {op}" for op, n in sorted(scalar.items())) or "-"
            print(f"  {name[:110]:110s} mul {total['mul']:3d}  add {total['add']:3d}  fma {total['fma']:3d}   with a loaded scalar: {with_scalar}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Are the kernels of two gfx950 code objects the same instructions?  Disassembles both (llvm-objdump -d), drops addresses,
raw encodings, branch-target labels and objdump's "..." padding marks, and compares function by function.  A template
parameter added with a default changes mangled names only: --strip removes such a fragment from the names of the second file.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DDSMI_BUILD -fvisibility=hidden --cuda-device-only -c score.hip -o x.co
    clang-offload-bundler --unbundle --type=o --input=x.co --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=x.elf
    python tools/same_isa.py before.elf after.elf --strip ELb0E:E
"""
import argparse
import re
import subprocess


def functions(path, objdump):
    out = subprocess.run([objdump, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    fs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1)
            fs[cur] = []
            continue
        ins = line.split("//")[0].strip()
        if cur and ins and ins != "...":
            fs[cur].append(re.sub(r"<[^>]*>", "<L>", ins))
    return fs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--strip", default="", help="OLD:NEW replacement applied to the second file's names")
    ap.add_argument("--objdump", default="/opt/rocm/llvm/bin/llvm-objdump")
    a = ap.parse_args()
    old, _, new = a.strip.partition(":")
    before = functions(a.before, a.objdump)
    after = {(k.replace(old, new) if old else k): v for k, v in functions(a.after, a.objdump).items()}
    same = True
    for name, ins in before.items():
        other = after.get(name)
        verdict = "identical" if other == ins else ("missing" if other is None else "DIFFERENT")
        same &= other == ins
        print("%-8s %6d instructions  %s" % (verdict, len(ins), name))
    print("only in the second:", sorted(set(after) - set(before)))
    raise SystemExit(0 if same else 1)


if __name__ == "__main__":
    main()

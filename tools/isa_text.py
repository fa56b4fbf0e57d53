#!/usr/bin/env python3
"""Text of the kernels in a gfx950 assembly listing, normalised so that two builds can be compared function by function
(the procedure of docs/MEASUREMENTS.md): every line between a function's label and its `.Lfunc_end`, comments and directives
dropped, the function's own number in `.LBB<fn>_<block>` and every `.Ltmp` number masked.

usage: isa_text.py <file.s> [prefix]        prints {mangled name: [lines, sha256]} as JSON for the functions whose name starts with
                                            one of the comma-separated prefixes (default: K1's, _ZN4p25k10k_frontendI and _ZN4p25k7k_chunkI)
(make -C p25rx_amd/csrc asm writes /tmp/p25fe_api-hip-amdgcn-amd-amdhsa-gfx950.s)"""
import hashlib
import json
import re
import sys

K1_PREFIXES = ("_ZN4p25k10k_frontendI", "_ZN4p25k7k_chunkI")


def functions(path, prefixes=K1_PREFIXES):
    src = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n", src, re.M):
        name = m.group(1)
        if not name.startswith(tuple(prefixes)):
            continue
        end = src.find(".Lfunc_end", m.end())
        if end < 0:                                                  # (a data symbol behind the last function)
            continue
        lines = []
        for l in src[m.end():end].split("\n"):
            s = l.split(";")[0].strip()
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue
            s = re.sub(r"\.LBB\d+_", ".LBB_", s)
            s = re.sub(r"\.Ltmp\d+", ".Ltmp", s)
            lines.append(re.sub(r"\s+", " ", s))
        out[name] = [len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()]
    return out


if __name__ == "__main__":
    pre = tuple(sys.argv[2].split(",")) if len(sys.argv) > 2 else K1_PREFIXES
    json.dump(functions(sys.argv[1], pre), sys.stdout, indent=1, sort_keys=True)
    print()

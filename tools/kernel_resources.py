#!/usr/bin/env python3
"""Tabulate the compiler's kernel-resource remarks of one HIP source (no GPU needed).

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only \\
        -Rpass-analysis=kernel-resource-usage -c -o /dev/null blend.hip 2> remarks.txt
    python tools/kernel_resources.py remarks.txt [other_remarks.txt]

One file: a table (kernel, VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy in waves per
SIMD, LDS bytes per block).  Two files: the kernels of the first whose row differs in the second,
or "identical" (profiles/median_resources.txt was made this way from the parent's blend.hip and
this tree's)."""
from __future__ import annotations

import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"),
          ("scratch", r"ScratchSize \[bytes/lane\]"), ("occupancy", r"Occupancy \[waves/SIMD\]"),
          ("LDS", r"LDS Size \[bytes/block\]"))


def demangle(name: str) -> str:
    try:
        out = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return name
    out = out.strip().replace("(anonymous namespace)::", "")
    return re.sub(r"^void |\(.*$", "", out)


def parse(path: str) -> dict:
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(demangle(m.group(1)), {})
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(r"remark: .*\b" + pat + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    return rows


def table(rows: dict) -> str:
    w = max(len(k) for k in rows)
    head = f"{'kernel':<{w}}  " + "  ".join(f"{k:>9}" for k, _ in FIELDS)
    lines = [head]
    for name in sorted(rows):
        lines.append(f"{name:<{w}}  " + "  ".join(f"{rows[name].get(k, -1):>9}" for k, _ in FIELDS))
    return "\n".join(lines)


def main(argv) -> int:
    if len(argv) not in (2, 3):
        print(__doc__)
        return 2
    a = parse(argv[1])
    print(table(a))
    if len(argv) == 3:
        b = parse(argv[2])
        diff = [k for k in a if k in b and a[k] != b[k]]
        print(f"\nkernels of {argv[1]} also in {argv[2]}: {sum(k in b for k in a)}; "
              + ("rows identical" if not diff else "rows that differ: " + ", ".join(diff)))
        print(f"kernels only in {argv[2]}: " + (", ".join(sorted(set(b) - set(a))) or "none"))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

#!/usr/bin/env python3
"""Per-kernel register / spill / occupancy table of one HIP source (hipcc
-Rpass-analysis=kernel-resource-usage), for checking an instance's register budget after a
change.  Usage: python3 tools/kres.py csrc/fc_kernels.hip [filter]"""
import re
import subprocess
import sys


def parse_remarks(text):
    """Rows (one dict per kernel, "name" demangled) of a kernel-resource-usage remark stream."""
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: (.+?) \[-Rpass", line)  # (keys such as "ScratchSize [bytes/lane]" hold brackets)
        if not m:
            continue
        key, _, val = m.group(1).partition(":")
        key, val = key.strip(), val.strip()
        if key == "Function Name":
            cur = {"name": subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip()}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    return rows


def format_row(r):
    return (f'{r["name"]:<60} VGPR {r.get("VGPRs", "?"):>4} AGPR {r.get("AGPRs", "?"):>3} '
            f'vspill {r.get("VGPRs Spill", "?"):>3} sspill {r.get("SGPRs Spill", "?"):>4} '
            f'scratch {r.get("ScratchSize [bytes/lane]", "?"):>4} occ {r.get("Occupancy [waves/SIMD]", "?")} '
            f'lds {r.get("LDS Size [bytes/block]", "?")} sgpr {r.get("TotalSGPRs", "?")}')


def main(argv):
    src = argv[1]
    flt = argv[2] if len(argv) > 2 else ""
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o",
                          "/tmp/kres.o", src, "-Rpass-analysis=kernel-resource-usage"] + argv[3:],
                         capture_output=True, text=True)
    for r in parse_remarks(res.stderr):
        if flt in r["name"]:
            print(format_row(r))


if __name__ == "__main__":
    main(sys.argv)

#!/usr/bin/env python3
"""Static instruction mix of a kernel's main loop, from a device assembly listing
(hipcc --cuda-device-only -S).  For the named kernel instance it prints the resource figures,
the instruction totals by class of its largest outermost loop (the batch loop of flip2_kernel)
and of every loop nested in it, and, in a listing of the phase-profile build (FC_LIB_VARIANT=prof),
the totals of the regions between the stamps, in listing order (the block layout follows the
source order only roughly: read those as a guide).

Instructions are classed by prefix alone; most of the loop runs about once per batch, so the
static totals are a usable proxy for the dynamic ones (SQ_INSTS_* of tools/pmc_lds.sh confirm).

Usage: python3 tools/loop_mix.py LISTING.s 'flip2_kernel<8, 4, false, false, false, false>'
           [--remarks FILE]   the compile's -Rpass-analysis=kernel-resource-usage output (adds spills)
           [--marker REGEX]   the instruction that separates regions (default: the stamps' clock read)
           [--by-line]        per source line, largest first (needs a listing with line tables)
           [--top N]          rows of the per-line table (default 40; 0: all)
           [--sort KEY]       rank the per-line table by "issue" (VALU + SALU + LDS, the default) or by
                              "scalar" (SALU + s_waitcnt + s_nop + branches: what the vector count leaves out)

--by-line attributes every instruction of each large outermost loop (a kernel that carries its body
twice, as the lean flip2_kernel instances do, has two batch loops: both are listed) to the source
file and line of the .loc directive in force, which for inlined code is the innermost callee's
line: every vote shows under the one line of its helper.  The column pairs counts the round trips
of a lane mask through a 0 / 1 register: a v_cmp_ne_u32 mask', 0, v whose v was last written, in
the same block, by v_cndmask_b32 v, 0, 1, mask.  The two instructions give back the mask they
started from; they are what a vote over a bool composed per lane costs beyond its compares
(fc_device.h, vote), and each pair is charged to the line of its compare.  The columns wait, nop
and branch count s_waitcnt, s_nop and the branch instructions.  The column spill counts the
v_readlane_b32 / v_writelane_b32 that move a scalar register out of or into the kernel's SGPR-spill
registers: the vector registers that, in the whole kernel, only v_writelane_b32 writes (a reload is
a vector issue slot of the loop that does no chain work; they are VALU and are counted there too).
The detection is a heuristic: a destination is the first operand of the v_*, ds_read / ds_*_rtn, global,
buffer, flat and scratch load families only, so a register that some other writer (v_swap_b32's second
operand, ds_consume / ds_append, image or tbuffer loads) shares with v_writelane_b32 would be misreported.
The listing it needs:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -gline-tables-only --cuda-device-only -S \
        -o flip2.s flipcomplexityempirical_amd/csrc/fc_flip2.hip

Line tables do not change the code: the instruction totals equal those of a listing without them.
It stands in for a ranking by sampled program counters where those cannot be had: static counts,
so a line inside a loop that runs often weighs more than its row shows.
"""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402

CLASSES = ["VALU", "SALU", "SMEM", "LDS", "VMEM", "branch", "wait/nop", "other"]
# first match wins
PREFIXES = [("s_cbranch", "branch"), ("s_branch", "branch"), ("s_setpc", "branch"), ("s_swappc", "branch"),
            ("s_call", "branch"), ("s_endpgm", "branch"),
            ("s_waitcnt", "wait/nop"), ("s_nop", "wait/nop"), ("s_sleep", "wait/nop"),
            ("s_load", "SMEM"), ("s_buffer_load", "SMEM"), ("s_memtime", "SMEM"), ("s_memrealtime", "SMEM"),
            ("s_", "SALU"), ("v_", "VALU"), ("ds_", "LDS"),
            ("global_", "VMEM"), ("flat_", "VMEM"), ("buffer_", "VMEM"), ("scratch_", "VMEM")]


def classify(mn):
    for pre, cls in PREFIXES:
        if mn.startswith(pre):
            return cls
    return "other"


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def kernel_body(lines, flt):
    """(mangled name, demangled name, body lines, info lines) of the one kernel matching flt."""
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := re.match(r"^(_Z\w+):\s", l))]
    dm = demangle([n for _, n in starts])
    hits = [(i, n) for i, n in starts if flt in dm[n]]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {flt!r}:\n" + "\n".join(dm[n] for _, n in hits[:40]))
    i0, name = hits[0]
    i1 = next(i for i in range(i0, len(lines)) if ".end_amdhsa_kernel" in lines[i] or lines[i].startswith(".Lfunc_end"))
    k = next((i for i in range(i1, min(i1 + 80, len(lines))) if lines[i].startswith("; Kernel info")), None)
    info = []
    if k is not None:
        for l in lines[k + 1:k + 40]:
            if not l.startswith(";"):
                break
            info.append(l[1:].strip())
    return name, dm[name], lines[i0 + 1:i1], info


def parse_blocks(body):
    """Blocks in listing order: {"label", "loops": headers of the enclosing loops, outermost first,
    "insts": mnemonics}.  The loop nest is read from the compiler's block comments."""
    blocks, cur, pending, loc = [], None, None, None
    for l in body:
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)(.*)", l)
        if m:
            cur = {"label": m.group(1) or f"bb.{m.group(2)}", "loops": [], "insts": [], "full": [], "self": False}
            blocks.append(cur)
            pending = cur
            l = ";" + m.group(3)
        s = l.strip()
        if s.startswith(";"):
            if pending is not None:
                for h, d in re.findall(r"(?:Parent Loop|in Loop: Header=)\s*(BB\d+_\d+) Depth[= ](\d+)", s):
                    pending["loops"].append((int(d), h))
                if re.search(r"This (Inner )?Loop Header: Depth=(\d+)", s):
                    d = int(re.search(r"Header: Depth=(\d+)", s).group(1))
                    pending["loops"].append((d, pending["label"]))
            continue
        if s.startswith(".loc"):
            f = s.split()
            loc = (int(f[1]), int(f[2]))
        if not s or s.startswith("."):
            continue
        pending = None
        if cur is not None:
            cur["insts"].append(s.split()[0])
            cur["full"].append((s.split(";")[0].strip(), loc))
    for b in blocks:
        b["loops"] = [h for _, h in sorted(set(b["loops"]))]
    # "in Loop: Header=H Depth=d" names only the innermost loop: complete the chain from H's own
    chain = {b["label"]: b["loops"] for b in blocks if b["loops"] and b["loops"][-1] == b["label"]}
    for b in blocks:
        if b["loops"] and b["loops"][-1] in chain:
            b["loops"] = chain[b["loops"][-1]]
    return blocks


def mix(insts):
    t = dict.fromkeys(CLASSES, 0)
    for mn in insts:
        t[classify(mn)] += 1
    return t


def file_table(lines):
    """{file number: path} of the listing's .file directives."""
    out = {}
    for l in lines:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            out[int(m.group(1))] = os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2)
    return out


SEL01 = re.compile(r"^v_cndmask_b32\w*\s+(v\d+), 0, 1, (?:s\[|vcc)")
CMP0 = re.compile(r"^v_cmp_ne_u32\w*\s+(?:s\[\d+:\d+\]|vcc), 0, (v\d+)$")
DEST = re.compile(r"^v_\w+\s+(v\d+)\b")
# an instruction's first operand where it is a vector destination (single register or range)
VDEST = re.compile(r"^(?:v_|ds_read|ds_bpermute|ds_permute|ds_\w+_rtn|global_load|global_atomic\w+_rtn|buffer_load|flat_load|"
                   r"scratch_load)\w*\s+v(?:(\d+)|\[(\d+):(\d+)\])")
LANE_MOVE = re.compile(r"^v_(readlane|writelane)_b32\s+(\w+), (\w+),")


def spill_registers(blocks):
    """The kernel's SGPR-spill VGPRs: written by v_writelane_b32 and by nothing else."""
    lane_written, written = set(), set()
    for b in blocks:
        for text, _ in b["full"]:
            m = VDEST.match(text)
            if not m:
                continue
            regs = {int(m.group(1))} if m.group(1) else set(range(int(m.group(2)), int(m.group(3)) + 1))
            (lane_written if text.startswith("v_writelane_b32") else written).update(regs)
    return {f"v{r}" for r in lane_written - written}


def is_spill_move(text, spill):
    m = LANE_MOVE.match(text)
    return bool(m) and (m.group(2) if m.group(1) == "writelane" else m.group(3)) in spill


SORT_KEYS = {"issue": ("VALU", "SALU", "LDS"), "scalar": ("SALU", "wait", "nop", "branch")}


def by_line(inl, files, top, spill=frozenset(), sort="issue"):
    """Per-line table of the blocks inl by instruction class, the SGPR-spill lane moves (spill) and
    the mask round trips (pairs)."""
    cols = ("VALU", "SALU", "LDS", "wait", "nop", "branch", "spill", "pairs", "all")
    tab = {}
    for b in inl:
        sel01 = set()  # registers holding a mask as 0 / 1
        for text, loc in b["full"]:
            t = tab.setdefault(loc, dict.fromkeys(cols, 0))
            mn = text.split()[0]
            cls = "wait" if mn.startswith("s_waitcnt") else "nop" if mn.startswith("s_nop") else classify(mn)
            if cls in t:
                t[cls] += 1
            t["all"] += 1
            t["spill"] += is_spill_move(text, spill)
            if (m := CMP0.match(text)) and m.group(1) in sel01:
                t["pairs"] += 1
            if m := DEST.match(text):
                sel01.discard(m.group(1))
            if m := SEL01.match(text):
                sel01.add(m.group(1))
    rows = sorted(tab.items(), key=lambda kv: (-sum(kv[1][c] for c in SORT_KEYS[sort]), str(kv[0])))
    fmt = lambda name, t: f"{name:<44}" + "".join(f"{t[c]:>7}" for c in cols)
    print(f"{'file:line':<44}" + "".join(f"{c:>7}" for c in cols))
    for loc, t in rows[:top or None]:
        print(fmt("(no line)" if loc is None else f"{os.path.basename(files.get(loc[0], str(loc[0])))}:{loc[1]}", t))
    print(fmt(f"total ({len(rows)} lines)", {c: sum(t[c] for t in tab.values()) for c in cols}))
    for loc, t in rows:
        if t["pairs"] and rows.index((loc, t)) >= (top or len(rows)):
            print(fmt(f"  (below the cut) {os.path.basename(files.get(loc[0], str(loc[0])))}:{loc[1]}", t))


def row(label, t):
    return f"{label:<28}" + "".join(f"{t[c]:>9}" for c in CLASSES) + f"{sum(t.values()):>9}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--remarks")
    ap.add_argument("--marker", default=r"^s_memtime")
    ap.add_argument("--by-line", action="store_true")
    ap.add_argument("--top", type=int, default=40)
    ap.add_argument("--sort", choices=sorted(SORT_KEYS), default="issue")
    args = ap.parse_args()
    with open(args.listing) as fh:
        lines = fh.read().splitlines()
    name, pretty, body, info = kernel_body(lines, args.kernel)
    print(pretty)
    keep = ("codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")
    print("  " + "  ".join(i.replace(" = ", ": ") for i in info if i.startswith(keep)))
    if args.remarks:
        with open(args.remarks) as fh:
            for r in kres.parse_remarks(fh.read()):
                if r["name"].startswith(pretty.split("(")[0]):
                    print("  " + kres.format_row(r))
    blocks = parse_blocks(body)
    top = {}
    for b in blocks:
        if b["loops"]:
            top[b["loops"][0]] = top.get(b["loops"][0], 0) + len(b["insts"])
    if not top:
        sys.exit("no loop in this kernel")
    if args.by_line:
        if not any(loc for b in blocks for _, loc in b["full"]):
            sys.exit("no .loc directives: compile the listing with -gline-tables-only")
        files = file_table(lines)
        spill = spill_registers(blocks)
        print(f"SGPR-spill registers (written by v_writelane_b32 only): {' '.join(sorted(spill)) or 'none'}")
        # the batch loops: every outermost loop at least half the largest one's size
        for h in [h for h in top if 2 * top[h] >= max(top.values())]:
            inl = [b for b in blocks if b["loops"] and b["loops"][0] == h]
            print(f"\nloop {h}: {len(inl)} blocks, static instructions by source line")
            print(f"{'':<28}" + "".join(f"{c:>9}" for c in CLASSES) + f"{'total':>9}")
            print(row("whole loop", mix([m for b in inl for m in b["insts"]])))
            by_line(inl, files, args.top, spill, args.sort)
        return
    main_loop = max(top, key=top.get)
    inl = [b for b in blocks if b["loops"] and b["loops"][0] == main_loop]
    print(f"\nmain loop {main_loop}: {len(inl)} blocks (static instructions)")
    print(f"{'':<28}" + "".join(f"{c:>9}" for c in CLASSES) + f"{'total':>9}")
    print(row("whole loop", mix([m for b in inl for m in b["insts"]])))
    own = [m for b in inl if len(b["loops"]) == 1 for m in b["insts"]]
    print(row("  outside nested loops", mix(own)))
    nested = []
    for b in inl:
        for d, h in enumerate(b["loops"][1:], 2):
            if (d, h) not in nested:
                nested.append((d, h))
    for d, h in nested:
        sub = [m for b in inl if len(b["loops"]) >= d and b["loops"][d - 1] == h for m in b["insts"]]
        print(row("  " * (d - 1) + f"loop {h} (depth {d})", mix(sub)))
    mk = re.compile(args.marker)
    seq = [m for b in inl for m in b["insts"]]
    cuts = [i for i, m in enumerate(seq) if mk.search(m)]
    if cuts:
        print(f"\nregions between the {len(cuts)} markers, in listing order")
        edges = [0] + cuts + [len(seq)]
        for r in range(len(edges) - 1):
            print(row(f"  region {r}", mix(seq[edges[r]:edges[r + 1]])))


if __name__ == "__main__":
    main()

"""Has a change moved an existing kernel?  python tools/device_code_diff.py parent.so this.so

Extracts the gfx950 code objects of two builds of libflipchain.so (the .hip_fatbin section's
uncompressed offload bundles) and compares, by symbol name, the bytes of every function and of
every kernel descriptor (*.kd) of the first build with the second's.  Needs no GPU.  Prints the
counts and every symbol that is missing or differs (DESIGN.md §5h records a run); for a function
that differs, both sizes and whether the two disassemblies hold the same instructions, counted by
mnemonic (so: the same code in another order or other registers); for a descriptor that differs,
whether anything but its kernel_code_entry_byte_offset does (bytes 16-23: the distance from the
descriptor to the code, which moves with the code object's layout -- a symbol-name string of
another length is enough -- and says nothing about the kernel)."""
import collections
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin/")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    tmp = tempfile.mkdtemp(prefix="cmp_")
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "copy.so")], check=True)
    data = open(fat, "rb").read()
    assert b"CCOB" not in data[:4], "compressed bundle"
    out = []
    pos = data.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + 24)[0]
        p = pos + 32
        for _ in range(n):
            off, size, idl = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idl].decode()
            p += 24 + idl
            if "gfx950" in ident and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + 1)
    return out, tmp


def symbols(lib):
    objs, tmp = code_objects(lib)
    syms = {}
    for i, blob in enumerate(objs):
        path = os.path.join(tmp, f"co{i}.elf")
        open(path, "wb").write(blob)
        secs = {}
        for line in subprocess.run([LLVM + "llvm-readelf", "-SW", path], capture_output=True, text=True, check=True).stdout.splitlines():
            m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
            if m:
                secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
        for line in subprocess.run([LLVM + "llvm-readelf", "-sW", path], capture_output=True, text=True, check=True).stdout.splitlines():
            f = line.split()
            if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or not f[6].isdigit():
                continue
            addr, size, name, ndx = int(f[1], 16), int(f[2]), f[7], int(f[6])
            if size == 0 or ndx not in secs:
                continue
            if f[3] == "OBJECT" and not name.endswith(".kd"):
                continue
            _, saddr, soff = secs[ndx]
            body = blob[soff + addr - saddr: soff + addr - saddr + size]
            syms[name] = (hashlib.sha256(body).hexdigest(), size, path, body if name.endswith(".kd") else None)
    return syms


def mnemonics(sym, name):
    """The function's instructions, counted by mnemonic."""
    out = subprocess.run([LLVM + "llvm-objdump", "-d", "--disassemble-symbols=" + name, sym[2]],
                         capture_output=True, text=True, check=True).stdout
    return collections.Counter(m.group(1) for m in re.finditer(r"^\s+([a-z]\w*)\b.*//", out, re.M))


a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
missing = [s for s in a if s not in b]
differ = [s for s in a if s in b and a[s][0] != b[s][0]]
new = [s for s in b if s not in a]
print(f"parent symbols {len(a)} (functions {sum(1 for s in a if not s.endswith('.kd'))}, descriptors {sum(1 for s in a if s.endswith('.kd'))}); "
      f"identical {len(a) - len(missing) - len(differ)}; missing {len(missing)}; differ {len(differ)}; new in this build {len(new)}")
for s in missing:
    print("  MOVED", s)
for s in differ:
    if s.endswith(".kd"):
        ka, kb = a[s][3], b[s][3]
        layout_only = len(ka) == len(kb) == 64 and ka[:16] + ka[24:] == kb[:16] + kb[24:]
        print("  MOVED", s + (": kernel_code_entry_byte_offset only (layout)" if layout_only else ""))
        continue
    ma, mb = mnemonics(a[s], s), mnemonics(b[s], s)
    print(f"  MOVED {s}: bytes {a[s][1]} -> {b[s][1]}; instructions {sum(ma.values())} -> {sum(mb.values())}, "
          f"mnemonic multiset {'same' if ma == mb else 'differs'}")
for s in new:
    print("  new", s)

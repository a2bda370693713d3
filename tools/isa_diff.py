#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libvermilion_hip.so, instruction stream by instruction stream.

    python tools/isa_diff.py OLD.so NEW.so [--show KERNEL_SUBSTRING] [--rename REGEX REPL]...

Every code object in the libraries' offload bundles is disassembled (llvm-objdump -d --no-show-raw-insn), the listing is
split per kernel symbol, addresses and branch-target comments are dropped, and kernels of the same name are compared.
Prints one line per kernel that differs, is new or is gone, then the totals; --show also prints the resource lines
(.vgpr_count, .sgpr_count, scratch, LDS) of the NEW library's kernels whose name contains the substring.
Exit status 1 if a kernel both libraries have differs."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    """the gfx950 code objects of every offload bundle in the file"""
    data = open(path, "rb").read()
    out, at = [], 0
    while True:
        at = data.find(MAGIC, at)
        if at < 0:
            return out
        n = struct.unpack_from("<Q", data, at + 24)[0]
        p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(data[at + off:at + off + size])
        at += len(MAGIC)


def kernels(blob):
    """{kernel symbol: [instruction lines]}, {kernel symbol: metadata text}"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(blob)
        f.flush()
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f.name], check=True,
                             capture_output=True, text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], check=True, capture_output=True,
                               text=True).stdout
    body, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            body[name] = []
        elif name and line.strip():
            ins = re.sub(r"//.*$", "", line).strip()          # the address comment
            ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<>", ins)  # branch targets by symbol + offset
            if ins != "...":  # (objdump's mark for the zero padding between two symbols)
                body[name].append(ins)
    for lines in body.values():  # (the s_nop padding up to the next symbol's alignment is not the kernel's)
        while lines and lines[-1].startswith("s_nop"):
            lines.pop()
    meta = {}
    for chunk in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        m = re.search(r"\.name:\s+(\S+)", chunk)
        if m:
            meta[m.group(1)] = "\n".join(l.strip() for l in chunk.splitlines() if re.search(
                r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):", l))
    return body, meta


def library(path):
    body, meta = {}, {}
    for blob in code_objects(path):
        b, m = kernels(blob)
        body.update(b), meta.update(m)
    return body, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"), ap.add_argument("new"), ap.add_argument("--show", default=None)
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"),
                    help="re.sub applied to the kernel symbols of BOTH libraries before they are matched: compares a kernel "
                         "with its successor under another mangled name (a template or an argument was added)")
    a = ap.parse_args()
    (ob, _), (nb, nm) = library(a.old), library(a.new)

    def renamed(d):
        out = {}
        for k, v in d.items():
            for rx, repl in a.rename:
                k = re.sub(rx, repl, k)
            assert k not in out, "two symbols are renamed to " + k
            out[k] = v
        return out

    ob, nb, nm = renamed(ob), renamed(nb), renamed(nm)
    same = differ = 0
    for k in sorted(set(ob) & set(nb)):
        if ob[k] == nb[k]:
            same += 1
        else:
            differ += 1
            print("DIFFERS", k, len(ob[k]), "->", len(nb[k]), "instructions")
    for k in sorted(set(nb) - set(ob)):
        print("NEW    ", k, len(nb[k]), "instructions")
    for k in sorted(set(ob) - set(nb)):
        print("GONE   ", k)
    print(f"{same} symbols identical, {differ} differ, {len(set(nb) - set(ob))} new, {len(set(ob) - set(nb))} gone")
    if a.show:
        for k in sorted(nm):
            if a.show in k:
                print(k)
                print("   " + nm[k].replace("\n", "\n   "))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())

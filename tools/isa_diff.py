#!/usr/bin/env python3
"""Diff the gfx950 machine code of chosen kernels between two builds of libnavenv.so.

    python tools/isa_diff.py OLD.so NEW.so 'k_mlp_fwdILi8ELi2ELi1ELi4E' \
        'k_test_rolloutILi8ELi2EE=k_test_rolloutILi8ELi2ELb0EE'

Every gfx950 code object of each library's offload bundles is disassembled (llvm-objdump -d); per
kernel whose mangled name contains one of the patterns, the instruction listing (addresses and
encodings dropped, so that a kernel that merely moved inside its code object compares equal) is
compared. A pattern OLD=NEW names a kernel whose mangled name changed (a template parameter
added): NEW is rewritten to OLD in the new library's names before matching. Prints one line per
kernel and exits 1 when a listing differs or a kernel is missing on either side. The gate that a change left a hot kernel exactly as the compiler made it before.
"""
import difflib
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


def code_objects(path):
    """The gfx950 code objects of every (uncompressed) offload bundle in the file."""
    blob = open(path, "rb").read()
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        pos = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tlen].decode()
            pos += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def listings(path, patterns, renames=()):
    """{kernel symbol: [instruction text]} of the kernels whose name contains a pattern."""
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name],
                                  capture_output=True, text=True, check=True).stdout
        name = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                sym = m.group(1)
                for old, new in renames:
                    sym = sym.replace(new, old)
                name = sym if any(p in sym for p in patterns) else None
                if name:
                    out[name] = []
                continue
            if name and line.strip() and line.strip() != "...":  # (elided padding)
                # drop the trailing address comment and branch targets' absolute addresses
                ins = re.sub(r"\s*//.*$", "", line).strip()
                out[name].append(ins)
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    renames = [tuple(p.split("=", 1)) for p in sys.argv[3:] if "=" in p]
    patterns = [p.split("=", 1)[0] for p in sys.argv[3:]]
    a, b = listings(old, patterns), listings(new, patterns, renames)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            if k in a:
                print(f"MISSING in new: {k}")
                bad += 1
            else:
                print(f"new only      : {k}")
            continue
        if a[k] == b[k]:
            print(f"identical ({len(a[k])} instructions): {k}")
        else:
            bad += 1
            d = list(difflib.unified_diff(a[k], b[k], "old", "new", lineterm="", n=1))
            print(f"DIFFERENT ({len(a[k])} vs {len(b[k])} instructions): {k}")
            print("\n".join(d[:40]))
    if not a:
        print("no kernel matched")
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

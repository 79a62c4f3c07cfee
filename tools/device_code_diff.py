"""Compares the DEVICE code of two builds of libkiez_amd.so (a refactor of host code must not change any of it):

    python tools/device_code_diff.py <parent.so> <head.so>

Every gfx950 code object of both libraries is taken out of its offload bundle; per kernel the resource metadata (VGPRs, SGPRs, LDS,
scratch, spills: llvm-readelf --notes) and the instruction text (llvm-objdump -d, addresses and encodings stripped -- a kernel that
moves inside its object is still the same kernel) are compared.  Prints the kernels that are missing, new or different and one
summary line; exit status 1 if anything differs.  Needs no GPU."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count", ".wavefront_size", ".max_flat_workgroup_size", ".kernarg_segment_size")


def code_objects(path):
    blob = open(path, "rb").read()
    pos = blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        at = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, at)
            triple = blob[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[pos + off:pos + off + size]
        pos = blob.find(MAGIC, pos + len(MAGIC))


def kernels(path):
    """{kernel name: (metadata tuple, sha1 of instruction text, instruction count)}; a name seen in two objects gets a #n suffix."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(path)):
            f = os.path.join(tmp, "co%d.elf" % i)
            open(f, "wb").write(co)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True, check=True).stdout
            meta = {}
            for block in re.split(r"\n  - ", notes)[1:]:   # (one entry of amdhsa.kernels each: the list items at two spaces)
                name = re.search(r"\n    \.name:\s+(\S+)", block)
                if name:
                    meta[name.group(1)] = tuple((k, (re.search(re.escape(k) + r":\s+(\S+)", block) or [None, None])[1]) for k in META)
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", f], capture_output=True, text=True,
                                 check=True).stdout
            cur, text = None, {}
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    text[cur] = []
                elif cur and line.strip():
                    text[cur].append(re.sub(r"\s*//.*$", "", line).strip())
            for name, md in meta.items():
                body = text.get(name, [])
                key, n = name, 1
                while key in out:
                    n += 1
                    key = "%s#%d" % (name, n)
                out[key] = (md, hashlib.sha1("\n".join(body).encode()).hexdigest(), len(body))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    missing, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in missing:
        print("MISSING", k)
    for k in new:
        print("NEW", k)
    for k in differ:
        what = "metadata" if a[k][0] != b[k][0] else "instructions"
        print("DIFFERENT (%s)" % what, k, a[k][2], "->", b[k][2], "instructions")
    empty = sum(1 for v in a.values() if v[2] == 0)
    print("%d / %d kernels (%d without text), %d missing, %d new, %d different" % (len(a), len(b), empty, len(missing), len(new), len(differ)))
    return 1 if missing or new or differ or not a else 0


if __name__ == "__main__":
    sys.exit(main())

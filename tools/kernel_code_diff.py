#!/usr/bin/env python3
"""Do two builds of the library hold the same kernels?  Extracts the gfx950 code objects from two shared libraries and compares,
per kernel, the code bytes and the 64-byte kernel descriptor (registers, LDS, scratch, kernarg size), byte for byte.

  python tools/kernel_code_diff.py PARENT/lib/libfsdp_hip.so ft-fsd-path-planning_amd/lib/libfsdp_hip.so

Prints "kernels in parent N differing D new M" and the names of the differing and the new ones; exit status 1 if any differ.
(The compiler's one-byte `__hip_cuid_<hash>` markers, named after a hash of each translation unit, are not kernels and are left out.)
"""
from __future__ import annotations

import hashlib
import os
import struct
import subprocess
import sys
import tempfile

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")


def code_objects(path):
    """the AMDGPU ELF images embedded in a host library"""
    data = open(path, "rb").read()
    out, at = [], 0
    while True:
        at = data.find(b"\x7fELF\x02\x01\x01", at)
        if at < 0:
            break
        if struct.unpack_from("<H", data, at + 18)[0] == 224:  # EM_AMDGPU
            (shoff,) = struct.unpack_from("<Q", data, at + 0x28)
            shentsize, shnum = struct.unpack_from("<HH", data, at + 0x3A)
            out.append(data[at : at + shoff + shentsize * shnum])
        at += 4
    return out


def kernels(path):
    """kernel name -> (sha1 of its code, code bytes, sha1 of its descriptor)"""
    code, desc = {}, {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(delete=False) as f:
            f.write(co)
        secs = subprocess.run([READELF, "-SW", f.name], capture_output=True, text=True, check=True).stdout
        syms = subprocess.run([READELF, "-sW", f.name], capture_output=True, text=True, check=True).stdout
        os.unlink(f.name)
        sec = {}
        for line in secs.splitlines():
            p = line.replace("[", " ").replace("]", " ").split()
            if len(p) > 5 and p[0].isdigit():
                try:
                    sec[int(p[0])] = (int(p[3], 16), int(p[4], 16))
                except ValueError:
                    pass
        for line in syms.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] in ("FUNC", "OBJECT") and p[6].isdigit() and int(p[6]) in sec and int(p[2]):
                addr, size, (base, offset), name = int(p[1], 16), int(p[2]), sec[int(p[6])], p[7]
                digest = hashlib.sha1(co[offset + addr - base : offset + addr - base + size]).hexdigest()[:16]
                if name.endswith(".kd"):
                    desc[name[:-3]] = digest
                elif p[3] == "FUNC":
                    code[name] = (digest, size)
    return {k: (*code[k], desc[k]) for k in code if k in desc}


def main(argv):
    a, b = kernels(argv[1]), kernels(argv[2])
    diff = sorted(k for k in a if b.get(k) != a[k])
    new = sorted(k for k in b if k not in a)
    print(f"{os.path.basename(argv[2])}: kernels in parent {len(a)} differing {len(diff)} new {len(new)}")
    for k in diff:
        print("  differs:", k, a[k], b.get(k))
    for k in new:
        print("  new:", k, f"{b[k][1]} code bytes")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

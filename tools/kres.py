#!/usr/bin/env python3
"""Summarise hipcc -Rpass-analysis=kernel-resource-usage output: one line per kernel (demangled name, VGPR/AGPR/SGPR, scratch, LDS, occupancy, and the kernel
descriptor's kernarg preload length: the dwords of leading plain arguments the command processor puts into SGPRs before a wave starts).
usage: tools/kres.py file.hip [filter-substring] [extra hipcc flags, e.g. -mllvm -amdgpu-kernarg-preload-count=16]

preload_lengths(path) reads the preload length of every kernel from a built file -- an object or a shared library that holds clang offload bundles -- without a
compiler: {mangled kernel name: dwords}."""
import os, re, struct, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _elf_kernel_descriptors(elf):
    """{name: the 64 descriptor bytes} of an AMDGPU ELF64 code object held in a bytes object"""
    if elf[:4] != b"\x7fELF" or elf[4] != 2 or elf[5] != 1:
        return {}
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, offset, size, link, info, align, entsize
    out = {}
    for _, typ, _, _, off, size, link, _, _, entsize in secs:
        if typ not in (2, 11) or not entsize:        # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff = secs[link][4]
        for i in range(size // entsize):
            st_name, _, _, shndx, value, st_size = struct.unpack_from("<IBBHQQ", elf, off + i * entsize)
            end = elf.index(b"\0", stroff + st_name)
            name = elf[stroff + st_name:end].decode("ascii", "replace")
            if not name.endswith(".kd") or st_size != 64 or not 0 < shndx < shnum:
                continue
            sec = secs[shndx]
            pos = sec[4] + value - sec[3]
            out[name[:-3]] = elf[pos:pos + 64]
    return out


def preload_lengths(path, arch="gfx950"):
    """{mangled kernel name: kernarg preload length in dwords} of every kernel for `arch` in the offload bundles of `path`; {} when there is none to read"""
    data = open(path, "rb").read()
    out = {}
    at = data.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", data, at + 24)
        o = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tl]
            o += 24 + tl
            if size and arch.encode() in triple:
                for name, kd in _elf_kernel_descriptors(data[at + off:at + off + size]).items():
                    out[name] = struct.unpack_from("<H", kd, 58)[0] & 0x7F     # kernarg_preload: bits 0..6 = length in dwords, bits 7..15 = offset
        at = data.find(BUNDLE_MAGIC, at + 1)
    return out


def main():
    src = sys.argv[1]; flt = sys.argv[2] if len(sys.argv) > 2 else ""
    obj = os.path.join(tempfile.gettempdir(), "kres.o")
    cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-DMINIGPT4_SHARED", "-DMINIGPT4_BUILD", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "minigpt4.cpp_amd", "csrc"), "--offload-arch=gfx950", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj] + sys.argv[3:]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    cur = None; rows = []
    for line in out.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m: continue
        k, v = m.groups()
        if k == "Function Name": cur = {"name": v}; rows.append(cur)
        elif cur is not None: cur[k.split()[0]] = v
    pre = preload_lengths(obj) if os.path.exists(obj) else {}
    names = subprocess.run(["c++filt"] + [r["name"] for r in rows], capture_output=True, text=True).stdout.splitlines() if rows else []
    for r, n in zip(rows, names):
        n = re.sub(r"\(.*", "", n).replace("void mg4::", "")
        if flt and flt not in n: continue
        print(f"{n:48s} vgpr {r.get('VGPRs'):>4} agpr {r.get('AGPRs'):>3} sgpr {r.get('TotalSGPRs'):>3} scratch {r.get('ScratchSize'):>4} lds {r.get('LDS'):>6} occ {r.get('Occupancy')}"
              f" preload {pre.get(r['name'], '?'):>2}")


if __name__ == "__main__":
    main()

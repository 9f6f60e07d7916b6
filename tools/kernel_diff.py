#!/usr/bin/env python3
"""Device code of two builds of libdust_amd.so, kernel for kernel: the instruction bytes of every kernel symbol and its entry in the
   code object's metadata note (registers, spills, LDS, scratch, arguments).  Prints the kernels that are added, missing or differ;
   exit status 1 if there are any.  For a host-only change nothing may be listed.
   python tools/kernel_diff.py A.so B.so"""
import os, re, shutil, struct, subprocess, sys, tempfile

llvm = "/opt/rocm/lib/llvm/bin"


def code_bytes(path):
    """{function symbol: its bytes} of one ELF64 code object"""
    b = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", b, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]  # name type flags addr off size link info align entsize
    out = {}
    for s in sec:
        if s[1] != 2:  # SHT_SYMTAB
            continue
        stro = sec[s[6]][4]
        for o in range(s[4], s[4] + s[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", b, o)
            if info & 15 == 2 and size and 0 < shndx < shnum:  # STT_FUNC
                t = sec[shndx]
                n = b[stro + name:b.index(b"\0", stro + name)].decode()
                out[n] = b[t[4] + value - t[3]:t[4] + value - t[3] + size]
    return out


def kernels(so):
    """{kernel name: (instruction bytes, metadata entry)} over the gfx950 code objects of a library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(so, os.path.join(d, "l.so"))
        subprocess.run([llvm + "/llvm-objdump", "--offloading", "l.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            code = code_bytes(os.path.join(d, f))
            notes = subprocess.run([llvm + "/llvm-readelf", "--notes", f], cwd=d, check=True, capture_output=True, text=True).stdout
            body = notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]
            for entry in re.split(r"\n  - ", body)[1:]:
                name = re.search(r"\.name:\s+(\S+)", entry).group(1)
                assert name not in out, name
                out[name] = (code[name], entry)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for n in sorted(set(a) | set(b)):
    what = "missing" if n not in b else "added" if n not in a else "code differs" if a[n][0] != b[n][0] else "metadata differs" if a[n][1] != b[n][1] else None
    if what:
        bad += 1
        print("%-16s %s" % (what, n))
print("%d kernels in %s, %d in %s: %d added, missing or different" % (len(a), sys.argv[1], len(b), sys.argv[2], bad))
sys.exit(1 if bad else 0)

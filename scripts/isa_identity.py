"""isa_identity.py OBJ... — for every gfx950 kernel inside the given host objects: demangled name, SHA-1 of its machine-code bytes, SHA-1 of
its kernel descriptor and the object it lies in, one kernel per line, sorted.  Two builds that print the same lines run the same code: the
twin of ab_identity.py that needs no GPU (a refactor that must not change a kernel is checked by diffing two listings).

    python scripts/isa_identity.py 3dgrut_amd/csrc/*.o > new.txt

The code object is extracted the way obj_resources.sh does it (llvm-objdump --offloading); the bytes of a kernel are its function symbol's
range in .text, the descriptor is its NAME.kd symbol's 64 bytes.  Bytes are hashed, no instruction is looked at.  A name that occurs in more
than one object is an error (exit status 1).
Only kernels (function symbols with a .kd twin) are hashed: a __device__ function that is not inlined into its callers lies outside every
hashed range.  The project's device code is __forceinline__ or template bodies inlined into kernels; check with llvm-readelf -s if that changes.
"""
import glob
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def code_object(obj, tmp):
    """Bytes of the gfx950 code object bundled in a host object (None: the object holds no device code)."""
    x = os.path.join(tmp, "x.o")
    shutil.copy(obj, x)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "x.o"], cwd=tmp, capture_output=True)
    found = sorted(glob.glob(x + ".*gfx950*"))
    data = open(found[0], "rb").read() if found else None
    for f in glob.glob(x + "*"):
        os.remove(f)
    return data


def kernels(elf):
    """{mangled name: (code bytes, descriptor bytes)} of an ELF64 little-endian code object."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr off size link info align entsize
    symtab = next(s for s in sections if s[1] == 2)
    strtab = sections[symtab[6]]
    symbols = {}
    for at in range(symtab[4], symtab[4] + symtab[5], 24):
        name_off, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, at)
        name = elf[strtab[4] + name_off:elf.index(b"\0", strtab[4] + name_off)].decode()
        if 0 < shndx < shnum:
            sec = sections[shndx]
            symbols[name] = elf[sec[4] + value - sec[3]:sec[4] + value - sec[3] + size]
    return {n[:-3]: (symbols[n[:-3]], kd) for n, kd in symbols.items() if n.endswith(".kd") and n[:-3] in symbols}


def main():
    rows, seen, dup = [], {}, False
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sys.argv[1:]:
            elf = code_object(obj, tmp)
            for name, (code, kd) in (kernels(elf) if elf else {}).items():
                if name in seen:
                    print(f"{name}: in {seen[name]} and in {os.path.basename(obj)}", file=sys.stderr)
                    dup = True
                seen[name] = os.path.basename(obj)
                rows.append((name, hashlib.sha1(code).hexdigest(), hashlib.sha1(kd).hexdigest(), os.path.basename(obj)))
    plain = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    # (the name without its namespace and parameter list, as kernel_resources.py prints it: template arguments tell the instances apart)
    short = [re.sub(r"\(.*", "", d.replace("grut::(anonymous namespace)::", "").replace("grut::", "")).replace("void ", "") for d in plain]
    for line in sorted(f"{d}  code {r[1]}  kd {r[2]}  {r[3]}" for r, d in zip(rows, short)):
        print(line)
    sys.exit(1 if dup else 0)


if __name__ == "__main__":
    main()

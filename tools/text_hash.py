#!/usr/bin/env python3
"""sha256 of the gfx950 .text section of every object under a directory (default upright_amd/csrc/build): what has to stay equal when
a source edit is meant to change no production code (comment / dead-branch removal).  No GPU needed.
usage: python tools/text_hash.py [dir]
       python tools/text_hash.py --kernels [dir]            one line per kernel: the bytes of its own symbol in .text
       python tools/text_hash.py --compare dir_a dir_b      the kernels of dir_a whose bytes differ in dir_b or are missing there (what
                                                            an edit that ADDS kernels must leave empty), and the kernels only in dir_b"""
import hashlib
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def _code_object(obj, td):
    co, fat = Path(td) / "dev.co", Path(td) / "fat.bin"
    subprocess.check_call([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(obj)])
    subprocess.check_call([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], stderr=subprocess.DEVNULL)
    return co


def _text(co, td):
    txt = Path(td) / "text.bin"
    subprocess.check_call([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.text", str(co), str(txt)])
    return txt.read_bytes()


def text_hash(obj):
    with tempfile.TemporaryDirectory() as td:
        b = _text(_code_object(obj, td), td)
        return hashlib.sha256(b).hexdigest()[:16], len(b)


def kernel_hashes(obj):
    """{kernel symbol: (hash, bytes)}: the FUNC symbols of the code object that have a kernel descriptor (<name>.kd), each hashed over
    its own address range of .text"""
    with tempfile.TemporaryDirectory() as td:
        co = _code_object(obj, td)
        text = _text(co, td)
        sec = subprocess.check_output([str(LLVM / "llvm-readelf"), "-S", "-W", str(co)], text=True)
        base = None
        for line in sec.splitlines():
            f = line.replace("[", " ").replace("]", " ").split()
            if len(f) > 3 and f[1] == ".text":
                base = int(f[3], 16)
        sym = subprocess.check_output([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], text=True)
        funcs, kds = {}, set()
        for line in sym.splitlines():
            f = line.split()
            if len(f) < 8:
                continue
            if f[3] == "FUNC":
                funcs[f[7]] = (int(f[1], 16), int(f[2], 0))
            elif f[7].endswith(".kd"):
                kds.add(f[7][:-3])
        out = {}
        for name, (addr, size) in funcs.items():
            if name in kds:
                b = _mask_pc_relative(text[addr - base:addr - base + size])
                out[name] = (hashlib.sha256(b).hexdigest()[:16], len(b))
        return out


def _mask_pc_relative(code):
    """The bytes of a kernel with the literals of its pc-relative addresses zeroed: s_getpc_b64 is followed by s_add_u32 / s_addc_u32
    with 32-bit literals that hold the distance to another symbol of the object (a function that was not inlined, a table), which
    moves when anything is added to the object while the kernel's own code stays what it was.  Zeroed: the literal slots of the two
    instructions after every s_getpc_b64."""
    b = bytearray(code)
    for off in range(0, len(b) - 3, 4):
        w = int.from_bytes(b[off:off + 4], "little")
        if w & 0xFF80FFFF != 0xBE801C00:      # SOP1 s_getpc_b64, any destination
            continue
        p = off + 4
        for _ in range(2):                   # s_add_u32 / s_addc_u32 with a literal (ssrc1 = 0xff): the word after it
            if p + 8 <= len(b) and (int.from_bytes(b[p:p + 4], "little") >> 8) & 0xFF == 0xFF:
                b[p + 4:p + 8] = bytes(4)
                p += 8
            else:
                p += 4
    return bytes(b)


def _dir_kernels(d):
    return {(o.name, k): v for o in sorted(Path(d).glob("*.o")) for k, v in kernel_hashes(o).items()}


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        a, b = _dir_kernels(args[1]), _dir_kernels(args[2])
        changed = [k for k in a if k not in b or b[k] != a[k]]
        for o, k in changed:
            print(f"CHANGED {o} {k}: {a[(o, k)]} -> {b.get((o, k))}")
        for o, k in b:
            if (o, k) not in a:
                print(f"new     {o} {k}: {b[(o, k)][1]} B  {b[(o, k)][0]}")
        allh = hashlib.sha256("".join(f"{o}{k}{a[(o, k)][0]}" for o, k in sorted(a)).encode()).hexdigest()[:16]
        print(f"{len(a)} kernels in {args[1]}, {len(a) - len(changed)} byte-identical in {args[2]}; hash over the first set {allh}")
        sys.exit(1 if changed else 0)
    if args and args[0] == "--kernels":
        for (o, k), (h, n) in _dir_kernels(args[1] if len(args) > 1 else "upright_amd/csrc/build").items():
            print(f"{o:24s} {n:9d} B  {h}  {k}")
        sys.exit(0)
    d = Path(args[0] if args else "upright_amd/csrc/build")
    for o in sorted(d.glob("*.o")):
        h, n = text_hash(o)
        print(f"{o.name:24s} {n:9d} B  {h}")

#!/usr/bin/env python3
"""Resource usage of every ahead-of-time instantiation of the production QP kernel (and of the kernels of the C-ABI's units,
__graft_entry__.ENGINE_UNITS, with `api`): VGPRs, spilled VGPRs, scratch bytes, LDS, occupancy -- from the compiler's
kernel-resource-usage remarks (no GPU needed).
    python tools/kernel_resources.py [part ...| api] [-DUPR_...]"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import CSRC, ENGINE_UNITS, HIPCC_FLAGS  # noqa: E402


def usage_of(src, extra=()):
    """the remarks of one translation unit: {kernel symbol: {vgpr, agpr, spill, scratch, lds, occ}}"""
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *HIPCC_FLAGS, *extra, "--cuda-device-only", "-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); out[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def usage(part, extra=()):
    """`api`: the merged table of the units of the C-ABI, compiled side by side (at most 8 at once); else part `part` of the production QP kernel"""
    if part != "api":
        return usage_of("upr_qp3_inst.hip", (*extra, f"-DUPR_QP3_PART={part}"))
    out = {}
    with ThreadPoolExecutor(max(1, min(len(ENGINE_UNITS), 8, os.cpu_count() or 1))) as ex:
        for r in ex.map(lambda u: usage_of(u, extra), ENGINE_UNITS):
            out.update(r)
    return out


def demangle(n):
    try:
        return subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", n], capture_output=True, text=True).stdout.strip()
    except Exception:
        return n


if __name__ == "__main__":
    extra = [a for a in sys.argv[1:] if a.startswith("-")]
    parts = [a for a in sys.argv[1:] if not a.startswith("-")] or [str(k) for k in range(6)]
    with ThreadPoolExecutor(4) as ex:
        res = list(ex.map(lambda p: usage(p, extra), parts))
    for p, r in zip(parts, res):
        for n, u in r.items():
            if "qp3" in n or p == "api":
                print(f"part {p}  {demangle(n)[:110]:110s}  " + "  ".join(f"{k} {v}" for k, v in u.items()))

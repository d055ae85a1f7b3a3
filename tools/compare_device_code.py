"""Has a change touched device code?  Compares two outputs of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize --cuda-device-only -S smalify_amd/csrc/smalfit_kernels.hip -o X.s
symbol by symbol: every function body and every .amdhsa_kernel block must be identical; only their order in the file may differ.
    python tools/compare_device_code.py before.s after.s      (exit status 1 when anything differs)"""
import re
import sys


def split(path):
    txt = open(path).read()
    txt = re.sub(r"^\s*(;|\.file|\.loc|\.ident|\.section\s+\.debug).*\n", "", txt, flags=re.M)
    txt = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI)\d+", r".\1", txt)       # labels carry the function's position in the file
    txt = re.sub(r"[ \t]*;.*$", "", txt, flags=re.M)                            # ... and comments name those labels
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\s*\.size\s+\1,", txt, re.S | re.M)}
    hsa = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", txt, re.S)}
    return bodies, hsa


(b0, h0), (b1, h1) = split(sys.argv[1]), split(sys.argv[2])
bad = [k for k in sorted(set(b0) | set(b1)) if b0.get(k) != b1.get(k) and not k.startswith("__hip_cuid")]     # (the unit's hash symbol)
bad += [k for k in sorted(set(h0) | set(h1)) if h0.get(k) != h1.get(k)]
print("%d symbols, %d kernels, %d differ %s" % (len(b1), len(h1), len(bad), bad))
sys.exit(1 if bad or not h1 else 0)

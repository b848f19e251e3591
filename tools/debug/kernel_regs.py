"""Registers, spills, LDS and scratch of every kernel in the shipped libhprt.so (from the code object's metadata; no GPU needed)."""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tree_walk_checks import LIBHPRT, kernel_metadata
kernels = kernel_metadata(sys.argv[1] if len(sys.argv) > 1 else LIBHPRT, tempfile.mkdtemp()).values()
flt = sys.argv[2] if len(sys.argv) > 2 else ""
for k in sorted(kernels, key=lambda k: k[".name"]):
    if flt in k[".name"]:
        name = subprocess.run(["c++filt", k[".name"]], capture_output=True, text=True).stdout.strip().split("(")[0]
        print("%-70s vgpr %3d  agpr %3d spill %3d  sgpr %3d  lds %6d  scratch %5d" % (name[:70], k[".vgpr_count"], k.get(".agpr_count", 0), k[".vgpr_spill_count"], k[".sgpr_count"], k[".group_segment_fixed_size"], k[".private_segment_fixed_size"]))

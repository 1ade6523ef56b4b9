#!/usr/bin/env python3
"""Developer tool (build container): registers, spills, occupancy and LDS of the library's kernels, from the compiler's own report.
   python tools/kernel_resources.py [substring ...]      e.g.  k_lossIf k_dual_hIf k_sddmm_mfma
   python tools/kernel_resources.py --append FILE [substring ...]   appends the lines of kernels FILE does not list yet and leaves
                                                                    its existing lines where they are; a kernel that spills or uses
                                                                    scratch is refused (profiles/batch_kernel_resources.txt)"""
import os, re, subprocess, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(root, "sig_sdp_mmw_amd", "csrc", "mmw_api.hip")
with tempfile.TemporaryDirectory() as d:
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "x.o")], capture_output=True, text=True)
t = r.stderr
want = sys.argv[1:]
append = None
if want[:1] == ["--append"]:
    append, want = want[1], want[2:]
    have = open(append).read()
for b in re.split(r"remark: Function Name: ", t)[1:]:
    name = b.split()[0]
    if want and not any(w in name for w in want): continue
    g = lambda k: (re.search(re.escape(k) + r": (\d+)", b) or [None, "?"])[1]
    line = "%-70s VGPR %3s AGPR %3s spill %2s scratch %3s waves/SIMD %s LDS %6s" % (name, g("VGPRs"), g("AGPRs"), g("VGPRs Spill"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]"), g("LDS Size [bytes/block]"))
    if append is None:
        print(line)
    elif name + " " not in have:
        if g("VGPRs Spill") != "0" or g("ScratchSize [bytes/lane]") != "0":
            sys.exit("refused: " + line)
        open(append, "a").write(line + "\n")
        print("appended: " + line)

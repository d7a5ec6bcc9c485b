"""Resource usage (VGPRs, spills, occupancy, LDS) of the product's kernels from the compiler's
kernel-resource-usage remarks:  python tools/kernel_regs.py [unit.hip] [--all] [-- extra hipcc flags]
(default unit: rt_render.hip, the render kernels; the probe kernels are rt_probe.hip)"""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the Makefile's HIPFLAGS (also tools/trace_asm_split.py)
HIPCC = "/opt/rocm/bin/hipcc"
HIPCC_FLAGS = ["-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
               "-fno-gpu-flush-denormals-to-zero", "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function",
               "-Wno-unknown-pragmas"]


def usage(src=None, extra=(), pattern=r"k_(trace|step|tail)"):
    src = src or os.path.join(REPO, "sycl-ray-tracing_amd", "csrc", "rt_render.hip")
    cmd = [HIPCC, *HIPCC_FLAGS, "-Rpass-analysis=kernel-resource-usage", *extra, "-c", src, "-o", "/tmp/kernel_regs.o"]
    out = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"\s(VGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return {k: v for k, v in rows.items() if re.search(pattern, k)}


if __name__ == "__main__":
    args = sys.argv[1:]
    extra = args[args.index("--") + 1:] if "--" in args else []
    args = args[:args.index("--")] if "--" in args else args
    # --all: every kernel of the unit (rt_probe.hip, rt_display.hip, rt_denoise.hip), not only the wavefront's three classes
    pattern = r"k_" if "--all" in args else r"k_(trace|step|tail)"
    args = [a for a in args if a != "--all"]
    src = args[0] if args else None
    for k, v in usage(src, extra, pattern).items():
        print(f"{k[:64]:64s} vgpr {v.get('VGPRs')} spill {v.get('VGPRs Spill')} sspill {v.get('SGPRs Spill')} "
              f"occ {v.get('Occupancy')} lds {v.get('LDS Size')}")

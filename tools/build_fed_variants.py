"""Analysis builds of the bitmap-fed decompress kernel at other residencies (kernels.h: LZF_DBG_FED_WAVES; LZF_FED_FAR_LATE of
lz4_decompress_fed.hip) -> rust-lz-fear_amd/liblzfear_hip_fed_<name>.so, and what the compiler says about each:
VGPRs, spilled SGPRs, scratch, LDS, waves per SIMD, static instructions of the kernel.
usage: python tools/build_fed_variants.py [name ...]        (no name: all)   --report: the compiler's figures only, no library"""
import os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_lz_fear_amd  # noqa
from rust_lz_fear_amd import build

VARIANTS = {
    "parent": ["LZF_DBG_FED_WAVES=0"],                                      # no bound: five waves per SIMD, the kernel before the study
    "r6": ["LZF_DBG_FED_WAVES=6"],                                          # the product's bound
    "r6late": ["LZF_DBG_FED_WAVES=6", "LZF_FED_FAR_LATE"],                  # far-match loads issued behind the literal copy
    "r7": ["LZF_DBG_FED_WAVES=7"],                                          # as many as the LDS admits (25 per CU)
    "fixed": ["LZF_DBG_FED_WAVES=6", "LZF_FED_FIXED_ROUNDS"],               # 1 KiB-aligned rounds, no carried tails: the kernel before the windows followed the chain
}
KERNEL = "lzf_decompress_fed_kernel"


def report(defines):
    """hipcc -Rpass-analysis=kernel-resource-usage + the device assembly of lz4_decompress_fed.hip."""
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "fed.s")
        cmd = [build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(build.ROOT, "include"), "--offload-device-only", "-S",
               "-Rpass-analysis=kernel-resource-usage", "-o", asm, os.path.join(build.CSRC, "lz4_decompress_fed.hip")] + [f"-D{x}" for x in defines + ["LZF_ANALYSIS"]]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        out, on = {}, False
        for ln in err.splitlines():
            m = re.search(r"remark: .*?\s+([A-Za-z][A-Za-z \[\]/]*?):\s+(\S+)", ln)
            if "Function Name" in ln:
                on = KERNEL in ln
            elif on and m:
                out[m.group(1).strip()] = m.group(2)
        n, inside = 0, False
        for ln in open(asm):
            s = ln.strip()
            if re.match(r"_ZN3lzf25" + KERNEL + r"\w*:", s):
                inside = True
            elif inside and s.startswith(".Lfunc_end"):
                break
            elif inside and s and not s.startswith((".", ";", "//")) and not s.endswith(":"):
                n += 1
        out["instructions"] = n
    return out


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(VARIANTS)
    for name in names:
        r = report(VARIANTS[name])
        lib = "-" if "--report" in sys.argv else os.path.basename(
            build.build_library(defines=VARIANTS[name], out=os.path.join(build.PKG_DIR, f"liblzfear_hip_fed_{name}.so")))
        print(f"{name:8s} {lib}  VGPRs {r.get('VGPRs')}  SGPRs {r.get('TotalSGPRs')} spilled {r.get('SGPRs Spill')}  VGPRs spilled {r.get('VGPRs Spill')}  "
              f"scratch {r.get('ScratchSize [bytes/lane]')}  LDS {r.get('LDS Size [bytes/block]')}  waves/SIMD {r.get('Occupancy [waves/SIMD]')}  "
              f"instructions {r['instructions']}   ({' '.join(VARIANTS[name])})", flush=True)

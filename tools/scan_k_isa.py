"""Resource report of the hm_scan_k kernels beside their hm_collect twins, from
the assembly's own metadata (dev tool, no GPU): hm_scan_k_tiled_kernel<W1, S, T>
against hm_collect_tiled_kernel<W1, S, T>, the chained and generic kernels
against theirs, and the fold kernel alone.  Both families come out of the same
tiled_task / chained_task (scan_tasks.hpp); hm_scan_k's reduction (WaveLowK)
keeps its list in LDS and its state in SGPRs.

Per kernel: VGPRs, SGPR spills (to VGPR lanes), scratch bytes, LDS bytes and
waves per SIMD -- min(8, 512 // VGPRs rounded up to 8), the unified register
file of a gfx950 SIMD; a tiled instantiation that loses a wave against its
twin is marked LOSS.

usage: make -C distributed_bitcoinminer_amd/csrc asm
       python tools/scan_k_isa.py build/hipminer/collect_kernels.aligned.s \
              build/hipminer/scan_k_kernels.aligned.s > profiles/scan_k/scan_k_isa.txt
"""
import re
import sys

FIELDS = {"vgpr": "vgpr_count", "sspill": "sgpr_spill_count", "vspill": "vgpr_spill_count",
          "scratch": "private_segment_fixed_size", "lds": "group_segment_fixed_size"}


def kernels(path):
    """symbol -> {field: int} from the .amdgpu_metadata block."""
    with open(path) as f:
        meta = f.read().split(".amdgpu_metadata", 1)[1]
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(re.search(rf"\.{v}:\s+(\d+)", block).group(1))
                     for k, v in FIELDS.items()}
    return out


def waves(vgpr):
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def twin_of(sym):
    return sym.replace("22hm_scan_k_tiled_kernel", "23hm_collect_tiled_kernel") \
              .replace("NS_14ScanKTiledArgsE", "NS_16CollectTiledArgsE") \
              .replace("24hm_scan_k_chained_kernel", "25hm_collect_chained_kernel") \
              .replace("NS_16ScanKChainedArgsE", "NS_18CollectChainedArgsE") \
              .replace("24hm_scan_k_generic_kernel", "25hm_collect_generic_kernel") \
              .replace("NS_16ScanKGenericArgsE", "NS_18CollectGenericArgsE")


def show(sym):
    m = re.search(r"hm_(\w+?)_kernel(?:ILi(\d+)ELb(\d)ELb(\d)E)?", sym)
    name = f"hm_{m.group(1)}_kernel"
    return name + (f"<{m.group(2)},{m.group(3)},{m.group(4)}>" if m.group(2) else "")


def cell(r):
    return (f"vgpr={r['vgpr']:3d} sgpr-spills={r['sspill']:3d} scratch={r['scratch']} "
            f"lds={r['lds']:4d} waves/SIMD={waves(r['vgpr'])}")


def main(collect_path, scan_k_path):
    col, sk = kernels(collect_path), kernels(scan_k_path)
    print("hm_scan_k kernels beside their hm_collect twins: registers, spills, scratch, LDS and "
          "occupancy from the assembly's metadata (tools/scan_k_isa.py)\n")
    lost = []
    for sym in sk:
        twin = twin_of(sym)
        line = f"{show(sym):34s} {cell(sk[sym])}"
        if twin != sym and twin in col:
            line += f" | {show(twin):34s} {cell(col[twin])}"
            d = waves(sk[sym]["vgpr"]) - waves(col[twin]["vgpr"])
            line += f" | vgpr {sk[sym]['vgpr'] - col[twin]['vgpr']:+d}"
            if d < 0:
                line += f"  LOSS: {-d} wave(s)"
                lost.append(show(sym))
            elif d > 0:
                line += f"  gain: {d} wave(s)"
        print(line)
    assert all(r["scratch"] == 0 and r["vspill"] == 0 for r in sk.values())
    print(f"\nno kernel uses scratch or spills a VGPR; instantiations that lose a wave per SIMD "
          f"against their twin: {len(lost)} {' '.join(lost)}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

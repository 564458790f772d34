"""Hot-loop diff of each hm_find kernel against the scan kernel whose task body
it shares (dev tool, no GPU): hm_find_tiled_kernel<W1, S, T> against
hm_tiled_kernel<W1, S, T>, hm_find_chained_kernel against hm_chained_kernel.
Both come out of the same tiled_task / chained_task (scan_tasks.hpp), with the
"first below target" reduction in place of the running minimum, so the
per-nonce loops should hold the same instructions.

The loops and their VALU mix are tools/isa_audit.py's (its --loop=last-big
selection, since the find kernels end on the publication atomic's short
loop); this tool only pairs the kernels and folds the _e32/_e64 encodings,
as tools/csum_isa_diff.py does for the checked kernels.

usage: make -C distributed_bitcoinminer_amd/csrc asm
       python tools/find_isa_diff.py build/hipminer/scan_kernels.aligned.s \
              build/hipminer/find_kernels.aligned.s > profiles/find/find_isa_diff.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from csum_isa_diff import fold  # noqa: E402
from isa_audit import HALF, loop_mix  # noqa: E402


def hot_loops(path):
    """kernel symbol -> folded VALU mix of its hot loop"""
    lines = open(path).read().split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_ZN2hm\w+):", l)
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
            out[m.group(1)] = fold(loop_mix(lines, i, j, big=True) or {})
    return out


def main(scan_path, find_path):
    scan, find = hot_loops(scan_path), hot_loops(find_path)
    print("hot-loop VALU diff, hm_find kernel minus its scan twin, encodings folded "
          "(tools/find_isa_diff.py)\n")
    worst = 0
    for sym in sorted(find):
        twin = sym.replace("20hm_find_tiled_kernel", "15hm_tiled_kernel") \
                  .replace("NS_13FindTiledArgsE", "NS_9TiledArgsE") \
                  .replace("22hm_find_chained_kernel", "17hm_chained_kernel") \
                  .replace("NS_15FindChainedArgsE", "NS_11ChainedArgsE")
        if twin == sym or twin not in scan:
            continue
        a, b = scan[twin], find[sym]
        extra = {k: b[k] - a[k] for k in sorted(set(a) | set(b)) if b[k] != a[k]}
        na, nb = sum(a.values()), sum(b.values())
        half = lambda m: sum(v for k, v in m.items() if k in HALF)  # noqa: E731
        worst = max(worst, abs(nb - na))
        print(f"{sym:66s} scan={na:5d} (half-rate {half(a)}) find={nb:5d} "
              f"(half-rate {half(b)}) {nb - na:+d} | "
              f"{' '.join(f'{k}:{v:+d}' for k, v in extra.items()) or 'same mix'}")
    print(f"\nlargest difference: {worst} VALU instructions per 64-nonce iteration")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

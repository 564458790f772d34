"""Hot-loop diff of each hm_collect kernel against the hm_find kernel whose
task body it shares (dev tool, no GPU): hm_collect_tiled_kernel<W1, S, T>
against hm_find_tiled_kernel<W1, S, T>, hm_collect_chained_kernel against
hm_find_chained_kernel.  Both come out of the same tiled_task / chained_task
(scan_tasks.hpp), with the "all below target" reduction (WaveCollect) in place
of "first below target" (WaveFirst); the per-nonce test is the same compare
against (target - 1) >> 32, so the per-nonce loops should hold the same
instructions.

The loops and their VALU mix are tools/isa_audit.py's (--loop=last-big, as
tools/find_isa_diff.py reads the find kernels); this tool only pairs the
kernels and folds the _e32/_e64 encodings.

usage: make -C distributed_bitcoinminer_amd/csrc asm
       python tools/collect_isa_diff.py build/hipminer/find_kernels.aligned.s \
              build/hipminer/collect_kernels.aligned.s > profiles/collect/collect_isa_diff.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from find_isa_diff import hot_loops  # noqa: E402
from isa_audit import HALF  # noqa: E402


def main(find_path, collect_path):
    find, col = hot_loops(find_path), hot_loops(collect_path)
    print("hot-loop VALU diff, hm_collect kernel minus its hm_find twin, encodings folded "
          "(tools/collect_isa_diff.py)\n")
    worst = 0
    for sym in sorted(col):
        twin = sym.replace("23hm_collect_tiled_kernel", "20hm_find_tiled_kernel") \
                  .replace("NS_16CollectTiledArgsE", "NS_13FindTiledArgsE") \
                  .replace("25hm_collect_chained_kernel", "22hm_find_chained_kernel") \
                  .replace("NS_18CollectChainedArgsE", "NS_15FindChainedArgsE")
        if twin == sym or twin not in find:
            continue
        a, b = find[twin], col[sym]
        extra = {k: b.get(k, 0) - a.get(k, 0) for k in sorted(set(a) | set(b))
                 if b.get(k, 0) != a.get(k, 0)}
        na, nb = sum(a.values()), sum(b.values())
        half = lambda m: sum(v for k, v in m.items() if k in HALF)  # noqa: E731
        worst = max(worst, abs(nb - na))
        print(f"{sym:72s} find={na:5d} (half-rate {half(a)}) collect={nb:5d} "
              f"(half-rate {half(b)}) {nb - na:+d} | "
              f"{' '.join(f'{k}:{v:+d}' for k, v in extra.items()) or 'same mix'}")
    print(f"\nlargest difference: {worst} VALU instructions per 64-nonce iteration")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

"""hm_find against hm_scan in ONE process, alternating rounds (dev tool, GPU box).

usage: python tools/find_rate.py [ROUNDS] > profiles/find/find_rate.jsonl

(a) No-hit rate.  hm_find(target = 1) hashes every nonce of the range and
    finds nothing, so its wall time is the find kernels' full-scan cost.  Per
    message (bradfitz, and BASELINE configs[2]'s 120-B message) over
    [0, 2^32) each round runs scan, find, scan in turn on two contexts: the
    scan-against-scan pair gives the run-to-run spread the find figure is
    read against.  Median and minimum wall ms, GH/s of the medians.
(b) Early-hit wall time.  hm_find over [0, 2^64 - 1] at targets 2^64 / 10^3,
    2^64 / 10^6 and 2^64 / 2^32, against hm_scan over [0, answer]: what a
    caller who knew the answer in advance would have paid to confirm it.

One JSON line per measurement."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402

MAX = (1 << 64) - 1


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    a, b = _lib.Context([0]), _lib.Context([0])
    for c in (a, b):  # warm: module, streams, kernels resolved
        c.scan(b"bradfitz", 0, 2 * 10**8)
        c.find(b"bradfitz", 0, 2 * 10**8, 1)
    print(json.dumps({"tool": "tools/find_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16()}),
          flush=True)
    lo, hi = 0, 2**32 - 1
    n = hi - lo + 1
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"scan_a": [], "find": [], "scan_b": []}
        for _ in range(rounds):
            sa, t = timed(lambda: a.scan(msg, lo, hi))
            res["scan_a"].append(t)
            got, t = timed(lambda: b.find(msg, lo, hi, 1))
            res["find"].append(t)
            st = b.find_stats()
            sb, t = timed(lambda: b.scan(msg, lo, hi))
            res["scan_b"].append(t)
            assert sa == sb and (got is None) == (sa[0] >= 1), (sa, sb, got)
        row = {"part": "a", "msg": name, "lo": lo, "hi": hi, "target": 1,
               "find_launches": st["launches"], "find_tasks_run": st["tasks_run"],
               "find_tasks_total": st["tasks_total"]}
        for k, v in res.items():
            row[k] = summary(v)
            row[k]["GHs"] = round(n / statistics.median(v) / 1e6, 3)
        meds = [row[k]["median_ms"] for k in ("scan_a", "scan_b")]
        row["scan_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        row["find_over_scan"] = round(min(meds) / row["find"]["median_ms"], 5)
        print(json.dumps(row), flush=True)
    for T in (2**64 // 10**3, 2**64 // 10**6, 2**64 // 2**32):
        find_ms, scan_ms = [], []
        for _ in range(rounds):
            got, t = timed(lambda: b.find(b"bradfitz", 0, MAX, T))
            find_ms.append(t)
            st = b.find_stats()
            assert got is not None and got[0] < T, (T, got)
            ref, t = timed(lambda: a.scan(b"bradfitz", 0, got[1]))
            scan_ms.append(t)
            assert ref[0] < T and (ref == got or ref[0] < got[0]), (ref, got)
        print(json.dumps({"part": "b", "msg": "bradfitz", "lo": 0, "hi": MAX, "target": T,
                          "answer": list(got), "find": summary(find_ms),
                          "scan_0_to_answer": summary(scan_ms), "launches": st["launches"],
                          "nonces_enqueued": st["nonces_enqueued"],
                          "tasks_run": st["tasks_run"], "tasks_total": st["tasks_total"],
                          "find_kernel_ms": round(st["kernel_ms"], 4)}), flush=True)
    a.close()
    b.close()


if __name__ == "__main__":
    main()

"""hm_collect_many against a loop of hm_collect on the PARENT commit's library,
in ONE process, alternating rounds (dev tool, GPU box).

usage: python tools/collect_many_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/collect_many/collect_many_rate.jsonl

(1) Per request, batch against loop.  Distinct messages (bradfitz + index, and
    BASELINE configs[2]'s 120-B message + index).  Each round runs, in turn, the
    loop of hm_collect on one context of the parent library, hm_collect_many on
    this tree's library, and the loop again on a second parent context: the
    parent-against-parent pair gives the run-to-run spread the batch figure is
    read against.  Median and minimum wall ms PER REQUEST, and batch / parent
    loop.  Rows:
      n = 1, 8, 64 over [0, 10^7] at 2^64 / 2^20 with cap = 2^13 (share-like)
      n = 1, 8, 64 over [0, 10^7] as a count (cap = 0)
      n = 64 over [0, 10^5] at 2^64 / 2^20 (small jobs)
      n = 1 over [0, 2^32 - 1] as a count: the pure fallback, expected at
          hm_collect's own time
(2) No-hit rate of the new kernel.  One request, target = 1 over [0, 2^27 - 1]
    (one full fused collect launch), against hm_scan (one fused scan launch)
    and hm_collect (per-segment launches) of the same range on this tree's
    library, in the same rounds.

One JSON line per measurement."""
import ctypes
import json
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402


class ParentCollect:
    """hm_collect of another build of the library, on its own context."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.hm_open.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                              ctypes.POINTER(ctypes.c_void_p)]
        L.hm_collect.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                 ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                 ctypes.POINTER(_lib.hm_result), ctypes.c_size_t,
                                 ctypes.POINTER(ctypes.c_uint64)]
        L.hm_close.argtypes = [ctypes.c_void_p]
        L.hm_close.restype = None
        L.hm_build_id.restype = ctypes.c_char_p
        self.L, self.h = L, ctypes.c_void_p()
        dev = (ctypes.c_int * 1)(0)
        assert L.hm_open(dev, 1, ctypes.byref(self.h)) == 0
        self.build_id = L.hm_build_id().decode()

    def loop(self, reqs, cap):
        """hm_collect request by request, each into the caller's one buffer:
        (totals, records of all requests in order)."""
        buf = (_lib.hm_result * cap)() if cap else None
        total = ctypes.c_uint64(0)
        totals, recs = [], []
        for m, lo, hi, T in reqs:
            assert self.L.hm_collect(self.h, m, len(m), lo, hi, T, buf, cap,
                                     ctypes.byref(total)) == 0
            t = int(total.value)
            totals.append(t)
            if cap:
                assert t <= cap
                words = struct.unpack_from(f"={2 * t}Q", buf)   # as _lib shapes a batch's
                recs += list(zip(words[0::2], words[1::2]))
        return totals, recs

    def close(self):
        self.L.hm_close(self.h)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5)}


def batch(c, reqs, cap):
    """(totals, records of all requests in order) of one hm_collect_many."""
    total, totals, recs = c.collect_many(reqs, cap)
    assert cap == 0 or recs is not None
    return totals, [r for rs in recs for r in rs] if cap else []


def main():
    parent = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    pa, pb, c = ParentCollect(parent), ParentCollect(parent), _lib.Context([0])
    warm = [(b"warm %d" % i, 0, 10**7, 2**64 // 2**20) for i in range(8)]
    for p in (pa, pb):  # warm: module, kernels resolved, buffers made
        p.loop(warm, 1 << 13)
    c.collect_many(warm, 1 << 13)
    c.collect(b"warm", 0, 10**7, 2**64 // 2**20, 1 << 13)
    c.scan(b"bradfitz", 0, 2**27 - 1)
    print(json.dumps({"tool": "tools/collect_many_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16(),
                      "parent_build_id": pa.build_id}), flush=True)
    share = 2**64 // 2**20
    rows = [(n, 10**7, share, 1 << 13, "share") for n in (1, 8, 64)] + \
           [(n, 10**7, share, 0, "count") for n in (1, 8, 64)] + \
           [(64, 10**5, share, 1 << 13, "small jobs"), (1, 2**32 - 1, share, 0, "fallback")]
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        for n, hi, T, cap, what in rows:
            reqs = [(msg + str(i).encode(), 0, hi, T) for i in range(n)]
            res = {"parent_a": [], "batch": [], "parent_b": []}
            for _ in range(rounds):
                ra, t = timed(lambda: pa.loop(reqs, cap))
                res["parent_a"].append(t / n)
                got, t = timed(lambda: batch(c, reqs, cap))
                res["batch"].append(t / n)
                st = c.collect_many_stats()
                rb, t = timed(lambda: pb.loop(reqs, cap))
                res["parent_b"].append(t / n)
                assert ra == rb == got, (name, what, n)
            row = {"part": 1, "msg": name, "what": what, "n": n, "lo": 0, "hi": hi,
                   "target": "2^64/2^20", "cap": cap, "total": st["total"], "fused": st["fused"],
                   "fallback": st["fallback"], "launches": st["launches"],
                   "batch_kernel_ms": round(st["kernel_ms"], 4)}
            for k, v in res.items():
                row[k] = summary(v)
            meds = [row[k]["median_ms"] for k in ("parent_a", "parent_b")]
            row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
            row["batch_over_parent"] = round(row["batch"]["median_ms"] / min(meds), 5)
            print(json.dumps(row), flush=True)
    lo, hi = 0, 2**27 - 1
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"scan_a": [], "collect_many": [], "collect": [], "scan_b": []}
        for _ in range(rounds):
            sa, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan_a"].append(t)
            got, t = timed(lambda: c.count_many([(msg, lo, hi, 1)]))
            res["collect_many"].append(t)
            st = c.collect_many_stats()
            one, t = timed(lambda: c.count(msg, lo, hi, 1))
            res["collect"].append(t)
            sb, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan_b"].append(t)
            assert sa == sb and got == [0] and one == 0 and st["fused"] == 1, (sa, sb, got, one)
        row = {"part": 2, "msg": name, "lo": lo, "hi": hi, "target": 1,
               "launches": st["launches"], "tasks": st["tasks"],
               "collect_many_kernel_ms": round(st["kernel_ms"], 4),
               "collect_kernel_ms": round(c.collect_stats()["kernel_ms"], 4),
               "collect_launches": c.collect_stats()["launches"],
               "scan_kernel_ms": round(c.stats()["kernel_ms"], 4)}
        for k, v in res.items():
            row[k] = summary(v)
            row[k]["GHs"] = round((hi - lo + 1) / statistics.median(v) / 1e6, 3)
        meds = [row[k]["median_ms"] for k in ("scan_a", "scan_b")]
        row["scan_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        row["collect_many_over_scan"] = round(min(meds) / row["collect_many"]["median_ms"], 5)
        row["collect_many_over_collect"] = round(
            row["collect"]["median_ms"] / row["collect_many"]["median_ms"], 5)
        print(json.dumps(row), flush=True)
    pa.close()
    pb.close()
    c.close()


if __name__ == "__main__":
    main()

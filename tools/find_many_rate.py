"""hm_find_many against a loop of hm_find on the PARENT commit's library, in ONE
process, alternating rounds (dev tool, GPU box).

usage: python tools/find_many_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/find_many/find_many_rate.jsonl

(1) Per request, batch against loop.  n = 1, 8, 64 distinct messages (bradfitz
    + index, and BASELINE configs[2]'s 120-B message + index) over
    [0, 2^64 - 1] at targets 2^64 / 10^3, 2^64 / 10^6 and 2^64 / 2^26.  Each
    round runs, in turn, the loop of hm_find on one context of the parent
    library, hm_find_many on this tree's library, and the loop again on a second
    parent context: the parent-against-parent pair gives the run-to-run spread
    the batch figure is read against.  Median and minimum ms PER REQUEST, and
    batch / parent loop.
(2) No-hit rate.  One request, target = 1 over [0, 2^27 - 1] (one full fused
    find launch, nothing skipped), against hm_scan of the same range (one fused
    scan launch) in the same rounds: the cost of ascending task order and the
    stop-word reads.

One JSON line per measurement."""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402

MAX = (1 << 64) - 1


class ParentFind:
    """hm_find of another build of the library, on its own context."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.hm_open.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                              ctypes.POINTER(ctypes.c_void_p)]
        L.hm_find.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64,
                              ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_lib.hm_result),
                              ctypes.POINTER(ctypes.c_int)]
        L.hm_close.argtypes = [ctypes.c_void_p]
        L.hm_close.restype = None
        L.hm_build_id.restype = ctypes.c_char_p
        self.L, self.h = L, ctypes.c_void_p()
        dev = (ctypes.c_int * 1)(0)
        assert L.hm_open(dev, 1, ctypes.byref(self.h)) == 0
        self.build_id = L.hm_build_id().decode()

    def find(self, m, lo, hi, T):
        out, found = _lib.hm_result(), ctypes.c_int(0)
        assert self.L.hm_find(self.h, m, len(m), lo, hi, T, ctypes.byref(out),
                              ctypes.byref(found)) == 0
        return (int(out.hash), int(out.nonce)) if found.value else None

    def loop(self, reqs):
        return [self.find(*r) for r in reqs]

    def close(self):
        self.L.hm_close(self.h)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5)}


def main():
    parent = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    pa, pb, c = ParentFind(parent), ParentFind(parent), _lib.Context([0])
    warm = [(b"warm %d" % i, 0, MAX, 2**64 // 10**6) for i in range(8)]
    for p in (pa, pb):  # warm: module, kernels resolved
        p.loop(warm)
    c.find_many(warm)
    c.scan(b"bradfitz", 0, 2**27 - 1)
    print(json.dumps({"tool": "tools/find_many_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16(),
                      "parent_build_id": pa.build_id}), flush=True)
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        for tname, T in (("2^64/10^3", 2**64 // 10**3), ("2^64/10^6", 2**64 // 10**6),
                         ("2^64/2^26", 2**64 // 2**26)):
            for n in (1, 8, 64):
                reqs = [(msg + str(i).encode(), 0, MAX, T) for i in range(n)]
                res = {"parent_a": [], "batch": [], "parent_b": []}
                for _ in range(rounds):
                    ra, t = timed(lambda: pa.loop(reqs))
                    res["parent_a"].append(t / n)
                    got, t = timed(lambda: c.find_many(reqs))
                    res["batch"].append(t / n)
                    st = c.find_many_stats()
                    rb, t = timed(lambda: pb.loop(reqs))
                    res["parent_b"].append(t / n)
                    assert ra == rb == got and all(g is not None for g in got), (name, tname, n)
                row = {"part": 1, "msg": name, "target": tname, "n": n,
                       "max_answer": max(g[1] for g in got), "fused": st["fused"],
                       "fallback": st["fallback"], "launches": st["launches"],
                       "tasks_run": st["tasks_run"], "tasks_total": st["tasks_total"],
                       "batch_kernel_ms": round(st["kernel_ms"], 4)}
                for k, v in res.items():
                    row[k] = summary(v)
                meds = [row[k]["median_ms"] for k in ("parent_a", "parent_b")]
                row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
                row["batch_over_parent"] = round(row["batch"]["median_ms"] / min(meds), 5)
                print(json.dumps(row), flush=True)
    lo, hi = 0, 2**27 - 1
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"scan_a": [], "find_many": [], "scan_b": []}
        for _ in range(rounds):
            sa, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan_a"].append(t)
            got, t = timed(lambda: c.find_many([(msg, lo, hi, 1)]))
            res["find_many"].append(t)
            st = c.find_many_stats()
            sb, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan_b"].append(t)
            assert sa == sb and got == [None] and st["tasks_run"] > 0, (sa, sb, got)
        row = {"part": 2, "msg": name, "lo": lo, "hi": hi, "target": 1,
               "launches": st["launches"], "tasks_run": st["tasks_run"],
               "tasks_total": st["tasks_total"], "find_many_kernel_ms": round(st["kernel_ms"], 4),
               "scan_kernel_ms": round(c.stats()["kernel_ms"], 4)}
        for k, v in res.items():
            row[k] = summary(v)
            row[k]["GHs"] = round((hi - lo + 1) / statistics.median(v) / 1e6, 3)
        meds = [row[k]["median_ms"] for k in ("scan_a", "scan_b")]
        row["scan_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        row["find_many_over_scan"] = round(min(meds) / row["find_many"]["median_ms"], 5)
        print(json.dumps(row), flush=True)
    pa.close()
    pb.close()
    c.close()


if __name__ == "__main__":
    main()

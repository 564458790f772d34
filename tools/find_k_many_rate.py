"""hm_find_k_many against a loop of hm_find_k on the PARENT commit's library, in
ONE process, alternating rounds (dev tool, GPU box).

usage: python tools/find_k_many_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/find_k_many/find_k_many_rate.jsonl

(1) Per request, batch against loop.  n = 1, 8, 64 distinct messages (bradfitz
    + index, and BASELINE configs[2]'s 120-B message + index) over
    [0, 2^64 - 1], k = 1, 8, 64, at targets 2^64 / 10^3, 2^64 / 10^6 and
    2^64 / 2^26.  Each round runs, in turn, the loop of hm_find_k on one context
    of the parent library, hm_find_k_many on this tree's library, and the loop
    again on a second parent context: the parent-against-parent pair gives the
    run-to-run spread the batch figure is read against.  Median and minimum ms
    PER REQUEST, and batch / parent loop.
(2) The moved kernels.  hm_find_k's kernels follow the new object in the code
    object, so hm_find_k itself, no-hit (target = 1, k = 64, [0, 2^32)), on the
    parent library, this tree's, and the parent again: this build / parent
    beside the parent-against-parent spread.

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

MAX = (1 << 64) - 1


class ParentFindK:
    """hm_find_k of another build of the library, on its own context."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.hm_open.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                              ctypes.POINTER(ctypes.c_void_p)]
        L.hm_find_k.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                ctypes.c_size_t, ctypes.POINTER(_lib.hm_result),
                                ctypes.POINTER(ctypes.c_size_t)]
        L.hm_close.argtypes = [ctypes.c_void_p]
        L.hm_close.restype = None
        L.hm_build_id.restype = ctypes.c_char_p
        self.L, self.h = L, ctypes.c_void_p()
        dev = (ctypes.c_int * 1)(0)
        assert L.hm_open(dev, 1, ctypes.byref(self.h)) == 0
        self.build_id = L.hm_build_id().decode()

    def find_k(self, m, lo, hi, T, k):
        buf, n = (_lib.hm_result * k)(), ctypes.c_size_t(0)
        assert self.L.hm_find_k(self.h, m, len(m), lo, hi, T, k, buf, ctypes.byref(n)) == 0
        words = struct.unpack_from(f"={2 * n.value}Q", buf) if n.value else ()
        return list(zip(words[0::2], words[1::2]))

    def loop(self, reqs):
        return [self.find_k(*r) for r in reqs]

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
    pa, pb, c = ParentFindK(parent), ParentFindK(parent), _lib.Context([0])
    warm = [(b"warm %d" % i, 0, MAX, 2**64 // 10**6, 8) for i in range(8)]
    for p in (pa, pb):  # warm: module, kernels resolved, buffers made
        p.loop(warm)
    c.find_k_many(warm)
    c.find_k(*warm[0])
    print(json.dumps({"tool": "tools/find_k_many_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16(),
                      "parent_build_id": pa.build_id}), flush=True)
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        for tname, T in (("2^64/10^3", 2**64 // 10**3), ("2^64/10^6", 2**64 // 10**6),
                         ("2^64/2^26", 2**64 // 2**26)):
            for k in (1, 8, 64):
                for n in (1, 8, 64):
                    reqs = [(msg + str(i).encode(), 0, MAX, T, k) for i in range(n)]
                    res = {"parent_a": [], "batch": [], "parent_b": []}
                    for _ in range(rounds):
                        ra, t = timed(lambda: pa.loop(reqs))
                        res["parent_a"].append(t / n)
                        got, t = timed(lambda: c.find_k_many(reqs))
                        res["batch"].append(t / n)
                        st = c.find_k_many_stats()
                        rb, t = timed(lambda: pb.loop(reqs))
                        res["parent_b"].append(t / n)
                        assert ra == rb == got and all(len(g) == k for g in got), (name, tname, n, k)
                    row = {"part": 1, "msg": name, "target": tname, "n": n, "k": k,
                           "max_answer": max(g[-1][1] for g in got), "fused": st["fused"],
                           "fallback": st["fallback"], "overflow": st["overflow"],
                           "launches": st["launches"], "records": st["records"],
                           "tasks_run": st["tasks_run"], "tasks_total": st["tasks_total"],
                           "batch_kernel_ms": round(st["kernel_ms"], 4)}
                    for key, v in res.items():
                        row[key] = summary(v)
                    meds = [row[key]["median_ms"] for key in ("parent_a", "parent_b")]
                    row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
                    row["batch_over_parent"] = round(row["batch"]["median_ms"] / min(meds), 5)
                    print(json.dumps(row), flush=True)
    lo, hi = 0, 2**32 - 1
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"parent_a": [], "this": [], "parent_b": []}
        for _ in range(rounds):
            ra, t = timed(lambda: pa.find_k(msg, lo, hi, 1, 64))
            res["parent_a"].append(t)
            got, t = timed(lambda: c.find_k(msg, lo, hi, 1, 64))
            res["this"].append(t)
            st = c.find_k_stats()
            rb, t = timed(lambda: pb.find_k(msg, lo, hi, 1, 64))
            res["parent_b"].append(t)
            assert ra == rb == got == [] and st["tasks_run"] == st["tasks_total"] > 0, st
        row = {"part": 2, "msg": name, "lo": lo, "hi": hi, "target": 1, "k": 64,
               "launches": st["launches"], "tasks_total": st["tasks_total"]}
        for key, v in res.items():
            row[key] = summary(v)
            row[key]["GHs"] = round((hi - lo + 1) / statistics.median(v) / 1e6, 3)
        meds = [row[key]["median_ms"] for key in ("parent_a", "parent_b")]
        row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        row["this_over_parent"] = round(row["this"]["median_ms"] / min(meds), 5)
        print(json.dumps(row), flush=True)
    pa.close()
    pb.close()
    c.close()


if __name__ == "__main__":
    main()

"""hm_find_k against hm_scan, hm_find and, on the PARENT commit's library, the
loop of hm_find calls it replaces, in ONE process, alternating rounds (dev tool,
GPU box).

usage: python tools/find_k_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/find_k/find_k_rate.jsonl

(a) No-hit rate.  hm_find_k(target = 1, k = 64) hashes every nonce of the range
    and finds nothing, so its wall time is the find_k kernels' full-scan cost.
    Per message (bradfitz, and BASELINE configs[2]'s 120-B message) over
    [0, 2^32) each round runs scan, find_k, find, scan in turn: the
    scan-against-scan pair gives the run-to-run spread.
(b) Share loop.  Over [0, 2^64 - 1] at 2^64 / 10^6 and 2^64 / 2^26, k = 1, 8,
    64, 1024.  Each round runs, in turn: the loop of k hm_find calls on one
    context of the parent library, each restarting at answer + 1; one
    hm_find_k on this tree's library; the loop again on a second parent
    context (the parent-against-parent pair gives the spread); and one
    hm_collect over [0, answer_k] on the parent library -- what a caller who
    knew the k-th answer in advance would have paid (the floor).
(c) Dense.  2^64 / 10^3 with k = 64, the same four columns: the in-flight tasks
    hold more hits than the buffer, so the overflow path is expected.

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


class Parent:
    """hm_find and hm_collect of another build of the library, on its own context."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.hm_open.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                              ctypes.POINTER(ctypes.c_void_p)]
        L.hm_find.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64,
                              ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_lib.hm_result),
                              ctypes.POINTER(ctypes.c_int)]
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

    def find_loop(self, m, lo, hi, T, k):
        """k hm_find calls, each restarting at answer + 1: the records."""
        out, found, recs = _lib.hm_result(), ctypes.c_int(0), []
        while len(recs) < k and lo <= hi:
            assert self.L.hm_find(self.h, m, len(m), lo, hi, T, ctypes.byref(out),
                                  ctypes.byref(found)) == 0
            if not found.value:
                break
            recs.append((int(out.hash), int(out.nonce)))
            lo = int(out.nonce) + 1
        return recs

    def collect(self, m, lo, hi, T, cap):
        buf = (_lib.hm_result * cap)()
        total = ctypes.c_uint64(0)
        assert self.L.hm_collect(self.h, m, len(m), lo, hi, T, buf, cap, ctypes.byref(total)) == 0
        t = int(total.value)
        assert t <= cap
        words = struct.unpack_from(f"={2 * t}Q", buf)
        return list(zip(words[0::2], words[1::2]))

    def close(self):
        self.L.hm_close(self.h)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def share_row(pa, pb, c, part, msg, T, tname, k, rounds):
    res = {"parent_loop_a": [], "find_k": [], "parent_loop_b": [], "parent_collect_floor": []}
    for _ in range(rounds):
        ra, t = timed(lambda: pa.find_loop(msg, 0, MAX, T, k))
        res["parent_loop_a"].append(t)
        got, t = timed(lambda: c.find_k(msg, 0, MAX, T, k))
        res["find_k"].append(t)
        st = c.find_k_stats()
        rb, t = timed(lambda: pb.find_loop(msg, 0, MAX, T, k))
        res["parent_loop_b"].append(t)
        floor, t = timed(lambda: pa.collect(msg, 0, got[-1][1], T, 2 * k + 4096))
        res["parent_collect_floor"].append(t)
        assert ra == rb == got == floor and len(got) == k, (tname, k)
    row = {"part": part, "msg": "bradfitz", "lo": 0, "hi": MAX, "target": tname, "k": k,
           "rounds": rounds, "answer_k": got[-1][1], "launches": st["launches"],
           "nonces_enqueued": st["nonces_enqueued"], "tasks_run": st["tasks_run"],
           "tasks_total": st["tasks_total"], "records": st["records"],
           "fallback": st["fallback"], "find_k_kernel_ms": round(st["kernel_ms"], 4)}
    for name, v in res.items():
        row[name] = summary(v)
    meds = [row[n]["median_ms"] for n in ("parent_loop_a", "parent_loop_b")]
    row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
    row["find_k_over_parent_loop"] = round(row["find_k"]["median_ms"] / min(meds), 5)
    row["find_k_over_floor"] = round(
        row["find_k"]["median_ms"] / row["parent_collect_floor"]["median_ms"], 5)
    print(json.dumps(row), flush=True)


def main():
    parent = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    pa, pb, c = Parent(parent), Parent(parent), _lib.Context([0])
    for p in (pa, pb):  # warm: module, kernels resolved, buffers made
        p.find_loop(b"warm", 0, MAX, 2**64 // 10**6, 2)
        p.collect(b"warm", 0, 10**7, 2**64 // 10**6, 1 << 13)
    c.scan(b"bradfitz", 0, 2 * 10**8)
    c.find(b"bradfitz", 0, 2 * 10**8, 1)
    c.find_k(b"bradfitz", 0, 2 * 10**8, 1, 64)
    c.find_k(b"warm", 0, MAX, 2**64 // 10**6, 1024)
    print(json.dumps({"tool": "tools/find_k_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16(),
                      "parent_build_id": pa.build_id}), flush=True)
    lo, hi = 0, 2**32 - 1
    n = hi - lo + 1
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"scan_a": [], "find_k": [], "find": [], "scan_b": []}
        for _ in range(rounds):
            sa, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan_a"].append(t)
            got, t = timed(lambda: c.find_k(msg, lo, hi, 1, 64))
            res["find_k"].append(t)
            st = c.find_k_stats()
            one, t = timed(lambda: c.find(msg, lo, hi, 1))
            res["find"].append(t)
            sb, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan_b"].append(t)
            assert sa == sb and got == [] and one is None and sa[0] >= 1, (sa, sb, got, one)
            assert st["tasks_run"] == st["tasks_total"], st
        row = {"part": "a", "msg": name, "lo": lo, "hi": hi, "target": 1, "k": 64,
               "launches": st["launches"], "tasks_total": st["tasks_total"]}
        for k, v in res.items():
            row[k] = summary(v)
            row[k]["GHs"] = round(n / statistics.median(v) / 1e6, 3)
        meds = [row[k]["median_ms"] for k in ("scan_a", "scan_b")]
        row["scan_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        row["find_k_over_scan"] = round(min(meds) / row["find_k"]["median_ms"], 5)
        row["find_over_scan"] = round(min(meds) / row["find"]["median_ms"], 5)
        print(json.dumps(row), flush=True)
    for T, tname in ((2**64 // 10**6, "2^64/10^6"), (2**64 // 2**26, "2^64/2^26")):
        for k in (1, 8, 64, 1024):
            share_row(pa, pb, c, "b", b"bradfitz", T, tname, k, rounds if k < 1024 else min(rounds, 5))
    share_row(pa, pb, c, "c", b"bradfitz", 2**64 // 10**3, "2^64/10^3", 64, rounds)
    pa.close()
    pb.close()
    c.close()


if __name__ == "__main__":
    main()

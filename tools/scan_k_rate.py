"""hm_scan_k against hm_scan and hm_collect in ONE process, alternating rounds,
and this tree's hm_scan against the PARENT commit's (dev tool, GPU box).

usage: python tools/scan_k_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/scan_k/scan_k_rate.jsonl

(a) [0, 2^32) on b"bradfitz" and BASELINE configs[2]'s 120-B message.  Each
    round runs the parent library's hm_scan, this tree's hm_scan, this tree's
    hm_scan_k at k = 1, 8, 32, and the parent's hm_scan again on a second
    context: the parent-against-parent pair is the run-to-run spread every
    ratio is read against.
(b) [0, 10^7] on b"bradfitz": hm_scan_k at k = 32 against the parent library's
    hm_scan on two contexts (rows parent_scan_a, parent_scan_b) and against
    the route it replaces -- hm_collect at the guessed target 4 k 2^64 / span
    (about 4 k records) plus the host's sort of them.

Median and minimum wall ms, GH/s of the medians; hm_scan_k's device-side
diagnostics of the last round.  One JSON line per measurement."""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402


def other_context(path):
    """A _lib.Context over another build of the library (the calls both have)."""
    L = ctypes.CDLL(path)
    for name in ("hm_open", "hm_close", "hm_scan", "hm_build_id"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    h = ctypes.c_void_p()
    dev = (ctypes.c_int * 1)(0)
    assert L.hm_open(dev, 1, ctypes.byref(h)) == 0
    c = _lib.Context.__new__(_lib.Context)
    c._h, c._lib = h, L
    return c, L.hm_build_id().decode()


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms, n):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "GHs": round(n / statistics.median(ms) / 1e6, 3)}


def main():
    parent = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    pa, parent_id = other_context(parent)
    pb, _ = other_context(parent)
    c = _lib.Context([0])
    for x in (pa, pb, c):  # warm: module, streams, kernels resolved
        x.scan(b"bradfitz", 0, 2 * 10**8)
    c.scan_k(b"bradfitz", 0, 2 * 10**8, 32)
    print(json.dumps({"tool": "tools/scan_k_rate.py", "rounds": rounds, "parent_build_id": parent_id,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16()}),
          flush=True)
    lo, hi = 0, 2**32 - 1
    n = hi - lo + 1
    ks = (1, 8, 32)
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"parent_a": [], "scan": [], "parent_b": []}
        res.update({f"scan_k{k}": [] for k in ks})
        diag = {}
        for _ in range(rounds):
            want, t = timed(lambda: pa.scan(msg, lo, hi))
            res["parent_a"].append(t)
            got, t = timed(lambda: c.scan(msg, lo, hi))
            res["scan"].append(t)
            assert got == want
            for k in ks:
                lst, t = timed(lambda: c.scan_k(msg, lo, hi, k))
                res[f"scan_k{k}"].append(t)
                assert lst[0] == want and len(lst) == k, (k, lst[:2], want)
                st = c.scan_k_stats()
                diag[k] = {"kernel_ms": round(st["kernel_ms"], 4), "inserted": st["inserted"],
                           "compactions": st["compactions"], "launches": st["launches"]}
            got, t = timed(lambda: pb.scan(msg, lo, hi))
            res["parent_b"].append(t)
            assert got == want
        row = {"part": "a", "msg": name, "lo": lo, "hi": hi}
        for key, v in res.items():
            row[key] = summary(v, n)
        meds = [row[key]["median_ms"] for key in ("parent_a", "parent_b")]
        row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        # rates relative to the parent's hm_scan (1.0 = as fast)
        row["scan_over_parent"] = round(min(meds) / row["scan"]["median_ms"], 5)
        for k in ks:
            row[f"scan_k{k}_over_parent"] = round(min(meds) / row[f"scan_k{k}"]["median_ms"], 5)
            row[f"scan_k{k}_over_scan"] = round(row["scan"]["median_ms"] /
                                                row[f"scan_k{k}"]["median_ms"], 5)
            row[f"scan_k{k}_diag"] = diag[k]
        print(json.dumps(row), flush=True)

    msg, lo, hi, k = b"bradfitz", 0, 10**7, 32
    n = hi - lo + 1
    T = 4 * k * 2**64 // n
    cap = 64 * k
    res = {"parent_scan_a": [], "scan_k32": [], "collect_sort": [], "parent_scan_b": []}
    for x in (c,):
        x.collect(msg, lo, hi, T, cap)
    for _ in range(rounds):
        want, t = timed(lambda: pa.scan(msg, lo, hi))
        res["parent_scan_a"].append(t)
        lst, t = timed(lambda: c.scan_k(msg, lo, hi, k))
        res["scan_k32"].append(t)

        def guessed():
            total, recs = c.collect(msg, lo, hi, T, cap)
            assert recs is not None and total >= k
            return sorted(recs)[:k]
        ref, t = timed(guessed)
        res["collect_sort"].append(t)
        assert ref == lst and lst[0] == want
        _, t = timed(lambda: pb.scan(msg, lo, hi))
        res["parent_scan_b"].append(t)
    row = {"part": "b", "msg": "bradfitz", "lo": lo, "hi": hi, "k": k, "collect_target": T,
           "collect_records": c.collect_stats()["total"]}
    for key, v in res.items():
        row[key] = summary(v, n)
    meds = [row[key]["median_ms"] for key in ("parent_scan_a", "parent_scan_b")]
    row["parent_scan_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
    row["scan_k32_over_parent_scan"] = round(min(meds) / row["scan_k32"]["median_ms"], 5)
    row["scan_k32_over_collect_sort"] = round(row["collect_sort"]["median_ms"] /
                                              row["scan_k32"]["median_ms"], 5)
    st = c.scan_k_stats()
    row["scan_k32_diag"] = {"kernel_ms": round(st["kernel_ms"], 4), "inserted": st["inserted"],
                            "compactions": st["compactions"], "launches": st["launches"]}
    print(json.dumps(row), flush=True)
    for x in (pa, pb, c):
        x.close()


if __name__ == "__main__":
    main()

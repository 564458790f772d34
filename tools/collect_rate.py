"""hm_collect against hm_scan and hm_find in ONE process, alternating rounds
(dev tool, GPU box).

usage: python tools/collect_rate.py [ROUNDS] > profiles/collect/collect_rate.jsonl

(a) No-hit rate.  At target = 1 nothing qualifies, so count and collect hash
    every nonce and their wall time is the collect kernels' full-scan cost.
    Per message (bradfitz, and BASELINE configs[2]'s 120-B message) over
    [0, 2^32) each round runs scan, find, count, collect, scan in turn on two
    contexts: the scan-against-scan pair gives the run-to-run spread, and
    hm_find's ratio to hm_scan in the same run is the yardstick collect's
    ratio is read against (the same loop, enqueued without host round trips).
(b) Share-like target 2^64 / 2^20 with cap = 2^13 over [0, 2^32): ~4096
    records.
(c) Dense target 2^64 / 64 over [0, 2^32): ~6.7 * 10^7 hits, as a count and
    with cap = HM_COLLECT_CAP_MAX (an overflow: the cursor's cost until the
    buffer is full, then the per-wave flag); and over [0, 2^29), where the
    ~8.4 * 10^6 records fit: the cursor throughout, the readback and the sort.

Median and minimum wall ms, GH/s of the medians.  One JSON line per
measurement."""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms, n):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "GHs": round(n / statistics.median(ms) / 1e6, 3)}


def raw_collect(c, buf, msg, lo, hi, T, cap):
    """hm_collect into a buffer made beforehand (256 MiB at the largest cap:
    allocating it is not the call's time): (total, records written)."""
    total = ctypes.c_uint64(0)
    rc = _lib.load().hm_collect(c._h, msg, len(msg), lo, hi, T, buf, cap, ctypes.byref(total))
    assert rc == _lib.HM_OK, rc
    t = int(total.value)
    return t, (t if t <= cap else None)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    a, b = _lib.Context([0]), _lib.Context([0])
    for c in (a, b):  # warm: module, streams, kernels resolved, the largest buffer made
        c.scan(b"bradfitz", 0, 2 * 10**8)
        c.find(b"bradfitz", 0, 2 * 10**8, 1)
        c.count(b"bradfitz", 0, 2 * 10**8, 1)
    b.collect(b"bradfitz", 0, 10**6, 1, _lib.HM_COLLECT_CAP_MAX)
    print(json.dumps({"tool": "tools/collect_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16()}),
          flush=True)
    lo, hi = 0, 2**32 - 1
    n = hi - lo + 1
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        res = {"scan_a": [], "find": [], "count": [], "collect": [], "scan_b": []}
        kernel = {"count": [], "collect": []}
        for _ in range(rounds):
            sa, t = timed(lambda: a.scan(msg, lo, hi))
            res["scan_a"].append(t)
            got, t = timed(lambda: b.find(msg, lo, hi, 1))
            res["find"].append(t)
            cnt, t = timed(lambda: b.count(msg, lo, hi, 1))
            res["count"].append(t)
            kernel["count"].append(b.collect_stats()["kernel_ms"])
            col, t = timed(lambda: b.collect(msg, lo, hi, 1, 2**13))
            res["collect"].append(t)
            st = b.collect_stats()
            kernel["collect"].append(st["kernel_ms"])
            sb, t = timed(lambda: b.scan(msg, lo, hi))
            res["scan_b"].append(t)
            assert sa == sb and got is None and cnt == 0 and col == (0, []), (sa, sb, got, cnt, col)
        row = {"part": "a", "msg": name, "lo": lo, "hi": hi, "target": 1,
               "collect_launches": st["launches"]}
        for k, v in res.items():
            row[k] = summary(v, n)
        for k, v in kernel.items():
            row[k]["kernel_median_ms"] = round(statistics.median(v), 4)
        meds = [row[k]["median_ms"] for k in ("scan_a", "scan_b")]
        row["scan_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        for k in ("find", "count", "collect"):
            row[f"{k}_over_scan"] = round(min(meds) / row[k]["median_ms"], 5)
        print(json.dumps(row), flush=True)
    msg = b"bradfitz"
    buf = (_lib.hm_result * _lib.HM_COLLECT_CAP_MAX)()
    for part, hi, T, caps in (("b", 2**32 - 1, 2**64 // 2**20, (2**13,)),
                              ("c", 2**32 - 1, 2**64 // 64, (0, _lib.HM_COLLECT_CAP_MAX)),
                              ("c", 2**29 - 1, 2**64 // 64, (_lib.HM_COLLECT_CAP_MAX,))):
        n = hi - lo + 1
        for cap in caps:
            ms, kms, scan_ms = [], [], []
            for _ in range(rounds):
                _, t = timed(lambda: a.scan(msg, lo, hi))
                scan_ms.append(t)
                (total, recs), t = timed(lambda: raw_collect(b, buf, msg, lo, hi, T, cap))
                ms.append(t)
                st = b.collect_stats()
                kms.append(st["kernel_ms"])
            row = {"part": part, "msg": "bradfitz", "lo": lo, "hi": hi, "target": T, "cap": cap,
                   "total": total, "overflow": st["overflow"],
                   "records": recs,
                   "collect": summary(ms, n), "scan": summary(scan_ms, n),
                   "kernel_median_ms": round(statistics.median(kms), 4)}
            row["collect_over_scan"] = round(row["scan"]["median_ms"] / row["collect"]["median_ms"], 5)
            print(json.dumps(row), flush=True)
    a.close()
    b.close()


if __name__ == "__main__":
    main()

"""hm_cancel: what the relay wave costs the find-family calls, against the PARENT
commit's library in ONE process with alternating rounds, and how long a cancel
takes (dev tool, GPU box).

usage: python tools/cancel_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/cancel/cancel_rate.jsonl

(1) Cost of the relay.  No-hit calls (target = 1), so every task runs and every
    task of the relay wave polls the flag: hm_find and hm_find_k (k = 64) over
    [0, 2^32), b"bradfitz" and BASELINE configs[2]'s 120-B message; hm_find_many
    and hm_find_k_many, 8 requests of 2^27 nonces (each one fused launch).  Each
    round runs the parent library, this tree's, and the parent again on a second
    context: the parent-against-parent pair is the run-to-run spread the ratio is
    read against.
(2) Latency.  hm_cancel_stats.latency_ms (hm_cancel's flag store to the cancelled
    call's return), the call's wall time and the launches in flight, for the
    shapes of tests/test_gpu_cancel.py: tiled, chained, generic, both batches,
    and the tiled case again with the cancel landing in the launch's first ms.

One JSON line per measurement."""
import ctypes
import json
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402


def other_context(path):
    """A _lib.Context over another build of the library (the calls both have)."""
    L = ctypes.CDLL(path)
    for name in ("hm_open", "hm_close", "hm_find", "hm_find_k", "hm_find_many",
                 "hm_find_k_many", "hm_build_id"):
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


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5)}


def cost(rounds, pa, pb, c):
    long120 = bench.long120()
    lo, hi = 0, 2**32 - 1
    rows = []
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", long120)):
        rows.append(("hm_find", name, hi - lo + 1, lambda x, m=msg: x.find(m, lo, hi, 1), None))
        rows.append(("hm_find_k", name, hi - lo + 1,
                     lambda x, m=msg: x.find_k(m, lo, hi, 1, 64), []))
    reqs = [(b"relay cost %d" % i, 0, 2**27 - 1, 1) for i in range(8)]
    rows.append(("hm_find_many", "8 x 2^27", 8 * 2**27, lambda x: x.find_many(reqs), [None] * 8))
    reqs_k = [r + (64,) for r in reqs]
    rows.append(("hm_find_k_many", "8 x 2^27", 8 * 2**27,
                 lambda x: x.find_k_many(reqs_k), [[]] * 8))
    for call, what, nonces, fn, want in rows:
        for x in (pa, c, pb):  # warm: kernels resolved, buffers made
            fn(x)
        res = {"parent_a": [], "this": [], "parent_b": []}
        for _ in range(rounds):
            for key, x in (("parent_a", pa), ("this", c), ("parent_b", pb)):
                got, t = timed(lambda: fn(x))
                assert got == want, (call, what, key, got)
                res[key].append(t)
        row = {"part": 1, "call": call, "what": what, "nonces": nonces, "target": 1}
        for key, v in res.items():
            row[key] = summary(v)
            row[key]["GHs"] = round(nonces / statistics.median(v) / 1e6, 3)
        meds = [row[key]["median_ms"] for key in ("parent_a", "parent_b")]
        row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
        row["this_over_parent"] = round(row["this"]["median_ms"] / min(meds), 5)
        row["this_over_parent_mean"] = round(row["this"]["median_ms"] / (sum(meds) / 2), 5)
        print(json.dumps(row), flush=True)


def latency(rounds, c):
    long120 = bench.long120()
    lo, hi = 10**10, 7 * 10**10
    many = [(b"cancel-job-%d" % i, 10**10, 2 * 10**10, 1) for i in range(8)]
    shapes = [
        ("tiled", 0.2, lambda: c.find(b"bradfitz", lo, hi, 1), None),
        ("chained", 0.2, lambda: c.find(long120, lo, hi, 1), None),
        ("find_k_tiled", 0.2, lambda: c.find_k(b"bradfitz", lo, hi, 1, 64), None),
        ("find_k_chained", 0.2, lambda: c.find_k(long120, lo, hi, 1, 64), None),
        ("generic", 0.05, lambda: c.find(b"bradfitz", 0, 2**33, 1), _lib.HM_OPT_FORCE_GENERIC),
        ("find_many", 0.1, lambda: c.find_many(many), None),
        ("find_k_many", 0.1, lambda: c.find_k_many([r + (4,) for r in many]), None),
        ("tiled_first_ms", 0.002, lambda: c.find(b"bradfitz", lo, hi, 1), None),
    ]
    for name, delay, fn, opt in shapes:
        lat, inflight, signalled = [], [], 0
        if opt is not None:
            c.set_option(opt, 1)
        for _ in range(rounds):
            got = []

            def canceller():
                time.sleep(delay)
                got.append(c.cancel())

            th = threading.Thread(target=canceller)
            th.start()
            try:
                fn()
                cancelled = False
            except _lib.HipMinerCancelled:
                cancelled = True
            th.join()
            if not cancelled:
                continue
            st = c.cancel_stats()
            signalled += got == [True]
            lat.append(st["latency_ms"])
            inflight.append(st["launches_in_flight"])
        if opt is not None:
            c.set_option(opt, 0)
        row = {"part": 2, "shape": name, "cancel_after_ms": delay * 1e3, "rounds": rounds,
               "cancelled": len(lat), "signalled": signalled}
        if lat:
            row.update({"latency_ms": {"median": round(statistics.median(lat), 4),
                                       "min": round(min(lat), 4), "max": round(max(lat), 4)},
                        "launches_in_flight": sorted(set(inflight))})
        print(json.dumps(row), flush=True)


def main():
    parent = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    (pa, pid), (pb, _), c = other_context(parent), other_context(parent), _lib.Context([0])
    print(json.dumps({"tool": "tools/cancel_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16(),
                      "parent_build_id": pid}), flush=True)
    cost(rounds, pa, pb, c)
    latency(max(3, rounds // 2 + 1), c)
    for x in (pa, pb, c):
        x.close()


if __name__ == "__main__":
    main()

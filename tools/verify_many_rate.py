"""hm_verify_many against a loop of hm_verify on the PARENT commit's library, in
ONE process, alternating rounds (dev tool, GPU box).

usage: python tools/verify_many_rate.py PARENT_LIBHIPMINER_SO [ROUNDS]
           > profiles/verify_many/verify_many_rate.jsonl

(1) Many small lists.  64 and 1024 requests x 64 and 1024 records each, distinct
    messages (bradfitz + index, and BASELINE configs[2]'s 120-B message + index),
    honest records with nonces of every digit count, target 2^64 - 1: none bad.
    Each round runs, in turn, the loop of hm_verify on one context of the parent
    library, hm_verify_many on this tree's library, and the loop again on a
    second parent context: the parent-against-parent pair gives the run-to-run
    spread the batch figure is read against.  Median and minimum ms PER REQUEST,
    and batch / parent loop.
(2) One large list.  One request of 2^22 records against hm_verify of the same
    list: what the host packing pass costs a caller who has no batch.

Both sides are called through ctypes with arrays built beforehand, count only
(cap = 0); the loop's per-call Python overhead (about a microsecond) is part of
the parent figure.  One JSON line per measurement."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402

MAX = (1 << 64) - 1
U64P = ctypes.POINTER(ctypes.c_uint64)
RECP = ctypes.POINTER(_lib.hm_result)
# nonces of d digits: LO[d] .. LO[d] + SPAN[d] - 1
LO = np.array([0, 0] + [10**(d - 1) for d in range(2, 21)], dtype=np.uint64)
SPAN = np.array([1] + [min(10**d - 1, MAX) + 1 - int(LO[d]) for d in range(1, 21)],
                dtype=np.uint64)


class ParentVerify:
    """hm_verify of another build of the library, on its own context."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.hm_open.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                              ctypes.POINTER(ctypes.c_void_p)]
        L.hm_verify.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, RECP,
                                ctypes.c_size_t, ctypes.c_uint64, U64P, ctypes.c_size_t, U64P]
        L.hm_close.argtypes = [ctypes.c_void_p]
        L.hm_close.restype = None
        L.hm_build_id.restype = ctypes.c_char_p
        self.L, self.h = L, ctypes.c_void_p()
        dev = (ctypes.c_int * 1)(0)
        assert L.hm_open(dev, 1, ctypes.byref(self.h)) == 0
        self.build_id = L.hm_build_id().decode()

    def loop(self, calls):
        """calls: [(msg, len, recs pointer, n, target)]; the summed bad count."""
        bad, total, verify, h = ctypes.c_uint64(0), 0, self.L.hm_verify, self.h
        ref = ctypes.byref(bad)
        for m, ln, p, n, T in calls:
            assert verify(h, m, ln, p, n, T, None, 0, ref) == 0
            total += bad.value
        return total

    def close(self):
        self.L.hm_close(self.h)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5)}


def honest(c, msg, n, rng):
    """n honest records of msg: nonces of every digit count, the GPU's hashes."""
    d = rng.integers(1, 21, n)
    nonces = LO[d] + rng.integers(0, 2**64, n, dtype=np.uint64) % SPAN[d]
    recs = np.empty((n, 2), dtype=np.uint64)
    recs[:, 0] = c.hash_many(msg, nonces)
    recs[:, 1] = nonces
    return recs


def measure(pa, pb, c, reqs, rounds):
    """reqs: [(msg, records, target)].  Per-request ms of the three sides."""
    lib = _lib.load()
    arr, n, keep = _lib.verify_requests(reqs)
    calls = [(m, len(m), r.ctypes.data_as(RECP), r.shape[0], reqs[i][2])
             for i, (m, r) in enumerate(keep)]
    per = (ctypes.c_uint64 * n)()
    bad = ctypes.c_uint64(0)

    def batch():
        assert lib.hm_verify_many(c._h, arr, n, per, None, 0, ctypes.byref(bad)) == 0
        return bad.value
    res = {"parent_a": [], "batch": [], "parent_b": []}
    for _ in range(rounds):
        ra, t = timed(lambda: pa.loop(calls))
        res["parent_a"].append(t / n)
        got, t = timed(batch)
        res["batch"].append(t / n)
        rb, t = timed(lambda: pb.loop(calls))
        res["parent_b"].append(t / n)
        assert ra == rb == got == 0, (ra, rb, got)
    st = c.verify_many_stats()
    row = {"launches": st["launches"], "copies": st["copies"], "tasks": st["tasks"],
           "records": st["records"], "batch_kernel_ms": round(st["kernel_ms"], 4),
           "batch_copy_ms": round(st["copy_ms"], 4)}
    for k, v in res.items():
        row[k] = summary(v)
    meds = [row[k]["median_ms"] for k in ("parent_a", "parent_b")]
    row["parent_spread"] = round(abs(meds[0] - meds[1]) / min(meds), 5)
    row["batch_over_parent"] = round(row["batch"]["median_ms"] / min(meds), 5)
    return row


def main():
    parent = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    pa, pb, c = ParentVerify(parent), ParentVerify(parent), _lib.Context([0])
    rng = np.random.default_rng(14)
    warm = [(b"warm %d" % i, honest(c, b"warm %d" % i, 100, rng), MAX) for i in range(4)]
    measure(pa, pb, c, warm, 2)  # warm: module, kernels resolved, buffers made
    print(json.dumps({"tool": "tools/verify_many_rate.py", "rounds": rounds,
                      "build_id": _lib.build_id(), "code_object": _lib.code_object_sha16(),
                      "parent_build_id": pa.build_id}), flush=True)
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        for nreq in (64, 1024):
            for nrec in (64, 1024):
                reqs = []
                for i in range(nreq):
                    m = msg + str(i).encode()
                    reqs.append((m, honest(c, m, nrec, rng), MAX))
                row = {"part": 1, "msg": name, "requests": nreq, "records_each": nrec}
                row.update(measure(pa, pb, c, reqs, rounds))
                print(json.dumps(row), flush=True)
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        reqs = [(msg, honest(c, msg, 2**22, rng), MAX)]
        row = {"part": 2, "msg": name, "requests": 1, "records_each": 2**22}
        row.update(measure(pa, pb, c, reqs, rounds))
        print(json.dumps(row), flush=True)
    pa.close()
    pb.close()
    c.close()


if __name__ == "__main__":
    main()

"""hm_verify and hm_hash_many against their host twins in ONE process,
alternating rounds (dev tool, GPU box).

usage: python tools/verify_rate.py [ROUNDS] [--out FILE]
       (appends JSON lines to FILE, default profiles/verify/verify_rate.jsonl,
       and prints them)

For bradfitz and BASELINE configs[2]'s 120-B message:
(a) hm_collect over [0, 2^32) at target 2^64 / 2^10: about 2^22 records.
    hm_verify of them (none bad): wall_ms, and hm_verify_stats' kernel_ms and
    copy_ms -- whether the copy in (16 bytes per record) or the kernel bounds
    the call -- and records/s.
(b) The same list through hm_verify_cpu with 1 and with 16 threads.
(c) hm_hash_many of as many random 64-bit nonces (mixed digit counts: the
    divergent path) against as many 10-digit nonces (the uniform path).
(d) Lists of 2^10, 2^14 and 2^18 records through hm_verify and through
    hm_verify_cpu with 16 threads: the size at which the GPU call overtakes
    the host.

Each round runs its measurements in turn; median and minimum ms per
measurement.  One JSON line per measurement."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402

RECP = ctypes.POINTER(_lib.hm_result)
U64P = ctypes.POINTER(ctypes.c_uint64)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summary(ms, n):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "Mrec_s": round(n / med / 1e3, 3), "ns_per_record": round(med * 1e6 / n, 3)}


def med(xs):
    return round(statistics.median(xs), 4)


def gpu_verify(c, msg, recs, T):
    bad = ctypes.c_uint64(0)
    rc = _lib.load().hm_verify(c._h, msg, len(msg), recs.ctypes.data_as(RECP), recs.shape[0], T,
                               None, 0, ctypes.byref(bad))
    assert rc == _lib.HM_OK, rc
    return int(bad.value)


def cpu_verify(msg, recs, T, threads):
    bad = ctypes.c_uint64(0)
    rc = _lib.load().hm_verify_cpu(msg, len(msg), recs.ctypes.data_as(RECP), recs.shape[0], T,
                                   threads, None, 0, ctypes.byref(bad))
    assert rc == _lib.HM_OK, rc
    return int(bad.value)


def gpu_hash_many(c, msg, nonces, out):
    rc = _lib.load().hm_hash_many(c._h, msg, len(msg), nonces.ctypes.data_as(U64P), nonces.size,
                                  out.ctypes.data_as(U64P))
    assert rc == _lib.HM_OK, rc


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "verify", "verify_rate.jsonl")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    rounds = int(args[0]) if args else 7
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    sink = open(out_path, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    c = _lib.Context([0])
    c.collect(b"bradfitz", 0, 10**6, 1, 2**23)   # warm: module, the largest collect buffer
    emit({"tool": "tools/verify_rate.py", "rounds": rounds, "build_id": _lib.build_id(),
          "code_object": _lib.code_object_sha16()})
    T = 2**64 // 2**10
    buf = np.empty((2**23, 2), dtype=np.uint64)
    rng = np.random.default_rng(1)
    for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
        total = ctypes.c_uint64(0)
        rc = _lib.load().hm_collect(c._h, msg, len(msg), 0, 2**32 - 1, T, buf.ctypes.data_as(RECP),
                                    2**23, ctypes.byref(total))
        assert rc == _lib.HM_OK and total.value <= 2**23, (rc, total.value)
        n = int(total.value)
        recs = buf[:n].copy()
        assert gpu_verify(c, msg, recs, T) == 0      # warm: the kernel, the chunk buffer
        cpu_rounds = max(3, rounds // 2)
        res = {"gpu": [], "cpu16": [], "cpu1": []}
        stats = {"kernel_ms": [], "copy_ms": []}
        for i in range(rounds):
            bad, t = timed(lambda: gpu_verify(c, msg, recs, T))
            assert bad == 0
            res["gpu"].append(t)
            st = c.verify_stats()
            for k in stats:
                stats[k].append(st[k])
            if i < cpu_rounds:
                bad, t = timed(lambda: cpu_verify(msg, recs, T, 16))
                assert bad == 0
                res["cpu16"].append(t)
                bad, t = timed(lambda: cpu_verify(msg, recs, T, 1))
                assert bad == 0
                res["cpu1"].append(t)
        emit({"part": "a", "msg": name, "records": n, "target": T, "verify": summary(res["gpu"], n),
              "kernel_median_ms": med(stats["kernel_ms"]), "copy_median_ms": med(stats["copy_ms"]),
              "launches": st["launches"],
              "bytes_in": 16 * n,
              "copy_GBs": round(16 * n / statistics.median(stats["copy_ms"]) / 1e6, 3)})
        emit({"part": "b", "msg": name, "records": n, "verify_cpu_16": summary(res["cpu16"], n),
              "verify_cpu_1": summary(res["cpu1"], n),
              "gpu_over_cpu16": round(statistics.median(res["cpu16"]) /
                                      statistics.median(res["gpu"]), 3)})
        # (c) divergent against uniform
        mixed = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        ten = rng.integers(10**9, 10**10, size=n, dtype=np.uint64)
        out = np.empty(n, dtype=np.uint64)
        gpu_hash_many(c, msg, mixed, out)            # warm
        res = {"mixed": [], "ten_digits": []}
        stats = {k: {"kernel_ms": [], "copy_ms": []} for k in res}
        for _ in range(rounds):
            for k, arr in (("mixed", mixed), ("ten_digits", ten)):
                _, t = timed(lambda: gpu_hash_many(c, msg, arr, out))
                res[k].append(t)
                st = c.verify_stats()
                for f in stats[k]:
                    stats[k][f].append(st[f])
        for i in (0, n // 2, n - 1):                 # the last round's output: ten digits
            assert int(out[i]) == _lib.host_hash(msg, int(ten[i]))
        row = {"part": "c", "msg": name, "nonces": n}
        for k in res:
            row[k] = summary(res[k], n)
            row[k]["kernel_median_ms"] = med(stats[k]["kernel_ms"])
            row[k]["copy_median_ms"] = med(stats[k]["copy_ms"])
        row["digit_counts_mixed"] = sorted({len(str(int(x))) for x in mixed[:4096]})
        emit(row)
        # (d) the crossover against 16 host threads
        for k in (10, 14, 18):
            part = recs[:2**k].copy()
            res = {"gpu": [], "cpu16": []}
            kms = []
            gpu_verify(c, msg, part, T)
            for _ in range(rounds):
                bad, t = timed(lambda: gpu_verify(c, msg, part, T))
                res["gpu"].append(t)
                kms.append(c.verify_stats()["kernel_ms"])
                bad2, t = timed(lambda: cpu_verify(msg, part, T, 16))
                res["cpu16"].append(t)
                assert bad == bad2 == 0
            emit({"part": "d", "msg": name, "records": 2**k, "verify": summary(res["gpu"], 2**k),
                  "kernel_median_ms": med(kms), "verify_cpu_16": summary(res["cpu16"], 2**k),
                  "gpu_over_cpu16": round(statistics.median(res["cpu16"]) /
                                          statistics.median(res["gpu"]), 3)})
    c.close()
    sink.close()


if __name__ == "__main__":
    main()

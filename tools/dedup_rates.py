"""Rates of the generic kernels (forced) and the list kernel of ONE built tree
(dev tool, GPU box): the A/B of a change to the device code these kernels
share (sha_device.hpp hash_nonce, scan_tasks.hpp).

usage: python tools/dedup_rates.py [TREE [LABEL [ROUNDS]]] >> rates.jsonl

TREE is the root of a built checkout (default: this one); its package and
library are the ones measured.  For an A/B build the other commit in a second
checkout and run the tool on the two trees in turn, several times, in one
session.  Per message (bradfitz, BASELINE configs[2]'s 120-B message):
hm_scan, hm_scan_checked, hm_find (target 1: no hit), hm_collect as a count
and into a buffer over [0, 2^26) with HM_OPT_FORCE_GENERIC; then hm_hash_many
and hm_verify (no bad record; every 7th bad) of 2^10, 2^14 and 2^18 records,
10-digit nonces (the uniform path) and random 64-bit ones (the divergent).
Every answer is checked against the first round's.  One JSON line per
measurement: wall ms around the C call and the library's own HIP-event
kernel ms, median / min / max over ROUNDS (default 7).
"""
import json
import os
import statistics
import sys
import time

tree = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label = sys.argv[2] if len(sys.argv) > 2 else "tree"
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
sys.path.insert(0, tree)
import numpy as np  # noqa: E402
import bench  # noqa: E402
from distributed_bitcoinminer_amd import _lib  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def summ(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
            "max": round(max(xs), 4)}


def emit(row):
    row["label"] = label
    print(json.dumps(row), flush=True)


c = _lib.Context([0])
emit({"tool": "tools/dedup_rates.py", "rounds": rounds, "build_id": _lib.build_id(),
      "code_object": _lib.code_object_sha16()})

# ---- generic kernels: forced, [0, 2^26) (digit counts 1..8), two messages
c.set_option(_lib.HM_OPT_FORCE_GENERIC, 1)
lo, hi = 0, 2**26 - 1
n = hi - lo + 1
T = 2**64 // 2**10
for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
    plan = _lib.debug_plan(msg, lo, hi, True)
    kinds = sorted({str(s.get("kind")) for s in plan})
    ref = c.scan(msg, lo, hi)
    assert c.find(msg, lo, hi, 1) is None or ref[0] < 1
    cnt = c.count(msg, lo, hi, T)
    tot, recs = c.collect(msg, lo, hi, T, 2**17)
    assert tot == cnt and recs is not None and len(recs) == cnt, (tot, cnt)
    res = {k: {"wall": [], "kernel": []} for k in ("scan", "scan_checked", "find", "count",
                                                    "collect")}
    for _ in range(rounds):
        got, t = timed(lambda: c.scan(msg, lo, hi))
        assert got == ref
        res["scan"]["wall"].append(t)
        res["scan"]["kernel"].append(c.stats()["kernel_ms"])
        got, t = timed(lambda: c.scan_checked(msg, lo, hi))
        assert got[0] == ref and got[2] == n, got
        res["scan_checked"]["wall"].append(t)
        res["scan_checked"]["kernel"].append(c.stats()["kernel_ms"])
        got, t = timed(lambda: c.find(msg, lo, hi, 1))
        res["find"]["wall"].append(t)
        res["find"]["kernel"].append(c.find_stats()["kernel_ms"])
        got, t = timed(lambda: c.count(msg, lo, hi, T))
        assert got == cnt
        res["count"]["wall"].append(t)
        res["count"]["kernel"].append(c.collect_stats()["kernel_ms"])
        got, t = timed(lambda: c.collect(msg, lo, hi, T, 2**17))
        assert got[0] == cnt
        res["collect"]["wall"].append(t)
        res["collect"]["kernel"].append(c.collect_stats()["kernel_ms"])
    for k, v in res.items():
        emit({"part": "generic", "call": k, "msg": name, "lo": lo, "hi": hi, "plan_kinds": kinds,
              "answer": list(ref), "count": cnt, "wall_ms": summ(v["wall"]),
              "kernel_ms": summ(v["kernel"]),
              "GHs_kernel": round(n / statistics.median(v["kernel"]) / 1e6, 3)})
c.set_option(_lib.HM_OPT_FORCE_GENERIC, 0)

# ---- list kernel: the sizes of profiles/verify/verify_rate.jsonl part d
rng = np.random.default_rng(1)
for name, msg in (("bradfitz", b"bradfitz"), ("long120", bench.long120())):
    for nrec in (1024, 16384, 262144):
        mixed = rng.integers(0, 2**64, size=nrec, dtype=np.uint64)
        ten = rng.integers(10**9, 10**10, size=nrec, dtype=np.uint64)
        for kind, nonces in (("uniform10", ten), ("mixed", mixed)):
            hashes = c.hash_many(msg, nonces)
            recs = np.stack([hashes, nonces], axis=1)
            recs_bad = recs.copy()
            recs_bad[::7, 0] ^= np.uint64(1)
            nbad = len(recs_bad[::7])
            r = {k: {"wall": [], "kernel": []} for k in ("hash_many", "verify_ok", "verify_bad")}
            for _ in range(rounds):
                got, t = timed(lambda: c.hash_many(msg, nonces))
                assert (got == hashes).all()
                r["hash_many"]["wall"].append(t)
                r["hash_many"]["kernel"].append(c.verify_stats()["kernel_ms"])
                got, t = timed(lambda: c.verify(msg, recs, 2**64 - 1, 2**20))
                assert got[0] == 0, got[0]
                r["verify_ok"]["wall"].append(t)
                r["verify_ok"]["kernel"].append(c.verify_stats()["kernel_ms"])
                got, t = timed(lambda: c.verify(msg, recs_bad, 2**64 - 1, 2**20))
                assert got[0] == nbad and len(got[1]) == nbad, (got[0], nbad)
                r["verify_bad"]["wall"].append(t)
                r["verify_bad"]["kernel"].append(c.verify_stats()["kernel_ms"])
            for k, v in r.items():
                emit({"part": "list", "call": k, "msg": name, "records": nrec, "digits": kind,
                      "wall_ms": summ(v["wall"]), "kernel_ms": summ(v["kernel"])})
c.close()

"""Concurrency of the C ABI (include/hipminer.h "Threading"): calls on one
context are serialised by its mutex and re-bind the device on every call, so
a Go miner may call from any OS thread; separate contexts on one GPU run
concurrently.  Python threads reach the ABI through ctypes, which releases
the GIL for the foreign call, so the calls really overlap.  Every answer must
equal the CPU oracle's (miner.go:46-59 over hash.go:13-17)."""
import random
import threading

import pytest

from distributed_bitcoinminer_amd import _lib

pytestmark = pytest.mark.gpu


def _requests(seed, n):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        L = rng.randrange(0, 130)
        m = bytes(rng.randrange(256) for _ in range(L))
        lo = max(0, 10 ** rng.randrange(1, 20) - rng.randrange(0, 50_000))
        out.append((m, lo, lo + rng.randrange(0, 400_000)))
    return out


def _run_threads(fns):
    errs = []

    def wrap(f):
        try:
            f()
        except BaseException as e:  # noqa: BLE001 -- reported below
            errs.append(e)

    ts = [threading.Thread(target=wrap, args=(f,)) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=240)
    assert not any(t.is_alive() for t in ts), "a scan thread hung"
    if errs:
        raise errs[0]


def test_one_context_many_threads(ctx, oracle_mod):
    """8 threads share one context: scans, checked scans, batches and stats
    interleave; each result is the oracle's."""
    reqs = [_requests(100 + i, 12) for i in range(8)]
    exp = [[oracle_mod.c_scan_sum(m, lo, hi) for m, lo, hi in r] for r in reqs]

    def worker(i):
        def f():
            for j, (m, lo, hi) in enumerate(reqs[i]):
                if (i + j) % 3 == 0:
                    assert ctx.scan_checked(m, lo, hi) == exp[i][j], (i, j)
                elif (i + j) % 3 == 1:
                    assert ctx.scan(m, lo, hi) == exp[i][j][0], (i, j)
                else:
                    assert ctx.scan_many([(m, lo, hi)] * 2) == [exp[i][j][0]] * 2, (i, j)
                st = ctx.stats()
                assert st["ndev"] == 1 and st["wall_ms"] > 0
        return f

    _run_threads([worker(i) for i in range(8)])


def test_finds_interleave_with_scans(ctx, oracle_mod):
    """8 threads share one context and interleave hm_find with hm_scan and
    hm_scan_checked: find resets the device's timing events and shares the
    tile records, the queue counter and stream 0 with the scans, all under the
    context's mutex.  Each find equals the oracle's first hit, each scan the
    oracle's; afterwards the scan stats still describe a scan and the find
    stats a find."""
    reqs = [_requests(300 + i, 9) for i in range(8)]
    exp = [[oracle_mod.c_scan_sum(m, lo, hi) for m, lo, hi in r] for r in reqs]

    def target(i, j):
        best = exp[i][j][0][0]
        return (2**64 // 10**3, best + 1, 2**64 // 10**5, best)[(i + j // 3) % 4]

    want = [[oracle_mod.c_find(m, lo, hi, target(i, j)) if (i + j) % 3 == 0 else None
             for j, (m, lo, hi) in enumerate(r)] for i, r in enumerate(reqs)]
    finds = [(i, j) for i in range(8) for j in range(9) if (i + j) % 3 == 0]
    assert sum(want[i][j] is None for i, j in finds) >= 4       # misses: full searches
    assert sum(want[i][j] is not None for i, j in finds) >= 8

    def worker(i):
        def f():
            for j, (m, lo, hi) in enumerate(reqs[i]):
                if (i + j) % 3 == 0:
                    assert ctx.find(m, lo, hi, target(i, j)) == want[i][j], (i, j)
                    fs = ctx.find_stats()
                    assert fs["ndev"] == 1 and 0 < fs["tasks_run"] <= fs["tasks_total"], fs
                elif (i + j) % 3 == 1:
                    assert ctx.scan(m, lo, hi) == exp[i][j][0], (i, j)
                else:
                    assert ctx.scan_checked(m, lo, hi) == exp[i][j], (i, j)
                st = ctx.stats()
                assert st["ndev"] == 1 and st["wall_ms"] > 0
        return f

    _run_threads([worker(i) for i in range(8)])
    # the two records are still apart: the last scan's and the last find's
    scans = {hi - lo + 1 for i in range(8) for j, (_, lo, hi) in enumerate(reqs[i])
             if (i + j) % 3 != 0}
    st, fs = ctx.stats(), ctx.find_stats()
    assert st["nonces"] in scans and st["launches"] >= 1 and st["kernel_ms"] > 0, st
    assert fs["found"] in (0, 1) and fs["launches"] >= 1 and fs["kernel_ms"] > 0, fs
    assert 0 < fs["nonces_enqueued"] <= max(hi - lo + 1 for r in reqs for _, lo, hi in r), fs
    assert fs["tasks_run"] <= fs["tasks_total"], fs
    m, lo, hi = reqs[0][1]
    assert ctx.scan(m, lo, hi) == exp[0][1][0]
    i, j = finds[-1]
    m2, lo2, hi2 = reqs[i][j]
    assert ctx.find(m2, lo2, hi2, target(i, j)) == want[i][j]
    assert ctx.stats()["nonces"] == hi - lo + 1
    assert ctx.find_stats()["found"] == (want[i][j] is not None)


def test_contexts_per_thread(oracle_mod):
    """4 threads, one context each on GPU 0: their kernels run concurrently on
    the device; a 2^28-nonce scan per thread checks coverage under overlap."""
    big = [(b"bradfitz", 3_000_000_000 + k * (1 << 28), 3_000_000_000 + (k + 1) * (1 << 28) - 1)
           for k in range(4)]
    small = [_requests(200 + k, 6) for k in range(4)]
    exp_small = [[oracle_mod.c_scan(m, lo, hi) for m, lo, hi in r] for r in small]
    results = [None] * 4

    def worker(k):
        def f():
            with _lib.Context([0]) as c:
                m, lo, hi = big[k]
                results[k] = c.scan_checked(m, lo, hi)
                for j, (m2, lo2, hi2) in enumerate(small[k]):
                    assert c.scan(m2, lo2, hi2) == exp_small[k][j], (k, j)
        return f

    _run_threads([worker(k) for k in range(4)])
    with _lib.Context([0]) as c:
        for k in range(4):
            m, lo, hi = big[k]
            assert results[k][2] == hi - lo + 1
            assert results[k] == c.scan_checked(m, lo, hi), k  # the same triple alone

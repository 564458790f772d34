"""hm_verify_many (ABI 1.14) on the GPU: the record lists of many messages in
one launch, against expectations built on the CPU from the C oracle's c_hash
(tests/test_verify_many_host.py has the builders) and against ctx.verify
request by request.

1. the message changes between adjacent waves: 131 requests, one per message
   length 0..130, 40 shuffled digit-edge nonces each -- every job a partial
   wave of mixed digit counts whose neighbours have another r and nb -- honest,
   then a seeded third corrupted; one launch and one copy for the batch;
2. job boundaries: n = 0, 1, 63, 64, 65, 128, 129, every record bad, then only
   each request's last record good, guard words around the refs;
3. the wave-uniform path: one digit count per request (10 and 20);
4. the slot-rank rule across jobs;
5. pieces, launches and devices: HM_OPT_VERIFY_CHUNK x HM_OPT_VERIFY_JOBS on
   contexts naming device 0 once, twice and three times, `launches` as the
   packing rule predicts;
6. one message at two targets, and the same request twice;
7. beside the other calls on one context;
8. a deadline that does not expire;
9. the round trip with hm_collect."""
import ctypes
import random

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_verify_host import MAXU64, SENTINEL, corruption_set, log_uniform_nonce, oracle_hashes
from tests.test_verify_many_host import (corrupt_third, edge_requests, expected, many_raw)

M44 = bytes(0x41 + i % 26 for i in range(44))   # r = 45: two tail blocks from 11 digits on
MSGS = [b"bradfitz", M44, b"", bytes(range(1, 121)), b"thom yorke", b"x" * 63, b"y" * 64]


def ints(a):
    return [int(x) for x in a]


def gpu_many(c):
    lib = _lib.load()
    return lambda arr, n, per, refs, cap, bad: lib.hm_verify_many(c._h, arr, n, per, refs, cap, bad)


def honest_request(oracle_mod, m, nonces):
    """(m, records with the oracle's hashes, a target just above the largest)."""
    hs = oracle_hashes(oracle_mod, m, nonces)
    return m, np.array(list(zip(hs, nonces)), dtype=np.uint64).reshape(-1, 2), max(hs, default=0) + 1


def mixed_request(oracle_mod, m, n, seed):
    rng = random.Random(seed)
    return honest_request(oracle_mod, m, [log_uniform_nonce(rng) for _ in range(n)])


def check_against_verify(c, reqs, got):
    """ctx.verify, request by request, gives the same counts and indices."""
    bad, per, refs = got
    for i, (m, recs, target) in enumerate(reqs):
        b, idx = c.verify(m, recs, target, max(1, len(recs)))
        assert b == per[i], i
        assert [(i, k) for k in ints(idx)] == [r for r in refs if r[0] == i], i


def with_options(c, chunk, jobs, f):
    """f() with HM_OPT_VERIFY_CHUNK = chunk and HM_OPT_VERIFY_JOBS = jobs, restored."""
    c.set_option(_lib.HM_OPT_VERIFY_CHUNK, chunk)
    c.set_option(_lib.HM_OPT_VERIFY_JOBS, jobs)
    try:
        return f()
    finally:
        c.set_option(_lib.HM_OPT_VERIFY_CHUNK, 0)
        c.set_option(_lib.HM_OPT_VERIFY_JOBS, 0)


@pytest.fixture(scope="module")
def multi():
    """Contexts naming device 0 twice and three times (as the collect tests)."""
    with _lib.Context([0, 0]) as c2, _lib.Context([0, 0, 0]) as c3:
        yield {2: c2, 3: c3}


# ---- 1. the message changes between adjacent waves ---------------------------

@pytest.mark.gpu
def test_message_changes_between_adjacent_waves(ctx, oracle_mod):
    honest = edge_requests(oracle_mod)
    assert len(honest) == 131 and all(len(r) == 40 for _, r, _ in honest)
    # neighbours differ in r, and lengths 35..53 put one- and two-block lanes in one wave
    shapes = [{1 if (len(m) + 1) % 64 + len(str(int(n))) + 9 <= 64 else 2 for n in r[:, 1]}
              for m, r, _ in honest]
    assert all(shapes[length] == {1, 2} for length in range(35, 54))
    assert ctx.verify_many(honest, 8) == (0, [0] * 131, [])
    st = ctx.verify_many_stats()
    assert (st["launches"], st["copies"], st["requests"], st["records"], st["tasks"]) == \
        (1, 1, 131, 131 * 40, 131)
    assert (st["bad"], st["overflow"], st["ndev"]) == (0, 0, 1)
    assert st["wall_ms"] > 0 and st["kernel_ms"] > 0 and st["copy_ms"] > 0
    reqs = corrupt_third(honest, seed=41)
    exp = expected(oracle_mod, reqs)
    assert 131 * 40 // 3 - 20 <= exp[0] <= 131 * 40 // 3 and all(c > 0 for c in exp[1])
    got = ctx.verify_many(reqs, exp[0])
    assert got == exp
    st = ctx.verify_many_stats()
    assert (st["launches"], st["copies"], st["bad"], st["overflow"]) == (1, 1, exp[0], 0)
    assert ctx.verify_many(reqs, exp[0] - 1) == (exp[0], exp[1], None)
    assert ctx.verify_many_stats()["overflow"] == 1
    assert ctx.verify_many(reqs, 0) == (exp[0], exp[1], None)
    check_against_verify(ctx, reqs, got)


# ---- 2. job boundaries --------------------------------------------------------

@pytest.mark.gpu
def test_job_boundaries_and_guard_words(ctx, oracle_mod):
    sizes = [0, 1, 63, 64, 65, 128, 129]
    honest = [mixed_request(oracle_mod, MSGS[i], n, seed=50 + i) for i, n in enumerate(sizes)]
    total = sum(sizes)
    # every record bad: a hash bit flipped, judged on the hash alone
    allbad = [(m, r ^ np.array([1, 0], dtype=np.uint64), MAXU64) for m, r, _ in honest]
    every = [(i, k) for i, n in enumerate(sizes) for k in range(n)]
    assert expected(oracle_mod, allbad) == (total, sizes, every)
    for cap in (total, total + 7):
        rc, bad, per, refs, intact = many_raw(gpu_many(ctx), allbad, cap)
        assert (rc, bad, per) == (_lib.HM_OK, total, sizes) and intact
        assert refs[:total] == every
        assert all(x == (SENTINEL, SENTINEL) for x in refs[total:])
    rc, bad, per, refs, intact = many_raw(gpu_many(ctx), allbad, total - 1)
    assert (rc, bad, per) == (_lib.HM_OK, total, sizes) and intact
    assert all(x == (SENTINEL, SENTINEL) for x in refs)
    # only each request's LAST record good: a lane that read over its job's
    # end would find the next job's first (bad) record
    lastgood = []
    for (m, r, _), (_, rb, _) in zip(honest, allbad):
        rb = rb.copy()
        if len(rb):
            rb[-1] = r[-1]
        lastgood.append((m, rb, MAXU64))
    want = [max(0, n - 1) for n in sizes]
    rc, bad, per, refs, intact = many_raw(gpu_many(ctx), lastgood, total)
    assert (rc, bad, per) == (_lib.HM_OK, sum(want), want) and intact
    assert refs[:sum(want)] == [(i, k) for i, n in enumerate(sizes) for k in range(n - 1)]
    assert all(x == (SENTINEL, SENTINEL) for x in refs[sum(want):])
    assert ctx.verify_many_stats()["tasks"] == sum(-(-n // 64) for n in sizes)


# ---- 3. the wave-uniform path -------------------------------------------------

@pytest.mark.gpu
def test_one_digit_count_per_request(ctx, oracle_mod):
    rng = random.Random(60)
    reqs = []
    for m, d in ((b"bradfitz", 10), (M44, 20)):
        lo, hi = 10**(d - 1), min(10**d - 1, MAXU64)
        reqs.append(honest_request(oracle_mod, m, [rng.randrange(lo, hi + 1) for _ in range(257)]))
    assert ctx.verify_many(reqs, 4) == (0, [0, 0], [])
    reqs[0][1][256, 0] ^= np.uint64(1 << 63)
    reqs[1][1][256, 1] -= np.uint64(1)
    assert expected(oracle_mod, reqs) == (2, [1, 1], [(0, 256), (1, 256)])
    assert ctx.verify_many(reqs, 4) == (2, [1, 1], [(0, 256), (1, 256)])


# ---- 4. the slot-rank rule across jobs ----------------------------------------

@pytest.mark.gpu
def test_slot_rank_across_jobs(ctx, oracle_mod):
    reqs = [mixed_request(oracle_mod, MSGS[i], 64, seed=70 + i) for i in range(4)]
    reqs[1][1][:, 0] ^= np.uint64(1)
    assert ctx.verify_many(reqs, 64) == (64, [0, 64, 0, 0], [(1, k) for k in range(64)])
    assert ctx.verify_many(reqs, 63) == (64, [0, 64, 0, 0], None)


# ---- 5. pieces, launches and devices ------------------------------------------

def predicted(sizes, ndev, chunk, jobs):
    """(launches, tasks) by the packing rule of include/hipminer.h: even
    contiguous shares of the flattened records; a share is walked in order, a
    launch closes at `chunk` records or `jobs` jobs, and a request is cut where
    a launch fills."""
    chunk, jobs = chunk or 2**22, jobs or 4096
    total = sum(sizes)
    start = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
    launches = tasks = 0
    for i in range(ndev):
        pos, hi = total * i // ndev, total * (i + 1) // ndev
        nrec = njobs = 0
        while pos < hi:
            r = max(k for k in range(len(sizes)) if start[k] <= pos and sizes[k])
            n = min(start[r + 1], hi) - pos
            n = min(n, chunk - nrec)
            njobs, nrec, pos, tasks = njobs + 1, nrec + n, pos + n, tasks + -(-n // 64)
            if nrec == chunk or njobs == jobs:
                launches, nrec, njobs = launches + 1, 0, 0
        launches += 1 if njobs else 0
    return launches, tasks


@pytest.mark.gpu
def test_pieces_launches_and_devices(ctx, multi, oracle_mod):
    reqs = []
    for seed, m, n in ((21, M44, 1000), (22, b"bradfitz", 300), (23, bytes(range(1, 121)), 77)):
        mm, target, recs, _ = corruption_set(oracle_mod, n, seed=seed, m=m)
        reqs.append((mm, recs, target))
    sizes = [1000, 300, 77]
    exp = expected(oracle_mod, reqs)
    assert len({t for _, _, t in reqs}) == 3 and all(c > n // 2 for c, n in zip(exp[1], sizes))
    assert predicted(sizes, 1, 0, 0) == (1, 16 + 5 + 2)
    assert predicted(sizes, 1, 64, 0)[0] == -(-1377 // 64) and predicted(sizes, 1, 0, 1)[0] == 3
    for c, ndev in ((ctx, 1), (multi[2], 2), (multi[3], 3)):
        for chunk in (64, 128, 0):
            for jobs in (1, 2, 0):
                got = with_options(c, chunk, jobs, lambda: c.verify_many(reqs, exp[0]))
                assert got == exp, (ndev, chunk, jobs)      # the indices stay request-global
                st = c.verify_many_stats()
                assert (st["launches"], st["tasks"]) == predicted(sizes, ndev, chunk, jobs), \
                    (ndev, chunk, jobs, st)
                assert (st["copies"], st["records"], st["bad"], st["ndev"], st["overflow"]) == \
                    (st["launches"], 1377, exp[0], ndev, 0)
                assert with_options(c, chunk, jobs, lambda: c.verify_many(reqs, exp[0] - 1)) == \
                    (exp[0], exp[1], None)
    # the jobs option takes 0..4096, the chunk option what it always took
    for v in (-1, 4097, 2**31):
        with pytest.raises(_lib.HipMinerError):
            ctx.set_option(_lib.HM_OPT_VERIFY_JOBS, v)
    for v in (1, 63, 65, 2**22 + 64, -64):
        with pytest.raises(_lib.HipMinerError):
            ctx.set_option(_lib.HM_OPT_VERIFY_CHUNK, v)
    ctx.set_option(_lib.HM_OPT_VERIFY_JOBS, 4096)
    ctx.set_option(_lib.HM_OPT_VERIFY_JOBS, 0)


# ---- 6. one message at two targets, the same request twice --------------------

@pytest.mark.gpu
def test_repeated_messages_and_requests(ctx, oracle_mod):
    m, target, recs, exp1 = corruption_set(oracle_mod, 400, seed=7)
    reqs = [(m, recs, target), (m, recs, MAXU64), (m, recs, target), (m, recs, 0)]
    exp = expected(oracle_mod, reqs)
    assert exp[1][0] == exp[1][2] == len(exp1) and exp[1][3] == 400 and exp[1][1] < exp[1][0]
    got = ctx.verify_many(reqs, exp[0])
    assert got == exp
    assert [k for i, k in got[2] if i == 2] == exp1
    check_against_verify(ctx, reqs, got)


# ---- 7. beside the other calls ------------------------------------------------

@pytest.mark.gpu
def test_beside_the_other_calls(oracle_mod):
    m, lo, hi, T = b"bradfitz", 0, 10**7, 2**64 // 10**6
    mm, target, recs, exp1 = corruption_set(oracle_mod, 400, seed=7)
    reqs = [(mm, recs, target), mixed_request(oracle_mod, M44, 100, seed=80)]
    exp = expected(oracle_mod, reqs)
    lib = _lib.load()
    stp = ctypes.POINTER(_lib.hm_verify_many_stats)
    with _lib.Context([0]) as c:
        st = _lib.hm_verify_many_stats()
        assert lib.hm_verify_many_stats_sized(c._h, ctypes.byref(st), ctypes.sizeof(st)) == \
            _lib.HM_ERR_INVALID                       # no verify_many yet
        scan0 = c.scan(m, lo, hi)
        find0 = c.find(m, lo, hi, T)
        many0 = c.find_many([(m, lo, hi, T), (M44, 0, 10**5, T)])
        coll0 = c.collect(m, lo, hi, T, 16)
        ver0 = c.verify(mm, recs, target, 400)
        assert (ver0[0], ints(ver0[1])) == (len(exp1), exp1)
        before = (c.stats(), c.find_stats(), c.find_many_stats(), c.collect_stats(),
                  c.verify_stats())
        made = c.streams_made()
        assert made >= 1
        assert c.verify_many(reqs, 400) == exp
        vs = c.verify_many_stats()
        assert (vs["records"], vs["bad"], vs["requests"], vs["launches"], vs["copies"],
                vs["tasks"], vs["ndev"], vs["overflow"]) == (500, exp[0], 2, 1, 1, 7 + 2, 1, 0)
        assert vs["wall_ms"] > 0 and vs["kernel_ms"] > 0 and vs["copy_ms"] > 0
        # the empty batch enqueues nothing and is a call like any other
        assert c.verify_many([], 0) == (0, [], [])
        vs = c.verify_many_stats()
        assert (vs["records"], vs["requests"], vs["launches"], vs["copies"]) == (0, 0, 0, 0)
        assert c.verify_many([(b"x", [], 5)], 0) == (0, [0], [])
        assert c.verify_many_stats()["launches"] == 0
        # no stream made, the other calls' stats as they were
        assert c.streams_made() == made
        assert (c.stats(), c.find_stats(), c.find_many_stats(), c.collect_stats(),
                c.verify_stats()) == before
        # a sized read writes the 1.14 prefix and no more
        buf = (ctypes.c_uint8 * 96)(*([0xA5] * 96))
        assert lib.hm_verify_many_stats_sized(c._h, ctypes.cast(buf, stp), 72) == _lib.HM_OK
        assert all(b == 0xA5 for b in buf[72:]) and any(b != 0xA5 for b in buf[:72])
        assert lib.hm_verify_many_stats_sized(c._h, ctypes.cast(buf, stp), 71) == \
            _lib.HM_ERR_INVALID
        # invalid arguments leave the outputs alone
        rc, bad, per, refs, intact = many_raw(
            lambda arr, n, p, r, cap, b: lib.hm_verify_many(c._h, arr, n, p, r, (1 << 20) + 1, b),
            reqs, 4)
        assert rc == _lib.HM_ERR_INVALID and bad == 777 and intact
        assert per == [SENTINEL] * 2 and refs == [(SENTINEL, SENTINEL)] * 4
        assert c.scan(m, lo, hi) == scan0 and c.find(m, lo, hi, T) == find0
        assert c.find_many([(m, lo, hi, T), (M44, 0, 10**5, T)]) == many0
        assert c.collect(m, lo, hi, T, 16) == coll0


# ---- 8. a deadline that does not expire ---------------------------------------

@pytest.mark.gpu
def test_deadline_that_does_not_expire(ctx, oracle_mod):
    """An expiring deadline is host_wait's, which tests/test_gpu_deadline.py
    covers (and it abandons a context)."""
    mm, target, recs, _ = corruption_set(oracle_mod, 400, seed=7)
    reqs = [(mm, recs, target), mixed_request(oracle_mod, M44, 100, seed=80)]
    exp = expected(oracle_mod, reqs)
    for ms in (60000, -1):
        ctx.set_option(_lib.HM_OPT_DEADLINE_MS, ms)
        try:
            got = ctx.verify_many(reqs, 400)
            # three launches on the one device: the staging-slot wait polls too
            cut = with_options(ctx, 192, 0, lambda: ctx.verify_many(reqs, 400))
            assert ctx.verify_many_stats()["launches"] == 3
        finally:
            ctx.set_option(_lib.HM_OPT_DEADLINE_MS, 0)
        assert got == exp and cut == exp


# ---- 9. the round trip with hm_collect ----------------------------------------

@pytest.mark.gpu
def test_round_trip_with_collect(ctx):
    T, cap = 2**64 // 2**10, 2**13
    msgs = [b"bradfitz", M44, bytes(range(1, 121)), b""]
    reqs = []
    for m in msgs:
        total, recs = ctx.collect(m, 0, 2**22 - 1, T, cap)
        assert 3700 < total < 4500 and len(recs) == total
        reqs.append((m, np.array(recs, dtype=np.uint64), T))
    assert ctx.verify_many(reqs, 8) == (0, [0] * 4, [])
    rng = random.Random(5)
    where = sorted((rng.randrange(4), rng.randrange(3700)) for _ in range(3))
    assert len(set(where)) == 3
    reqs[where[0][0]][1][where[0][1], 0] ^= np.uint64(1)       # a wrong hash
    reqs[where[1][0]][1][where[1][1], 1] += np.uint64(1)       # another nonce
    reqs[where[2][0]][1][where[2][1], 0] = np.uint64(T)        # not below the target
    per = [sum(1 for i, _ in where if i == r) for r in range(4)]
    assert ctx.verify_many(reqs, 8) == (3, per, where)

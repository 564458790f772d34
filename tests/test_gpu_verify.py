"""hm_hash_many and hm_verify (ABI 1.12) on the GPU: Hash(msg, n) at a list of
arbitrary nonces, one per lane with its own digit count and tail layout, and
which (hash, nonce) records of a list are bad, against the committed C
oracle's c_hash per nonce (tests/test_verify_host.py builds the cases).

  a. layout sweep: every message length 0..130 at the 40 digit-edge nonces,
     shuffled (a wave of mixed digit counts: the divergent path);
  b. the wave-uniform path: lists of one digit count;
  c. list shapes around the wave and block sizes, with guard words;
  d. chunks and devices: indices stay global and ascending;
  e. the verify contract, every buffer size, the slot-rank rule;
  f. the round trip with hm_collect;
  g. beside hm_scan, hm_find and hm_collect on one context;
  h. a deadline that does not expire.
"""
import ctypes
import random

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_verify_host import (EDGE_NONCES, LENGTHS, MAXU64, SENTINEL, check_cap_contract,
                                    corruption_set, edge_case, log_uniform_nonce, oracle_hashes)

M44 = bytes(0x41 + i % 26 for i in range(44))   # r = 45: two tail blocks from 11 digits on
U64P = ctypes.POINTER(ctypes.c_uint64)


def ints(a):
    return [int(x) for x in a]


def gpu_call(c):
    lib = _lib.load()
    return lambda m, ln, r, n, T, idx, cap, bad: lib.hm_verify(c._h, m, ln, r, n, T, idx, cap, bad)


def mixed_nonces(n, seed):
    rng = random.Random(seed)
    return [log_uniform_nonce(rng) for _ in range(n)]


def with_chunk(c, chunk, f):
    """f() with HM_OPT_VERIFY_CHUNK = chunk, restored."""
    c.set_option(_lib.HM_OPT_VERIFY_CHUNK, chunk)
    try:
        return f()
    finally:
        c.set_option(_lib.HM_OPT_VERIFY_CHUNK, 0)


@pytest.fixture(scope="module")
def multi():
    """Contexts naming device 0 twice and three times (as the collect tests)."""
    with _lib.Context([0, 0]) as c2, _lib.Context([0, 0, 0]) as c3:
        yield {2: c2, 3: c3}


# ---- a. the layout sweep ----------------------------------------------------

def tail_shape(length, d):
    """(r, nb) of a message length and a digit count, from the formulas."""
    r = (length + 1) % 64
    return r, 1 if r + d + 9 <= 64 else 2


def test_layout_sweep_covers_the_ground():
    """Host-only: the sweep's case list holds every length that matters."""
    assert callable(_lib.Context.hash_many)          # what test_layout_sweep calls per length
    lengths = list(LENGTHS)
    assert lengths == list(range(131))
    ds = sorted({len(str(n)) for n in EDGE_NONCES})
    assert ds == list(range(1, 21))
    for length in lengths:
        m, ns = edge_case(length)
        assert len(m) == length and sorted(ns) == sorted(EDGE_NONCES)
    # 35..53 (mod 64): r = len + 1, nb flips at d = 55 - r inside 1..20, so one
    # wave holds one-block and two-block lanes
    for base in (0, 64):
        for length in range(base + 35, base + 54):
            assert length in lengths
            r = tail_shape(length, 1)[0]
            assert r == length - base + 1
            flip = 55 - r
            assert 1 <= flip <= 19
            assert {tail_shape(length, d)[1] for d in ds} == {1, 2}
            assert tail_shape(length, flip) == (r, 1) and tail_shape(length, flip + 1) == (r, 2)
    # below 35 every lane has one block, from 55 to 62 every lane has two
    assert all({tail_shape(L, d)[1] for d in ds} == {1} for L in range(0, 35))
    assert all({tail_shape(L, d)[1] for d in ds} == {2} for L in range(55, 63))
    # >= 44: the digits cross the block boundary (r + 20 > 64)
    assert all(L in lengths and tail_shape(L, 20)[0] + 20 > 64 for L in range(44, 63))
    # r = 63, 0, 1
    assert [tail_shape(L, 1)[0] for L in (62, 63, 64)] == [63, 0, 1]
    assert all(L in lengths for L in (62, 63, 64, 127))
    assert tail_shape(127, 20) == (0, 1)


@pytest.mark.gpu
def test_layout_sweep(ctx, oracle_mod):
    for length in LENGTHS:
        m, ns = edge_case(length)
        got = ctx.hash_many(m, ns)
        assert got.dtype == np.uint64 and ints(got) == oracle_hashes(oracle_mod, m, ns), length


# ---- b. the wave-uniform path -----------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("m", [b"bradfitz", M44], ids=["bradfitz", "len44"])
@pytest.mark.parametrize("d", [10, 20])
def test_uniform_digit_count(ctx, oracle_mod, m, d):
    rng = random.Random(d)
    lo, hi = 10**(d - 1), min(10**d - 1, MAXU64)
    for n in (64, 65, 257):
        ns = [lo, hi] + [rng.randrange(lo, hi + 1) for _ in range(n - 2)]
        assert {len(str(x)) for x in ns} == {d}
        assert ints(ctx.hash_many(m, ns)) == oracle_hashes(oracle_mod, m, ns), (d, n)
        # the same as records: all good, then one bad in the last (partial) wave
        recs = np.array(list(zip(oracle_hashes(oracle_mod, m, ns), ns)), dtype=np.uint64)
        assert ctx.verify(m, recs, MAXU64, 4)[0] == 0
        recs[n - 1, 0] ^= np.uint64(1)
        bad, idx = ctx.verify(m, recs, MAXU64, 4)
        assert (bad, ints(idx)) == (1, [n - 1]), (d, n)


# ---- c. list shapes ---------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_list_shapes_and_guard_words(ctx, oracle_mod, n):
    """Lanes past the end of the list neither write nor count: guard words
    around the output stay, and verify counts each bad record once."""
    lib = _lib.load()
    m = M44
    ns = mixed_nonces(n, 100 + n)
    want = oracle_hashes(oracle_mod, m, ns)
    a = np.array(ns, dtype=np.uint64)
    out = np.full(n + 16, SENTINEL, dtype=np.uint64)
    rc = lib.hm_hash_many(ctx._h, m, len(m), a.ctypes.data_as(U64P), n,
                          out[8:].ctypes.data_as(U64P))
    assert rc == _lib.HM_OK
    assert ints(out[8:8 + n]) == want
    assert all(int(x) == SENTINEL for x in out[:8]) and all(int(x) == SENTINEL for x in out[8 + n:])
    assert ints(a) == ns                                  # the caller's list is not altered
    # every record bad, element 0 included: n, not a multiple of 64
    recs = np.array(list(zip(want, ns)), dtype=np.uint64)
    recs[:, 0] ^= np.uint64(1)
    rc, bad, buf = _raw(ctx, m, recs, MAXU64, n)
    assert (rc, bad) == (_lib.HM_OK, n) and buf[:n] == list(range(n))
    assert all(x == SENTINEL for x in buf[n:])


def _raw(c, m, recs, target, cap, pad=8):
    from tests.test_verify_host import verify_raw
    return verify_raw(gpu_call(c), m, recs, target, cap, pad)


# ---- d. chunks and devices --------------------------------------------------

@pytest.mark.gpu
def test_chunks_and_devices(ctx, multi, oracle_mod):
    m, target, recs, exp = corruption_set(oracle_mod, 1000, seed=21, m=M44)
    ns = ints(recs[:, 1])
    hashes = oracle_hashes(oracle_mod, m, ns)
    one = ctx.verify(m, recs, target, 1000)
    assert (one[0], ints(one[1])) == (len(exp), exp)
    assert ctx.verify_stats()["launches"] == 1
    for c, ndev in ((ctx, 1), (multi[2], 2), (multi[3], 3)):
        for chunk in (64, 128, 0):
            bad, idx = with_chunk(c, chunk, lambda: c.verify(m, recs, target, len(exp)))
            assert (bad, ints(idx)) == (len(exp), exp), (ndev, chunk)
            st = c.verify_stats()
            assert (st["records"], st["bad"], st["ndev"], st["overflow"]) == (1000, len(exp), ndev, 0)
            if chunk:
                share = [1000 * (i + 1) // ndev - 1000 * i // ndev for i in range(ndev)]
                assert st["launches"] == sum(-(-s // chunk) for s in share), (ndev, chunk, st)
            else:
                assert st["launches"] == ndev
            got = with_chunk(c, chunk, lambda: c.hash_many(m, ns))
            assert ints(got) == hashes, (ndev, chunk)
            assert with_chunk(c, chunk, lambda: c.verify(m, recs, target, len(exp) - 1)) == \
                (len(exp), None)
            assert c.verify_stats()["overflow"] == 1
    # the option takes multiples of 64 in [64, 2^22] and 0 only
    for v in (1, 63, 65, 100, 2**22 + 64, -64):
        with pytest.raises(_lib.HipMinerError):
            ctx.set_option(_lib.HM_OPT_VERIFY_CHUNK, v)
    ctx.set_option(_lib.HM_OPT_VERIFY_CHUNK, 2**22)
    ctx.set_option(_lib.HM_OPT_VERIFY_CHUNK, 0)


# ---- e. the verify contract -------------------------------------------------

@pytest.mark.gpu
def test_verify_contract(ctx, oracle_mod):
    n = 2000
    m, target, recs, exp = corruption_set(oracle_mod, n, seed=9)
    cpu = _lib.verify_cpu(m, recs, target, n, threads=3)
    assert (cpu[0], ints(cpu[1])) == (len(exp), exp)
    check_cap_contract(gpu_call(ctx), m, recs, target, exp)
    bad, idx = ctx.verify(m, recs, target, _lib.HM_VERIFY_CAP_MAX)
    assert (bad, ints(idx)) == (len(exp), exp)
    # every record bad, fitting exactly and one short
    bad, idx = ctx.verify(m, recs, 0, n)
    assert bad == n and ints(idx) == list(range(n))
    rc, bad, buf = _raw(ctx, m, recs, 0, n - 1)
    assert (rc, bad) == (_lib.HM_OK, n) and all(x == SENTINEL for x in buf)
    # no record bad
    honest = [i for i in range(n) if int(recs[i, 0]) == oracle_mod.c_hash(m, int(recs[i, 1]))]
    good = recs[honest]
    rc, bad, buf = _raw(ctx, m, good, int(good[:, 0].max()) + 1, 16)
    assert (rc, bad) == (_lib.HM_OK, 0) and all(x == SENTINEL for x in buf)
    # target = UINT64_MAX: the hash alone
    bad, idx = ctx.verify(m, recs, MAXU64, n)
    assert ints(idx) == [i for i in range(n) if i not in set(honest)]
    # every lane of one wave bad, its neighbours good: the slot-rank rule
    wave = good[:256].copy()
    wave[64:128, 0] ^= np.uint64(1)
    bad, idx = ctx.verify(m, wave, MAXU64, 64)
    assert (bad, ints(idx)) == (64, list(range(64, 128)))
    assert ctx.verify(m, wave, MAXU64, 63) == (64, None)
    # n = 0, and the invalid arguments, leave the outputs alone
    lib = _lib.load()
    idxb = (ctypes.c_uint64 * 2)(SENTINEL, SENTINEL)
    badc = ctypes.c_uint64(777)
    bp = ctypes.byref(badc)
    rp = good.ctypes.data_as(ctypes.POINTER(_lib.hm_result))
    assert lib.hm_verify(ctx._h, m, len(m), None, 0, MAXU64, idxb, 2, bp) == _lib.HM_OK
    assert badc.value == 0 and idxb[0] == SENTINEL
    assert ctx.verify_stats()["records"] == 0 and ctx.verify_stats()["launches"] == 0
    assert ctx.hash_many(m, []).size == 0
    badc.value = 777
    inv = [lib.hm_verify(ctx._h, m, len(m), None, 1, MAXU64, idxb, 2, bp),
           lib.hm_verify(ctx._h, m, len(m), rp, 1, MAXU64, idxb, (1 << 20) + 1, bp),
           lib.hm_verify(ctx._h, m, len(m), rp, 1, MAXU64, None, 2, bp),
           lib.hm_verify(ctx._h, m, len(m), rp, 1, MAXU64, idxb, 2, None),
           lib.hm_verify(ctx._h, None, 3, rp, 1, MAXU64, idxb, 2, bp),
           lib.hm_hash_many(ctx._h, m, len(m), None, 1, idxb),
           lib.hm_hash_many(ctx._h, m, len(m), idxb, 1, None)]
    assert inv == [_lib.HM_ERR_INVALID] * len(inv)
    assert badc.value == 777 and idxb[0] == SENTINEL and idxb[1] == SENTINEL
    # the empty message passed as NULL
    h7 = oracle_mod.c_hash(b"", 7)
    one = (_lib.hm_result * 1)()
    one[0].hash, one[0].nonce = h7, 7
    assert lib.hm_verify(ctx._h, None, 0, one, 1, h7 + 1, None, 0, bp) == _lib.HM_OK
    assert badc.value == 0
    assert lib.hm_verify(ctx._h, None, 0, one, 1, h7, None, 0, bp) == _lib.HM_OK  # strict '<'
    assert badc.value == 1


# ---- f. the round trip with hm_collect --------------------------------------

@pytest.mark.gpu
def test_round_trip_with_collect(ctx):
    m, T, cap = b"bradfitz", 2**64 // 2**12, 2**14
    total, recs = ctx.collect(m, 0, 2**24 - 1, T, cap)
    assert 3500 < total < 4700 and len(recs) == total
    r = np.array(recs, dtype=np.uint64)
    assert ctx.verify(m, r, T, 8)[0] == 0
    assert ints(ctx.hash_many(m, r[:, 1])) == [h for h, _ in recs]
    where = sorted(random.Random(5).sample(range(total), 3))
    r[where[0], 0] ^= np.uint64(1)           # a wrong hash
    r[where[1], 1] += np.uint64(1)           # another nonce
    r[where[2], 0] = np.uint64(T)            # not below the target
    bad, idx = ctx.verify(m, r, T, 8)
    assert (bad, ints(idx)) == (3, where)


# ---- g. beside the other calls ----------------------------------------------

@pytest.mark.gpu
def test_beside_the_other_calls(oracle_mod):
    m, lo, hi, T = b"bradfitz", 0, 10**7, 2**64 // 10**6
    _, target, recs, exp = corruption_set(oracle_mod, 400, seed=7)
    lib = _lib.load()
    with _lib.Context([0]) as c:
        st = _lib.hm_verify_stats()
        assert lib.hm_verify_stats_sized(c._h, ctypes.byref(st), ctypes.sizeof(st)) == \
            _lib.HM_ERR_INVALID                       # no list call yet
        scan0 = c.scan(m, lo, hi)
        find0 = c.find(m, lo, hi, T)
        coll0 = c.collect(m, lo, hi, T, 16)
        assert find0 == (7182149750005, 2351907) == coll0[1][0]
        s0, f0, c0 = c.stats(), c.find_stats(), c.collect_stats()
        assert c.streams_made() >= 1
        made = c.streams_made()
        bad, idx = c.verify(m, recs, target, 400)
        assert (bad, ints(idx)) == (len(exp), exp)
        vs = c.verify_stats()
        assert (vs["records"], vs["bad"], vs["ndev"], vs["overflow"]) == (400, len(exp), 1, 0)
        assert vs["launches"] >= 1 and vs["wall_ms"] > 0 and vs["kernel_ms"] > 0 and vs["copy_ms"] > 0
        got = c.hash_many(m, recs[:, 1])
        assert ints(got) == oracle_hashes(oracle_mod, m, ints(recs[:, 1]))
        vs = c.verify_stats()
        assert (vs["records"], vs["bad"], vs["launches"]) == (400, 0, 1)
        # the list calls made no stream and left the other calls' stats alone
        assert c.streams_made() == made
        assert (c.stats(), c.find_stats(), c.collect_stats()) == (s0, f0, c0)
        # a sized read writes the 1.12 prefix and no more
        buf = (ctypes.c_uint8 * 80)(*([0xA5] * 80))
        assert lib.hm_verify_stats_sized(c._h, ctypes.cast(buf, ctypes.POINTER(_lib.hm_verify_stats)),
                                         56) == _lib.HM_OK
        assert all(b == 0xA5 for b in buf[56:])
        assert lib.hm_verify_stats_sized(c._h, ctypes.cast(buf, ctypes.POINTER(_lib.hm_verify_stats)),
                                         55) == _lib.HM_ERR_INVALID
        assert c.scan(m, lo, hi) == scan0 and c.find(m, lo, hi, T) == find0
        assert c.collect(m, lo, hi, T, 16) == coll0


# ---- h. a deadline that does not expire -------------------------------------

@pytest.mark.gpu
def test_deadline_that_does_not_expire(ctx, oracle_mod):
    """An expiring deadline is host_wait's, which tests/test_gpu_deadline.py
    and the collect tests cover (and it abandons a context)."""
    m, target, recs, exp = corruption_set(oracle_mod, 400, seed=7)
    for ms in (60000, -1):
        ctx.set_option(_lib.HM_OPT_DEADLINE_MS, ms)
        try:
            bad, idx = ctx.verify(m, recs, target, 400)
            got = ctx.hash_many(m, recs[:, 1])
        finally:
            ctx.set_option(_lib.HM_OPT_DEADLINE_MS, 0)
        assert (bad, ints(idx)) == (len(exp), exp)
        assert ints(got) == oracle_hashes(oracle_mod, m, ints(recs[:, 1]))

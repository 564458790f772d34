"""hm_collect_many (ABI 1.15) on the GPU: a batch of collects, each fusible
request one launch of the fused collect kernel (fused_collect_kernels.hip), any
other request hm_collect's per-segment path.  Every comparison is exact, and
every case asserts through hm_collect_many_stats which path it took.

  1. known small answers, against the oracle and against hm_collect;
  2. every layout at its segment edges (the case lists of
     tests/test_collect_layouts_host.py), dense: the surplus-lane check;
  3. several segments per launch (the draws of tests/test_gpu_find_many.py);
  4. trailer and chained layouts with a guided tail;
  5. the size-query contract, and an overflow decided in the first chunk;
  6. batch shapes: chunks, "devices", streams, dead requests, the top of u64;
  7. the fused/unfused boundary and the fallback;
  8. the neighbouring calls, their stats and the shared record buffer.

The primary reference is the CPU oracle (oracle_loop / oracle_list, c_hash,
c_scan_sum); hm_collect on the same context is a second witness."""
import ctypes
import random

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_collect_layouts_host as L
from tests.test_collect_host import oracle_loop
from tests.test_collect_many_host import SENTINEL, check_cap_ladder, expected, many_raw
from tests.test_gpu_collect import collect_np, oracle_list
from tests.test_gpu_collect_layouts import edge_hashes, scan_sum, wrapped_sum
from tests.test_gpu_find_many import layout_cases  # noqa: F401  (a fixture)
from tests.test_gpu_find_paths import _chained_case

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
U64P = ctypes.POINTER(ctypes.c_uint64)


def many_np(c, reqs, cap):
    """hm_collect_many into a numpy buffer (no Python tuples: millions of
    records): (total, totals, [per request an (k, 2) uint64 array of (hash,
    nonce)] or None on overflow)."""
    arr, n, keep = _lib.collect_requests(reqs)
    per = np.zeros(max(1, n), dtype=np.uint64)
    buf = np.empty((max(cap, 1), 2), dtype=np.uint64)
    total = ctypes.c_uint64(0)
    rc = _lib.load().hm_collect_many(c._h, arr, n, per.ctypes.data_as(U64P),
                                     buf.ctypes.data_as(ctypes.POINTER(_lib.hm_result))
                                     if cap else None, cap, ctypes.byref(total))
    del keep
    assert rc == _lib.HM_OK, rc
    t, totals = int(total.value), [int(x) for x in per[:n]]
    if t > cap:
        return t, totals, None
    ends = np.cumsum([0] + totals)
    return t, totals, [buf[ends[i]:ends[i + 1]] for i in range(n)]


def gpu_many(c):
    lib = _lib.load()
    return lambda arr, n, per, out, cap, tot: lib.hm_collect_many(c._h, arr, n, per, out, cap, tot)


def live(reqs):
    return sum(lo <= hi and T != 0 for _, lo, hi, T in reqs)


def all_fused(st, reqs):
    n = live(reqs)
    return (st["requests"] == len(reqs) and st["fused"] == st["launches"] == n and
            st["fallback"] == 0)


class options:
    """Options set for a block and put back to their defaults."""
    DEFAULTS = {_lib.HM_OPT_FORCE_GENERIC: 0, _lib.HM_OPT_FUSED: 1, _lib.HM_OPT_FUSED_TAIL: 2,
                _lib.HM_OPT_STREAMS: 4, _lib.HM_OPT_COLLECT_WINDOW: 0,
                _lib.HM_OPT_TABLE_DIGITS: 0}

    def __init__(self, c, opts):
        self.c, self.opts = c, opts

    def __enter__(self):
        for o, v in self.opts.items():
            self.c.set_option(o, v)

    def __exit__(self, *exc):
        for o in self.opts:
            self.c.set_option(o, self.DEFAULTS[o])


def small_requests(seed, n):
    """n requests of at most 3000 nonces near a digit-count change."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        a = max(0, 10**rng.randrange(1, 20) - rng.randrange(1, 2000))
        out.append((b"job %d" % i, a, min(MAX, a + rng.randrange(3000)), 2**64 // 100))
    return out


# ---- 1. known small ---------------------------------------------------------

def test_known_small(ctx, oracle_mod):
    reqs = [(b"bradfitz", 0, 10**5, 2**64 // 10**3), (b"thom yorke", 0, 10**5, 2**64 // 10**3),
            (b"", 0, 10**5, 2**64 // 10**2), (b"x" * 120, 0, 10**5, 2**64 // 10**4),
            (b"bradfitz", 0, 10**5, 2**64 // 10**4)]
    want = [oracle_loop(oracle_mod, m, lo, hi, T, 0) for m, lo, hi, T in reqs]
    assert want[0][0] == (6697378768932333, 203)
    per = [len(w) for w in want]
    assert ctx.collect_many(reqs, sum(per) + 3) == (sum(per), per, want)
    st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["launches"] == len(reqs), st
    assert st["total"] == sum(per) and st["overflow"] == 0 and st["ndev"] == 1, st
    assert st["nonces"] == len(reqs) * (10**5 + 1) and st["tasks"] > 0 and st["kernel_ms"] > 0, st
    for r, w in zip(reqs, want):
        assert ctx.collect(*r, len(w)) == (len(w), w)
    assert ctx.count_many(reqs) == per
    st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["overflow"] == (1 if sum(per) else 0), st


# ---- 2. every layout at segment edges ---------------------------------------

@pytest.mark.parametrize("how", ["fast", "generic"])
@pytest.mark.parametrize("group", range(len(L.EDGE_GROUPS)), ids=L.EDGE_IDS)
def test_segment_edges(ctx, oracle_mod, group, how):
    """Every message length 0..130 x every digit count of the group, the first
    and last (at most) 300 nonces of the digit segment, in ONE call at T =
    2^64 - 1: each request's total is its span, its nonces are exactly lo..hi
    (a surplus lane that hit would repeat one), every hash is the oracle's."""
    cases = L.edge_cases(group)
    reqs = [(m, lo, hi, MAX) for m, _, lo, hi in cases]
    spans = [hi - lo + 1 for _, lo, hi, _ in reqs]
    assert sum(spans) <= 393_000
    with options(ctx, {_lib.HM_OPT_FORCE_GENERIC: 1 if how == "generic" else 0}):
        total, totals, recs = many_np(ctx, reqs, sum(spans))
        st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["nonces"] == sum(spans), st
    assert totals == spans and total == sum(spans)
    for (m, d, lo, hi), got, hs in zip(cases, recs, edge_hashes(oracle_mod, group)):
        tag = f"msg_hex={m.hex()} d={d} lo={lo} hi={hi} {how}"
        want = np.array(range(lo, hi + 1), dtype=np.uint64)
        assert np.array_equal(got[:, 1], want), (tag, got[:4, 1])
        bad = np.flatnonzero(got[:, 0] != hs)
        assert bad.size == 0, (tag, [(lo + int(i), int(got[i, 0]), int(hs[i])) for i in bad[:4]])


# ---- 3. several segments per launch -----------------------------------------

_SPARSE = {}


def sparse_lists(oracle_mod, name, reqs):
    """oracle_list of every request, once per list."""
    if name not in _SPARSE:
        _SPARSE[name] = [oracle_list(oracle_mod, *r) for r in reqs]
    return _SPARSE[name]


def test_layout_draws(ctx, oracle_mod, layout_cases):
    """The 131 draws of tests/test_gpu_find_many.py (message lengths 0..130, at
    most 5 * 10^4 nonces across a digit-count change).  At T = 2^64 - 1: total
    = span, nonces = lo..hi, the wrapped hash sum and the minimum equal the
    oracle's.  At 2^64 / 2^10: the list equals the oracle's."""
    find_reqs, _, kinds = layout_cases
    assert kinds >= {_lib.HM_KIND_TILED, _lib.HM_KIND_CHAINED, _lib.HM_KIND_GENERIC}
    draws = [r[:3] for r in find_reqs[0::3]]
    assert len(draws) == 131
    reqs = [(m, lo, hi, MAX) for m, lo, hi in draws]
    spans = [hi - lo + 1 for _, lo, hi in draws]
    total, totals, recs = many_np(ctx, reqs, sum(spans))
    st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["nonces"] == sum(spans), st
    assert totals == spans
    for (m, lo, hi), got in zip(draws, recs):
        tag = f"msg_hex={m.hex()} lo={lo} hi={hi}"
        best, s, count = scan_sum(oracle_mod, m, lo, hi)
        assert count == hi - lo + 1
        assert np.array_equal(got[:, 1], np.array(range(lo, hi + 1), dtype=np.uint64)), tag
        assert wrapped_sum(got[:, 0]) == s, tag
        k = int(np.argmin(got[:, 0]))
        assert (int(got[k, 0]), lo + k) == tuple(best), tag
    T = 2**64 // 2**10
    reqs = [(m, lo, hi, T) for m, lo, hi in draws]
    want = sparse_lists(oracle_mod, "draws", reqs)
    per = [len(w) for w in want]
    assert ctx.collect_many(reqs, sum(per) + 1) == (sum(per), per, want)
    assert all_fused(ctx.collect_many_stats(), reqs)


# ---- 4. trailer and chained layouts with a guided tail ----------------------

def trailer_requests(T):
    """The lengths and the three ranges of tests/test_gpu_find_many.py::
    test_trailer_and_chained_layouts."""
    rng = random.Random(606)
    reqs = []
    for n in (44, 45, 50, 54, 55, 56, 57, 60, 63, 64, 100, 119, 120, 127):
        m = bytes(rng.randrange(33, 127) for _ in range(n))
        for lo, hi in ((0, 2_000_000), (10**9 - 700_000, 10**9 + 700_000),
                       (10**11 - 300_000, 10**11 + 900_000)):
            reqs.append((m, lo, hi, T))
    return reqs


@pytest.mark.parametrize("tail", [2, 1, 10])
def test_trailer_and_chained_layouts(ctx, oracle_mod, tail):
    sparse = trailer_requests(2**64 // 10**5)
    want = sparse_lists(oracle_mod, "trailer", sparse)
    per = [len(w) for w in want]
    dense = trailer_requests(MAX)
    spans = [hi - lo + 1 for _, lo, hi, _ in dense]
    mid = trailer_requests(2**64 // 64)
    with options(ctx, {_lib.HM_OPT_FUSED_TAIL: tail}):
        assert ctx.collect_many(sparse, sum(per) + 1) == (sum(per), per, want)
        assert all_fused(ctx.collect_many_stats(), sparse)
        assert ctx.count_many(dense) == spans
        st = ctx.collect_many_stats()
        assert all_fused(st, dense) and st["nonces"] == st["total"] == sum(spans), st
        total, totals, recs = many_np(ctx, mid, 1 << 21)
        assert all_fused(ctx.collect_many_stats(), mid)
    # bit for bit what hm_collect writes for each request (a secondary check)
    assert recs is not None and total == sum(totals)
    for (m, lo, hi, T), t, got in zip(mid, totals, recs):
        n, hashes, nonces = collect_np(ctx, m, lo, hi, T, t)
        assert n == t, (m.hex(), lo, hi)
        assert np.array_equal(got[:, 0], hashes) and np.array_equal(got[:, 1], nonces), \
            (m.hex(), lo, hi)


# ---- 5. the contract on the GPU ---------------------------------------------

def test_cap_ladder_with_sentinels(ctx, oracle_mod):
    reqs = small_requests(51, 12)
    reqs.insert(4, (b"empty", 3, 2, MAX))
    reqs.append((b"top of u64", MAX - 500, MAX, 2**64 // 4))
    exp = expected(oracle_mod, reqs)
    check_cap_ladder(gpu_many(ctx), reqs, exp)
    st = ctx.collect_many_stats()   # the ladder's last call: the pure counts
    assert all_fused(st, reqs) and st["overflow"] == 1 and st["total"] == exp[0], st


def test_overflow_decided_in_the_first_chunk(ctx, oracle_mod):
    """130 requests, three chunks; the first request alone holds more records
    than the cap: every total is still exact, and `out` is not written."""
    reqs = small_requests(52, 130)
    reqs[0] = (b"dense", 0, 2999, MAX)
    total, per, _ = expected(oracle_mod, reqs)
    assert per[0] == 3000
    rc, t, totals, got, intact = many_raw(gpu_many(ctx), reqs, 2500)
    assert (rc, t, totals) == (_lib.HM_OK, total, per) and intact
    assert all(x == (SENTINEL, SENTINEL) for x in got)
    st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["overflow"] == 1 and st["total"] == total, st


# ---- 6. batch shapes --------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 64, 65, 130])
def test_chunks(ctx, oracle_mod, n):
    reqs = small_requests(60 + n, n)
    exp = expected(oracle_mod, reqs)
    assert ctx.collect_many(reqs, exp[0] + 2) == exp
    st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["launches"] == n and st["total"] == exp[0], st
    if n == 0:
        assert st["nonces"] == st["tasks"] == 0 and st["kernel_ms"] == 0, st


@pytest.mark.parametrize("ndev", [2, 3])
def test_several_devices(oracle_mod, ndev):
    reqs = small_requests(70, 67) + [(b"dead", 5, 4, MAX)]
    exp = expected(oracle_mod, reqs)
    with _lib.Context([0] * ndev) as c:
        with pytest.raises(_lib.HipMinerError) as ei:
            c.collect_many_stats()
        assert ei.value.rc == _lib.HM_ERR_INVALID
        assert c.collect_many(reqs, exp[0]) == exp
        st = c.collect_many_stats()
        assert st["ndev"] == ndev and all_fused(st, reqs) and st["fused"] == 67, st
        assert c.collect_many(reqs, exp[0] - 1) == (exp[0], exp[1], None)


@pytest.mark.parametrize("streams", [1, 2, 3, 4])
def test_streams(ctx, oracle_mod, streams):
    reqs = small_requests(80, 70)
    exp = expected(oracle_mod, reqs)
    with options(ctx, {_lib.HM_OPT_STREAMS: streams}):
        assert ctx.collect_many(reqs, exp[0]) == exp
        assert all_fused(ctx.collect_many_stats(), reqs)


def test_edges(ctx, oracle_mod):
    h = oracle_mod.c_hash
    reqs = [(b"dead", 5, 4, MAX), (b"no target", 0, 10**5, 0),
            (None, 0, 2000, 2**64 // 100), (b"", 0, 2000, 2**64 // 100),
            (b"x", MAX, MAX, h(b"x", MAX) + 1), (b"x", MAX, MAX, h(b"x", MAX)),
            (b"top", MAX - 150_000, MAX, 2**64 // 1000), (b"x", 0, 0, MAX),
            (b"top", MAX - 150_000, MAX, 2**64 // 1000)]
    exp = expected(oracle_mod, reqs)
    assert exp[1][:2] == [0, 0] and exp[2][2] == exp[2][3] and exp[1][2] > 5
    assert exp[2][4] == [(h(b"x", MAX), MAX)] and exp[2][5] == [] and exp[2][6] == exp[2][8]
    assert ctx.collect_many(reqs, exp[0]) == exp
    st = ctx.collect_many_stats()
    # the two requests that enqueue nothing count in neither
    assert st["fused"] == st["launches"] == len(reqs) - 2 and st["fallback"] == 0, st
    assert st["requests"] == len(reqs), st
    # the last 150,001 nonces of u64, every one of them: nonce 2^64 - 1 is an ordinary record
    total, totals, recs = many_np(ctx, [(b"top", MAX - 150_000, MAX, MAX)], 150_001)
    assert totals == [150_001] and int(recs[0][-1, 1]) == MAX
    assert int(recs[0][-1, 0]) == h(b"top", MAX) and int(recs[0][0, 0]) == h(b"top", MAX - 150_000)


# ---- 7. the boundary and the fallback ---------------------------------------

def test_window_boundary(ctx, oracle_mod):
    """HM_OPT_COLLECT_WINDOW = 1000: requests of 999 and 1000 nonces are fused,
    one of 1001 is not."""
    m, T = b"window edge", 2**64 // 50
    sizes = (1001, 999, 1000, 1001, 1000, 64, 1001)
    reqs = [(m + bytes([i]), 99_500 + i, 99_500 + i + s - 1, T) for i, s in enumerate(sizes)]
    exp = expected(oracle_mod, reqs)
    assert sum(exp[1]) > 50 and min(exp[1][:4]) > 5
    with options(ctx, {_lib.HM_OPT_COLLECT_WINDOW: 1000}):
        assert ctx.collect_many(reqs, exp[0] + 1) == exp
        st = ctx.collect_many_stats()
        assert ctx.count_many(reqs) == exp[1]
        st0 = ctx.collect_many_stats()
    assert st["fallback"] == 3 and st["fused"] == 4 and st["requests"] == 7, st
    assert st["launches"] >= 4 + 2 * 3 and st["overflow"] == 0, st   # 1001 nonces: two segments
    assert (st0["fallback"], st0["fused"], st0["overflow"]) == (3, 4, 1), st0
    for bad in (1, 63, (1 << 27) + 1, -1):
        with pytest.raises(_lib.HipMinerError) as ei:
            ctx.set_option(_lib.HM_OPT_COLLECT_WINDOW, bad)
        assert ei.value.rc == _lib.HM_ERR_INVALID
    # past the default window: 2^27 nonces are fused, 2^27 + 1 are not
    assert ctx.count_many([(b"w", 0, 2**27 - 1, 1), (b"w", 0, 2**27, 1)]) == [0, 0]
    st = ctx.collect_many_stats()
    assert (st["fused"], st["fallback"]) == (1, 1) and st["nonces"] == 2**28 + 1, st


def test_unfusible_request_and_fused_off(ctx, oracle_mod):
    """A chained request of five final-block digits cannot be fused: it takes
    the per-segment path whole, between fused neighbours.  HM_OPT_FUSED = 0:
    the same answers, every live request on that path."""
    m, lo, hi, _ = _chained_case(random.Random(77))
    T = 2**64 // 10**5
    reqs = small_requests(90, 3) + [(m, lo, hi, T)] + small_requests(91, 2) + [(b"dead", 1, 0, T)]
    want = [oracle_list(oracle_mod, *r) if r[1] <= r[2] else [] for r in reqs]
    per = [len(w) for w in want]
    assert per[3] > 20
    exp = (sum(per), per, want)
    assert ctx.collect_many(reqs, sum(per)) == exp
    st = ctx.collect_many_stats()
    assert (st["fused"], st["fallback"]) == (5, 1) and st["launches"] >= 6, st
    assert ctx.collect(m, lo, hi, T, per[3]) == (per[3], want[3])
    with options(ctx, {_lib.HM_OPT_FUSED: 0}):
        assert ctx.collect_many(reqs, sum(per)) == exp
        st = ctx.collect_many_stats()
        assert ctx.collect_many(reqs, sum(per) - 1) == (sum(per), per, None)
        st0 = ctx.collect_many_stats()
    assert (st["fused"], st["fallback"], st["tasks"]) == (0, 6, 0) and st["launches"] >= 6, st
    assert (st0["fused"], st0["fallback"], st0["overflow"]) == (0, 6, 1), st0


# ---- 8. neighbours ----------------------------------------------------------

def test_other_calls_and_their_stats_untouched(ctx, oracle_mod):
    T = 2**64 // 10**4
    scan = ctx.scan(b"thom yorke", 0, 10**6)
    find = ctx.find(b"thom yorke", 0, 10**6, T)
    fmany = ctx.find_many([(b"thom yorke", 0, 10**6, T)])
    coll = ctx.collect(b"thom yorke", 0, 10**5, T, 64)
    ver = ctx.verify(b"thom yorke", coll[1], T, 8)
    vmany = ctx.verify_many([(b"thom yorke", coll[1], T)], 8)

    def others():
        return (ctx.stats(), ctx.find_stats(), ctx.find_many_stats(), ctx.collect_stats(),
                ctx.verify_stats(), ctx.verify_many_stats())
    before = others()
    reqs = [(b"thom yorke", 0, 10**5, T), (b"thom yorke", 0, 10**5 + 500, T)]
    want = [oracle_list(oracle_mod, *r) for r in reqs]
    assert want[0] == coll[1]
    with options(ctx, {_lib.HM_OPT_COLLECT_WINDOW: 10**5 + 1}):   # a fallback too
        got = ctx.collect_many(reqs, 64)
        st = ctx.collect_many_stats()
    assert got == (len(want[0]) + len(want[1]), [len(w) for w in want], want)
    assert (st["fused"], st["fallback"]) == (1, 1), st
    assert others() == before
    # hm_collect after it on the same context: the record buffer is shared
    assert ctx.collect(b"thom yorke", 0, 10**5, T, 64) == coll
    assert ctx.collect_many(reqs, 64) == got
    assert ctx.scan(b"thom yorke", 0, 10**6) == scan
    assert ctx.find(b"thom yorke", 0, 10**6, T) == find
    assert ctx.find_many([(b"thom yorke", 0, 10**6, T)]) == fmany
    assert ver[0] == 0 and vmany[0] == 0


def test_cap_grows_across_calls(oracle_mod):
    """A fresh context: cap 16, then 2^16 (the record and tag buffers are
    replaced by larger ones), hm_collect in between and after."""
    reqs = small_requests(95, 20)
    exp = expected(oracle_mod, reqs)
    dense = [(b"grow", 10**6 - 20_000, 10**6 + 19_999, MAX), (b"grow", 0, 9_999, MAX)]
    with _lib.Context([0]) as c:
        assert exp[0] > 16 and c.collect_many(reqs, 16) == (exp[0], exp[1], None)
        one = (1419516646206828, 9898)   # the minimum of bradfitz over [0, 9999]
        assert c.collect_many([(b"bradfitz", 0, 9999, one[0] + 1)], 16) == (1, [1], [[one]])
        assert c.collect(*reqs[1], 64) == (exp[1][1], exp[2][1])
        total, totals, recs = many_np(c, dense, 1 << 16)
        assert totals == [40_000, 10_000] and all_fused(c.collect_many_stats(), dense)
        assert np.array_equal(recs[0][:, 1], np.arange(10**6 - 20_000, 10**6 + 20_000,
                                                       dtype=np.uint64))
        assert np.array_equal(recs[1][:, 1], np.arange(10_000, dtype=np.uint64))
        n, hashes, _ = collect_np(c, *dense[0], 1 << 16)
        assert n == 40_000 and np.array_equal(hashes, recs[0][:, 0])
        assert c.collect_many(reqs, exp[0]) == exp

"""hm_find_k_many (ABI 1.17) on the GPU: a batch of hm_find_k requests, each
request's window one fused launch that records as hm_find_k does and exits
early (fused_find_k_kernels.hip), the rest of a range through hm_find_k's
per-segment path.  Every answer is compared, request by request, with hm_find_k
(itself pinned against hm_collect by test_gpu_find_k.py), and a subset or all
of each test's requests with the iterated-c_find oracle truncated to k."""
import ctypes
import random

import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_collect_host import oracle_collect
from tests.test_gpu_find import KATS
from tests.test_gpu_find_k import bradfitz_hits
from tests.test_gpu_find_many import layout_cases  # noqa: F401  (the shared draws, a fixture)

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A)


def oracle_first_k(oracle_mod, m, lo, hi, T, k):
    """The k lowest hits of [lo, hi]: c_find from lo, restarted at answer + 1."""
    out, n = [], lo
    while n <= hi and len(out) < k and T:
        got = oracle_mod.c_find(m, n, hi, T, threads=1)
        if got is None:
            break
        out.append(got)
        n = got[1] + 1
    return out


def run(c, reqs):
    """find_k_many over reqs: (answers, stats), every answer equal to hm_find_k's."""
    got = c.find_k_many(reqs)
    st = c.find_k_many_stats()
    assert len(got) == len(reqs)
    for i, r in enumerate(reqs):
        assert got[i] == c.find_k(*r), (i, len(r[0]), r[1:], st)
    assert st["requests"] == len(reqs) and st["found"] == sum(len(g) for g in got), st
    return got, st


@pytest.fixture
def generic(ctx):
    def set_(on):
        ctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 1 if on else 0)
    yield set_
    ctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 0)


# ---- known answers ----------------------------------------------------------

def test_known_answers(ctx, oracle_mod):
    m, lo, hi, T = b"bradfitz", 0, 10**7, 2**64 // 10**5
    want = bradfitz_hits()   # the host's list, shared with test_gpu_find_k.py
    total = len(want)
    assert want[:7] == oracle_first_k(oracle_mod, m, lo, hi, T, 7)
    assert want[0] == (158752571039048, 91989) and total >= 70
    ks = (1, 2, 7, 64, total, total + 5)
    reqs = [(m, lo, hi, T, k) for k in ks]
    got, st = run(ctx, reqs)
    assert got == [want[:k] for k in ks]
    assert st["fused"] == st["launches"] == st["requests"] == len(ks), st
    assert st["fallback"] == 0 and st["overflow"] == 0 and st["ndev"] == 1, st
    assert 0 < st["tasks_run"] <= st["tasks_total"] and st["kernel_ms"] > 0, st
    assert st["records"] >= st["found"] == sum(min(k, total) for k in ks), st


# ---- every layout -----------------------------------------------------------

@pytest.mark.parametrize("force_generic", [0, 1], ids=["fast", "generic"])
def test_every_layout(ctx, oracle_mod, generic, layout_cases, force_generic):  # noqa: F811
    """The 131 draws of test_gpu_find_many.layout_cases (message lengths 0..130,
    at most 5*10^4 nonces across a digit-count change) at 2^64 / 2^12, k in
    (1, 5, total + 3): 393 requests in one call, with and without
    HM_OPT_FORCE_GENERIC, all against the oracle."""
    drawn, _, kinds = layout_cases
    assert kinds >= {_lib.HM_KIND_TILED, _lib.HM_KIND_CHAINED, _lib.HM_KIND_GENERIC}
    T = 2**64 // 2**12
    reqs, want = [], []
    for m, lo, hi, _ in drawn[0::3]:
        full = oracle_collect(oracle_mod, m, lo, hi, T)
        for k in (1, 5, len(full) + 3):
            reqs.append((m, lo, hi, T, k))
            want.append(full[:k])
    assert len(reqs) == 393 and {len(r[0]) for r in reqs} == set(range(131))
    generic(force_generic)
    got, st = run(ctx, reqs)
    bad = [(i, len(reqs[i][0]), reqs[i][1:], got[i], want[i])
           for i in range(len(reqs)) if got[i] != want[i]]
    assert not bad, bad[:3]
    assert st["fused"] == st["launches"] == len(reqs), st
    assert st["fallback"] == 0 and st["overflow"] == 0, st


def test_trailer_and_chained_layouts(ctx, oracle_mod):
    """The lengths and ranges of test_gpu_find_many.test_trailer_and_chained_
    layouts at 2^64 / 10^5, k = 3 and k beyond every total; one length in
    three against the oracle (its first range at k = 3, its second in full)."""
    rng = random.Random(606)
    T = 2**64 // 10**5
    reqs = []
    for L in (44, 45, 50, 54, 55, 56, 57, 60, 63, 64, 100, 119, 120, 127):
        m = bytes(rng.randrange(33, 127) for _ in range(L))
        for lo, hi in ((0, 2_000_000), (10**9 - 700_000, 10**9 + 700_000),
                       (10**11 - 300_000, 10**11 + 900_000)):
            reqs += [(m, lo, hi, T, 3), (m, lo, hi, T, 1000)]
    got, st = run(ctx, reqs)
    assert st["fused"] == st["requests"] == len(reqs) and st["fallback"] == 0, st
    for i in range(0, len(reqs), 18):
        for j in (i, i + 3):
            assert got[j] == oracle_first_k(oracle_mod, *reqs[j]), j


# ---- the early exit inside the launch ---------------------------------------

def test_early_exit_inside_the_launch(ctx):
    """bradfitz over [10^9, 10^9 + 2^27 - 1] at 2^64 / 10^4, k = 64.  The first
    2*10^6 nonces hold 194 hits, the first at offset 5,039 and the 64th at
    offset 666,860 (hashlib), so a first round of about 3*10^3 tasks of 640
    nonces stays far inside the default slice of 4224 records.  tasks_run * 4
    <= tasks_total is the fixed cap of the other early-exit tests, a condition
    and not a measurement."""
    m, lo, T, k = b"bradfitz", 10**9, 2**64 // 10**4, 64
    total, ref = ctx.collect(m, lo, lo + 2 * 10**6, T, 4096)
    assert total == len(ref) == 194
    assert (ref[0][1] - lo, ref[63][1] - lo) == (5_039, 666_860)
    got = ctx.find_k_many([(m, lo, lo + 2**27 - 1, T, k)])
    st = ctx.find_k_many_stats()
    print("early exit:", st)
    assert got == [ref[:k]]
    assert st["launches"] == 1 and st["fused"] == 1 and st["overflow"] == 0, st
    assert st["fallback"] == 0 and st["found"] == k <= st["records"], st
    assert st["nonces_enqueued"] == 2**27 and st["tasks_total"] >= 50_000, ("vacuous", st)
    assert 0 < st["tasks_run"] and st["tasks_run"] * 4 <= st["tasks_total"], st


# ---- the window's end -------------------------------------------------------

def test_window_end(ctx, oracle_mod):
    """HM_OPT_FIND_WINDOW = 1000: the fused launch covers window nonces 0..999,
    the per-segment path the rest.  H is every hit of 120,000 nonces at 2^64 /
    200 from the oracle; with lo = H[j] - w and k = the hits of [lo, H[j]], the
    k-th hit is window nonce w exactly and the earlier ones lie inside the
    window."""
    m, base, T = b"window edge k", 7_000_000, 2**64 // 200
    full = oracle_collect(oracle_mod, m, base, base + 119_999, T)
    hits = [n for _, n in full]
    assert len(hits) >= 400

    def request(j, w):
        lo = hits[j] - w
        assert lo >= base
        k = sum(1 for n in hits if lo <= n <= hits[j])
        return (m, lo, lo + 59_999, T, k), [r for r in full if r[1] >= lo][:k]

    ws = (998, 999, 1000, 1001, 50_000)
    j0 = next(j for j in range(len(hits)) if hits[j] - base > 1001)
    reqs, want = [], []
    for i, w in enumerate(ws):
        j = j0 + 2 * i if w < 50_000 else next(j for j in range(len(hits))
                                                if hits[j] - base > 50_000)
        r, wnt = request(j, w)
        assert r[4] >= 2 and wnt[-1][1] - r[1] == w, (w, r)
        reqs.append(r)
        want.append(wnt)
    # a range that ends exactly at the window with fewer than k hits
    lo = base + 2000
    inside = [r for r in full if lo <= r[1] <= lo + 999]
    assert inside
    reqs.append((m, lo, lo + 999, T, len(inside) + 3))
    want.append(inside)
    ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 1000)
    try:
        got, st = run(ctx, reqs)
    finally:
        ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 0)
    assert got == want
    for g in got:
        assert [n for _, n in g] == sorted(n for _, n in g)
    past = sum(w > 999 for w in ws)
    assert st["fallback"] == past == 3 and st["fused"] == len(reqs) - past == 3, st
    assert st["overflow"] == 0 and st["launches"] >= len(reqs) + past, st


# ---- overflow ---------------------------------------------------------------

def test_forced_overflow(ctx, oracle_mod):
    """HM_OPT_FIND_K_BUF = k: a slice of exactly k records at a hit per 64
    nonces.  The records beyond the first k are lost, so the request goes down
    hm_find_k's own path whole."""
    m, lo, hi, T, k = b"bradfitz", 0, 10**6, 2**64 // 64, 64
    ctx.set_option(_lib.HM_OPT_FIND_K_BUF, k)
    try:
        got = ctx.find_k_many([(m, lo, hi, T, k)])
        st = ctx.find_k_many_stats()
    finally:
        ctx.set_option(_lib.HM_OPT_FIND_K_BUF, 0)
    assert got == [oracle_first_k(oracle_mod, m, lo, hi, T, k)]
    assert st["overflow"] == 1 and st["fallback"] == 1 and st["fused"] == 0, st
    assert st["found"] == k and st["launches"] >= 2, st


def test_natural_overflow_beside_requests_that_fit(ctx, oracle_mod):
    """T = 2^64-1: every nonce hits, one round of tasks overruns the default
    slice.  Its neighbours in the batch, on the same device, keep theirs."""
    m, lo, k = b"bradfitz", 12345, 1000
    dense = (m, lo, 10**9, MAX, k)
    sparse = [(b"bradfitz", 0, 10**6, 2**64 // 10**4, 5), (b"neighbour", 10**6, 2 * 10**6, 2**64 // 10**4, 50)]
    reqs = [sparse[0], dense, sparse[1]]
    got, st = run(ctx, reqs)
    assert got[1] == [(_lib.host_hash(m, n), n) for n in range(lo, lo + k)]
    assert got[0] == oracle_first_k(oracle_mod, *sparse[0])
    assert got[2] == oracle_first_k(oracle_mod, *sparse[1])
    assert st["overflow"] == 1 and st["fallback"] == 1 and st["fused"] == 2, st
    # alone
    got, st = run(ctx, [dense])
    assert len(got[0]) == k and st["overflow"] == 1 == st["fallback"], st


# ---- edges ------------------------------------------------------------------

def test_edges(ctx, oracle_mod):
    h = oracle_mod.c_hash
    reqs = [(b"bradfitz", 5, 4, MAX, 3), (b"bradfitz", 0, 10**5, 0, 3)]
    want = [[], []]
    for n in (0, 9, 10, 10**19, MAX):
        reqs += [(b"x", n, n, h(b"x", n) + 1, 2), (b"x", n, n, h(b"x", n), 2)]
        want += [[(h(b"x", n), n)], []]
    lo = MAX - 150_000
    T = 2**64 // 10**4
    top = oracle_collect(oracle_mod, b"bradfitz", lo, MAX, T)
    assert len(top) >= 5
    reqs += [(b"bradfitz", lo, MAX, T, 3), (b"bradfitz", lo, MAX, T, len(top) + 2),
             (b"", MAX - 9, MAX, MAX, 5), (b"", MAX - 9, MAX, MAX, 12),
             (b"", 0, 10**5, 2**64 // 10**3, 7), (None, 0, 10**5, 2**64 // 10**3, 7)]
    tail = [(h(b"", n), n) for n in range(MAX - 9, MAX + 1)]
    empty = oracle_first_k(oracle_mod, b"", 0, 10**5, 2**64 // 10**3, 7)
    want += [top[:3], top, tail[:5], tail, empty, empty]
    got = ctx.find_k_many(reqs)
    st = ctx.find_k_many_stats()
    assert got == want
    assert got[:-1] == [ctx.find_k(*r) for r in reqs[:-1]]
    # the two requests that enqueue nothing count in neither
    assert st["fused"] == len(reqs) - 2 and st["fallback"] == 0, st
    assert st["launches"] == len(reqs) - 2 and st["requests"] == len(reqs), st
    assert ctx.find_k_many([]) == []
    st = ctx.find_k_many_stats()
    assert st["requests"] == st["launches"] == st["tasks_total"] == st["found"] == 0, st


def test_sixty_four_targets_and_chunk_boundaries(ctx, oracle_mod):
    # one message 64 times, 64 targets
    reqs = [(b"bradfitz", 0, 10**6, 2**64 // (500 * (i + 1)), 1 + i % 9) for i in range(64)]
    got, st = run(ctx, reqs)
    assert got[::8] == [oracle_first_k(oracle_mod, *r) for r in reqs[::8]]
    assert st["fused"] == 64 and st["fallback"] == 0, st
    # one request past a chunk, and past two chunks
    rng = random.Random(65)
    for n in (65, 129):
        reqs = []
        for i in range(n):
            a = rng.randrange(10**rng.randrange(1, 19))
            reqs.append((b"chunk %d" % i, a, a + rng.randrange(3000), 2**64 // 100,
                         rng.randrange(1, 12)))
        got, st = run(ctx, reqs)
        assert got == [oracle_first_k(oracle_mod, *r) for r in reqs], n
        assert st["requests"] == st["fused"] == st["launches"] == n, st


def test_slab_rule_cuts_the_chunk(ctx):
    """k = 2^20 asks for a slice of 2 * 2^20 + 4096 records: eight of them
    exceed the 2^24 records one device's slab may hold, so the chunk is cut
    before the eighth.  No hit (target 1): every request stays fused."""
    big = 1 << 20
    ks = [3, big, big, 1, big, big, big, 7, big, big, big, big, 2]
    assert sum(2 * k + 4096 for k in ks if k == big) > _lib.HM_COLLECT_CAP_MAX
    reqs = [(b"slab %d" % i, 1000 * i, 1000 * i + 999, 1, k) for i, k in enumerate(ks)]
    assert ctx.find_k_many(reqs) == [[] for _ in ks]
    st = ctx.find_k_many_stats()
    assert st["fused"] == st["launches"] == len(ks), st
    assert st["fallback"] == st["overflow"] == st["found"] == st["records"] == 0, st
    assert st["tasks_run"] == st["tasks_total"] > 0, st


def test_nothing_beyond_the_counts_is_touched(ctx):
    m, T = b"bradfitz", 2**64 // 10**4
    reqs = [(m, 0, 10**5, T, 4), (m, 5, 4, MAX, 2), (m, 0, 30_000, T, 50), (m, 0, 10**6, T, 1)]
    want = [ctx.find_k(*r) for r in reqs]
    assert 0 < len(want[2]) < 50 and len(want[0]) == 4
    arr, n, keep = _lib.find_k_requests(reqs)
    total = sum(r[4] for r in reqs)
    out = (_lib.hm_result * (total + 2))()
    for r in out:
        r.hash, r.nonce = SENTINEL
    counts = (ctypes.c_size_t * n)(*([777] * n))
    assert _lib.load().hm_find_k_many(ctx._h, arr, n, out, counts) == _lib.HM_OK
    flat = [(int(r.hash), int(r.nonce)) for r in out]
    off = 0
    for i, (w, r) in enumerate(zip(want, reqs)):
        assert counts[i] == len(w) and flat[off:off + len(w)] == w, i
        assert all(x == SENTINEL for x in flat[off + len(w):off + r[4]]), i
        off += r[4]
    assert flat[total:] == [SENTINEL] * 2
    del keep


# ---- options ----------------------------------------------------------------

def mixed_requests():
    rng = random.Random(117)
    reqs = []
    for i in range(20):
        m = bytes(rng.randrange(256) for _ in range(rng.randrange(131)))
        lo = max(0, 10**rng.randrange(1, 20) - rng.randrange(1, 60_000))
        hi = min(MAX, lo + rng.randrange(120_000))
        reqs.append((m, lo, hi, 2**64 // 10**rng.randrange(2, 5), rng.randrange(1, 30)))
    reqs += [(b"bradfitz", 5, 4, MAX, 2), (b"bradfitz", 0, 10**7, 2**64 // 10**5, 7)]
    return reqs


def test_fused_off_takes_the_per_segment_path(ctx, oracle_mod):
    reqs = mixed_requests()
    want = [oracle_first_k(oracle_mod, *r) for r in reqs]
    assert ctx.find_k_many(reqs) == want
    ctx.set_option(_lib.HM_OPT_FUSED, 0)
    try:
        got = ctx.find_k_many(reqs)
        st = ctx.find_k_many_stats()
    finally:
        ctx.set_option(_lib.HM_OPT_FUSED, 1)
    assert got == want
    live = len(reqs) - 1
    assert st["fused"] == 0 and st["fallback"] == live and st["launches"] >= live, st
    assert st["overflow"] == 0, st


@pytest.mark.parametrize("ndev", [2, 3])
def test_several_devices(ctx, ndev):
    reqs = mixed_requests()
    want = ctx.find_k_many(reqs)
    with _lib.Context([0] * ndev) as c:
        got, st = run(c, reqs)
        assert got == want
        assert st["ndev"] == ndev and st["fused"] == len(reqs) - 1 and st["fallback"] == 0, st


def test_streams(ctx):
    reqs = mixed_requests()
    want = ctx.find_k_many(reqs)
    try:
        for s in (1, 2, 4):
            ctx.set_option(_lib.HM_OPT_STREAMS, s)
            assert ctx.find_k_many(reqs) == want, s
            assert ctx.find_k_many_stats()["fused"] == len(reqs) - 1
    finally:
        ctx.set_option(_lib.HM_OPT_STREAMS, 4)


def test_other_calls_and_their_stats_untouched(ctx):
    with _lib.Context([0]) as c:
        with pytest.raises(_lib.HipMinerError) as ei:
            c.find_k_many_stats()
        assert ei.value.rc == _lib.HM_ERR_INVALID
    m, T = b"thom yorke", 2**64 // 10**4
    find = ctx.find(m, 0, 10**6, T)
    find_k = ctx.find_k(m, 0, 10**6, T, 5)
    coll = ctx.collect(m, 0, 10**5, T, 64)
    many = ctx.find_many([(m, 0, 10**6, T)])
    before = (ctx.find_stats(), ctx.find_k_stats(), ctx.collect_stats(), ctx.find_many_stats())
    ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 64)   # a fallback too
    try:
        assert ctx.find_k_many([(m, 0, 10**6, T, 5), (b"x", 0, 99, 1, 2)]) == [find_k, []]
        assert ctx.find_k_many_stats()["fallback"] == 2
    finally:
        ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 0)
    assert ctx.find_k_many([(m, 0, 10**6, T, 5)]) == [find_k]
    assert (ctx.find_stats(), ctx.find_k_stats(), ctx.collect_stats(),
            ctx.find_many_stats()) == before
    assert ctx.find(m, 0, 10**6, T) == find and ctx.find_k(m, 0, 10**6, T, 5) == find_k
    assert ctx.collect(m, 0, 10**5, T, 64) == coll and ctx.find_many([(m, 0, 10**6, T)]) == many


def test_deadline_applies_to_the_whole_call():
    """A 1-ms deadline on 64 no-hit requests of 2^27 nonces (~0.2 s of kernel):
    HM_ERR_TIMEOUT, outputs untouched, the context abandoned."""
    c = _lib.Context([0])
    assert c.find_k_many([(b"bradfitz", 0, 10**6, KATS[0][0], 1)]) == [[KATS[0][1]]]
    c.set_option(_lib.HM_OPT_DEADLINE_MS, 1)
    n = 64
    reqs = [(b"deadline %d" % i, 0, 2**27 - 1, 1, 2) for i in range(n)]
    arr, n, keep = _lib.find_k_requests(reqs)
    out = (_lib.hm_result * (2 * n))()
    for r in out:
        r.hash, r.nonce = SENTINEL
    counts = (ctypes.c_size_t * n)(*([777] * n))
    lib = _lib.load()
    assert lib.hm_find_k_many(c._h, arr, n, out, counts) == _lib.HM_ERR_TIMEOUT
    assert all((int(r.hash), int(r.nonce)) == SENTINEL for r in out) and list(counts) == [777] * n
    assert lib.hm_find_k_many(c._h, arr, 1, out, counts) == _lib.HM_ERR_TIMEOUT
    with pytest.raises(_lib.HipMinerError) as ei:
        c.find_k_many([(b"x", 0, 9, MAX, 1)])
    assert ei.value.rc == _lib.HM_ERR_TIMEOUT
    del keep
    c.close()  # host memory only: the queued work drains on its own


# ---- a seeded sweep ---------------------------------------------------------

def test_random_requests_vs_oracle(ctx, oracle_mod):
    """200 requests: lengths 0..130, ranges of at most 2*10^5 nonces near digit
    boundaries or anywhere, targets 2^64 / 10^2 .. 2^64 / 10^6, k in 1..50, in
    batches of 1..80."""
    rng = random.Random(2117)
    reqs = []
    for _ in range(200):
        m = bytes(rng.randrange(256) for _ in range(rng.randrange(131)))
        if rng.random() < 0.6:
            lo = max(0, 10**rng.randrange(1, 20) - rng.randrange(1, 100_000))
        else:
            lo = rng.randrange(MAX)
        hi = min(MAX, lo + rng.randrange(200_000))
        reqs.append((m, lo, hi, 2**64 // 10**rng.randrange(2, 7), rng.randrange(1, 51)))
    want = [oracle_first_k(oracle_mod, *r) for r in reqs]
    assert any(len(w) == r[4] for w, r in zip(want, reqs))
    assert any(0 < len(w) < r[4] for w, r in zip(want, reqs)) and any(not w for w in want)
    i = 0
    while i < len(reqs):
        n = rng.randrange(1, 81)
        got = ctx.find_k_many(reqs[i:i + n])
        assert got == want[i:i + n], (i, n, ctx.find_k_many_stats())
        i += n

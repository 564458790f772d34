"""hm_find_many (ABI 1.13) on the GPU: a batch of finds, each request's window
one fused launch with hm_find's early exit (fused_find_kernels.hip), the rest of
a range through hm_find's per-segment path.  Every answer is compared exactly
with the C oracle's first-hit search (oracle.c_find) or its min-hash scan
(oracle.c_scan): strictness at target = min, the argmin at min + 1 (every task
must run), early hits, the window's end, the top of u64, batching across chunks
of 64 and across "devices", and the work accounting."""
import ctypes
import random

import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_gpu_find import KATS

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1


def _expect(oracle_mod, reqs):
    return [oracle_mod.c_find(m, lo, hi, T) for m, lo, hi, T in reqs]


@pytest.fixture
def generic(ctx):
    def set_(on):
        ctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 1 if on else 0)
    yield set_
    ctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 0)


@pytest.fixture(scope="module")
def layout_cases(oracle_mod):
    """The draws of test_gpu_fused.py::test_every_layout_checked_vs_oracle
    (message lengths 0..130, a range of at most 5*10^4 nonces across a
    digit-count change), three targets each: (requests, expected, kinds)."""
    rng = random.Random(505)
    reqs, want, kinds = [], [], set()
    for L in range(131):
        m = bytes(rng.randrange(32, 127) for _ in range(L))
        d = rng.randrange(2, 20)
        lo = max(0, 10**d - rng.randrange(1, 25_000))
        hi = min(MAX, 10**d + rng.randrange(0, 25_000))
        mn = oracle_mod.c_scan(m, lo, hi)
        kinds |= {s["kind"] for s in _lib.debug_plan(m, lo, hi)}
        early = 2**64 // 2**12
        reqs += [(m, lo, hi, mn[0]), (m, lo, hi, mn[0] + 1), (m, lo, hi, early)]
        want += [None, mn, oracle_mod.c_find(m, lo, hi, early)]
    return reqs, want, kinds


def test_known_answers(ctx):
    reqs = [(b"bradfitz", 0, 10**7, T) for T, _ in KATS]
    got = ctx.find_many(reqs)
    assert got == [want for _, want in KATS]
    st = ctx.find_many_stats()
    assert got == [ctx.find(*r) for r in reqs]
    assert st["requests"] == st["fused"] == st["found"] == len(KATS), st
    assert st["fallback"] == 0 and st["launches"] == len(KATS) and st["ndev"] == 1, st
    assert 0 < st["tasks_run"] <= st["tasks_total"] and st["kernel_ms"] > 0, st


@pytest.mark.parametrize("force_generic", [0, 1], ids=["fast", "generic"])
def test_every_layout(ctx, generic, layout_cases, force_generic):
    """393 requests in one call (seven chunks): target = min gives none, min + 1
    the argmin, 2^64 / 2^12 an early hit; with and without HM_OPT_FORCE_GENERIC."""
    reqs, want, kinds = layout_cases
    assert kinds >= {_lib.HM_KIND_TILED, _lib.HM_KIND_CHAINED, _lib.HM_KIND_GENERIC}
    generic(force_generic)
    got = ctx.find_many(reqs)
    bad = [(i, len(reqs[i][0]), reqs[i][1:], got[i], want[i])
           for i in range(len(reqs)) if got[i] != want[i]]
    assert not bad, bad[:5]
    st = ctx.find_many_stats()
    assert st["requests"] == st["fused"] == st["launches"] == len(reqs), st
    assert st["fallback"] == 0 and st["found"] == sum(w is not None for w in want), st


def test_trailer_and_chained_layouts(ctx, oracle_mod):
    """The lengths and ranges of test_gpu_fused.py::
    test_layouts_with_trailer_and_chained_segments, at min + 1 and 2^64 / 10^5."""
    rng = random.Random(606)
    reqs, want = [], []
    for L in (44, 45, 50, 54, 55, 56, 57, 60, 63, 64, 100, 119, 120, 127):
        m = bytes(rng.randrange(33, 127) for _ in range(L))
        for lo, hi in ((0, 2_000_000), (10**9 - 700_000, 10**9 + 700_000),
                       (10**11 - 300_000, 10**11 + 900_000)):
            mn = oracle_mod.c_scan(m, lo, hi)
            T = 2**64 // 10**5
            reqs += [(m, lo, hi, mn[0] + 1), (m, lo, hi, T)]
            want += [mn, oracle_mod.c_find(m, lo, hi, T)]
    assert ctx.find_many(reqs) == want
    st = ctx.find_many_stats()
    assert st["fused"] == st["requests"] == len(reqs) and st["fallback"] == 0, st


def test_window_end(ctx, oracle_mod):
    """HM_OPT_FIND_WINDOW = 1000: the fused launch covers window nonces 0..999,
    the per-segment path the rest.  hs[p] is the strongest hash of 150,000
    nonces from `base`, so over [base + p - k, ...] at target hs[p] + 1 the
    first hit is window nonce k exactly.  The planner offers no segment that
    a fused launch cannot hold at this size (a 1000-nonce window has no chained
    segment of more than four final-block digits, for any message length 0..130
    and digit count), so no request here has an unfusible first segment."""
    m, base = b"window edge 1", 7_000_000
    hs = [oracle_mod.c_hash(m, base + i) for i in range(150_000)]
    p = min(range(len(hs)), key=hs.__getitem__)
    assert p >= 50_000 and hs.count(hs[p]) == 1
    T = hs[p] + 1
    ks = (998, 999, 1000, 1001, 50_000)
    reqs = [(m, base + p - k, base + p - k + 59_999, T) for k in ks]
    want = [(hs[p], base + p)] * len(ks)
    # ranges that end exactly at the window: the argmin, and no hit
    lo = base + 2000
    mn = min((hs[i], base + i) for i in range(2000, 3000))
    reqs += [(m, lo, lo + 999, mn[0] + 1), (m, lo, lo + 999, mn[0])]
    want += [mn, None]
    assert want == _expect(oracle_mod, reqs)
    ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 1000)
    try:
        got = ctx.find_many(reqs)
        st = ctx.find_many_stats()
    finally:
        ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 0)
    assert got == want
    past = sum(k > 999 for k in ks)
    assert st["fallback"] == past == 3 and st["fused"] == len(reqs) - past, st
    assert st["found"] == len(reqs) - 1 and st["launches"] >= len(reqs) + past, st
    for bad in (1, 63, (1 << 27) + 1, -1):
        with pytest.raises(_lib.HipMinerError) as ei:
            ctx.set_option(_lib.HM_OPT_FIND_WINDOW, bad)
        assert ei.value.rc == _lib.HM_ERR_INVALID


def test_edges(ctx, oracle_mod):
    h = oracle_mod.c_hash
    reqs = [(b"bradfitz", 5, 4, MAX), (b"bradfitz", 0, 10**5, 0)]
    want = [None, None]
    for n in (0, 9, 10, 10**19, MAX):
        reqs += [(b"x", n, n, h(b"x", n) + 1), (b"x", n, n, h(b"x", n))]
        want += [(h(b"x", n), n), None]
    lo = MAX - 150_000
    mn = oracle_mod.c_scan(b"bradfitz", lo, MAX)
    reqs += [(b"bradfitz", lo, MAX, mn[0] + 1), (b"bradfitz", lo, MAX, mn[0]),
             (b"", MAX, MAX, MAX), (b"bradfitz", lo, MAX, h(b"bradfitz", MAX) + 1)]
    want += [mn, None, (h(b"", MAX), MAX),
             oracle_mod.c_find(b"bradfitz", lo, MAX, h(b"bradfitz", MAX) + 1)]
    assert ctx.find_many(reqs) == want
    st = ctx.find_many_stats()
    # the two requests that enqueue nothing count in neither
    assert st["fused"] == len(reqs) - 2 and st["fallback"] == 0, st
    assert st["launches"] == len(reqs) - 2 and st["requests"] == len(reqs), st
    assert ctx.find_many([]) == []
    st = ctx.find_many_stats()
    assert st["requests"] == st["launches"] == st["tasks_total"] == 0, st
    # one message 64 times, 64 targets
    reqs = [(b"bradfitz", 0, 10**6, 2**64 // (500 * (i + 1))) for i in range(64)]
    assert ctx.find_many(reqs) == _expect(oracle_mod, reqs)
    # one and two requests past a chunk, and past two chunks
    rng = random.Random(65)
    for n in (65, 129):
        reqs = []
        for i in range(n):
            a = rng.randrange(10**rng.randrange(1, 19))
            reqs.append((b"chunk %d" % i, a, a + rng.randrange(3000), 2**64 // 1000))
        assert ctx.find_many(reqs) == _expect(oracle_mod, reqs), n
        st = ctx.find_many_stats()
        assert st["requests"] == st["fused"] == st["launches"] == n, st


def test_early_exit_inside_the_launch(ctx):
    """bradfitz over 2^27 nonces at 2^64 / 10^3 hits at nonce 203: one launch,
    and at most a quarter of its ~2.1e5 tasks run (a grid's first round is
    ~3e3 tasks; the condition of test_early_exit_inside_a_launch)."""
    T, want = KATS[0]
    assert ctx.find_many([(b"bradfitz", 0, 2**27 - 1, T)]) == [want]
    st = ctx.find_many_stats()
    assert st["launches"] == 1 and st["fused"] == 1 and st["nonces_enqueued"] == 2**27, st
    assert 0 < st["tasks_run"] <= st["tasks_total"] / 4, st


def test_random_requests_vs_oracle(ctx, oracle_mod):
    rng = random.Random(2027)
    reqs = []
    for _ in range(200):
        m = bytes(rng.randrange(256) for _ in range(rng.randrange(131)))
        if rng.random() < 0.6:
            lo = max(0, 10**rng.randrange(1, 20) - rng.randrange(1, 100_000))
        else:
            lo = rng.randrange(MAX)
        hi = min(MAX, lo + rng.randrange(200_000))
        reqs.append((m, lo, hi, 2**64 // 10**rng.randrange(2, 7)))
    want = _expect(oracle_mod, reqs)
    i = 0
    while i < len(reqs):
        n = rng.randrange(1, 81)
        got = ctx.find_many(reqs[i:i + n])
        assert got == want[i:i + n], (i, n)
        i += n


def test_fused_off_takes_the_per_segment_path(ctx, layout_cases):
    reqs, want, _ = layout_cases
    ctx.set_option(_lib.HM_OPT_FUSED, 0)
    try:
        got = ctx.find_many(reqs[:60])
        st = ctx.find_many_stats()
    finally:
        ctx.set_option(_lib.HM_OPT_FUSED, 1)
    assert got == want[:60]
    assert st["fused"] == 0 and st["fallback"] == 60 and st["launches"] >= 60, st


@pytest.mark.parametrize("ndev", [2, 3])
def test_several_devices(layout_cases, oracle_mod, ndev):
    reqs, want, _ = layout_cases
    reqs = reqs[30:38] + [(b"bradfitz", 0, 10**7, KATS[2][0]), (b"bradfitz", 5, 4, MAX)]
    want = want[30:38] + [KATS[2][1], None]
    with _lib.Context([0] * ndev) as c:
        assert c.find_many(reqs) == want
        st = c.find_many_stats()
        assert st["ndev"] == ndev and st["requests"] == 10 and st["fused"] == 9, st


def test_other_calls_and_their_stats_untouched(ctx, oracle_mod):
    with _lib.Context([0]) as c:
        with pytest.raises(_lib.HipMinerError) as ei:
            c.find_many_stats()
        assert ei.value.rc == _lib.HM_ERR_INVALID
    T = 2**64 // 10**4
    scan = ctx.scan(b"thom yorke", 0, 10**6)
    find = ctx.find(b"thom yorke", 0, 10**6, T)
    coll = ctx.collect(b"thom yorke", 0, 10**5, T, 64)
    ver = ctx.verify(b"thom yorke", coll[1], T, 8)
    before = (ctx.stats(), ctx.find_stats(), ctx.collect_stats(), ctx.verify_stats())
    ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 64)   # a fallback too
    try:
        assert ctx.find_many([(b"thom yorke", 0, 10**6, T), (b"x", 0, 99, 1)]) == [find, None]
        assert ctx.find_many_stats()["fallback"] == 2
    finally:
        ctx.set_option(_lib.HM_OPT_FIND_WINDOW, 0)
    assert (ctx.stats(), ctx.find_stats(), ctx.collect_stats(), ctx.verify_stats()) == before
    assert ctx.scan(b"thom yorke", 0, 10**6) == scan
    assert ctx.find(b"thom yorke", 0, 10**6, T) == find
    assert ctx.collect(b"thom yorke", 0, 10**5, T, 64) == coll
    assert ver[0] == 0


def test_deadline_applies_to_the_whole_call():
    """A 1-ms deadline on 64 no-hit requests of 2^27 nonces (~0.2 s of kernel):
    HM_ERR_TIMEOUT, outputs untouched, the context abandoned."""
    c = _lib.Context([0])
    assert c.find_many([(b"bradfitz", 0, 10**6, KATS[0][0])]) == [KATS[0][1]]
    c.set_option(_lib.HM_OPT_DEADLINE_MS, 1)
    n = 64
    keep = [b"deadline %d" % i for i in range(n)]
    arr = (_lib.hm_find_request * n)()
    outs = (_lib.hm_result * n)()
    found = (ctypes.c_int * n)()
    for i in range(n):
        arr[i] = _lib.hm_find_request(keep[i], len(keep[i]), 0, 2**27 - 1, 1)
        outs[i] = _lib.hm_result(0x5a5a, 0xa5a5)
        found[i] = 77
    lib = _lib.load()
    assert lib.hm_find_many(c._h, arr, n, outs, found) == _lib.HM_ERR_TIMEOUT
    assert all((outs[i].hash, outs[i].nonce, found[i]) == (0x5a5a, 0xa5a5, 77) for i in range(n))
    assert lib.hm_find_many(c._h, arr, 1, outs, found) == _lib.HM_ERR_TIMEOUT
    with pytest.raises(_lib.HipMinerError) as ei:
        c.find_many([(b"x", 0, 9, MAX)])
    assert ei.value.rc == _lib.HM_ERR_TIMEOUT
    c.close()  # host memory only: the queued work drains on its own

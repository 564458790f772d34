"""hm_find_k (ABI 1.16) on the GPU: the k LOWEST nonces of an inclusive range
whose hash is below a target, ascending, with hm_find's early exit -- "from
nonce lo, the next k shares" of the reference loop (cmu440/bitcoin/miner/
miner.go:46-59 over bitcoin.Hash, hash.go:13-17).  The reference is the already
pinned hm_collect (ctx.collect on the GPU, _lib.collect_cpu on the host) over a
bounded range, truncated to k: the answer must equal it bit for bit."""
import random

import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_find_host import TOP_CLEAR, top_nonce_case
from tests.test_gpu_find import KATS
from tests.test_gpu_find_paths import _piece_boundary
from tests.test_gpu_soak import _case

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
CAP = 1 << 16


def collect(c, m, lo, hi, T, cap=CAP):
    total, recs = c.collect(m, lo, hi, T, cap)
    assert recs is not None and total == len(recs), (total, cap)
    return recs


def target_for(hits, span):
    """The target at which `span` nonces hold about `hits` hits."""
    return min(MAX, 2**64 * hits // max(span, 1))


@pytest.fixture(params=["fast", "generic"])
def ctx_kernels(request, ctx):
    """The session context with and without HM_OPT_FORCE_GENERIC."""
    ctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 1 if request.param == "generic" else 0)
    try:
        yield ctx
    finally:
        ctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 0)


_BRADFITZ = {}


def bradfitz_hits():
    """Every hit of bradfitz over [0, 10^7] at 2^64 / 10^5, from the host (once)."""
    if "r" not in _BRADFITZ:
        total, recs = _lib.collect_cpu(b"bradfitz", 0, 10**7, 2**64 // 10**5, 4096)
        assert recs is not None and total >= 70
        _BRADFITZ["r"] = recs
    return _BRADFITZ["r"]


# ---- 1. known answers -------------------------------------------------------

def test_known_answers(ctx_kernels):
    c = ctx_kernels
    m, lo, hi, T = b"bradfitz", 0, 10**7, 2**64 // 10**5
    want = bradfitz_hits()
    assert want[0] == (158752571039048, 91989)
    total = len(want)
    for k in (1, 2, 7, 64, total, total + 5):
        assert c.find_k(m, lo, hi, T, k) == want[:k], k
        st = c.find_k_stats()
        assert st["found"] == min(k, total) and st["ndev"] == 1 and st["launches"] >= 1, st
        assert 0 < st["tasks_run"] <= st["tasks_total"] and st["fallback"] == 0, st
        assert st["records"] >= st["found"], st
    for T1, first in KATS:
        assert c.find_k(m, lo, hi, T1, 1) == [first] == [c.find(m, lo, hi, T1)], T1
    assert c.find_k(m, lo, hi, 0, 5) == []
    assert c.find_k_stats()["launches"] == 0
    assert c.find_k(m, 5, 4, MAX, 5) == []
    st = c.find_k_stats()
    assert st["launches"] == 0 and st["found"] == 0 and st["records"] == 0, st


def test_other_stats_unchanged(ctx):
    """hm_find_k keeps its own record: what hm_find's and hm_collect's report stays."""
    assert ctx.find(b"bradfitz", 0, 10**7, KATS[0][0]) == KATS[0][1]
    collect(ctx, b"bradfitz", 0, 10**6, 2**64 // 10**4)
    before = (ctx.find_stats(), ctx.collect_stats())
    assert ctx.find_k(b"bradfitz", 0, 10**7, 2**64 // 10**5, 3) == bradfitz_hits()[:3]
    assert (ctx.find_stats(), ctx.collect_stats()) == before


# ---- 2. every tiled layout --------------------------------------------------

def test_whole_tiles_every_layout(ctx):
    """One range of whole tiles per distinct planner layout (picked as
    test_gpu_find.test_whole_tiles_every_layout picks them), about 50 hits in
    each.  k beyond the total: nothing may be skipped."""
    rng = random.Random(77)
    seen = set()
    for L in range(0, 131):
        m = bytes(rng.randrange(32, 127) for _ in range(L))
        for d in (7, 8, 10, 12, 16, 20):
            dlo, dhi = 10**(d - 1), min(10**d - 1, MAX)
            seg = _lib.debug_plan(m, dlo, dhi)[0]
            if seg["kind"] == _lib.HM_KIND_GENERIC:
                continue
            key = (seg["kind"], seg["W1"], seg["straddle"], seg["trailer"], seg["V"], seg["lane3"])
            if key in seen:
                continue
            seen.add(key)
            span = min(2 * 10**seg["V"] + 12345, 3 * 10**8, (dhi - dlo) // 2)
            lo = rng.randrange(dlo, dhi - span)
            hi = lo + span
            T = target_for(50, span)
            want = collect(ctx, m, lo, hi, T)
            total = len(want)
            assert total >= 10, (key, total)
            for k in (1, 10, total + 3):
                assert ctx.find_k(m, lo, hi, T, k) == want[:k], (L, d, key, k)
                st = ctx.find_k_stats()
                assert st["fallback"] == 0 and 0 < st["tasks_run"] <= st["tasks_total"], (key, st)
            assert st["found"] == total and st["tasks_run"] == st["tasks_total"], (key, st)
    assert len(seen) >= 40, len(seen)


# ---- 3. the early exit inside one launch ------------------------------------

def test_early_exit_inside_a_launch(ctx):
    """One launch of 4e9 nonces at 2^64 / 10^6 (a hit per 10^6 nonces), k = 64:
    the 64th hit lies about 6.4e7 nonces in, and the waves stop at the stop
    word.  tasks_run * 4 <= tasks_total is a cap, not a measurement (as
    test_gpu_find.test_early_exit_inside_a_launch's); measured on one MI355X:
    15 347 of 680 497 tasks run (2.3 %), 106 records for the 64 answers."""
    m, lo, hi, T, k = b"bradfitz", 10**9, 5 * 10**9, 2**64 // 10**6, 64
    ref = collect(ctx, m, lo, lo + 2 * 10**8, T)
    assert len(ref) >= k, len(ref)
    assert ctx.find_k(m, lo, hi, T, k) == ref[:k]
    st = ctx.find_k_stats()
    print("early exit:", st)
    assert st["fallback"] == 0 and st["records"] >= k and st["found"] == k, st
    assert st["tasks_total"] >= 50_000, ("vacuous", st)
    assert st["tasks_run"] * 4 <= st["tasks_total"], st


# ---- 4. a digit boundary inside the answer ----------------------------------

def _boundary_case(c):
    m, lo, hi, T = b"bradfitz", 10**9 - 5 * 10**5, 10**9 + 5 * 10**7, 2**64 // 10**5
    want = collect(c, m, lo, hi, T)
    below = sum(1 for _, n in want if n < 10**9)
    assert below >= 1 and len(want) >= below + 3
    return m, lo, hi, T, want, below + 3


def test_digit_boundary_inside_the_answer(ctx_kernels, ctx):
    m, lo, hi, T, want, k = _boundary_case(ctx)
    got = ctx_kernels.find_k(m, lo, hi, T, k)
    assert got == want[:k] and got[-1][1] >= 10**9 > got[0][1]
    assert ctx_kernels.find_k_stats()["launches"] >= 2


# ---- 5. overflow ------------------------------------------------------------

def test_forced_overflow(ctx_kernels):
    """HM_OPT_FIND_K_BUF = k: a buffer of exactly k records, at a hit per 64
    nonces.  The records beyond the first k are lost, so the answer comes from
    the overflow path."""
    c = ctx_kernels
    m, lo, hi, T, k = b"bradfitz", 0, 10**6, 2**64 // 64, 100
    total, want = _lib.collect_cpu(m, lo, hi, T, CAP)
    assert want is not None and total > 10 * k
    c.set_option(_lib.HM_OPT_FIND_K_BUF, k)
    try:
        assert c.find_k(m, lo, hi, T, k) == want[:k]
        st = c.find_k_stats()
        assert st["fallback"] == 1 and st["found"] == k and st["records"] == k, st
    finally:
        c.set_option(_lib.HM_OPT_FIND_K_BUF, 0)
    # the default buffer (2k + 4096 records) holds this call's records or not:
    # the answer is the same
    assert c.find_k(m, lo, hi, T, k) == want[:k]


def test_natural_overflow(ctx_kernels):
    """T = 2^64-1: every nonce hits, one task alone overflows the default
    buffer.  The answer is the 1000 consecutive nonces from lo."""
    m, lo, hi, k = b"bradfitz", 12345, 10**9, 1000
    got = ctx_kernels.find_k(m, lo, hi, MAX, k)
    assert got == [(_lib.host_hash(m, n), n) for n in range(lo, lo + k)]
    st = ctx_kernels.find_k_stats()
    assert st["fallback"] == 1 and st["found"] == k, st


# ---- 6. the top of the nonce space ------------------------------------------

def test_top_of_the_nonce_space(ctx_kernels):
    m, h = top_nonce_case()
    lo = MAX - TOP_CLEAR
    assert ctx_kernels.find_k(m, lo, MAX, h + 1, 2) == [(h, MAX)]
    st = ctx_kernels.find_k_stats()
    assert st["found"] == 1 and st["tasks_run"] == st["tasks_total"], st
    assert ctx_kernels.find_k(m, lo, MAX, h + 1, 1) == [(h, MAX)]
    assert ctx_kernels.find_k(m, lo, MAX, h, 2) == []
    want = [(_lib.host_hash(b"", n), n) for n in range(MAX - 9, MAX + 1)]
    assert ctx_kernels.find_k(b"", MAX - 9, MAX, MAX, 5) == want[:5]
    assert ctx_kernels.find_k(b"", MAX - 9, MAX, MAX, 10) == want
    assert ctx_kernels.find_k(b"", MAX - 9, MAX, MAX, 12) == want


# ---- 7. two devices ---------------------------------------------------------

def test_two_devices(ctx):
    """Device 0 opened twice: each seeks k in its own shard, the host merges
    the union.  The single-device answers, and a range across the first
    multi-device piece boundary."""
    want = bradfitz_hits()
    bm, blo, bhi, bT, bwant, bk = _boundary_case(ctx)
    with _lib.Context([0, 0]) as c:
        for k in (1, 2, 7, 64, len(want), len(want) + 5):
            assert c.find_k(b"bradfitz", 0, 10**7, 2**64 // 10**5, k) == want[:k], k
            assert c.find_k_stats()["ndev"] == 2
        assert c.find_k(bm, blo, bhi, bT, bk) == bwant[:bk]
        m = b"jonny greenwood"
        B = _piece_boundary(m, 2, False)
        lo, hi = B - 70_000, B + 70_000
        T = target_for(50, hi - lo + 1)
        ref = collect(ctx, m, lo, hi, T)
        below = sum(1 for _, n in ref if n < B)
        assert below >= 5 and len(ref) >= below + 5, (below, len(ref))
        for k in (1, below, below + 3, len(ref) + 2):
            assert c.find_k(m, lo, hi, T, k) == ref[:k], k
            st = c.find_k_stats()
            # the second piece is issued when the first holds fewer than k hits,
            # and never after a device has found k in its shard of the first
            if k > below:
                assert st["nonces_enqueued"] > B - lo, (k, below, st)
            if k == 1:
                assert st["nonces_enqueued"] <= B - lo, (k, below, st)


# ---- 8. chained epochs ------------------------------------------------------

def test_chained_with_epochs(ctx):
    """Two-block tail with 5 final-block digits (b"x" * 56 at 12 digits) and a
    table of 10^3 rows: 10^2 epochs over the same tiles, whose launches are not
    ascending in their nonces (as test_gpu_find.test_chained_with_epochs)."""
    m = b"x" * 56
    rng = random.Random(56)
    a = 10**11 + rng.randrange(0, 300_000)
    b = 10**11 + 6_400_000 - 1 - rng.randrange(0, 300_000)
    T = target_for(50, b - a + 1)
    try:
        ctx.set_option(_lib.HM_OPT_TABLE_DIGITS, 3)
        seg = _lib.debug_plan(m, a, b)[0]
        assert seg["kind"] == _lib.HM_KIND_CHAINED and seg["f"] == 5, seg
        want = collect(ctx, m, a, b, T)
        assert len(want) >= 10
        for k in (1, 5):
            assert ctx.find_k(m, a, b, T, k) == want[:k], k
            st = ctx.find_k_stats()
            assert st["fallback"] == 0 and st["launches"] >= 2, st
    finally:
        ctx.set_option(_lib.HM_OPT_TABLE_DIGITS, 0)
    assert want == collect(ctx, m, a, b, T)


# ---- 9. a seeded sweep ------------------------------------------------------

def test_random_sweep(ctx):
    """40 seeded cases drawn as test_gpu_find_paths.test_random_sweep draws
    its ranges (spans capped at 3 * 10^8), the target set for about 30 hits, k
    random in 1..40, forced-generic and grid options and one or two "devices"
    at random: every answer equals hm_collect's first k records."""
    rng = random.Random(16)
    short = 0
    with _lib.Context([0, 0]) as c2:
        for i in range(40):
            m, lo, hi = _case(rng)
            hi = min(hi, lo + 3 * 10**8 - 1)
            T = target_for(30, hi - lo + 1)
            k = rng.randrange(1, 41)
            opts = {_lib.HM_OPT_FORCE_GENERIC: rng.choice([0, 0, 1]),
                    _lib.HM_OPT_GRID_PER_CU: rng.choice([0, 1, 2])}
            c = rng.choice([ctx, ctx, c2])
            want = collect(ctx, m, lo, hi, T)
            short += len(want) < k
            try:
                for o, v in opts.items():
                    c.set_option(o, v)
                got = c.find_k(m, lo, hi, T, k)
                st = c.find_k_stats()
            finally:
                for o in opts:
                    c.set_option(o, 0)
            tag = (i, m.hex(), lo, hi, T, k, opts, st)
            assert got == want[:k], tag
            assert st["found"] == min(k, len(want)), tag
            if len(want) < k and not st["fallback"]:
                assert st["tasks_run"] == st["tasks_total"], tag
    assert 3 <= short <= 37, short

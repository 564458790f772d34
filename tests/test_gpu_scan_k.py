"""hm_scan_k (ABI 1.19) on the GPU: the k lowest (hash, nonce) pairs of a
range, on every kernel instantiation it ships, bit-exact against references
that share no code with its reduction.

The case lists are those of tests/test_collect_layouts_host.py (every case
keyed by the plan of the exact range it runs); the oracle's per-nonce hashes of
the segment-edge windows are computed once per session by
tests/test_gpu_collect_layouts.py's edge_hashes.

  1. segment edges: every message length 0..130 x every digit count, fast and
     forced generic, k = 1, 32 and span + 5 clamped to 32, against the sorted
     oracle hashes;
  2. whole small tiles (<= 10^6 nonces per tile), k = 32, at the default grid
     and with one workgroup per CU, against a dense hm_collect sorted on the
     host, the oracle's minimum and the oracle's hash per record;
  3. whole big tiles (V = 7, 8, chained f <= 6): fast == forced generic,
     out[0] == hm_scan, the oracle's hash per record, and completeness by an
     hm_collect count at the k-th hash + 1;
  4. the carried bound across several launches and folds;
  5. piece boundaries on two and three "devices";
  6. the edges; 7. order independence; 8. the other families afterwards.
"""
import ctypes

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_collect_layouts_host as L
from tests.test_gpu_collect import collect_np, collect_with
from tests.test_gpu_collect_layouts import edge_hashes, scan_sum
from tests.test_gpu_find_paths import DEFAULTS, OPT_NAMES

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
KMAX = _lib.HM_SCAN_K_MAX
FAST = {_lib.HM_OPT_FORCE_GENERIC: 0}
GENERIC = {_lib.HM_OPT_FORCE_GENERIC: 1}
ONE_PER_CU = {_lib.HM_OPT_GRID_PER_CU: 1}
SMALL_PARTS = 8
BIG_PARTS = 8
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A)


def tag_of(m, lo, hi, k, opts, key=None):
    return (f"msg_hex={m.hex()} lo={lo} hi={hi} k={k} "
            f"opts={ {OPT_NAMES[o]: v for o, v in opts.items()} } key={key}")


def scan_k_with(c, opts, m, lo, hi, k):
    """(list, scan_k stats) of one hm_scan_k under `opts`, which are restored."""
    try:
        for o, v in opts.items():
            c.set_option(o, v)
        got = c.scan_k(m, lo, hi, k)
        return got, c.scan_k_stats()
    finally:
        for o in opts:
            c.set_option(o, DEFAULTS[o])


def lowest(hashes, nonces, k):
    """The k lexicographically smallest (hash, nonce) of two numpy arrays."""
    k = min(k, len(hashes))
    if len(hashes) > 4 * k:
        keep = hashes <= np.partition(hashes, k - 1)[k - 1]   # every record tied at the k-th too
        hashes, nonces = hashes[keep], nonces[keep]
    order = np.lexsort((nonces, hashes))[:k]
    return [(int(hashes[i]), int(nonces[i])) for i in order]


def dense_reference(c, m, lo, hi, k):
    """The first k of np.lexsort over a dense hm_collect of [lo, hi]."""
    span = hi - lo + 1
    total, hashes, nonces = collect_np(c, m, lo, hi, MAX, span)
    assert total == span, (total, span)     # no nonce of these ranges hashes to 2^64 - 1
    return lowest(hashes, nonces, k)


# ---- 1. segment edges -------------------------------------------------------

@pytest.mark.parametrize("how", ["fast", "generic"])
@pytest.mark.parametrize("group", range(len(L.EDGE_GROUPS)), ids=L.EDGE_IDS)
def test_segment_edges(ctx, oracle_mod, group, how):
    opts = GENERIC if how == "generic" else FAST
    try:
        for o, v in opts.items():
            ctx.set_option(o, v)
        for (m, d, lo, hi), hs in zip(L.edge_cases(group), edge_hashes(oracle_mod, group)):
            span = hi - lo + 1
            want = lowest(hs, np.arange(span, dtype=np.uint64), KMAX)
            want = [(h, lo + i) for h, i in want]
            for k in sorted({1, KMAX, min(span + 5, KMAX)}):
                got = ctx.scan_k(m, lo, hi, k)
                assert got == want[:k], (tag_of(m, lo, hi, k, opts), d, got[:3], want[:3])
                st = ctx.scan_k_stats()
                assert st["nonces"] == span and st["k"] == k and st["count"] == min(k, span), \
                    (tag_of(m, lo, hi, k, opts), st)
    finally:
        for o in opts:
            ctx.set_option(o, DEFAULTS[o])


# ---- 2. whole small tiles ---------------------------------------------------

@pytest.mark.parametrize("part", range(SMALL_PARTS))
def test_whole_tiles_small(ctx, oracle_mod, part):
    """One range per layout key with tiles of at most 10^6 nonces.  With one
    workgroup per CU every wave sees thousands of nonces: the bound, repeated
    compactions and the guided tail all run."""
    for c in L.parts(L.tile_cases()[0], SMALL_PARTS)[part]:
        m, lo, hi, key = c["m"], c["lo"], c["hi"], c["key"]
        span = hi - lo + 1
        want = dense_reference(ctx, m, lo, hi, KMAX)
        best, _, count = scan_sum(oracle_mod, m, lo, hi)
        assert count == span
        for opts in (FAST, ONE_PER_CU):
            tag = tag_of(m, lo, hi, KMAX, opts, key)
            got, st = scan_k_with(ctx, opts, m, lo, hi, KMAX)
            assert got == want, (tag, got[:3], want[:3])
            assert got[0] == tuple(best), (tag, got[0], best)
            assert st["nonces"] == span and st["count"] == min(KMAX, span), (tag, st)
            assert st["compactions"] > 0, (tag, st)
            if span >= 10**5:
                assert st["inserted"] < span, (tag, st)     # the bound is at work
        for h, n in want:
            assert oracle_mod.c_hash(m, n) == h, (tag_of(m, lo, hi, KMAX, FAST, key), h, n)


# ---- 3. whole big tiles -----------------------------------------------------

@pytest.mark.parametrize("part", range(BIG_PARTS))
def test_whole_tiles_big(ctx, oracle_mod, part):
    """One range per layout key with tiles of 10^7 nonces or more.  No CPU
    rescans these: the references are the forced-generic kernel, hm_scan, the
    oracle's hash per record, and hm_collect as a count for completeness."""
    for c in L.parts(L.tile_cases()[1], BIG_PARTS)[part]:
        m, lo, hi, key = c["m"], c["lo"], c["hi"], c["key"]
        span = hi - lo + 1
        tag = tag_of(m, lo, hi, KMAX, FAST, key)
        got, st = scan_k_with(ctx, FAST, m, lo, hi, KMAX)
        slow, _ = scan_k_with(ctx, GENERIC, m, lo, hi, KMAX)
        assert got == slow, (tag, got[:3], slow[:3])
        assert len(got) == KMAX and st["nonces"] == span, (tag, st)
        assert got[0] == ctx.scan(m, lo, hi), (tag, got[0])
        assert got == sorted(got) and len({n for _, n in got}) == KMAX, tag
        for h, n in got:
            assert lo <= n <= hi and oracle_mod.c_hash(m, n) == h, (tag, h, n)
        # completeness: exactly k records lie at or below the k-th hash, but for ties at it
        last = got[-1]
        (total, recs), _ = collect_with(ctx, FAST, m, lo, hi, last[0] + 1, 4 * KMAX)
        assert total >= KMAX and recs is not None, (tag, total)
        extra = sorted(set(recs) - set(got))
        assert total == KMAX + len(extra), (tag, total, extra)
        assert all(h == last[0] and n > last[1] for h, n in extra), (tag, extra)
        assert sorted(set(recs) & set(got)) == got, tag


# ---- 4. the carried bound ---------------------------------------------------

@pytest.mark.parametrize("lo,hi", [(0, 2_000_000), (999_000, 10_001_000), (5, 5)])
def test_carried_bound_across_launches(ctx, lo, hi):
    """Several digit segments, so several launches, each followed by its fold:
    the waves of a later launch start from the bound the earlier ones left."""
    m = b"bradfitz"
    want = dense_reference(ctx, m, lo, hi, KMAX)
    for k in (KMAX, 5, 1):
        got, st = scan_k_with(ctx, FAST, m, lo, hi, k)
        assert got == want[:k], (tag_of(m, lo, hi, k, FAST), got[:3], want[:3])
        assert st["nonces"] == hi - lo + 1 and st["count"] == len(want[:k]), st
        # at least one launch (and one fold) per digit segment
        assert st["launches"] >= len(_lib.debug_plan(m, lo, hi, False)), st
    assert got[0] == ctx.scan(m, lo, hi)


# ---- 5. piece boundaries ----------------------------------------------------

@pytest.mark.parametrize("generic", [0, 1], ids=["fast", "generic"])
@pytest.mark.parametrize("ndev", [2, 3])
def test_piece_boundaries(ndev, generic):
    """Ranges around, from, up to and at the first piece boundary of a context
    that names device 0 twice or three times: each "device" keeps its own list,
    the host merges them."""
    opts = {_lib.HM_OPT_FORCE_GENERIC: generic}
    with _lib.Context([0] * ndev) as c:
        for m, B, ranges in L.piece_cases(ndev, generic):
            for lo, hi in ranges:
                want = dense_reference(c, m, lo, hi, KMAX)
                got, st = scan_k_with(c, opts, m, lo, hi, KMAX)
                tag = tag_of(m, lo, hi, KMAX, opts)
                assert got == want, (tag, B, got[:3], want[:3])
                assert st["ndev"] == ndev and st["nonces"] == hi - lo + 1, (tag, st)


# ---- 6. edges ---------------------------------------------------------------

def scan_k_raw(c, m, lo, hi, k, room):
    buf = (_lib.hm_result * room)()
    for i in range(room):
        buf[i].hash, buf[i].nonce = SENTINEL
    n = ctypes.c_size_t(777)
    rc = _lib.load().hm_scan_k(c._h, m, len(m), lo, hi, k, buf, ctypes.byref(n))
    return rc, int(n.value), [(int(r.hash), int(r.nonce)) for r in buf]


def test_edges(ctx, oracle_mod, golden):
    m = b"bradfitz"
    # an empty range: *n = 0, the poisoned out untouched
    rc, n, buf = scan_k_raw(ctx, m, 5, 4, KMAX, KMAX + 1)
    assert (rc, n) == (_lib.HM_OK, 0) and all(r == SENTINEL for r in buf)
    assert ctx.scan_k_stats()["count"] == 0 and ctx.scan_k_stats()["launches"] == 0
    # span < k, across a digit-count change
    want = sorted((oracle_mod.c_hash(m, x), x) for x in range(95, 105))
    rc, n, buf = scan_k_raw(ctx, m, 95, 104, KMAX, KMAX + 1)
    assert (rc, n) == (_lib.HM_OK, 10) and buf[:10] == want and all(r == SENTINEL for r in buf[10:])
    # the top of the nonce space: all 20 records, nonce 2^64-1 among them
    want = sorted((oracle_mod.c_hash(m, x), x) for x in range(MAX - 19, MAX + 1))
    for opts in (FAST, GENERIC):
        got, st = scan_k_with(ctx, opts, m, MAX - 19, MAX, KMAX)
        assert got == want and MAX in [x for _, x in got] and st["count"] == 20, (opts, got[:3])
    # invalid arguments leave the outputs alone
    for k in (0, KMAX + 1):
        rc, n, buf = scan_k_raw(ctx, m, 0, 99, k, KMAX + 2)
        assert (rc, n) == (_lib.HM_ERR_INVALID, 777) and all(r == SENTINEL for r in buf)
    # k = 1 is every golden range scan
    for kat in golden["scan_kats"]:
        msg, lo, hi = bytes.fromhex(kat["msg_hex"]), int(kat["lo"]), int(kat["hi"])
        if lo > hi:
            assert ctx.scan_k(msg, lo, hi, 1) == []
            continue
        assert ctx.scan_k(msg, lo, hi, 1) == [(int(kat["hash"]), int(kat["nonce"]))], kat.get("name")


# ---- 7. order independence --------------------------------------------------

def test_order_independence(ctx):
    """The same request five times: which wave hashes what differs from run to
    run, the bytes of the answer do not."""
    c = max(L.tile_cases()[0], key=lambda c: c["hi"] - c["lo"])
    m, lo, hi = c["m"], c["lo"], c["hi"]
    runs = [scan_k_raw(ctx, m, lo, hi, KMAX, KMAX + 1) for _ in range(5)]
    assert runs[0][0] == _lib.HM_OK and runs[0][1] == KMAX
    assert all(r == runs[0] for r in runs[1:]), tag_of(m, lo, hi, KMAX, FAST, c["key"])
    got, _ = scan_k_with(ctx, ONE_PER_CU, m, lo, hi, KMAX)
    assert got == runs[0][2][:KMAX]


# ---- 8. the other families --------------------------------------------------

def test_other_families_after_scan_k(ctx, oracle_mod):
    """hm_scan_k leaves the context as it found it: hm_scan, hm_collect and
    hm_find_k answer exactly afterwards and keep their stats records; a
    deadline that holds changes nothing; hm_cancel has nothing to stop."""
    m, lo, hi = b"thom yorke", 10**9 - 500_000, 10**9 + 500_000
    best = oracle_mod.c_scan(m, lo, hi)
    assert ctx.scan(m, lo, hi) == best
    scan_st = ctx.stats()
    want = ctx.scan_k(m, lo, hi, KMAX)
    assert want[0] == best and ctx.stats() == scan_st
    T = want[-1][0] + 1
    assert ctx.scan(m, lo, hi) == best
    total, recs = ctx.collect(m, lo, hi, T, 4 * KMAX)
    assert total == KMAX and sorted(recs) == want
    by_nonce = sorted(want, key=lambda r: r[1])
    assert ctx.find_k(m, lo, hi, T, 5) == by_nonce[:5]
    assert ctx.cancel() is False
    got, st = scan_k_with(ctx, {_lib.HM_OPT_DEADLINE_MS: 60_000}, m, lo, hi, KMAX)
    assert got == want and st["count"] == KMAX
    got, _ = scan_k_with(ctx, {_lib.HM_OPT_DEADLINE_MS: -1}, m, lo, hi, KMAX)
    assert got == want
    assert ctx.scan_k(m, lo, hi, 7) == want[:7]

"""hm_collect on every kernel instantiation it ships, against the oracle.

The case lists are built, and their coverage checked on the host, by
tests/test_collect_layouts_host.py; every case is keyed by the plan of the
exact range it runs.  Every comparison is bit-exact.

  2. segment edges: every message length 0..130 x every digit count, the
     first and last 300 nonces of the digit segment, every hash against the
     CPU oracle's, on the fast kernels and on the generic one;
  3. whole tiles of every layout with tiles of at most 10^6 nonces, against
     the CPU oracle (every nonce, the hash sum, the minimum, a sparse list);
  4. whole tiles of every layout with larger tiles (V = 7, 8, chained f <= 6),
     against the forced-generic collect, hm_scan and, per record, the CPU
     oracle; then a dense window of each across a tile boundary, against the
     CPU oracle;
  5. piece boundaries on two and three "devices".

A failing case names its message (hex), range, target, options and key.
"""
import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_collect_layouts_host as L
from tests.test_gpu_collect import collect_np, collect_with, oracle_list
from tests.test_gpu_find_paths import DEFAULTS, OPT_NAMES

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
FAST = {_lib.HM_OPT_FORCE_GENERIC: 0}
GENERIC = {_lib.HM_OPT_FORCE_GENERIC: 1}
SPARSE_SMALL = 2**64 // 10**3
SPARSE_BIG = 2**64 // 10**5
TILE_PARTS = 8


def tag_of(m, lo, hi, T, opts, key):
    """The case as text: pytest prints a string in full, but abbreviates a
    tuple or a dict."""
    return (f"msg_hex={m.hex()} lo={lo} hi={hi} target={T} "
            f"opts={ {OPT_NAMES[o]: v for o, v in opts.items()} } key={key}")


def say(tag, *what):
    return tag + " | " + " | ".join(repr(w) for w in what)


def dense(c, opts, m, lo, hi, key):
    """hm_collect at T = 2^64 - 1 with cap = span under `opts` (restored):
    total == span, the nonces are exactly lo..hi ascending, the stats count
    span nonces.  Returns the hashes (numpy uint64)."""
    span = hi - lo + 1
    tag = tag_of(m, lo, hi, MAX, opts, key)
    try:
        for o, v in opts.items():
            c.set_option(o, v)
        total, hashes, nonces = collect_np(c, m, lo, hi, MAX, span)
        st = c.collect_stats()
    finally:
        for o in opts:
            c.set_option(o, DEFAULTS[o])
    assert total == span, say(tag, total)
    assert st["nonces"] == span and st["total"] == span and st["overflow"] == 0, say(tag, st)
    want = np.arange(lo, hi + 1, dtype=np.uint64) if hi < MAX else \
        np.array(range(lo, hi + 1), dtype=np.uint64)
    assert np.array_equal(nonces, want), say(tag, nonces[:4], np.flatnonzero(nonces != want)[:4])
    return hashes


def scan_sum(oracle_mod, m, lo, hi):
    """The CPU oracle's ((min hash, its nonce), sum of all hashes mod 2^64, count)."""
    if oracle_mod.fast_available():
        return oracle_mod.fast_scan_sum(m, lo, hi)
    return oracle_mod.c_scan_sum(m, lo, hi)


def wrapped_sum(hashes):
    return int(np.sum(hashes, dtype=np.uint64))     # uint64 addition wraps: mod 2^64


# ---- 2. segment edges -------------------------------------------------------

_EDGE_HASHES = {}


def edge_hashes(oracle_mod, group):
    """oracle.c_hash of every nonce of every window of the group, once."""
    if group not in _EDGE_HASHES:
        _EDGE_HASHES[group] = [np.array([oracle_mod.c_hash(m, n) for n in range(lo, hi + 1)],
                                        dtype=np.uint64)
                               for m, _, lo, hi in L.edge_cases(group)]
    return _EDGE_HASHES[group]


@pytest.mark.parametrize("how", ["fast", "generic"])
@pytest.mark.parametrize("group", range(len(L.EDGE_GROUPS)), ids=L.EDGE_IDS)
def test_segment_edges(ctx, oracle_mod, group, how):
    """Every message length 0..130 x every digit count: the first and last (at
    most) 300 nonces of the digit segment.  At T = 2^64 - 1 every nonce comes
    back once, ascending, with the oracle's hash; at T = the 4th-smallest hash
    + 1 the list is the oracle's filtered list (the strict '<')."""
    opts = GENERIC if how == "generic" else FAST
    for (m, d, lo, hi), hs in zip(L.edge_cases(group), edge_hashes(oracle_mod, group)):
        span = hi - lo + 1
        key = L.plan_key(m, lo, hi, how == "generic")
        got = dense(ctx, opts, m, lo, hi, key)
        bad = np.flatnonzero(got != hs)
        assert bad.size == 0, say(tag_of(m, lo, hi, MAX, opts, key), d,
                                  [(lo + int(i), int(got[i]), int(hs[i])) for i in bad[:4]])
        T = int(np.sort(hs)[min(3, span - 1)]) + 1
        want = [(int(h), lo + i) for i, h in enumerate(hs) if int(h) < T]
        assert 1 <= len(want) and (len(want) >= 4 or span < 4)
        (total, recs), st = collect_with(ctx, opts, m, lo, hi, T, span)
        assert (total, recs) == (len(want), want), say(tag_of(m, lo, hi, T, opts, key), d, total,
                                                       recs, want)
        assert st["nonces"] == span, say(tag_of(m, lo, hi, T, opts, key), st)


# ---- 3. whole tiles against the CPU oracle ----------------------------------

@pytest.mark.parametrize("part", range(TILE_PARTS))
def test_whole_tiles_small_vs_cpu_oracle(ctx, oracle_mod, part):
    """One range per layout key with tiles of at most 10^6 nonces: two whole
    tiles and a partial tile at each end, or the whole digit segment where
    that is a single tile.  T = 2^64 - 1: every nonce once, the wrapped sum of
    the hashes and the record at the minimum equal the oracle's.  T = 2^64 /
    10^3: the list equals the ascending oracle loop's."""
    for c in L.parts(L.tile_cases()[0], TILE_PARTS)[part]:
        m, lo, hi, key = c["m"], c["lo"], c["hi"], c["key"]
        span = hi - lo + 1
        best, total, count = scan_sum(oracle_mod, m, lo, hi)
        assert count == span
        hashes = dense(ctx, FAST, m, lo, hi, key)
        tag = tag_of(m, lo, hi, MAX, FAST, key)
        assert wrapped_sum(hashes) == total, say(tag, wrapped_sum(hashes), total)
        k = int(np.argmin(hashes))                  # the first of equal minima: the lowest nonce
        assert (int(hashes[k]), lo + k) == tuple(best), say(tag, int(hashes[k]), lo + k, best)
        want = oracle_list(oracle_mod, m, lo, hi, SPARSE_SMALL)
        (n, recs), st = collect_with(ctx, FAST, m, lo, hi, SPARSE_SMALL, len(want) + 8)
        tag = tag_of(m, lo, hi, SPARSE_SMALL, FAST, key)
        assert n == len(want) and recs == want, say(tag, n, len(want), (recs or [])[:4], want[:4])
        assert st["nonces"] == span, say(tag, st)


# ---- 4. whole tiles against independent kernels -----------------------------

def count_with(c, opts, m, lo, hi, T):
    (total, _), st = collect_with(c, opts, m, lo, hi, T, 0)
    return total, st


@pytest.mark.parametrize("part", range(TILE_PARTS))
def test_whole_tiles_big_vs_independent_kernels(ctx, oracle_mod, part):
    """One range per layout key with tiles of 10^7 nonces or more (tiled V =
    7, 8, chained up to f = 6), of min(2 * 10^V + 12345, 3 * 10^8) nonces.
    No CPU rescans these; the references share no tail-building text with the
    tiled and chained task bodies: the forced-generic collect, hm_scan, and
    the CPU oracle per record (and on a dense window, the next test)."""
    for c in L.parts(L.tile_cases()[1], TILE_PARTS)[part]:
        m, lo, hi, key = c["m"], c["lo"], c["hi"], c["key"]
        span = hi - lo + 1
        # exact count, and with one workgroup per CU: the guided-split tail
        for opts in (FAST, {_lib.HM_OPT_GRID_PER_CU: 1}):
            total, st = count_with(ctx, opts, m, lo, hi, MAX)
            assert total == span and st["nonces"] == span, say(tag_of(m, lo, hi, MAX, opts, key),
                                                               total, st)
        # the sparse list: the generic kernel's, and the oracle's hash per record
        T = SPARSE_BIG
        tag = tag_of(m, lo, hi, T, FAST, key)
        cap = span // 10**5 * 2 + 4096
        (n, recs), _ = collect_with(ctx, FAST, m, lo, hi, T, cap)
        (gn, grecs), _ = collect_with(ctx, GENERIC, m, lo, hi, T, cap)
        assert recs is not None and (n, recs) == (gn, grecs), say(tag, n, gn)
        assert n > 0 and all(a[1] < b[1] for a, b in zip(recs, recs[1:])), tag
        for h, nonce in recs:
            assert lo <= nonce <= hi and h < T, say(tag, h, nonce)
            assert oracle_mod.c_hash(m, nonce) == h, say(tag, h, nonce)
        # the minimum
        best = ctx.scan(m, lo, hi)
        (n, recs), _ = collect_with(ctx, FAST, m, lo, hi, best[0] + 1, 8)
        assert (n, recs) == (1, [best]), say(tag_of(m, lo, hi, best[0] + 1, FAST, key), n, recs)
        assert oracle_mod.c_hash(m, best[1]) == best[0]


@pytest.mark.parametrize("part", range(TILE_PARTS))
def test_dense_windows_big(ctx, oracle_mod, part):
    """A dense window of each of those ranges at T = 2^64 - 1: every nonce
    once, the wrapped sum of the hashes equal to the CPU oracle's.  High lane
    values, vmax clamping and, where the range has one, a tile change.

    The window is [k 10^V - 10^5, k 10^V + 10^5) where it plans to the case's
    key.  Chained f = 5 with 5 lane digits needs whole lane chunks on both
    sides of the boundary (9.6 * 10^6 nonces).  A digit segment of a single
    tile has no boundary: the window is the segment's last 2 * 10^5 nonces,
    for chained f = 5 its last whole lane chunks (up to 1.44 * 10^7 nonces).
    Chained f = 6 has no window: 2^24 nonces, the most one collect returns,
    are a quarter of one of its lane chunks, and the planner runs such a
    range tiled."""
    for c in L.parts(L.window_cases(), TILE_PARTS, L.window_size)[part]:
        m, key = c["m"], c["key"]
        wlo, whi, _ = c["window"]
        _, total, count = scan_sum(oracle_mod, m, wlo, whi)
        assert count == whi - wlo + 1
        got = wrapped_sum(dense(ctx, FAST, m, wlo, whi, key))
        assert got == total, say(tag_of(m, wlo, whi, MAX, FAST, key), got, total)


# ---- 5. piece boundaries ----------------------------------------------------

@pytest.mark.parametrize("generic", [0, 1], ids=["fast", "generic"])
@pytest.mark.parametrize("ndev", [2, 3])
def test_piece_boundaries(oracle_mod, ndev, generic):
    """Ranges around, from, up to and at the first piece boundary B of a
    context that names device 0 twice or three times: a nonce dropped or
    doubled at the cut changes the total."""
    opts = {_lib.HM_OPT_FORCE_GENERIC: generic}
    with _lib.Context([0] * ndev) as c:
        for m, B, ranges in L.piece_cases(ndev, generic):
            for lo, hi in ranges:
                span = hi - lo + 1
                key = L.plan_key(m, lo, hi, bool(generic))
                _, total, count = scan_sum(oracle_mod, m, lo, hi)
                assert count == span
                hashes = dense(c, opts, m, lo, hi, key)
                assert c.collect_stats()["ndev"] == ndev
                tag = tag_of(m, lo, hi, MAX, opts, key)
                assert wrapped_sum(hashes) == total, say(tag, B, wrapped_sum(hashes), total)
                want = oracle_list(oracle_mod, m, lo, hi, SPARSE_SMALL)
                (n, recs), st = collect_with(c, opts, m, lo, hi, SPARSE_SMALL, len(want) + 8)
                tag = tag_of(m, lo, hi, SPARSE_SMALL, opts, key)
                assert (n, recs) == (len(want), want), say(tag, B, n, len(want))
                assert st["ndev"] == ndev and st["nonces"] == span, say(tag, st)

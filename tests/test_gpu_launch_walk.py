"""hm_scan, hm_find and hm_collect turn a segment into the same launches.

The three drivers share one walk over a segment (csrc/seg_walk.cpp SegWalk):
generic chunks, tile windows, chained epochs, the K+W table a short device
shrinks.  These cases pin that they agree: on a miss (target = 1: no 64-bit
hash is below it) hm_find prunes nothing and so issues every launch
hm_collect does, and with the fused launches off the scan issues them too --
but for a generic segment, which the scan runs as one launch and find and
collect in chunks of 2^30 nonces.  One device throughout.
"""
import random

import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_gpu_collect import oracle_list

pytestmark = pytest.mark.gpu
THREADS = 16  # the GPU box's CPU share
MAX = (1 << 64) - 1
MISS = 1      # a target no hash is below

M58 = bytes(random.Random(58).randrange(33, 127) for _ in range(58))  # test_epoch_edges_and_partial_lanes
M48 = bytes(random.Random(48).randrange(33, 127) for _ in range(48))  # test_top_of_the_nonce_space
CHAINED = (M58, 10**9 + 4_321_987, 10**9 + 35_556_554)
# (name, message, lo, hi, options, layout of the largest segment)
CASES = [
    # crosses two digit counts, starts and ends inside a tile
    ("tiled", b"bradfitz", 10**6 - 12_345, 10**7 + 54_321, {}, _lib.HM_KIND_TILED),
    ("chained-10^2-rows", *CHAINED, {_lib.HM_OPT_TABLE_DIGITS: 2}, _lib.HM_KIND_CHAINED),
    ("chained-10^4-rows", *CHAINED, {_lib.HM_OPT_TABLE_DIGITS: 4}, _lib.HM_KIND_CHAINED),
    ("generic", b"bradfitz", 10**9, 10**9 + 2**30 + 5, {_lib.HM_OPT_FORCE_GENERIC: 1},
     _lib.HM_KIND_GENERIC),
    ("top", M48, MAX - 30_000_000, MAX, {}, _lib.HM_KIND_CHAINED),
]
RESTORE = {_lib.HM_OPT_TABLE_DIGITS: 0, _lib.HM_OPT_FORCE_GENERIC: 0, _lib.HM_OPT_FUSED: 1,
           _lib.HM_OPT_TAIL_FUSED: 1, _lib.HM_OPT_TABLE_ROWS_CAP: 0}


@pytest.fixture()
def options(ctx):
    """Set options on the session context; every one is restored."""
    def set_all(opts):
        for o, v in opts.items():
            ctx.set_option(o, v)
    try:
        yield set_all
    finally:
        set_all(RESTORE)


def miss_launches(c, m, lo, hi):
    """Launch counts of a find and a collect that meet nothing, after checking
    that each enqueued every nonce of [lo, hi] exactly once."""
    assert c.find(m, lo, hi, MISS) is None
    fs = c.find_stats()
    assert c.collect(m, lo, hi, MISS, 0) == (0, [])
    cs = c.collect_stats()
    assert fs["nonces_enqueued"] == cs["nonces"] == hi - lo + 1, (fs, cs)
    assert fs["tasks_run"] == fs["tasks_total"], fs
    return fs["launches"], cs["launches"]


@pytest.mark.parametrize("name,m,lo,hi,opts,kind", CASES, ids=[c[0] for c in CASES])
def test_find_and_collect_agree_on_a_miss(ctx, options, name, m, lo, hi, opts, kind):
    options(opts)
    generic = bool(opts.get(_lib.HM_OPT_FORCE_GENERIC))
    seg = max(_lib.debug_plan(m, lo, hi, generic), key=lambda s: s["hi"] - s["lo"])
    assert seg["kind"] == kind, seg
    find, collect = miss_launches(ctx, m, lo, hi)
    print(f"{name}: find launches {find}, collect launches {collect}")
    assert find == collect >= 1
    if generic:
        assert find == 2  # chunks of 2^30 nonces


@pytest.mark.parametrize("name,m,lo,hi,opts,kind", CASES[:4], ids=[c[0] for c in CASES[:4]])
def test_scan_agrees_with_find_per_segment(ctx, options, name, m, lo, hi, opts, kind):
    options({**opts, _lib.HM_OPT_FUSED: 0, _lib.HM_OPT_TAIL_FUSED: 0})
    assert ctx.find(m, lo, hi, MISS) is None
    find = ctx.find_stats()["launches"]
    ctx.scan(m, lo, hi)
    st = ctx.stats()
    print(f"{name}: scan launches {st['launches']} ({st['dom_launches']} of {st['dom_kernel']}), "
          f"find launches {find}")
    assert st["dom_kind"] == kind, st
    if kind == _lib.HM_KIND_GENERIC:
        # by design: the scan runs a generic segment as one launch
        assert (st["launches"], find) == (1, 2)
    else:
        assert st["launches"] == find


def test_the_table_shrinks_the_same_way(oracle_mod):
    """A device that may not grow its K+W table past 100 rows keeps the 10^4
    rows hm_open made: the segment, planned with a 10^5-row table, runs as 10
    epochs -- in all three drivers alike, and with the oracle's answers."""
    m, lo, hi = CHAINED
    seg = _lib.debug_plan(m, lo, hi)[0]
    assert seg["kind"] == _lib.HM_KIND_CHAINED and (seg["f"], seg["fe"]) == (5, 5), seg
    T = 2**64 // 10**6  # about 30 records
    exp_scan = oracle_mod.fast_scan_sum(m, lo, hi, threads=THREADS)
    exp_list = oracle_list(oracle_mod, m, lo, hi, T)
    with _lib.Context([0]) as c:
        for o, v in {_lib.HM_OPT_TABLE_ROWS_CAP: 100, _lib.HM_OPT_FUSED: 0,
                     _lib.HM_OPT_TAIL_FUSED: 0}.items():
            c.set_option(o, v)
        assert c.scan_checked(m, lo, hi) == exp_scan
        st = c.stats()
        find, collect = miss_launches(c, m, lo, hi)
        print(f"rows cap: scan launches {st['launches']}, find {find}, collect {collect}")
        assert st["launches"] == find == collect >= 10
        assert st["table_grows"] == 0, st
        assert c.collect(m, lo, hi, T, 256) == (len(exp_list), exp_list)
        assert c.collect_stats()["launches"] == collect

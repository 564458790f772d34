"""hm_collect (ABI 1.11) on the GPU: every nonce of a range whose hash is below
a target, ascending, and their exact count, against the CPU oracle of the
question (tests/test_collect_host.py: the committed oracle's c_find iterated
from lo, restarted at answer + 1 -- a plain ascending loop over the oracle's
own SHA-256 and formatting).

  a. a seeded differential sweep over messages, ranges, target edges, dense
     targets, options, buffer sizes (fitting, exact, maximal, too small, none)
     and 1-3 "devices", plus chained cases with epochs;
  b. surplus lanes: the smallest shapes that can double-count, at a target
     every nonce meets;
  c. self-consistency over [0, 2^30), a size no CPU rescans;
  d. buffer growth and reuse on one context, beside hm_scan and hm_find;
  e. nonce 2^64-1 as an ordinary record;
  f. a deadline expiring inside a collect.

The case list of (a) is a pure function of its seed; a host-only test checks
what it covers.
"""
import ctypes
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_collect_host import SENTINEL, oracle_loop
from tests.test_find_host import TOP_CLEAR, top_nonce_case
from tests.test_gpu_find_paths import DEFAULTS, OPT_NAMES, _chained_case, _draw_target
from tests.test_gpu_soak import _case

MAX = (1 << 64) - 1
CAP_MAX = _lib.HM_COLLECT_CAP_MAX


def oracle_list(oracle_mod, m, lo, hi, T):
    """The oracle's list for one case: the range cut into up to 16 contiguous
    parts, each walked by the ascending c_find loop (one thread per call), in
    parallel; the parts ascend, so their concatenation is the whole loop's.
    A dense target is walked in one part: its cost is the c_find call per
    record (about 5 us), which threads of one interpreter only slow down.
    The 150 cases hold about 3.5 * 10^6 records in all, so the list costs
    some 20 s of CPU once per session, whichever test asks first."""
    span = hi - lo + 1
    n = 1 if T > 2**64 // 100 else max(1, min(16, span // 4096))
    b = [lo + span * i // n for i in range(n + 1)]
    with ThreadPoolExecutor(n) as ex:
        parts = list(ex.map(lambda i: oracle_loop(oracle_mod, m, b[i], b[i + 1] - 1, T), range(n)))
    return [r for p in parts for r in p]


def collect_with(c, opts, m, lo, hi, T, cap):
    """((total, records or None), collect stats) of one collect under `opts`,
    which are restored."""
    try:
        for o, v in opts.items():
            c.set_option(o, v)
        got = c.collect(m, lo, hi, T, cap)
        return got, c.collect_stats()
    finally:
        for o in opts:
            c.set_option(o, DEFAULTS[o])


def collect_np(c, m, lo, hi, T, cap):
    """hm_collect into a numpy buffer (no Python tuples: millions of records):
    (total, hashes, nonces) with the arrays None on overflow."""
    buf = np.empty((max(cap, 1), 2), dtype=np.uint64)
    total = ctypes.c_uint64(0)
    rc = _lib.load().hm_collect(c._h, m, len(m), lo, hi, T,
                                buf.ctypes.data_as(ctypes.POINTER(_lib.hm_result)), cap,
                                ctypes.byref(total))
    assert rc == _lib.HM_OK, rc
    t = int(total.value)
    return (t, None, None) if t > cap else (t, buf[:t, 0], buf[:t, 1])


def kinds_of(m, lo, hi, generic=False):
    return {s["kind"] for s in _lib.debug_plan(m, lo, hi, generic)}


# ---- a. the seeded differential sweep ---------------------------------------

SWEEP_SEED = 1
SWEEP_CASES = 150
EPOCH_CASES = 10
SPAN_CAP = 300_000
SWEEP_PARTS = 5
# The chained-with-epochs cases span ~6 * 10^6 nonces (one lane chunk of 64 *
# 10^5).  The oracle costs one c_find call per record, so their targets are
# redrawn until they meet at most about one nonce in 10^3; dense targets on the
# chained layout (f <= 4) come from the 150 other cases and from (b).
EPOCH_T_MAX = 2**64 // 10**3
_CASES = {}


def sweep_cases(oracle_mod, seed, n, epochs):
    """The sweep's cases with the oracle's lists: a pure function of the seed
    (no GPU), computed once and shared."""
    key = (seed, n, epochs)
    if key in _CASES:
        return _CASES[key]
    rng = random.Random(seed)
    cases = []
    for i in range(n):
        if epochs:
            m, lo, hi, table = _chained_case(rng)
        else:
            m, lo, hi = _case(rng)
            hi = min(hi, lo + SPAN_CAP - 1)
            table = 0
        T = _draw_target(rng, oracle_mod, m, lo, hi)
        while epochs and T > EPOCH_T_MAX:
            T = _draw_target(rng, oracle_mod, m, lo, hi)
        opts = {_lib.HM_OPT_FORCE_GENERIC: rng.choice([0, 1]),
                _lib.HM_OPT_GRID_PER_CU: rng.choice([0, 1, 2]),
                _lib.HM_OPT_TABLE_DIGITS: table}
        ndev = rng.choice([1, 1, 2, 3])
        cap_draw = rng.randrange(8)
        exp = oracle_list(oracle_mod, m, lo, hi, T)
        total = len(exp)
        if cap_draw < 6 or total == 0:   # three quarters: the records fit
            cap = (total, total + 7, CAP_MAX)[cap_draw % 3]
        else:                            # the rest: no buffer, or one record short
            cap = (0, total - 1)[cap_draw - 6]
        cases.append({"i": i, "m": m, "lo": lo, "hi": hi, "T": T, "opts": opts, "ndev": ndev,
                      "cap": cap, "exp": exp,
                      "kinds": kinds_of(m, lo, hi, bool(opts[_lib.HM_OPT_FORCE_GENERIC]))})
    _CASES[key] = cases
    return cases


def test_sweep_seed_covers_the_ground(oracle_mod):
    """Host-only: the seeded case list holds every layout kind, an empty
    answer, an answer that is the whole range, and an overflow."""
    cases = sweep_cases(oracle_mod, SWEEP_SEED, SWEEP_CASES, epochs=False)
    assert cases == sweep_cases(oracle_mod, SWEEP_SEED, SWEEP_CASES, epochs=False)
    assert len(cases) == SWEEP_CASES
    kinds = set().union(*(c["kinds"] for c in cases))
    assert kinds >= {_lib.HM_KIND_GENERIC, _lib.HM_KIND_TILED, _lib.HM_KIND_CHAINED}, kinds
    fast = set().union(*(c["kinds"] for c in cases if not c["opts"][_lib.HM_OPT_FORCE_GENERIC]))
    assert fast >= {_lib.HM_KIND_TILED, _lib.HM_KIND_CHAINED}, fast
    empty = sum(len(c["exp"]) == 0 for c in cases)
    whole = sum(len(c["exp"]) == c["hi"] - c["lo"] + 1 for c in cases)
    over = sum(len(c["exp"]) > c["cap"] for c in cases)
    big = sum(c["cap"] == CAP_MAX for c in cases)
    multi = sum(c["ndev"] > 1 for c in cases)
    print(f"sweep seed {SWEEP_SEED}: {empty} empty, {whole} whole-range, {over} overflows, "
          f"{big} at the largest cap, {multi} on several devices")
    assert empty >= 1 and whole >= 1 and over >= 1 and big >= 1 and multi >= 1
    for c in cases:
        assert c["hi"] - c["lo"] + 1 <= SPAN_CAP and 0 <= c["cap"] <= CAP_MAX
        assert all(c["lo"] <= n <= c["hi"] and h < c["T"] for h, n in c["exp"])


@pytest.fixture(scope="module")
def multi():
    """Contexts that name device 0 twice and three times."""
    with _lib.Context([0, 0]) as c2, _lib.Context([0, 0, 0]) as c3:
        yield {2: c2, 3: c3}


def _run_sweep(ctx, multi, cases):
    for case in cases:
        c = ctx if case["ndev"] == 1 else multi[case["ndev"]]
        m, lo, hi, T, cap, exp = (case[k] for k in ("m", "lo", "hi", "T", "cap", "exp"))
        tag = {"case": case["i"], "msg_hex": m.hex(), "lo": lo, "hi": hi, "target": T, "cap": cap,
               "ndev": case["ndev"], "opts": {OPT_NAMES[o]: v for o, v in case["opts"].items()}}
        (total, recs), st = collect_with(c, case["opts"], m, lo, hi, T, cap)
        assert total == len(exp), (tag, total, len(exp))
        if total > cap:
            assert recs is None and st["overflow"] == 1, (tag, st)
        else:
            assert recs == exp, (tag, recs[:4], exp[:4])
            assert st["overflow"] == 0, (tag, st)
        assert st["nonces"] == hi - lo + 1 and st["total"] == total, (tag, st)
        assert st["ndev"] == case["ndev"] and st["launches"] >= 1, (tag, st)


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_random_sweep(ctx, multi, oracle_mod, part):
    """150 seeded cases drawn as test_gpu_soak._case draws them (spans capped
    at 3 * 10^5), each with a target from the find sweep's edge set, under
    random generic / grid options on one, two or three "devices", with a
    buffer that fits (exactly, with room, or HM_COLLECT_CAP_MAX) on three
    quarters of them and none or one record short on the rest: the total and
    the list equal the oracle's, or the overflow contract holds."""
    cases = sweep_cases(oracle_mod, SWEEP_SEED, SWEEP_CASES, epochs=False)
    _run_sweep(ctx, multi, cases[part::SWEEP_PARTS])


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(2))
def test_random_sweep_chained_epochs(ctx, multi, oracle_mod, part):
    """Ten further cases on the chained layout (f = 5) under a random
    HM_OPT_TABLE_DIGITS: up to 10^4 epochs over the same tiles."""
    cases = sweep_cases(oracle_mod, SWEEP_SEED + 1, EPOCH_CASES, epochs=True)
    assert any(c["opts"][_lib.HM_OPT_FORCE_GENERIC] == 0 and
               c["opts"][_lib.HM_OPT_TABLE_DIGITS] in (1, 2, 3, 4) for c in cases)
    assert all(c["kinds"] == {_lib.HM_KIND_CHAINED} for c in cases
               if not c["opts"][_lib.HM_OPT_FORCE_GENERIC])
    _run_sweep(ctx, multi, cases[part::2])


# ---- b. surplus lanes -------------------------------------------------------

def _all_of(c, m, lo, hi, opts=None):
    """At T = 2^64-1 every nonce is a hit (a hash of 2^64-1 aside: none in
    these ranges, or the count would fall short): a lane that repeats a nonce
    makes total > span.  The count, and the records with cap = span."""
    span = hi - lo + 1
    opts = opts or {}
    try:
        for o, v in opts.items():
            c.set_option(o, v)
        assert c.count(m, lo, hi, MAX) == span, (m, lo, hi, opts)
        total, hashes, nonces = collect_np(c, m, lo, hi, MAX, span)
    finally:
        for o in opts:
            c.set_option(o, DEFAULTS[o])
    assert total == span, (m, lo, hi, opts, total)
    assert np.array_equal(nonces, np.arange(lo, hi + 1, dtype=np.uint64)), (m, lo, hi, opts)
    for k in sorted({0, span // 2, span - 1}):
        assert int(hashes[k]) == _lib.host_hash(m, lo + k)


SMALL = (1, 63, 64, 65, 100)
SHAPES = {"generic": (b"bradfitz", 0, _lib.HM_KIND_GENERIC),
          "tiled": (b"bradfitz", 123456, _lib.HM_KIND_TILED),
          "chained": (b"y" * 55, 10**8 + 7, _lib.HM_KIND_CHAINED)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_surplus_lanes_small_ranges(ctx, multi, kind):
    """Ranges of 1, 63, 64, 65 and 100 nonces on each kernel kind: fewer
    nonces than one wave has lanes, exactly as many, one more."""
    m, lo, want = SHAPES[kind]
    for n in SMALL:
        assert kinds_of(m, lo, lo + n - 1) == {want}, (kind, n)
        _all_of(ctx, m, lo, lo + n - 1)
        _all_of(multi[3], m, lo, lo + n - 1)


@pytest.mark.gpu
def test_surplus_lanes_partial_chunks(ctx):
    """A tiled segment whose vmax + 1 is no multiple of 64 (10^q lane values:
    the last lane chunk of every tile is part surplus), a guided-split tail
    (more units than the grid has waves, so whole units and tenth-units run
    in one launch), and a generic segment of 64 k + 1 nonces with more
    workgroups than the grid, so waves stride."""
    m = b"bradfitz"
    assert kinds_of(m, 10**5, 10**5 + 9999) == {_lib.HM_KIND_TILED}
    _all_of(ctx, m, 10**5, 10**5 + 9999)
    _all_of(ctx, b"y" * 55, 10**8, 10**8 + 99_999)      # chained: whole lane chunks and a part
    assert kinds_of(b"y" * 55, 10**8, 10**8 + 99_999) == {_lib.HM_KIND_CHAINED}
    lo, hi = 2 * 10**7, 2 * 10**7 + 8_000_036            # 1251 units of 6400 nonces, 1024 waves
    assert kinds_of(m, lo, hi) == {_lib.HM_KIND_TILED}
    _all_of(ctx, m, lo, hi, {_lib.HM_OPT_GRID_PER_CU: 1})
    lo, hi = 10**6, 10**6 + 64 * 10_000                  # 640001 nonces
    assert kinds_of(m, lo, hi, True) == {_lib.HM_KIND_GENERIC}
    _all_of(ctx, m, lo, hi, {_lib.HM_OPT_FORCE_GENERIC: 1})
    _all_of(ctx, m, lo, lo + 64, {_lib.HM_OPT_FORCE_GENERIC: 1})


# ---- c. self-consistency at 2^30 nonces -------------------------------------

@pytest.mark.gpu
def test_self_consistency_2_30(ctx):
    m, lo, hi = b"bradfitz", 0, 2**30 - 1
    T, cap = 2**64 // 2**16, 2**15   # 16384 hits expected, the buffer twice that
    total = ctx.count(m, lo, hi, T)
    assert ctx.collect_stats()["nonces"] == 2**30
    print(f"count([0, 2^30), 2^64 / 2^16) = {total}")
    assert total <= cap, (total, cap)                    # fails, never skips
    shards = _lib.partition(m, lo, hi, 3)
    assert sum(ctx.count(m, a, b, T) for a, b in shards) == total
    got, recs = ctx.collect(m, lo, hi, T, cap)
    assert got == total == len(recs)
    assert all(a[1] < b[1] for a, b in zip(recs, recs[1:]))
    assert all(h < T and _lib.host_hash(m, n) == h for h, n in recs)
    best = ctx.scan(m, lo, hi)
    got, recs = ctx.collect(m, lo, hi, best[0] + 1, 64)
    assert got == len(recs) >= 1 and min(recs) == best, (best, recs)
    dense = ctx.count(m, lo, hi, MAX)
    assert 2**30 - 1 <= dense <= 2**30, dense


# ---- d. buffer growth and reuse ---------------------------------------------

@pytest.mark.gpu
def test_buffer_growth_and_reuse(oracle_mod):
    """cap 0, 16, 2^16 and 16 again on one fresh context: the device buffer
    is made, grown and reused; hm_scan and hm_find answer as before and their
    stats still describe them."""
    m, lo, hi, T = b"bradfitz", 0, 10**7, 2**64 // 10**6
    exp = oracle_loop(oracle_mod, m, lo, hi, T, threads=0)
    k = len(exp)
    assert 2 <= k <= 16 and exp[0] == (7182149750005, 2351907)
    lib = _lib.load()
    with _lib.Context([0]) as c:
        st = _lib.hm_collect_stats()
        assert lib.hm_collect_stats_sized(c._h, ctypes.byref(st), ctypes.sizeof(st)) == \
            _lib.HM_ERR_INVALID                       # no collect yet
        scan0 = c.scan(m, lo, hi)
        find0 = c.find(m, lo, hi, T)
        assert find0 == exp[0]
        s0, f0 = c.stats(), c.find_stats()
        assert c.collect(m, lo, hi, T, 0) == (k, None) and c.collect_stats()["overflow"] == 1
        for cap in (16, 2**16, 16):
            assert c.collect(m, lo, hi, T, cap) == (k, exp), cap
            cs = c.collect_stats()
            assert (cs["total"], cs["overflow"], cs["nonces"], cs["ndev"]) == (k, 0, hi - lo + 1, 1)
            assert cs["launches"] >= 1 and cs["kernel_ms"] > 0 and cs["wall_ms"] > 0
        # the overflow contract through the C call: out untouched, out[k] untouched
        buf = (_lib.hm_result * (k + 1))()
        for cap in (k - 1, k):
            for r in buf:
                r.hash, r.nonce = SENTINEL
            total = ctypes.c_uint64(777)
            assert lib.hm_collect(c._h, m, len(m), lo, hi, T, buf, cap, ctypes.byref(total)) == 0
            got = [(int(r.hash), int(r.nonce)) for r in buf]
            assert total.value == k
            assert got == ([SENTINEL] * (k + 1) if cap < k else exp + [SENTINEL]), cap
        # invalid arguments leave the outputs alone
        total = ctypes.c_uint64(777)
        tp = ctypes.byref(total)
        assert [lib.hm_collect(c._h, m, len(m), lo, hi, T, None, 4, tp),
                lib.hm_collect(c._h, m, len(m), lo, hi, T, buf, CAP_MAX + 1, tp),
                lib.hm_collect(c._h, None, 3, lo, hi, T, buf, 4, tp),
                lib.hm_collect(c._h, m, len(m), lo, hi, T, buf, 4, None)] == [_lib.HM_ERR_INVALID] * 4
        assert total.value == 777 and (int(buf[k].hash), int(buf[k].nonce)) == SENTINEL
        assert c.collect(m, 5, 4, MAX, 4) == (0, []) and c.collect(m, lo, hi, 0, 4) == (0, [])
        # collect left the scan's and the find's stats alone
        s1, f1 = c.stats(), c.find_stats()
        assert s1 == s0 and f1 == f0
        assert c.scan(m, lo, hi) == scan0 and c.find(m, lo, hi, T) == find0
        assert c.stats()["nonces"] == hi - lo + 1 and c.find_stats()["found"] == 1


# ---- e. the top nonce -------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("how", ["fast", "generic", "two_devices"])
def test_top_nonce_is_an_ordinary_record(ctx, multi, oracle_mod, how):
    m, h = top_nonce_case()
    assert oracle_mod.c_hash(m, MAX) == h
    lo = MAX - TOP_CLEAR
    assert oracle_loop(oracle_mod, m, lo, MAX, h + 1, threads=0) == [(h, MAX)]
    opts = {_lib.HM_OPT_FORCE_GENERIC: 1 if how == "generic" else 0}
    c = multi[2] if how == "two_devices" else ctx
    for a in (lo, MAX):
        got, st = collect_with(c, opts, m, a, MAX, h + 1, 4)
        assert got == (1, [(h, MAX)]), (how, a, got)
        assert st["nonces"] == MAX - a + 1
        got, st = collect_with(c, opts, m, a, MAX, h, 4)
        assert got == (0, []), (how, a, got)
    lower = lo - 1
    hl = oracle_mod.c_hash(m, lower)
    got, _ = collect_with(c, opts, m, lower, MAX, h + 1, 2)
    assert got == (2, [(hl, lower), (h, MAX)]), (how, got)


# ---- f. the deadline --------------------------------------------------------

@pytest.mark.gpu
def test_deadline_expires_inside_a_collect():
    """As test_gpu_find_paths.test_deadline_expires_inside_a_find: a 1-ms
    deadline on the [10^9, 2 * 10^9) request returns HM_ERR_TIMEOUT, leaves
    `out` and `*total` as the caller set them, and abandons the context."""
    import time
    lib = _lib.load()
    c = _lib.Context([0])
    assert c.count(b"bradfitz", 0, 9999, 1419516646206828 + 1) == 1
    c.set_option(_lib.HM_OPT_DEADLINE_MS, 1)
    buf = (_lib.hm_result * 4)()
    buf[0].hash, buf[0].nonce = SENTINEL
    total = ctypes.c_uint64(777)
    t = time.perf_counter()
    rc = lib.hm_collect(c._h, b"bradfitz", 8, 10**9, 2 * 10**9 - 1, 1, buf, 4, ctypes.byref(total))
    assert time.perf_counter() - t < 1.0
    assert rc == _lib.HM_ERR_TIMEOUT
    t = time.perf_counter()
    rc = lib.hm_collect(c._h, b"bradfitz", 8, 0, 9, MAX, buf, 4, ctypes.byref(total))
    assert rc == _lib.HM_ERR_TIMEOUT and time.perf_counter() - t < 0.05
    assert total.value == 777 and (int(buf[0].hash), int(buf[0].nonce)) == SENTINEL
    t = time.perf_counter()
    c.close()  # host memory only
    assert time.perf_counter() - t < 0.05
    with _lib.Context([0]) as c2:
        assert c2.collect(b"bradfitz", 0, 9999, 1419516646206828 + 1, 2) == \
            (1, [(1419516646206828, 9898)])

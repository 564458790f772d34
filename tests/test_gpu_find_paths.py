"""hm_find (ABI 1.10) against an independent CPU oracle of the question itself
(oracle.c_find: a plain ascending "first nonce whose hash is below the target"
loop over the oracle's own SHA-256 and formatting -- the proof-of-work form of
cmu440/bitcoin/miner/miner.go:46-59 over hash.go:13-17), on the host paths
tests/test_gpu_find.py does not reach:

  a. a seeded differential sweep over messages, ranges, target edges, dense
     targets, the options find honours or inherits, and 1-3 "devices";
  b. multi-device pieces: ranges across a multiple of ndev * 2^40 nonces;
  c. nonce 2^64-1 as the only hit (the one the stop word cannot carry);
  d. more launches than the lookahead window in one segment;
  e. a K+W table capped mid-call (smaller tables, more epochs);
  f. a deadline expiring inside a find.

hm_find has no coverage checksum; on a miss nothing may be skipped, so
tasks_run == tasks_total and nonces_enqueued == hi - lo + 1 stand in for one.
"""
import ctypes
import random
import time

import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_find_host import TOP_CLEAR, top_nonce_case
from tests.test_gpu_soak import _case

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1

DEFAULTS = {_lib.HM_OPT_FORCE_GENERIC: 0, _lib.HM_OPT_GRID_PER_CU: 0, _lib.HM_OPT_QUEUE_BATCH: 0,
            _lib.HM_OPT_DEADLINE_MS: 0, _lib.HM_OPT_TABLE_DIGITS: 0,
            _lib.HM_OPT_TABLE_ROWS_CAP: 0}
OPT_NAMES = {_lib.HM_OPT_FORCE_GENERIC: "generic", _lib.HM_OPT_GRID_PER_CU: "grid_per_cu",
             _lib.HM_OPT_QUEUE_BATCH: "queue_batch", _lib.HM_OPT_DEADLINE_MS: "deadline_ms",
             _lib.HM_OPT_TABLE_DIGITS: "table_digits", _lib.HM_OPT_TABLE_ROWS_CAP: "rows_cap"}


def find_with(c, opts, m, lo, hi, T):
    """(answer, find stats) of one find under `opts`, which are restored."""
    try:
        for o, v in opts.items():
            c.set_option(o, v)
        got = c.find(m, lo, hi, T)
        return got, c.find_stats()
    finally:
        for o in opts:
            c.set_option(o, DEFAULTS[o])


def check_stats(st, got, lo, hi, tag):
    """On a miss nothing was skipped; on a hit something ran."""
    if got is None:
        assert st["found"] == 0, (tag, st)
        assert st["tasks_run"] == st["tasks_total"], (tag, st)
        assert st["nonces_enqueued"] == hi - lo + 1, (tag, st)
    else:
        assert st["found"] == 1, (tag, st)
        assert 0 < st["tasks_run"] <= st["tasks_total"], (tag, st)


# ---- a. the randomised differential sweep -----------------------------------

SWEEP_SEED = 1
SWEEP_CASES = 150
EPOCH_CASES = 10
SPAN_CAP = 300_000
LANE_CHUNK = 64 * 10**5  # one wave's lanes x 10^5 final-block values


def _chained_case(rng):
    """test_gpu_soak._epoch_case's shape -- a two-block tail with f = 5
    final-block digits -- over most of ONE lane chunk of 64 * 10^5 nonces (as
    test_gpu_find.test_chained_with_epochs), which the CPU oracle can rescan:
    the planner takes the chained layout only where its lanes are well
    filled, so candidates are drawn until it does."""
    for _ in range(64):
        L = rng.choice([58, 59, 60, 122, 123, 124])
        m = bytes(rng.randrange(256) for _ in range(L))
        d = 5 + 64 - (L + 1) % 64
        c = rng.randrange(10 ** (d - 1) // LANE_CHUNK + 1, 10**d // LANE_CHUNK - 1)
        lo = c * LANE_CHUNK + rng.randrange(0, 300_000)
        hi = (c + 1) * LANE_CHUNK - 1 - rng.randrange(0, 300_000)
        table = rng.randrange(0, 6)
        seg = _lib.debug_plan(m, lo, hi)
        if len(seg) == 1 and seg[0]["kind"] == _lib.HM_KIND_CHAINED and seg[0]["f"] == 5:
            return m, lo, hi, table
    raise AssertionError("no chained layout in 64 draws")


def _draw_target(rng, oracle_mod, m, lo, hi):
    kind = rng.randrange(16)
    j = rng.randrange(0, hi - lo + 1)
    if kind < 8:
        return ([MAX, 2**63] + [2**64 // 10**k for k in range(1, 7)])[kind]
    if kind < 11:
        return (1, 2**32, 2**32 + 1)[kind - 8]
    if kind < 13:
        return oracle_mod.c_scan(m, lo, hi)[0] + (1 if kind == 11 else 0)
    # hashes[j] + 1: a strict-< boundary at an arbitrary nonce (three draws in
    # sixteen: the answers strictly inside the range come from here)
    return oracle_mod.c_hash(m, lo + j) + 1


def sweep_cases(oracle_mod, seed, n, epochs):
    """The sweep's cases with the oracle's answers: a pure function of the
    seed (no GPU), so the seed can be checked on the host."""
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
        opts = {_lib.HM_OPT_FORCE_GENERIC: rng.choice([0, 1]),
                _lib.HM_OPT_GRID_PER_CU: rng.choice([0, 1, 2]),
                _lib.HM_OPT_QUEUE_BATCH: rng.choice([0, 4, 8, 16, 32]),
                _lib.HM_OPT_DEADLINE_MS: rng.choice([0, -1]),
                _lib.HM_OPT_TABLE_DIGITS: table}
        cases.append({"i": i, "m": m, "lo": lo, "hi": hi, "T": T, "opts": opts,
                      "ndev": rng.choice([1, 1, 2, 3]),
                      "exp": oracle_mod.c_find(m, lo, hi, T)})
    return cases


def sweep_counts(cases):
    """(misses, answers equal to lo, answers strictly inside the range), from
    the oracle's answers alone."""
    miss = sum(c["exp"] is None for c in cases)
    at_lo = sum(c["exp"] is not None and c["exp"][1] == c["lo"] for c in cases)
    inside = sum(c["exp"] is not None and c["lo"] < c["exp"][1] < c["hi"] for c in cases)
    return miss, at_lo, inside


def _run_sweep(ctx, cases):
    with _lib.Context([0, 0]) as c2, _lib.Context([0, 0, 0]) as c3:
        for case in cases:
            c = {1: ctx, 2: c2, 3: c3}[case["ndev"]]
            m, lo, hi, T = case["m"], case["lo"], case["hi"], case["T"]
            tag = {"case": case["i"], "msg_hex": m.hex(), "lo": lo, "hi": hi, "target": T,
                   "ndev": case["ndev"],
                   "opts": {OPT_NAMES[o]: v for o, v in case["opts"].items()}}
            got, st = find_with(c, case["opts"], m, lo, hi, T)
            assert got == case["exp"], (tag, got, case["exp"])
            assert st["ndev"] == case["ndev"], (tag, st)
            check_stats(st, got, lo, hi, tag)


def test_random_sweep(ctx, oracle_mod):
    """150 seeded cases drawn as test_gpu_soak._case draws them (spans capped
    at 3 * 10^5), each with a target from the edges of the target's high
    word, dense targets, the range's minimum (+ 1) and hashes[j] + 1, under
    random generic / grid / queue-batch / deadline options on one, two or
    three "devices": every answer equals the CPU oracle's first hit."""
    cases = sweep_cases(oracle_mod, SWEEP_SEED, SWEEP_CASES, epochs=False)
    miss, at_lo, inside = sweep_counts(cases)
    print(f"sweep seed {SWEEP_SEED}: {miss} misses, {at_lo} at lo, {inside} inside")
    assert miss >= 15 and at_lo >= 15 and inside >= 40, (miss, at_lo, inside)
    _run_sweep(ctx, cases)


def test_random_sweep_chained_epochs(ctx, oracle_mod):
    """Ten further cases on the chained layout (f = 5) under a random
    HM_OPT_TABLE_DIGITS: up to 10^4 epochs whose launches are not ascending in
    their nonces."""
    cases = sweep_cases(oracle_mod, SWEEP_SEED + 1, EPOCH_CASES, epochs=True)
    assert any(c["opts"][_lib.HM_OPT_FORCE_GENERIC] == 0 and
               c["opts"][_lib.HM_OPT_TABLE_DIGITS] in (1, 2, 3, 4) for c in cases)
    _run_sweep(ctx, cases)


# ---- b. piece boundaries on two and three "devices" -------------------------

PIECE_HALF = 70_000


def _piece_boundary(m, ndev, generic):
    """The first multiple of the multi-device piece span, as PieceWalk
    computes it: ndev * 2^40 nonces, rounded down to whole tiles of 10^V
    where the segment is not generic."""
    span = ndev << 40
    seg = _lib.debug_plan(m, span - PIECE_HALF, span + PIECE_HALF, generic)[0]
    if seg["kind"] != _lib.HM_KIND_GENERIC:
        span = span // 10 ** seg["V"] * 10 ** seg["V"]
        again = _lib.debug_plan(m, span - PIECE_HALF, span + PIECE_HALF, generic)
        assert len(again) == 1 and again[0]["V"] == seg["V"] and again[0]["kind"] == seg["kind"]
    assert seg["d"] == 13 and 10**12 + PIECE_HALF < span < 10**13 - PIECE_HALF
    return span


@pytest.mark.parametrize("generic", [0, 1], ids=["fast", "generic"])
@pytest.mark.parametrize("ndev", [2, 3])
def test_piece_boundaries(oracle_mod, ndev, generic):
    """[B - 70000, B + 70000] around the first piece boundary B: a hit only
    reachable in the second piece, a hit in the first piece (the second is
    never issued), and a miss (both pieces run in full); then ranges that
    start exactly at B and end exactly at B - 1."""
    opts = {_lib.HM_OPT_FORCE_GENERIC: generic}
    rng = random.Random(4100 + 10 * ndev + generic)
    kept = []
    for _ in range(16):
        m = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 100)))
        B = _piece_boundary(m, ndev, bool(generic))
        lo, hi = B - PIECE_HALF, B + PIECE_HALF
        first, second = oracle_mod.c_scan(m, lo, B - 1), oracle_mod.c_scan(m, B, hi)
        if second[0] < first[0]:
            kept.append((m, B, first, second))
            if len(kept) == 2:
                break
    assert len(kept) == 2, "fewer than two messages whose second piece holds the minimum"
    with _lib.Context([0] * ndev) as c:
        for m, B, first, second in kept:
            lo, hi = B - PIECE_HALF, B + PIECE_HALF
            tag = (m.hex(), ndev, generic, B)
            # the first piece runs dry, the second is issued
            T = second[0] + 1
            got, st = find_with(c, opts, m, lo, hi, T)
            assert got == oracle_mod.c_find(m, lo, hi, T) == second and got[1] >= B, (tag, got)
            check_stats(st, got, lo, hi, tag)
            assert st["ndev"] == ndev and st["nonces_enqueued"] > B - lo, (tag, st)
            # a hit in the first piece: the second is never issued
            T = first[0] + 1
            got, st = find_with(c, opts, m, lo, hi, T)
            assert got == oracle_mod.c_find(m, lo, hi, T) and got[1] < B, (tag, got)
            check_stats(st, got, lo, hi, tag)
            assert st["nonces_enqueued"] <= B - lo, (tag, st)
            # a miss: both pieces in full
            T = second[0]
            got, st = find_with(c, opts, m, lo, hi, T)
            assert got is None and oracle_mod.c_find(m, lo, hi, T) is None, (tag, got)
            check_stats(st, got, lo, hi, tag)
        # lo exactly B, hi exactly B - 1: one piece each, no empty piece
        m, B = kept[0][0], kept[0][1]
        for lo, hi in ((B, B + PIECE_HALF), (B - PIECE_HALF, B - 1), (B - 1, B), (B, B)):
            best = oracle_mod.c_scan(m, lo, hi)
            for T in (best[0] + 1, best[0], 2**64 // 10**3):
                got, st = find_with(c, opts, m, lo, hi, T)
                assert got == oracle_mod.c_find(m, lo, hi, T), (m.hex(), lo, hi, T, got)
                check_stats(st, got, lo, hi, (m.hex(), lo, hi, T))
            assert find_with(c, opts, m, lo, hi, best[0] + 1)[0] == best


# ---- c. the top nonce -------------------------------------------------------

@pytest.mark.parametrize("how", ["fast", "generic", "two_devices"])
def test_top_nonce_is_the_only_hit(ctx, oracle_mod, how):
    """Nonce 2^64-1 never crosses in the stop word: the host tests it.  A
    message whose hash there is so low that the 4454 nonces below it all hash
    at or above it; one nonce further down hashes lower."""
    m, h = top_nonce_case()
    assert oracle_mod.c_hash(m, MAX) == h
    assert oracle_mod.c_scan(m, MAX - TOP_CLEAR, MAX - 1)[0] >= h
    lower = MAX - TOP_CLEAR - 1
    hl = oracle_mod.c_hash(m, lower)
    assert hl < h
    opts = {_lib.HM_OPT_FORCE_GENERIC: 1 if how == "generic" else 0}
    c = _lib.Context([0, 0]) if how == "two_devices" else ctx
    try:
        for lo in (MAX, MAX - TOP_CLEAR):
            got, st = find_with(c, opts, m, lo, MAX, h + 1)
            assert got == (h, MAX) == oracle_mod.c_find(m, lo, MAX, h + 1), (how, lo, got)
            check_stats(st, got, lo, MAX, (how, lo))
            got, st = find_with(c, opts, m, lo, MAX, h)
            assert got is None and oracle_mod.c_find(m, lo, MAX, h) is None, (how, lo, got)
            check_stats(st, got, lo, MAX, (how, lo))
        for T in (h + 1, h):
            got, st = find_with(c, opts, m, lower, MAX, T)
            assert got == (hl, lower) == oracle_mod.c_find(m, lower, MAX, T), (how, T, got)
            check_stats(st, got, lower, MAX, (how, T))
    finally:
        if c is not ctx:
            c.close()


# ---- d. more launches than the lookahead in one segment ---------------------

def test_two_windows_of_generic_launches(ctx):
    """Forced generic, [10^9, 10^9 + 5 * 2^30]: six launches of 2^30 nonces in
    one segment, so the lookahead window (4) is collected and refilled and the
    generic cursor advances.  The CPU cannot rescan 5.4 * 10^9 nonces: the
    reference is ctx.scan on the fast kernels, itself pinned by
    tests/test_gpu_checked.py (test_checked_min_equals_scan and the checked
    layout and full-size tests)."""
    m, lo, hi = b"bradfitz", 10**9, 10**9 + 5 * 2**30
    generic = {_lib.HM_OPT_FORCE_GENERIC: 1}
    best = ctx.scan(m, lo, hi)
    assert lo <= best[1] <= hi and _lib.host_hash(m, best[1]) == best[0]
    t0 = time.perf_counter()
    got, st = find_with(ctx, generic, m, lo, hi, best[0])
    t1 = time.perf_counter()
    assert got is None, got
    assert st["launches"] == 6, st
    check_stats(st, got, lo, hi, "miss")
    assert st["nonces_enqueued"] == 5 * 2**30 + 1
    got, st = find_with(ctx, generic, m, lo, hi, best[0] + 1)
    t2 = time.perf_counter()
    assert got == best, (got, best)
    check_stats(st, got, lo, hi, "min + 1")
    got, st = find_with(ctx, generic, m, lo, hi, 2**64 // 10**3)
    assert got is not None and st["launches"] <= 4, (got, st)
    assert got == ctx.find(m, lo, hi, 2**64 // 10**3)
    check_stats(st, got, lo, hi, "early")
    print(f"generic find over 5 * 2^30 nonces: miss {t1 - t0:.2f} s, min + 1 {t2 - t1:.2f} s")


# ---- e. the table cap -------------------------------------------------------

OPEN_TABLE_DIGITS = 4  # hm_open makes every stream a K+W table of 10^4 rows


def test_table_rows_cap_mid_call(oracle_mod):
    """A device that refuses to grow its K+W table beyond 10^4, then 10^2,
    rows: the segment is planned with fe = 5 (10^5 rows), SegWalk::open's
    chained_table shrinks it mid-call to the largest table the device has or
    may make -- 10^4 rows under either cap, the table hm_open made -- and the
    find runs 10^(5 - fe) epochs over the same tiles.  (Tables below 10^4
    rows: HM_OPT_TABLE_DIGITS in the sweep above and in
    test_gpu_find.test_chained_with_epochs.)"""
    m = b"x" * 56
    rng = random.Random(56)
    a = 10**11 + rng.randrange(0, 300_000)
    b = 10**11 + LANE_CHUNK - 1 - rng.randrange(0, 300_000)
    seg = _lib.debug_plan(m, a, b)[0]
    assert seg["kind"] == _lib.HM_KIND_CHAINED and seg["f"] == 5 and seg["fe"] == 5, seg
    best = oracle_mod.c_scan(m, a, b)
    targets = (best[0] + 1, best[0], 2**64 // 10**5)
    exp = [oracle_mod.c_find(m, a, b, T) for T in targets]
    assert exp[0] == best and exp[1] is None and exp[2] is not None
    with _lib.Context([0]) as c:
        for cap_digits in (4, 2):
            fe = max(cap_digits, OPEN_TABLE_DIGITS)
            opts = {_lib.HM_OPT_TABLE_ROWS_CAP: 10**cap_digits}
            for T, want in zip(targets, exp):
                got, st = find_with(c, opts, m, a, b, T)
                assert got == want, (cap_digits, T, got)
                check_stats(st, got, a, b, (cap_digits, T))
                if got is None:
                    assert st["launches"] >= 10 ** (5 - fe) > 1, st
        # without the cap the planned table is made: one epoch
        got, st = find_with(c, {}, m, a, b, targets[1])
        assert got is None and st["launches"] < 10, st
        check_stats(st, got, a, b, "uncapped")


# ---- f. the deadline --------------------------------------------------------

def test_deadline_expires_inside_a_find():
    """As test_gpu_deadline.test_deadline_timeout_abandons_the_context, for
    hm_find: a 1-ms deadline on the [10^9, 2 * 10^9) request with a target
    nothing meets returns HM_ERR_TIMEOUT, leaves `out` and `found` as the
    caller set them, and abandons the context."""
    lib = _lib.load()
    c = _lib.Context([0])
    assert c.find(b"bradfitz", 0, 10**7, 2**64 // 10**5) == (158752571039048, 91989)
    c.set_option(_lib.HM_OPT_DEADLINE_MS, 1)
    out, found = _lib.hm_result(123, 456), ctypes.c_int(77)
    t = time.perf_counter()
    rc = lib.hm_find(c._h, b"bradfitz", 8, 10**9, 2 * 10**9 - 1, 1, ctypes.byref(out),
                     ctypes.byref(found))
    assert time.perf_counter() - t < 1.0
    assert rc == _lib.HM_ERR_TIMEOUT
    assert (int(out.hash), int(out.nonce), found.value) == (123, 456, 77)
    t = time.perf_counter()
    rc = lib.hm_find(c._h, b"bradfitz", 8, 0, 9, MAX, ctypes.byref(out), ctypes.byref(found))
    assert rc == _lib.HM_ERR_TIMEOUT and time.perf_counter() - t < 0.05
    assert (int(out.hash), int(out.nonce), found.value) == (123, 456, 77)
    t = time.perf_counter()
    c.close()  # host memory only
    assert time.perf_counter() - t < 0.05
    with _lib.Context([0]) as c2:
        assert c2.find(b"bradfitz", 0, 10**7, 2**64 // 10**3) == (6697378768932333, 203)
        assert c2.find_stats()["found"] == 1

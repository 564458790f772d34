"""hm_collect_many on the paths tests/test_gpu_collect_many.py does not reach
(tests/test_collect_many_paths_host.py builds the lists, shows what they reach,
and shows that the comparison helpers used here reject corrupted answers):

  1. launches of several wave rounds on every kernel instantiation: whole tasks
     dequeued from the counter, the segment search over many ids, the tiled,
     chained and generic decoders at large task numbers;
  2. HM_OPT_FUSED_PARTS x HM_OPT_FUSED_TAIL on the collect kernel, over several
     rounds and on windows where every id is a piece;
  3. overflow inside the kernel (caps of 1, 63, 64, 65 under dense steps, stale
     records and tags afterwards) and across the host's steps: a later chunk, a
     fallback, one of two streams, one of two devices;
  4. a batch of mixed sizes and targets, on 1 and 4 streams and 2 and 3 devices;
  5. the deadline around the call, and the abandoned context;
  6. host threads, on contexts of their own and on a shared one.

Every comparison is exact, the reference is the CPU oracle (hm_collect on the
same request is a second witness in 1), and every case asserts through
hm_collect_many_stats which path it took."""
import threading
import time

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_collect_many_paths_host as H
from tests import test_find_many_paths_host as F
from tests import test_gpu_collect_many as M
from tests.test_collect_layouts_host import parts
from tests.test_collect_many_host import SENTINEL, expected, many_raw
from tests.test_gpu_collect import collect_np
from tests.test_gpu_collect_layouts import scan_sum
from tests.test_gpu_collect_many import all_fused, gpu_many, many_np, small_requests
from tests.test_gpu_find_many_paths import cus, expected_ids  # noqa: F401  (cus: a fixture)
from tests.test_gpu_verify import multi  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
MAX = (1 << 64) - 1
UNTOUCHED = (SENTINEL, SENTINEL)
DEFAULTS = {**M.options.DEFAULTS, _lib.HM_OPT_GRID_PER_CU: 0, _lib.HM_OPT_FUSED_PARTS: 1,
            _lib.HM_OPT_DEADLINE_MS: 0}


class options(M.options):
    DEFAULTS = DEFAULTS


@pytest.fixture(scope="module")
def primed(oracle_mod):
    """The oracle's answers for the multi-round list, once, ahead of the items
    that use them: an item's own time is then the GPU's and the comparison's."""
    H.prime(oracle_mod)


def run(c, reqs, cap):
    """(total, totals, records or None, stats) of one call."""
    total, totals, recs = many_np(c, reqs, cap)
    return total, totals, recs, c.collect_many_stats()


def case_opts(c):
    return {_lib.HM_OPT_GRID_PER_CU: 1, _lib.HM_OPT_FORCE_GENERIC: int(c["generic"])}


def count_dense(ctx, c, tag):
    """The case's window as a count at T = 2^64 - 1: every nonce once."""
    span = H.span_of(c)
    total, totals, _, st = run(ctx, [(c["m"], c["lo"], c["hi"], MAX)], 0)
    assert total == span and totals == [span], (tag, total, st)
    assert st["nonces"] == span and st["total"] == span, (tag, st)
    assert st["requests"] == st["fused"] == st["launches"] == 1 and st["fallback"] == 0, (tag, st)
    assert st["overflow"] == 1, (tag, st)
    return st


def records_dense(ctx, oracle_mod, c, tag):
    """A small case's window with a buffer of span records at T = 2^64 - 1."""
    span = H.span_of(c)
    total, totals, recs, st = run(ctx, [(c["m"], c["lo"], c["hi"], MAX)], span)
    assert total == span and totals == [span] and st["overflow"] == 0, (tag, total, st)
    assert st["fused"] == st["launches"] == 1 and st["fallback"] == 0, (tag, st)
    H.check_dense(recs[0], c["lo"], c["hi"], H.window_sum(oracle_mod, c), tag,
                  sub=(H.mid_target(c), H.mid_list(oracle_mod, c)))
    return st


def records_mid(ctx, oracle_mod, c, tag):
    """The case's window at its mid target: the oracle's list, bit for bit."""
    want = H.mid_list(oracle_mod, c)
    total, totals, recs, st = run(ctx, [(c["m"], c["lo"], c["hi"], H.mid_target(c))], len(want) + 64)
    assert total == len(want) and totals == [len(want)], (tag, total, len(want), st)
    assert st["fused"] == st["launches"] == 1 and st["fallback"] == 0, (tag, st)
    assert st["nonces"] == H.span_of(c) and st["overflow"] == 0, (tag, st)
    H.check_list(recs[0], want, tag)
    return st


# ---- 1. several rounds on every layout key ----------------------------------

@pytest.mark.parametrize("part", range(F.LIST_ITEMS))
def test_several_rounds_every_kernel(ctx, oracle_mod, primed, cus, part):  # noqa: F811
    cases = parts(F.multi_round_cases(), F.LIST_ITEMS)[part]
    assert cases
    for c in cases:
        tag = f"{c['name']} L={c['L']} lo={c['lo']} hi={c['hi']} msg_hex={c['m'].hex()}"
        with options(ctx, case_opts(c)):
            st = count_dense(ctx, c, tag)
            # three rounds on THIS device, or the list is too small for it
            assert st["tasks"] >= F.ROUNDS * 4 * cus, (tag, st)
            if H.is_small(c):
                assert records_dense(ctx, oracle_mod, c, tag)["tasks"] == st["tasks"], tag
            assert records_mid(ctx, oracle_mod, c, tag)["tasks"] == st["tasks"], tag
            # hm_collect on the same request: a second witness
            want = H.mid_list(oracle_mod, c)
            n, hashes, nonces = collect_np(ctx, c["m"], c["lo"], c["hi"], H.mid_target(c),
                                           len(want) + 64)
            assert n == len(want), (tag, n, len(want))
            H.check_list(np.stack([hashes, nonces], axis=1), want, tag)


# ---- 2. the split options ----------------------------------------------------

@pytest.mark.parametrize("tail", [1, 5, 10])
@pytest.mark.parametrize("nparts", [2, 5, 10])
def test_split_options_over_several_rounds(ctx, oracle_mod, primed, cus, nparts, tail):  # noqa: F811
    """The subset's multi-round windows under every PARTS x TAIL: the same
    count, dense records and mid list; the ids are those of the TAIL = 1 run
    with its last tasks split."""
    differ = []
    for what, c in F.split_subset().items():
        tag = f"{what} {c['name']} PARTS={nparts} TAIL={tail}"
        with options(ctx, {**case_opts(c), _lib.HM_OPT_FUSED_PARTS: nparts,
                           _lib.HM_OPT_FUSED_TAIL: 1}):
            st1 = count_dense(ctx, c, tag)
            assert st1["tasks"] >= F.ROUNDS * 4 * cus, (tag, st1)
            ctx.set_option(_lib.HM_OPT_FUSED_TAIL, tail)
            want_ids = expected_ids(st1["tasks"], 4 * cus, tail)
            assert count_dense(ctx, c, tag)["tasks"] == want_ids, (tag, st1)
            if H.is_small(c):
                assert records_dense(ctx, oracle_mod, c, tag)["tasks"] == want_ids, tag
            assert records_mid(ctx, oracle_mod, c, tag)["tasks"] == want_ids, tag
            differ.append(want_ids != st1["tasks"])
    print(f"PARTS {nparts} TAIL {tail}: {sum(differ)} of {len(differ)} launches have pieces")
    if tail > 1:
        assert any(differ)      # some launch ended on a partial round and was split


def piece_run(ctx, oracle_mod, c, cap, tag):
    lo, hi = F.piece_window(c)
    total, totals, recs, st = run(ctx, [(c["m"], lo, hi, MAX)], cap)
    assert total == 20_000 and totals == [20_000], (tag, total, st)
    assert st["fused"] == st["launches"] == 1 and st["fallback"] == 0 and st["nonces"] == 20_000, \
        (tag, st)
    if cap >= 20_000:
        assert st["overflow"] == 0, (tag, st)
        H.check_window(recs[0], lo, H.window_hashes(oracle_mod, c), tag)
    return st


@pytest.mark.parametrize("nparts", [2, 5, 10])
def test_split_options_every_id_a_piece(ctx, oracle_mod, nparts):
    """Windows of 2 * 10^4 nonces at HM_OPT_GRID_PER_CU = 16: fewer tasks than a
    tenth of a round, so every task runs as HM_OPT_FUSED_TAIL pieces.  Dense,
    with a buffer of 20 000 records: every nonce once, every hash the oracle's."""
    for what, c in F.split_subset().items():
        opts = {_lib.HM_OPT_GRID_PER_CU: F.SPLIT_GRID, _lib.HM_OPT_FUSED_PARTS: nparts,
                _lib.HM_OPT_FORCE_GENERIC: int(c["generic"]), _lib.HM_OPT_FUSED_TAIL: 1}
        with options(ctx, opts):
            st1 = piece_run(ctx, oracle_mod, c, 20_000, (what, nparts, 1))
            assert st1["tasks"] > 0
            for tail in (2, 5, 10):
                ctx.set_option(_lib.HM_OPT_FUSED_TAIL, tail)
                st = piece_run(ctx, oracle_mod, c, 20_000, (what, c["name"], nparts, tail))
                assert st["tasks"] == tail * st1["tasks"], (what, nparts, tail, st, st1)


# ---- 3. overflow ------------------------------------------------------------

def overflowed(c, reqs, cap, per, tag=""):
    """An overflowed call through many_raw: HM_OK, every total and *total
    exact, `out` still all sentinels, the guards intact, overflow = 1."""
    rc, t, totals, got, intact = many_raw(gpu_many(c), reqs, cap)
    assert rc == _lib.HM_OK and intact, (tag, rc, intact)
    H.check_totals(t, totals, per, tag)
    assert t > cap and len(got) == cap and all(x == UNTOUCHED for x in got), (tag, cap, t)
    st = c.collect_many_stats()
    assert st["overflow"] == 1 and st["total"] == t and st["requests"] == len(reqs), (tag, st)
    return st


@pytest.mark.parametrize("what", list(F.split_subset()))
def test_caps_around_a_step(ctx, oracle_mod, what):
    """A dense window under caps of 1, 63, 64, 65 (a step's 64 hits straddle the
    cap, or begin at it) and 19 999; then cap 20 000 on the same context, over
    the stale records and tags and the re-zeroed cursor: every record exact."""
    c = F.split_subset()[what]
    lo, hi = F.piece_window(c)
    reqs = [(c["m"], lo, hi, MAX)]
    with options(ctx, {_lib.HM_OPT_FORCE_GENERIC: int(c["generic"])}):
        for cap in (1, 63, 64, 65, 19_999):
            st = overflowed(ctx, reqs, cap, [20_000], (what, cap))
            assert all_fused(st, reqs) and st["nonces"] == 20_000, (what, cap, st)
        piece_run(ctx, oracle_mod, c, 20_000, (what, "after the overflows"))
        # and a guarded buffer of exactly the total: nothing beyond it is written
        rc, t, totals, got, intact = many_raw(gpu_many(ctx), reqs, 20_000)
        assert (rc, t, totals) == (_lib.HM_OK, 20_000, [20_000]) and intact
        H.check_window(H.as_array(got), lo, H.window_hashes(oracle_mod, c), what)


@pytest.mark.parametrize("streams", [2, 4])
def test_two_dense_requests_share_one_cap(ctx, oracle_mod, streams):
    """Two dense windows on different streams reserve on the one cursor: a cap
    below either's count, one between a count and the sum, and the sum."""
    sub = F.split_subset()
    a, b = sub["plain"], sub["chained1"]
    reqs = [(c["m"], *F.piece_window(c), MAX) for c in (a, b)]
    with options(ctx, {_lib.HM_OPT_STREAMS: streams}):
        for cap in (15_000, 30_000, 39_999):
            st = overflowed(ctx, reqs, cap, [20_000, 20_000], (streams, cap))
            assert all_fused(st, reqs), st
        total, totals, recs, st = run(ctx, reqs, 40_000)
        assert total == 40_000 and totals == [20_000, 20_000] and st["overflow"] == 0, st
        assert all_fused(st, reqs), st
        for c, got in zip((a, b), recs):
            H.check_window(got, F.piece_window(c)[0], H.window_hashes(oracle_mod, c), streams)


def test_overflow_in_a_later_chunk(ctx, oracle_mod):
    """130 requests, three chunks: the records of the first chunk (of the first
    two) fit the cap exactly, so the overflow is first reached in the second
    (third) chunk, after the earlier ones were read back.  A cap of exactly the
    total fits and returns every record; cap 0 gives the pure counts."""
    reqs, (total, per, recs) = H.overflow_requests(oracle_mod)
    for cap in (sum(per[:64]), sum(per[:128]), total - 1):
        st = overflowed(ctx, reqs, cap, per, cap)
        assert all_fused(st, reqs), st
    assert ctx.collect_many(reqs, total) == (total, per, recs)
    st = ctx.collect_many_stats()
    assert all_fused(st, reqs) and st["overflow"] == 0 and st["total"] == total, st
    rc, t, totals, got, intact = many_raw(gpu_many(ctx), reqs, 0)
    assert (rc, got) == (_lib.HM_OK, []) and intact
    H.check_totals(t, totals, per)
    assert ctx.collect_many_stats()["overflow"] == 1


def test_overflow_reached_by_a_fallback(ctx, oracle_mod):
    """HM_OPT_COLLECT_WINDOW = 1000: the chunk's fused records fit the cap
    exactly; the first fallback request then overflows it."""
    reqs, (total, per, recs), fused = H.window_requests(oracle_mod)
    nfall = len(reqs) - len(fused)
    with options(ctx, {_lib.HM_OPT_COLLECT_WINDOW: H.WINDOW}):
        for cap in (sum(per[i] for i in fused), total - 1):
            st = overflowed(ctx, reqs, cap, per, cap)
            assert st["fused"] == len(fused) > 0 and st["fallback"] == nfall > 0, st
        assert ctx.collect_many(reqs, total) == (total, per, recs)
        st = ctx.collect_many_stats()
        assert (st["fused"], st["fallback"], st["overflow"]) == (len(fused), nfall, 0), st


def test_one_device_over_the_cap(multi, oracle_mod):  # noqa: F811
    """Two devices, request r on device r mod 2: the even requests dense, so
    device 0's records exceed the cap while device 1's fit; the mirror; and a
    cap of the exact total."""
    c = multi[2]
    base = small_requests(54, 8)
    for dense_on in (0, 1):
        reqs = [(m, lo, hi, MAX if i % 2 == dense_on else T) for i, (m, lo, hi, T) in enumerate(base)]
        total, per, recs = expected(oracle_mod, reqs)
        heavy = sum(per[dense_on::2])
        light = total - heavy
        cap = (heavy + light) // 2
        assert light < cap < heavy, (per, cap)
        st = overflowed(c, reqs, cap, per, (dense_on, cap))
        assert st["ndev"] == 2 and all_fused(st, reqs), st
        assert c.collect_many(reqs, total) == (total, per, recs)
        st = c.collect_many_stats()
        assert st["ndev"] == 2 and all_fused(st, reqs) and st["overflow"] == 0, st
        overflowed(c, reqs, total - 1, per, (dense_on, total - 1))


# ---- 4. the mixed batch ------------------------------------------------------

def check_mixed(oracle_mod, c, tag):
    mix = H.mixed_batch(oracle_mod)
    ans = H.mixed_answers(oracle_mod)
    reqs = [r for _, r in mix]
    per = [H.answer_total(a) for a in ans]
    total, totals, recs, st = run(c, reqs, sum(per))
    H.check_totals(total, totals, per, tag)
    assert recs is not None and st["overflow"] == 0 and st["total"] == sum(per), (tag, st)
    for i, ((_, (m, lo, hi, T)), (how, want), got) in enumerate(zip(mix, ans, recs)):
        t = f"{tag} request {i} lo={lo} hi={hi} T={T} msg_hex={m.hex()}"
        if how == "dense":
            H.check_dense(got, lo, hi, want, t)
        else:
            H.check_list(got, want, t)
    return reqs, st


@pytest.mark.parametrize("how", ["streams1", "streams4", "dev2", "dev3"])
def test_mixed_batch(ctx, multi, oracle_mod, how):  # noqa: F811
    """About 40 requests of 1 .. 2^22 nonces, dense, 1/8, 1/1000, no-hit and
    one-record targets, shuffled: multi-round dense launches share the device's
    cursor with many tiny ones on the other streams."""
    c = {"dev2": multi[2], "dev3": multi[3]}.get(how, ctx)
    with options(c, {_lib.HM_OPT_STREAMS: 1 if how == "streams1" else 4}):
        reqs, st = check_mixed(oracle_mod, c, how)
    assert all_fused(st, reqs) and st["ndev"] == {"dev2": 2, "dev3": 3}.get(how, 1), st
    assert st["nonces"] == sum(hi - lo + 1 for _, lo, hi, T in reqs if lo <= hi and T), st


def test_mixed_batch_with_fallbacks(ctx, oracle_mod):
    """HM_OPT_COLLECT_WINDOW = 10^5: the large requests take the per-segment
    path among fused neighbours; the answers stay the same."""
    with options(ctx, {_lib.HM_OPT_COLLECT_WINDOW: 10**5}):
        reqs, st = check_mixed(oracle_mod, ctx, "window 10^5")
    big = sum(hi - lo + 1 > 10**5 for _, lo, hi, T in reqs if lo <= hi and T)
    assert big >= 9 and st["fallback"] == big and st["fused"] == M.live(reqs) - big > 0, st


# ---- 5. the deadline ---------------------------------------------------------

def test_deadline_that_holds_changes_nothing(ctx, oracle_mod):
    """HM_OPT_DEADLINE_MS = -1 (auto) and 60 000 around a batch of fused and
    fallback requests: the answers of deadline 0."""
    reqs, exp, fused = H.window_requests(oracle_mod)
    with options(ctx, {_lib.HM_OPT_COLLECT_WINDOW: H.WINDOW}):
        for ms in (0, -1, 60_000):
            with options(ctx, {_lib.HM_OPT_DEADLINE_MS: ms}):
                assert ctx.collect_many(reqs, exp[0]) == exp, ms
                st = ctx.collect_many_stats()
                assert ctx.count_many(reqs) == exp[1], ms
            assert (st["fused"], st["fallback"]) == (len(fused), len(reqs) - len(fused)), (ms, st)


def test_deadline_expires_inside_the_call():
    """A 1-ms deadline on 64 no-hit requests of 2^27 nonces: HM_ERR_TIMEOUT,
    totals, out and *total as the caller set them, the context abandoned."""
    lib = _lib.load()
    c = _lib.Context([0])
    one = (1419516646206828, 9898)      # the minimum of bradfitz over [0, 9999]
    small = [(b"bradfitz", 0, 9999, one[0] + 1)]
    assert c.collect_many(small, 2) == (1, [1], [[one]])
    c.set_option(_lib.HM_OPT_DEADLINE_MS, 1)
    reqs = [(b"deadline %d" % i, 0, 2**27 - 1, 1) for i in range(64)]
    rc, total, totals, got, intact = many_raw(gpu_many(c), reqs, 4)
    assert rc == _lib.HM_ERR_TIMEOUT and intact
    assert total == 777 and totals == [SENTINEL] * 64 and got == [UNTOUCHED] * 4
    t = time.perf_counter()
    rc, total, totals, got, intact = many_raw(gpu_many(c), small, 2)
    assert rc == _lib.HM_ERR_TIMEOUT and time.perf_counter() - t < 0.05
    assert total == 777 and totals == [SENTINEL] and got == [UNTOUCHED] * 2 and intact
    t = time.perf_counter()
    with pytest.raises(_lib.HipMinerError) as ei:
        c.count_many(small)
    assert ei.value.rc == _lib.HM_ERR_TIMEOUT and time.perf_counter() - t < 0.05
    t = time.perf_counter()
    assert lib.hm_set_option(c._h, _lib.HM_OPT_DEADLINE_MS, 0) == _lib.HM_ERR_TIMEOUT
    assert time.perf_counter() - t < 0.05
    t = time.perf_counter()
    c.close()   # host memory only: the queued work drains on its own
    assert time.perf_counter() - t < 0.05
    with _lib.Context([0]) as c2:
        assert c2.collect_many(small, 2) == (1, [1], [[one]])


# ---- 6. threads --------------------------------------------------------------

def thread_batch(oracle_mod, seed):
    """small_requests plus one dense request of 10^5 nonces, with the answers."""
    def build():
        reqs = small_requests(seed, 20)
        dense = (b"dense %d" % seed, 10**7 - 40_000 - seed, 10**7 + 59_999 - seed, MAX)
        return reqs[:9] + [dense] + reqs[9:], expected(oracle_mod, reqs), \
            scan_sum(oracle_mod, *dense[:3])
    return H.memo(("collect_many_thread_batch", seed), build)


def check_thread_batch(c, batch, tag):
    reqs, (total, per, recs), ssum = batch
    per = per[:9] + [10**5] + per[9:]
    t, totals, got = many_np(c, reqs, total + 10**5)
    H.check_totals(t, totals, per, tag)
    H.check_dense(got[9], reqs[9][1], reqs[9][2], ssum, tag)
    for i, g in enumerate(got[:9] + got[10:]):
        H.check_list(g, H.as_array(recs[i]), (tag, i))


def run_threads(fns):
    errs = []

    def wrap(f):
        try:
            f()
        except BaseException as e:  # noqa: BLE001 -- reported below
            errs.append(e)

    ts = [threading.Thread(target=wrap, args=(f,)) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=240)
    assert not any(t.is_alive() for t in ts), "a collect_many thread hung"
    if errs:
        raise errs[0]


def test_threads_with_contexts_of_their_own(oracle_mod):
    """Two host threads, a context each on GPU 0, different batches, three
    times each: the launches of the two overlap on the device."""
    batches = [thread_batch(oracle_mod, 56 + k) for k in range(2)]

    def worker(k):
        def f():
            with _lib.Context([0]) as c:
                for rep in range(3):
                    check_thread_batch(c, batches[k], (k, rep))
                    assert all_fused(c.collect_many_stats(), batches[k][0])
        return f

    run_threads([worker(k) for k in range(2)])


def test_threads_share_one_context(ctx, oracle_mod):
    """Two host threads on one context: the calls are serialised by its mutex
    and share the device's cursor, record and tag buffers."""
    batches = [thread_batch(oracle_mod, 56 + k) for k in range(2)]

    def worker(k):
        def f():
            for rep in range(3):
                check_thread_batch(ctx, batches[k], (k, rep))
        return f

    run_threads([worker(k) for k in range(2)])
    check_thread_batch(ctx, batches[0], "after the threads")
    assert all_fused(ctx.collect_many_stats(), batches[0][0])

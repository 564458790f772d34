"""hm_cancel (ABI 1.18) on the GPU: a find-family call in flight on one thread is
stopped from another, inside a running launch, and the context stays usable.

Every call here is bounded by its range, so a cancel that does not work makes a
test fail after a second or two and can never hang.  The canceller is a
threading.Thread that sleeps and then calls Context.cancel(); ctypes releases
the GIL while the other thread is inside the library.

The time caps are half of the uncancelled call's time at the rates the README
records for the parent's hm_find (36.70 GH/s on b"bradfitz", 47.99 GH/s on the
120-byte message): a cancel that only took effect between launches could not
meet them, the signal has to arrive inside the launch.  Latencies are printed,
not asserted."""
import ctypes
import random
import threading
import time

import pytest

import bench
from distributed_bitcoinminer_amd import _lib

pytestmark = pytest.mark.gpu

MSG = b"bradfitz"
T_HIT = 2**64 // 10**6            # the first hit of [0, 2^64-1] is nonce 2,351,907
FIRST_HIT = (7182149750005, 2351907)
SCAN_1E7 = (356393768206, 7645578)       # hm_scan(b"bradfitz", [0, 10^7])
SCAN_2_32 = (5256245051, 1626825724)     # golden: hm_scan(b"bradfitz", [0, 2^32))
TILED_S = 6e10 / 36.70e9                 # [10^10, 7*10^10] uncancelled: 1.63 s
CHAINED_S = 6e10 / 47.99e9               # the same on the 120-byte message: 1.25 s
BATCH_S = 8e10 / 36.70e9                 # 8 requests of 10^10 nonces: 2.18 s


@pytest.fixture(scope="module")
def cctx():
    """A context of this module's own: a cancel gone wrong must not take the
    session's context with it."""
    c = _lib.Context([0])
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """The host's answers the survival checks compare with, computed once."""
    k8 = _lib.find_k_cpu(MSG, 0, 2 * 10**7, T_HIT, 8)
    assert len(k8) == 8 and k8[0] == FIRST_HIT == _lib.find_cpu(MSG, 0, 10**7, T_HIT)
    return {"k8": k8, "count": _lib.count_cpu(MSG, 0, 10**7, T_HIT)}


def run_cancelled(ctx, call, delay_s, cancels=1):
    """Run call() with a canceller that sleeps delay_s and then calls
    ctx.cancel() `cancels` times: (the call's result or its HipMinerError, its
    wall time in seconds, what the cancels returned)."""
    got = []

    def canceller():
        if delay_s > 0:
            time.sleep(delay_s)
        for _ in range(cancels):
            got.append(ctx.cancel())

    th = threading.Thread(target=canceller)
    th.start()
    t0 = time.perf_counter()
    try:
        out = call()
    except _lib.HipMinerError as e:
        out = e
    wall = time.perf_counter() - t0
    th.join()
    return out, wall, got


def check_survives(ctx, refs):
    """After a cancelled call the context answers every family exactly, and the
    find record is the later good call's."""
    assert ctx.find(MSG, 0, 2**64 - 1, T_HIT) == FIRST_HIT
    st = ctx.find_stats()
    assert st["found"] == 1 and st["launches"] >= 1, st
    assert ctx.find_k(MSG, 0, 2**64 - 1, T_HIT, 8) == refs["k8"]
    assert ctx.scan(MSG, 0, 10**7) == SCAN_1E7
    assert ctx.count(MSG, 0, 10**7, T_HIT) == refs["count"]


def kind_of(msg, lo, hi):
    plan = _lib.debug_plan(msg, lo, hi)
    assert len(plan) == 1, plan
    return plan[0]["kind"]


def test_cancel_inside_one_tiled_launch(cctx, refs):
    """1. hm_find(b"bradfitz", [10^10, 7*10^10], target 1): one 11-digit tiled
    segment, no hit, 1.63 s uncancelled.  Cancelled after 200 ms it must return
    within 0.8 s, and no stats record of the family moves."""
    assert kind_of(MSG, 10**10, 7 * 10**10) == _lib.HM_KIND_TILED
    assert cctx.find(MSG, 0, 10**7, T_HIT) == FIRST_HIT
    before, cs0 = cctx.find_stats(), cctx.cancel_stats()
    out, wall, got = run_cancelled(cctx, lambda: cctx.find(MSG, 10**10, 7 * 10**10, 1), 0.2)
    cs = cctx.cancel_stats()
    print(f"tiled: wall {wall:.3f} s, cancel_stats {cs}")
    assert got == [True]
    assert isinstance(out, _lib.HipMinerCancelled) and out.rc == _lib.HM_ERR_CANCELLED, out
    assert wall < 0.8 < TILED_S / 2 + 1e-9, wall
    assert cctx.find_stats() == before
    assert cs["cancels"] == cs0["cancels"] + 1
    assert cs["cancelled_calls"] == cs0["cancelled_calls"] + 1
    assert cs["family"] == _lib.HM_CANCEL_FAMILY_FIND and cs["launches_in_flight"] >= 1, cs
    assert 0 < cs["latency_ms"] < 1000 * wall, cs
    check_survives(cctx, refs)


@pytest.mark.parametrize("which", ["find_chained", "find_k_tiled", "find_k_chained"])
def test_cancel_chained_and_find_k(cctx, refs, which):
    """2. The chained kernel (the 120-byte message; it fills every wave slot, so
    only a wave of the launch itself can relay the signal): 1.25 s uncancelled,
    cap 0.6 s.  The same for hm_find_k (k = 64) on both messages."""
    chained = which.endswith("chained")
    msg = bench.long120() if chained else MSG
    lo, hi = 10**10, 7 * 10**10
    assert kind_of(msg, lo, hi) == (_lib.HM_KIND_CHAINED if chained else _lib.HM_KIND_TILED)
    if which.startswith("find_k"):
        call, family = (lambda: cctx.find_k(msg, lo, hi, 1, 64)), _lib.HM_CANCEL_FAMILY_FIND_K
    else:
        call, family = (lambda: cctx.find(msg, lo, hi, 1)), _lib.HM_CANCEL_FAMILY_FIND
    out, wall, got = run_cancelled(cctx, call, 0.2)
    cs = cctx.cancel_stats()
    print(f"{which}: wall {wall:.3f} s, cancel_stats {cs}")
    assert got == [True]
    assert isinstance(out, _lib.HipMinerCancelled), out
    cap = 0.6 if chained else 0.8
    assert wall < cap < (CHAINED_S if chained else TILED_S) / 2 + 1e-9, wall
    assert cs["family"] == family, cs
    check_survives(cctx, refs)


def test_cancel_generic(cctx, refs):
    """3. HM_OPT_FORCE_GENERIC, [0, 2^33], target 1, cancelled after 50 ms.  No
    time cap: the generic rate is not on record."""
    cctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 1)
    try:
        out, wall, got = run_cancelled(cctx, lambda: cctx.find(MSG, 0, 2**33, 1), 0.05)
        outk, wallk, gotk = run_cancelled(cctx, lambda: cctx.find_k(MSG, 0, 2**33, 1, 64), 0.05)
    finally:
        cctx.set_option(_lib.HM_OPT_FORCE_GENERIC, 0)
    print(f"generic: find wall {wall:.3f} s, find_k wall {wallk:.3f} s, "
          f"cancel_stats {cctx.cancel_stats()}")
    assert got == [True] and isinstance(out, _lib.HipMinerCancelled), (got, out)
    assert gotk == [True] and isinstance(outk, _lib.HipMinerCancelled), (gotk, outk)
    check_survives(cctx, refs)


@pytest.mark.parametrize("family", ["find_many", "find_k_many"])
def test_cancel_batches(cctx, refs, family):
    """4. Eight requests of distinct messages over [10^10, 2*10^10], target 1:
    the fused windows, then the leftovers on the per-segment path (2.18 s
    uncancelled).  Cancelled after 100 ms: HM_ERR_CANCELLED within half that
    time, and the caller's output arrays keep their poison."""
    lib = _lib.load()
    n, k = 8, 4
    msgs = [b"cancel-job-%d" % i for i in range(n)]
    if family == "find_many":
        arr, _, keep = _lib._requests(_lib.hm_find_request,
                                      [(m, 10**10, 2 * 10**10, 1) for m in msgs])
        outs, aux = (_lib.hm_result * n)(), (ctypes.c_int * n)()
        entry, fam = lib.hm_find_many, _lib.HM_CANCEL_FAMILY_FIND_MANY
    else:
        arr, _, keep = _lib.find_k_requests([(m, 10**10, 2 * 10**10, 1, k) for m in msgs])
        outs, aux = (_lib.hm_result * (n * k))(), (ctypes.c_size_t * n)()
        entry, fam = lib.hm_find_k_many, _lib.HM_CANCEL_FAMILY_FIND_K_MANY
    ctypes.memset(outs, 0xA5, ctypes.sizeof(outs))
    ctypes.memset(aux, 0xA5, ctypes.sizeof(aux))

    def call():
        rc = entry(cctx._h, arr, n, outs, aux)
        if rc != _lib.HM_OK:
            raise _lib._error(rc, family)
        return rc

    out, wall, got = run_cancelled(cctx, call, 0.1)
    del keep
    cs = cctx.cancel_stats()
    print(f"{family}: wall {wall:.3f} s, cancel_stats {cs}")
    assert got == [True]
    assert isinstance(out, _lib.HipMinerCancelled) and out.rc == _lib.HM_ERR_CANCELLED, out
    assert wall < BATCH_S / 2, wall
    assert bytes(outs) == b"\xA5" * ctypes.sizeof(outs)
    assert bytes(aux) == b"\xA5" * ctypes.sizeof(aux)
    assert cs["family"] == fam, cs
    check_survives(cctx, refs)


def test_no_stickiness(cctx, refs):
    """6. A cancel with nothing cancellable in flight returns False and leaves no
    trace; two cancels on one call give one HipMinerCancelled."""
    assert cctx.cancel() is False
    assert cctx.find(MSG, 0, 10**7, T_HIT) == FIRST_HIT
    # a scan is not cancellable: cancel() says so and the scan is exact
    out, wall, got = run_cancelled(cctx, lambda: cctx.scan(MSG, 0, 2**32 - 1), 0.03)
    assert got == [False] and out == SCAN_2_32, (got, out)
    assert cctx.find(MSG, 0, 10**7, T_HIT) == FIRST_HIT
    # two cancels on one call ([10^10, 3*10^10]: 0.54 s uncancelled)
    cs0 = cctx.cancel_stats()
    out, wall, got = run_cancelled(cctx, lambda: cctx.find(MSG, 10**10, 3 * 10**10, 1), 0.1,
                                   cancels=2)
    assert got[0] is True and got[1] in (True, False), got
    assert isinstance(out, _lib.HipMinerCancelled), out
    assert cctx.cancel_stats()["cancelled_calls"] == cs0["cancelled_calls"] + 1
    assert cctx.cancel() is False
    check_survives(cctx, refs)


def test_race_soak(cctx, refs):
    """7. The forged-word hazard: 40 rounds of hm_find(b"bradfitz", [0, 3*10^8],
    2^64/10^6) and 40 of hm_find_k (k = 8), each with a cancel at a seeded random
    delay in 0-3 ms.  A round ends in HipMinerCancelled or in exactly the
    host's answer -- never another error, never another record -- and both
    outcomes occur."""
    rng = random.Random(118)
    outcomes = {"cancelled": 0, "answered": 0}
    for call, want in ((lambda: cctx.find(MSG, 0, 3 * 10**8, T_HIT), FIRST_HIT),
                       (lambda: cctx.find_k(MSG, 0, 3 * 10**8, T_HIT, 8), refs["k8"])):
        for _ in range(40):
            out, wall, got = run_cancelled(cctx, call, rng.uniform(0.0, 0.003))
            if isinstance(out, _lib.HipMinerCancelled):
                assert got == [True]
                outcomes["cancelled"] += 1
            else:
                assert out == want, out
                outcomes["answered"] += 1
    print(f"soak: {outcomes}")
    assert outcomes["cancelled"] >= 1 and outcomes["answered"] >= 1, outcomes
    check_survives(cctx, refs)


def test_null_relay_runs_to_the_end(cctx, refs):
    """8. hm_debug_no_relay: the launches get no cancel pointer and the host
    does not test the flag, so the signalled call ([10^9, 5*10^9], about 0.11 s)
    runs to its end and finds nothing: what stops a launch is the relay."""
    cctx.debug_no_relay(True)
    try:
        out, wall, got = run_cancelled(cctx, lambda: cctx.find(MSG, 10**9, 5 * 10**9, 1), 0.02)
    finally:
        cctx.debug_no_relay(False)
    print(f"null relay: wall {wall:.3f} s")
    assert got == [True] and out is None, (got, out)
    st = cctx.find_stats()
    assert st["found"] == 0 and st["tasks_run"] > 0, st
    check_survives(cctx, refs)

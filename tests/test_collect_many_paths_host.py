"""The case lists of tests/test_gpu_collect_many_paths.py, what they reach, and
the comparison helpers that module uses.

hm_collect_many's kernel (hm_fused_collect_kernel, fused_collect_kernels.hip)
keeps its own task decoders, its own piece arithmetic and its own id-to-piece
decode, and adds a reservation protocol (one cursor per device, a `full` flag, a
tag per record).  The lists of tests/test_gpu_collect_many.py stay below one
round of a launch's waves, run HM_OPT_FUSED_PARTS = 1 only, and decide an
overflow once, in the first chunk.  The lists here are pure functions (fixed
seeds, the planner's debug export, the CPU oracle; no GPU):

  multi-round  multi_round_cases() of tests/test_find_many_paths_host.py as is:
               68 layout keys, each with >= 3 rounds of whole tasks in the keyed
               segment at HM_OPT_GRID_PER_CU = 1 on 256 CUs.  "Small" cases fit
               HM_COLLECT_CAP_MAX (2^24) nonces and also run dense with a buffer;
               "big" ones (the chained f >= 2 keys) run as a count and at the
               mid target.  Mid targets: 2^64 / 16 (small: four hits per 64-lane
               step on average) and 2^64 / BIG_DIV (big).
  pieces       the 8 all-piece windows of split_subset() with every hash.
  mixed        about 40 requests of 1 .. 2^22 nonces, five kinds of target.
  overflow     130 small requests (three chunks) and a list around
               HM_OPT_COLLECT_WINDOW = 1000 that begins with a fallback.

The oracle's answers are memoised per session (memo of
tests/test_collect_layouts_host.py) and kept as numpy arrays.  Measured once:
scan_sum plus the mid list of all 68 cases (1.12 * 10^7 records) take 78 s on a
16-CPU host and 214 s on an 8-CPU one (184 s the 64 small cases, whose cost is
the oracle call per record on one thread; 30 s the 4 big ones).  That is below
three minutes on 16 CPUs, so the big cases keep the divisor 128; 256 would put
the shortest big list (158 146 records) below 10^5.

The last test corrupts correct answers and shows that each helper rejects
them: the evidence that the GPU module would notice a subtly wrong kernel.
"""
import random
import time

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_find_many_paths_host as F
from tests.test_collect_layouts_host import MAX, WINDOW_CAP, memo, message, segment
from tests.test_collect_many_host import expected
from tests.test_gpu_collect import oracle_list
from tests.test_gpu_collect_layouts import scan_sum, wrapped_sum
from tests.test_gpu_collect_many import small_requests

SMALL_DIV = 16
BIG_DIV = 128                 # below oracle_list's 1/100: the list is walked in 16 parts
FUSED_MAX = 1 << 27           # kFusedNonces
MID_MIN, MID_MAX = 10**5, 1 << 24


def as_array(recs):
    """A list of (hash, nonce) pairs as a (k, 2) uint64 array."""
    return np.array(recs, dtype=np.uint64).reshape(-1, 2)


def span_of(c):
    return c["hi"] - c["lo"] + 1


# ---- the multi-round list ---------------------------------------------------

def is_small(c):
    return span_of(c) <= WINDOW_CAP


def mid_target(c):
    return 2**64 // (SMALL_DIV if is_small(c) else BIG_DIV)


def window_sum(oracle_mod, c):
    """scan_sum of the case's whole window: ((min hash, its nonce), sum, count)."""
    return memo(("collect_many_sum", c["name"]),
                lambda: scan_sum(oracle_mod, c["m"], c["lo"], c["hi"]))


def mid_list(oracle_mod, c):
    """oracle_list of the case's window at its mid target, as an array."""
    return memo(("collect_many_mid", c["name"]),
                lambda: as_array(oracle_list(oracle_mod, c["m"], c["lo"], c["hi"], mid_target(c))))


def prime(oracle_mod):
    """Every answer of the multi-round list, ahead of the tests that use them."""
    for c in F.multi_round_cases():
        window_sum(oracle_mod, c)
        mid_list(oracle_mod, c)


# ---- the piece windows ------------------------------------------------------

def window_hashes(oracle_mod, c):
    """c_hash of every nonce of piece_window(c), a uint64 array."""
    def build():
        lo, hi = F.piece_window(c)
        return np.array([oracle_mod.c_hash(c["m"], n) for n in range(lo, hi + 1)], dtype=np.uint64)
    return memo(("collect_many_window_hashes", c["name"]), build)


# ---- the mixed batch --------------------------------------------------------

MIX_LENGTHS = (0, 8, 55, 56, 64, 120)
# (span, kinds of target): "all" 2^64 - 1, "eighth" 2^64 / 8, "sparse" 2^64 / 1000,
# "none" 1, "one" the window's minimum + 1
MIX_SHAPE = [(1, "all none one eighth"), (63, "all sparse one"), (64, "all eighth none"),
             (65, "all one sparse"), (640, "all eighth one"), (641, "all sparse eighth"),
             (10**4, "all eighth sparse one"), (10**5, "all eighth sparse none"),
             (10**6, "all all eighth sparse one"), (2**22, "all sparse none one")]
MIX_TARGETS = {"all": MAX, "eighth": 2**64 // 8, "sparse": 2**64 // 1000, "none": 1}


def mixed_batch(oracle_mod):
    """[(kind, (m, lo, hi, T)), ...], shuffled with a fixed seed: MIX_SHAPE's
    requests, each across a digit-count change (drawn until every segment of
    the window is fusible) with a message of one of MIX_LENGTHS; two dead
    requests ("dead"), one at the top of u64 and a copy of another ("copy")."""
    def build():
        rng = random.Random(4040)
        out = []
        for i, (span, kinds) in enumerate(MIX_SHAPE):
            for j, kind in enumerate(kinds.split()):
                L = MIX_LENGTHS[(i + j) % len(MIX_LENGTHS)]
                m = message(L, rng)
                while True:
                    d = rng.randrange(len(str(span)) + 1, 20)
                    lo = 10**d - (rng.randrange(1, span) if span > 1 else 1)
                    hi = lo + span - 1
                    if all(F.fusible(s) for s in _lib.debug_plan(m, lo, hi)):
                        break
                T = MIX_TARGETS.get(kind) or scan_sum(oracle_mod, m, lo, hi)[0][0] + 1
                out.append((kind, (m, lo, hi, T)))
        out.append(("eighth", (b"top of u64", MAX - 9_999, MAX, MIX_TARGETS["eighth"])))
        out.append(("dead", (b"dead", 5, 4, MAX)))
        out.append(("dead", (b"no target", 0, 10**5, 0)))
        out.append(("copy", next(r for k, r in out if k == "eighth" and r[2] - r[1] + 1 == 10**4)))
        rng.shuffle(out)
        return out
    return memo("collect_many_mixed", build)


def mixed_answers(oracle_mod):
    """Per request of the mixed batch ("dense", scan_sum's triple) for target
    2^64 - 1 and ("list", the oracle's records as an array) otherwise."""
    def build():
        out = []
        for kind, (m, lo, hi, T) in mixed_batch(oracle_mod):
            if kind == "dead":
                out.append(("list", as_array([])))
            elif kind == "all":
                out.append(("dense", scan_sum(oracle_mod, m, lo, hi)))
            else:
                out.append(("list", as_array(oracle_list(oracle_mod, m, lo, hi, T))))
        return out
    return memo("collect_many_mixed_answers", build)


def answer_total(a):
    return a[1][2] if a[0] == "dense" else len(a[1])


# ---- the overflow lists -----------------------------------------------------

def overflow_requests(oracle_mod):
    """130 requests (chunks of 64, 64 and 2) with the oracle's (total, per, recs)."""
    def build():
        reqs = small_requests(53, 130)
        return reqs, expected(oracle_mod, reqs)
    return memo("collect_many_overflow", build)


WINDOW = 1000
WINDOW_SIZES = (1001, 999, 1000, 1001, 1000, 999, 1001, 1000)


def window_requests(oracle_mod):
    """Requests of 999, 1000 and 1001 nonces for HM_OPT_COLLECT_WINDOW = 1000:
    the first is a fallback, the last is fused and dense.  (reqs, expected,
    the indices of the fused requests)."""
    def build():
        m = b"collect window"
        reqs = [(m + bytes([i]), 99_500 + i, 99_500 + i + s - 1, 2**64 // 50)
                for i, s in enumerate(WINDOW_SIZES)]
        reqs[-1] = reqs[-1][:3] + (MAX,)
        fused = [i for i, s in enumerate(WINDOW_SIZES) if s <= WINDOW]
        return reqs, expected(oracle_mod, reqs), fused
    return memo("collect_many_window", build)


# ---- the comparison helpers of the GPU module -------------------------------

def check_list(got, want, tag=""):
    """`got` (a (k, 2) uint64 array of (hash, nonce)) is `want` bit for bit, in order."""
    assert got is not None and got.shape == want.shape, (tag, None if got is None else got.shape,
                                                          want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (tag, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def check_dense(got, lo, hi, ssum, tag="", sub=None):
    """`got` holds every nonce of lo..hi once, ascending; the wrapped sum of the
    hashes and the (hash, nonce) minimum are scan_sum's.  sub = (T, list): the
    records with hash < T are that list, bit for bit.  Sum, minimum and nonce
    set do not see two hashes swapped between nonces; `sub` does where one of
    the two is below T, the mid-target runs compare such hashes exactly, and
    check_window compares every hash."""
    best, s, count = ssum
    span = hi - lo + 1
    assert count == span and got is not None and got.shape == (span, 2), (tag, count, span)
    want = np.arange(lo, hi + 1, dtype=np.uint64) if hi < MAX else \
        np.array(range(lo, hi + 1), dtype=np.uint64)
    bad = np.flatnonzero(got[:, 1] != want)
    assert bad.size == 0, (tag, lo + int(bad[0]), int(got[bad[0], 1]))
    assert wrapped_sum(got[:, 0]) == s, (tag, wrapped_sum(got[:, 0]), s)
    k = int(np.argmin(got[:, 0]))           # the first of equal minima: the lowest nonce
    assert (int(got[k, 0]), lo + k) == tuple(best), (tag, int(got[k, 0]), lo + k, best)
    if sub is not None:
        check_list(got[got[:, 0] < np.uint64(sub[0])], sub[1], tag)


def check_window(got, lo, hashes, tag=""):
    """`got` holds nonces lo, lo + 1, ... in order, each with its hash of `hashes`."""
    assert got is not None and got.shape == (len(hashes), 2), tag
    check_list(got, np.stack([hashes, np.arange(lo, lo + len(hashes), dtype=np.uint64)], axis=1),
               tag)


def check_totals(total, totals, per, tag=""):
    """Every request's total and their sum."""
    assert list(totals) == list(per), (tag, [(i, a, b) for i, (a, b) in
                                             enumerate(zip(totals, per)) if a != b][:4])
    assert total == sum(per), (tag, total, sum(per))


# ---- the host tests ---------------------------------------------------------

def test_multi_round_list_suits_collect(oracle_mod):
    """Every window of the find list is wholly fusible (collect fuses all of a
    request or nothing) and within one fused launch; the mid lists are long
    enough to cross many steps and fit HM_COLLECT_CAP_MAX."""
    cases = F.multi_round_cases()
    assert len(cases) == 68 and len({c["name"] for c in cases}) == 68
    spent = {True: 0.0, False: 0.0}
    for c in cases:
        t0 = time.perf_counter()
        window_sum(oracle_mod, c)
        mid_list(oracle_mod, c)
        spent[is_small(c)] += time.perf_counter() - t0
    small = big = 0
    sizes = []
    for c in cases:
        segs, _ = F.plan_of(c)
        assert all(F.fusible(s) for s in segs), c
        assert span_of(c) <= FUSED_MAX, c
        if is_small(c):
            small += 1
            assert F.task_nonces(c["key"]) == 640 and span_of(c) <= 2_700_000, c
        else:
            big += 1
            assert c["key"][0] == "chained" and c["key"][1] >= 2, c
            assert 2.0e7 <= span_of(c) <= 2.7e7, c
        best, _, count = window_sum(oracle_mod, c)
        assert count == span_of(c) and c["lo"] <= best[1] <= c["hi"]
        want = mid_list(oracle_mod, c)
        sizes.append(len(want))
        assert MID_MIN <= len(want) <= MID_MAX, (c["name"], len(want))
        assert int(want[:, 0].max()) < mid_target(c) and np.all(want[1:, 1] > want[:-1, 1])
        assert c["lo"] <= int(want[0, 1]) and int(want[-1, 1]) <= c["hi"]
    assert small + big == 68 and small > 0 and big > 0
    assert mid_target(next(c for c in cases if not is_small(c))) < 2**64 // 100
    print(f"collect multi-round list: {small} small cases (window <= 2^24 nonces, dense with a "
          f"buffer, mid target 2^64 / {SMALL_DIV}), {big} big cases (chained f >= 2, mid target "
          f"2^64 / {BIG_DIV}); records per mid list: min {min(sizes)}, max {max(sizes)}, "
          f"{sum(sizes)} in all: " + " ".join(map(str, sizes))
          + f"; oracle time {spent[True]:.0f} s for the small cases, {spent[False]:.0f} s for "
          f"the big ones")


def test_piece_windows_have_every_hash(oracle_mod):
    sub = F.split_subset()
    assert len(sub) == 8
    for what, c in sub.items():
        lo, hi = F.piece_window(c)
        hs = window_hashes(oracle_mod, c)
        assert hs.dtype == np.uint64 and len(hs) == hi - lo + 1 == 20_000, what
        assert lo < c["edge"] <= hi
        for n in (lo, c["edge"] - 1, c["edge"], hi):
            assert int(hs[n - lo]) == _lib.host_hash(c["m"], n), (what, n)


def test_mixed_batch_shape(oracle_mod):
    mix = mixed_batch(oracle_mod)
    ans = mixed_answers(oracle_mod)
    assert mix == mixed_batch(oracle_mod) and 38 <= len(mix) <= 42
    kinds = [k for k, _ in mix]
    reqs = [r for _, r in mix]
    spans = [hi - lo + 1 if lo <= hi else 0 for _, lo, hi, _ in reqs]
    assert {s for k, s in zip(kinds, spans) if k != "dead"} == {s for s, _ in MIX_SHAPE}
    assert {len(m) for m, *_ in reqs} >= set(MIX_LENGTHS)
    assert {"all", "eighth", "sparse", "none", "one", "dead", "copy"} == set(kinds)
    assert kinds.count("dead") == 2 and any(hi == MAX for _, _, hi, _ in reqs)
    copy = reqs[kinds.index("copy")]
    assert reqs.count(copy) == 2
    assert kinds != sorted(kinds)                       # shuffled
    for (kind, (m, lo, hi, T)), a in zip(mix, ans):
        if kind == "dead":
            assert answer_total(a) == 0
            continue
        segs = _lib.debug_plan(m, lo, hi)
        assert all(F.fusible(s) for s in segs), (kind, lo, hi)
        if hi < MAX:
            assert segs[0]["d"] + 1 == segs[-1]["d"] or hi == lo, (lo, hi)
        assert answer_total(a) == {"all": hi - lo + 1, "none": 0, "one": 1}.get(kind,
                                                                                 answer_total(a))
    per = [answer_total(a) for a in ans]
    dense = [s for (k, _), s in zip(mix, spans) if k == "all"]
    sparse = sum(p for (k, _), p in zip(mix, per) if k != "all")
    assert sum(per) <= 1 << 24
    assert sum(s >= 10**6 for s in dense) >= 2
    assert sparse <= 5 * 10**5
    print(f"mixed batch: {len(mix)} requests, spans {sorted(set(spans))}, "
          f"{len(dense)} dense ({sum(dense)} records), {sparse} records in the others, "
          f"{sum(per)} in all; kinds " + " ".join(f"{k}:{kinds.count(k)}" for k in sorted(set(kinds))))


def test_overflow_lists(oracle_mod):
    reqs, (total, per, _) = overflow_requests(oracle_mod)
    assert len(reqs) == 130 and total == sum(per)
    # three distinct caps: the second and the third chunk each add records
    assert sum(per[:64]) > 0 and sum(per[64:128]) > 0 and sum(per[128:]) > 0
    wreqs, (wtotal, wper, _), fused = window_requests(oracle_mod)
    spans = [hi - lo + 1 for _, lo, hi, _ in wreqs]
    assert set(spans) == {999, 1000, 1001} and spans[0] == 1001 and wper[0] > 0
    assert fused == [i for i, s in enumerate(spans) if s <= WINDOW] and fused[-1] == len(wreqs) - 1
    assert wreqs[-1][3] == MAX and wper[-1] == spans[-1] == 1000
    assert 0 < sum(wper[i] for i in fused) < wtotal
    for m, lo, hi, _ in wreqs:      # fusible but for the window
        assert all(F.fusible(s) for s in _lib.debug_plan(m, lo, hi))
    print(f"overflow lists: 130 requests, records per chunk {sum(per[:64])} {sum(per[64:128])} "
          f"{sum(per[128:])}; window list {wper}, fused {fused}")


def _rejects(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def test_checkers_reject_corrupted_answers(oracle_mod):
    """Each comparison helper accepts the oracle's own answer and rejects it
    with one record dropped, one duplicated, two hashes swapped between nonces,
    one hash off by one; check_totals rejects a total off by one."""
    m, lo, hi, T = b"checker", 99_000, 101_999, 2**64 // 16
    want = as_array(oracle_list(oracle_mod, m, lo, hi, T))
    hs = np.array([oracle_mod.c_hash(m, n) for n in range(lo, hi + 1)], dtype=np.uint64)
    dense = np.stack([hs, np.arange(lo, hi + 1, dtype=np.uint64)], axis=1)
    ssum = scan_sum(oracle_mod, m, lo, hi)
    assert np.array_equal(want, dense[hs < np.uint64(T)]) and len(want) > 100
    kmin = int(np.argmin(hs))

    def corruptions(a, i, j):
        drop = np.delete(a, i, axis=0)
        dup = np.insert(a, i, a[i], axis=0)
        swap = a.copy()
        swap[[i, j], 0] = a[[j, i], 0]
        off = a.copy()
        off[i, 0] += np.uint64(1)
        return {"dropped": drop, "duplicated": dup, "swapped": swap, "off by one": off}

    check_list(want, want)
    for name, bad in corruptions(want, 7, 50).items():
        _rejects(check_list, bad, want, name)
    check_window(dense, lo, hs)
    for name, bad in corruptions(dense, 1234, 2000).items():
        _rejects(check_window, bad, lo, hs, name)
    # sum, minimum and nonce set: a swap shows where it moves the minimum ...
    check_dense(dense, lo, hi, ssum)
    other = kmin + 1 if kmin + 1 < len(hs) else kmin - 1
    for name, bad in corruptions(dense, kmin, other).items():
        _rejects(check_dense, bad, lo, hi, ssum, name)
    for name, bad in corruptions(dense, 1234, 2000).items():
        if name != "swapped":
            _rejects(check_dense, bad, lo, hi, ssum, name)
    # ... and, with the mid list beside it, where either hash is below the mid target
    check_dense(dense, lo, hi, ssum, sub=(T, want))
    i = int(np.flatnonzero(hs < np.uint64(T))[3])
    j = int(np.flatnonzero(hs >= np.uint64(T))[3])
    assert i != kmin
    for name, bad in corruptions(dense, i, j).items():
        _rejects(check_dense, bad, lo, hi, ssum, name, sub=(T, want))
    per = [3, 0, 17]
    check_totals(20, per, per)
    _rejects(check_totals, 21, per, per)
    _rejects(check_totals, 20, [3, 1, 17], per)
    _rejects(check_totals, 20, [3, 0, 16], per)

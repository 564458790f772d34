"""hm_find_k_many on the paths tests/test_gpu_find_k_many.py does not reach
(tests/test_find_k_many_paths_host.py builds the lists, shows what they reach,
and shows that the comparison used here rejects corrupted answers):

  a. launches of several wave rounds on every kernel instantiation: the counter
     dequeue, waves that enter a task after `stop` was lowered, a bound set in
     one segment pruning another, and the `room` arithmetic of
     take_step(WaveFirstK&) when k falls inside one step's hits;
  b. HM_OPT_FUSED_PARTS x HM_OPT_FUSED_TAIL on the find_k kernel, over several
     rounds and on windows where every id is a piece; a slice that the records
     fill exactly (cursor == B);
  c. windows one fused launch cannot hold: the k-th hit at the last fused and
     at the first unfused nonce, the rest of the range supplying hits, no prefix
     at all, such requests mixed with launched and dead ones on one and two
     devices;
  d. a stop word lowered to 0;
  e. guided-tail pieces whose task_lo lies above their segment's end in a
     segment that is not the launch's last (the clamp of fk_enter).

Every answer is compared exactly, record by record and in order, with the C
oracle's; hm_find_k answers every multi-round and prefix request too and must
agree.  Every case asserts through hm_find_k_many_stats which path it took.
Which wave fills slot k is a race no test can force; the answers must not
depend on it."""
import ctypes

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_find_k_many_paths_host as H
from tests import test_find_many_paths_host as F
from tests import test_gpu_collect_many_paths as P
from tests.test_collect_layouts_host import parts
from tests.test_collect_many_paths_host import as_array, check_list
from tests.test_gpu_collect_many_paths import primed  # noqa: F401  (the fixture)
from tests.test_gpu_find_many_paths import cus, expected_ids  # noqa: F401  (cus: a fixture)
from tests.test_gpu_verify import multi  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
RES = ctypes.POINTER(_lib.hm_result)


class options(P.options):
    DEFAULTS = {**P.options.DEFAULTS, _lib.HM_OPT_FIND_K_BUF: 0}


def many(c, reqs):
    """hm_find_k_many into a numpy buffer: (per request a (count, 2) uint64
    array of (hash, nonce), stats)."""
    arr, n, keep = _lib.find_k_requests(reqs)
    ks = [r[4] for r in reqs]
    buf = np.empty((max(1, sum(ks)), 2), dtype=np.uint64)
    counts = (ctypes.c_size_t * max(1, n))()
    rc = _lib.load().hm_find_k_many(c._h, arr, n, buf.ctypes.data_as(RES), counts)
    del keep
    assert rc == _lib.HM_OK, (rc, [r[1:] for r in reqs][:4])
    ends = np.cumsum([0] + ks)
    return ([buf[ends[i]:ends[i] + int(counts[i])] for i in range(n)], c.find_k_many_stats())


def one(c, req):
    """(answer, stats) of a one-request call: the stats are the request's."""
    got, st = many(c, [req])
    return got[0], st


def find_k(c, req):
    """hm_find_k on the same request, as an array."""
    m, lo, hi, T, k = req
    buf = np.empty((k, 2), dtype=np.uint64)
    n = ctypes.c_size_t(0)
    rc = _lib.load().hm_find_k(c._h, m, len(m), lo, hi, T, k, buf.ctypes.data_as(RES),
                               ctypes.byref(n))
    assert rc == _lib.HM_OK, (rc, req[1:])
    return buf[:int(n.value)]


def case_opts(c):
    return {_lib.HM_OPT_GRID_PER_CU: 1, _lib.HM_OPT_FORCE_GENERIC: int(c["generic"])}


def has_chained(c):
    return any(k[0] == "chained" for k in F.plan_of(c)[1])


# ---- a. several rounds, every kernel ------------------------------------------

@pytest.mark.parametrize("part", range(F.LIST_ITEMS))
def test_several_rounds_every_kernel(ctx, oracle_mod, primed, cus, part):  # noqa: F811
    cases = parts(F.multi_round_cases(), F.LIST_ITEMS)[part]
    assert cases
    for c in cases:
        kc = H.k_cases(oracle_mod, c)
        full, n, j = kc["full"], kc["N"], kc["j"]
        with options(ctx, {**case_opts(c), _lib.HM_OPT_FIND_K_BUF: H.FIND_K_BUF}):
            for k in kc["ks"]:
                req = (c["m"], c["lo"], c["hi"], kc["T"], k)
                got, st = one(ctx, req)
                tag = f"{c['name']} L={c['L']} lo={c['lo']} hi={c['hi']} k={k} N={n} j={j} {st}"
                print(f"{c['name']} k={k}: tasks_run {st['tasks_run']} of {st['tasks_total']}, "
                      f"records {st['records']}")
                check_list(got, full[:k], tag)
                check_list(find_k(ctx, req), full[:k], "hm_find_k " + tag)
                assert st["requests"] == st["fused"] == st["launches"] == 1, tag
                assert st["fallback"] == st["overflow"] == 0 and st["found"] == min(k, n), tag
                assert st["nonces_enqueued"] == c["hi"] - c["lo"] + 1, tag
                # three rounds on THIS device, or the list is too small for it
                assert st["tasks_total"] >= F.ROUNDS * 4 * cus, tag
                if k == n + 3:
                    if not has_chained(c):
                        assert st["tasks_run"] == st["tasks_total"], tag
                    else:
                        assert 0 < st["tasks_run"] <= st["tasks_total"], tag
                elif k in (1, H.K_MID):
                    # the k-th hit lies in the first quarter of a >= 3-round window: `stop`
                    # is lowered in round one, and later rounds' tasks are skipped
                    assert 0 < st["tasks_run"] < st["tasks_total"], tag
                else:
                    assert 0 < st["tasks_run"] <= st["tasks_total"], tag
                if k == j:
                    assert int(got[-1, 1]) < c["edge"], tag
                elif k == j + 1:
                    assert int(got[-1, 1]) >= c["edge"], tag


# ---- b. the split options ----------------------------------------------------

@pytest.mark.parametrize("tail", [1, 5, 10])
@pytest.mark.parametrize("nparts", [2, 5, 10])
def test_split_options_over_several_rounds(ctx, oracle_mod, primed, cus, nparts, tail):  # noqa: F811
    """The subset's multi-round windows under every PARTS x TAIL, k = 1, j + 1
    and N + 3: the same answers; the ids are those of the TAIL = 1 run with its
    last tasks split."""
    differ = []
    for what, c in F.split_subset().items():
        kc = H.k_cases(oracle_mod, c)
        full, n, j = kc["full"], kc["N"], kc["j"]
        opts = {**case_opts(c), _lib.HM_OPT_FUSED_PARTS: nparts, _lib.HM_OPT_FUSED_TAIL: 1,
                _lib.HM_OPT_FIND_K_BUF: H.FIND_K_BUF}
        with options(ctx, opts):
            got, st1 = one(ctx, (c["m"], c["lo"], c["hi"], kc["T"], n + 3))
            check_list(got, full, (what, nparts, "TAIL 1", st1))
            assert st1["tasks_total"] >= F.ROUNDS * 4 * cus, (what, st1)
            ctx.set_option(_lib.HM_OPT_FUSED_TAIL, tail)
            for k in (1, j + 1, n + 3):
                got, st = one(ctx, (c["m"], c["lo"], c["hi"], kc["T"], k))
                tag = (what, c["name"], nparts, tail, k, st)
                check_list(got, full[:k], tag)
                assert st["fused"] == st["launches"] == 1, tag
                assert st["fallback"] == st["overflow"] == 0 and st["found"] == min(k, n), tag
                assert st["tasks_total"] == expected_ids(st1["tasks_total"], 4 * cus, tail), tag
                assert 0 < st["tasks_run"] <= st["tasks_total"], tag
                if k == 1:
                    assert st["tasks_run"] < st["tasks_total"], tag
            differ.append(st["tasks_total"] != st1["tasks_total"])
    print(f"PARTS {nparts} TAIL {tail}: {sum(differ)} of {len(differ)} launches have pieces")
    if tail > 1:
        assert any(differ)      # some launch ended on a partial round and was split


def piece_run(ctx, c, T, k, want, buf, tag):
    lo, hi = F.piece_window(c)
    with options(ctx, {_lib.HM_OPT_FIND_K_BUF: buf}):
        got, st = one(ctx, (c["m"], lo, hi, T, k))
    tag = (tag, T, k, buf, st)
    check_list(got, want, tag)
    assert st["requests"] == 1 and st["found"] == len(want), tag
    assert st["nonces_enqueued"] == 20_000 or st["fallback"], tag
    return st


@pytest.mark.parametrize("nparts", [2, 5, 10])
def test_split_options_every_id_a_piece(ctx, oracle_mod, nparts):
    """Windows of 2 * 10^4 nonces at HM_OPT_GRID_PER_CU = 16: fewer tasks than a
    tenth of a round, so every task runs as HM_OPT_FUSED_TAIL pieces (the ids
    are TAIL times those of the TAIL = 1 run, which are the task model's).
    Dense with k = 20 000 and a slice of exactly 20 000 records: every nonce of
    the window once, with the oracle's hash, the cursor ending exactly at the
    slice's size (not an overflow) -- a piece that drops or repeats a nonce
    cannot pass."""
    for what, c in F.split_subset().items():
        cases = H.piece_cases(oracle_mod, c)
        opts = {_lib.HM_OPT_GRID_PER_CU: F.SPLIT_GRID, _lib.HM_OPT_FUSED_PARTS: nparts,
                _lib.HM_OPT_FORCE_GENERIC: int(c["generic"]), _lib.HM_OPT_FUSED_TAIL: 1}
        with options(ctx, opts):
            total1 = None
            for tail in (1, 2, 5, 10):
                ctx.set_option(_lib.HM_OPT_FUSED_TAIL, tail)
                for kind, T, k, want in cases:
                    tag = (what, c["name"], nparts, tail, kind)
                    if kind == "sparse":
                        st = piece_run(ctx, c, T, k, want, 0, tag)
                    elif k == 19_999:
                        # whether the slice overflows depends on whether the last task ran
                        st = piece_run(ctx, c, T, k, want, 19_999, tag)
                        assert st["fused"] + st["fallback"] == 1 and st["overflow"] in (0, 1), tag
                        assert st["fused"] == 1 - st["overflow"], (tag, st)
                        continue
                    else:
                        st = piece_run(ctx, c, T, k, want, 20_000, tag)
                    assert (st["fused"], st["fallback"], st["overflow"], st["launches"]) == \
                        (1, 0, 0, 1), (tag, st)
                    if total1 is None:
                        total1 = st["tasks_total"]
                        segs, _ = F.plan_of(c, *F.piece_window(c))
                        assert total1 == sum(H.seg_tasks(s, nparts) for s in segs), (tag, st)
                    assert st["tasks_total"] == tail * total1, (tag, st, total1)
                    assert 0 < st["tasks_run"] <= st["tasks_total"], (tag, st)


# ---- c. windows one fused launch cannot hold ---------------------------------

def check_prefix(c, case, table_digits=0):
    req, want = case["req"], as_array(case["want"])
    with options(c, {_lib.HM_OPT_TABLE_DIGITS: table_digits}):
        got, st = one(c, req)
        tag = (case["L"], case["d"], case["what"], req[1:], table_digits, st)
        check_list(got, want, tag)
        check_list(find_k(c, req), want, ("hm_find_k", tag))
    assert st["requests"] == 1 and st["found"] == len(want) == req[4] and st["overflow"] == 0, tag
    if case["what"] == "last":
        assert (st["fused"], st["fallback"], st["launches"]) == (1, 0, 1), tag
    elif case["what"] == "empty":
        assert (st["fused"], st["fallback"]) == (0, 1) and st["launches"] >= 1, tag
    else:
        assert (st["fused"], st["fallback"]) == (0, 1) and st["launches"] >= 2, tag
        # the answer's first records are the prefix's
        check_list(got[:len(case["prefix"])], as_array(case["prefix"]), tag)


@pytest.mark.parametrize("which", range(len(F.UNFUSED)), ids=[f"L{L}-d{d}" for L, d in F.UNFUSED])
def test_natural_unfused_prefixes(ctx, oracle_mod, which):
    """The planner itself ends the fusible prefix (a chained f = 5 segment
    follows): the k-th hit at the last fused nonce (one launch, no fallback),
    at the first unfused one, five hits from the rest, and no prefix at all."""
    cases = H.prefix_cases(oracle_mod)[4 * which:4 * which + 4]
    assert sorted(c["what"] for c in cases) == ["empty", "first", "last", "more"]
    for case in cases:
        check_prefix(ctx, case)


def test_table_digits_leave_the_prefix_fusible(ctx, oracle_mod):
    """HM_OPT_TABLE_DIGITS = 3 reaches the chained layout with f >= 5 alone: the
    prefix stays fusible and the rest runs in epochs; the answers and the paths
    are those of the default."""
    for case in H.prefix_cases(oracle_mod)[:4]:
        check_prefix(ctx, case, table_digits=3)


@pytest.mark.parametrize("ndev", [1, 2])
def test_mixed_chunk(ctx, multi, oracle_mod, ndev):  # noqa: F811
    """65 requests: launched, empty-prefix and dead ones, the 65th a chunk of
    its own without a launch; on two devices every request of device 1 has an
    empty prefix, so that device launches nothing (and its slab is empty)."""
    c = ctx if ndev == 1 else multi[ndev]
    mix = H.mix_requests(oracle_mod)
    n = {kind: sum(k == kind for k, _, _ in mix) for kind in ("launched", "empty", "dead")}
    got, st = many(c, [r for _, r, _ in mix])
    for i, ((kind, r, want), g) in enumerate(zip(mix, got)):
        check_list(g, as_array(want), (i, kind, r[1:]))
    assert st["requests"] == 65 == sum(n.values()) and st["ndev"] == ndev, st
    assert st["fused"] == n["launched"] and st["fallback"] == n["empty"], (st, n)
    assert st["found"] == sum(len(w) for _, _, w in mix) and st["overflow"] == 0, (st, n)
    assert st["launches"] >= n["launched"] + n["empty"], (st, n)


# ---- d. a stop word of 0 ------------------------------------------------------

@pytest.mark.parametrize("force_generic", [0, 1], ids=["fast", "generic"])
def test_stop_word_zero(ctx, oracle_mod, cus, force_generic):  # noqa: F811
    """The k-th hit is nonce 0 of [0, 10^6]: `stop` is lowered to 0, which is a
    bound like any other and not "unset".
    "alone": nonce 0 is the range's only hit, so the one record is in slot 0 and
    the stop word can only become 0; its task (id 0, the ten one-digit nonces)
    publishes after one step.  At HM_OPT_GRID_PER_CU = 1 the range has more
    tasks than the launch has waves (asserted), the others of 640 nonces each,
    so the ids beyond the first round are drawn after that publish and skipped.
    "easy": the target may be as easy as 2^64 / 100.  Then another wave's record
    may take slot 0, `stop` becomes that record's nonce, published at the end of
    a 640-nonce task while the second round is being drawn (once all 1599 of
    1599 tasks ran): only the answers and the path are asserted, with k = 1 and
    with k = 2 (nonce 0 and a later hit), and the slice sized to hold every hit
    of the range (shown on the host; the default one overflows in round one)."""
    zero = H.zero_cases(oracle_mod)
    ra, wa = zero["alone"]
    (r1, w1), (r2, w2) = zero["easy"]
    base = {_lib.HM_OPT_FORCE_GENERIC: force_generic, _lib.HM_OPT_FIND_K_BUF: H.ZERO_BUF}
    with options(ctx, {**base, _lib.HM_OPT_GRID_PER_CU: 1}):
        got, st = one(ctx, ra)
        print("stop word 0:", st)
        check_list(got, as_array(wa), st)
        assert (st["fused"], st["fallback"], st["overflow"], st["launches"]) == (1, 0, 0, 1), st
        assert st["records"] == 1 and st["nonces_enqueued"] == H.ZERO_HI + 1, st
        assert st["tasks_total"] > 4 * cus, ("too few tasks for this device", st)
        assert 0 < st["tasks_run"] < st["tasks_total"], st
        for req, want in ((r1, w1), (r2, w2)):
            got, st = one(ctx, req)
            check_list(got, as_array(want), st)
            assert (st["fused"], st["fallback"], st["overflow"]) == (1, 0, 0), st
            assert 0 < st["tasks_run"] <= st["tasks_total"], st
    # and at the default grid, in one call
    with options(ctx, base):
        got, st = many(ctx, [ra, r1, r2])
        for g, w in zip(got, (wa, w1, w2)):
            check_list(g, as_array(w), st)
        assert (st["fused"], st["fallback"], st["found"]) == (3, 0, 4), st


# ---- e. the clamp --------------------------------------------------------------

@pytest.mark.parametrize("tail", H.CLAMP_TAILS)
def test_pieces_that_start_above_their_segments_end(ctx, oracle_mod, tail):
    """Windows of a few tasks, every id a piece: a piece of a generic segment
    that is not the last starts (task_lo) above that segment's end, with `stop`
    in a later segment ("later") or in its own ("earlier").  tasks_total shows
    that every task ran as `tail` pieces."""
    for c in H.clamp_cases(oracle_mod):
        assert H.clamped_pieces(c["segs"], tail)
        opts = {_lib.HM_OPT_FORCE_GENERIC: int(c["generic"]), _lib.HM_OPT_FUSED_TAIL: tail}
        with options(ctx, opts):
            for req, want, where in c["reqs"]:
                for _ in range(3):      # the order in which the pieces run is not fixed
                    got, st = one(ctx, req)
                    tag = (c["name"], tail, where, req[1:], st)
                    check_list(got, as_array(want), tag)
                    assert (st["fused"], st["fallback"], st["overflow"]) == (1, 0, 0), tag
                    assert st["tasks_total"] == tail * c["tasks"], tag
                    assert 0 < st["tasks_run"] <= st["tasks_total"], tag

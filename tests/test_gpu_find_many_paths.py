"""hm_find_many on the paths tests/test_gpu_find_many.py does not reach
(tests/test_find_many_paths_host.py builds the lists and shows what they reach):

  1. launches of several wave rounds on every kernel instantiation: whole
     tasks, the counter dequeue, waves that enter a task after a hit was
     published, bounds carried from one segment's task into another's;
  2. HM_OPT_FUSED_PARTS x HM_OPT_FUSED_TAIL on the find kernel, over several
     rounds and on windows where every id is a piece;
  3. windows one fused launch cannot hold, partly or wholly: an empty and a
     shorter prefix, hits at the last fused and the first unfused nonce, such
     requests mixed with launched and dead ones across a chunk boundary and on
     two devices;
  4. hm_find on the requests of 1 and 3.

Every answer is compared exactly with the C oracle's first-hit search.  Which
wave publishes a hit first is a race no test can force; the answers must not
depend on it, and these runs only make it likelier that they would show it.
"""
import contextlib
import subprocess
import sys

import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_find_many_paths_host as H
from tests.test_collect_layouts_host import parts
from tests.test_gpu_verify import multi  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEFAULTS = {_lib.HM_OPT_FORCE_GENERIC: 0, _lib.HM_OPT_GRID_PER_CU: 0, _lib.HM_OPT_FUSED_PARTS: 1,
            _lib.HM_OPT_FUSED_TAIL: 2, _lib.HM_OPT_TABLE_DIGITS: 0}


@contextlib.contextmanager
def options(c, opts):
    try:
        for o, v in opts.items():
            c.set_option(o, v)
        yield
    finally:
        for o in opts:
            c.set_option(o, DEFAULTS[o])


@pytest.fixture(scope="module")
def cus():
    """The device's CU count as torch reports it, asked in a child process:
    torch initialises a HIP runtime of its own, which finds no device in a
    process where the library's runtime holds it already (the session's ctx)."""
    out = subprocess.run(
        [sys.executable, "-c", "import torch; "
         "print(torch.cuda.get_device_properties(0).multi_processor_count)"],
        check=True, capture_output=True, text=True, timeout=300).stdout
    return int(out.split()[-1])


def one(c, req):
    """(answer, stats) of a one-request call: the stats are the request's."""
    got = c.find_many([req])
    return got[0], c.find_many_stats()


def has_chained(c):
    return any(k[0] == "chained" for k in H.plan_of(c)[1])


# ---- 1. several rounds, every kernel (and 4. hm_find on the same) -----------

@pytest.mark.parametrize("part", range(H.LIST_ITEMS))
def test_several_rounds_every_kernel(ctx, oracle_mod, cus, part):
    cases = parts(H.multi_round_cases(), H.LIST_ITEMS)[part]
    assert cases
    for c in cases:
        a = H.answers(oracle_mod, c)
        opts = {_lib.HM_OPT_GRID_PER_CU: 1, _lib.HM_OPT_FORCE_GENERIC: int(c["generic"])}
        with options(ctx, opts):
            for i, (req, want) in enumerate(zip(a["reqs"], a["want"])):
                got, st = one(ctx, req)
                tag = (c["name"], c["L"], c["lo"], c["hi"], i, st)
                assert got == want, tag
                assert ctx.find(*req) == want, tag
                assert st["requests"] == st["fused"] == st["launches"] == 1, tag
                assert st["fallback"] == 0 and st["found"] == (want is not None), tag
                assert st["nonces_enqueued"] == c["hi"] - c["lo"] + 1, tag
                # three rounds on THIS device, or the list is too small for it
                assert st["tasks_total"] >= H.ROUNDS * 4 * cus, tag
                if i == 0 and not has_chained(c):
                    assert st["tasks_run"] == st["tasks_total"], tag
                elif i == 3:
                    assert 0 < st["tasks_run"] < st["tasks_total"], tag
                else:
                    assert 0 < st["tasks_run"] <= st["tasks_total"], tag


# ---- 2. the split options ----------------------------------------------------

def expected_ids(tasks, waves, tail):
    """Task ids of a fused launch of `tasks` tasks: the tasks % waves last ones
    run as the most pieces (10, 5, 2; at most HM_OPT_FUSED_TAIL) that still fit
    one round of `waves` (hipminer.h, HM_OPT_FUSED_TAIL)."""
    nsplit = tasks % waves
    for p in (10, 5, 2):
        if p <= tail and nsplit * p <= waves:
            return tasks + nsplit * (p - 1)
    return tasks


@pytest.mark.parametrize("tail", [1, 5, 10])
@pytest.mark.parametrize("nparts", [2, 5, 10])
def test_split_options_over_several_rounds(ctx, oracle_mod, cus, nparts, tail):
    """The subset's multi-round requests under every PARTS x TAIL: the same
    answers; the ids are those of the TAIL = 1 run with its last tasks split."""
    differ = []
    for what, c in H.split_subset().items():
        a = H.answers(oracle_mod, c)
        opts = {_lib.HM_OPT_GRID_PER_CU: 1, _lib.HM_OPT_FORCE_GENERIC: int(c["generic"]),
                _lib.HM_OPT_FUSED_PARTS: nparts, _lib.HM_OPT_FUSED_TAIL: 1}
        with options(ctx, opts):
            got, st1 = one(ctx, a["reqs"][0])
            assert got is None and 0 < st1["tasks_run"] <= st1["tasks_total"], (what, st1)
            assert st1["tasks_total"] >= H.ROUNDS * 4 * cus, (what, st1)
            ctx.set_option(_lib.HM_OPT_FUSED_TAIL, tail)
            for i, (req, want) in enumerate(zip(a["reqs"], a["want"])):
                got, st = one(ctx, req)
                tag = (what, c["name"], nparts, tail, i, st)
                assert got == want, tag
                assert st["fused"] == st["launches"] == 1 and st["fallback"] == 0, tag
                assert st["tasks_total"] == expected_ids(st1["tasks_total"], 4 * cus, tail), tag
                assert 0 < st["tasks_run"] <= st["tasks_total"], tag
                if i == 3:
                    assert st["tasks_run"] < st["tasks_total"], tag
            differ.append(st["tasks_total"] != st1["tasks_total"])
    print(f"PARTS {nparts} TAIL {tail}: {sum(differ)} of {len(differ)} requests have pieces")
    if tail > 1:
        assert any(differ)      # some launch ended on a partial round and was split


@pytest.mark.parametrize("nparts", [2, 5, 10])
def test_split_options_every_id_a_piece(ctx, oracle_mod, nparts):
    """Windows of 2 * 10^4 nonces at HM_OPT_GRID_PER_CU = 16: fewer tasks than a
    tenth of a round, so every task runs as HM_OPT_FUSED_TAIL pieces (the ids
    are TAIL times those of the TAIL = 1 run).  Targets: no hit, and every
    prefix minimum of the window, each the first hit of its own request."""
    for what, c in H.split_subset().items():
        reqs, want = H.piece_answers(oracle_mod, c)
        assert len(reqs) >= 4
        opts = {_lib.HM_OPT_GRID_PER_CU: H.SPLIT_GRID, _lib.HM_OPT_FUSED_PARTS: nparts,
                _lib.HM_OPT_FORCE_GENERIC: int(c["generic"]), _lib.HM_OPT_FUSED_TAIL: 1}
        with options(ctx, opts):
            assert ctx.find_many(reqs) == want, (what, nparts)
            st1 = ctx.find_many_stats()
            for tail in (2, 5, 10):
                ctx.set_option(_lib.HM_OPT_FUSED_TAIL, tail)
                got = ctx.find_many(reqs)
                st = ctx.find_many_stats()
                tag = (what, c["name"], nparts, tail, st)
                assert got == want, tag
                assert st["fused"] == st["launches"] == len(reqs) and st["fallback"] == 0, tag
                assert st["tasks_total"] == tail * st1["tasks_total"], (tag, st1)
                assert 0 < st["tasks_run"] <= st["tasks_total"], tag


# ---- 3. windows one fused launch cannot hold (and 4.) -----------------------

def check_unfused(c, oracle_mod, case, table_digits=0):
    m, E, P = case["m"], case["empty"], case["partial"]
    T_in = case["pre"][0] + 1           # the prefix's argmin qualifies: a hit inside the prefix
    runs = [
        # request, answer, fused, fallback
        ((m, *E, case["mn_empty"][0]), None, 0, 1),
        ((m, *E, case["mn_empty"][0] + 1), case["mn_empty"], 0, 1),
        ((m, *P, T_in), oracle_mod.c_find(m, *P, T_in), 1, 0),
        ((m, *P, case["rest"][0] + 1), case["rest"], 0, 1),     # min + 1 of the whole range
        ((m, *P, case["rest"][0]), None, 0, 1),                 # min: none
    ]
    assert runs[2][1][1] < case["B"]
    with options(c, {_lib.HM_OPT_TABLE_DIGITS: table_digits}):
        for req, want, fused, fallback in runs:
            got, st = one(c, req)
            tag = (case["L"], case["d"], req[1:], table_digits, st)
            assert got == want, tag
            assert c.find(*req) == want, tag
            assert (st["fused"], st["fallback"]) == (fused, fallback), tag
            assert st["found"] == (want is not None) and st["requests"] == 1, tag
            if fused:
                assert st["launches"] == 1, tag
            elif req[1] == P[0]:
                assert st["launches"] >= 2, tag     # the prefix's launch, then the rest
            else:
                assert st["launches"] >= 1, tag


@pytest.mark.parametrize("which", range(len(H.UNFUSED)), ids=[f"L{L}-d{d}" for L, d in H.UNFUSED])
def test_unfused_windows(ctx, oracle_mod, which):
    check_unfused(ctx, oracle_mod, H.unfused_cases(oracle_mod)[which])


def test_boundary_of_the_fused_prefix(ctx, oracle_mod):
    """First hits at the last fused nonce and at the first unfused one."""
    for b in H.boundary_cases(oracle_mod):
        req = (b["m"], b["lo"], b["hi"], b["T"])
        got, st = one(ctx, req)
        tag = (b["L"], b["d"], b["lo"], b["nstar"] - b["B"], st)
        assert got == b["want"], tag
        assert ctx.find(*req) == b["want"], tag
        if b["nstar"] < b["B"]:
            assert (st["fused"], st["fallback"], st["launches"]) == (1, 0, 1), tag
        else:
            assert (st["fused"], st["fallback"]) == (0, 1) and st["launches"] >= 2, tag
        assert st["found"] == 1, tag


@pytest.mark.parametrize("ndev", [1, 2])
def test_mixed_chunk(ctx, multi, oracle_mod, ndev):  # noqa: F811
    """65 requests: launched, empty-prefix and dead ones, the 65th a chunk of
    its own without a launch; on two devices every request of device 1 has an
    empty prefix, so that device launches nothing."""
    c = ctx if ndev == 1 else multi[ndev]
    mix = H.mix_requests(oracle_mod)
    reqs = [r for _, r in mix]
    want = [None if kind == "dead" else oracle_mod.c_find(*r) for kind, r in mix]
    n = {kind: sum(k == kind for k, _ in mix) for kind in ("launched", "empty", "dead")}
    hits = sum(w is not None for w in want)
    # every empty-prefix request has a hit; the launched ones with and without
    assert all(w is not None for (kind, _), w in zip(mix, want) if kind == "empty")
    assert n["empty"] < hits < n["empty"] + n["launched"]
    assert c.find_many(reqs) == want
    st = c.find_many_stats()
    assert st["requests"] == 65 == sum(n.values()) and st["ndev"] == ndev, st
    assert st["fused"] == n["launched"] and st["fallback"] == n["empty"], (st, n)
    assert st["found"] == hits, (st, n, hits)
    assert st["launches"] >= n["launched"] + n["empty"], (st, n)


def test_table_digits_leave_the_prefix_fusible(ctx, oracle_mod):
    """HM_OPT_TABLE_DIGITS reaches the chained layout with f >= 5 alone
    (plan.cpp consider_chained_epochs): the f = 4 prefix keeps fe = f and stays
    fusible, the f = 5 rest runs in epochs of 10^3 rows on the per-segment path;
    answers and counts are those of the default.  With -1 the rest is tiled and
    the whole window one fused launch."""
    case = H.unfused_cases(oracle_mod)[0]
    check_unfused(ctx, oracle_mod, case, table_digits=3)
    m, P = case["m"], case["partial"]
    with options(ctx, {_lib.HM_OPT_TABLE_DIGITS: -1}):
        for T, want in ((case["rest"][0] + 1, case["rest"]), (case["rest"][0], None)):
            got, st = one(ctx, (m, *P, T))
            assert got == want, st
            assert (st["fused"], st["fallback"], st["launches"]) == (1, 0, 1), st
            assert st["nonces_enqueued"] == H.UNFUSED_SPAN, st

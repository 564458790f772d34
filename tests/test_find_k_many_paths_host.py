"""The case lists of tests/test_gpu_find_k_many_paths.py, what they reach, and
the comparison that module uses.

hm_find_k_many's kernel (hm_fused_find_k_kernel, fused_find_k_kernels.hip) keeps
private copies of the task decoders, of the piece arithmetic and of the
id-to-piece decode, and adds hm_find_k's publish protocol (`c`, `mx`, filled,
maxk, the stop word).  tests/test_gpu_find_k_many.py keeps every oracle-checked
request below one round of a launch's waves, sets neither split option, and
reaches the unfused rest of a range through HM_OPT_FIND_WINDOW only.  The lists
here are pure functions (fixed seeds, the planner's debug export, the C oracle;
no GPU):

  multi-round  multi_round_cases() of tests/test_find_many_paths_host.py (F) as
               is: 68 layout keys with >= 3 rounds of whole tasks in the keyed
               segment at HM_OPT_GRID_PER_CU = 1 on 256 CUs.  k_cases(): the
               window's hits at the mid target of tests/
               test_collect_many_paths_host.py (2^64 / 16 small, 2^64 / 128
               big), ks 1, 1000, j, j + 1 and N + 3 with j the hits below the
               digit-count change.
  pieces       the 8 all-piece windows of F.split_subset(): dense (every nonce
               a hit) with k = 20 000, 1, 63, 64, 65, 19 999, and sparse
               (2^64 / 64) with k = 1, j, j + 1, N, N + 3.
  prefix       per F.UNFUSED (L, d) a range whose fusible prefix is 10^5 nonces
               and whose rest is a chained f = 5 segment: the k-th hit at the
               last fused nonce, at the first unfused one, k + 5, and the window
               with no prefix at all.
  mix          F.mix_requests() with a k of 1..12 each.
  zero         the k-th hit at nonce 0 of a longer range: a stop word of 0.
  clamp        windows in which a task of a segment that is not the last has
               task_lo > seg_hi (fk_enter's clamp): clamp_search() shows which
               tasks these are, clamp_cases() has GPU cases on them.

Measured once: building every list takes 3 min 47 s on an 8-CPU host (about
80 s on 16 CPUs by test_collect_many_paths_host.py's figures).  All but 25 s of
that is the mid lists of the 68 multi-round cases, which a whole-suite session
computes once for that module, its GPU module and the two here; 18 s are the
scans of F.unfused_cases() under the mix list, shared with F's own tests; the
prefix, piece, zero and clamp lists take under 5 s together.

The last test corrupts correct answers and shows that the comparison rejects
them: the evidence that the GPU module would notice a subtly wrong kernel.
"""
import random

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib
from tests import test_find_many_paths_host as F
from tests.test_collect_layouts_host import (DIGITS, KINDS, MAX, MAX_LEN, PIECE_HALF, memo,
                                             message)
from tests.test_collect_many_paths_host import (as_array, check_list, is_small, mid_list,
                                                mid_target, span_of, window_hashes)
from tests.test_gpu_collect import oracle_list
from tests.test_gpu_find_k_many import oracle_first_k
from tests.test_gpu_find_paths import _piece_boundary

FIND_K_BUF = 1 << 22          # HM_OPT_FIND_K_BUF of the multi-round runs
K_MID = 1000
PIECE_SPARSE = 2**64 // 64
PIECE_DENSE_KS = (20_000, 1, 63, 64, 65, 19_999)


def below(recs, nonce):
    """How many records of an ascending (k, 2) array have a nonce below `nonce`."""
    return int(np.searchsorted(recs[:, 1], np.uint64(nonce)))


# ---- the multi-round list ---------------------------------------------------

def k_cases(oracle_mod, c):
    """A multi-round case's requests: T its mid target, full the window's hits
    (the memoised oracle list), N = len(full), j the hits below c["edge"], ks;
    the answer of k is full[:k]."""
    full = mid_list(oracle_mod, c)
    n, j = len(full), below(full, c["edge"])
    return {"T": mid_target(c), "full": full, "N": n, "j": j, "ks": (1, K_MID, j, j + 1, n + 3)}


# ---- the piece windows ------------------------------------------------------

def piece_cases(oracle_mod, c):
    """Requests over F.piece_window(c): [(kind, T, k, want), ...] with want the
    first k hits of the window as an array; kind "dense" (T = 2^64 - 1: every
    nonce) or "sparse" (2^64 / 64; j the hits below the digit-count change)."""
    def build():
        lo, hi = F.piece_window(c)
        hs = window_hashes(oracle_mod, c)
        every = np.stack([hs, np.arange(lo, hi + 1, dtype=np.uint64)], axis=1)
        assert int(hs.max()) < MAX
        out = [("dense", MAX, k, every[:k]) for k in PIECE_DENSE_KS]
        hits = every[hs < np.uint64(PIECE_SPARSE)]
        n, j = len(hits), below(hits, c["edge"])
        out += [("sparse", PIECE_SPARSE, k, hits[:k]) for k in (1, j, j + 1, n, n + 3)]
        return out
    return memo(("find_k_many_piece_cases", c["name"]), build)


# ---- windows one fused launch cannot hold -----------------------------------

PREFIX_MAX_HASH = 2**64 // 1000


def _drawn(oracle_mod, L, nonce, seed):
    """The first message of the seeded draw whose hash at `nonce` is below
    2^64 / 1000, with that hash."""
    rng = random.Random(seed)
    while True:
        m = message(L, rng)
        h = oracle_mod.c_hash(m, nonce)
        if h < PREFIX_MAX_HASH:
            return m, h


def prefix_cases(oracle_mod):
    """Per (L, d) of F.UNFUSED, B = 10^(d-1) the first nonce of the chained
    f = 5 segment, lo = B - 10^5, hi = lo + 10^7 - 1: a list of
    {L, d, B, what, req, want, prefix} with `prefix` the hits of [lo, B - 1]:
      last    T = hash(B - 1) + 1, k = the hits of [lo, B - 1]: the k-th hit is
              the last fused nonce
      first   another message, T = hash(B) + 1, k = the hits of [lo, B]: the
              k-th hit is the first unfused nonce
      more    last's message and T with k + 5: the rest supplies five hits
      empty   [B, B + 10^7 - 1] at last's T, k = 3: no fusible prefix"""
    def build():
        out = []
        for L, d in F.UNFUSED:
            B = 10**(d - 1)
            lo = B - F.UNFUSED_PREFIX
            hi = lo + F.UNFUSED_SPAN - 1
            base = {"L": L, "d": d, "B": B}
            m, h = _drawn(oracle_mod, L, B - 1, 4400 + L)
            T = h + 1
            pre = oracle_list(oracle_mod, m, lo, B - 1, T)
            out.append({**base, "what": "last", "req": (m, lo, hi, T, len(pre)), "want": pre,
                        "prefix": pre})
            k5 = len(pre) + 5
            out.append({**base, "what": "more", "req": (m, lo, hi, T, k5), "prefix": pre,
                        "want": oracle_first_k(oracle_mod, m, lo, hi, T, k5)})
            out.append({**base, "what": "empty", "req": (m, B, B + F.UNFUSED_SPAN - 1, T, 3),
                        "prefix": [],
                        "want": oracle_first_k(oracle_mod, m, B, B + F.UNFUSED_SPAN - 1, T, 3)})
            m, h = _drawn(oracle_mod, L, B, 4500 + L)
            T = h + 1
            upto = oracle_list(oracle_mod, m, lo, B, T)
            out.append({**base, "what": "first", "req": (m, lo, hi, T, len(upto)), "want": upto,
                        "prefix": upto[:-1]})
        return out
    return memo("find_k_many_prefix", build)


def mix_requests(oracle_mod):
    """The 65 requests of F.mix_requests (odd indices and the 65th with an
    empty prefix, even ones launched and dead in turn) with a k of 1..12 each:
    [(kind, request, want), ...]."""
    def build():
        rng = random.Random(6517)
        out = []
        for kind, r in F.mix_requests(oracle_mod):
            req = r + (rng.randrange(1, 13),)
            out.append((kind, req, [] if kind == "dead" else oracle_first_k(oracle_mod, *req)))
        return out
    return memo("find_k_many_mix", build)


# ---- a stop word of 0 -------------------------------------------------------

ZERO_HI = 10**6
ZERO_BUF = 1 << 15            # HM_OPT_FIND_K_BUF of these runs: every hit of the range fits


def _zero_message(oracle_mod, i, below_):
    """(i, m, hash(m, 0)) of the first m = b"stop word zero <i>" from i on whose
    hash at nonce 0 is below `below_` (about 3 us a try)."""
    while True:
        m = b"stop word zero %d" % i
        h = oracle_mod.c_hash(m, 0)
        if h < below_:
            return i, m, h
        i += 1


def zero_cases(oracle_mod):
    """Requests over [0, 10^6] with T = hash(m, 0) + 1, so that nonce 0 is the
    first hit: {"alone": (request, want), "easy": [(request, want), ...]}.
      alone  m taken until hash(m, 0) < 2^64 / 10^6 and no other nonce of the
             range hits: with k = 1 the only record is nonce 0, so the stop word
             can only be lowered to 0, and by a task of one step
      easy   m taken until hash(m, 0) < 2^64 / 100: k = 1 (the k-th hit is
             nonce 0, but at a hit per few hundred nonces another wave's record
             may take slot 0 and bound the stop word) and k = 2 (nonce 0 and a
             later hit)"""
    def build():
        i = 0
        while True:
            i, m, h = _zero_message(oracle_mod, i, 2**64 // 10**6)
            if oracle_first_k(oracle_mod, m, 0, ZERO_HI, h + 1, 2) == [(h, 0)]:
                break
            i += 1
        alone = ((m, 0, ZERO_HI, h + 1, 1), [(h, 0)])
        _, m, h = _zero_message(oracle_mod, 0, 2**64 // 100)
        two = oracle_first_k(oracle_mod, m, 0, ZERO_HI, h + 1, 2)
        return {"alone": alone,
                "easy": [((m, 0, ZERO_HI, h + 1, 1), [(h, 0)]), ((m, 0, ZERO_HI, h + 1, 2), two)]}
    return memo("find_k_many_zero", build)


# ---- the clamp: a model of the fused launch's tasks --------------------------

PIECES = (1, 2, 5, 10)        # np of a task id: 1 a whole task, else HM_OPT_FUSED_TAIL's pieces
PARTS = (1, 2, 5, 10)         # HM_OPT_FUSED_PARTS


def piece_of(b, e, pp, np_):
    """fk_piece_of: piece pp of np_ of the run [b, e)."""
    n = -(-(e - b) // np_)
    x = min(b + pp * n, e)
    return x, min(x + n, e)


def _units(seg, per_chunk, step):
    """launch_units (seg_walk.cpp): the first and the last unit kept."""
    P = 10**seg["V"]
    t, nt = seg["lo"] // P, seg["hi"] // P - seg["lo"] // P + 1
    per_tile = -(-10**_lane_digits(seg) // 64) * per_chunk
    first = (seg["lo"] - t * P) // step // 64 * per_chunk if seg["lo"] > t * P else 0
    bl = (t + nt - 1) * P
    last = (nt - 1) * per_tile + ((seg["hi"] - bl) // step // 64 + 1) * per_chunk - 1
    return first, last


def _lane_digits(seg):
    return seg["V"] - (seg["f"] if seg["kind"] == _lib.HM_KIND_CHAINED else 2)


def seg_tasks(seg, nparts=1):
    """The tasks plan_fused (scan.cpp) gives a fusible segment."""
    if seg["kind"] == _lib.HM_KIND_GENERIC:
        return -(-(seg["hi"] - seg["lo"] + 1) // 640)
    if seg["kind"] == _lib.HM_KIND_TILED:
        first, last = _units(seg, 1, 100)
        return (last - first + 1) * 10 * nparts
    first, last = _units(seg, 10**seg["f"] // seg["tch"], 10**seg["f"])
    return (last - first + 1) * -(-seg["tch"] // 100)


def last_task_los(seg, nparts, np_):
    """task_lo (the formulas at the top of fused_tasks.hpp) of every non-empty
    piece of np_ of the segment's LAST task.  Within a segment ids ascend in
    task_lo, so these are the segment's largest."""
    hi = seg["hi"]
    if seg["kind"] == _lib.HM_KIND_GENERIC:
        base = seg["lo"] + (hi - seg["lo"]) // 640 * 640
        return [base + 64 * jb for jb, je in (piece_of(0, 10, pp, np_) for pp in range(np_))
                if jb < je]
    P = 10**seg["V"]
    bl = hi // P * P
    if seg["kind"] == _lib.HM_KIND_TILED:
        chunk = (hi - bl) // 100 // 64          # the last unit kept (launch_units)
        steps = 10 // nparts
        b = (nparts - 1) * steps                # t1 = 9, the last part
        return [bl + chunk * 6400 + 90 + t0b
                for t0b, t0e in (piece_of(b, b + steps, pp, np_) for pp in range(np_)) if t0b < t0e]
    p10f, tch = 10**seg["f"], seg["tch"]
    chunk = (hi - bl) // p10f // 64
    tc, tpu = p10f // tch - 1, -(-tch // 100)
    piece = -(-tch // tpu)
    t_begin = tc * tch + (tpu - 1) * piece
    t_end = min(tc * tch + tch, t_begin + piece)
    return [bl + chunk * 64 * p10f + tb
            for tb, te in (piece_of(t_begin, t_end, pp, np_) for pp in range(np_)) if tb < te]


def fused_prefix(m, lo, hi, generic):
    """The segments a batch launch fuses (batch.cpp: the longest fusible prefix)."""
    out = []
    for s in _lib.debug_plan(m, lo, hi, generic):
        if not F.fusible(s):
            break
        out.append(s)
    return out


CLAMP_BACK = (1, 64, 260, 640, 900, 6437, 10**5)   # nonces ahead of the digit-count change
CLAMP_AHEAD = 1000


def clamp_search():
    """Lengths 0..130 x every digit-count change 10^d (d = 1..19), default and
    forced-generic plans, windows [10^d - a, 10^d + 999] for a of CLAMP_BACK and,
    for d <= 7, [10^d - a, 10^(d+1) + 999] (a whole digit segment in the middle);
    and, for the multi-device piece boundaries (2 and 3 devices), the windows
    around them.  Every segment of the fused prefix but its last, every
    HM_OPT_FUSED_PARTS, every piece count: (whole, pieces, windows, boundary) with
    whole / pieces the sorted (kind name, np) at which some task has task_lo >
    seg_hi, windows the number searched, and boundary the segment counts of the
    piece-boundary windows."""
    def build():
        found, windows = set(), 0
        for generic in (False, True):
            for L in range(MAX_LEN + 1):
                m = bytes(L)
                for d in DIGITS[:-1]:
                    E = 10**d
                    his = [E + CLAMP_AHEAD - 1] + ([10 * E + CLAMP_AHEAD - 1] if d <= 7 else [])
                    for hi in his:
                        for a in CLAMP_BACK:
                            if a > E:
                                continue
                            segs = fused_prefix(m, E - a, hi, generic)
                            windows += 1
                            for s in segs[:-1]:
                                for nparts in PARTS if s["kind"] == _lib.HM_KIND_TILED else (1,):
                                    for np_ in PIECES:
                                        if max(last_task_los(s, nparts, np_)) > s["hi"]:
                                            found.add((KINDS[s["kind"]], np_))
        boundary = set()
        for ndev in (2, 3):
            for generic in (False, True):
                for L in (0, 20, 55, 99):
                    Bd = _piece_boundary(bytes(L), ndev, generic)
                    boundary.add(len(_lib.debug_plan(bytes(L), Bd - PIECE_HALF, Bd + PIECE_HALF,
                                                     generic)))
        return (sorted(f for f in found if f[1] == 1), sorted(f for f in found if f[1] > 1),
                windows, sorted(boundary))
    return memo("find_k_many_clamp_search", build)


# windows of the GPU clamp cases: (name, L, generic, lo, hi); every id of such a
# launch is a piece on any device of >= 4 CUs (a handful of tasks)
CLAMP_WINDOWS = [("fast-d3", 20, False, 10**3 - 260, 10**3 + 999),
                 ("fast-d3-d4-d5", 77, False, 10**3 - 260, 10**4 + 259),
                 ("generic-d12", 60, True, 10**12 - 900, 10**12 + 999),
                 ("generic-d19", 130, True, 10**19 - 260, 10**19 + 1299)]
CLAMP_TAILS = (2, 5, 10)


def clamp_cases(oracle_mod):
    """Per window of CLAMP_WINDOWS: m, lo, hi, generic, segs (its plan), tasks
    (seg_tasks summed) and reqs = [(request, want, where), ...]: at 2^64 / 8 the
    k-th hit in the last segment with hits in the first ("later"), and at
    2^64 / 4 the k-th hit the last hit of the first segment ("earlier")."""
    def build():
        rng = random.Random(3131)
        out = []
        for name, L, generic, lo, hi in CLAMP_WINDOWS:
            m = message(L, rng)
            segs = _lib.debug_plan(m, lo, hi, generic)
            reqs = []
            for T, where in ((2**64 // 8, "later"), (2**64 // 4, "earlier")):
                hits = oracle_list(oracle_mod, m, lo, hi, T)
                a = sum(n <= segs[0]["hi"] for _, n in hits)
                b = sum(n < segs[-1]["lo"] for _, n in hits)
                k = b + 2 if where == "later" else a
                reqs.append(((m, lo, hi, T, k), hits[:k], where))
            out.append({"name": name, "m": m, "lo": lo, "hi": hi, "generic": generic, "segs": segs,
                        "tasks": sum(seg_tasks(s) for s in segs), "reqs": reqs})
        return out
    return memo("find_k_many_clamp_cases", build)


def clamped_pieces(segs, tail):
    """(segment index, task_lo) of the pieces of `tail` of a non-final segment's
    last task whose task_lo lies above the segment's end."""
    return [(i, t) for i, s in enumerate(segs[:-1]) for t in last_task_los(s, 1, tail)
            if t > s["hi"]]


# ---- the host tests ---------------------------------------------------------

def test_k_cases_suit_the_early_exit(oracle_mod):
    """Every multi-round case: 1 <= j < N, 1000 < N, N + 3 <= HM_FIND_K_MAX and
    N <= the slice of HM_OPT_FIND_K_BUF = 2^22 (no launch can overflow it); the
    1000th hit lies in the first quarter of the window's nonces, so a kernel that
    lowers `stop` when slot k fills skips tasks of the later rounds; at the small
    cases' four hits per step some five hits near index 1000 lie within 64
    nonces, so a step's hits straddle a slot boundary near k."""
    cases = F.multi_round_cases()
    assert len(cases) == 68
    quarter, js = [], []
    for c in cases:
        kc = k_cases(oracle_mod, c)
        full, n, j = kc["full"], kc["N"], kc["j"]
        assert 1 <= j < n, (c["name"], j, n)
        assert K_MID < n and n + 3 <= _lib.HM_FIND_K_MAX and n <= FIND_K_BUF, (c["name"], n)
        assert span_of(c) <= 27_000_000, c["name"]
        assert kc["ks"] == (1, 1000, j, j + 1, n + 3)
        assert int(full[j - 1, 1]) < c["edge"] <= int(full[j, 1])
        at = int(full[K_MID - 1, 1]) - c["lo"]
        assert 4 * at < span_of(c), (c["name"], at, span_of(c))
        quarter.append(at / span_of(c))
        js.append(j)
        if is_small(c):
            near = (full[900:1100, 1] - full[900, 1]).astype(np.int64)
            assert int((near[4:] - near[:-4]).min()) < 64, c["name"]
    print(f"find_k multi-round list: {len(cases)} cases, j from {min(js)} to {max(js)}, the 1000th "
          f"hit at most {max(quarter):.4f} of the window in")


def test_piece_cases(oracle_mod):
    sub = F.split_subset()
    assert len(sub) == 8
    for what, c in sub.items():
        lo, hi = F.piece_window(c)
        cases = piece_cases(oracle_mod, c)
        dense = [x for x in cases if x[0] == "dense"]
        sparse = [x for x in cases if x[0] == "sparse"]
        assert [k for _, _, k, _ in dense] == [20_000, 1, 63, 64, 65, 19_999]
        for _, T, k, want in dense:
            assert T == MAX and len(want) == k and int(want[0, 1]) == lo
            assert np.array_equal(want[:, 1], np.arange(lo, lo + k, dtype=np.uint64))
        assert int(dense[0][3][-1, 1]) == hi
        n = len(sparse[3][3])
        j = sparse[1][2]
        assert [k for _, _, k, _ in sparse] == [1, j, j + 1, n, n + 3] and 1 <= j < n, (what, j, n)
        assert [len(w) for _, _, _, w in sparse] == [1, j, j + 1, n, n]
        assert int(sparse[1][3][-1, 1]) < c["edge"] <= int(sparse[2][3][-1, 1])
        for _, T, _, want in sparse:
            assert int(want[:, 0].max()) < T == PIECE_SPARSE


def test_prefix_windows_plan_as_meant(oracle_mod):
    """A fusible first segment ending at B - 1, then a chained f = 5 segment;
    the empty-prefix window is one unfusible segment; the k-th hit is B - 1
    ("last") and B ("first") exactly; 2 <= k <= 500."""
    cases = prefix_cases(oracle_mod)
    assert [(c["L"], c["d"]) for c in cases[::4]] == F.UNFUSED and len(cases) == 4 * len(F.UNFUSED)
    for c in cases:
        m, lo, hi, T, k = c["req"]
        B = c["B"]
        segs = _lib.debug_plan(m, lo, hi)
        if c["what"] == "empty":
            assert lo == B and k == 3 and len(c["want"]) == 3 and c["prefix"] == []
            assert len(segs) == 1 and not F.fusible(segs[0]) and segs[0]["f"] == 5, segs
            continue
        assert (lo, hi) == (B - 10**5, B - 10**5 + 10**7 - 1)
        assert len(segs) == 2 and F.fusible(segs[0]) and not F.fusible(segs[1]), segs
        assert segs[0]["hi"] == B - 1 and segs[1]["kind"] == _lib.HM_KIND_CHAINED
        assert segs[1]["f"] == 5
        assert len(fused_prefix(m, lo, hi, False)) == 1
        assert len(c["want"]) == k and c["want"][:len(c["prefix"])] == c["prefix"]
        assert all(h < T and lo <= n <= hi for h, n in c["want"])
        assert [n for _, n in c["want"]] == sorted({n for _, n in c["want"]})
        if c["what"] == "last":
            assert 2 <= k <= 500 and c["want"][-1][1] == B - 1 and c["want"][-1][0] == T - 1
            assert len(c["prefix"]) == k
        elif c["what"] == "first":
            assert k >= 2 and c["want"][-1] == (T - 1, B) and len(c["prefix"]) == k - 1
        else:
            assert c["what"] == "more" and len(c["prefix"]) == k - 5
            assert all(n >= B for _, n in c["want"][-5:])
    print("prefix cases: k = " + " ".join(f"{c['what']}:{c['req'][4]}" for c in cases))


def test_mix_and_zero_requests(oracle_mod):
    mix = mix_requests(oracle_mod)
    kinds = [k for k, _, _ in mix]
    assert len(mix) == 65 and all(k == "empty" for k in kinds[1::2]) and kinds[64] == "empty"
    assert {"launched", "dead"} == set(kinds[0:64:2])
    assert {r[4] for _, r, _ in mix} == set(range(1, 13))
    for kind, (m, lo, hi, T, k), want in mix:
        assert len(want) <= k
        if kind == "launched":
            assert all(F.fusible(s) for s in _lib.debug_plan(m, lo, hi))
        elif kind == "empty":
            assert fused_prefix(m, lo, hi, False) == [] and len(want) == k
        else:
            assert want == []
    launched = [w for kind, _, w in mix if kind == "launched"]
    assert any(launched) and any(len(w) < r[4] for kind, r, w in mix if kind == "launched")
    zero = zero_cases(oracle_mod)
    ra, wa = zero["alone"]
    assert ra[1:3] == (0, ZERO_HI) and ra[3] == wa[0][0] + 1 < 2**64 // 10**6 and wa[0][1] == 0
    assert oracle_list(oracle_mod, ra[0], 0, ZERO_HI, ra[3]) == wa      # no other hit
    (r1, w1), (r2, w2) = zero["easy"]
    assert r1[1:3] == (0, ZERO_HI) and r1[3] == w1[0][0] + 1 < 2**64 // 100 and w1[0][1] == 0
    assert len(w2) == 2 and w2[0] == w1[0] and 0 < w2[1][1] <= ZERO_HI and w2[1][0] < r2[3]
    # up to a hit per 100 nonces: a round of tasks would overrun the default slice
    assert len(oracle_list(oracle_mod, r1[0], 0, ZERO_HI, r1[3])) <= ZERO_BUF
    for m in (ra[0], r1[0]):
        for g in (False, True):
            assert all(F.fusible(s) for s in _lib.debug_plan(m, 0, ZERO_HI, g))


def test_the_clamp_is_reached_by_generic_pieces_only(oracle_mod):
    """fk_enter skips a task when min(task_lo, seg_hi) > stop.  The clamp
    matters for a task with task_lo > seg_hi in a segment that is not the
    launch's last.  The search (clamp_search) finds:

      - no WHOLE task of a non-final segment has task_lo > seg_hi, under any
        plan or HM_OPT_FUSED_PARTS.  A non-final segment of a batch launch ends
        at a digit-count change 10^d - 1; the multi-device piece boundary cuts
        no batch window (a request goes whole to one device: one segment).  A
        tiled or chained task's lane 0 starts at a multiple of 100 (of 10^f)
        plus a loop value below 100 (10^f), and 10^d is a multiple of both, so
        lane 0's first value stays at or below the segment's end; a whole
        generic task starts at seg_lo + 640 k <= seg_hi.  The same holds for the
        pieces of tiled and chained tasks.
      - a guided-tail PIECE of a generic segment's last task starts at
        seg_lo + 640 k + 64 jb, which lies above seg_hi whenever that task
        holds fewer than 64 jb + 1 nonces.  The last task of a non-final
        segment runs as pieces when the later segments hold fewer tasks than
        the launch's last partial round: on the fast path for ranges across
        10^1 .. 10^4 (generic at up to five digits), and under
        HM_OPT_FORCE_GENERIC at any digit-count change.

    So the clamp is reachable, by generic pieces alone; clamp_cases() are GPU
    cases on such windows, with HM_OPT_FUSED_TAIL = 2 (the default), 5 and 10."""
    whole, pieces, windows, boundary = clamp_search()
    print(f"clamp search: {windows} windows; whole tasks with task_lo > seg_hi in a non-final "
          f"segment: {whole}; pieces: {pieces}; segments of a window across the multi-device "
          f"piece boundary: {boundary}")
    assert windows > 30_000
    assert whole == []
    assert pieces == [("generic", 2), ("generic", 5), ("generic", 10)]
    assert boundary == [1]
    for c in clamp_cases(oracle_mod):
        segs = c["segs"]
        assert len(segs) >= 2 and all(F.fusible(s) for s in segs), c["name"]
        assert all(s["kind"] == _lib.HM_KIND_GENERIC for s in segs[:-1]), c["name"]
        assert 2 <= c["tasks"] <= 40
        for tail in CLAMP_TAILS:
            assert clamped_pieces(segs, tail), (c["name"], tail)
        (later, wl, _), (earlier, we, _) = c["reqs"]
        assert len(wl) == later[4] >= 3 and wl[0][1] <= segs[0]["hi"] and wl[-1][1] >= segs[-1]["lo"]
        assert len(we) == earlier[4] >= 1 and we[-1][1] <= segs[0]["hi"]


def test_the_task_model_counts_the_lists_tasks():
    """seg_tasks against what is known of the lists: a keyed segment of a
    multi-round case holds at least the whole tasks its docstring promises, and
    no more tasks than one per 64 nonces."""
    for c in F.multi_round_cases():
        segs, keys = F.plan_of(c)
        for s, k in zip(segs, keys):
            n = seg_tasks(s)
            assert n >= F.least_tasks(s, k), (c["name"], n)
            assert n <= (s["hi"] - s["lo"] + 1) // 64 + 2000, (c["name"], n)
        assert seg_tasks(segs[c["ki"]]) >= F.ROUNDS * F.ROUND


def _rejects(got, want, name):
    with pytest.raises(AssertionError):
        check_list(got, want, name)


def test_the_comparison_rejects_corrupted_answers(oracle_mod):
    """check_list, the one comparison of the GPU module, accepts the oracle's
    answer and rejects it with a record dropped, one duplicated, two swapped,
    a hash off by one, one record short, one long, and the k lowest HASHES in
    place of the k lowest nonces."""
    m, lo, hi, T, k = b"find_k checker", 99_000, 101_999, 2**64 // 16, 40
    full = as_array(oracle_list(oracle_mod, m, lo, hi, T))
    assert len(full) > 100
    want = full[:k]
    assert np.array_equal(want, as_array(oracle_first_k(oracle_mod, m, lo, hi, T, k)))
    check_list(want.copy(), want)
    swapped = want.copy()
    swapped[[7, 8]] = want[[8, 7]]
    off = want.copy()
    off[11, 0] += np.uint64(1)
    lowest = full[np.argsort(full[:, 0], kind="stable")[:k]]
    lowest = lowest[np.argsort(lowest[:, 1], kind="stable")]
    assert lowest.shape == want.shape and not np.array_equal(lowest, want)
    bad = {"dropped": np.concatenate([np.delete(want, 7, axis=0), full[k:k + 1]]),
           "dropped, short": np.delete(want, 7, axis=0),
           "duplicated": np.insert(want, 7, want[7], axis=0)[:k],
           "duplicated, long": np.insert(want, 7, want[7], axis=0),
           "swapped": swapped, "hash off by one": off, "lowest hashes": lowest,
           "one short": want[:-1], "one long": full[:k + 1]}
    for name, got in bad.items():
        _rejects(got, want, name)
    _rejects(None, want, "no answer")
    _rejects(as_array([]), want, "empty")
    check_list(as_array([]), as_array([]))

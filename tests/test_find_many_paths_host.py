"""The case lists of tests/test_gpu_find_many_paths.py and what they reach.

hm_find_many's kernel (hm_fused_find_kernel, fused_find_kernels.hip) has its
own task decoders, its own piece arithmetic and its own id-to-piece decode.  The
lists of tests/test_gpu_find_many.py keep every request below one round of the
grid's waves, so there every id is a half-task piece that a wave takes as its
slot.  The lists here are pure functions (fixed seeds, no GPU); this module
builds them and checks on the host, through the planner's debug export, that
they reach what they are meant to reach.  A case is classified by the plan of
the exact window it runs (tests/test_collect_layouts_host.py has the keys).

Multi-round list.  A fused launch at HM_OPT_GRID_PER_CU = 1 has 4 waves per CU,
ROUND = 1024 on the 256 CUs the list is sized for.  A task holds at most
640 nonces (tiled, generic, chained f = 1) or 6400 (chained f = 2..4: 64 lanes x
100 loop values), so a segment of n nonces has at least ceil(n / that) tasks.
The guided tail splits the launch's last tasks, fewer than ROUND of them.  A
case's keyed segment therefore holds at least
    ceil(n_keyed / task) - max(0, ROUND - 1 - (lower bound of the later tasks))
whole tasks, and a window is taken only where that is >= 3 * ROUND.  Two window
shapes, both across a digit-count change:
    A   5000 nonces of d - 1 digits, then the keyed segment: 4 rounds of d digits
    B   the keyed segment: the last 3 rounds of d digits, then one round (of
        640-nonce tasks) of d + 1 digits
The fusible layouts (tiled, generic, chained with f <= 4) are chosen from the
message length and the digit count alone (plan.cpp: only the chained layout with
f >= 5 weighs the range), so a fusible key that shows in no window of the search
shows at digit counts only whose whole segment is smaller than three rounds.
The search below finds exactly that, and names those keys.
"""
import random

from distributed_bitcoinminer_amd import _lib
from tests.test_collect_layouts_host import (DIGITS, MAX, MAX_LEN, instantiation, key_of, memo,
                                             message, segment, segment_keys)

CUS = 256                     # the device the lists are sized for
ROUND = 4 * CUS               # waves of a launch at HM_OPT_GRID_PER_CU = 1
ROUNDS = 3
SHORT = 5000                  # shape A: nonces ahead of the keyed segment
EARLY = 2**64 // 2**12
LIST_ITEMS = 16               # items the GPU module deals the multi-round list into
SPLIT_GRID = 16               # HM_OPT_GRID_PER_CU of the all-piece runs
SPLIT_HALF = 10_000           # the all-piece windows: this many nonces either side of the edge


def task_nonces(key):
    """The most nonces one task of the key's layout holds."""
    return 6400 if key[0] == "chained" and key[1] >= 2 else 640


def fusible(seg):
    """scan.cpp fusible(), per segment: chained only with f <= 4 and no epochs."""
    return not (seg["kind"] == _lib.HM_KIND_CHAINED and (seg["f"] > 4 or seg["fe"] != seg["f"]))


def least_tasks(seg, key):
    return -(-(seg["hi"] - seg["lo"] + 1) // task_nonces(key))


def whole_tasks(segs, keys, ki):
    """A lower bound of the tasks of segment ki that run whole (module docstring)."""
    later = sum(least_tasks(s, k) for s, k in zip(segs[ki + 1:], keys[ki + 1:]))
    return least_tasks(segs[ki], keys[ki]) - max(0, ROUND - 1 - later)


def _windows(d):
    """The search's windows at digit count d: (shape, lo, hi, index of the keyed segment)."""
    dlo, dhi = segment(d)
    out = []
    for task in (640, 6400):
        n = (ROUNDS + 1) * ROUND * task
        if d >= 2 and dlo + n - 1 <= dhi:
            out.append(("A", dlo - SHORT, dlo + n - 1, 1))
        n = ROUNDS * ROUND * task
        if d < 20 and dhi + 1 - n >= dlo:
            out.append(("B", dhi + 1 - n, dhi + ROUND * 640, 0))
    return out


def search():
    """(reached, seen).  reached: (key, generic) -> the smallest window (then the
    shortest message) whose keyed segment plans to the key with >= 3 rounds of
    whole tasks, as (nonces // 10^5, other shape, L, d, shape, lo, hi, ki).  seen: (key, generic) ->
    the digit counts at which any plan of (L, d) gave the fusible key: the
    digit segment, its first 1000 nonces, and every segment of every window."""
    def build():
        reached, seen = {}, {}
        for generic in (False, True):
            for L in range(MAX_LEN + 1):
                m = bytes(L)
                for d in DIGITS:
                    dlo, dhi = segment(d)
                    for lo, hi in ((dlo, dhi), (dlo, min(dhi, dlo + 999))):
                        for s in _lib.debug_plan(m, lo, hi, generic):
                            if fusible(s):
                                seen.setdefault((key_of(s, L), generic), set()).add(d)
                    for shape, lo, hi, ki in _windows(d):
                        segs = _lib.debug_plan(m, lo, hi, generic)
                        keys = [key_of(s, L) for s in segs]
                        for s, k in zip(segs, keys):
                            if fusible(s):
                                seen.setdefault((k, generic), set()).add(s["d"])
                        if len(segs) != 2 or not all(fusible(s) for s in segs):
                            continue
                        if whole_tasks(segs, keys, ki) < ROUNDS * ROUND:
                            continue
                        # the two shapes differ by 5000 nonces: a key takes the shape
                        # its own digits pick, so that the list holds both evenly
                        odd = sum(int(x) for x in keys[ki][1:]) % 2
                        c = ((hi - lo + 1) // 10**5, shape != "AB"[odd], L, d, shape, lo, hi, ki)
                        if c < reached.get((keys[ki], generic), (MAX,)):
                            reached[(keys[ki], generic)] = c
        return reached, seen
    return memo("find_many_search", build)


def wanted(key, generic):
    """The list holds the fast path's keys other than generic, and the generic
    kernel under HM_OPT_FORCE_GENERIC with one and two tail blocks: the fast path
    plans generic segments at up to 5 digits only, far below one round."""
    return generic == (key[0] == "generic")


def multi_round_cases():
    """One case per reached key, sorted: m, lo, hi, key, ki (the keyed segment),
    generic (run under HM_OPT_FORCE_GENERIC), L, d, shape, edge (the digit-count
    change inside the window), name."""
    def build():
        rng = random.Random(1301)
        out = []
        for (key, generic), (_, _, L, d, shape, lo, hi, ki) in sorted(search()[0].items(), key=str):
            if not wanted(key, generic):
                continue
            edge = segment(d)[0] if shape == "A" else segment(d)[1] + 1
            out.append({"m": message(L, rng), "lo": lo, "hi": hi, "key": key, "ki": ki,
                        "generic": generic, "L": L, "d": d, "shape": shape, "edge": edge,
                        "name": "-".join(str(int(x)) if not isinstance(x, str) else x
                                         for x in key)})
        return out
    return memo("find_many_multi_round", build)


def plan_of(c, lo=None, hi=None):
    segs = _lib.debug_plan(c["m"], c["lo"] if lo is None else lo, c["hi"] if hi is None else hi,
                           c["generic"])
    return segs, [key_of(s, c["L"]) for s in segs]


def answers(oracle_mod, c):
    """The oracle's answers for a multi-round case, computed once: mn (the
    range's (hash, nonce) minimum), reqs and want (targets min: none; min + 1:
    the argmin; the larger of the two halves' minima + 1: a hit in either half;
    2^64 / 2^12: an early hit), and first_not_argmin for the two-hit target."""
    def build():
        m, lo, hi = c["m"], c["lo"], c["hi"]
        mid = lo + (hi - lo) // 2
        a, b = oracle_mod.c_scan(m, lo, mid), oracle_mod.c_scan(m, mid + 1, hi)
        mn = min(a, b)
        two = max(a[0], b[0]) + 1
        targets = [mn[0], mn[0] + 1, two, EARLY]
        want = [None, mn, oracle_mod.c_find(m, lo, hi, two), oracle_mod.c_find(m, lo, hi, EARLY)]
        return {"mn": mn, "reqs": [(m, lo, hi, T) for T in targets], "want": want,
                "first_not_argmin": want[2][1] != mn[1]}
    return memo(("find_many_answers", c["name"]), build)


# ---- the split options: a subset of the list, and all-piece windows ----------

def split_subset():
    """name -> case: the keys HM_OPT_FUSED_PARTS x HM_OPT_FUSED_TAIL run on."""
    cases = multi_round_cases()

    def pick(what, pred):
        return next(c for c in cases if pred(c["key"])), what
    t = lambda k: k[0] == "tiled"       # noqa: E731  (W1, straddle, trailer, V, q, lane3)
    picks = [pick("plain", lambda k: t(k) and not (k[2] or k[3] or k[6]) and k[5] == 6),
             pick("straddle", lambda k: t(k) and k[2] and not k[3] and k[5] == 5),
             pick("trailer", lambda k: t(k) and k[3] and not k[2]),
             pick("q5", lambda k: t(k) and k[5] == 5 and not (k[2] or k[3] or k[6])),
             pick("q3", lambda k: t(k) and k[5] == 3),
             pick("chained1", lambda k: k[0] == "chained" and k[1] == 1),
             pick("chained4", lambda k: k[0] == "chained" and k[1] == 4),
             pick("generic", lambda k: k == ("generic", 2))]
    return {what: c for c, what in picks}


def piece_window(c):
    """A window of 2 * 10^4 nonces across the case's digit-count change: at
    HM_OPT_GRID_PER_CU = 16 it has fewer tasks than a tenth of a round, so every
    id is a piece and each task has HM_OPT_FUSED_TAIL of them."""
    return c["edge"] - SPLIT_HALF, c["edge"] + SPLIT_HALF - 1


def records(hashes):
    """Indices of the strict prefix minima of `hashes`: at target hashes[i] + 1
    the first hit is i exactly."""
    out, best = [], None
    for i, h in enumerate(hashes):
        if best is None or h < best:
            out.append(i)
            best = h
    return out


def piece_answers(oracle_mod, c):
    """Requests over piece_window(c) with the answers: target min (none) and,
    for every prefix minimum of the window's hashes, its hash + 1 -- the first
    hit is that nonce, the last of them the argmin."""
    def build():
        lo, hi = piece_window(c)
        hs = [oracle_mod.c_hash(c["m"], n) for n in range(lo, hi + 1)]
        rec = records(hs)
        reqs = [(c["m"], lo, hi, min(hs))] + [(c["m"], lo, hi, hs[i] + 1) for i in rec]
        return reqs, [None] + [(hs[i], lo + i) for i in rec]
    return memo(("find_many_piece_answers", c["name"]), build)


# ---- windows one fused launch cannot hold ------------------------------------

UNFUSED = [(48, 20), (50, 18), (112, 20), (120, 12)]   # (length, digits of the f = 5 segment)
UNFUSED_SPAN = 10**7
UNFUSED_PREFIX = 10**5
BOUNDARY_BACK = 4096


def _chained_over_4(seg):
    return seg["kind"] == _lib.HM_KIND_CHAINED and seg["f"] > 4


def unfused_cases(oracle_mod):
    """Per (length, d) of UNFUSED, B = 10^(d-1) the first nonce of the chained
    f = 5 segment: m, B, `empty` = [B, B + 10^7) (no fusible prefix) and
    `partial` = [B - 10^5, B - 10^5 + 10^7) (a fusible prefix of 10^5 nonces);
    per window the minimum (mn), and for `partial` the prefix's minimum (pre)
    and the rest's (rest), the message drawn until rest < pre: at rest + 1 the
    prefix holds no hit."""
    def build():
        out = []
        for L, d in UNFUSED:
            B = 10**(d - 1)
            rng = random.Random(7700 + L)
            for _ in range(8):
                m = message(L, rng)
                pre = oracle_mod.c_scan(m, B - UNFUSED_PREFIX, B - 1)
                rest = oracle_mod.c_scan(m, B, B - UNFUSED_PREFIX + UNFUSED_SPAN - 1)
                if rest[0] < pre[0]:
                    break
            tail = oracle_mod.c_scan(m, B - UNFUSED_PREFIX + UNFUSED_SPAN, B + UNFUSED_SPAN - 1)
            out.append({"m": m, "L": L, "d": d, "B": B, "pre": pre, "rest": rest,
                        "empty": (B, B + UNFUSED_SPAN - 1),
                        "partial": (B - UNFUSED_PREFIX, B - UNFUSED_PREFIX + UNFUSED_SPAN - 1),
                        "mn_empty": min(rest, tail), "mn_partial": min(pre, rest)})
        return out
    return memo("find_many_unfused", build)


def boundary_cases(oracle_mod):
    """Per (length, d) of UNFUSED two requests whose first hit is the last fused
    nonce (B - 1) and the first unfused one (B): target = hash(n*) + 1, lo one
    past the last earlier nonce (of the BOUNDARY_BACK before n*) whose hash is
    <= hash(n*), the message drawn until lo <= B - 64.
    [{m, L, d, B, lo, hi, T, nstar, want}, ...]."""
    def build():
        out = []
        for L, d in UNFUSED:
            B = 10**(d - 1)
            for nstar in (B - 1, B):
                rng = random.Random(9100 + 2 * L + (nstar == B))
                for _ in range(4000):
                    m = message(L, rng)
                    h = oracle_mod.c_hash(m, nstar)
                    if any(oracle_mod.c_hash(m, n) <= h for n in range(B - 64, nstar)):
                        continue
                    lo = nstar - BOUNDARY_BACK
                    for n in range(B - 65, lo - 1, -1):
                        if oracle_mod.c_hash(m, n) <= h:
                            lo = n + 1
                            break
                    out.append({"m": m, "L": L, "d": d, "B": B, "lo": lo,
                                "hi": lo + UNFUSED_SPAN - 1, "T": h + 1, "nstar": nstar,
                                "want": (h, nstar)})
                    break
        return out
    return memo("find_many_boundary", build)


def mix_requests(oracle_mod):
    """65 requests, (kind, request) each: odd indices have an empty prefix (on
    two devices every request of device 1), even ones alternate launched and
    dead (lo > hi, then target 0), the 65th -- a chunk of its own -- has an
    empty prefix."""
    def build():
        rng = random.Random(6500)
        cases = unfused_cases(oracle_mod)
        out = []
        for i in range(65):
            if i % 2 or i == 64:
                c = cases[(i // 2) % len(cases)]
                out.append(("empty", (c["m"], c["empty"][0], c["empty"][1],
                                      2**64 // (1000 * (i + 1)))))
            elif i % 4 == 0:
                a = rng.randrange(10**rng.randrange(1, 19))
                out.append(("launched", (b"mix %d" % i, a, a + rng.randrange(3000),
                                         2**64 // 1000)))
            else:
                out.append(("dead", (b"mix %d" % i, 5, 4, MAX) if i % 8 == 2 else
                            (b"mix %d" % i, 0, 10**5, 0)))
        return out
    return memo("find_many_mix", build)




# ---- the host tests ---------------------------------------------------------

# Fusible keys the planner gives somewhere in lengths 0..130 x digits 1..20 that
# no window reaches with three rounds of whole tasks.  Tiled: V = 5 (q = 3) shows
# at d = 5 and V = 6 (q = 4) at d = 6 only, as (W1, straddle, trailer, lane3).
UNREACHED_TILED = {
    5: [(1, 0, 0, 0), (2, 0, 0, 0), (2, 1, 0, 0), (3, 0, 0, 0), (3, 1, 0, 0), (4, 0, 0, 0),
        (4, 1, 0, 0), (5, 0, 0, 0), (5, 1, 0, 0), (6, 0, 0, 0), (6, 1, 0, 0), (7, 0, 0, 0),
        (7, 1, 0, 0), (8, 0, 0, 0), (8, 1, 0, 0), (9, 0, 0, 0), (9, 1, 0, 0), (10, 0, 0, 0),
        (10, 1, 0, 0), (11, 0, 0, 0), (11, 1, 0, 0), (12, 0, 0, 0), (12, 1, 0, 0), (13, 0, 0, 0),
        (13, 0, 1, 0), (13, 1, 0, 0), (14, 0, 1, 0), (14, 1, 1, 0), (15, 0, 1, 0), (15, 1, 1, 0)],
    6: [(2, 0, 0, 0), (2, 1, 0, 1), (3, 0, 0, 0), (3, 1, 0, 1), (4, 0, 0, 0), (4, 1, 0, 1),
        (5, 0, 0, 0), (5, 1, 0, 1), (6, 0, 0, 0), (6, 1, 0, 1), (7, 0, 0, 0), (7, 1, 0, 1),
        (8, 0, 0, 0), (8, 1, 0, 1), (9, 0, 0, 0), (9, 1, 0, 1), (10, 0, 0, 0), (10, 1, 0, 1),
        (11, 0, 0, 0), (11, 1, 0, 1), (12, 0, 0, 0), (12, 1, 0, 1), (13, 0, 0, 0), (13, 0, 1, 0),
        (13, 1, 0, 1), (14, 0, 1, 0), (14, 1, 1, 1), (15, 0, 1, 0), (15, 1, 1, 1)],
}
# Chained (f, fe, tch, q): q < 5 lane digits at d = 3..7.
UNREACHED_CHAINED = [(1, 1, 10, 2), (1, 1, 10, 3), (1, 1, 10, 4), (2, 2, 100, 2), (2, 2, 100, 3),
                     (2, 2, 100, 4), (3, 3, 1000, 2), (3, 3, 1000, 3), (3, 3, 1000, 4),
                     (4, 4, 1000, 2), (4, 4, 1000, 3)]


def test_multi_round_list_reaches_every_kernel():
    """Every tiled instantiation, chained f = 1..4 and the generic kernel with
    one and two tail blocks have a case whose keyed segment holds >= 3 rounds of
    whole tasks; every case has two fusible segments across a digit-count change;
    the keys left out are exactly those whose digit segments are too short."""
    _, seen = search()
    cases = multi_round_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        segs, keys = plan_of(c)
        assert len(segs) == 2 and all(fusible(s) for s in segs), c
        assert segs[0]["d"] + 1 == segs[1]["d"] and segs[1]["lo"] == c["edge"], c
        assert keys[c["ki"]] == c["key"], c
        assert whole_tasks(segs, keys, c["ki"]) >= ROUNDS * ROUND, c
        assert c["hi"] - c["lo"] + 1 <= (ROUNDS + 1) * ROUND * task_nonces(c["key"]) + SHORT, c
        assert c["generic"] == (c["key"][0] == "generic")
    keys = {c["key"] for c in cases}
    insts = {instantiation(k) for k in keys if k[0] == "tiled"}
    assert insts == {instantiation(k) for k in segment_keys() if k[0] == "tiled"}
    assert len(insts) == 31
    assert {k[1] for k in keys if k[0] == "chained"} == {1, 2, 3, 4}
    assert {k for k in keys if k[0] == "generic"} == {("generic", 1), ("generic", 2)}

    # the fast path's own generic segments: five digits at the most
    assert max(d for (k, g), ds in seen.items() if k[0] == "generic" and not g for d in ds) <= 5
    universe = {k for k, g in seen if wanted(k, g)}
    assert {k for k in segment_keys()
            if k[0] == "tiled" or (k[0] == "chained" and k[1] <= 4)} <= universe
    left = universe - keys
    for k in left:
        # nowhere the key shows does the digit segment hold three rounds of its tasks
        assert all(segment(d)[1] - segment(d)[0] + 1 < ROUNDS * ROUND * task_nonces(k)
                   for d in seen[(k, False)]), (k, sorted(seen[(k, False)]))
    tiled_left = {V: sorted((k[1], int(k[2]), int(k[3]), int(k[6]))
                            for k in left if k[0] == "tiled" and k[4] == V) for V in (5, 6)}
    chained_left = sorted(k[1:] for k in left if k[0] == "chained")
    print(f"multi-round list: {len(cases)} keys reached ({len(insts)} tiled instantiations, "
          f"chained f = {sorted({k[1] for k in keys if k[0] == 'chained'})}, generic nb = "
          f"{sorted(k[1] for k in keys if k[0] == 'generic')}), "
          f"{sum(c['shape'] == 'A' for c in cases)} of shape A and "
          f"{sum(c['shape'] == 'B' for c in cases)} of shape B; {len(left)} fusible keys proven "
          f"unreachable (digit segment below three rounds): {len(tiled_left[5])} tiled V = 5 at "
          f"d = 5, {len(tiled_left[6])} tiled V = 6 at d = 6, {len(chained_left)} chained "
          f"q < 5 at d = 3..7")
    assert tiled_left == UNREACHED_TILED
    assert chained_left == UNREACHED_CHAINED
    assert len(left) == sum(map(len, tiled_left.values())) + len(chained_left)


def test_two_hit_targets_tell_first_from_lowest(oracle_mod):
    """Over the list, the two-hit target's first hit is not the range's argmin in
    at least a third of the cases: a kernel that returned the lowest hash among
    the hits instead of the first hit would fail there."""
    cases = multi_round_cases()
    n = 0
    for c in cases:
        a = answers(oracle_mod, c)
        lo, hi = c["lo"], c["hi"]
        assert a["want"][0] is None and a["want"][1] == a["mn"]
        first = a["want"][2]
        assert first is not None and lo <= first[1] <= a["mn"][1]
        assert first[1] <= lo + (hi - lo) // 2          # the first half holds a hit
        assert a["want"][3] is not None and a["want"][3][1] < lo + 10**5
        n += a["first_not_argmin"]
    print(f"two-hit targets: first hit is not the argmin in {n} of {len(cases)} cases")
    assert 3 * n >= len(cases)


def test_split_subset_and_piece_windows():
    sub = split_subset()
    assert len({c["name"] for c in sub.values()}) == len(sub) == 8
    k = {what: c["key"] for what, c in sub.items()}
    assert k["plain"][:4] == ("tiled", 1, False, False) and k["straddle"][2] and k["trailer"][3]
    assert k["q5"][5] == 5 and k["q3"][5] == 3 and k["chained1"][1] == 1 and k["chained4"][1] == 4
    for c in sub.values():
        lo, hi = piece_window(c)
        segs, keys = plan_of(c, lo, hi)
        assert len(segs) == 2 and all(fusible(s) for s in segs) and keys[c["ki"]] == c["key"], c
        # far fewer tasks than a tenth of the 16 * 4 * CUS waves, whatever the parts: a
        # tiled segment of n nonces touches at most n // 6400 + 2 lane chunks of 100 tasks
        assert (SPLIT_HALF // 6400 + 2) * 100 * 2 * 10 <= SPLIT_GRID * ROUND
    assert records([5, 7, 5, 3, 9, 3, 1]) == [0, 3, 6]


def test_unfused_windows_plan_as_meant(oracle_mod):
    """The empty-prefix window is one chained f = 5 segment; the partial one a
    fusible segment of 10^5 nonces and then that; the boundary requests keep a
    prefix of >= 64 nonces and hit exactly at B - 1 and at B."""
    cases = unfused_cases(oracle_mod)
    assert [(c["L"], c["d"]) for c in cases] == UNFUSED
    for c in cases:
        segs = _lib.debug_plan(c["m"], *c["empty"])
        assert len(segs) == 1 and _chained_over_4(segs[0]) and segs[0]["f"] == 5, segs
        segs = _lib.debug_plan(c["m"], *c["partial"])
        assert len(segs) == 2 and fusible(segs[0]) and _chained_over_4(segs[1]), segs
        assert (segs[0]["lo"], segs[0]["hi"]) == (c["B"] - UNFUSED_PREFIX, c["B"] - 1)
        assert segs[0]["kind"] == _lib.HM_KIND_CHAINED and segs[0]["f"] == 4
        assert c["rest"][0] < c["pre"][0] and c["rest"][1] >= c["B"]
        assert c["mn_partial"] == c["rest"] and c["mn_empty"][1] >= c["B"]
    bounds = boundary_cases(oracle_mod)
    assert len(bounds) == 2 * len(UNFUSED)
    for b in bounds:
        assert b["nstar"] in (b["B"] - 1, b["B"]) and b["lo"] <= b["B"] - 64, b
        segs = _lib.debug_plan(b["m"], b["lo"], b["hi"])
        assert len(segs) == 2 and fusible(segs[0]) and _chained_over_4(segs[1]), segs
        assert segs[0]["hi"] == b["B"] - 1
        assert oracle_mod.c_find(b["m"], b["lo"], b["hi"], b["T"]) == b["want"]
    print("unfused windows: " + ", ".join(
        f"L={c['L']} d={c['d']}" for c in cases) + "; boundary prefixes of "
        + " ".join(str(b["B"] - b["lo"]) for b in bounds) + " nonces")
    kinds = [k for k, _ in mix_requests(oracle_mod)]
    assert len(kinds) == 65 and all(k == "empty" for k in kinds[1::2]) and kinds[64] == "empty"
    assert {"launched", "dead"} == set(kinds[0:64:2])
    for kind, (m, lo, hi, T) in mix_requests(oracle_mod):
        if kind == "launched":
            assert all(fusible(s) for s in _lib.debug_plan(m, lo, hi))

"""The case lists of tests/test_gpu_collect_layouts.py and what they cover.

hm_collect has 32 tiled kernel instantiations of its own
(hm_collect_tiled_kernel<W1, STRADDLE, TRAILER>), one chained and one generic
kernel, each looked up by name on first use.  The GPU module runs them on
four deterministic case lists; the lists are pure functions (fixed seeds, no
GPU) built here, and this module checks on the host, through the planner's
debug export, that they reach what they are meant to reach.

Every case is classified by the plan of THE EXACT RANGE IT RUNS, never by the
plan of its digit segment: the chained layout with >= 5 final-block digits is
picked by modelled cost, which depends on how well the range fills its lane
chunks, so a sub-range of a segment can plan differently from the segment.

A layout key is
    ("generic", nb)
    ("tiled", W1, straddle, trailer, V, q, lane3)
    ("chained", f, fe, tch, q)
with q the lane digits (tiled: V - 2, chained: V - f) and nb the tail blocks.

Runnable ranges.  A range is runnable when it lies in one digit segment, has
at most 3 * 10^8 nonces, and its span is the one its own key asks for:
  * V <= 6: two whole tiles of 10^V nonces, 10^V // 16 + 7 nonces of the tile
    before and 10^V // 32 + 5 of the tile after (at most 2 093 762 nonces);
    where the digit segment is a single tile (d == V), the whole segment;
  * V >= 7: min(2 * 10^V + 12345, 3 * 10^8) nonces, fewer only where the
    digit segment itself is shorter: two whole tiles where that many nonces
    hold them, else a tile boundary a third of the way in (at the end of a
    lane chunk of 64 * 10^f nonces for chained f >= 5, so that the chunks are
    well filled); where the digit segment is a single tile, its top.
Each (length, digit count) has up to two runnable ranges: one found from its
segment's plan and one from the plan of a tiny range (the layout the planner
falls back to where the chained one does not pay).  Chained f >= 7 is out of
reach: one lane chunk alone is 6.4 * 10^8 nonces, so no runnable range plans
to it, and the segments that plan to it run tiled here.
"""
import random

from distributed_bitcoinminer_amd import _lib

MAX = (1 << 64) - 1
MAX_LEN = 130
DIGITS = range(1, 21)
BIG_SPAN_CAP = 3 * 10**8
WINDOW_HALF = 10**5
WINDOW_CAP = 1 << 24          # HM_COLLECT_CAP_MAX: a dense window's records must fit
EDGE_WINDOW = 300
EDGE_GROUPS = [range(1, 6), range(6, 11), range(11, 16), range(16, 21)]
EDGE_IDS = ["d1-5", "d6-10", "d11-15", "d16-20"]
PIECE_HALF = 70_000
KINDS = {_lib.HM_KIND_GENERIC: "generic", _lib.HM_KIND_TILED: "tiled",
         _lib.HM_KIND_CHAINED: "chained"}


# ---- keys -------------------------------------------------------------------

def segment(d):
    """The inclusive digit segment of d-digit nonces."""
    return (0 if d == 1 else 10**(d - 1)), min(10**d - 1, MAX)


def tail_blocks(L, d):
    """Tail blocks of a message of L bytes with d digits: the prefix
    remainder, the digits, 0x80 and the 8-byte bit length in 1 or 2 blocks."""
    return 1 if (L + 1) % 64 + d + 9 <= 64 else 2


def key_of(seg, L):
    kind = KINDS[seg["kind"]]
    if kind == "generic":
        return (kind, tail_blocks(L, seg["d"]))
    if kind == "tiled":
        return (kind, seg["W1"], bool(seg["straddle"]), bool(seg["trailer"]), seg["V"],
                seg["V"] - 2, bool(seg["lane3"]))
    return (kind, seg["f"], seg["fe"], seg["tch"], seg["V"] - seg["f"])


def plan_key(m, lo, hi, generic=False):
    """The key of the one segment [lo, hi] plans to."""
    segs = _lib.debug_plan(m, lo, hi, generic)
    assert len(segs) == 1 and (segs[0]["lo"], segs[0]["hi"]) == (lo, hi), (m.hex(), lo, hi, segs)
    return key_of(segs[0], len(m))


def key_V(key):
    """Digits that vary inside a tile of the key (0: generic, no tiles)."""
    if key[0] == "generic":
        return 0
    return key[4] if key[0] == "tiled" else key[1] + key[4]


def instantiation(key):
    return key[1:4] if key[0] == "tiled" else None


_MEMO = {}


def memo(name, fn):
    if name not in _MEMO:
        _MEMO[name] = fn()
    return _MEMO[name]


def segment_keys(max_len=MAX_LEN):
    """key -> [(L, d), ...] over lengths 0..max_len x digit counts 1..20, by
    the plan of the whole digit segment.  The plan depends on the length of
    the message only, never on its bytes."""
    def build():
        out = {}
        for L in range(max_len + 1):
            m = bytes(L)
            for d in DIGITS:
                out.setdefault(plan_key(m, *segment(d)), []).append((L, d))
        return out
    return memo(("segment_keys", max_len), build)


def message(L, rng):
    return bytes(rng.randrange(256) for _ in range(L))


# ---- segment edges ----------------------------------------------------------

def edge_cases(group):
    """Every length 0..130 x every digit count of EDGE_GROUPS[group]: the
    first and the last (at most) 300 nonces of the digit segment.
    [(m, d, lo, hi), ...]."""
    def build():
        digits = EDGE_GROUPS[group]
        rng = random.Random(2300 + digits[0])
        out = []
        for L in range(MAX_LEN + 1):
            m = message(L, rng)
            for d in digits:
                dlo, dhi = segment(d)
                out.append((m, d, dlo, min(dhi, dlo + EDGE_WINDOW - 1)))
                out.append((m, d, max(dlo, dhi - EDGE_WINDOW + 1), dhi))
        return out
    return memo(("edge_cases", group), build)


# ---- whole tiles ------------------------------------------------------------

def _small_range(d, V):
    dlo, dhi = segment(d)
    P = 10**V
    if d <= V:                      # the digit segment is one (part of a) tile
        return dlo, dhi
    t = dlo // P + 3                # dlo is a multiple of P: nine or more tiles in the segment
    return t * P - (P // 16 + 7), (t + 2) * P + (P // 32 + 5) - 1


def _big_range(d, V, chained_f):
    dlo, dhi = segment(d)
    P = 10**V
    span = min(2 * P + 12345, BIG_SPAN_CAP)
    if span >= dhi - dlo + 1:
        return dlo, dhi
    if d <= V:                      # one tile, no boundary: its top, the highest lane values
        return dhi - span + 1, dhi
    B = (dlo // P + 4) * P if d > V else dlo + (dhi - dlo) // 2 // 10**5 * 10**5
    if B + span > dhi:
        B = dlo + (dhi - dlo) // 2 // 10**5 * 10**5
    # two whole tiles where 2 * 10^V + 12345 nonces are allowed, else B a third of the way in
    lo = B - 6172 if span > 2 * P else B - span // 3 - 777
    if chained_f >= 5:              # start on a lane chunk: the planner's cost model fills it
        C = 64 * 10**chained_f
        lo = B - ((10**(V - chained_f) % 64 or 64) * 10**chained_f + span // 3 // C * C)
    lo = max(lo, dlo)
    return lo, lo + span - 1


def range_for(key, d):
    V = key_V(key)
    if key[0] == "generic":
        return None
    if V <= 6:
        return _small_range(d, V)
    return _big_range(d, V, key[1] if key[0] == "chained" else 0)


def runnable_ranges(L, d):
    """The runnable ranges of (L, d) (module docstring): [(lo, hi, key), ...]
    with key the plan of exactly [lo, hi], at most two, distinct keys."""
    m = bytes(L)
    dlo, dhi = segment(d)
    out = {}
    for start in (plan_key(m, dlo, dhi), plan_key(m, dlo, min(dhi, dlo + 999))):
        key = start
        for _ in range(4):
            r = range_for(key, d)
            if r is None:
                break
            got = plan_key(m, *r)
            if got == key:
                out.setdefault(key, (r[0], r[1], key))
                break
            key = got
    return list(out.values())


def runnable_keys():
    """key -> [(L, d, lo, hi), ...] of every runnable range over lengths
    0..130 x digit counts 1..20."""
    def build():
        out = {}
        for L in range(MAX_LEN + 1):
            for d in DIGITS:
                for lo, hi, key in runnable_ranges(L, d):
                    out.setdefault(key, []).append((L, d, lo, hi))
        return out
    return memo("runnable_keys", build)


def whole_tiles(lo, hi, V):
    """Tiles of 10^V nonces wholly inside [lo, hi]."""
    P = 10**V
    return max(0, (hi + 1) // P - (lo + P - 1) // P)


def dense_window(m, key, lo, hi):
    """A window of [lo, hi] across a tile boundary that plans to `key`:
    [B - 10^5, B + 10^5), widened for chained f >= 5 to whole lane chunks on
    both sides of B (the planner gives a window that fills its chunks badly
    the tiled layout).  Where [lo, hi] is a digit segment of a single tile
    there is no boundary: the window is its last 2 * 10^5 nonces, the highest
    lane values.  (wlo, whi, how) with how one of "boundary", "widened",
    "no boundary", or None: no window of at most 2^24 nonces plans to the key."""
    V = key_V(key)
    P = 10**V
    sides = [(WINDOW_HALF, WINDOW_HALF)]
    if key[0] == "chained" and key[1] >= 5:
        f, q = key[1], key[4]
        C = 64 * 10**f
        last = (10**q % 64 or 64) * 10**f      # the last lane chunk of a tile: part filled
        sides += sorted(((last + j * C, i * C) for j in range(3) for i in (1, 2)), key=sum)
    if lo // P == hi // P:
        for a in [2 * WINDOW_HALF] + sorted({a for a, _ in sides[1:]}):
            if a <= WINDOW_CAP and lo <= hi + 1 - a and plan_key(m, hi + 1 - a, hi) == key:
                return hi + 1 - a, hi, "no boundary"
        return None
    for B in range((lo // P + 1) * P, hi + 1, P):
        for a, b in sides:
            if a + b <= WINDOW_CAP and lo <= B - a and B + b - 1 <= hi and \
                    plan_key(m, B - a, B + b - 1) == key:
                return B - a, B + b - 1, "boundary" if (a, b) == sides[0] else "widened"
    return None


def tile_cases():
    """One case per runnable key, as (small, big): small = keys with V <= 6
    (checked against the CPU oracle), big = the others (checked against
    independent kernels).  A case: m, d, lo, hi, key, segkey (the plan of its
    digit segment), tiles (whole tiles in range) and, big only, window."""
    def build():
        rng = random.Random(8800)
        small, big = [], []
        for key in sorted(runnable_keys(), key=str):
            V = key_V(key)
            where = runnable_keys()[key]
            # a digit segment longer than one tile where there is one; then the shortest message
            L, d, lo, hi = min(where, key=lambda w: (w[1] <= V, w[0], w[1]))
            m = message(L, rng)
            case = {"m": m, "d": d, "lo": lo, "hi": hi, "key": key,
                    "segkey": plan_key(m, *segment(d)), "tiles": whole_tiles(lo, hi, V)}
            if V <= 6:
                small.append(case)
            else:
                case["window"] = dense_window(m, key, lo, hi)
                big.append(case)
        return small, big
    return memo("tile_cases", build)


def parts(cases, n, size=lambda c: c["hi"] - c["lo"]):
    """cases dealt into n parts, the largest first, so that every part gets
    its share of them."""
    by_size = sorted(cases, key=size, reverse=True)
    return [by_size[i::n] for i in range(n)]


def window_cases():
    """The big cases that have a dense window."""
    return [c for c in tile_cases()[1] if c["window"]]


def window_size(c):
    return c["window"][1] - c["window"][0]


# ---- piece boundaries -------------------------------------------------------

def piece_boundary(m, ndev, generic):
    """The first multiple of the multi-device piece span, as PieceWalk computes
    it: ndev * 2^40 nonces, rounded down to whole tiles of 10^V where the
    segment is not generic."""
    span = ndev << 40
    seg = _lib.debug_plan(m, span - PIECE_HALF, span + PIECE_HALF, generic)[0]
    if seg["kind"] != _lib.HM_KIND_GENERIC:
        span = span // 10 ** seg["V"] * 10 ** seg["V"]
        again = _lib.debug_plan(m, span - PIECE_HALF, span + PIECE_HALF, generic)
        assert len(again) == 1 and again[0]["V"] == seg["V"] and again[0]["kind"] == seg["kind"]
    assert seg["d"] == 13 and 10**12 + PIECE_HALF < span < 10**13 - PIECE_HALF
    return span


def piece_cases(ndev, generic):
    """Two seeded messages with the ranges around their first piece boundary B:
    [(m, B, [(lo, hi), ...]), ...]."""
    rng = random.Random(5100 + 10 * ndev + generic)
    out = []
    for _ in range(2):
        m = message(rng.randrange(0, 100), rng)
        B = piece_boundary(m, ndev, bool(generic))
        out.append((m, B, [(B - PIECE_HALF, B + PIECE_HALF), (B, B + PIECE_HALF),
                           (B - PIECE_HALF, B - 1), (B - 1, B), (B, B)]))
    return out


# ---- the host tests ---------------------------------------------------------

def _tiled(keys):
    return {instantiation(k) for k in keys if k[0] == "tiled"}


def test_planner_reaches_31_tiled_instantiations():
    """Lengths 0..130 x digit counts 1..20 reach 31 of the 32 instantiations;
    <13, true, true> is planned for no length 0..400."""
    insts = _tiled(segment_keys())
    assert len(insts) == 31, sorted(insts)
    every = {(w, s, t) for w in range(1, 14) for s in (False, True) for t in (False,)} | \
            {(w, s, True) for w in (13, 14, 15) for s in (False, True)}
    assert len(every) == 32 and every - insts == {(13, True, True)}
    wide = _tiled(segment_keys(400))
    assert wide == insts and (13, True, True) not in wide
    nongeneric = [k for k in segment_keys() if k[0] != "generic"]
    print(f"planner, lengths 0..{MAX_LEN} x d 1..20: {len(insts)} tiled instantiations, "
          f"{len(nongeneric)} non-generic keys by digit segment")


def test_old_sweep_coverage_reported(oracle_mod):
    """What the 150-case seeded sweep of tests/test_gpu_collect.py reaches,
    by the plan of each case's own range under its own options: reported, not
    asserted -- the figure the lists below replace."""
    from tests.test_gpu_collect import SWEEP_CASES, SWEEP_SEED, sweep_cases
    insts, keys, full = set(), set(), set()
    for c in sweep_cases(oracle_mod, SWEEP_SEED, SWEEP_CASES, epochs=False):
        for seg in _lib.debug_plan(c["m"], c["lo"], c["hi"],
                                   bool(c["opts"][_lib.HM_OPT_FORCE_GENERIC])):
            key = key_of(seg, len(c["m"]))
            if key[0] != "generic":
                keys.add(key)
            if key[0] == "tiled":
                insts.add(instantiation(key))
                if seg["hi"] - seg["lo"] + 1 >= 6400:
                    full.add(instantiation(key))
    missing = sorted(_tiled(segment_keys()) - insts)
    print(f"old collect sweep (seed {SWEEP_SEED}, {SWEEP_CASES} cases): {len(insts)} of 31 tiled "
          f"instantiations ({len(full)} with a segment of >= 6400 nonces), {len(keys)} "
          f"non-generic keys; never planned: "
          + " ".join(f"<{w},{int(s)},{int(t)}>" for w, s, t in missing))


def test_segment_edges_cover_every_kernel():
    """The fast half of the segment-edge list reaches all 31 tiled
    instantiations, the chained layout, and the generic kernel with one and
    two tail blocks; the forced-generic half is generic throughout."""
    fast, forced, n = set(), set(), 0
    for g in range(len(EDGE_GROUPS)):
        cases = edge_cases(g)
        assert cases == edge_cases(g)
        n += len(cases)
        for m, d, lo, hi in cases:
            assert 1 <= hi - lo + 1 <= EDGE_WINDOW and segment(d)[0] <= lo <= hi <= segment(d)[1]
            fast.add(plan_key(m, lo, hi))
            forced.add(plan_key(m, lo, hi, True))
    assert n == 131 * 20 * 2
    insts = _tiled(fast)
    print(f"segment edges: {n} windows; fast: {len(insts)} tiled instantiations, "
          f"{sum(k[0] == 'chained' for k in fast)} chained keys, generic nb "
          f"{sorted(k[1] for k in fast if k[0] == 'generic')}, {len(fast)} keys; forced generic: "
          f"nb {sorted(k[1] for k in forced)}")
    assert insts == _tiled(segment_keys()) and len(insts) == 31
    assert any(k[0] == "chained" for k in fast)
    assert {("generic", 1), ("generic", 2)} <= fast
    assert forced == {("generic", 1), ("generic", 2)}


def test_whole_tile_lists_cover_every_runnable_key():
    """The two whole-tile lists hold exactly one case per key the planner gives
    for runnable ranges; every case's key is the plan of its own range."""
    small, big = tile_cases()
    universe = runnable_keys()
    for c in small + big:
        assert plan_key(c["m"], c["lo"], c["hi"]) == c["key"], c
        assert segment(c["d"])[0] <= c["lo"] <= c["hi"] <= segment(c["d"])[1]
    keys = [c["key"] for c in small + big]
    assert len(keys) == len(set(keys)) and set(keys) == set(universe)
    assert not any(k[0] == "generic" for k in keys)

    # the small list: V <= 6 against the CPU oracle
    for c in small:
        V = key_V(c["key"])
        assert V <= 6 and c["hi"] - c["lo"] + 1 <= 2_100_000, c
        if c["d"] > V:      # two whole tiles and a partial tile at each end
            assert c["tiles"] == 2 and c["lo"] % 10**V and (c["hi"] + 1) % 10**V, c
        else:               # the digit segment is a single tile: all of it
            assert (c["lo"], c["hi"]) == segment(c["d"]) and c["d"] == V, c
    # the big list: V >= 7 against independent kernels
    for c in big:
        V = key_V(c["key"])
        dlo, dhi = segment(c["d"])
        want = min(2 * 10**V + 12345, BIG_SPAN_CAP, dhi - dlo + 1)
        assert V >= 7 and c["hi"] - c["lo"] + 1 == want, c
        if c["window"]:
            wlo, whi, how = c["window"]
            assert c["lo"] <= wlo < whi <= c["hi"]
            assert 2 * WINDOW_HALF <= whi - wlo + 1 <= WINDOW_CAP
            assert plan_key(c["m"], wlo, whi) == c["key"]
            if how == "no boundary":    # the whole digit segment is one tile
                assert c["d"] == V and whi == c["hi"]
            else:
                assert wlo // 10**V + 1 == whi // 10**V

    two = _tiled(c["key"] for c in small + big if c["tiles"] >= 2)
    two_small = _tiled(c["key"] for c in small if c["tiles"] >= 2)
    assert two == _tiled(segment_keys()) and len(two) == 31, sorted(two)
    # an instantiation has two whole tiles of at most 10^6 nonces only where some
    # (length, d) gives it V <= 6 on a digit segment longer than one tile: the
    # others hold V <= 6 only at d == V, and have their whole tiles in the big list
    can = _tiled(k for k, where in segment_keys().items()
                 if k[0] == "tiled" and k[4] <= 6 and any(d > k[4] for _, d in where))
    assert two_small == can, sorted(can - two_small)
    lanes = {(k[4], k[6]) for k in segment_keys() if k[0] == "tiled"}
    got_small = {(c["key"][4], c["key"][6]) for c in small if c["key"][0] == "tiled"}
    got_big = {(c["key"][4], c["key"][6]) for c in big if c["key"][0] == "tiled"}
    assert got_small == {vl for vl in lanes if vl[0] <= 6} == {(5, False), (6, False), (6, True)}
    assert got_big == {vl for vl in lanes if vl[0] >= 7} == {(7, False), (7, True), (8, False)}
    chained_f = {c["key"][1] for c in small + big if c["key"][0] == "chained"}
    assert chained_f == {1, 2, 3, 4, 5, 6}, chained_f

    differ = sorted((c["segkey"], c["key"]) for c in small + big if c["segkey"] != c["key"])
    lost = sorted(k for k in segment_keys() if k[0] != "generic" and k not in universe)
    assert all(k[0] == "chained" and k[1] >= 7 for k in lost), lost
    widened = [c["key"] for c in big if c["window"] and c["window"][2] == "widened"]
    single = [c["key"] for c in big if c["window"] and c["window"][2] == "no boundary"]
    none = [c["key"] for c in big if not c["window"]]
    # a window of <= 2^24 nonces fills at most a quarter of one 6.4 * 10^7-nonce
    # lane chunk of chained f = 6: the planner never gives it that layout
    assert all(k[0] == "chained" and k[1] == 5 for k in widened), widened
    assert all(k[0] == "chained" and k[1] == 6 for k in none), none
    print(f"whole tiles, small (V <= 6, CPU oracle): {len(small)} keys, "
          f"{len(two_small)} tiled instantiations with two whole tiles, "
          f"{sum(c['d'] == key_V(c['key']) for c in small)} keys whose digit segment is one tile")
    print(f"whole tiles, big (V >= 7, independent kernels): {len(big)} keys, "
          f"{len(_tiled(c['key'] for c in big))} tiled instantiations; both lists: {len(keys)} "
          f"keys = every runnable key, {len(two)} tiled instantiations with two whole tiles")
    print(f"keys by digit segment that no runnable range plans to: {len(lost)} "
          f"(chained f = {sorted({k[1] for k in lost})}); cases whose digit segment plans "
          f"differently from the range run: {len(differ)}")
    print(f"dense windows: {len(widened)} keys widened to whole lane chunks {widened}, "
          f"{len(none)} keys with no window of <= 2^24 nonces {none}, {len(single)} keys whose "
          f"digit segment is one tile (no boundary) {single}")


def test_piece_cases_straddle_the_boundary():
    for ndev in (2, 3):
        for generic in (0, 1):
            cases = piece_cases(ndev, generic)
            assert cases == piece_cases(ndev, generic) and len(cases) == 2
            for m, B, ranges in cases:
                assert len(ranges) == 5 and ranges[0] == (B - PIECE_HALF, B + PIECE_HALF)
                span = ndev << 40
                assert span - 10**8 < B <= span
                for lo, hi in ranges:
                    assert len(_lib.debug_plan(m, lo, hi, bool(generic))) == 1

"""The CPU oracle pinned against published SHA-256 KATs and the golden fixtures
(tests/golden/gen_golden.py, an independent hashlib restatement)."""
import hashlib

import pytest

MAX = (1 << 64) - 1


def test_fips_kats(oracle_mod, golden):
    for k in golden["fips_kats"]:
        data = k["text"].encode() if k["text"] is not None else b"a" * k["repeat_a"]
        assert oracle_mod.c_sha256(data).hex() == k["sha256"]
        assert hashlib.sha256(data).hexdigest() == k["sha256"]


def test_sha256_all_padding_lengths(oracle_mod):
    for n in range(0, 260):
        data = bytes((i * 131 + n) & 0xFF for i in range(n))
        assert oracle_mod.c_sha256(data) == hashlib.sha256(data).digest(), n


def test_hash_kats(oracle_mod, golden):
    for k in golden["hash_kats"]:
        m, n, h = bytes.fromhex(k["msg_hex"]), int(k["nonce"]), int(k["hash"])
        assert oracle_mod.c_hash(m, n) == h, (k["name"], n)
    for k in golden["hash_kats"][::17]:
        m, n, h = bytes.fromhex(k["msg_hex"]), int(k["nonce"]), int(k["hash"])
        assert oracle_mod.py_hash(m, n) == h


def test_scan_kats(oracle_mod, golden):
    for k in golden["scan_kats"]:
        m, lo, hi = bytes.fromhex(k["msg_hex"]), int(k["lo"]), int(k["hi"])
        if hi >= lo and hi - lo > 400_000:
            continue  # the 10^7 case is covered on the GPU and by test_config1_oracle
        exp = (int(k["hash"]), int(k["nonce"]))
        assert oracle_mod.c_scan(m, lo, hi, threads=4) == exp, (k["name"], lo, hi)
        assert oracle_mod.c_scan(m, lo, hi, threads=1) == exp
        if "sum" in k:  # coverage checksum of hm_scan_checked
            assert oracle_mod.c_scan_sum(m, lo, hi, threads=3) == \
                (exp, int(k["sum"]), int(k["count"])), (k["name"], lo, hi)


def test_scan_sum_thread_invariance_and_python(oracle_mod):
    for m, lo, hi in [(b"bradfitz", 0, 2000), (b"q" * 56, 99_000, 101_000), (b"", MAX - 40, MAX),
                      (b"x", 5, 4)]:
        exp = oracle_mod.py_scan_sum(m, lo, hi)
        for t in (1, 2, 7):
            assert oracle_mod.c_scan_sum(m, lo, hi, threads=t) == exp, (m, lo, hi, t)


def test_config1_oracle(oracle_mod):
    # reference client: `client host:port bradfitz 10000000` -> Result 356393768206 7645578
    assert oracle_mod.c_scan(b"bradfitz", 0, 10**7, threads=8) == (356393768206, 7645578)


def test_miner_eval_kats(oracle_mod, golden):
    for k in golden["miner_eval_kats"]:
        m = bytes.fromhex(k["msg_hex"])
        lo, up = int(k["lower"]), int(k["upper"])
        exp = (int(k["hash"]), int(k["nonce"]))
        assert oracle_mod.c_miner_eval(m, lo, up) == exp
        assert oracle_mod.py_miner_eval(m, lo, up) == exp


@pytest.mark.parametrize("threads", [1, 2, 3, 7, 16])
def test_thread_split_invariance(oracle_mod, threads):
    for lo, hi in [(0, 0), (0, 1), (5, 9), (99_990, 100_009), (MAX - 20, MAX), (MAX, MAX)]:
        assert oracle_mod.c_scan(b"x", lo, hi, threads) == oracle_mod.py_scan(b"x", lo, hi)


# ---- c_find / py_find: the first nonce below a target ------------------------

FIND_THREADS = (1, 2, 7, 16)
# bradfitz, [0, 10^7]: the first nonce below each target (tests/test_find_host.py)
FIND_KATS = [(2**64 // 10**3, (6697378768932333, 203)),
             (2**64 // 10**5, (158752571039048, 91989)),
             (2**64 // 10**6, (7182149750005, 2351907))]


def _find_targets(oracle_mod, m, lo, hi):
    """Dense, sparse and boundary targets for one range: every first-hit
    position from `lo` to none."""
    best = oracle_mod.py_scan(m, lo, hi)[0]
    mid = oracle_mod.py_hash(m, lo + (hi - lo) // 2)
    return [MAX, 2**63, 2**64 // 10, 2**64 // 10**3, 2**32 + 1, 2**32, 1, 0,
            best + 1, best, mid + 1, mid]


def test_find_against_python(oracle_mod):
    """c_find == py_find across every digit boundary, at the top of the nonce
    space and on one-nonce and empty ranges, for every thread count."""
    ranges = [(max(0, 10**d - 150), min(MAX, 10**d + 150)) for d in range(1, 20)]
    ranges += [(MAX - 400, MAX), (MAX - 1, MAX), (MAX, MAX), (0, 0), (7, 7), (0, 1), (5, 4),
               (MAX, 0)]
    for i, (lo, hi) in enumerate(ranges):
        m = bytes((37 * i + 11 * j) & 0xFF for j in range((i * 7) % 131))
        if lo > hi:
            for t in FIND_THREADS:
                assert oracle_mod.c_find(m, lo, hi, MAX, threads=t) is None
            assert oracle_mod.py_find(m, lo, hi, MAX) is None
            continue
        for T in _find_targets(oracle_mod, m, lo, hi):
            exp = oracle_mod.py_find(m, lo, hi, T)
            for t in FIND_THREADS:
                assert oracle_mod.c_find(m, lo, hi, T, threads=t) == exp, (m.hex(), lo, hi, T, t)


def test_find_top_nonce(oracle_mod):
    """hi == 2^64-1 does not wrap: the top nonce is found when it alone hits,
    and a miss ends."""
    m = b"x"
    hs = [oracle_mod.py_hash(m, n) for n in range(MAX - 99, MAX + 1)]
    for t in FIND_THREADS:
        assert oracle_mod.c_find(m, MAX, MAX, hs[-1] + 1, threads=t) == (hs[-1], MAX)
        assert oracle_mod.c_find(m, MAX, MAX, hs[-1], threads=t) is None
        assert oracle_mod.c_find(m, MAX - 99, MAX, min(hs), threads=t) is None
        i = hs.index(min(hs))
        assert oracle_mod.c_find(m, MAX - 99, MAX, min(hs) + 1, threads=t) == (hs[i], MAX - 99 + i)
    # the range whose only hit is the top nonce: cut below every lower hit
    T = hs[-1] + 1
    first = max((i for i, h in enumerate(hs[:-1]) if h < T), default=-1) + 1
    for t in FIND_THREADS:
        assert oracle_mod.c_find(m, MAX - 99 + first, MAX, T, threads=t) == (hs[-1], MAX)


def test_find_known_answers(oracle_mod):
    for T, want in FIND_KATS:
        assert oracle_mod.py_hash(b"bradfitz", want[1]) == want[0] < T
        for t in FIND_THREADS:
            assert oracle_mod.c_find(b"bradfitz", 0, 10**7, T, threads=t) == want, (T, t)
    assert oracle_mod.py_find(b"bradfitz", 0, 10**7, FIND_KATS[1][0]) == FIND_KATS[1][1]
    assert oracle_mod.c_find(b"bradfitz", 0, 10**7, 0) is None
    # strict '<': the hit's own hash as the target passes over that nonce
    h, n = FIND_KATS[0][1]
    got = oracle_mod.c_find(b"bradfitz", 0, 10**4, h)
    assert got is not None and got[1] > n and got == oracle_mod.py_find(b"bradfitz", 0, 10**4, h)


def test_find_golden_sweep(oracle_mod, golden):
    """For every golden scan (hash, nonce): target hash + 1 gives exactly that
    pair (the lowest nonce among ties), target hash gives None."""
    for i, k in enumerate(golden["scan_kats"]):
        m, lo, hi = bytes.fromhex(k["msg_hex"]), int(k["lo"]), int(k["hi"])
        h, n = int(k["hash"]), int(k["nonce"])
        t = FIND_THREADS[i % len(FIND_THREADS)]
        if lo > hi:
            assert oracle_mod.c_find(m, lo, hi, MAX, threads=t) is None
            continue
        if hi - lo > 400_000:
            t = 16  # the 10^7 case: both targets search the whole range
        assert oracle_mod.c_find(m, lo, hi, h + 1, threads=t) == (h, n), k.get("name")
        assert oracle_mod.c_find(m, lo, hi, h, threads=t) is None, k.get("name")


@pytest.mark.parametrize("threads", FIND_THREADS)
def test_find_thread_split_invariance(oracle_mod, threads):
    """The lowest hit wins whichever chunk holds it: ranges shorter than,
    equal to and longer than the thread count, hits in several chunks."""
    for lo, hi in [(0, 0), (0, 1), (5, 9), (0, 15), (0, 16), (99_990, 100_009), (MAX - 20, MAX)]:
        hs = sorted(oracle_mod.py_hash(b"x", n) for n in range(lo, hi + 1))
        for T in {hs[0], hs[0] + 1, hs[len(hs) // 2] + 1, hs[-1] + 1, MAX}:
            assert oracle_mod.c_find(b"x", lo, hi, T, threads) == \
                oracle_mod.py_find(b"x", lo, hi, T), (lo, hi, T)

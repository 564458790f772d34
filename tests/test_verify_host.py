"""hm_hash_many_cpu and hm_verify_cpu (ABI 1.12): Hash(msg, n) at a LIST of
arbitrary nonces, and which (hash, nonce) records of a list are wrong for msg
or not below a target -- the receiving side of share collection (the
reference server believes what a miner sends: server.go:273 only compares the
hash).  The oracle is the committed C oracle's c_hash per nonce, which shares
nothing with the product code; expected bad lists are computed here from it.
Checked with both compressions: every message length 0..130 at the 40
digit-edge nonces, seeded random (length, nonce) pairs over every digit count,
a seeded set of corruptions under every buffer size of the size-query
contract, target 0, the empty list, invalid arguments, the hm_verify_stats
layout, and once a ThreadSanitizer build of the host path as a stand-alone
program.  No GPU needed."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from distributed_bitcoinminer_amd import _lib

MAXU64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")
PATHS = ["sha", "c"]
SENTINEL = 0xA5A5A5A5A5A5A5A5
NEW_SYMBOLS = ("hm_hash_many", "hm_hash_many_cpu", "hm_verify", "hm_verify_cpu",
               "hm_verify_stats_sized")
# 0, 10^k - 1 and 10^k for k = 1..19, and 2^64-1: both ends of every digit
# count.  That list has 1 + 2 * 19 + 1 = 40 members (the request for this
# feature called it "the 41 digit-edge nonces" and spelt out these 40).
EDGE_NONCES = [0] + [v for k in range(1, 20) for v in (10**k - 1, 10**k)] + [MAXU64]
LENGTHS = range(0, 131)


def message(length, salt=0):
    """A message of `length` bytes, different for every (length, salt)."""
    rng = random.Random(1000 * salt + length)
    return bytes(rng.randrange(256) for _ in range(length))


def edge_case(length):
    """(message, the 40 edge nonces in a shuffled order) of one length."""
    ns = list(EDGE_NONCES)
    random.Random(length).shuffle(ns)
    return message(length), ns


def log_uniform_nonce(rng):
    """A nonce whose digit count is uniform over 1..20."""
    d = rng.randrange(1, 21)
    lo = 0 if d == 1 else 10**(d - 1)
    hi = min(10**d - 1, MAXU64)
    return rng.randrange(lo, hi + 1)


_HASHES = {}


def oracle_hashes(oracle_mod, m, nonces):
    """[c_hash(m, n)], computed once per list and shared (do not change it)."""
    key = (bytes(m), tuple(nonces))
    if key not in _HASHES:
        _HASHES[key] = [oracle_mod.c_hash(m, n) for n in nonces]
    return _HASHES[key]


def corruption_set(oracle_mod, n, seed=7, m=b"bradfitz"):
    """A list of n records for m at a target, built from the oracle's true
    hashes and corrupted at a seeded subset: (m, target, records, expected bad
    indices ascending).  The target is the list's median true hash, so about
    half the honest records are bad for not being below it; on top
      hash low bit flipped, hash high word changed, nonce + 1 (each wrong for
      its nonce whatever the target), a true hash exactly == target (the
      median record itself: strict '<'), and the nonce 2^64-1 record, honest.
    """
    rng = random.Random(seed)
    nonces = [log_uniform_nonce(rng) for _ in range(n - 1)] + [MAXU64]
    rng.shuffle(nonces)
    true = oracle_hashes(oracle_mod, m, nonces)
    target = sorted(true)[n // 2]
    recs = [[h, x] for h, x in zip(true, nonces)]
    wrong = set()
    picks = rng.sample(range(n), 3 * (n // 10))
    for j, i in enumerate(picks):
        if nonces[i] == MAXU64 or true[i] == target:
            continue  # both stay honest (and nonce + 1 would wrap)
        kind = j % 3
        if kind == 0:
            recs[i][0] ^= 1
        elif kind == 1:
            recs[i][0] ^= 0x8000_0001 << 32
        else:
            recs[i][1] += 1
            if oracle_mod.c_hash(m, recs[i][1]) == recs[i][0]:
                continue  # (a 2^-64 event)
        wrong.add(i)
    exp = [i for i in range(n) if i in wrong or recs[i][0] >= target]
    at_target = [i for i in range(n) if recs[i][0] == target and i not in wrong]
    assert at_target and all(i in exp for i in at_target)
    top = nonces.index(MAXU64)
    assert recs[top] == [true[top], MAXU64] and (top in exp) == (true[top] >= target)
    return m, target, np.array(recs, dtype=np.uint64), exp


def verify_raw(call, m, recs, target, cap, pad=3):
    """A verify entry point through ctypes with a sentinel-filled index buffer
    of cap + pad: (rc, bad, the whole buffer as a list)."""
    r = np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 2)
    buf = np.full(cap + pad, SENTINEL, dtype=np.uint64)
    bad = ctypes.c_uint64(777)
    rc = call(m, len(m), r.ctypes.data_as(ctypes.POINTER(_lib.hm_result)), r.shape[0], target,
              buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), cap, ctypes.byref(bad))
    return rc, int(bad.value), [int(x) for x in buf]


def check_cap_contract(call, m, recs, target, exp):
    """bad and the ascending index list under every buffer size of the
    size-query contract: fitting, exactly bad, bad - 1 (nothing written), and
    0 with NULL."""
    k = len(exp)
    assert k >= 2
    rc, bad, buf = verify_raw(call, m, recs, target, k + 5)
    assert (rc, bad) == (_lib.HM_OK, k) and buf[:k] == exp
    assert all(x == SENTINEL for x in buf[k:])            # nothing beyond bad is touched
    rc, bad, buf = verify_raw(call, m, recs, target, k)
    assert (rc, bad) == (_lib.HM_OK, k) and buf[:k] == exp and all(x == SENTINEL for x in buf[k:])
    rc, bad, buf = verify_raw(call, m, recs, target, k - 1)
    assert (rc, bad) == (_lib.HM_OK, k) and all(x == SENTINEL for x in buf)  # not written at all
    r = np.ascontiguousarray(recs, dtype=np.uint64)
    bad = ctypes.c_uint64(777)
    assert call(m, len(m), r.ctypes.data_as(ctypes.POINTER(_lib.hm_result)), r.shape[0], target,
                None, 0, ctypes.byref(bad)) == _lib.HM_OK
    assert bad.value == k


def cpu_call(threads):
    lib = _lib.load()
    return lambda m, ln, r, n, T, idx, cap, bad: lib.hm_verify_cpu(m, ln, r, n, T, threads, idx,
                                                                   cap, bad)


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    """Run the test once with each compression (as tests/test_collect_host.py)."""
    if request.param == "c":
        monkeypatch.setenv("HM_CPU_NO_SHA", "1")
    else:
        monkeypatch.delenv("HM_CPU_NO_SHA", raising=False)
    return request.param


def test_version_and_symbols():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 12
    assert set(NEW_SYMBOLS) <= set(_lib.header_symbols())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define HM_VERIFY_CAP_MAX \(1u << (\d+)\)", text).group(1)) == 20
    assert _lib.HM_VERIFY_CAP_MAX == 1 << 20
    dbg = open(os.path.join(ROOT, "include", "hipminer_debug.h")).read()
    assert int(re.search(r"#define HM_OPT_VERIFY_CHUNK (\d+)", dbg).group(1)) == 19 == \
        _lib.HM_OPT_VERIFY_CHUNK
    assert len(EDGE_NONCES) == 40 and len(set(EDGE_NONCES)) == 40
    assert {len(str(n)) for n in EDGE_NONCES} == set(range(1, 21))


def test_hash_many_every_length_at_the_digit_edges(oracle_mod, path):
    for length in LENGTHS:
        m, ns = edge_case(length)
        want = oracle_hashes(oracle_mod, m, ns)
        got = _lib.hash_many_cpu(m, ns, threads=1 + length % 3)
        assert got.dtype == np.uint64 and [int(x) for x in got] == want, length


def test_hash_many_random_pairs(oracle_mod, path):
    """5,000 seeded (length <= 200, nonce) pairs, nonces log-uniform so every
    digit count occurs; grouped by message, one call per message."""
    rng = random.Random(12)
    groups = {}
    for _ in range(5000):
        groups.setdefault(rng.randrange(201), []).append(log_uniform_nonce(rng))
    assert {len(str(n)) for ns in groups.values() for n in ns} == set(range(1, 21))
    for length, ns in sorted(groups.items()):
        m = message(length, salt=1)
        assert [int(x) for x in _lib.hash_many_cpu(m, ns, threads=2)] == \
            oracle_hashes(oracle_mod, m, ns), length
    # a list long enough that 16 threads each take a part
    m, ns = b"bradfitz", [log_uniform_nonce(rng) for _ in range(20000)]
    want = oracle_hashes(oracle_mod, m, ns)
    for t in (1, 3, 16, 0):
        assert [int(x) for x in _lib.hash_many_cpu(m, ns, threads=t)] == want, t
    assert _lib.hash_many_cpu(m, [], threads=3).size == 0
    assert int(_lib.hash_many_cpu(b"", [7])[0]) == oracle_mod.c_hash(b"", 7)


def test_verify_corruptions_and_cap_contract(oracle_mod, path):
    for n, seed in ((400, 7), (20000, 8)):
        m, target, recs, exp = corruption_set(oracle_mod, n, seed)
        assert len(exp) > n // 2
        for t in (1, 3, 16):
            check_cap_contract(cpu_call(t), m, recs, target, exp)
            bad, idx = _lib.verify_cpu(m, recs, target, len(exp), threads=t)
            assert bad == len(exp) and [int(i) for i in idx] == exp
            assert _lib.verify_cpu(m, recs, target, len(exp) - 1, threads=t) == (len(exp), None)
        # target = UINT64_MAX checks the hash alone: the corrupted records only
        honest = set(i for i in range(n)
                     if int(recs[i, 0]) == oracle_mod.c_hash(m, int(recs[i, 1])))
        bad, idx = _lib.verify_cpu(m, recs, MAXU64, n, threads=3)
        assert [int(i) for i in idx] == [i for i in range(n) if i not in honest] and bad < len(exp)
        # target = 0: every record is bad
        bad, idx = _lib.verify_cpu(m, recs, 0, n, threads=3)
        assert bad == n and [int(i) for i in idx] == list(range(n))
        assert _lib.verify_cpu(m, recs, 0, n - 1, threads=16) == (n, None)
        # no record bad: the honest ones at a target above their hashes
        good = recs[sorted(honest)]
        bad, idx = _lib.verify_cpu(m, good, int(good[:, 0].max()) + 1, 4, threads=3)
        assert bad == 0 and idx.size == 0


def test_verify_edges_and_invalid_arguments(oracle_mod):
    lib = _lib.load()
    h7 = oracle_mod.c_hash(b"", 7)
    assert _lib.verify_cpu(b"", [(h7, 7)], h7 + 1, 1)[0] == 0
    assert [int(i) for i in _lib.verify_cpu(b"", [(h7, 7)], h7, 1)[1]] == [0]   # strict '<'
    # a record whose hash is UINT64_MAX is bad at target UINT64_MAX whatever its nonce
    assert _lib.verify_cpu(b"", [(MAXU64, 7)], MAXU64, 1)[0] == 1
    # repeats and any order are fine
    bad, idx = _lib.verify_cpu(b"", [(h7, 7), (h7, 7), (h7 ^ 1, 7), (h7, 7)], MAXU64, 4)
    assert (bad, [int(i) for i in idx]) == (1, [2])
    u64p = ctypes.POINTER(ctypes.c_uint64)
    recs = (_lib.hm_result * 2)()
    recs[0].hash, recs[0].nonce = h7, 7
    idx = (ctypes.c_uint64 * 2)(SENTINEL, SENTINEL)
    bad = ctypes.c_uint64(777)
    bp = ctypes.byref(bad)
    # n = 0: HM_OK, *bad = 0, nothing written; the list may be NULL
    assert lib.hm_verify_cpu(b"x", 1, None, 0, MAXU64, 1, idx, 2, bp) == _lib.HM_OK
    assert bad.value == 0 and idx[0] == SENTINEL
    assert lib.hm_hash_many_cpu(b"x", 1, None, 0, 1, None) == _lib.HM_OK
    # the empty message passed as NULL
    bad.value = 777
    assert lib.hm_verify_cpu(None, 0, recs, 1, h7 + 1, 1, idx, 2, bp) == _lib.HM_OK
    assert bad.value == 0
    bad.value = 777
    nn = (ctypes.c_uint64 * 1)(7)
    out = (ctypes.c_uint64 * 1)(SENTINEL)
    assert lib.hm_hash_many_cpu(None, 0, nn, 1, 1, out) == _lib.HM_OK and out[0] == h7
    out[0] = SENTINEL
    inv = [lib.hm_verify_cpu(None, 3, recs, 1, MAXU64, 1, idx, 2, bp),          # msg NULL, len > 0
           lib.hm_verify_cpu(b"x", 1, None, 1, MAXU64, 1, idx, 2, bp),          # n > 0, NULL list
           lib.hm_verify_cpu(b"x", 1, recs, 1, MAXU64, 1, idx, (1 << 20) + 1, bp),  # cap too large
           lib.hm_verify_cpu(b"x", 1, recs, 1, MAXU64, 1, None, 2, bp),         # cap > 0, NULL idx
           lib.hm_verify_cpu(b"x", 1, recs, 1, MAXU64, 1, idx, 2, None),        # bad NULL
           lib.hm_hash_many_cpu(b"x", 1, None, 1, 1, out),                      # n > 0, NULL list
           lib.hm_hash_many_cpu(b"x", 1, nn, 1, 1, None),                       # hashes NULL
           lib.hm_hash_many_cpu(None, 3, nn, 1, 1, out),                        # msg NULL, len > 0
           lib.hm_verify(None, b"x", 1, recs, 1, MAXU64, idx, 2, bp),           # no context
           lib.hm_hash_many(None, b"x", 1, nn, 1, out)]
    assert inv == [_lib.HM_ERR_INVALID] * len(inv)
    assert bad.value == 777 and idx[0] == SENTINEL and out[0] == SENTINEL
    st = _lib.hm_verify_stats()
    assert lib.hm_verify_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID
    assert ctypes.cast(idx, u64p)[1] == SENTINEL


def test_verify_stats_layout_matches_header(tmp_path):
    """The ctypes mirror of hm_verify_stats has the header's C layout, the
    header pins its 1.12 size, and the older structs keep theirs."""
    fields = [f for f, _ in _lib.hm_verify_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %d %zu %zu %zu\\n", sizeof(hm_verify_stats), HM_VERIFY_STATS_SIZE_1_12,'
             ' sizeof(hm_collect_stats), sizeof(hm_find_stats), sizeof(hm_stats));']
    lines += [f'  printf("%zu\\n", offsetof(hm_verify_stats, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:5] == [ctypes.sizeof(_lib.hm_verify_stats), 56, 48, 56, 168]
    assert out[5:] == [getattr(_lib.hm_verify_stats, f).offset for f in fields]
    assert out[5:] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert fields[:8] == ["wall_ms", "kernel_ms", "copy_ms", "records", "bad", "launches", "ndev",
                          "overflow"]


TSAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hipminer.h"
int main(void) {
    const char *msg = "bradfitz";
    enum { N = 40000 };
    static uint64_t nonces[N], hashes[N], again[N], idx[N];
    static hm_result recs[N];
    uint64_t x = 88172645463325252ull;
    for (int i = 0; i < N; ++i) {           /* xorshift; a shift spreads the digit counts */
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        nonces[i] = x >> (i % 64);
    }
    nonces[0] = 0; nonces[1] = ~0ull; nonces[2] = 9898;
    int threads[] = {1, 3, 16};
    for (int t = 0; t < 3; ++t) {
        if (hm_hash_many_cpu((const uint8_t *)msg, strlen(msg), nonces, N, threads[t],
                             t ? again : hashes))
            return 2;
        if (t && memcmp(again, hashes, sizeof hashes)) return 3;
    }
    if (hashes[2] != 1419516646206828ull) return 4;   /* the reference's known answer */
    uint64_t want = 0;
    for (int i = 0; i < N; ++i) {
        recs[i].hash = hashes[i] ^ (i % 5 == 0);    /* every fifth record is wrong */
        recs[i].nonce = nonces[i];
        want += i % 5 == 0;
    }
    for (int t = 0; t < 3; ++t) {
        uint64_t bad = 0;
        if (hm_verify_cpu((const uint8_t *)msg, strlen(msg), recs, N, ~0ull, threads[t], idx, N,
                          &bad))
            return 5;
        if (bad != want) return 6;
        for (uint64_t k = 0; k < bad; ++k)
            if (idx[k] != 5 * k) return 7;
        uint64_t count = 0;                  /* every part overflows the cap */
        if (hm_verify_cpu((const uint8_t *)msg, strlen(msg), recs, N, 0, threads[t], idx, 16,
                          &count))
            return 8;
        if (count != N) return 9;
    }
    puts("tsan ok");
    return 0;
}
"""


def test_thread_sanitizer_standalone(tmp_path):
    """host_scan.cpp and plan.cpp built with -fsanitize=thread into a
    stand-alone program that calls hm_hash_many_cpu and hm_verify_cpu from 1, 3
    and 16 threads: no data race reported.  Nothing is preloaded and nothing
    is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = tmp_path / "tsan_main.c.cpp"
    main.write_text(TSAN_MAIN)
    exe = tmp_path / "tsan_verify"
    inc = os.path.join(ROOT, "include")
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-fsanitize=thread", "-pthread",
           "-Wno-unknown-pragmas", f"-I{inc}", "-o", str(exe), str(main),
           os.path.join(CSRC, "host_scan.cpp"), os.path.join(CSRC, "plan.cpp")]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "tsan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]

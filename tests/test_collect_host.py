"""hm_collect_cpu (ABI 1.11): EVERY nonce of an inclusive range whose hash is
below a target, ascending, and their exact count -- the share-collection form
of the reference loop (cmu440/bitcoin/miner/miner.go:46-59 over bitcoin.Hash,
hash.go:13-17):
    for n = lo .. hi: if Hash(msg, n) < target: emit (Hash, n)
The oracle of the question is built here from the committed C oracle: its
first-hit search c_find iterated from lo, restarting at answer + 1, until it
finds nothing -- a plain ascending loop over the oracle's own SHA-256 and
formatting -- cross-checked once against hashlib.  Checked with both
compressions and several thread counts: known answers, strict '<', the golden
scans, dense targets, every digit boundary, the top of the nonce space, the
overflow (size-query) contract, invalid arguments, the hm_collect_stats
layout, and once a ThreadSanitizer build of the host path as a stand-alone
program.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from distributed_bitcoinminer_amd import _lib
from tests.test_find_host import TOP_CLEAR, py_hash, top_nonce_case

MAXU64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")
PATHS = ["sha", "c"]
THREADS = (1, 2, 7, 16, 0)
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A)


_ORACLE = {}


def oracle_loop(oracle_mod, m, lo, hi, T, threads=1):
    """Every (hash, nonce) of [lo, hi] with hash < T, ascending: c_find from
    n = lo, restarted at answer + 1, until it returns None."""
    out, n = [], lo
    while n <= hi:
        got = oracle_mod.c_find(m, n, hi, T, threads=threads)
        if got is None:
            break
        out.append(got)
        n = got[1] + 1
    return out


def oracle_collect(oracle_mod, m, lo, hi, T):
    """oracle_loop, computed once per question and shared (callers must not
    change the list).  Dense targets take one thread (each call then stops at
    its first hit: one pass over the range in all); sparse ones split every
    call's remaining range."""
    key = (bytes(m), lo, hi, T)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_loop(oracle_mod, m, lo, hi, T, 1 if T > 2**64 // 10**4 else 0)
    return _ORACLE[key]


def collect_raw(m, lo, hi, T, threads, cap):
    """hm_collect_cpu through ctypes with a sentinel-filled buffer of cap + 1
    records: (rc, total, the whole buffer as a list of pairs)."""
    lib = _lib.load()
    n = cap + 1
    buf = (_lib.hm_result * n)()
    for i in range(n):
        buf[i].hash, buf[i].nonce = SENTINEL
    total = ctypes.c_uint64(777)
    rc = lib.hm_collect_cpu(m, len(m), lo, hi, T, threads, buf, cap, ctypes.byref(total))
    return rc, int(total.value), [(int(r.hash), int(r.nonce)) for r in buf]


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    """Run the test once with each compression (as tests/test_host_scan.py)."""
    if request.param == "c":
        monkeypatch.setenv("HM_CPU_NO_SHA", "1")
    else:
        monkeypatch.delenv("HM_CPU_NO_SHA", raising=False)
    return request.param


def test_version_symbols_and_merge():
    v = _lib.load().hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 11
    assert {"hm_collect", "hm_collect_cpu", "hm_collect_stats_sized"} <= set(_lib.header_symbols())
    for s in ("hm_collect", "hm_collect_cpu", "hm_collect_stats_sized", "hm_find"):
        assert hasattr(_lib.load(), s), s
    import re
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define HM_COLLECT_CAP_MAX \(1u << (\d+)\)", text).group(1)) == 24
    assert _lib.HM_COLLECT_CAP_MAX == 1 << 24
    from distributed_bitcoinminer_amd import parallel
    assert parallel.merge_collect([], 0) == (0, [])
    assert parallel.merge_collect([(0, []), (2, [(5, 10), (7, 11)]), (1, [(3, 40)])], 3) == \
        (3, [(5, 10), (7, 11), (3, 40)])
    assert parallel.merge_collect([(2, [(5, 10), (7, 11)]), (2, None)], 3) == (4, None)
    assert parallel.merge_collect([(2, [(5, 10), (7, 11)]), (1, [(3, 40)])], 2) == (3, None)
    with pytest.raises(ValueError):
        parallel.merge_collect([(2, None), (1, [(3, 40)])], 8)


def test_oracle_loop_against_hashlib(oracle_mod):
    """The iterated-c_find oracle equals a hashlib loop on a few thousand nonces."""
    for m, lo, hi, T in ((b"bradfitz", 0, 4000, 2**64 // 10), (b"thom yorke", 9_000, 11_500, 2**63),
                         (b"x" * 60, 99_000, 101_000, 2**64 // 100)):
        want = [(py_hash(m, n), n) for n in range(lo, hi + 1) if py_hash(m, n) < T]
        assert want and oracle_collect(oracle_mod, m, lo, hi, T) == want


def test_known_answers(oracle_mod, path):
    m, lo, hi = b"bradfitz", 0, 10**7
    for T, first in ((2**64 // 10**3, (6697378768932333, 203)),
                     (2**64 // 10**6, (7182149750005, 2351907))):
        want = oracle_collect(oracle_mod, m, lo, hi, T)
        assert want[0] == first
        for t in THREADS:
            total, recs = _lib.collect_cpu(m, lo, hi, T, len(want) + 3, threads=t)
            assert total == len(want) and recs == want, (T, t)
            assert all(a[1] < b[1] for a, b in zip(recs, recs[1:]))
        assert _lib.count_cpu(m, lo, hi, T, threads=0) == len(want)
        step = max(1, len(want) // 200)
        assert all(_lib.host_hash(m, n) == h < T for h, n in want[::step])
    # strict '<': T = the hash of a known hit leaves that nonce out, T + 1 takes it
    h, n = 7182149750005, 2351907
    total, recs = _lib.collect_cpu(m, lo, hi, h, 64, threads=16)
    assert recs is not None and n not in [r[1] for r in recs]
    total1, recs1 = _lib.collect_cpu(m, lo, hi, h + 1, 64, threads=16)
    assert total1 == total + 1 and (h, n) in recs1
    assert recs1 == oracle_collect(oracle_mod, m, lo, hi, h + 1)


def test_golden_sweep(golden, path):
    """For every golden scan (hash, nonce): T = hash + 1 gives a list whose
    minimum-hash element is the golden pair, every hash <= hash; T = hash
    leaves that nonce out.  The empty ranges give total == 0."""
    kats = golden["scan_kats"]
    if path == "c":  # the portable compression on a subset (it is ~4x slower)
        kats = [k for k in kats if int(k["hi"]) - int(k["lo"]) <= 20000]
    for i, k in enumerate(kats):
        m = bytes.fromhex(k["msg_hex"])
        lo, hi, h, n = int(k["lo"]), int(k["hi"]), int(k["hash"]), int(k["nonce"])
        t = THREADS[i % len(THREADS)]
        if lo > hi:
            assert _lib.collect_cpu(m, lo, hi, MAXU64, 4, threads=t) == (0, [])
            assert _lib.count_cpu(m, lo, hi, MAXU64, threads=t) == 0
            continue
        total, recs = _lib.collect_cpu(m, lo, hi, h + 1, 16, threads=t)
        assert total == len(recs) >= 1, k.get("name")
        assert min(recs) == (h, n) and all(r[0] <= h and lo <= r[1] <= hi for r in recs)
        total0, recs0 = _lib.collect_cpu(m, lo, hi, h, 16, threads=t)
        assert n not in [r[1] for r in recs0] and total0 == len(recs0) < total, k.get("name")


def test_dense(oracle_mod, path):
    """T = 2^64-1: every nonce but those hashing to 2^64-1 (the oracle says
    which; none here), consecutive."""
    for m, lo, hi in ((b"bradfitz", 0, 19_999), (b"x" * 56, 10**11 - 3_000, 10**11 + 3_000),
                      (bytes(range(120)), 10**19 - 2_500, 10**19 + 2_500),
                      (b"", MAXU64 - 5_000, MAXU64), (b"q", 77, 77)):
        want = oracle_collect(oracle_mod, m, lo, hi, MAXU64)
        span = hi - lo + 1
        top = [n for n in range(lo, hi + 1) if oracle_mod.c_hash(m, n) == MAXU64]
        assert len(want) == span - len(top)
        assert [r[1] for r in want] == [n for n in range(lo, hi + 1) if n not in top]
        for t in THREADS:
            total, recs = _lib.collect_cpu(m, lo, hi, MAXU64, span, threads=t)
            assert total == len(want) and recs == want, (m, lo, t)


def test_digit_boundaries(oracle_mod, path):
    T = 2**64 // 10**3
    for d in range(1, 20):
        lo, hi = max(10**d - 1500, 0), min(MAXU64, 10**d + 1500)
        for m in (b"bradfitz", bytes(0x41 + i % 26 for i in range(50 + d))):
            want = oracle_collect(oracle_mod, m, lo, hi, T)
            for t in (1, 3):
                assert _lib.collect_cpu(m, lo, hi, T, 64, threads=t) == (len(want), want), (d, m, t)


def test_top_of_the_nonce_space(oracle_mod, path):
    """Nonce 2^64-1 is an ordinary record: the only one of
    [2^64-1-4454, 2^64-1] at T = h + 1, and none at T = h."""
    m, h = top_nonce_case()
    assert oracle_mod.c_hash(m, MAXU64) == h
    lo = MAXU64 - TOP_CLEAR
    assert oracle_collect(oracle_mod, m, lo, MAXU64, h + 1) == [(h, MAXU64)]
    for t in THREADS:
        assert _lib.collect_cpu(m, lo, MAXU64, h + 1, 4, threads=t) == (1, [(h, MAXU64)])
        assert _lib.collect_cpu(m, MAXU64, MAXU64, h + 1, 1, threads=t) == (1, [(h, MAXU64)])
        assert _lib.collect_cpu(m, lo, MAXU64, h, 4, threads=t) == (0, [])
        assert _lib.count_cpu(m, lo, MAXU64, h, threads=t) == 0
    # one nonce further down hashes lower: two records
    lower = lo - 1
    hl = oracle_mod.c_hash(m, lower)
    assert _lib.collect_cpu(m, lower, MAXU64, h + 1, 4, threads=2) == (2, [(hl, lower), (h, MAXU64)])


def test_overflow_contract(oracle_mod, path):
    m, lo, hi, T = b"thom yorke", 999_000, 1_201_000, 2**64 // 10**4
    want = oracle_collect(oracle_mod, m, lo, hi, T)
    k = len(want)
    assert k >= 2
    for t in THREADS:
        # cap = k - 1: HM_OK, *total = k, out untouched
        rc, total, buf = collect_raw(m, lo, hi, T, t, k - 1)
        assert (rc, total) == (_lib.HM_OK, k) and all(r == SENTINEL for r in buf), t
        # cap = k: exactly k records, out[k] untouched
        rc, total, buf = collect_raw(m, lo, hi, T, t, k)
        assert (rc, total) == (_lib.HM_OK, k) and buf[:k] == want and buf[k] == SENTINEL, t
        # a larger cap: nothing beyond out[total) is touched
        rc, total, buf = collect_raw(m, lo, hi, T, t, k + 5)
        assert (rc, total) == (_lib.HM_OK, k) and buf[:k] == want, t
        assert all(r == SENTINEL for r in buf[k:]), t
        # cap = 0 with out = NULL: the count
        total = ctypes.c_uint64(0)
        assert _lib.load().hm_collect_cpu(m, len(m), lo, hi, T, t, None, 0,
                                          ctypes.byref(total)) == _lib.HM_OK
        assert total.value == k
        assert _lib.collect_cpu(m, lo, hi, T, k - 1, threads=t) == (k, None)
    # a dense target whose every chunk overflows the cap on its own
    assert _lib.collect_cpu(m, lo, hi, MAXU64, 10, threads=7) == (hi - lo + 1, None)


def test_edges_and_invalid_arguments():
    lib = _lib.load()
    assert _lib.collect_cpu(b"bradfitz", 0, 10**5, 0, 8) == (0, [])      # target 0 never hits
    assert _lib.collect_cpu(b"bradfitz", 5, 4, MAXU64, 8) == (0, [])     # lo > hi
    h7 = _lib.host_hash(b"", 7)
    assert _lib.collect_cpu(b"", 7, 7, h7 + 1, 1) == (1, [(h7, 7)])
    assert _lib.collect_cpu(b"", 7, 7, h7, 1) == (0, [])
    # the empty message passed as NULL
    total = ctypes.c_uint64(0)
    assert lib.hm_collect_cpu(None, 0, 0, 5000, 2**64 // 10, 2, None, 0,
                              ctypes.byref(total)) == _lib.HM_OK
    assert total.value == _lib.count_cpu(b"", 0, 5000, 2**64 // 10) > 0
    buf = (_lib.hm_result * 2)()
    buf[0].hash, buf[0].nonce = SENTINEL
    total = ctypes.c_uint64(777)
    tp = ctypes.byref(total)
    bad = [lib.hm_collect_cpu(None, 3, 0, 9, 5, 1, buf, 2, tp),                  # msg NULL, len > 0
           lib.hm_collect_cpu(b"x", 1, 0, 9, MAXU64, 1, None, 2, tp),            # cap > 0, out NULL
           lib.hm_collect_cpu(b"x", 1, 0, 9, MAXU64, 1, buf, 2, None),           # total NULL
           lib.hm_collect_cpu(b"x", 1, 0, 9, MAXU64, 1, buf, (1 << 24) + 1, tp),  # cap too large
           lib.hm_collect(None, b"x", 1, 0, 9, MAXU64, buf, 2, tp)]              # no context
    assert bad == [_lib.HM_ERR_INVALID] * 5
    assert total.value == 777 and (int(buf[0].hash), int(buf[0].nonce)) == SENTINEL
    st = _lib.hm_collect_stats()
    assert lib.hm_collect_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID


def test_collect_stats_layout_matches_header(tmp_path):
    """The ctypes mirror of hm_collect_stats has the header's C layout, the
    header pins its 1.11 size, and the older structs keep theirs."""
    fields = [f for f, _ in _lib.hm_collect_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %d %zu %zu\\n", sizeof(hm_collect_stats), HM_COLLECT_STATS_SIZE_1_11,'
             ' sizeof(hm_find_stats), sizeof(hm_stats));']
    lines += [f'  printf("%zu\\n", offsetof(hm_collect_stats, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:4] == [ctypes.sizeof(_lib.hm_collect_stats), 48, 56, 168]
    assert out[4:] == [getattr(_lib.hm_collect_stats, f).offset for f in fields]
    assert fields[:7] == ["wall_ms", "kernel_ms", "nonces", "total", "launches", "ndev", "overflow"]


TSAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "hipminer.h"
int main(void) {
    const char *msg = "bradfitz";
    const uint64_t T = 18446744073709551615ull / 1000ull;   /* first hit: 203 */
    int threads[] = {1, 2, 7, 16};
    static hm_result out[4096];
    uint64_t first_total = 0;
    for (int i = 0; i < 4; ++i) {
        uint64_t total = 0;
        if (hm_collect_cpu((const uint8_t *)msg, strlen(msg), 0, 2000000, T, threads[i], out, 4096,
                           &total))
            return 2;
        if (total < 1000 || total > 4096 || out[0].nonce != 203ull ||
            out[0].hash != 6697378768932333ull)
            return 3;
        for (uint64_t k = 1; k < total; ++k)
            if (out[k].nonce <= out[k - 1].nonce || out[k].hash >= T) return 4;
        if (i == 0) first_total = total;
        if (total != first_total) return 5;
        uint64_t count = 0;
        if (hm_collect_cpu((const uint8_t *)msg, strlen(msg), 0, 2000000, T, threads[i], NULL, 0,
                           &count))
            return 6;
        if (count != total) return 7;
        /* every chunk overflows */
        if (hm_collect_cpu((const uint8_t *)msg, strlen(msg), 0, 200000, ~0ull, threads[i], out, 16,
                           &count))
            return 8;
        if (count != 200001ull) return 9;
    }
    puts("tsan ok");
    return 0;
}
"""


def test_thread_sanitizer_standalone(tmp_path):
    """host_scan.cpp and plan.cpp built with -fsanitize=thread into a
    stand-alone program that calls hm_collect_cpu from 1, 2, 7 and 16
    threads: no data race reported."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = tmp_path / "tsan_main.c.cpp"
    main.write_text(TSAN_MAIN)
    exe = tmp_path / "tsan_collect"
    inc = os.path.join(ROOT, "include")
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-fsanitize=thread", "-pthread",
           "-Wno-unknown-pragmas", f"-I{inc}", "-o", str(exe), str(main),
           os.path.join(CSRC, "host_scan.cpp"), os.path.join(CSRC, "plan.cpp")]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "tsan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]

"""hm_find_cpu (ABI 1.10): the lowest nonce of an inclusive range whose hash
is below a target -- the proof-of-work form of the reference loop
(cmu440/bitcoin/miner/miner.go:46-59 over bitcoin.Hash, hash.go:13-17):
    for n = lo .. hi: if Hash(msg, n) < target: return (Hash, n)
Checked against hashlib known answers, the committed golden scans and the C
oracle (its min-hash scan, and its own first-hit search c_find at the target
edges, dense targets and the top nonce -- the reference the GPU path is
judged by too), with both compressions and several thread counts; the hm_find_stats
layout and the ABI version; and, once, a ThreadSanitizer build of the host
search as a stand-alone program.  No GPU needed."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import pytest

from distributed_bitcoinminer_amd import _lib

MAXU64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")
PATHS = ["sha", "c"]
THREADS = (1, 2, 7, 16)

# bradfitz, [0, 10^7]: the first nonce below each target
KATS = [(2**64 // 10**3, (6697378768932333, 203)),
        (2**64 // 10**5, (158752571039048, 91989)),
        (2**64 // 10**6, (7182149750005, 2351907))]


def py_hash(m: bytes, n: int) -> int:
    return int.from_bytes(hashlib.sha256(m + b" " + str(n).encode()).digest()[:8], "big")


def check_find(scan, m, lo, hi, T, got):
    """`got` is find's answer for (m, [lo, hi], T); `scan(m, a, b)` a trusted
    min-hash scan."""
    if got is None:
        assert scan(m, lo, hi)[0] >= T, (m, lo, hi, T)
        return
    h, n = got
    assert lo <= n <= hi, (got, lo, hi)
    assert _lib.host_hash(m, n) == h < T, (got, T)
    assert n == lo or scan(m, lo, n - 1)[0] >= T, (got, lo, T)


@pytest.fixture(params=PATHS)
def path(request, monkeypatch):
    """Run the test once with each compression (as tests/test_host_scan.py)."""
    if request.param == "c":
        monkeypatch.setenv("HM_CPU_NO_SHA", "1")
    else:
        monkeypatch.delenv("HM_CPU_NO_SHA", raising=False)
    return request.param


def test_version_is_1_10():
    v = _lib.load().hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 10
    assert {"hm_find", "hm_find_cpu", "hm_find_stats_sized"} <= set(_lib.header_symbols())


def test_known_answers(oracle_mod, path):
    for T, want in KATS:
        assert py_hash(b"bradfitz", want[1]) == want[0] < T
        assert all(py_hash(b"bradfitz", n) >= T for n in range(min(want[1], 3000)))
        for t in THREADS:
            assert _lib.find_cpu(b"bradfitz", 0, 10**7, T, threads=t) == want, (T, t)
    # strict '<': a target equal to the last hit's hash does not take that nonce
    h, n = KATS[-1][1]
    got = _lib.find_cpu(b"bradfitz", 0, 10**7, h, threads=16)
    assert got is None or got[1] != n
    check_find(oracle_mod.c_scan, b"bradfitz", 0, 10**7, h, got)


def test_golden_sweep(golden, path):
    """For every golden scan (hash, nonce): target hash + 1 gives exactly that
    pair (the lowest nonce among ties), target hash gives None."""
    kats = golden["scan_kats"]
    if path == "c":  # the portable compression on a subset (it is ~4x slower)
        kats = [k for k in kats if int(k["hi"]) - int(k["lo"]) <= 20000]
    for i, k in enumerate(kats):
        m = bytes.fromhex(k["msg_hex"])
        lo, hi, h, n = int(k["lo"]), int(k["hi"]), int(k["hash"]), int(k["nonce"])
        t = THREADS[i % len(THREADS)]
        if lo > hi:
            # an empty range: the pair is the seed (MaxUint64, 0), which the C
            # call writes with *found = 0 (hash + 1 does not fit a target)
            out, found = _lib.hm_result(), ctypes.c_int(-1)
            assert _lib.load().hm_find_cpu(m, len(m), lo, hi, MAXU64, t, ctypes.byref(out),
                                           ctypes.byref(found)) == _lib.HM_OK
            assert (int(out.hash), int(out.nonce), found.value) == (h, n, 0) == (MAXU64, 0, 0)
            continue
        assert _lib.find_cpu(m, lo, hi, h + 1, threads=t) == (h, n), k.get("name")
        assert _lib.find_cpu(m, lo, hi, h, threads=t) is None, k.get("name")


def test_thread_counts_agree(oracle_mod, path):
    lo, hi = 999_000, 1_201_000  # crosses 6 -> 7 digits
    for T in (2**64 // 10**3, 2**64 // 10**5, 2**64 // 10**7):
        got = {t: _lib.find_cpu(b"thom yorke", lo, hi, T, threads=t) for t in THREADS + (0,)}
        assert len(set(got.values())) == 1, got
        check_find(oracle_mod.c_scan, b"thom yorke", lo, hi, T, got[1])


def test_edges(oracle_mod, path):
    scan = oracle_mod.c_scan
    T = 2**64 // 10**3
    assert _lib.find_cpu(b"bradfitz", 0, 10**5, 0) is None           # target 0 never hits
    assert _lib.find_cpu(b"bradfitz", 5, 4, MAXU64) is None          # lo > hi
    h7 = oracle_mod.c_hash(b"", 7)
    assert _lib.find_cpu(b"", 7, 7, h7 + 1) == (h7, 7)                # lo == hi
    assert _lib.find_cpu(b"", 7, 7, h7) is None
    hx = oracle_mod.c_hash(b"x", MAXU64)
    assert _lib.find_cpu(b"x", MAXU64, MAXU64, hx + 1) == (hx, MAXU64)
    assert _lib.find_cpu(b"x", MAXU64, MAXU64, hx) is None
    # the last 10^5 nonces below 2^64
    top = (MAXU64 - 10**5 + 1, MAXU64)
    for t in (2**64 // 10**4, 2**64 // 10**6):
        check_find(scan, b"bradfitz", *top, t, _lib.find_cpu(b"bradfitz", *top, t, threads=7))
    h, n = scan(b"bradfitz", *top)
    assert _lib.find_cpu(b"bradfitz", *top, h + 1, threads=16) == (h, n)
    assert _lib.find_cpu(b"bradfitz", *top, h, threads=16) is None
    # the empty message passed as NULL
    out, found = _lib.hm_result(), ctypes.c_int(-1)
    assert _lib.load().hm_find_cpu(None, 0, 0, 5000, T, 2, ctypes.byref(out),
                                   ctypes.byref(found)) == _lib.HM_OK
    got = (int(out.hash), int(out.nonce)) if found.value else None
    assert got == _lib.find_cpu(b"", 0, 5000, T)
    check_find(scan, b"", 0, 5000, T, got)
    # ranges across every digit boundary: the hit before, at and after it
    for d in range(1, 20):
        lo, hi = 10**d - 1500, min(MAXU64, 10**d + 1500)
        lo = max(lo, 0)
        for m in (b"bradfitz", bytes(0x41 + i % 26 for i in range(50 + d))):
            check_find(scan, m, lo, hi, T, _lib.find_cpu(m, lo, hi, T, threads=2))
            h, n = scan(m, lo, hi)
            assert _lib.find_cpu(m, lo, hi, h + 1, threads=3) == (h, n), (d, m)
            assert _lib.find_cpu(m, lo, hi, h, threads=3) is None, (d, m)


def target_edges(oracle_mod, m, lo, hi, j):
    """The targets at which a first-hit search can go wrong, for one range:
    dense ones (the answer is lo or a neighbour), the edges of the target's
    high word ((T - 1) >> 32 at 1, 2^32, 2^32 + 1, 2^63, 2^64 - 1), the
    range's minimum (a miss) and minimum + 1 (a full search), and a strict-<
    boundary at the arbitrary nonce lo + j."""
    best = oracle_mod.c_scan(m, lo, hi)[0]
    return [MAXU64, 2**63] + [2**64 // 10**k for k in range(1, 7)] + \
        [1, 2**32, 2**32 + 1, best + 1, best, oracle_mod.c_hash(m, lo + j) + 1]


def top_nonce_case():
    """(msg, hash at 2^64-1): the first of b"top-0" .. b"top-3999" whose hash
    at nonce 2^64-1 is the lowest of the 4000 -- low enough that thousands of
    nonces below 2^64-1 all hash above it."""
    h, i = min((py_hash(b"top-%d" % i, MAXU64), i) for i in range(4000))
    return b"top-%d" % i, h


TOP_CLEAR = 4454  # nonces below 2^64-1 hashing at or above top_nonce_case()'s hash


def test_target_edges_against_the_oracle(oracle_mod, path):
    """find_cpu == c_find at every target edge, dense targets included, on
    ranges across digit boundaries and at the top of the nonce space."""
    cases = [(b"bradfitz", 0, 12_000, 5_000), (b"thom yorke", 99_000, 104_000, 4_999),
             (b"x" * 56, 10**11 - 3_000, 10**11 + 3_000, 3_000),
             (bytes(range(120)), 10**19 - 2_500, 10**19 + 2_500, 17),
             (b"", MAXU64 - 5_000, MAXU64, 5_000), (b"q", 77, 77, 0)]
    for m, lo, hi, j in cases:
        for T in target_edges(oracle_mod, m, lo, hi, j):
            exp = oracle_mod.c_find(m, lo, hi, T)
            for t in THREADS:
                assert _lib.find_cpu(m, lo, hi, T, threads=t) == exp, (m, lo, hi, T, t)
        # the dense targets answer at lo or next to it
        assert oracle_mod.c_find(m, lo, hi, MAXU64)[1] in (lo, lo + 1)


def test_top_nonce_against_the_oracle(oracle_mod, path):
    """Nonce 2^64-1 as the only hit of a one-nonce and of a 4455-nonce range,
    and a lower hit one nonce further down."""
    m, h = top_nonce_case()
    assert (m, h) == (b"top-444", 1599801557507019)
    assert oracle_mod.c_hash(m, MAXU64) == h
    assert oracle_mod.c_scan(m, MAXU64 - TOP_CLEAR, MAXU64 - 1)[0] >= h
    lower = MAXU64 - TOP_CLEAR - 1
    assert oracle_mod.c_hash(m, lower) < h
    for t in THREADS:
        for lo in (MAXU64, MAXU64 - TOP_CLEAR):
            assert _lib.find_cpu(m, lo, MAXU64, h + 1, threads=t) == (h, MAXU64) == \
                oracle_mod.c_find(m, lo, MAXU64, h + 1, threads=t), (lo, t)
            assert _lib.find_cpu(m, lo, MAXU64, h, threads=t) is None
            assert oracle_mod.c_find(m, lo, MAXU64, h, threads=t) is None
        for T in (h + 1, h):
            got = _lib.find_cpu(m, lower, MAXU64, T, threads=t)
            assert got == (oracle_mod.c_hash(m, lower), lower) == \
                oracle_mod.c_find(m, lower, MAXU64, T, threads=t), (T, t)


def test_invalid_arguments():
    lib = _lib.load()
    out, found = _lib.hm_result(), ctypes.c_int(7)
    o, f = ctypes.byref(out), ctypes.byref(found)
    assert lib.hm_find_cpu(None, 3, 0, 1, 5, 1, o, f) == _lib.HM_ERR_INVALID
    assert lib.hm_find_cpu(b"x", 1, 0, 1, 5, 1, None, f) == _lib.HM_ERR_INVALID
    assert lib.hm_find_cpu(b"x", 1, 0, 1, 5, 1, o, None) == _lib.HM_ERR_INVALID
    assert found.value == 7                                  # untouched on error
    assert lib.hm_find(None, b"x", 1, 0, 1, 5, o, f) == _lib.HM_ERR_INVALID
    st = _lib.hm_find_stats()
    assert lib.hm_find_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID


def test_find_stats_layout_matches_header(tmp_path):
    """The ctypes mirror of hm_find_stats has the header's C layout, and the
    header pins its 1.10 size; hm_stats keeps its 168 bytes."""
    fields = [f for f, _ in _lib.hm_find_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %d %zu\\n", sizeof(hm_find_stats), HM_FIND_STATS_SIZE_1_10,'
             ' sizeof(hm_stats));']
    lines += [f'  printf("%zu\\n", offsetof(hm_find_stats, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:3] == [ctypes.sizeof(_lib.hm_find_stats), 56, 168]
    assert out[3:] == [getattr(_lib.hm_find_stats, f).offset for f in fields]


def test_merge_first():
    from distributed_bitcoinminer_amd import parallel
    assert parallel.merge_first([]) is None
    assert parallel.merge_first([None, None]) is None
    assert parallel.merge_first([None, (5, 900), (9, 30), None, (1, 31)]) == (9, 30)


TSAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "hipminer.h"
int main(void) {
    const char *msg = "bradfitz";
    const uint64_t T = 18446744073709551615ull / 100000ull;   /* first hit: 91989 */
    int threads[] = {1, 2, 7, 16};
    for (int i = 0; i < 4; ++i) {
        hm_result out;
        int found = 0;
        if (hm_find_cpu((const uint8_t *)msg, strlen(msg), 0, 2000000, T, threads[i], &out, &found))
            return 2;
        if (!found || out.nonce != 91989ull || out.hash != 158752571039048ull) return 3;
        if (hm_find_cpu((const uint8_t *)msg, strlen(msg), 0, 90000, T, threads[i], &out, &found))
            return 4;
        if (found) return 5;
        hm_result s;
        if (hm_scan_cpu((const uint8_t *)msg, strlen(msg), 0, 9999, threads[i], &s)) return 6;
        if (s.nonce != 9898ull) return 7;
    }
    puts("tsan ok");
    return 0;
}
"""


def test_thread_sanitizer_standalone(tmp_path):
    """host_scan.cpp and plan.cpp built with -fsanitize=thread into a
    stand-alone program that calls hm_find_cpu from 1, 2, 7 and 16 threads:
    no data race reported."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = tmp_path / "tsan_main.c.cpp"
    main.write_text(TSAN_MAIN)
    exe = tmp_path / "tsan_find"
    inc = os.path.join(ROOT, "include")
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-fsanitize=thread", "-pthread",
           "-Wno-unknown-pragmas", f"-I{inc}", "-o", str(exe), str(main),
           os.path.join(CSRC, "host_scan.cpp"), os.path.join(CSRC, "plan.cpp")]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "tsan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]

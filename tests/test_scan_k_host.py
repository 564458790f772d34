"""hm_scan_k (ABI 1.19), host side: the k lexicographically smallest
(Hash(msg, nonce), nonce) pairs of an inclusive range, ascending -- the ranking
form of the reference loop (cmu440/bitcoin/miner/miner.go:46-59 over
bitcoin.Hash, hash.go:13-17, is k = 1).  hm_scan_k_cpu is checked against
    sorted((oracle.c_hash(m, n), n) for n in range)[:k]
over digit-count changes, k = 1, 5, 32, several thread counts and both
compressions; then the golden scans, the edges, the invalid arguments, the
stats layout, the Makefile facts, a stand-alone AddressSanitizer + UBSan
program over the host path, and the placement of the new kernels' hot loops.
No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from distributed_bitcoinminer_amd import _lib
from distributed_bitcoinminer_amd import build_id as bid

MAXU64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")
KS = (1, 5, 32)
THREADS = (1, 3, 16)
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A)
ALIGNED = os.path.join(ROOT, "build", "hipminer", "scan_k_kernels.aligned.s")

# ranges of at most 3000 nonces: inside one digit count, and across 1 -> 2 -> 3 -> 4
# digits, 4 -> 5, 9 -> 10, 19 -> 20 digits and the top of the nonce space
RANGES = [(b"bradfitz", 0, 2999), (b"thom yorke", 9_000, 11_500), (b"", 0, 120),
          (b"x" * 55, 999_999_000, 1_000_001_500), (bytes(range(120)), 10**19 - 1200, 10**19 + 1200),
          (b"q" * 64, MAXU64 - 2500, MAXU64), (b"one", 77, 77), (b"few", 95, 104)]

_SORTED = {}


def oracle_sorted(oracle_mod, m, lo, hi):
    """sorted((oracle.c_hash(m, n), n) for n in [lo, hi]), once per range."""
    key = (m, lo, hi)
    if key not in _SORTED:
        _SORTED[key] = sorted((oracle_mod.c_hash(m, n), n) for n in range(lo, hi + 1))
    return _SORTED[key]


def scan_k_raw(m, lo, hi, k, threads, room=None):
    """hm_scan_k_cpu through ctypes with a sentinel-filled buffer of `room`
    records (default k + 1): (rc, n, the whole buffer as a list of pairs)."""
    room = k + 1 if room is None else room
    buf = (_lib.hm_result * room)()
    for i in range(room):
        buf[i].hash, buf[i].nonce = SENTINEL
    n = ctypes.c_size_t(777)
    rc = _lib.load().hm_scan_k_cpu(m, len(m), lo, hi, k, threads, buf, ctypes.byref(n))
    return rc, int(n.value), [(int(r.hash), int(r.nonce)) for r in buf]


@pytest.fixture(params=["sha", "c"])
def path(request, monkeypatch):
    """Run the test once with each compression (as tests/test_host_scan.py)."""
    if request.param == "c":
        monkeypatch.setenv("HM_CPU_NO_SHA", "1")
    else:
        monkeypatch.delenv("HM_CPU_NO_SHA", raising=False)
    return request.param


def test_version_and_symbols():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 19
    names = {"hm_scan_k", "hm_scan_k_cpu", "hm_scan_k_stats_sized"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.PROTOTYPES)
    for s in names:
        assert hasattr(lib, s), s
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define HM_SCAN_K_MAX (\d+)u", text).group(1)) == 32
    assert _lib.HM_SCAN_K_MAX == 32
    # no new option ids: 23 stays the highest
    ids = [int(x) for x in re.findall(r"#define HM_OPT_\w+\s+(\d+)", text)]
    debug = open(os.path.join(ROOT, "include", "hipminer_debug.h")).read()
    ids += [int(x) for x in re.findall(r"#define HM_OPT_\w+\s+(\d+)", debug)]
    assert max(ids) == 23


def test_invalid_arguments():
    lib = _lib.load()
    buf = (_lib.hm_result * 40)()
    buf[0].hash, buf[0].nonce = SENTINEL
    n = ctypes.c_size_t(777)
    np_ = ctypes.byref(n)
    bad = [lib.hm_scan_k_cpu(b"x", 1, 0, 9, 0, 1, buf, np_),            # k == 0
           lib.hm_scan_k_cpu(b"x", 1, 0, 9, 33, 1, buf, np_),           # k > HM_SCAN_K_MAX
           lib.hm_scan_k_cpu(b"x", 1, 0, 9, 4, 1, None, np_),           # out NULL
           lib.hm_scan_k_cpu(b"x", 1, 0, 9, 4, 1, buf, None),           # n NULL
           lib.hm_scan_k_cpu(None, 3, 0, 9, 4, 1, buf, np_),            # msg NULL, len > 0
           lib.hm_scan_k(None, b"x", 1, 0, 9, 4, buf, np_)]             # no context
    assert bad == [_lib.HM_ERR_INVALID] * 6
    assert n.value == 777 and (int(buf[0].hash), int(buf[0].nonce)) == SENTINEL
    st = _lib.hm_scan_k_stats()
    assert lib.hm_scan_k_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID
    for k in (0, 33, 1 << 32, -1):
        with pytest.raises(_lib.HipMinerError) as e:
            _lib.scan_k_cpu(b"x", 0, 9, k)
        assert e.value.rc == _lib.HM_ERR_INVALID
    # the empty message passed as NULL
    assert lib.hm_scan_k_cpu(None, 0, 0, 500, 3, 2, buf, np_) == _lib.HM_OK
    assert n.value == 3
    assert [(int(buf[i].hash), int(buf[i].nonce)) for i in range(3)] == _lib.scan_k_cpu(b"", 0, 500, 3)


def test_scan_k_stats_layout_matches_header(tmp_path):
    """The ctypes mirror of hm_scan_k_stats has the header's C layout, the
    header pins its 1.19 size, and the older structs keep theirs."""
    fields = [f for f, _ in _lib.hm_scan_k_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %d %zu %zu %zu\\n", sizeof(hm_scan_k_stats), HM_SCAN_K_STATS_SIZE_1_19,'
             ' sizeof(hm_collect_stats), sizeof(hm_find_k_stats), sizeof(hm_stats));']
    lines += [f'  printf("%zu\\n", offsetof(hm_scan_k_stats, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:5] == [ctypes.sizeof(_lib.hm_scan_k_stats), 56, 48, 64, 168]
    assert out[0] == 56
    assert out[5:] == [getattr(_lib.hm_scan_k_stats, f).offset for f in fields]
    assert fields == ["wall_ms", "kernel_ms", "nonces", "inserted", "compactions", "launches",
                      "ndev", "k", "count"]


def test_makefile_facts():
    text = open(os.path.join(CSRC, "Makefile")).read()
    link = re.search(r"^\$\(BUILD\)/hipminer_scan\.hsaco:(.*)$", text, re.M).group(1).split()
    # the last two objects stay where other tests pin them; the new one is just in front
    assert link[-3:] == ["$(BUILD)/scan_k_kernels.co.o", "$(BUILD)/fused_find_k_kernels.co.o",
                         "$(BUILD)/find_k_kernels.co.o"]
    asm = re.search(r"^asm:(.*)$", text, re.M).group(1).split()
    assert "$(BUILD)/scan_k_kernels.aligned.s" in asm
    objs = re.search(r"^HIP_HOST_OBJS := \$\(addprefix \$\(BUILD\)/,(.*)\)$", text, re.M).group(1)
    assert "scan_k.o" in objs.split()
    files = bid.source_files()
    assert "distributed_bitcoinminer_amd/csrc/scan_k_kernels.hip" in files
    assert "distributed_bitcoinminer_amd/csrc/scan_k.cpp" in files


@pytest.mark.parametrize("case", range(len(RANGES)))
def test_cpu_against_sorted_oracle(oracle_mod, path, case):
    m, lo, hi = RANGES[case]
    want = oracle_sorted(oracle_mod, m, lo, hi)
    assert len(want) == hi - lo + 1 <= 3000
    for k in KS:
        for t in THREADS:
            got = _lib.scan_k_cpu(m, lo, hi, k, threads=t)
            assert got == want[:k], (m, lo, hi, k, t, got[:3], want[:3])
    assert _lib.scan_k_cpu(m, lo, hi, 1, threads=0) == [oracle_mod.c_scan(m, lo, hi)]


def test_threads_split_a_larger_range(oracle_mod, path):
    """16 threads get a chunk each only from 65536 nonces up: the merge of 16
    lists, against hm_collect_cpu's dense list sorted."""
    m, lo, hi = b"bradfitz", 9_000, 9_000 + 70_000
    total, recs = _lib.collect_cpu(m, lo, hi, MAXU64, hi - lo + 1, threads=4)
    assert total == hi - lo + 1
    want = sorted(recs)
    for k in KS:
        for t in (1, 3, 16, 0):
            assert _lib.scan_k_cpu(m, lo, hi, k, threads=t) == want[:k], (k, t)
    assert want[0] == oracle_mod.c_scan(m, lo, hi)


def test_first_record_is_the_golden_scan(golden, path):
    kats = [k for k in golden["scan_kats"] if int(k["hi"]) - int(k["lo"]) < 10**6]
    if path == "c":  # the portable compression on a subset (it is ~4x slower)
        kats = [k for k in kats if int(k["hi"]) - int(k["lo"]) <= 20000]
    assert kats
    for i, kat in enumerate(kats):
        m = bytes.fromhex(kat["msg_hex"])
        lo, hi = int(kat["lo"]), int(kat["hi"])
        k, t = KS[i % 3], (1, 3, 16, 0)[i % 4]
        got = _lib.scan_k_cpu(m, lo, hi, k, threads=t)
        if lo > hi:
            assert got == []
            continue
        assert got[0] == (int(kat["hash"]), int(kat["nonce"])), kat.get("name")
        assert len(got) == min(k, hi - lo + 1) and got == sorted(got)
        assert all(lo <= n <= hi and _lib.host_hash(m, n) == h for h, n in got)


def test_edges_and_untouched_tail(oracle_mod):
    m = b"bradfitz"
    # an empty range: *n = 0, out unwritten
    rc, n, buf = scan_k_raw(m, 5, 4, 32, 2)
    assert (rc, n) == (_lib.HM_OK, 0) and all(r == SENTINEL for r in buf)
    # span < k: every nonce, nothing beyond out[*n)
    want = oracle_sorted(oracle_mod, m, 95, 104)
    rc, n, buf = scan_k_raw(m, 95, 104, 32, 3)
    assert (rc, n) == (_lib.HM_OK, 10) and buf[:10] == want
    assert all(r == SENTINEL for r in buf[10:])
    # the top of the nonce space: all 20 records, nonce 2^64-1 among them
    lo = MAXU64 - 19
    want = oracle_sorted(oracle_mod, m, lo, MAXU64)
    for t in THREADS:
        rc, n, buf = scan_k_raw(m, lo, MAXU64, 32, t)
        assert (rc, n) == (_lib.HM_OK, 20) and buf[:20] == want, t
        assert MAXU64 in [r[1] for r in buf[:20]] and all(r == SENTINEL for r in buf[20:])
    # span >= k: exactly k records, out[k] untouched
    want = oracle_sorted(oracle_mod, m, 0, 2999)
    for k in KS:
        rc, n, buf = scan_k_raw(m, 0, 2999, k, 3)
        assert (rc, n) == (_lib.HM_OK, k) and buf[:k] == want[:k] and buf[k] == SENTINEL


SAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include "hipminer.h"
static int below(const hm_result *a, const hm_result *b) {
    return a->hash < b->hash || (a->hash == b->hash && a->nonce < b->nonce);
}
int main(void) {
    const char *msg = "bradfitz";
    const size_t len = strlen(msg);
    int threads[] = {1, 3, 16};
    uint32_t ks[] = {1, 5, 32};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            hm_result out[33], one;
            size_t n = 777;
            out[ks[j]].hash = 0xA5A5A5A5A5A5A5A5ull;
            if (hm_scan_k_cpu((const uint8_t *)msg, len, 0, 99999, ks[j], threads[i], out, &n))
                return 2;
            if (n != ks[j] || out[ks[j]].hash != 0xA5A5A5A5A5A5A5A5ull) return 3;
            for (size_t r = 0; r < n; ++r) {
                /* the record's hash: the one-nonce scan */
                if (out[r].nonce > 99999 ||
                    hm_scan_cpu((const uint8_t *)msg, len, out[r].nonce, out[r].nonce, 1, &one) ||
                    one.hash != out[r].hash)
                    return 4;
                if (r && !below(&out[r - 1], &out[r])) return 5;
            }
            if (hm_scan_cpu((const uint8_t *)msg, len, 0, 99999, threads[i], &one)) return 6;
            if (one.hash != out[0].hash || one.nonce != out[0].nonce) return 7;
            /* digit-count changes, span < k, the top of the nonce space, empty */
            if (hm_scan_k_cpu((const uint8_t *)msg, len, 95, 104, 32, threads[i], out, &n) || n != 10)
                return 8;
            if (hm_scan_k_cpu((const uint8_t *)msg, len, ~0ull - 19, ~0ull, 32, threads[i], out, &n) ||
                n != 20)
                return 9;
            if (hm_scan_k_cpu((const uint8_t *)msg, len, 5, 4, ks[j], threads[i], out, &n) || n != 0)
                return 10;
            if (hm_scan_k_cpu(NULL, 0, 9990, 10010, ks[j], threads[i], out, &n) ||
                n != (ks[j] < 21 ? ks[j] : 21))
                return 11;
        }
    if (hm_scan_k_cpu((const uint8_t *)msg, len, 0, 9, 0, 1, NULL, NULL) != HM_ERR_INVALID) return 12;
    puts("san ok");
    return 0;
}
"""


def test_address_and_ub_sanitizer_standalone(tmp_path):
    """host_scan.cpp and plan.cpp built with -fsanitize=address,undefined into
    a stand-alone program (its own main) that runs the small cases above from
    1, 3 and 16 threads: nothing reported.  (The pattern of the stand-alone
    ThreadSanitizer program of tests/test_find_host.py.)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = tmp_path / "san_main.c.cpp"
    main.write_text(SAN_MAIN)
    exe = tmp_path / "san_scan_k"
    inc = os.path.join(ROOT, "include")
    # the sanitizer runtimes are linked statically: the program then needs nothing of
    # its environment (a shared ASan runtime insists on being the first library loaded)
    static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") and \
        not cxx.endswith("clang++") else ["-static-libsan"]
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-fsanitize=address,undefined", *static,
           "-fno-sanitize-recover=undefined", "-pthread", "-Wno-unknown-pragmas", f"-I{inc}",
           "-o", str(exe), str(main), os.path.join(CSRC, "host_scan.cpp"),
           os.path.join(CSRC, "plan.cpp")]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "san ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(ALIGNED), reason="library not built")
def test_shipped_scan_k_kernels_are_placed():
    """The tiled and chained hm_scan_k kernels keep one innermost hot loop (the
    compaction is unrolled, so it adds no loop inside it) and the placement
    pass holds every 8-byte VALU instruction of it at 4 mod 8."""
    from tests.test_placement import al
    with open(ALIGNED) as f:
        lines = f.read().split("\n")
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        obj = os.path.join(td, "a.o")
        al.assemble(ALIGNED, obj)
        funcs = al.disassemble(obj)
    where = al.source_insts(lines)
    hot = [s for s in where if "hm_scan_k_tiled_kernel" in s or "hm_scan_k_chained_kernel" in s]
    assert len(hot) == 33  # 32 tiled layouts + chained
    for sym in hot:
        insts = funcs[sym]
        loop = al.hot_loop(insts, al.inner_headers(lines, where[sym]))
        assert loop is not None, sym
        good, n = al.stats(insts, *loop)
        assert good == n and n > 300, (sym, good, n)

"""hm_collect_many_cpu (ABI 1.15) without a GPU: hm_collect's answer for every
request of a batch -- the exact totals, their sum and, when the sum fits the
call's ONE cap, every record request-major and ascending by nonce inside a
request.  The oracle is tests/test_collect_host.py's oracle_loop (the committed
C oracle's first-hit search iterated).  Checked with both compressions: a few
dozen seeded requests, empty requests and target = 0, repeated requests, the
top of the nonce space, the size-query ladder with sentinels around the buffer
and the totals, every invalid argument with the outputs untouched, the struct
layouts against a gcc compile of the header, the exported symbols, and the new
kernel's code-object metadata in the build's assembly.  No GPU needed."""
import ctypes
import os
import random
import re
import subprocess

from distributed_bitcoinminer_amd import _lib
from distributed_bitcoinminer_amd import build_id as bid
from tests.test_collect_host import oracle_loop, path  # noqa: F401  (path: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXU64 = (1 << 64) - 1
NEW_SYMBOLS = ("hm_collect_many", "hm_collect_many_cpu", "hm_collect_many_stats_sized")
SENTINEL = 0xA5A5A5A5A5A5A5A5
U64P = ctypes.POINTER(ctypes.c_uint64)
PAD = 3  # guard records on either side of the caller's buffer


def expected(oracle_mod, requests):
    """(total, totals, per-request record lists) by the rule of the header."""
    recs = [oracle_loop(oracle_mod, m or b"", lo, hi, T) if lo <= hi and T else []
            for m, lo, hi, T in requests]
    per = [len(r) for r in recs]
    return sum(per), per, recs


def seeded_requests(seed, n):
    """n requests of a few hundred to a few thousand nonces, every message
    length class, ranges across digit-count changes, targets 2^64 / 10..1000."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        m = bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 8, 54, 55, 56, 63, 64, 120])))
        lo = max(0, 10**rng.randrange(1, 20) - rng.randrange(1, 1500))
        hi = min(MAXU64, lo + rng.randrange(3000))
        out.append((m, lo, hi, 2**64 // 10**rng.randrange(1, 4)))
    return out


def many_raw(call, requests, cap):
    """A collect_many entry point through ctypes, the buffer of `cap` records
    with PAD sentinel records before and after it, the totals (a sentinel word
    on either side) and *total preset: (rc, total, totals, the records inside
    the buffer as (hash, nonce) pairs, all guards intact)."""
    arr, n, keep = _lib.collect_requests(requests)
    per = (ctypes.c_uint64 * (n + 2))(*([SENTINEL] * (n + 2)))
    buf = (ctypes.c_uint64 * (2 * (cap + 2 * PAD)))(*([SENTINEL] * (2 * (cap + 2 * PAD))))
    total = ctypes.c_uint64(777)
    out = ctypes.cast(ctypes.addressof(buf) + 16 * PAD, ctypes.POINTER(_lib.hm_result))
    rc = call(arr, n, ctypes.cast(ctypes.addressof(per) + 8, U64P), out if cap else None, cap,
              ctypes.byref(total))
    del keep
    words = list(buf)
    inner = words[2 * PAD:2 * (PAD + cap)]
    guards = words[:2 * PAD] + words[2 * (PAD + cap):] + [per[0], per[n + 1]]
    return (rc, int(total.value), [int(x) for x in per[1:n + 1]],
            list(zip(inner[0::2], inner[1::2])), all(g == SENTINEL for g in guards))


def check_cap_ladder(call, requests, exp):
    """The totals and the request-major records under every buffer size of the
    size-query contract: fitting, exactly total, total - 1 (out untouched,
    totals written), and 0 with NULL."""
    total, per, recs = exp
    flat = [r for rs in recs for r in rs]
    assert total >= 2 and len(flat) == total
    untouched = (SENTINEL, SENTINEL)
    for cap in (total + 5, total):
        rc, t, totals, got, intact = many_raw(call, requests, cap)
        assert (rc, t, totals) == (_lib.HM_OK, total, per) and intact
        assert got[:total] == flat
        assert all(x == untouched for x in got[total:])   # nothing beyond total is touched
    rc, t, totals, got, intact = many_raw(call, requests, total - 1)
    assert (rc, t, totals) == (_lib.HM_OK, total, per) and intact
    assert all(x == untouched for x in got)               # not written at all
    rc, t, totals, got, intact = many_raw(call, requests, 0)
    assert (rc, t, totals, got) == (_lib.HM_OK, total, per, []) and intact


def cpu_many(threads):
    lib = _lib.load()
    return lambda arr, n, per, out, cap, tot: lib.hm_collect_many_cpu(arr, n, threads, per, out,
                                                                      cap, tot)


def test_version_symbols_and_sources():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 15
    assert set(NEW_SYMBOLS) <= set(_lib.header_symbols())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert callable(_lib.Context.collect_many) and callable(_lib.Context.count_many)
    assert callable(_lib.Context.collect_many_stats) and callable(_lib.collect_many_cpu)
    dbg = open(os.path.join(ROOT, "include", "hipminer_debug.h")).read()
    assert int(re.search(r"#define HM_OPT_COLLECT_WINDOW (\d+)", dbg).group(1)) == 22 == \
        _lib.HM_OPT_COLLECT_WINDOW
    files = bid.source_files()
    for f in ("fused_collect_kernels.hip", "collect_many.cpp"):
        assert f"distributed_bitcoinminer_amd/csrc/{f}" in files, f


def test_struct_layouts_match_header(tmp_path):
    structs = (_lib.hm_collect_request, _lib.hm_collect_many_stats)
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %zu %d %zu\\n", sizeof(hm_collect_request),',
             "         sizeof(hm_collect_many_stats), HM_COLLECT_MANY_STATS_SIZE_1_15,",
             "         sizeof(hm_find_request));"]
    for s in structs:
        lines += [f'  printf("%zu\\n", offsetof({s.__name__}, {f}));' for f, _ in s._fields_]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:4] == [40, 64, 64, 40]
    assert [ctypes.sizeof(s) for s in structs] == [40, 64]
    assert out[4:] == [getattr(s, f).offset for s in structs for f, _ in s._fields_]
    fields = [f for f, _ in _lib.hm_collect_many_stats._fields_]
    assert fields == ["wall_ms", "kernel_ms", "nonces", "total", "tasks", "requests", "fused",
                      "fallback", "launches", "ndev", "overflow"]
    # the sized getter refuses a NULL context
    st = _lib.hm_collect_many_stats()
    assert _lib.load().hm_collect_many_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID


def test_against_the_oracle(oracle_mod, path):
    """Three dozen seeded requests with empty ones (lo > hi), target = 0,
    repeated requests and the last 501 nonces of u64 among them; 1, 3 and 16
    threads; and hm_collect_cpu request by request."""
    reqs = seeded_requests(41, 36)
    reqs.insert(5, (b"empty", 10, 9, MAXU64))
    reqs.insert(11, (b"no target", 0, 5000, 0))
    reqs.insert(20, reqs[3])
    reqs.append(reqs[3])
    reqs.append((b"top of u64", MAXU64 - 500, MAXU64, 2**64 // 10))
    reqs.append((b"top of u64", MAXU64 - 500, MAXU64, MAXU64))
    exp = expected(oracle_mod, reqs)
    assert exp[1][5] == exp[1][11] == 0 and exp[2][20] == exp[2][3] == exp[2][-3]
    assert exp[1][-1] == 501 and exp[2][-1][-1][1] == MAXU64 and 20 < exp[1][-2] < 100
    assert sum(p > 0 for p in exp[1]) > 30
    for t in (1, 3, 16):
        assert _lib.collect_many_cpu(reqs, exp[0], threads=t) == exp, t
        assert _lib.collect_many_cpu(reqs, exp[0] - 1, threads=t) == (exp[0], exp[1], None), t
        assert _lib.collect_many_cpu(reqs, 0, threads=t) == (exp[0], exp[1], None), t
    for i, (m, lo, hi, T) in enumerate(reqs):
        assert _lib.collect_cpu(m, lo, hi, T, exp[1][i] + 1, threads=2) == (exp[1][i], exp[2][i]), i
    # nothing qualifies anywhere: fits any cap, the pure count included
    none = [(m, lo, hi, 1) for m, lo, hi, _ in reqs[:6]]
    assert _lib.collect_many_cpu(none, 0) == (0, [0] * 6, [[]] * 6)


def test_cap_ladder_with_sentinels(oracle_mod, path):
    reqs = seeded_requests(42, 12)
    reqs.insert(4, (b"empty", 3, 2, MAXU64))
    reqs.append((b"top of u64", MAXU64 - 500, MAXU64, 2**64 // 4))
    exp = expected(oracle_mod, reqs)
    for t in (1, 3):
        check_cap_ladder(cpu_many(t), reqs, exp)


def test_edges_and_invalid_arguments(oracle_mod):
    lib = _lib.load()
    h7 = oracle_mod.c_hash(b"", 7)
    rq = _lib.hm_collect_request
    per = (ctypes.c_uint64 * 4)(*([SENTINEL] * 4))
    out = (_lib.hm_result * 2)()
    for r in out:
        r.hash = r.nonce = SENTINEL
    total = ctypes.c_uint64(777)
    tp = ctypes.byref(total)

    def untouched():
        return (total.value == 777 and all(x == SENTINEL for x in per) and
                all(r.hash == SENTINEL and r.nonce == SENTINEL for r in out))
    # n = 0: HM_OK, *total = 0, nothing else written; every pointer but total may be NULL
    assert lib.hm_collect_many_cpu(None, 0, 1, None, None, 0, tp) == _lib.HM_OK
    assert total.value == 0
    total.value = 777
    assert untouched()
    # the empty message passed as NULL; strict '<'; an empty request among others
    arr = (rq * 3)(rq(None, 0, 7, 7, h7 + 1), rq(b"x", 1, 5, 4, MAXU64), rq(None, 0, 7, 7, h7))
    assert lib.hm_collect_many_cpu(arr, 3, 1, per, out, 2, tp) == _lib.HM_OK
    assert total.value == 1 and list(per) == [1, 0, 0, SENTINEL]
    assert (out[0].hash, out[0].nonce, out[1].hash) == (h7, 7, SENTINEL)
    assert _lib.collect_many_cpu([(None, 7, 7, h7 + 1), (b"x", 5, 4, MAXU64), (b"", 7, 7, h7)],
                                 2) == (1, [1, 0, 0], [[(h7, 7)], [], []])
    for i in range(4):
        per[i] = SENTINEL
    out[0].hash = out[0].nonce = SENTINEL
    total.value = 777
    good = (rq * 2)(rq(b"x", 1, 0, 9, MAXU64), rq(b"y", 1, 0, 9, MAXU64))
    nomsg = (rq * 2)(rq(b"x", 1, 0, 9, MAXU64), rq(None, 3, 0, 9, MAXU64))
    inv = [lib.hm_collect_many_cpu(good, -1, 1, per, out, 2, tp),                  # n < 0
           lib.hm_collect_many_cpu(None, 2, 1, per, out, 2, tp),                   # reqs NULL
           lib.hm_collect_many_cpu(good, 2, 1, None, out, 2, tp),                  # totals NULL
           lib.hm_collect_many_cpu(good, 2, 1, per, out, 2, None),                 # total NULL
           lib.hm_collect_many_cpu(None, 0, 1, None, None, 0, None),               # ... with n = 0 too
           lib.hm_collect_many_cpu(good, 2, 1, per, out, (1 << 24) + 1, tp),       # cap too large
           lib.hm_collect_many_cpu(good, 2, 1, per, None, 2, tp),                  # cap > 0, out NULL
           lib.hm_collect_many_cpu(nomsg, 2, 1, per, out, 2, tp),                  # msg NULL, len > 0
           lib.hm_collect_many(None, good, 2, per, out, 2, tp)]                    # no context
    assert inv == [_lib.HM_ERR_INVALID] * len(inv)
    assert untouched()


def test_fused_collect_kernel_metadata():
    """The new kernel's code-object metadata in the build's shipped assembly:
    no scratch and no VGPR spills, as every kernel of the library."""
    text = open(os.path.join(ROOT, "build", "hipminer", "fused_collect_kernels.aligned.s")).read()
    blocks = [b for b in re.split(r"\n  - ", text.split("amdhsa.kernels:")[-1])
              if re.search(r"\.name:\s+\S*hm_fused_collect_kernel", b)]
    assert len(blocks) == 1
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blocks[0]).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blocks[0]).group(1)) == 0

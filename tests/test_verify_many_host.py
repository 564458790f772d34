"""hm_verify_many_cpu (ABI 1.14) without a GPU: which (hash, nonce) records of
MANY lists, each with its own message and target, are bad -- hm_verify's answer
for every request of a batch.  The oracle is the committed C oracle's c_hash
per nonce; the expected counts and (request, index) refs are computed here from
it, and hm_verify_cpu is asked request by request as a second witness.  Checked
with both compressions: a batch that mixes every message length 0..130 at the
40 digit-edge nonces with two corruption sets (one long enough that 16 threads
each take a part, so parts begin and end inside requests), the size-query
contract with guard words around the refs, every invalid argument, the empty
batch, empty requests, the empty message as NULL, the struct layouts against a
gcc compile of the header, the exported symbols, and once a ThreadSanitizer
build of the host path as a stand-alone program.  No GPU needed."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np

from distributed_bitcoinminer_amd import _lib
from distributed_bitcoinminer_amd import build_id as bid
from tests.test_verify_host import (LENGTHS, MAXU64, SENTINEL, corruption_set, edge_case,
                                    oracle_hashes, path)  # noqa: F401  (path: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")
NEW_SYMBOLS = ("hm_verify_many", "hm_verify_many_cpu", "hm_verify_many_stats_sized")
U64P = ctypes.POINTER(ctypes.c_uint64)
PAD = 3  # guard refs on either side of the caller's buffer


def expected(oracle_mod, requests):
    """(bad, per-request counts, refs ascending) of [(msg, records, target), ...]
    by the rule of the header, from the oracle's hashes."""
    per, refs = [], []
    for i, (m, recs, target) in enumerate(requests):
        r = np.ascontiguousarray(recs, dtype=np.uint64).reshape(-1, 2)
        true = oracle_hashes(oracle_mod, m, [int(x) for x in r[:, 1]])
        bad = [k for k in range(r.shape[0]) if int(r[k, 0]) != true[k] or int(r[k, 0]) >= target]
        per.append(len(bad))
        refs += [(i, k) for k in bad]
    return sum(per), per, refs


def edge_requests(oracle_mod, lengths=LENGTHS):
    """One honest request per message length: edge_case's message with its 40
    shuffled edge nonces, at a target just above its largest hash."""
    out = []
    for length in lengths:
        m, ns = edge_case(length)
        hs = oracle_hashes(oracle_mod, m, ns)
        out.append((m, np.array(list(zip(hs, ns)), dtype=np.uint64), max(hs) + 1))
    return out


def corrupt_third(requests, seed):
    """A seeded third of all records of `requests` corrupted -- a hash bit, the
    nonce + 1, or hash = target, in turn: new requests (the inputs are not
    changed).  What is bad afterwards is for expected() to say."""
    rng = random.Random(seed)
    where = [(i, k) for i, (_, r, _) in enumerate(requests) for k in range(len(r))]
    out = [(m, r.copy(), t) for m, r, t in requests]
    for j, (i, k) in enumerate(rng.sample(where, len(where) // 3)):
        _, r, target = out[i]
        kind = j % 3
        if kind == 1 and int(r[k, 1]) == MAXU64:
            kind = 0  # nonce + 1 would wrap
        if kind == 0:
            r[k, 0] ^= np.uint64(1 << rng.randrange(64))
        elif kind == 1:
            r[k, 1] += np.uint64(1)
        else:
            r[k, 0] = np.uint64(target)
    return out


def many_raw(call, requests, cap):
    """A verify_many entry point through ctypes, the refs buffer of `cap` refs
    with PAD sentinel refs before and after it, the counts and *bad preset:
    (rc, bad, counts, refs inside the buffer as (request, index) pairs, all
    guards intact)."""
    arr, n, keep = _lib.verify_requests(requests)
    per = np.full(n + 2, SENTINEL, dtype=np.uint64)
    buf = np.full(2 * (cap + 2 * PAD), SENTINEL, dtype=np.uint64)
    bad = ctypes.c_uint64(777)
    refs = ctypes.cast(ctypes.c_void_p(buf.ctypes.data + 16 * PAD),
                       ctypes.POINTER(_lib.hm_bad_ref))
    rc = call(arr, n, per[1:].ctypes.data_as(U64P), refs if cap else None, cap, ctypes.byref(bad))
    del keep
    inner = [int(x) for x in buf[2 * PAD:2 * (PAD + cap)]]
    guards = [int(x) for x in buf[:2 * PAD]] + [int(x) for x in buf[2 * (PAD + cap):]] + \
        [int(per[0]), int(per[n + 1])]
    return (rc, int(bad.value), [int(x) for x in per[1:n + 1]],
            list(zip(inner[0::2], inner[1::2])), all(g == SENTINEL for g in guards))


def check_many_cap_contract(call, requests, exp):
    """The counts and the ascending refs under every buffer size of the
    size-query contract: fitting, exactly bad, bad - 1 (refs untouched, counts
    written), and 0 with NULL."""
    total, per, refs = exp
    assert total >= 2
    untouched = (SENTINEL, SENTINEL)
    for cap in (total + 5, total):
        rc, bad, counts, got, intact = many_raw(call, requests, cap)
        assert (rc, bad, counts) == (_lib.HM_OK, total, per) and intact
        assert got[:total] == refs
        assert all(x == untouched for x in got[total:])   # nothing beyond bad is touched
    rc, bad, counts, got, intact = many_raw(call, requests, total - 1)
    assert (rc, bad, counts) == (_lib.HM_OK, total, per) and intact
    assert all(x == untouched for x in got)               # not written at all
    rc, bad, counts, got, intact = many_raw(call, requests, 0)
    assert (rc, bad, counts, got) == (_lib.HM_OK, total, per, []) and intact


def cpu_many(threads):
    lib = _lib.load()
    return lambda arr, n, per, refs, cap, bad: lib.hm_verify_many_cpu(arr, n, threads, per, refs,
                                                                      cap, bad)


def test_version_symbols_and_sources():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 14
    assert set(NEW_SYMBOLS) <= set(_lib.header_symbols())
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert callable(_lib.Context.verify_many) and callable(_lib.Context.verify_many_stats)
    assert callable(_lib.verify_many_cpu)
    dbg = open(os.path.join(ROOT, "include", "hipminer_debug.h")).read()
    assert int(re.search(r"#define HM_OPT_VERIFY_JOBS (\d+)", dbg).group(1)) == 21 == \
        _lib.HM_OPT_VERIFY_JOBS
    files = bid.source_files()
    for f in ("verify_many_kernels.hip", "verify_many.cpp"):
        assert f"distributed_bitcoinminer_amd/csrc/{f}" in files, f


def test_struct_layouts_match_header(tmp_path):
    structs = (_lib.hm_verify_request, _lib.hm_bad_ref, _lib.hm_verify_many_stats)
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %zu %zu %d %zu\\n", sizeof(hm_verify_request), sizeof(hm_bad_ref),',
             "         sizeof(hm_verify_many_stats), HM_VERIFY_MANY_STATS_SIZE_1_14,",
             "         sizeof(hm_verify_stats));"]
    for s in structs:
        lines += [f'  printf("%zu\\n", offsetof({s.__name__}, {f}));' for f, _ in s._fields_]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:5] == [40, 16, 72, 72, 56]
    assert [ctypes.sizeof(s) for s in structs] == [40, 16, 72]
    assert out[5:] == [getattr(s, f).offset for s in structs for f, _ in s._fields_]
    fields = [f for f, _ in _lib.hm_verify_many_stats._fields_]
    assert fields == ["wall_ms", "kernel_ms", "copy_ms", "records", "bad", "tasks", "requests",
                      "launches", "copies", "ndev", "overflow", "reserved"]
    # the sized getter refuses a NULL context
    st = _lib.hm_verify_many_stats()
    assert _lib.load().hm_verify_many_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID


def test_against_the_oracle_and_verify_cpu(oracle_mod, path):
    """Every message length at the digit edges (a third of the records
    corrupted), an empty request, and two corruption sets; 1, 3 and 16
    threads."""
    reqs = corrupt_third(edge_requests(oracle_mod), seed=31)
    reqs.insert(40, (b"nothing", np.empty((0, 2), dtype=np.uint64), 5))
    for n, seed, m in ((400, 7, b"bradfitz"), (20000, 8, b"bradfitz")):
        mm, target, recs, _ = corruption_set(oracle_mod, n, seed, m)
        reqs.append((mm, recs, target))
    exp = expected(oracle_mod, reqs)
    assert exp[0] > 10000 and exp[1][40] == 0 and all(c > 0 for c in exp[1][:40])
    for t in (1, 3, 16):
        bad, per, refs = _lib.verify_many_cpu(reqs, exp[0], threads=t)
        assert (bad, per) == exp[:2], t
        assert refs == exp[2], t
        assert _lib.verify_many_cpu(reqs, exp[0] - 1, threads=t) == (exp[0], exp[1], None)
    # hm_verify_cpu, request by request
    for i, (m, recs, target) in enumerate(reqs):
        bad, idx = _lib.verify_cpu(m, recs, target, len(recs), threads=2)
        assert bad == exp[1][i], i
        assert [(i, int(k)) for k in idx] == [r for r in exp[2] if r[0] == i], i
    # the honest batch: nothing bad
    honest = edge_requests(oracle_mod)
    assert _lib.verify_many_cpu(honest, 4, threads=3) == (0, [0] * len(honest), [])


def test_cap_contract_with_guard_words(oracle_mod, path):
    reqs = corrupt_third(edge_requests(oracle_mod, range(30, 70)), seed=32)
    mm, target, recs, _ = corruption_set(oracle_mod, 400, 7)
    reqs.append((mm, recs, target))
    exp = expected(oracle_mod, reqs)
    for t in (1, 3):
        check_many_cap_contract(cpu_many(t), reqs, exp)
    # every record bad (target 0), and a target of UINT64_MAX: the hash alone
    m, target, recs, _ = corruption_set(oracle_mod, 400, 7)
    zero = [(m, recs, 0), (m, recs, MAXU64)]
    e = expected(oracle_mod, zero)
    assert e[1][0] == 400 and 0 < e[1][1] < 400
    check_many_cap_contract(cpu_many(2), zero, e)


def test_edges_and_invalid_arguments(oracle_mod):
    lib = _lib.load()
    h7 = oracle_mod.c_hash(b"", 7)
    one = (_lib.hm_result * 1)()
    one[0].hash, one[0].nonce = h7, 7
    rq = _lib.hm_verify_request
    per = (ctypes.c_uint64 * 4)(*([SENTINEL] * 4))
    refs = (_lib.hm_bad_ref * 2)()
    for r in refs:
        r.request = r.index = SENTINEL
    bad = ctypes.c_uint64(777)
    bp = ctypes.byref(bad)

    def untouched():
        return (bad.value == 777 and all(x == SENTINEL for x in per) and
                all(r.request == SENTINEL and r.index == SENTINEL for r in refs))
    # nreq = 0: HM_OK, *bad = 0, nothing else written; every pointer but bad may be NULL
    assert lib.hm_verify_many_cpu(None, 0, 1, None, None, 0, bp) == _lib.HM_OK
    assert bad.value == 0
    bad.value = 777
    assert untouched()
    # the empty message passed as NULL; strict '<'; an n = 0 request (NULL list) among others
    arr = (rq * 3)(rq(None, 0, one, 1, h7 + 1), rq(b"x", 1, None, 0, MAXU64),
                   rq(None, 0, one, 1, h7))
    assert lib.hm_verify_many_cpu(arr, 3, 1, per, refs, 2, bp) == _lib.HM_OK
    assert bad.value == 1 and list(per) == [0, 0, 1, SENTINEL]
    assert (refs[0].request, refs[0].index, refs[1].request) == (2, 0, SENTINEL)
    assert _lib.verify_many_cpu([(b"", [(h7, 7)], h7 + 1), (b"x", [], 9), (b"", [(h7, 7)], h7)],
                                2) == (1, [0, 0, 1], [(2, 0)])
    # a record whose hash is UINT64_MAX is bad at target UINT64_MAX
    assert _lib.verify_many_cpu([(b"", [(MAXU64, 7)], MAXU64)], 1) == (1, [1], [(0, 0)])
    for i in range(4):
        per[i] = SENTINEL
    refs[0].request = refs[0].index = SENTINEL
    bad.value = 777
    good = (rq * 2)(rq(b"x", 1, one, 1, MAXU64), rq(b"y", 1, one, 1, MAXU64))
    nomsg = (rq * 2)(rq(b"x", 1, one, 1, MAXU64), rq(None, 3, one, 1, MAXU64))
    nolist = (rq * 2)(rq(b"x", 1, one, 1, MAXU64), rq(b"y", 1, None, 1, MAXU64))
    inv = [lib.hm_verify_many_cpu(good, -1, 1, per, refs, 2, bp),              # nreq < 0
           lib.hm_verify_many_cpu(None, 2, 1, per, refs, 2, bp),               # reqs NULL
           lib.hm_verify_many_cpu(good, 2, 1, None, refs, 2, bp),              # bad_per_req NULL
           lib.hm_verify_many_cpu(good, 2, 1, per, refs, 2, None),             # bad NULL
           lib.hm_verify_many_cpu(None, 0, 1, None, None, 0, None),            # ... with nreq = 0 too
           lib.hm_verify_many_cpu(good, 2, 1, per, refs, (1 << 20) + 1, bp),   # cap too large
           lib.hm_verify_many_cpu(good, 2, 1, per, None, 2, bp),               # cap > 0, refs NULL
           lib.hm_verify_many_cpu(nomsg, 2, 1, per, refs, 2, bp),              # msg NULL, len > 0
           lib.hm_verify_many_cpu(nolist, 2, 1, per, refs, 2, bp),             # recs NULL, n > 0
           lib.hm_verify_many(None, good, 2, per, refs, 2, bp)]                # no context
    assert inv == [_lib.HM_ERR_INVALID] * len(inv)
    assert untouched()


TSAN_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hipminer.h"
int main(void) {
    enum { R = 37, N = 40000 };
    static hm_result recs[N];
    static uint64_t nonces[N], hashes[N];
    static hm_verify_request reqs[R];
    static uint64_t per[R], again[R];
    static hm_bad_ref refs[N], refs2[N];
    static char msgs[R][16];
    /* R requests of growing size over one record array, a message each */
    size_t at = 0;
    uint64_t x = 88172645463325252ull, want = 0;
    for (int r = 0; r < R; ++r) {
        size_t n = r == 5 ? 0 : (r + 1 == R ? N - at : 60 * (size_t)(r + 1));
        snprintf(msgs[r], sizeof msgs[r], "message %d", r);
        reqs[r].msg = (const uint8_t *)msgs[r];
        reqs[r].len = strlen(msgs[r]);
        reqs[r].recs = recs + at;
        reqs[r].n = n;
        reqs[r].target = ~0ull;
        for (size_t i = 0; i < n; ++i) {      /* xorshift; a shift spreads the digit counts */
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            nonces[at + i] = x >> ((at + i) % 64);
        }
        if (hm_hash_many_cpu(reqs[r].msg, reqs[r].len, nonces + at, n, 1, hashes + at)) return 1;
        for (size_t i = 0; i < n; ++i) {
            recs[at + i].nonce = nonces[at + i];
            recs[at + i].hash = hashes[at + i] ^ ((at + i) % 5 == 0);
            want += (at + i) % 5 == 0;        /* every fifth record is wrong */
        }
        at += n;
    }
    if (at != N) return 2;
    int threads[] = {1, 3, 16};
    for (int t = 0; t < 3; ++t) {
        uint64_t bad = 0;
        if (hm_verify_many_cpu(reqs, R, threads[t], t ? again : per, t ? refs2 : refs, N, &bad))
            return 3;
        if (bad != want) return 4;
        if (t && (memcmp(again, per, sizeof per) || memcmp(refs2, refs, bad * sizeof refs[0])))
            return 5;
        for (uint64_t k = 0; k < bad; ++k) {  /* ref k is flattened record 5 k */
            const hm_bad_ref *f = &refs[k];
            if ((size_t)(reqs[f->request].recs - recs) + f->index != 5 * k) return 6;
        }
        uint64_t count = 0;                  /* every part overflows the cap */
        reqs[0].target = 0;
        int rc = hm_verify_many_cpu(reqs, R, threads[t], again, refs2, 16, &count);
        reqs[0].target = ~0ull;
        if (rc || count < want || again[5] != 0 || again[0] != 60) return 7;
    }
    puts("tsan ok");
    return 0;
}
"""


def test_thread_sanitizer_standalone(tmp_path):
    """host_scan.cpp and plan.cpp built with -fsanitize=thread into a
    stand-alone program that calls hm_verify_many_cpu from 1, 3 and 16 threads:
    no data race reported.  Nothing is preloaded and nothing is loaded into
    Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = tmp_path / "tsan_main.c.cpp"
    main.write_text(TSAN_MAIN)
    exe = tmp_path / "tsan_verify_many"
    inc = os.path.join(ROOT, "include")
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-fsanitize=thread", "-pthread",
           "-Wno-unknown-pragmas", f"-I{inc}", "-o", str(exe), str(main),
           os.path.join(CSRC, "host_scan.cpp"), os.path.join(CSRC, "plan.cpp")]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "tsan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]

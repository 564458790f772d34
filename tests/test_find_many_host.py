"""hm_find_many (ABI 1.13) without a GPU: the exported symbols and version, the
layouts of hm_find_request and hm_find_many_stats against a gcc compile of the
header, the debug option's id, hm_find_many_cpu against the C oracle's first-hit
search on a mixed batch, and the argument checks of both entry points."""
import ctypes
import os
import random
import re
import subprocess

from distributed_bitcoinminer_amd import _lib
from distributed_bitcoinminer_amd import build_id as bid

MAX = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_HEADER = os.path.join(ROOT, "include", "hipminer_debug.h")


def test_symbols_and_version():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 13
    new = {"hm_find_many", "hm_find_many_cpu", "hm_find_many_stats_sized"}
    assert new <= set(_lib.header_symbols())
    for s in new:
        assert hasattr(lib, s), s
    assert callable(_lib.Context.find_many) and callable(_lib.Context.find_many_stats)
    assert callable(_lib.find_many_cpu)


def test_build_id_covers_the_new_sources():
    files = bid.source_files()
    for f in ("fused_find_kernels.hip", "find_many.cpp"):
        assert f"distributed_bitcoinminer_amd/csrc/{f}" in files, f


def test_struct_layouts_match_header(tmp_path):
    rf = [f for f, _ in _lib.hm_find_request._fields_]
    sf = [f for f, _ in _lib.hm_find_many_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %zu %d\\n", sizeof(hm_find_request), sizeof(hm_find_many_stats),',
             "         HM_FIND_MANY_STATS_SIZE_1_13);"]
    lines += [f'  printf("%zu\\n", offsetof(hm_find_request, {f}));' for f in rf]
    lines += [f'  printf("%zu\\n", offsetof(hm_find_many_stats, {f}));' for f in sf]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:3] == [40, 64, 64]
    assert ctypes.sizeof(_lib.hm_find_request) == 40
    assert ctypes.sizeof(_lib.hm_find_many_stats) == 64
    assert out[3:3 + len(rf)] == [getattr(_lib.hm_find_request, f).offset for f in rf]
    assert out[3 + len(rf):] == [getattr(_lib.hm_find_many_stats, f).offset for f in sf]
    # sized getter: refuses a NULL context and a size below the 1.13 layout
    st = _lib.hm_find_many_stats()
    lib = _lib.load()
    assert lib.hm_find_many_stats_sized(None, ctypes.byref(st), 64) == _lib.HM_ERR_INVALID


def test_find_window_option_is_a_debug_hook():
    assert _lib.HM_OPT_FIND_WINDOW == 20
    with open(DEBUG_HEADER) as f:
        assert re.search(r"#define\s+HM_OPT_FIND_WINDOW\s+20\b", f.read())
    with open(_lib.HEADER_PATH) as f:
        assert "HM_OPT_FIND_WINDOW" not in f.read()


def _mixed_batch(oracle_mod):
    """100 requests: message lengths 0..130, ranges of at most 2*10^4 nonces
    anywhere in u64, and the edge cases of the contract."""
    rng = random.Random(1313)
    reqs = []
    top = (MAX - 1000, MAX)
    for i in range(100):
        m = bytes(rng.randrange(256) for _ in range((i * 131) // 100 if i < 99 else 130))
        if i % 10 == 0:
            lo, hi = top
        elif i % 3 == 0:
            lo = max(0, 10**rng.randrange(1, 20) - rng.randrange(1, 10_000))
            hi = min(MAX, lo + rng.randrange(20_000))
        else:
            lo = rng.randrange(MAX)
            hi = min(MAX, lo + rng.randrange(20_000))
        mn = oracle_mod.c_scan(m, lo, hi)[0]
        kind = i % 6
        if kind == 0:
            T = mn          # strict '<': none
        elif kind == 1:
            T = mn + 1      # the argmin
        elif kind == 2:
            T = 0
        elif kind == 3:
            lo, hi, T = (hi, lo, MAX) if lo < hi else (5, 4, MAX)   # lo > hi
        else:
            T = 2**64 // 10**rng.randrange(1, 5)
        reqs.append((m, lo, hi, T))
    assert {len(r[0]) for r in reqs} >= {0, 130}
    return reqs


def test_find_many_cpu_vs_oracle(oracle_mod):
    reqs = _mixed_batch(oracle_mod)
    want = [oracle_mod.c_find(m, lo, hi, T) for m, lo, hi, T in reqs]
    assert any(w is None for w in want) and any(w is not None for w in want)
    assert any(w is not None and w[1] > MAX - 1001 for w in want)
    for threads in (1, 5):
        assert _lib.find_many_cpu(reqs, threads=threads) == want, threads
    assert _lib.find_many_cpu([]) == []


def _raw(reqs):
    arr = (_lib.hm_find_request * max(1, len(reqs)))()
    keep = []
    for i, (m, n, lo, hi, T) in enumerate(reqs):
        keep.append(m)
        arr[i] = _lib.hm_find_request(m, n, lo, hi, T)
    return arr, keep


def test_invalid_arguments_leave_outputs_untouched():
    lib = _lib.load()
    arr, _keep = _raw([(b"bradfitz", 8, 0, 999, MAX), (None, 3, 0, 9, MAX)])
    ok, _keep2 = _raw([(b"bradfitz", 8, 0, 999, MAX), (None, 0, 0, 9, MAX)])

    def sentinel():
        outs = (_lib.hm_result * 2)()
        found = (ctypes.c_int * 2)()
        for i in range(2):
            outs[i] = _lib.hm_result(0x5a5a, 0xa5a5)
            found[i] = 77
        return outs, found

    def untouched(outs, found):
        return all((outs[i].hash, outs[i].nonce, found[i]) == (0x5a5a, 0xa5a5, 77)
                   for i in range(2))

    cpu = lambda a, n, o, f: lib.hm_find_many_cpu(a, n, 1, o, f)    # noqa: E731
    gpu = lambda a, n, o, f: lib.hm_find_many(None, a, n, o, f)     # noqa: E731
    for call in (cpu, gpu):
        outs, found = sentinel()
        assert call(ok, -1, outs, found) == _lib.HM_ERR_INVALID
        assert call(None, 2, outs, found) == _lib.HM_ERR_INVALID
        assert call(ok, 2, None, found) == _lib.HM_ERR_INVALID
        assert call(ok, 2, outs, None) == _lib.HM_ERR_INVALID
        assert call(arr, 2, outs, found) == _lib.HM_ERR_INVALID    # msg NULL, len 3
        assert untouched(outs, found)
    # a NULL context is invalid whatever else is passed
    outs, found = sentinel()
    assert gpu(ok, 0, outs, found) == _lib.HM_ERR_INVALID
    # n = 0 is HM_OK and writes nothing; a NULL message of length 0 is the empty one
    assert cpu(None, 0, None, None) == _lib.HM_OK
    assert cpu(ok, 0, outs, found) == _lib.HM_OK and untouched(outs, found)
    assert cpu(ok, 2, outs, found) == _lib.HM_OK
    assert [(outs[i].hash, outs[i].nonce, found[i]) for i in range(2)] == [
        (_lib.host_hash(b"bradfitz", 0), 0, 1), (_lib.host_hash(b"", 0), 0, 1)]

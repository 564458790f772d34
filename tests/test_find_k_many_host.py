"""hm_find_k_many (ABI 1.17) without a GPU: a batch of hm_find_k requests, each
answered as hm_find_k answers it -- the k LOWEST nonces of an inclusive range
whose hash is below a target, ascending, request i's records in its own slot
out[off_i .. off_i + k_i) with off_i the sum of the earlier k's.
The oracle is test_collect_host's iterated c_find (the committed C oracle's
first-hit search restarted at answer + 1; never hm_collect_cpu), truncated to
k.  Checked: the version, the symbols, the build's lists, the kernel's name in
the embedded code object, the layouts against a gcc compile of the header,
every invalid-argument case, and hm_find_k_many_cpu under both compressions
with 1, 2, 7 and 16 threads on a mixed batch, with sentinels around every
answer."""
import ctypes
import os
import re
import subprocess

import pytest

from distributed_bitcoinminer_amd import _lib
from distributed_bitcoinminer_amd import build_id as bid
from tests.test_collect_host import oracle_collect

MAX = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")
THREADS = (1, 2, 7, 16)
SENTINEL = (0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A)


@pytest.fixture(params=["sha", "c"])
def path(request, monkeypatch):
    """Run the test once with each compression (as tests/test_find_k_host.py)."""
    if request.param == "c":
        monkeypatch.setenv("HM_CPU_NO_SHA", "1")
    else:
        monkeypatch.delenv("HM_CPU_NO_SHA", raising=False)
    return request.param


def test_version_and_symbols():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 17
    names = {"hm_find_k_many", "hm_find_k_many_cpu", "hm_find_k_many_stats_sized"}
    assert names <= set(_lib.header_symbols())
    for s in names:
        assert hasattr(lib, s), s
    assert callable(_lib.Context.find_k_many) and callable(_lib.Context.find_k_many_stats)
    assert callable(_lib.find_k_many_cpu)
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define HM_FIND_K_MAX \(1u << (\d+)\)", text).group(1)) == 20
    assert _lib.HM_FIND_K_MAX == 1 << 20
    # no new option id: the hooks are hm_find_many's and hm_find_k's
    debug = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "hipminer_debug.h")).read()
    ids = [int(x) for x in re.findall(r"#define HM_OPT_[A-Z_]+\s+(\d+)", text + debug)]
    assert max(ids) == 23 == _lib.HM_OPT_FIND_K_BUF and _lib.HM_OPT_FIND_WINDOW == 20


def test_makefile_lists_the_new_sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "find_k_many.o" in mk.split("HIP_HOST_OBJS :=")[1].splitlines()[0]
    link = next(l for l in mk.splitlines() if l.startswith("$(BUILD)/hipminer_scan.hsaco:"))
    objs = link.split()[1:]
    # just before find_k_kernels.co.o, which stays last: every kernel but
    # hm_find_k's keeps its offset in the code object
    assert objs.index("$(BUILD)/fused_find_k_kernels.co.o") == \
        objs.index("$(BUILD)/find_k_kernels.co.o") - 1 == len(objs) - 2
    asm = next(l for l in mk.splitlines() if l.startswith("asm:"))
    assert "$(BUILD)/fused_find_k_kernels.aligned.s" in asm.split()
    files = bid.source_files()
    for f in ("fused_find_k_kernels.hip", "find_k_many.cpp"):
        assert os.path.exists(os.path.join(CSRC, f)), f
        assert f"distributed_bitcoinminer_amd/csrc/{f}" in files, f


def test_makefile_lists_the_shared_batch_sources():
    """The task walker and the chunk runner the three batch calls share."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "batch.o" in mk.split("HIP_HOST_OBJS :=")[1].splitlines()[0].rstrip(")").split()
    deps = mk.split("SRCS_DEPS :=")[1].splitlines()[0].split()
    assert "fused_tasks.hpp" in deps
    files = bid.source_files()
    for f in ("fused_tasks.hpp", "batch.cpp"):
        assert os.path.exists(os.path.join(CSRC, f)), f
        assert f"distributed_bitcoinminer_amd/csrc/{f}" in files, f


def test_code_object_holds_the_kernel():
    lib = _lib.load()
    p = ctypes.c_void_p()
    size = lib.hm_debug_code_object(ctypes.byref(p))
    blob = ctypes.string_at(p.value, size)
    assert b"_ZN2hm22hm_fused_find_k_kernelENS_14FusedFindKArgsE" in blob


def test_layouts_match_header(tmp_path):
    """The ctypes mirrors of hm_find_k_request and hm_find_k_many_stats have the
    header's C layout, and the header pins the stats' 1.17 size at 80."""
    rf = [f for f, _ in _lib.hm_find_k_request._fields_]
    sf = [f for f, _ in _lib.hm_find_k_many_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %zu %d %zu\\n", sizeof(hm_find_k_request), sizeof(hm_find_k_many_stats),',
             "         HM_FIND_K_MANY_STATS_SIZE_1_17, sizeof(hm_find_k_stats));"]
    lines += [f'  printf("%zu\\n", offsetof(hm_find_k_request, {f}));' for f in rf]
    lines += [f'  printf("%zu\\n", offsetof(hm_find_k_many_stats, {f}));' for f in sf]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:4] == [48, 80, 80, 64]
    assert ctypes.sizeof(_lib.hm_find_k_request) == 48
    assert ctypes.sizeof(_lib.hm_find_k_many_stats) == 80
    assert out[4:4 + len(rf)] == [getattr(_lib.hm_find_k_request, f).offset for f in rf]
    assert out[4 + len(rf):] == [getattr(_lib.hm_find_k_many_stats, f).offset for f in sf]
    assert rf == ["msg", "len", "lo", "hi", "target", "k"]
    assert sf == ["wall_ms", "kernel_ms", "nonces_enqueued", "tasks_total", "tasks_run", "records",
                  "found", "requests", "fused", "fallback", "overflow", "launches", "ndev"]


def raw_requests(reqs):
    """[(msg or None, len, lo, hi, T, k), ...] as a raw hm_find_k_request array."""
    arr = (_lib.hm_find_k_request * max(1, len(reqs)))()
    keep = []
    for i, (m, n, lo, hi, T, k) in enumerate(reqs):
        keep.append(m)
        arr[i] = _lib.hm_find_k_request(m, n, lo, hi, T, k)
    return arr, keep


def test_invalid_arguments_leave_outputs_untouched():
    lib = _lib.load()
    ok, _k0 = raw_requests([(b"bradfitz", 8, 0, 999, MAX, 2), (None, 0, 0, 9, MAX, 1)])
    bad = {"msg NULL, len 3": [(b"bradfitz", 8, 0, 999, MAX, 2), (None, 3, 0, 9, MAX, 1)],
           "k == 0": [(b"bradfitz", 8, 0, 999, MAX, 2), (b"x", 1, 0, 9, MAX, 0)],
           "k > HM_FIND_K_MAX": [(b"x", 1, 0, 9, MAX, (1 << 20) + 1), (b"x", 1, 0, 9, MAX, 1)]}

    def sentinel():
        out = (_lib.hm_result * 3)()
        counts = (ctypes.c_size_t * 2)()
        for i in range(3):
            out[i].hash, out[i].nonce = SENTINEL
        counts[0] = counts[1] = 777
        return out, counts

    def untouched(out, counts):
        return all((int(r.hash), int(r.nonce)) == SENTINEL for r in out) and \
            list(counts) == [777, 777]

    cpu = lambda a, n, o, c: lib.hm_find_k_many_cpu(a, n, 1, o, c)    # noqa: E731
    gpu = lambda a, n, o, c: lib.hm_find_k_many(None, a, n, o, c)     # noqa: E731  no context
    for call in (cpu, gpu):
        out, counts = sentinel()
        assert call(ok, -1, out, counts) == _lib.HM_ERR_INVALID
        assert call(None, 2, out, counts) == _lib.HM_ERR_INVALID
        assert call(ok, 2, None, counts) == _lib.HM_ERR_INVALID
        assert call(ok, 2, out, None) == _lib.HM_ERR_INVALID
        for what, reqs in bad.items():
            arr, _k = raw_requests(reqs)
            assert call(arr, 2, out, counts) == _lib.HM_ERR_INVALID, what
        assert untouched(out, counts)
    # a NULL context is invalid whatever else is passed, an empty batch included
    out, counts = sentinel()
    assert gpu(ok, 0, out, counts) == _lib.HM_ERR_INVALID
    assert gpu(ok, 2, out, counts) == _lib.HM_ERR_INVALID
    st = _lib.hm_find_k_many_stats()
    assert lib.hm_find_k_many_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID
    # n = 0 is HM_OK and writes nothing; a NULL message of length 0 is the empty one
    assert cpu(None, 0, None, None) == _lib.HM_OK
    assert cpu(ok, 0, out, counts) == _lib.HM_OK and untouched(out, counts)
    assert cpu(ok, 2, out, counts) == _lib.HM_OK
    assert list(counts) == [2, 1]
    assert [(int(r.hash), int(r.nonce)) for r in out] == [
        (_lib.host_hash(b"bradfitz", 0), 0), (_lib.host_hash(b"bradfitz", 1), 1),
        (_lib.host_hash(b"", 0), 0)]
    with pytest.raises(_lib.HipMinerError):
        _lib.find_k_many_cpu([(b"x", 0, 9, MAX, 0)])
    with pytest.raises(_lib.HipMinerError):
        _lib.find_k_many_cpu([(b"x", 0, 9, MAX, (1 << 20) + 1)])
    # k = HM_FIND_K_MAX itself is accepted
    assert [len(r) for r in _lib.find_k_many_cpu([(b"x", 0, 9, MAX, 1 << 20)], threads=1)] == [10]
    assert _lib.find_k_many_cpu([]) == []


_BATCH = {}


def mixed_batch(oracle_mod):
    """65 requests and their oracle answers, computed once: several messages
    (lengths 0..130), k of 1, 2, 7 and total + 5, dead requests (lo > hi,
    target = 0) and the top of the nonce space."""
    if _BATCH:
        return _BATCH["reqs"], _BATCH["want"]
    reqs, want = [], []
    for i in range(65):
        m = bytes((i * 7 + j) % 251 for j in range((i * 130) // 64))
        T = 2**64 // (40, 300, 2000)[i % 3]
        if i % 8 == 5:
            lo, hi = MAX - 3000 - i, MAX
        elif i % 8 == 6:
            lo = 10**(1 + i % 19) - 700
            hi = lo + 2500
        else:
            lo = (i * 0x9E3779B97F4A7C15) % (MAX - 5000)
            hi = lo + 1500 + 37 * i
        full = oracle_collect(oracle_mod, m, lo, hi, T)
        k = (1, 2, 7, len(full) + 5)[i % 4]
        if i % 16 == 9:
            lo, hi, full = hi, lo, []      # lo > hi
        elif i % 16 == 11:
            T, full = 0, []
        reqs.append((m if i != 0 else None, lo, hi, T, k))
        want.append(full[:k])
    assert {len(r[0] or b"") for r in reqs} >= {0, 130}
    assert any(w and w[-1][1] > MAX - 3100 for w in want)
    assert any(len(w) == r[4] for w, r in zip(want, reqs) if r[4] > 2)
    assert any(0 < len(w) < r[4] for w, r in zip(want, reqs))
    _BATCH.update(reqs=reqs, want=want)
    return reqs, want


def test_find_k_many_cpu_vs_oracle(oracle_mod, path):
    reqs, want = mixed_batch(oracle_mod)
    for t in THREADS:
        assert _lib.find_k_many_cpu(reqs, threads=t) == want, t
    # request by request it is hm_find_k_cpu
    for (m, lo, hi, T, k), w in list(zip(reqs, want))[:12]:
        assert _lib.find_k_cpu(m or b"", lo, hi, T, k, threads=2) == w


def test_nothing_beyond_the_counts_is_touched(oracle_mod, path):
    """Sentinel-filled `out` of sum(k) + 3 records: inside a slot nothing at or
    past out[off_i + counts[i]] changes, nor anything past the last slot."""
    reqs, want = mixed_batch(oracle_mod)
    arr, n, keep = _lib.find_k_requests(reqs)
    total = sum(r[4] for r in reqs)
    for t in THREADS:
        out = (_lib.hm_result * (total + 3))()
        for r in out:
            r.hash, r.nonce = SENTINEL
        counts = (ctypes.c_size_t * n)(*([777] * n))
        assert _lib.load().hm_find_k_many_cpu(arr, n, t, out, counts) == _lib.HM_OK
        flat = [(int(r.hash), int(r.nonce)) for r in out]
        off = 0
        for i, (w, r) in enumerate(zip(want, reqs)):
            assert counts[i] == len(w), (t, i)
            assert flat[off:off + len(w)] == w, (t, i)
            assert all(x == SENTINEL for x in flat[off + len(w):off + r[4]]), (t, i)
            off += r[4]
        assert off == total and flat[total:] == [SENTINEL] * 3
    del keep

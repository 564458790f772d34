"""hm_cancel (ABI 1.18), host side: the symbol, the version, the error code's
text, the NULL context, the hm_cancel_stats layout, and the cancel state machine
(csrc/cancel.hpp: the flag, cancel_mu, in-flight) driven from two threads in a
stand-alone ThreadSanitizer program.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

from distributed_bitcoinminer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_bitcoinminer_amd", "csrc")


def test_symbol_and_version():
    lib = _lib.load()
    v = lib.hm_version()
    assert v >> 16 == 1 and v & 0xFFFF >= 18
    assert {"hm_cancel", "hm_cancel_stats_sized"} <= set(_lib.header_symbols())
    assert hasattr(lib, "hm_cancel") and hasattr(lib, "hm_cancel_stats_sized")


def test_error_code_in_header_and_strerror():
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define HM_ERR_CANCELLED \((-?\d+)\)", text).group(1)) == \
        _lib.HM_ERR_CANCELLED == -8
    msg = _lib.strerror(-8)
    assert msg and msg != "unknown error"
    others = [_lib.strerror(rc) for rc in range(0, -8, -1)] + [_lib.strerror(-99)]
    assert msg not in others
    e = _lib.HipMinerCancelled(_lib.HM_ERR_CANCELLED, "hm_find")
    assert isinstance(e, _lib.HipMinerError) and e.rc == -8 and msg in str(e)


def test_null_context():
    lib = _lib.load()
    assert lib.hm_cancel(None) == _lib.HM_ERR_INVALID
    st = _lib.hm_cancel_stats()
    assert lib.hm_cancel_stats_sized(None, ctypes.byref(st), ctypes.sizeof(st)) == \
        _lib.HM_ERR_INVALID


def test_no_relay_hook_is_a_debug_export():
    """The null-relay hook is hm_debug_no_relay of hipminer_debug.h: not in the
    product header, and not an option id (the ids still end at 23)."""
    inc = os.path.dirname(_lib.HEADER_PATH)
    dbg = open(os.path.join(inc, "hipminer_debug.h")).read()
    assert re.search(r"\bint hm_debug_no_relay\(hm_ctx \*ctx, int on\);", dbg)
    assert "no_relay" not in open(_lib.HEADER_PATH).read()
    assert _lib.load().hm_debug_no_relay(None, 1) == _lib.HM_ERR_INVALID


def test_cancel_stats_layout_matches_header(tmp_path):
    """The ctypes mirror of hm_cancel_stats has the header's C layout, and the
    header pins its 1.18 size."""
    fields = [f for f, _ in _lib.hm_cancel_stats._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{_lib.HEADER_PATH}"',
             "int main(void) {",
             '  printf("%zu %d\\n", sizeof(hm_cancel_stats), HM_CANCEL_STATS_SIZE_1_18);']
    lines += [f'  printf("%zu\\n", offsetof(hm_cancel_stats, {f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[:2] == [ctypes.sizeof(_lib.hm_cancel_stats), 32]
    assert out[2:] == [getattr(_lib.hm_cancel_stats, f).offset for f in fields]
    assert {"latency_ms", "launches_in_flight", "family", "cancels", "cancelled_calls"} == \
        set(fields)


# Two threads on one CancelState whose flag is a plain word.  The caller runs
# ROUNDS calls: begin, a stubbed wait (a few polls of seen(), as the host tests
# the flag after each wait), finish with HM_ERR_CANCELLED if it saw the flag and
# HM_OK otherwise.  The canceller calls request() at irregular intervals.
#   exit 3/4   a request with nothing in flight returned non-zero or set the flag
#   exit 5     a call saw the flag although no request returned 1 during it: a
#              cancel was observed by a call it was not issued during
#   exit 6     a call began with the flag still set (stickiness)
#   exit 7/8   the record disagrees with what the two threads counted
#   exit 9     one of the two outcomes never happened: the run shows nothing
TSAN_MAIN = r"""
#include <stdio.h>
#include <atomic>
#include <thread>
#include "cancel.hpp"

int main() {
    const int ROUNDS = 100000;
    hm::CancelState st;
    uint32_t word = 0;
    st.flag = &word;
    if (st.request() != 0 || st.seen()) return 3;          /* no call at all */
    st.begin(HM_CANCEL_FAMILY_FIND);
    st.finish(HM_OK);
    if (st.request() != 0 || st.seen()) return 4;          /* after a call */

    std::atomic<bool> done{false};
    uint64_t ones = 0, zeros = 0;
    std::thread canceller([&] {
        uint32_t x = 12345u;
        while (!done.load(std::memory_order_acquire)) {
            if (st.request() == 1) ++ones; else ++zeros;
            x = x * 1664525u + 1013904223u;
            for (uint32_t i = 0, n = (x >> 20) & 1023u; i < n; ++i) std::this_thread::yield();
        }
    });
    uint64_t cancelled = 0, finished = 0;
    int bad = 0;
    for (int r = 0; r < ROUNDS && !bad; ++r) {
        const uint64_t c0 = st.read().cancels;   /* a request from here to begin() returns 0 */
        st.begin(1 + r % 4);
        if (st.seen() && st.read().cancels == c0) { bad = 6; }
        bool saw = false;
        for (int poll = 0; poll < 1 + r % 7 && !saw; ++poll) {  /* the stubbed wait */
            std::this_thread::yield();
            saw = st.seen();
        }
        if (saw) st.observed(r % 5);
        st.finish(saw ? HM_ERR_CANCELLED : HM_OK);
        const hm_cancel_stats s = st.read();     /* a request since finish() returned 0 */
        if (saw) {
            ++cancelled;
            if (s.cancels == c0) bad = 5;
            if (s.family != 1 + r % 4 || s.launches_in_flight != r % 5 || s.latency_ms < 0) bad = 7;
        } else {
            ++finished;
        }
    }
    done.store(true, std::memory_order_release);
    canceller.join();
    if (bad) return bad;
    const hm_cancel_stats s = st.read();
    if (s.cancelled_calls != cancelled || s.cancels != ones) return 8;
    if (!cancelled || !finished || !zeros) return 9;
    printf("tsan ok cancelled=%llu finished=%llu ones=%llu zeros=%llu\n",
           (unsigned long long)cancelled, (unsigned long long)finished,
           (unsigned long long)ones, (unsigned long long)zeros);
    return 0;
}
"""


def test_thread_sanitizer_standalone(tmp_path):
    """cancel.hpp built with -fsanitize=thread into a stand-alone program (as
    tests/test_find_host.py builds the host search): 10^5 calls on one thread
    against a canceller on another.  A cancel with nothing in flight returns
    0 and leaves no trace; one issued during a call is observed by that call
    or by none; no data race is reported."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = tmp_path / "tsan_cancel.cpp"
    main.write_text(TSAN_MAIN)
    exe = tmp_path / "tsan_cancel"
    cmd = [cxx, "-O1", "-g", "-std=c++20", "-fsanitize=thread", "-pthread", f"-I{CSRC}",
           "-o", str(exe), str(main)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "tsan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]
    print(r.stdout.strip())

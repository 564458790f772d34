"""ctypes binding of libhipminer.so (include/hipminer.h; the test hooks and
debug exports of include/hipminer_debug.h).

The library is built in-tree by ``__graft_entry__.build()`` (or ``make -C
distributed_bitcoinminer_amd/csrc``).  There is no silent fallback: if the
library or a GPU is missing, the calls raise ``HipMinerError``; ``scan_cpu``
(hm_scan_cpu) is the host scan a caller may pick explicitly.
"""
from __future__ import annotations

import ctypes
import os
import re
import struct
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhipminer.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hipminer.h")

HM_OK = 0
HM_ERR_INVALID = -1
HM_ERR_NO_DEVICE = -2
HM_ERR_HIP = -3
HM_ERR_NOMEM = -4
HM_ERR_RCCL = -5
HM_ERR_INTERNAL = -6
HM_ERR_TIMEOUT = -7
HM_ERR_CANCELLED = -8

HM_KIND_NONE, HM_KIND_GENERIC, HM_KIND_TILED, HM_KIND_CHAINED, HM_KIND_FUSED = 0, 1, 2, 3, 4
HM_OPT_FORCE_GENERIC, HM_OPT_MERGE_RCCL, HM_OPT_GRID_PER_CU, HM_OPT_STREAMS = 1, 2, 3, 4
HM_OPT_TABLE_DIGITS = 7
HM_OPT_TABLE_ROWS_CAP = 8
HM_OPT_TEST_MID_SYNC = 9
HM_OPT_FUSED = 10
HM_OPT_FUSED_FLAGS = 11
HM_OPT_FUSED_PARTS = 12
HM_OPT_DEADLINE_MS = 13
HM_OPT_FUSED_TAIL = 14
HM_OPT_TAIL_FUSED = 15
HM_OPT_QUEUE_BATCH = 17
HM_OPT_VERIFY_CHUNK = 19
HM_OPT_FIND_WINDOW = 20
HM_OPT_VERIFY_JOBS = 21
HM_OPT_COLLECT_WINDOW = 22
HM_OPT_FIND_K_BUF = 23
HM_MERGE_NONE, HM_MERGE_HOST, HM_MERGE_RCCL = 0, 1, 2


class HipMinerError(RuntimeError):
    def __init__(self, rc: int, what: str = ""):
        self.rc = rc
        msg = strerror(rc) if _lib_or_none() else f"rc={rc}"
        super().__init__(f"{what}: {msg} (rc={rc})" if what else f"{msg} (rc={rc})")


class HipMinerCancelled(HipMinerError):
    """A find, find_k, find_many or find_k_many that Context.cancel stopped
    (rc = HM_ERR_CANCELLED): nothing was written and the context is usable."""


def _error(rc: int, what: str) -> HipMinerError:
    return (HipMinerCancelled if rc == HM_ERR_CANCELLED else HipMinerError)(rc, what)


class hm_result(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint64), ("nonce", ctypes.c_uint64)]


class hm_request(ctypes.Structure):
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t),
                ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64)]


class _Stats(ctypes.Structure):
    """Base of the stats structs of include/hipminer.h."""

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        if "dom_kernel" in d:
            d["dom_kernel"] = d["dom_kernel"].decode()
        return d


class hm_stats(_Stats):
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("dom_kernel_ms", ctypes.c_double), ("nonces", ctypes.c_uint64),
                ("dom_nonces", ctypes.c_uint64), ("dom_compressions", ctypes.c_uint64),
                ("launches", ctypes.c_int32), ("dom_kind", ctypes.c_int32),
                ("ndev", ctypes.c_int32), ("dom_grid", ctypes.c_int32),
                ("dom_launches", ctypes.c_int32), ("merge", ctypes.c_int32),
                ("dom_kernel", ctypes.c_char * 64), ("dom_compressions_eff", ctypes.c_double),
                ("enqueue_ms", ctypes.c_double), ("mid_call_syncs", ctypes.c_int32),
                ("table_grows", ctypes.c_int32), ("deadline_ms", ctypes.c_double)]


class hm_find_stats(_Stats):
    """hm_find_stats of include/hipminer.h (ABI 1.10)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces_enqueued", ctypes.c_uint64), ("tasks_total", ctypes.c_uint64),
                ("tasks_run", ctypes.c_uint64), ("launches", ctypes.c_int32),
                ("ndev", ctypes.c_int32), ("found", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class hm_find_request(ctypes.Structure):
    """hm_find_request of include/hipminer.h (ABI 1.13)."""
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t),
                ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64),
                ("target", ctypes.c_uint64)]


class hm_find_many_stats(_Stats):
    """hm_find_many_stats of include/hipminer.h (ABI 1.13)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces_enqueued", ctypes.c_uint64), ("tasks_total", ctypes.c_uint64),
                ("tasks_run", ctypes.c_uint64), ("requests", ctypes.c_int32),
                ("found", ctypes.c_int32), ("fused", ctypes.c_int32),
                ("fallback", ctypes.c_int32), ("launches", ctypes.c_int32),
                ("ndev", ctypes.c_int32)]


class hm_find_k_stats(_Stats):
    """hm_find_k_stats of include/hipminer.h (ABI 1.16)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces_enqueued", ctypes.c_uint64), ("tasks_total", ctypes.c_uint64),
                ("tasks_run", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("launches", ctypes.c_int32), ("ndev", ctypes.c_int32),
                ("found", ctypes.c_int32), ("fallback", ctypes.c_int32)]


class hm_find_k_request(ctypes.Structure):
    """hm_find_k_request of include/hipminer.h (ABI 1.17)."""
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t),
                ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64),
                ("target", ctypes.c_uint64), ("k", ctypes.c_size_t)]


class hm_find_k_many_stats(_Stats):
    """hm_find_k_many_stats of include/hipminer.h (ABI 1.17)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces_enqueued", ctypes.c_uint64), ("tasks_total", ctypes.c_uint64),
                ("tasks_run", ctypes.c_uint64), ("records", ctypes.c_uint64),
                ("found", ctypes.c_uint64), ("requests", ctypes.c_int32),
                ("fused", ctypes.c_int32), ("fallback", ctypes.c_int32),
                ("overflow", ctypes.c_int32), ("launches", ctypes.c_int32),
                ("ndev", ctypes.c_int32)]


class hm_scan_k_stats(_Stats):
    """hm_scan_k_stats of include/hipminer.h (ABI 1.19)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces", ctypes.c_uint64), ("inserted", ctypes.c_uint64),
                ("compactions", ctypes.c_uint64), ("launches", ctypes.c_int32),
                ("ndev", ctypes.c_int32), ("k", ctypes.c_int32),
                ("count", ctypes.c_int32)]


class hm_cancel_stats(_Stats):
    """hm_cancel_stats of include/hipminer.h (ABI 1.18)."""
    _fields_ = [("latency_ms", ctypes.c_double), ("cancels", ctypes.c_uint64),
                ("cancelled_calls", ctypes.c_uint64), ("launches_in_flight", ctypes.c_int32),
                ("family", ctypes.c_int32)]


HM_CANCEL_FAMILY_NONE, HM_CANCEL_FAMILY_FIND, HM_CANCEL_FAMILY_FIND_K = 0, 1, 2
HM_CANCEL_FAMILY_FIND_MANY, HM_CANCEL_FAMILY_FIND_K_MANY = 3, 4


class hm_collect_stats(_Stats):
    """hm_collect_stats of include/hipminer.h (ABI 1.11)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces", ctypes.c_uint64), ("total", ctypes.c_uint64),
                ("launches", ctypes.c_int32), ("ndev", ctypes.c_int32),
                ("overflow", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class hm_verify_stats(_Stats):
    """hm_verify_stats of include/hipminer.h (ABI 1.12)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("copy_ms", ctypes.c_double), ("records", ctypes.c_uint64),
                ("bad", ctypes.c_uint64), ("launches", ctypes.c_int32),
                ("ndev", ctypes.c_int32), ("overflow", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class hm_verify_request(ctypes.Structure):
    """hm_verify_request of include/hipminer.h (ABI 1.14)."""
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t),
                ("recs", ctypes.POINTER(hm_result)), ("n", ctypes.c_size_t),
                ("target", ctypes.c_uint64)]


class hm_bad_ref(ctypes.Structure):
    """hm_bad_ref of include/hipminer.h (ABI 1.14)."""
    _fields_ = [("request", ctypes.c_uint64), ("index", ctypes.c_uint64)]


class hm_verify_many_stats(_Stats):
    """hm_verify_many_stats of include/hipminer.h (ABI 1.14)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("copy_ms", ctypes.c_double), ("records", ctypes.c_uint64),
                ("bad", ctypes.c_uint64), ("tasks", ctypes.c_uint64),
                ("requests", ctypes.c_int32), ("launches", ctypes.c_int32),
                ("copies", ctypes.c_int32), ("ndev", ctypes.c_int32),
                ("overflow", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class hm_collect_request(ctypes.Structure):
    """hm_collect_request of include/hipminer.h (ABI 1.15)."""
    _fields_ = [("msg", ctypes.c_char_p), ("len", ctypes.c_size_t),
                ("lo", ctypes.c_uint64), ("hi", ctypes.c_uint64),
                ("target", ctypes.c_uint64)]


class hm_collect_many_stats(_Stats):
    """hm_collect_many_stats of include/hipminer.h (ABI 1.15)."""
    _fields_ = [("wall_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("nonces", ctypes.c_uint64), ("total", ctypes.c_uint64),
                ("tasks", ctypes.c_uint64), ("requests", ctypes.c_int32),
                ("fused", ctypes.c_int32), ("fallback", ctypes.c_int32),
                ("launches", ctypes.c_int32), ("ndev", ctypes.c_int32),
                ("overflow", ctypes.c_int32)]


HM_COLLECT_CAP_MAX = 1 << 24
HM_FIND_K_MAX = 1 << 20
HM_SCAN_K_MAX = 32
HM_VERIFY_CAP_MAX = 1 << 20


def _prototypes() -> dict:
    """name -> (restype, argtypes) of every function include/hipminer.h
    declares and of the debug exports this binding uses."""
    P = ctypes.POINTER
    i, i64, u64, sz, dbl = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t,
                            ctypes.c_double)
    u32 = ctypes.c_uint32
    ctx, msg, ip, szp, u64p, res = (ctypes.c_void_p, ctypes.c_char_p, P(i), P(sz), P(u64),
                                    P(hm_result))
    rng = [msg, sz, u64, u64]  # msg, len, lo, hi
    table = {
        "hm_hash": (u64, [msg, sz, u64]),
        "hm_version": (i, []),
        "hm_build_id": (ctypes.c_char_p, []),
        "hm_strerror": (ctypes.c_char_p, [i]),
        "hm_partition": (i, rng + [i, u64p]),
        "hm_open": (i, [ip, i, P(ctx)]),
        "hm_close": (None, [ctx]),
        "hm_set_option": (i, [ctx, i, i64]),
        "hm_scan": (i, [ctx] + rng + [res]),
        "hm_scan_many": (i, [ctx, P(hm_request), i, res]),
        "hm_scan_checked": (i, [ctx] + rng + [res, u64p, u64p]),
        "hm_scan_cpu": (i, rng + [i, res]),
        "hm_scan_stats": (i, [ctx, P(hm_stats)]),
        "hm_find": (i, [ctx] + rng + [u64, res, ip]),
        "hm_find_cpu": (i, rng + [u64, i, res, ip]),
        "hm_find_many": (i, [ctx, P(hm_find_request), i, res, ip]),
        "hm_find_many_cpu": (i, [P(hm_find_request), i, i, res, ip]),
        "hm_find_k": (i, [ctx] + rng + [u64, sz, res, szp]),
        "hm_find_k_cpu": (i, rng + [u64, sz, i, res, szp]),
        "hm_find_k_many": (i, [ctx, P(hm_find_k_request), i, res, szp]),
        "hm_find_k_many_cpu": (i, [P(hm_find_k_request), i, i, res, szp]),
        "hm_cancel": (i, [ctx]),
        "hm_scan_k": (i, [ctx] + rng + [u32, res, szp]),
        "hm_scan_k_cpu": (i, rng + [u32, i, res, szp]),
        "hm_collect": (i, [ctx] + rng + [u64, res, sz, u64p]),
        "hm_collect_cpu": (i, rng + [u64, i, res, sz, u64p]),
        "hm_collect_many": (i, [ctx, P(hm_collect_request), i, u64p, res, sz, u64p]),
        "hm_collect_many_cpu": (i, [P(hm_collect_request), i, i, u64p, res, sz, u64p]),
        "hm_hash_many": (i, [ctx, msg, sz, u64p, sz, u64p]),
        "hm_hash_many_cpu": (i, [msg, sz, u64p, sz, i, u64p]),
        "hm_verify": (i, [ctx, msg, sz, res, sz, u64, u64p, sz, u64p]),
        "hm_verify_cpu": (i, [msg, sz, res, sz, u64, i, u64p, sz, u64p]),
        "hm_verify_many": (i, [ctx, P(hm_verify_request), i, u64p, P(hm_bad_ref), sz, u64p]),
        "hm_verify_many_cpu": (i, [P(hm_verify_request), i, i, u64p, P(hm_bad_ref), sz, u64p]),
        "hm_debug_code_object": (sz, [P(ctypes.c_void_p)]),
        "hm_debug_auto_deadline_ms": (dbl, rng + [i]),
        "hm_debug_streams_made": (i, [ctx, i]),
        "hm_debug_plan": (i, rng + [i, P(i64), i]),
        "hm_debug_no_relay": (i, [ctx, i]),
    }
    for cls in (hm_stats, hm_find_stats, hm_find_many_stats, hm_find_k_stats,
                hm_find_k_many_stats, hm_collect_stats, hm_collect_many_stats, hm_verify_stats,
                hm_verify_many_stats, hm_cancel_stats, hm_scan_k_stats):
        family = "scan" if cls is hm_stats else cls.__name__[3:-6]
        table[f"hm_{family}_stats_sized"] = (i, [ctx, P(cls), sz])
    return table


PROTOTYPES = _prototypes()

_lib = None
_lock = threading.Lock()


def _lib_or_none():
    return _lib


def load() -> ctypes.CDLL:
    """Load the in-tree libhipminer.so; raise if it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipMinerError(HM_ERR_NO_DEVICE,
                                f"{LIB_PATH} missing: run __graft_entry__.build()")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def strerror(rc: int) -> str:
    return load().hm_strerror(rc).decode()


def header_symbols() -> list[str]:
    """Function names declared in include/hipminer.h."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(hm_[a-z_]+)\s*\(", text)))


def as_bytes(msg) -> bytes:
    """Go strings are byte strings; str is encoded as UTF-8 (Go source literals)."""
    return msg.encode("utf-8") if isinstance(msg, str) else bytes(msg)


class Context:
    """One hipminer context (hm_open .. hm_close) on a set of HIP devices."""

    def __init__(self, devices=None):
        lib = load()
        handle = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = lib.hm_open(arr, len(devices), ctypes.byref(handle))
        else:
            rc = lib.hm_open(None, 0, ctypes.byref(handle))
        if rc != HM_OK:
            raise HipMinerError(rc, "hm_open")
        self._h = handle
        self._lib = lib

    def scan(self, msg, lo: int, hi: int) -> tuple[int, int]:
        m = as_bytes(msg)
        out = hm_result()
        rc = self._lib.hm_scan(self._h, m, len(m), lo, hi, ctypes.byref(out))
        if rc != HM_OK:
            raise HipMinerError(rc, "hm_scan")
        return int(out.hash), int(out.nonce)

    def scan_checked(self, msg, lo: int, hi: int) -> tuple[tuple[int, int], int, int]:
        """hm_scan_checked: ((hash, nonce), sum of all keys mod 2^64, nonces hashed)."""
        m = as_bytes(msg)
        out = hm_result()
        s, c = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._lib.hm_scan_checked(self._h, m, len(m), lo, hi, ctypes.byref(out),
                                       ctypes.byref(s), ctypes.byref(c))
        if rc != HM_OK:
            raise HipMinerError(rc, "hm_scan_checked")
        return (int(out.hash), int(out.nonce)), int(s.value), int(c.value)

    def scan_many(self, requests) -> list[tuple[int, int]]:
        """hm_scan_many over [(msg, lo, hi), ...]."""
        reqs = list(requests)
        n = len(reqs)
        keep = [as_bytes(m) for m, _, _ in reqs]
        arr = (hm_request * max(1, n))()
        for i, ((_, lo, hi), m) in enumerate(zip(reqs, keep)):
            arr[i] = hm_request(m, len(m), lo, hi)
        outs = (hm_result * max(1, n))()
        rc = self._lib.hm_scan_many(self._h, arr, n, outs)
        if rc != HM_OK:
            raise HipMinerError(rc, "hm_scan_many")
        return [(int(outs[i].hash), int(outs[i].nonce)) for i in range(n)]

    def _stats(self, getter: str, cls, what: str = None) -> dict:
        """The family's stats record through its hm_X_stats_sized, as a dict."""
        st = cls()
        rc = getattr(self._lib, getter)(self._h, ctypes.byref(st), ctypes.sizeof(st))
        if rc != HM_OK:
            raise HipMinerError(rc, what or getter)
        return st.as_dict()

    def stats(self) -> dict:
        return self._stats("hm_scan_stats_sized", hm_stats, "hm_scan_stats")

    def find(self, msg, lo: int, hi: int, target: int):
        """hm_find (ABI 1.10): (hash, nonce) of the LOWEST nonce in the
        inclusive [lo, hi] whose hash is below `target`, or None; the call
        stops early once that nonce is known."""
        m = as_bytes(msg)
        out = hm_result()
        found = ctypes.c_int(0)
        rc = self._lib.hm_find(self._h, m, len(m), lo, hi, target, ctypes.byref(out),
                               ctypes.byref(found))
        if rc != HM_OK:
            raise _error(rc, "hm_find")
        return (int(out.hash), int(out.nonce)) if found.value else None

    def cancel(self) -> bool:
        """hm_cancel (ABI 1.18): stop the find, find_k, find_many or
        find_k_many that another thread has in flight on this context.  True:
        such a call was in flight and is signalled -- it raises
        HipMinerCancelled, or returns its exact answer if that was already in
        hand.  False: nothing cancellable was in flight, and nothing is
        remembered (a later call is not affected).  ctypes releases the GIL
        for the duration of a foreign call, so a Python thread can call this
        while another is inside find(); it takes no lock and returns at once."""
        rc = self._lib.hm_cancel(self._h)
        if rc < 0:
            raise HipMinerError(rc, "hm_cancel")
        return rc == 1

    def cancel_stats(self) -> dict:
        """hm_cancel_stats_sized: cancels and cancelled calls since the context
        was opened; latency_ms, launches_in_flight and family of the last
        cancelled call."""
        return self._stats("hm_cancel_stats_sized", hm_cancel_stats)

    def find_stats(self) -> dict:
        """hm_find_stats_sized: work accounting of the last find on this context."""
        return self._stats("hm_find_stats_sized", hm_find_stats)

    def find_many(self, requests):
        """hm_find_many (ABI 1.13) over [(msg, lo, hi, target), ...]: for each
        request what Context.find returns, (hash, nonce) or None; each
        request's first 2^27 nonces run as one fused launch that exits early."""
        return _find_many(lambda arr, n, outs, found: self._lib.hm_find_many(
            self._h, arr, n, outs, found), "hm_find_many", requests)

    def find_many_stats(self) -> dict:
        """hm_find_many_stats_sized: work accounting of the last find_many on this context."""
        return self._stats("hm_find_many_stats_sized", hm_find_many_stats)

    def find_k(self, msg, lo: int, hi: int, target: int, k: int):
        """hm_find_k (ABI 1.16): the (hash, nonce) of the k LOWEST nonces in the
        inclusive [lo, hi] whose hash is below `target`, ascending by nonce --
        fewer than k when the range holds fewer; the call stops early once the
        k-th is known."""
        return _find_k(lambda m, out, n: self._lib.hm_find_k(
            self._h, m, len(m), lo, hi, target, k, out, n), "hm_find_k", msg, k)

    def find_k_stats(self) -> dict:
        """hm_find_k_stats_sized: work accounting of the last find_k on this context."""
        return self._stats("hm_find_k_stats_sized", hm_find_k_stats)

    def scan_k(self, msg, lo: int, hi: int, k: int):
        """hm_scan_k (ABI 1.19): the min(k, nonces of the range) lexicographically
        smallest (hash, nonce) pairs of the inclusive [lo, hi], ascending; the
        first is Context.scan's answer.  1 <= k <= HM_SCAN_K_MAX; the whole
        range is hashed."""
        return _scan_k(lambda m, kk, out, n: self._lib.hm_scan_k(
            self._h, m, len(m), lo, hi, kk, out, n), "hm_scan_k", msg, k)

    def scan_k_stats(self) -> dict:
        """hm_scan_k_stats_sized: work accounting of the last scan_k on this context."""
        return self._stats("hm_scan_k_stats_sized", hm_scan_k_stats)

    def find_k_many(self, requests):
        """hm_find_k_many (ABI 1.17) over [(msg, lo, hi, target, k), ...]: for
        each request what Context.find_k returns, a list of (hash, nonce); each
        request's first 2^27 nonces run as one fused launch that exits early.
        A msg of None is the empty message passed as a NULL pointer."""
        return _find_k_many(lambda arr, n, out, counts: self._lib.hm_find_k_many(
            self._h, arr, n, out, counts), "hm_find_k_many", requests)

    def find_k_many_stats(self) -> dict:
        """hm_find_k_many_stats_sized: work accounting of the last find_k_many."""
        return self._stats("hm_find_k_many_stats_sized", hm_find_k_many_stats)

    def collect(self, msg, lo: int, hi: int, target: int, cap: int):
        """hm_collect (ABI 1.11): (total, records).  total = the number of
        nonces in the inclusive [lo, hi] whose hash is below `target`, always
        exact; records = every (hash, nonce) of them, ascending by nonce, when
        total <= cap, and None when total > cap (retry with cap >= total)."""
        return _collect(lambda m, out, n, tot: self._lib.hm_collect(
            self._h, m, len(m), lo, hi, target, out, n, tot), "hm_collect", msg, cap)

    def count(self, msg, lo: int, hi: int, target: int) -> int:
        """hm_collect with no buffer: how many nonces of [lo, hi] hash below `target`."""
        return self.collect(msg, lo, hi, target, 0)[0]

    def collect_stats(self) -> dict:
        """hm_collect_stats_sized: work accounting of the last collect on this context."""
        return self._stats("hm_collect_stats_sized", hm_collect_stats)

    def collect_many(self, requests, cap: int):
        """hm_collect_many (ABI 1.15) over [(msg, lo, hi, target), ...]:
        (total, per-request totals, records).  The totals (a list of ints, what
        Context.collect returns for each request) and their sum are always
        exact; records = for each request the list of its (hash, nonce),
        ascending by nonce, when total <= cap, and None when total > cap.  A
        msg of None is the empty message passed as a NULL pointer."""
        return _collect_many(lambda arr, n, per, out, c, tot: self._lib.hm_collect_many(
            self._h, arr, n, per, out, c, tot), "hm_collect_many", requests, cap)

    def count_many(self, requests) -> list:
        """hm_collect_many with no buffer: for each request how many nonces of
        its range hash below its target."""
        return self.collect_many(requests, 0)[1]

    def collect_many_stats(self) -> dict:
        """hm_collect_many_stats_sized: work accounting of the last collect_many."""
        return self._stats("hm_collect_many_stats_sized", hm_collect_many_stats)

    def hash_many(self, msg, nonces):
        """hm_hash_many (ABI 1.12): numpy.uint64 array of Hash(msg, n) for each
        n of `nonces` (a numpy.uint64 array or a sequence of ints), any order,
        any digit counts."""
        return _hash_many(lambda m, a, n, o: self._lib.hm_hash_many(self._h, m, len(m), a, n, o),
                          "hm_hash_many", msg, nonces)

    def verify(self, msg, records, target: int, cap: int):
        """hm_verify (ABI 1.12): (bad, indices).  A record (hash, nonce) is bad
        when hash != Hash(msg, nonce) or hash >= target.  bad = their number,
        always exact; indices = numpy.uint64 array of their positions,
        ascending, when bad <= cap, and None when bad > cap.  `records` is an
        (n, 2) numpy.uint64 array or a list of (hash, nonce) pairs."""
        return _verify(lambda m, r, n, idx, c, bad: self._lib.hm_verify(
            self._h, m, len(m), r, n, target, idx, c, bad), "hm_verify", msg, records, cap)

    def verify_stats(self) -> dict:
        """hm_verify_stats_sized: accounting of the last hash_many or verify."""
        return self._stats("hm_verify_stats_sized", hm_verify_stats)

    def verify_many(self, requests, cap: int):
        """hm_verify_many (ABI 1.14) over [(msg, records, target), ...]:
        (bad, per-request counts, refs).  bad and the counts (a list of ints,
        what Context.verify returns for each request) are always exact; refs =
        the bad (request, index) pairs, ascending, as a list of tuples when
        bad <= cap, and None when bad > cap.  `records` as Context.verify's."""
        return _verify_many(lambda arr, n, per, refs, c, bad: self._lib.hm_verify_many(
            self._h, arr, n, per, refs, c, bad), "hm_verify_many", requests, cap)

    def verify_many_stats(self) -> dict:
        """hm_verify_many_stats_sized: accounting of the last verify_many."""
        return self._stats("hm_verify_many_stats_sized", hm_verify_many_stats)

    def streams_made(self, device_index: int = 0) -> int:
        """HIP streams (hardware queues) the context has made on its
        device_index-th device (debug export; ABI 1.8 makes them on first use)."""
        return int(self._lib.hm_debug_streams_made(self._h, device_index))

    def debug_no_relay(self, on: bool) -> None:
        """hm_debug_no_relay (test hook): no relay wave and no host test of the
        cancel flag, so a call that cancel() signalled runs to its end."""
        rc = self._lib.hm_debug_no_relay(self._h, int(on))
        if rc != HM_OK:
            raise HipMinerError(rc, "hm_debug_no_relay")

    def set_option(self, opt: int, value: int) -> None:
        rc = self._lib.hm_set_option(self._h, opt, value)
        if rc != HM_OK:
            raise HipMinerError(rc, "hm_set_option")

    def close(self) -> None:
        if self._h:
            self._lib.hm_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_hash(msg, nonce: int) -> int:
    """hm_hash: bitcoin.Hash on the host (hash.go:13-17)."""
    m = as_bytes(msg)
    return int(load().hm_hash(m, len(m), nonce))


def scan_cpu(msg, lo: int, hi: int, threads: int = 0) -> tuple[int, int]:
    """hm_scan_cpu (ABI 1.7): the same scan as Context.scan on the host's
    cores, for callers whose GPU is missing or failed; never
    used by Context."""
    m = as_bytes(msg)
    out = hm_result()
    rc = load().hm_scan_cpu(m, len(m), lo, hi, threads, ctypes.byref(out))
    if rc != HM_OK:
        raise HipMinerError(rc, "hm_scan_cpu")
    return int(out.hash), int(out.nonce)


def find_cpu(msg, lo: int, hi: int, target: int, threads: int = 0):
    """hm_find_cpu (ABI 1.10): Context.find's answer on the host's cores."""
    m = as_bytes(msg)
    out = hm_result()
    found = ctypes.c_int(0)
    rc = load().hm_find_cpu(m, len(m), lo, hi, target, threads, ctypes.byref(out),
                            ctypes.byref(found))
    if rc != HM_OK:
        raise HipMinerError(rc, "hm_find_cpu")
    return (int(out.hash), int(out.nonce)) if found.value else None


def _requests(cls, requests):
    """[(msg, ...), ...] as an array of the request struct cls, whose fields are
    msg, len and then the tuple's other members: (array, n, the byte strings
    the array borrows -- keep them alive for the call).  A msg of None becomes
    a NULL pointer with len 0."""
    reqs = list(requests)
    n = len(reqs)
    keep = [None if r[0] is None else as_bytes(r[0]) for r in reqs]
    arr = (cls * max(1, n))()
    for i, (r, m) in enumerate(zip(reqs, keep)):
        if len(r) + 1 != len(cls._fields_):
            raise ValueError(f"{cls.__name__}: {len(cls._fields_) - 1} values expected, got {r!r}")
        arr[i] = cls(m, len(m) if m is not None else 0, *r[1:])
    return arr, n, keep


def _find_many(call, what: str, requests):
    """Run a find_many entry point over [(msg, lo, hi, target), ...] and shape
    its answers: a list of (hash, nonce) or None."""
    arr, n, keep = _requests(hm_find_request, requests)
    outs = (hm_result * max(1, n))()
    found = (ctypes.c_int * max(1, n))()
    rc = call(arr, n, outs, found)
    del keep
    if rc != HM_OK:
        raise _error(rc, what)
    return [(int(outs[i].hash), int(outs[i].nonce)) if found[i] else None for i in range(n)]


def find_many_cpu(requests, threads: int = 0):
    """hm_find_many_cpu (ABI 1.13): Context.find_many's answers on the host's cores."""
    return _find_many(lambda arr, n, outs, found: load().hm_find_many_cpu(
        arr, n, threads, outs, found), "hm_find_many_cpu", requests)


def _find_k(call, what: str, msg, k: int):
    """Run a find_k entry point with a buffer of k records and shape its
    answer: a list of (hash, nonce)."""
    m = as_bytes(msg)
    buf = (hm_result * k)() if 0 < k <= HM_FIND_K_MAX else None
    n = ctypes.c_size_t(0)
    rc = call(m, buf, ctypes.byref(n))
    if rc != HM_OK:
        raise _error(rc, what)
    t = int(n.value)
    if t == 0:
        return []
    words = struct.unpack_from(f"={2 * t}Q", buf)
    return list(zip(words[0::2], words[1::2]))


def find_k_cpu(msg, lo: int, hi: int, target: int, k: int, threads: int = 0):
    """hm_find_k_cpu (ABI 1.16): Context.find_k's answer on the host's cores."""
    return _find_k(lambda m, out, n: load().hm_find_k_cpu(
        m, len(m), lo, hi, target, k, threads, out, n), "hm_find_k_cpu", msg, k)


def _scan_k(call, what: str, msg, k: int):
    """Run a scan_k entry point with a buffer of k records and shape its
    answer: a list of (hash, nonce).  A k the ABI refuses goes through with no
    buffer (k as 0 when it does not fit 32 bits), so the library refuses it."""
    m = as_bytes(msg)
    valid = 0 < k <= HM_SCAN_K_MAX
    buf = (hm_result * k)() if valid else None
    n = ctypes.c_size_t(0)
    rc = call(m, k if 0 <= k < 1 << 32 else 0, buf, ctypes.byref(n))
    if rc != HM_OK:
        raise _error(rc, what)
    t = int(n.value)
    if t == 0:
        return []
    words = struct.unpack_from(f"={2 * t}Q", buf)
    return list(zip(words[0::2], words[1::2]))


def scan_k_cpu(msg, lo: int, hi: int, k: int, threads: int = 0):
    """hm_scan_k_cpu (ABI 1.19): Context.scan_k's answer on the host's cores."""
    return _scan_k(lambda m, kk, out, n: load().hm_scan_k_cpu(
        m, len(m), lo, hi, kk, threads, out, n), "hm_scan_k_cpu", msg, k)


def find_k_requests(requests):
    """[(msg, lo, hi, target, k), ...] as an hm_find_k_request array (_requests)."""
    return _requests(hm_find_k_request, requests)


def _find_k_many(call, what: str, requests):
    """Run a find_k_many entry point with one buffer of sum(k) records and
    shape its answers: a list of lists of (hash, nonce)."""
    arr, n, keep = find_k_requests(requests)
    ks = [int(arr[i].k) for i in range(n)]
    valid = all(0 < k <= HM_FIND_K_MAX for k in ks)
    buf = (hm_result * max(1, sum(ks)))() if valid else (hm_result * 1)()
    counts = (ctypes.c_size_t * max(1, n))()
    rc = call(arr, n, buf, counts)
    del keep
    if rc != HM_OK:
        raise _error(rc, what)
    out, off = [], 0
    for i in range(n):
        c = int(counts[i])
        words = struct.unpack_from(f"={2 * c}Q", buf, 16 * off) if c else ()
        out.append(list(zip(words[0::2], words[1::2])))
        off += ks[i]
    return out


def find_k_many_cpu(requests, threads: int = 0):
    """hm_find_k_many_cpu (ABI 1.17): Context.find_k_many's answers on the host's cores."""
    return _find_k_many(lambda arr, n, out, counts: load().hm_find_k_many_cpu(
        arr, n, threads, out, counts), "hm_find_k_many_cpu", requests)


def _collect(call, what: str, msg, cap: int):
    """Run a collect entry point with a buffer of `cap` records (none for
    cap = 0) and shape its answer: (total, list of (hash, nonce) or None)."""
    m = as_bytes(msg)
    buf = (hm_result * cap)() if cap else None
    total = ctypes.c_uint64(0)
    rc = call(m, buf, cap, ctypes.byref(total))
    if rc != HM_OK:
        raise HipMinerError(rc, what)
    t = int(total.value)
    if t > cap:
        return t, None
    if t == 0:
        return 0, []
    words = struct.unpack_from(f"={2 * t}Q", buf)
    return t, list(zip(words[0::2], words[1::2]))


def collect_cpu(msg, lo: int, hi: int, target: int, cap: int, threads: int = 0):
    """hm_collect_cpu (ABI 1.11): Context.collect's answer on the host's cores."""
    return _collect(lambda m, out, n, tot: load().hm_collect_cpu(
        m, len(m), lo, hi, target, threads, out, n, tot), "hm_collect_cpu", msg, cap)


def count_cpu(msg, lo: int, hi: int, target: int, threads: int = 0) -> int:
    """hm_collect_cpu with no buffer: Context.count's answer on the host's cores."""
    return collect_cpu(msg, lo, hi, target, 0, threads)[0]


def collect_requests(requests):
    """[(msg, lo, hi, target), ...] as an hm_collect_request array (_requests)."""
    return _requests(hm_collect_request, requests)


def _collect_many(call, what: str, requests, cap: int):
    """Run a collect_many entry point with one buffer of `cap` records (none
    for cap = 0) and shape its answer: (total, [totals], [[(hash, nonce), ...]
    per request] or None)."""
    arr, n, keep = collect_requests(requests)
    per = (ctypes.c_uint64 * max(1, n))()
    buf = (hm_result * cap)() if cap else None
    total = ctypes.c_uint64(0)
    rc = call(arr, n, per, buf, cap, ctypes.byref(total))
    del keep
    if rc != HM_OK:
        raise HipMinerError(rc, what)
    t = int(total.value)
    totals = [int(per[i]) for i in range(n)]
    if t > cap:
        return t, totals, None
    words = struct.unpack_from(f"={2 * t}Q", buf) if t else ()
    recs, at = [], 0
    for k in totals:
        recs.append(list(zip(words[2 * at:2 * (at + k):2], words[2 * at + 1:2 * (at + k):2])))
        at += k
    return t, totals, recs


def collect_many_cpu(requests, cap: int, threads: int = 0):
    """hm_collect_many_cpu (ABI 1.15): Context.collect_many's answer on the host's cores."""
    return _collect_many(lambda arr, n, per, out, c, tot: load().hm_collect_many_cpu(
        arr, n, threads, per, out, c, tot), "hm_collect_many_cpu", requests, cap)


def _hash_many(call, what: str, msg, nonces):
    import numpy as np
    m = as_bytes(msg)
    a = np.ascontiguousarray(nonces, dtype=np.uint64).reshape(-1)
    out = np.empty(a.size, dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    rc = call(m, a.ctypes.data_as(u64p) if a.size else None, a.size,
              out.ctypes.data_as(u64p) if a.size else None)
    if rc != HM_OK:
        raise HipMinerError(rc, what)
    return out


def _verify(call, what: str, msg, records, cap: int):
    import numpy as np
    m = as_bytes(msg)
    r = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 2)
    n = r.shape[0]
    idx = np.empty(cap, dtype=np.uint64) if cap else None
    bad = ctypes.c_uint64(0)
    rc = call(m, r.ctypes.data_as(ctypes.POINTER(hm_result)) if n else None, n,
              idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if cap else None, cap,
              ctypes.byref(bad))
    if rc != HM_OK:
        raise HipMinerError(rc, what)
    b = int(bad.value)
    return (b, None) if b > cap else (b, idx[:b].copy() if cap else np.empty(0, np.uint64))


def verify_requests(requests):
    """[(msg, records, target), ...] as an hm_verify_request array: (array, n,
    the objects the array borrows from -- keep them alive for the call)."""
    import numpy as np
    reqs = list(requests)
    n = len(reqs)
    arr = (hm_verify_request * max(1, n))()
    keep = []
    for i, (msg, records, target) in enumerate(reqs):
        m = as_bytes(msg)
        r = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, 2)
        keep.append((m, r))
        arr[i] = hm_verify_request(m, len(m),
                                   r.ctypes.data_as(ctypes.POINTER(hm_result)) if r.shape[0]
                                   else None, r.shape[0], target)
    return arr, n, keep


def _verify_many(call, what: str, requests, cap: int):
    import numpy as np
    arr, n, keep = verify_requests(requests)
    per = np.zeros(max(1, n), dtype=np.uint64)
    refs = (hm_bad_ref * cap)() if cap else None
    bad = ctypes.c_uint64(0)
    rc = call(arr, n, per.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), refs, cap,
              ctypes.byref(bad))
    del keep
    if rc != HM_OK:
        raise HipMinerError(rc, what)
    b = int(bad.value)
    counts = [int(x) for x in per[:n]]
    if b > cap:
        return b, counts, None
    if b == 0:
        return 0, counts, []
    words = struct.unpack_from(f"={2 * b}Q", refs)
    return b, counts, list(zip(words[0::2], words[1::2]))


def verify_many_cpu(requests, cap: int, threads: int = 0):
    """hm_verify_many_cpu (ABI 1.14): Context.verify_many's answer on the host's cores."""
    return _verify_many(lambda arr, n, per, refs, c, bad: load().hm_verify_many_cpu(
        arr, n, threads, per, refs, c, bad), "hm_verify_many_cpu", requests, cap)


def hash_many_cpu(msg, nonces, threads: int = 0):
    """hm_hash_many_cpu (ABI 1.12): Context.hash_many's answer on the host's cores."""
    return _hash_many(lambda m, a, n, o: load().hm_hash_many_cpu(m, len(m), a, n, threads, o),
                      "hm_hash_many_cpu", msg, nonces)


def verify_cpu(msg, records, target: int, cap: int, threads: int = 0):
    """hm_verify_cpu (ABI 1.12): Context.verify's answer on the host's cores."""
    return _verify(lambda m, r, n, idx, c, bad: load().hm_verify_cpu(
        m, len(m), r, n, target, threads, idx, c, bad), "hm_verify_cpu", msg, records, cap)


def partition(msg, lo: int, hi: int, n: int) -> list:
    """hm_partition: n contiguous shards of [lo, hi] with near-equal modelled
    GPU cost for msg; each entry is (lo_i, hi_i) or None when empty.  Host-only."""
    m = as_bytes(msg)
    buf = (ctypes.c_uint64 * (2 * max(1, n)))()
    rc = load().hm_partition(m, len(m), lo, hi, n, buf)
    if rc != HM_OK:
        raise HipMinerError(rc, "hm_partition")
    out = []
    for i in range(n):
        a, b = int(buf[2 * i]), int(buf[2 * i + 1])
        out.append((a, b) if a <= b else None)
    return out


def build_id() -> str:
    """hm_build_id: digest of the sources the loaded library was built from."""
    return load().hm_build_id().decode()


def build_matches_tree() -> bool:
    """True when the loaded libhipminer.so was built from this tree's sources
    (build_id.tree_digest over csrc/ and the headers under include/)."""
    from distributed_bitcoinminer_amd import build_id as bid
    return build_id() == bid.tree_digest()


def code_object_sha16() -> str:
    """sha256 (16 hex digits) of the scan kernels' code object embedded in the
    loaded libhipminer.so (the bytes hipModuleLoadData gets)."""
    import hashlib
    p = ctypes.c_void_p()
    n = load().hm_debug_code_object(ctypes.byref(p))
    return hashlib.sha256(ctypes.string_at(p.value, n)).hexdigest()[:16]


def debug_plan(msg, lo: int, hi: int, force_generic: bool = False) -> list[dict]:
    m = as_bytes(msg)
    cap = 32
    keys = ("d", "lo", "hi", "kind", "W1", "V", "trailer", "straddle", "cost", "lane3",
            "f", "tch", "fe")
    k = len(keys)
    buf = (ctypes.c_int64 * (k * cap))()
    n = load().hm_debug_plan(m, len(m), lo, hi, int(force_generic), buf, cap)
    out = []
    for i in range(min(n, cap)):
        row = dict(zip(keys, buf[k * i: k * i + k]))
        row["lo"] &= (1 << 64) - 1
        row["hi"] &= (1 << 64) - 1
        out.append(row)
    return out

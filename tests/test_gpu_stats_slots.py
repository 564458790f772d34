"""The nine stats getters (hm_scan_stats_sized and the eight hm_X_stats_sized)
on a fresh one-device context: each answers HM_ERR_INVALID until its own
family has run and HM_OK after, whatever the other families did; it writes
the prefix it was asked for and nothing past it, and refuses a size below the
family's first layout (the HM_*_STATS_SIZE_* of include/hipminer.h).

The calls are the smallest that still launch a kernel: b"bradfitz" over
[0, 999], target 2^64 / 16, k = 2, cap = 64, two requests for the batch forms,
three records for the list forms."""
import ctypes
import re

import pytest

from distributed_bitcoinminer_amd import _lib

pytestmark = pytest.mark.gpu

MSG, LO, HI = b"bradfitz", 0, 999
TARGET = (1 << 64) // 16
K, CAP = 2, 64


def _records():
    return [(_lib.host_hash(MSG, n), n) for n in range(3)]


# getter -> (struct, the header's minimum size, the Context method over it,
#            the calls of its family: each one alone must fill the slot)
GETTERS = {
    "hm_scan_stats_sized": (
        _lib.hm_stats, "HM_STATS_SIZE_1_0", "stats",
        [lambda c: c.scan(MSG, LO, HI)]),
    "hm_find_stats_sized": (
        _lib.hm_find_stats, "HM_FIND_STATS_SIZE_1_10", "find_stats",
        [lambda c: c.find(MSG, LO, HI, TARGET)]),
    "hm_find_many_stats_sized": (
        _lib.hm_find_many_stats, "HM_FIND_MANY_STATS_SIZE_1_13", "find_many_stats",
        [lambda c: c.find_many([(MSG, LO, HI, TARGET)] * 2)]),
    "hm_find_k_stats_sized": (
        _lib.hm_find_k_stats, "HM_FIND_K_STATS_SIZE_1_16", "find_k_stats",
        [lambda c: c.find_k(MSG, LO, HI, TARGET, K)]),
    "hm_find_k_many_stats_sized": (
        _lib.hm_find_k_many_stats, "HM_FIND_K_MANY_STATS_SIZE_1_17", "find_k_many_stats",
        [lambda c: c.find_k_many([(MSG, LO, HI, TARGET, K)] * 2)]),
    "hm_collect_stats_sized": (
        _lib.hm_collect_stats, "HM_COLLECT_STATS_SIZE_1_11", "collect_stats",
        [lambda c: c.collect(MSG, LO, HI, TARGET, CAP)]),
    "hm_collect_many_stats_sized": (
        _lib.hm_collect_many_stats, "HM_COLLECT_MANY_STATS_SIZE_1_15", "collect_many_stats",
        [lambda c: c.collect_many([(MSG, LO, HI, TARGET)] * 2, CAP)]),
    # hm_hash_many and hm_verify share the verify slot
    "hm_verify_stats_sized": (
        _lib.hm_verify_stats, "HM_VERIFY_STATS_SIZE_1_12", "verify_stats",
        [lambda c: c.hash_many(MSG, [0, 1, 2]),
         lambda c: c.verify(MSG, _records(), TARGET, CAP)]),
    "hm_verify_many_stats_sized": (
        _lib.hm_verify_many_stats, "HM_VERIFY_MANY_STATS_SIZE_1_14", "verify_many_stats",
        [lambda c: c.verify_many([(MSG, _records(), TARGET)] * 2, CAP)]),
}


@pytest.fixture(scope="module")
def min_sizes():
    text = open(_lib.HEADER_PATH).read()
    sizes = {n: int(v) for n, v in re.findall(r"^#define (HM_\w*STATS_SIZE_\w+) (\d+)\b", text,
                                              re.M)}
    out = {g: sizes[macro] for g, (_, macro, _, _) in GETTERS.items()}
    assert all(0 < s <= ctypes.sizeof(GETTERS[g][0]) for g, s in out.items()), out
    return out


def _get(ctx, getter, size, fill=0xA5):
    """(rc, the 256-byte buffer the getter was handed, filled with `fill`)."""
    buf = (ctypes.c_uint8 * 256)(*([fill] * 256))
    fn = getattr(_lib.load(), getter)
    rc = fn(ctx._h, ctypes.cast(buf, ctypes.POINTER(GETTERS[getter][0])), size)
    return rc, bytes(buf)


def _filled(ctx, min_sizes):
    """The getters that answer HM_OK at their minimum size; every other one
    must answer HM_ERR_INVALID and leave the buffer alone."""
    ok = set()
    for g in GETTERS:
        rc, buf = _get(ctx, g, min_sizes[g])
        assert rc in (_lib.HM_OK, _lib.HM_ERR_INVALID), (g, rc)
        if rc == _lib.HM_OK:
            ok.add(g)
        else:
            assert buf == b"\xa5" * 256, g
    return ok


@pytest.mark.parametrize("getter", list(GETTERS))
def test_slot_fills_with_its_own_family_only(getter, min_sizes):
    cls, _, method, calls = GETTERS[getter]
    lo, full = min_sizes[getter], ctypes.sizeof(cls)
    fields = {f for f, _ in cls._fields_}
    for call in calls:
        with _lib.Context([0]) as c:
            assert _filled(c, min_sizes) == set()
            with pytest.raises(_lib.HipMinerError) as ei:
                getattr(c, method)()
            assert ei.value.rc == _lib.HM_ERR_INVALID
            call(c)
            assert _filled(c, min_sizes) == {getter}
            # the minimum size: that prefix and not a byte more
            rc, buf = _get(c, getter, lo)
            assert rc == _lib.HM_OK
            assert buf[lo:] == b"\xa5" * (256 - lo) and buf[:lo] != b"\xa5" * lo
            rc, buf0 = _get(c, getter, lo, fill=0x5A)
            assert rc == _lib.HM_OK and buf0[:lo] == buf[:lo] and buf0[lo:] == b"\x5a" * (256 - lo)
            # one byte less: refused, nothing written
            rc, small = _get(c, getter, lo - 1)
            assert rc == _lib.HM_ERR_INVALID and small == b"\xa5" * 256
            # the whole struct
            rc, buf = _get(c, getter, full)
            assert rc == _lib.HM_OK and buf[full:] == b"\xa5" * (256 - full)
            assert buf[:lo] == buf0[:lo]
            st = cls.from_buffer_copy(buf[:full])
            assert st.ndev == 1 and st.wall_ms > 0
            if "requests" in fields:
                assert st.requests == 2
            assert getattr(c, method)() == st.as_dict()
            # a larger size than the struct: the struct and not a byte more
            rc, big = _get(c, getter, 256)
            assert rc == _lib.HM_OK and big == buf


def test_find_leaves_the_scans_record_alone(min_sizes):
    with _lib.Context([0]) as c:
        c.scan(MSG, LO, HI)
        rc, before = _get(c, "hm_scan_stats_sized", ctypes.sizeof(_lib.hm_stats))
        assert rc == _lib.HM_OK
        c.find(MSG, LO, HI, TARGET)
        assert _filled(c, min_sizes) == {"hm_scan_stats_sized", "hm_find_stats_sized"}
        rc, after = _get(c, "hm_scan_stats_sized", ctypes.sizeof(_lib.hm_stats))
        assert rc == _lib.HM_OK and after == before
        assert _lib.hm_stats.from_buffer_copy(after[:168]).nonces == HI - LO + 1

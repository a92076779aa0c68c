"""The mixed-plan batched parity update in the C ABI (ezrs_update_set_create / ezrs_update_set_destroy /
ezrs_update_ptrs_mixed): exported, declared, bound, and refusing bad arguments before anything
touches a device.  No GPU needed."""
import ctypes as C
import errno
import re

import ezrs

NAMES = (("ezrs_update_set_create", 3), ("ezrs_update_set_destroy", 1), ("ezrs_update_ptrs_mixed", 10))


def test_declared_exported_and_bound():
    names = ezrs.exported_symbols()
    L = ezrs.lib()
    hdr = open(ezrs.HEADER).read()
    for name, nargs in NAMES:
        assert name in names and hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs, name
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    assert list(L.ezrs_update_set_create.argtypes) == [C.POINTER(vp), vp, u]
    assert list(L.ezrs_update_set_destroy.argtypes) == [vp]
    # set, plan_of, table, table_pitch, new_table, new_pitch, shard_len, nstripes, align, stream
    assert list(L.ezrs_update_ptrs_mixed.argtypes) == [vp, vp, vp, sz, vp, sz, sz, sz, u, vp]
    assert re.search(r"typedef\s+struct\s+ezrs_update_set\s+ezrs_update_set\s*;", hdr)


def test_abi_version_unchanged():
    assert ezrs.lib().ezrs_abi_version() == 5


def test_set_create_refuses_before_any_device():
    L = ezrs.lib()
    EINVAL = -errno.EINVAL
    arr = (C.c_void_p * 3)()                        # three NULL plans
    assert L.ezrs_update_set_create(None, arr, 3) == EINVAL         # null out
    for plans, n in ((None, 3), (arr, 0), (arr, 3), (arr, 1)):      # null plans, none, NULL entries
        h = C.c_void_p(0x1234)                      # *out is reset whatever it held
        assert L.ezrs_update_set_create(C.byref(h), plans, n) == EINVAL, (plans, n)
        assert not h.value
        assert L.ezrs_last_error().decode().startswith("update set:")


def test_null_set_calls():
    L = ezrs.lib()
    EINVAL = -errno.EINVAL
    arr, new = (C.c_void_p * 4)(), (C.c_void_p * 4)()
    po = (C.c_uint32 * 2)()
    assert L.ezrs_update_ptrs_mixed(None, po, arr, 4, new, 2, 16, 2, 1, None) == EINVAL
    # ... before the "nothing to do" of an empty call
    assert L.ezrs_update_ptrs_mixed(None, po, arr, 4, new, 2, 16, 0, 1, None) == EINVAL
    assert L.ezrs_update_ptrs_mixed(None, po, arr, 4, new, 2, 0, 2, 1, None) == EINVAL
    assert L.ezrs_update_ptrs_mixed(None, None, None, 0, None, 0, 0, 0, 0, None) == EINVAL
    assert L.ezrs_update_set_destroy(None) == 0


def test_python_set_refuses_what_is_no_plan():
    import pytest
    with pytest.raises(ezrs.EzrsError):
        ezrs.UpdateSet([])
    with pytest.raises(ezrs.EzrsError):
        ezrs.UpdateSet([None])

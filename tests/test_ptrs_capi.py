"""The pointer-array forms in the C ABI (ezrs_reconstruct_ptrs / ezrs_update_ptrs): exported,
declared, and refusing a null plan before anything touches a device.  No GPU needed."""
import ctypes as C
import errno
import re

import ezrs


def test_null_plan_is_einval():
    L = ezrs.lib()
    arr = (C.c_void_p * 4)()
    assert L.ezrs_reconstruct_ptrs(None, arr, 16, None, None) == -errno.EINVAL
    assert L.ezrs_update_ptrs(None, arr, arr, 16, None) == -errno.EINVAL
    assert L.ezrs_reconstruct_ptrs(None, None, 0, None, None) == -errno.EINVAL
    assert L.ezrs_update_ptrs(None, None, None, 0, None) == -errno.EINVAL


def test_abi_version_unchanged():
    assert ezrs.lib().ezrs_abi_version() == 5


def test_declared_and_bound():
    names = ezrs.exported_symbols()
    assert "ezrs_reconstruct_ptrs" in names and "ezrs_update_ptrs" in names
    L = ezrs.lib()
    assert L.ezrs_reconstruct_ptrs.argtypes is not None and len(L.ezrs_reconstruct_ptrs.argtypes) == 5
    assert L.ezrs_update_ptrs.argtypes is not None and len(L.ezrs_update_ptrs.argtypes) == 5
    m = re.search(r"#define\s+EZRS_PTRS_MAX\s+(\d+)", open(ezrs.HEADER).read())
    assert m and int(m.group(1)) == 320

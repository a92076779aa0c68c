"""The batched pointer-table forms in the C ABI (ezrs_reconstruct_ptrs_batch /
ezrs_update_ptrs_batch): exported, declared, bound, and refusing a null plan before anything touches
a device.  No GPU needed."""
import ctypes as C
import errno
import re

import ezrs


def test_null_plan_is_einval():
    L = ezrs.lib()
    arr = (C.c_void_p * 4)()
    assert L.ezrs_reconstruct_ptrs_batch(None, arr, 4, 16, 2, 1, None, None) == -errno.EINVAL
    assert L.ezrs_update_ptrs_batch(None, arr, 4, arr, 1, 16, 2, 1, None) == -errno.EINVAL
    # ... before the "nothing to do" of an empty call
    assert L.ezrs_reconstruct_ptrs_batch(None, arr, 4, 16, 0, 1, None, None) == -errno.EINVAL
    assert L.ezrs_update_ptrs_batch(None, arr, 4, arr, 1, 16, 0, 1, None) == -errno.EINVAL
    assert L.ezrs_reconstruct_ptrs_batch(None, None, 0, 0, 0, 0, None, None) == -errno.EINVAL
    assert L.ezrs_update_ptrs_batch(None, None, 0, None, 0, 0, 0, 0, None) == -errno.EINVAL


def test_abi_version_unchanged():
    assert ezrs.lib().ezrs_abi_version() == 5


def test_declared_and_bound():
    names = ezrs.exported_symbols()
    assert "ezrs_reconstruct_ptrs_batch" in names and "ezrs_update_ptrs_batch" in names
    L = ezrs.lib()
    assert L.ezrs_reconstruct_ptrs_batch.argtypes is not None and len(L.ezrs_reconstruct_ptrs_batch.argtypes) == 8
    # plan, table, table_pitch, new_table, new_pitch, shard_len, nstripes, align, stream
    assert L.ezrs_update_ptrs_batch.argtypes is not None and len(L.ezrs_update_ptrs_batch.argtypes) == 9
    hdr = open(ezrs.HEADER).read()
    for name, nargs in (("ezrs_reconstruct_ptrs_batch", 8), ("ezrs_update_ptrs_batch", 9)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name

"""The pointer forms of the staged decode in the C ABI (ezrs_decode_ptrs, ezrs_decode_ptrs_batch,
their _ws forms and ezrs_decode_ptrs_workspace_bytes): exported, declared, bound, and refusing a null
codec before anything touches a device.  No GPU needed."""
import ctypes as C
import errno
import re

import ezrs

# name -> (return type in the header, arguments)
SYMBOLS = {
    "ezrs_decode_ptrs_workspace_bytes": ("size_t", 4),
    "ezrs_decode_ptrs": ("int", 13),
    "ezrs_decode_ptrs_ws": ("int", 15),
    "ezrs_decode_ptrs_batch": ("int", 16),
    "ezrs_decode_ptrs_batch_ws": ("int", 18),
}


def test_null_codec_is_einval():
    L = ezrs.lib()
    EINVAL = -errno.EINVAL
    arr = (C.c_void_p * 16)()
    res = (C.c_int32 * 64)()
    out = (None, 0, None, res, None, 0, None, 0)          # eras .. corr_stride
    for shard_len in (16, 0):
        assert L.ezrs_decode_ptrs(None, arr, 10, shard_len, *out, None) == EINVAL
        assert L.ezrs_decode_ptrs_ws(None, arr, 10, shard_len, *out, None, 0, None) == EINVAL
    for nstripes, shard_len in ((2, 16), (0, 16), (2, 0), (0, 0)):
        assert L.ezrs_decode_ptrs_batch(None, arr, 16, 10, shard_len, nstripes, 1, *out, None) == EINVAL
        assert L.ezrs_decode_ptrs_batch_ws(None, arr, 16, 10, shard_len, nstripes, 1, *out, None, 0,
                                           None) == EINVAL
    assert L.ezrs_decode_ptrs(None, None, 0, 0, None, 0, None, None, None, 0, None, 0, None) == EINVAL
    assert L.ezrs_decode_ptrs_batch(None, None, 0, 0, 0, 0, 0, None, 0, None, None, None, 0, None, 0,
                                    None) == EINVAL
    assert list(res) == [0] * 64


def test_workspace_bytes_of_null_codec():
    assert ezrs.lib().ezrs_decode_ptrs_workspace_bytes(None, 10, 4096, 3) == 0


def test_abi_version_unchanged():
    assert ezrs.lib().ezrs_abi_version() == 5


def test_declared_and_bound():
    names = ezrs.exported_symbols()
    L = ezrs.lib()
    hdr = open(ezrs.HEADER).read()
    for name, (ret, nargs) in SYMBOLS.items():
        assert name in names, name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == nargs, name
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert L.ezrs_decode_ptrs_workspace_bytes.restype is C.c_size_t
    for meth in ("decode_ptrs", "decode_ptrs_batch", "decode_ptrs_workspace_bytes"):
        assert callable(getattr(ezrs.Codec, meth))

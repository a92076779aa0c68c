"""CPU tests of the selection calls' boundary (ezrs_select_failed, ezrs_decode_ptrs_select,
ezrs_decode_interleaved_select and their _ws and workspace forms): exported, declared, bound with
the right argument counts, and a null codec rejected before any device is touched."""
import errno
import re
import subprocess

import ezrs

# name -> number of arguments in include/ezrs.h
CALLS = {
    "ezrs_select_workspace_bytes": 1,
    "ezrs_select_failed": 8,
    "ezrs_select_failed_ws": 10,
    "ezrs_decode_select_workspace_bytes": 3,
    "ezrs_decode_ptrs_select": 18,
    "ezrs_decode_ptrs_select_ws": 20,
    "ezrs_decode_interleaved_select": 19,
    "ezrs_decode_interleaved_select_ws": 21,
}


def test_symbols_exported_declared_and_bound():
    """The eight functions and the EZRS_SEL_NONE macro: the nine names of the selection surface."""
    L = ezrs.lib()
    declared = set(ezrs.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", ezrs.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(ezrs.HEADER).read()
    for name, nargs in CALLS.items():
        assert name in declared, name
        assert name in exported, name
        assert len(getattr(L, name).argtypes) == nargs, name
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
    assert re.search(r"^#define EZRS_SEL_NONE UINT64_MAX\b", hdr, re.M)
    assert ezrs.SEL_NONE == -1 and ezrs.SEL_NONE & (2 ** 64 - 1) == 2 ** 64 - 1


def test_null_codec_is_einval_before_any_device():
    L = ezrs.lib()
    EINVAL = -errno.EINVAL
    assert L.ezrs_select_failed(None, None, 0, 0, None, 0, None, None) == EINVAL
    assert L.ezrs_select_failed_ws(None, None, 0, 0, None, 0, None, None, 0, None) == EINVAL
    out = (None, 0, None, None, None, 0, None, 0)              # eras .. corr_stride
    assert L.ezrs_decode_ptrs_select(None, None, 0, 1, 1, 1, None, 1, None, *out, None) == EINVAL
    assert L.ezrs_decode_ptrs_select(None, None, 0, 1, 1, 1, None, 0, None, *out, None) == EINVAL
    assert L.ezrs_decode_ptrs_select_ws(None, None, 0, 1, 1, 1, None, 1, None, *out, None, 0, None) == EINVAL
    assert L.ezrs_decode_interleaved_select(None, None, 0, 1, 1, 1, 1, None, 1, None, *out, None) == EINVAL
    assert L.ezrs_decode_interleaved_select(None, None, 0, 1, 1, 1, 1, None, 0, None, *out, None) == EINVAL
    assert L.ezrs_decode_interleaved_select_ws(None, None, 0, 1, 1, 1, 1, None, 1, None, *out, None, 0,
                                               None) == EINVAL


def test_workspace_figures():
    """A null codec's decode workspace is 0; the selection's depends on n alone: 8 bytes per chunk
    of 4096 results."""
    L = ezrs.lib()
    assert L.ezrs_decode_select_workspace_bytes(None, 10, 1000) == 0
    assert L.ezrs_select_workspace_bytes(0) == 0
    assert L.ezrs_select_workspace_bytes(1) == L.ezrs_select_workspace_bytes(4096) == 8
    assert L.ezrs_select_workspace_bytes(4097) == 16


def test_abi_version_unchanged():
    assert ezrs.lib().ezrs_abi_version() == 5

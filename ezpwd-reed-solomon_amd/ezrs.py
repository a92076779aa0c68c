"""Python host mirror of the MI355X RS engine (ctypes over lib/libezrs_hip.so, include/ezrs.h).

Mirrors the reference's RS codec surface for the batch hot path:

* ``Codec.rs(n, k)``          -- ezpwd::RS<N,K>                  (c++/ezpwd/rs:74-89)
* ``Codec.ccsds(k, dual)``    -- ezpwd::RS_CCSDS[_CONV]<255,K>   (c++/ezpwd/rs:101-104)
* ``Codec.encode(...)``       -- encode<TYP>(data, len, parity)  (c++/ezpwd/rs_base:868-904) per row
* ``Codec.decode(...)``       -- decode<TYP>(data, len, parity, eras_pos, no_eras, corr)
                                                                 (c++/ezpwd/rs_base:1170-1242) per row

Device forms take torch tensors on the codec's device (PyTorch is only the allocator/stream
provider here); host forms take numpy arrays and go through the library's pinned, double-buffered
copy pipeline.  There is no CPU fallback: if the HIP library is missing or no GPU is visible,
constructing a codec raises.
"""
from __future__ import annotations

import ctypes as C
import errno
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libezrs_hip.so")
# timing experiments only: a variant build of the same library (tools/build_variant.sh)
LIB_PATH = os.environ.get("EZRS_LIB_VARIANT") or LIB_PATH
HEADER = os.path.join(os.path.dirname(HERE), "include", "ezrs.h")
BCH_HEADER = os.path.join(os.path.dirname(HERE), "include", "ezbch.h")

_vp, _sz, _u, _i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int


class EzrsError(RuntimeError):
    pass


class Info(C.Structure):
    _fields_ = [("symbol_bits", _u), ("size", _u), ("nroots", _u), ("load", _u), ("poly", _u),
                ("fcr", _u), ("prim", _u), ("datum_bytes", _u), ("dual", _i), ("device", _i)]


class BCHInfo(C.Structure):
    _fields_ = [("m", _u), ("n", _u), ("t", _u), ("ecc_bits", _u), ("ecc_bytes", _u),
                ("prim_poly", _u), ("device", _i)]


_lib = None


def lib():
    """Load libezrs_hip.so; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EzrsError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                            "(make -C ezpwd-reed-solomon_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        L.ezrs_abi_version.restype = _i
        L.ezrs_device_count.restype = _i
        L.ezrs_last_error.restype = C.c_char_p
        L.ezrs_create.argtypes = [C.POINTER(_vp), _u, _u, _u, _u, _u, _i, _i]
        L.ezrs_create_rs.argtypes = [C.POINTER(_vp), _u, _u, _i]
        L.ezrs_create_ccsds.argtypes = [C.POINTER(_vp), _u, _i, _i]
        L.ezrs_destroy.argtypes = [_vp]
        L.ezrs_get_info.argtypes = [_vp, C.POINTER(Info)]
        L.ezrs_reserve.argtypes = [_vp, _sz]
        L.ezrs_reserve_stream.argtypes = [_vp, _sz, _vp]
        L.ezrs_workspace_bytes.argtypes = [_vp, _sz]
        L.ezrs_workspace_bytes.restype = _sz
        L.ezrs_encode.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _sz, _vp]
        L.ezrs_encode_rows.argtypes = [_vp, _vp, _sz, _u, _sz, _vp]
        L.ezrs_encode_ws.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _sz, _vp, _sz, _vp]
        L.ezrs_encode_rows_ws.argtypes = [_vp, _vp, _sz, _u, _sz, _vp, _sz, _vp]
        L.ezrs_decode.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz,
                                  _vp, _sz, _sz, _vp]
        L.ezrs_decode_ws.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _sz,
                                     _vp, _sz, _sz, _vp, _sz, _vp]
        L.ezrs_encode_host.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _sz, _sz]
        L.ezrs_encode_rows_host.argtypes = [_vp, _vp, _sz, _u, _sz, _sz]
        L.ezrs_decode_host.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _vp, _sz, _vp, _vp, _vp,
                                       _sz, _vp, _sz, _sz, _sz]
        L.ezrs_stream_encoded_bound.argtypes = [_vp, _sz, _u]
        L.ezrs_stream_encoded_bound.restype = _sz
        L.ezrs_stream_encode.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, C.POINTER(_sz)]
        L.ezrs_stream_decode.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, C.POINTER(_sz),
                                         C.POINTER(_sz)]
        L.ezrs_shard_codewords.restype = _sz
        L.ezrs_shard_codewords.argtypes = [_vp, _sz, _u]
        L.ezrs_shard_encoded_len.restype = _sz
        L.ezrs_shard_encoded_len.argtypes = [_vp, _sz, _u]
        L.ezrs_encode_shards.argtypes = [_vp, _vp, _sz, _sz, _u, _sz, _vp]
        L.ezrs_decode_shards.argtypes = [_vp, _vp, _sz, _sz, _u, _sz, _vp, _sz, _vp, _vp, _vp, _sz,
                                         _vp, _sz, _vp]
        L.ezrs_interleaved_workspace_bytes.restype = _sz
        L.ezrs_interleaved_workspace_bytes.argtypes = [_vp, _u, _sz, _sz]
        L.ezrs_encode_interleaved.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _sz, _vp]
        L.ezrs_encode_interleaved_ws.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _sz, _vp, _sz, _vp]
        L.ezrs_decode_interleaved.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _sz, _vp, _sz, _vp, _vp,
                                              _vp, _sz, _vp, _sz, _vp]
        L.ezrs_decode_interleaved_ws.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _sz, _vp, _sz, _vp,
                                                 _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]
        L.ezrs_recon_create.argtypes = [C.POINTER(_vp), _vp, _u, _vp, _u]
        L.ezrs_recon_destroy.argtypes = [_vp]
        L.ezrs_reconstruct_interleaved.argtypes = [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]
        L.ezrs_recon_bitmatrix.argtypes = [_u, _u, _u, _u, _u, _i, _u, _vp, _u, _vp, _sz, _vp]
        L.ezrs_update_create.argtypes = [C.POINTER(_vp), _vp, _u, _vp, _u]
        L.ezrs_update_destroy.argtypes = [_vp]
        L.ezrs_update_interleaved.argtypes = [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _sz, _vp]
        L.ezrs_update_bitmatrix.argtypes = [_u, _u, _u, _u, _u, _i, _u, _vp, _u, _vp, _sz]
        L.ezrs_reconstruct_ptrs.argtypes = [_vp, _vp, _sz, _vp, _vp]
        L.ezrs_update_ptrs.argtypes = [_vp, _vp, _vp, _sz, _vp]
        L.ezrs_reconstruct_ptrs_batch.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _vp, _vp]
        L.ezrs_update_ptrs_batch.argtypes = [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _u, _vp]
        L.ezrs_recon_set_create.argtypes = [C.POINTER(_vp), _vp, _u]
        L.ezrs_recon_set_destroy.argtypes = [_vp]
        L.ezrs_reconstruct_ptrs_mixed.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, _u, _vp, _vp]
        L.ezrs_update_set_create.argtypes = [C.POINTER(_vp), _vp, _u]
        L.ezrs_update_set_destroy.argtypes = [_vp]
        L.ezrs_update_ptrs_mixed.argtypes = [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _u, _vp]
        L.ezrs_decode_ptrs_workspace_bytes.restype = _sz
        L.ezrs_decode_ptrs_workspace_bytes.argtypes = [_vp, _u, _sz, _sz]
        L.ezrs_decode_ptrs.argtypes = [_vp, _vp, _u, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp]
        L.ezrs_decode_ptrs_ws.argtypes = [_vp, _vp, _u, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz,
                                          _vp, _sz, _vp]
        L.ezrs_decode_ptrs_batch.argtypes = [_vp, _vp, _sz, _u, _sz, _sz, _u, _vp, _sz, _vp, _vp, _vp,
                                             _sz, _vp, _sz, _vp]
        L.ezrs_decode_ptrs_batch_ws.argtypes = [_vp, _vp, _sz, _u, _sz, _sz, _u, _vp, _sz, _vp, _vp,
                                                _vp, _sz, _vp, _sz, _vp, _sz, _vp]
        L.ezrs_select_workspace_bytes.restype = _sz
        L.ezrs_select_workspace_bytes.argtypes = [_sz]
        L.ezrs_select_failed.argtypes = [_vp, _vp, _sz, C.c_uint64, _vp, _sz, _vp, _vp]
        L.ezrs_select_failed_ws.argtypes = [_vp, _vp, _sz, C.c_uint64, _vp, _sz, _vp, _vp, _sz, _vp]
        L.ezrs_decode_select_workspace_bytes.restype = _sz
        L.ezrs_decode_select_workspace_bytes.argtypes = [_vp, _u, _sz]
        L.ezrs_decode_ptrs_select.argtypes = [_vp, _vp, _sz, _u, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp,
                                              _vp, _vp, _sz, _vp, _sz, _vp]
        L.ezrs_decode_ptrs_select_ws.argtypes = [_vp, _vp, _sz, _u, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp,
                                                 _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]
        L.ezrs_decode_interleaved_select.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _sz, _vp, _sz, _vp, _vp,
                                                     _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp]
        L.ezrs_decode_interleaved_select_ws.argtypes = [_vp, _vp, _sz, _sz, _sz, _u, _sz, _vp, _sz, _vp,
                                                        _vp, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz,
                                                        _vp]
        L.ezrs_kernel_path.argtypes = [_vp]
        L.ezrs_set_launch_rows.argtypes = [_vp, _sz]
        L.ezrs_set_semantics.argtypes = [_vp, _i]
        L.ezrs_get_semantics.argtypes = [_vp]
        L.ezrs_host_alloc.argtypes = [C.POINTER(_vp), _sz]
        L.ezrs_host_free.argtypes = [_vp]
        L.ezbch_last_error.restype = C.c_char_p
        L.ezbch_create.argtypes = [C.POINTER(_vp), _u, _u, _u, _i]
        L.ezbch_create_nkt.argtypes = [C.POINTER(_vp), _u, _u, _u, _i]
        L.ezbch_destroy.argtypes = [_vp]
        L.ezbch_get_info.argtypes = [_vp, C.POINTER(BCHInfo)]
        L.ezbch_encode.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _sz, _vp]
        L.ezbch_encode_rows.argtypes = [_vp, _vp, _sz, _u, _sz, _vp]
        L.ezbch_encode_rows_host.argtypes = [_vp, _vp, _sz, _u, _sz, _sz]
        L.ezbch_decode.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _vp, _vp, _sz, _sz, _vp]
        L.ezbch_decode_ecc.argtypes = [_vp, _vp, _sz, _u, _vp, _vp, _sz, _sz, _vp]
        L.ezbch_decode_syn.argtypes = [_vp, _vp, _sz, _u, _vp, _vp, _sz, _sz, _vp]
        L.ezbch_encode_host.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _sz, _sz]
        L.ezbch_decode_host.argtypes = [_vp, _vp, _sz, _u, _vp, _sz, _vp, _vp, _sz, _sz, _sz]
        L.ezbch_decode_syn_host.argtypes = [_vp, _vp, _sz, _u, _vp, _vp, _sz, _sz]
        _lib = L
    return _lib


def _check(rc, what, bch=False):
    if rc < 0:
        msg = (lib().ezbch_last_error() if bch else lib().ezrs_last_error()).decode(errors="replace")
        raise EzrsError(f"{what} failed: {errno.errorcode.get(-rc, rc)} {msg}")
    return rc


def _tp(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _np(a):
    return None if a is None else a.ctypes.data_as(_vp)


_ITEM = {"uint8": 1, "int8": 1, "uint16": 2, "int16": 2, "uint32": 4, "int32": 4}


def _dev_rows(t, what, device, itemsize, ndim=2):
    """Validate a device tensor argument: on the codec's device, rows of contiguous elements of the
    expected width; returns its row stride in elements (0 for None)."""
    if t is None:
        return 0
    _dev_elems(t, what, device, itemsize)
    if t.dim() != ndim or (ndim == 2 and t.shape[1] > 1 and t.stride(1) != 1):
        raise EzrsError(f"{what}: expected a {ndim}-D tensor with contiguous rows")
    return t.stride(0) if ndim == 2 else 1


def _dev_elems(t, what, device, itemsize):
    """A tensor on the codec's device with elements of the expected width, whatever its shape."""
    if not getattr(t, "is_cuda", False):
        raise EzrsError(f"{what}: expected a GPU tensor")
    if t.device.index != device:
        raise EzrsError(f"{what}: tensor on cuda:{t.device.index}, codec on cuda:{device}")
    if t.element_size() != itemsize:
        raise EzrsError(f"{what}: expected {itemsize}-byte elements, got {t.dtype}")


def _host_rows(a, what, itemsize, ndim=2):
    """Validate a numpy argument of the host forms; returns its row stride in elements."""
    if a is None:
        return 0
    if not isinstance(a, np.ndarray):
        raise EzrsError(f"{what}: expected a numpy array")
    if a.itemsize != itemsize:
        raise EzrsError(f"{what}: expected {itemsize}-byte elements, got {a.dtype}")
    if a.ndim != ndim or (ndim == 2 and a.shape[1] > 1 and a.strides[1] != itemsize) or \
            (ndim == 2 and a.strides[0] % itemsize):
        raise EzrsError(f"{what}: expected a {ndim}-D array with contiguous rows")
    if ndim == 1 and a.strides[0] != itemsize:
        raise EzrsError(f"{what}: expected a contiguous array")
    if ndim == 2 and a.strides[0] < 0:
        raise EzrsError(f"{what}: rows in reverse order (negative row stride) are not supported")
    return a.strides[0] // itemsize if ndim == 2 else 1


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream) if hasattr(stream, "cuda_stream") else C.c_void_p(stream)


def _shard_ptrs(seq, what, n, optional, device, w, shard_len=None):
    """Validate a sequence of n 1-D contiguous device tensors of one length (None allowed at the
    indices in `optional`); returns (host array of their device pointers, that length)."""
    seq = list(seq)
    if len(seq) != n:
        raise EzrsError(f"{what}: {len(seq)} entries, expected {n}")
    arr = (C.c_void_p * max(n, 1))()
    for i, t in enumerate(seq):
        if t is None:
            if i not in optional:
                raise EzrsError(f"{what}[{i}]: None where the call needs a buffer")
            continue
        if not getattr(t, "is_cuda", False):
            raise EzrsError(f"{what}[{i}]: expected a GPU tensor")
        if t.device.index != device:
            raise EzrsError(f"{what}[{i}]: tensor on cuda:{t.device.index}, expected cuda:{device}")
        if t.element_size() != w:
            raise EzrsError(f"{what}[{i}]: expected {w}-byte elements, got {t.dtype}")
        if t.dim() != 1 or (t.shape[0] > 1 and t.stride(0) != 1):
            raise EzrsError(f"{what}[{i}]: expected a 1-D contiguous tensor")
        if shard_len is None:
            shard_len = t.shape[0]
        elif t.shape[0] != shard_len:
            raise EzrsError(f"{what}[{i}]: {t.shape[0]} symbols, the other shards have {shard_len}")
        arr[i] = t.data_ptr()
    return arr, (0 if shard_len is None else shard_len)


def _ptr_table(t, what, need, device):
    """Validate an int64 device tensor [nstripes, pitch >= need] with a contiguous last dimension;
    returns (nstripes, pitch in entries)."""
    import torch
    if not getattr(t, "is_cuda", False):
        raise EzrsError(f"{what}: expected a GPU tensor")
    if t.device.index != device:
        raise EzrsError(f"{what}: tensor on cuda:{t.device.index}, expected cuda:{device}")
    if t.dtype != torch.int64:
        raise EzrsError(f"{what}: expected int64 entries (device pointers), got {t.dtype}")
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise EzrsError(f"{what}: expected a 2-D tensor [nstripes, pitch] with a contiguous last dimension")
    if t.shape[1] < need:
        raise EzrsError(f"{what}: {t.shape[1]} entries per stripe, the call needs {need}")
    pitch = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if pitch < need:
        raise EzrsError(f"{what}: a stripe stride of {pitch} entries, the call needs {need}")
    return t.shape[0], pitch


def _align(align, w):
    align = w if align is None else int(align)
    if align not in (16, 4, w):
        raise EzrsError(f"align: {align}, expected 16, 4 or the datum size {w}")
    return align


class Codec:
    """An RS(N,K) codec resident on one HIP device."""

    def __init__(self, symbol_bits, poly, fcr, prim, nroots, dual=False, device=0, _h=None):
        h = _vp()
        if _h is None:
            _check(lib().ezrs_create(C.byref(h), symbol_bits, poly, fcr, prim, nroots,
                                     int(bool(dual)), device), "ezrs_create")
        else:
            h = _h
        self._h = h
        info = Info()
        _check(lib().ezrs_get_info(self._h, C.byref(info)), "ezrs_get_info")
        self.info = info
        self.symbol_bits, self.nn, self.nroots, self.load = (info.symbol_bits, info.size,
                                                             info.nroots, info.load)
        self.dual, self.device = bool(info.dual), info.device
        self.dtype = np.uint8 if info.datum_bytes == 1 else np.uint16

    @classmethod
    def rs(cls, n, k, device=0):
        h = _vp()
        _check(lib().ezrs_create_rs(C.byref(h), n, k, device), f"ezrs_create_rs({n},{k})")
        return cls(0, 0, 0, 0, 0, _h=h)

    @classmethod
    def ccsds(cls, k, dual=True, device=0):
        h = _vp()
        _check(lib().ezrs_create_ccsds(C.byref(h), k, int(bool(dual)), device), "ezrs_create_ccsds")
        return cls(0, 0, 0, 0, 0, _h=h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().ezrs_destroy(h)
            except Exception:
                pass
            self._h = None

    def __repr__(self):
        i = self.info
        kind = ("RS_CCSDS" if i.dual else "RS_CCSDS_CONV") if i.poly == 0x187 else "RS"
        return f"{kind}({i.size},{i.load})"

    @property
    def torch_dtype(self):
        import torch
        return torch.uint8 if self.dtype == np.uint8 else torch.uint16

    @property
    def kernel_path(self):
        """'generic' | 'bitslice' | 'planeslice' | 'wide' (ezrs_kernel_path)."""
        return ("generic", "bitslice", "planeslice", "wide")[_check(lib().ezrs_kernel_path(self._h),
                                                                      "ezrs_kernel_path")]

    @property
    def semantics(self):
        """'ezpwd' (decode_symbols, the default) or 'karn' (libfec decode_rs_*: full-NN-frame
        erasures and positions, none of ezpwd's extra failure checks) -- ezrs_set_semantics."""
        return ("ezpwd", "karn")[_check(lib().ezrs_get_semantics(self._h), "ezrs_get_semantics")]

    @semantics.setter
    def semantics(self, mode):
        _check(lib().ezrs_set_semantics(self._h, {"ezpwd": 0, "karn": 1}[mode]), "ezrs_set_semantics")

    def set_launch_rows(self, rows):
        """Test hook (ezrs_set_launch_rows): cap the codewords one plane-sliced launch of this codec
        takes; 0 = the default.  Results never depend on it."""
        _check(lib().ezrs_set_launch_rows(self._h, int(rows)), "ezrs_set_launch_rows")

    def reserve(self, ncw, stream=None):
        """Pre-size the workspace of `stream` (default: the current torch stream)."""
        _check(lib().ezrs_reserve_stream(self._h, ncw, _stream_ptr(stream)), "ezrs_reserve_stream")

    def workspace_bytes(self, ncw):
        return int(lib().ezrs_workspace_bytes(self._h, ncw))

    def _decode_out(self, ncw, eras, neras, result, positions, corr, like=None):
        """The decode outputs of ncw codewords, validated: device tensors on the device of the
        tensor `like`, or (like is None: the host forms) numpy arrays.  Allocates `result` when it
        is None.  Returns result and the eight arguments eras .. corr_stride of the C call."""
        w = self.info.datum_bytes
        if like is None:
            rows, ptr = _host_rows, _np
            if result is None:
                result = np.zeros(ncw, np.int32)
        else:
            def rows(t, what, itemsize, ndim=2):
                return _dev_rows(t, what, self.device, itemsize, ndim)
            ptr = _tp
        es = rows(eras, "eras", 4)
        rows(neras, "neras", 4, ndim=1)
        qs = rows(positions, "positions", 4)
        cs = rows(corr, "corr", w)
        if result is None:
            import torch
            result = torch.empty(ncw, dtype=torch.int32, device=like.device)
        rows(result, "result", 4, ndim=1)
        return result, (ptr(eras), es, ptr(neras), ptr(result), ptr(positions), qs, ptr(corr), cs)

    # -- device batch forms ------------------------------------------------------------------
    def encode(self, data, length=None, parity=None, stream=None):
        """data: [ncw, stride] device tensor; parity: [ncw, >=nroots] tensor, or None: each row
        carries its parity in columns length..length+nroots (ezrs_encode_rows)."""
        w = self.info.datum_bytes
        ncw = data.shape[0]
        ds = _dev_rows(data, "data", self.device, w)
        ps = _dev_rows(parity, "parity", self.device, w)
        length = data.shape[1] - self.nroots if length is None else length
        if parity is None:
            _check(lib().ezrs_encode_rows(self._h, _tp(data), ds, length, ncw, _stream_ptr(stream)),
                   "ezrs_encode_rows")
        else:
            _check(lib().ezrs_encode(self._h, _tp(data), ds, length, _tp(parity), ps, ncw,
                                     _stream_ptr(stream)), "ezrs_encode")

    def decode(self, data, length=None, parity=None, eras=None, neras=None, result=None,
               positions=None, corr=None, stream=None):
        """In-place batch decode; returns the int32 result tensor."""
        w = self.info.datum_bytes
        ncw = data.shape[0]
        ds = _dev_rows(data, "data", self.device, w)
        ps = _dev_rows(parity, "parity", self.device, w)
        result, out = self._decode_out(ncw, eras, neras, result, positions, corr, like=data)
        length = data.shape[1] - self.nroots if length is None else length
        _check(lib().ezrs_decode(self._h, _tp(data), ds, length, _tp(parity), ps, *out, ncw,
                                 _stream_ptr(stream)), "ezrs_decode")
        return result

    # -- shard batches (rsencode layout per shard) --------------------------------------------
    def shard_codewords(self, shard_len, chunk=None):
        """Codewords per shard of shard_len data symbols cut into chunks (default: the load)."""
        return int(lib().ezrs_shard_codewords(self._h, shard_len, chunk or self.load))

    def shard_encoded_len(self, shard_len, chunk=None):
        return int(lib().ezrs_shard_encoded_len(self._h, shard_len, chunk or self.load))

    def encode_shards(self, shards, shard_len, chunk=None, stream=None):
        """shards: [nshards, pitch] device tensor, each row one shard in the rsencode layout
        (chunks of `chunk` data symbols, each followed by its parity; the last chunk shorter);
        writes every codeword's parity (ezrs_encode_shards)."""
        w = self.info.datum_bytes
        sp = _dev_rows(shards, "shards", self.device, w)
        _check(lib().ezrs_encode_shards(self._h, _tp(shards), sp, shard_len, chunk or self.load,
                                        shards.shape[0], _stream_ptr(stream)), "ezrs_encode_shards")

    def decode_shards(self, shards, shard_len, chunk=None, eras=None, neras=None, result=None,
                      positions=None, corr=None, stream=None):
        """In-place decode of every codeword of every shard; returns the int32 result tensor
        [nshards * codewords per shard] (shard-major)."""
        chunk = chunk or self.load
        sp = _dev_rows(shards, "shards", self.device, self.info.datum_bytes)
        ncw = shards.shape[0] * self.shard_codewords(shard_len, chunk)
        result, out = self._decode_out(ncw, eras, neras, result, positions, corr, like=shards)
        _check(lib().ezrs_decode_shards(self._h, _tp(shards), sp, shard_len, chunk, shards.shape[0], *out,
                                        _stream_ptr(stream)), "ezrs_decode_shards")
        return result

    # -- interleaved frames (CCSDS depth I, striped shards) ------------------------------------
    def _frames(self, frames):
        """Validate a [nframes, len + nroots, depth] device tensor with a contiguous last
        dimension; returns (frame_pitch, sym_stride, depth, len, nframes)."""
        _dev_elems(frames, "frames", self.device, self.info.datum_bytes)
        if frames.dim() != 3 or (frames.shape[2] > 1 and frames.stride(2) != 1):
            raise EzrsError("frames: expected a 3-D tensor [nframes, len + nroots, depth] with a "
                            "contiguous last dimension")
        nframes, nsym, depth = frames.shape
        if nsym <= self.nroots or nsym > self.nn or depth == 0:
            raise EzrsError(f"frames: {nsym} symbols per codeword, expected {self.nroots + 1}.."
                            f"{self.nn}, and a depth of at least 1")
        return frames.stride(0), frames.stride(1), depth, nsym - self.nroots, nframes

    def interleaved_workspace_bytes(self, length, depth, nframes):
        return int(lib().ezrs_interleaved_workspace_bytes(self._h, length, depth, nframes))

    def encode_interleaved(self, frames, stream=None):
        """frames: [nframes, len + nroots, depth] device tensor (a CCSDS buffer: buf.view(F, 255, I);
        a stripe of N shards: shards[None] of a [N, pitch] tensor sliced to [:, :shard_len]); writes
        the nroots parity symbols of every codeword (ezrs_encode_interleaved)."""
        fp, ss, depth, length, nframes = self._frames(frames)
        _check(lib().ezrs_encode_interleaved(self._h, _tp(frames), fp, ss, depth, length, nframes,
                                             _stream_ptr(stream)), "ezrs_encode_interleaved")

    def decode_interleaved(self, frames, eras=None, neras=None, result=None, positions=None,
                           corr=None, stream=None):
        """In-place decode of every codeword of every frame; returns the int32 result tensor
        [nframes * depth] (frame-major, k = f * depth + j) -- ezrs_decode_interleaved."""
        fp, ss, depth, length, nframes = self._frames(frames)
        result, out = self._decode_out(nframes * depth, eras, neras, result, positions, corr, like=frames)
        _check(lib().ezrs_decode_interleaved(self._h, _tp(frames), fp, ss, depth, length, nframes, *out,
                                             _stream_ptr(stream)), "ezrs_decode_interleaved")
        return result

    # -- pointer forms of the staged decode: every shard a buffer of its own ---------------------
    def decode_ptrs_workspace_bytes(self, length, shard_len, nstripes):
        return int(lib().ezrs_decode_ptrs_workspace_bytes(self._h, length, shard_len, nstripes))

    def decode_ptrs(self, shards, length, eras=None, neras=None, result=None, positions=None,
                    corr=None, stream=None):
        """The pointer form of ``decode_interleaved`` (ezrs_decode_ptrs): one stripe.  shards:
        length + nroots 1-D contiguous device tensors of equal length, by position (data first, then
        parity); codeword j is symbol j of every shard and is decoded in place, errors and erasures.
        Every shard is read and may be written; a lost shard is a tensor to rebuild into, its position
        in every codeword's erasure list.  Returns the int32 result tensor [shard_len]."""
        shards = list(shards)
        arr, n = _shard_ptrs(shards, "shards", length + self.nroots, (), self.device,
                             self.info.datum_bytes)
        result, out = self._decode_out(n, eras, neras, result, positions, corr, like=shards[0])
        _check(lib().ezrs_decode_ptrs(self._h, arr, length, n, *out, _stream_ptr(stream)),
               "ezrs_decode_ptrs")
        return result

    def decode_ptrs_batch(self, table, length, shard_len, align=None, eras=None, neras=None,
                          result=None, positions=None, corr=None, stream=None):
        """The batched pointer form (ezrs_decode_ptrs_batch): table is the int64 device tensor
        [nstripes, pitch >= length + nroots] of ``Recon.reconstruct_ptrs_batch`` (``ptr_table`` builds
        one), every entry below length + nroots a buffer of shard_len symbols.  align: what every
        pointer is a multiple of, 16, 4 or the datum size (None); a promise, not checked.  The table
        is read while the kernels run.  Returns the int32 result tensor [nstripes * shard_len],
        stripe-major."""
        nstripes, pitch = _ptr_table(table, "table", length + self.nroots, self.device)
        shard_len, align = int(shard_len), _align(align, self.info.datum_bytes)
        if shard_len < 0:
            raise EzrsError("shard_len: negative")
        result, out = self._decode_out(nstripes * shard_len, eras, neras, result, positions, corr, like=table)
        _check(lib().ezrs_decode_ptrs_batch(self._h, _tp(table), pitch, length, shard_len, nstripes, align,
                                            *out, _stream_ptr(stream)), "ezrs_decode_ptrs_batch")
        return result

    # -- selection: list the failed codewords of a verify on the device, decode only those --------
    def _sel_list(self, t, what, n=None):
        """Validate an int64 1-D contiguous device tensor (of at least n entries); None passes."""
        import torch
        if t is None:
            return
        _dev_rows(t, what, self.device, 8, ndim=1)
        if t.dtype != torch.int64:
            raise EzrsError(f"{what}: expected int64 entries, got {t.dtype}")
        if t.shape[0] > 1 and t.stride(0) != 1:
            raise EzrsError(f"{what}: expected a contiguous tensor")
        if n is not None and t.shape[0] < n:
            raise EzrsError(f"{what}: {t.shape[0]} entries, the call needs {n}")

    def _sel_rows(self, sel, count, **outs):
        """The checks the two selected decodes share; returns nsel.  The outputs are compact: a row
        per entry of sel."""
        self._sel_list(sel, "sel", 0)
        self._sel_list(count, "count", 1)
        if sel is None:
            raise EzrsError("sel: None")
        for what, t in outs.items():
            if t is not None and getattr(t, "shape", None) is not None and t.shape[0] < sel.shape[0]:
                raise EzrsError(f"{what}: {t.shape[0]} rows, sel has {sel.shape[0]} entries")
        return sel.shape[0]

    def select_workspace_bytes(self, n):
        return int(lib().ezrs_select_workspace_bytes(n))

    def select_failed(self, result, cap=None, base=0, sel=None, count=None, stream=None):
        """ezrs_select_failed: result is an int32 1-D contiguous device tensor (a verify's or a
        decode's); returns (sel, count), int64 device tensors of cap entries (default: one per
        result) and of one: sel[:min(count, cap)] = base + k for every k with result[k] < 0,
        ascending, the rest of sel ``SEL_NONE``, count the number of such k (it may exceed cap).
        Nothing is read on the host: both feed ``decode_ptrs_select`` / ``decode_interleaved_select``
        on the same stream as they are."""
        import torch
        _dev_rows(result, "result", self.device, 4, ndim=1)
        if result.dtype != torch.int32:
            raise EzrsError(f"result: expected int32 entries, got {result.dtype}")
        n = result.shape[0]
        if n > 1 and result.stride(0) != 1:
            raise EzrsError("result: expected a contiguous tensor")
        cap, base = (n if cap is None else int(cap)), int(base)
        if cap < 0 or base < 0:
            raise EzrsError("cap, base: negative")
        if sel is None:
            sel = torch.empty(cap, dtype=torch.int64, device=result.device)
        if count is None:
            count = torch.empty(1, dtype=torch.int64, device=result.device)
        self._sel_list(sel, "sel", cap)
        self._sel_list(count, "count", 1)
        # an empty tensor may have no address: with cap == 0 nothing is written through sel
        _check(lib().ezrs_select_failed(self._h, _tp(result), n, base, _tp(sel if cap else count), cap,
                                        _tp(count), _stream_ptr(stream)), "ezrs_select_failed")
        return sel, count

    def decode_select_workspace_bytes(self, length, nsel):
        return int(lib().ezrs_decode_select_workspace_bytes(self._h, length, nsel))

    def decode_ptrs_select(self, table, length, shard_len, sel, count=None, eras=None, neras=None,
                           result=None, positions=None, corr=None, stream=None):
        """ezrs_decode_ptrs_select: ``decode_ptrs_batch`` of only the codewords sel names.  table,
        length and shard_len as there (no align: symbols move one element at a time); sel: an int64
        device tensor, row i of the call decodes codeword sel[i] = s * shard_len + j; count: None, or
        an int64 device tensor whose first entry bounds the rows used.  A row past count[0], or whose
        entry is not a codeword of the table (``SEL_NONE``), is skipped: nothing of it is read or
        written and its outputs are those of an all-zero codeword.  eras, neras, result, positions
        and corr have one row per entry of sel.  sel, count and the table are read while the kernels
        run.  Returns the int32 result tensor [len(sel)]."""
        nstripes, pitch = _ptr_table(table, "table", length + self.nroots, self.device)
        shard_len = int(shard_len)
        if shard_len < 0:
            raise EzrsError("shard_len: negative")
        nsel = self._sel_rows(sel, count, eras=eras, neras=neras, result=result, positions=positions, corr=corr)
        result, out = self._decode_out(nsel, eras, neras, result, positions, corr, like=table)
        _check(lib().ezrs_decode_ptrs_select(self._h, _tp(table), pitch, length, shard_len, nstripes, _tp(sel),
                                             nsel, _tp(count), *out, _stream_ptr(stream)),
               "ezrs_decode_ptrs_select")
        return result

    def decode_interleaved_select(self, frames, sel, count=None, eras=None, neras=None, result=None,
                                  positions=None, corr=None, stream=None):
        """ezrs_decode_interleaved_select: ``decode_interleaved`` of only the codewords sel names,
        sel[i] = f * depth + j; sel, count and the outputs as in ``decode_ptrs_select``.  Returns the
        int32 result tensor [len(sel)]."""
        fp, ss, depth, length, nframes = self._frames(frames)
        nsel = self._sel_rows(sel, count, eras=eras, neras=neras, result=result, positions=positions, corr=corr)
        result, out = self._decode_out(nsel, eras, neras, result, positions, corr, like=frames)
        _check(lib().ezrs_decode_interleaved_select(self._h, _tp(frames), fp, ss, depth, length, nframes,
                                                    _tp(sel), nsel, _tp(count), *out, _stream_ptr(stream)),
               "ezrs_decode_interleaved_select")
        return result

    def recon_plan(self, length, lost):
        """Reconstruction plan for codewords of `length` data symbols whose symbols at the
        positions `lost` (relative to the first data symbol, parity at length..) are gone in
        every codeword -- ezrs_recon_create.  Returns a Recon."""
        return Recon(self, length, lost)

    def update_plan(self, length, changed):
        """Parity-update plan for codewords of `length` data symbols whose data symbols at the
        positions `changed` (relative to the first data symbol) are replaced in every codeword --
        ezrs_update_create.  Returns an Update."""
        return Update(self, length, changed)

    # -- host batch forms ----------------------------------------------------------------------
    def encode_host(self, data, length=None, parity=None, chunk=0):
        """data: [ncw, stride] numpy rows (only read); parity: [ncw, >=nroots] array, or None:
        each row carries its parity after its data (ezrs_encode_rows_host)."""
        w = self.info.datum_bytes
        ncw = data.shape[0]
        ds = _host_rows(data, "data", w)
        ps = _host_rows(parity, "parity", w)
        length = data.shape[1] - self.nroots if length is None else length
        if parity is None:
            _check(lib().ezrs_encode_rows_host(self._h, _np(data), ds, length, ncw, chunk),
                   "ezrs_encode_rows_host")
        else:
            _check(lib().ezrs_encode_host(self._h, _np(data), ds, length, _np(parity), ps, ncw,
                                          chunk), "ezrs_encode_host")

    def decode_host(self, data, length=None, parity=None, eras=None, neras=None,
                    positions=None, corr=None, chunk=0):
        w = self.info.datum_bytes
        ncw = data.shape[0]
        ds = _host_rows(data, "data", w)
        ps = _host_rows(parity, "parity", w)
        result, out = self._decode_out(ncw, eras, neras, None, positions, corr)
        length = data.shape[1] - self.nroots if length is None else length
        _check(lib().ezrs_decode_host(self._h, _np(data), ds, length, _np(parity), ps, *out, ncw, chunk),
               "ezrs_decode_host")
        return result

    # -- rsencode wire format -------------------------------------------------------------------
    def stream_encode(self, data, chunk=128):
        """bytes -> rsencode-format bytes (each chunk followed by its parity; include/ezrs.h
        ezrs_stream_encode).  Returns (encoded, ok); ok is False when a trailing partial symbol
        stopped the stream (the whole chunks before it are encoded, as rsencode does)."""
        src = np.frombuffer(bytes(data), np.uint8)
        cap = int(lib().ezrs_stream_encoded_bound(self._h, src.size, chunk)) or 1
        out = np.zeros(cap, np.uint8)
        n = _sz(0)
        rc = lib().ezrs_stream_encode(self._h, _np(src) if src.size else None, src.size, chunk,
                                      _np(out), cap, C.byref(n))
        if rc not in (0, -errno.EMSGSIZE):
            _check(rc, "ezrs_stream_encode")
        return out[:n.value].tobytes(), rc == 0

    def stream_decode(self, data, chunk=128):
        """rsencode-format bytes -> (decoded bytes, chunks that failed to decode, ok)."""
        src = np.frombuffer(bytes(data), np.uint8)
        out = np.zeros(max(src.size, 1), np.uint8)
        n, nf = _sz(0), _sz(0)
        rc = lib().ezrs_stream_decode(self._h, _np(src) if src.size else None, src.size, chunk,
                                      _np(out), out.size, C.byref(n), C.byref(nf))
        if rc not in (0, -errno.EMSGSIZE):
            _check(rc, "ezrs_stream_decode")
        return out[:n.value].tobytes(), nf.value, rc == 0


class _Plan:
    """What Recon and Update share: the plan's handle (made by ``_create``, released by the C
    function named ``_destroy``) and the check of the tensors a plan is applied to."""

    def _create(self, create, codec, length, positions):
        self.length, self.nroots, self.device = int(length), codec.nroots, codec.device
        self._w = codec.info.datum_bytes
        arr = (C.c_uint32 * max(len(positions), 1))(*positions)
        h = _vp()
        self._h = None
        _check(getattr(lib(), create)(C.byref(h), codec._h, self.length, arr, len(positions)), create)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                getattr(lib(), self._destroy)(h)
            except Exception:
                pass
            self._h = None

    def _sym_rows(self, t, what, nsym, shape):
        """Validate a [nframes, nsym, depth] device tensor with a contiguous last dimension."""
        if not getattr(t, "is_cuda", False):
            raise EzrsError(f"{what}: expected a GPU tensor")
        if t.device.index != self.device:
            raise EzrsError(f"{what}: tensor on cuda:{t.device.index}, plan on cuda:{self.device}")
        if t.element_size() != self._w:
            raise EzrsError(f"{what}: expected {self._w}-byte elements, got {t.dtype}")
        if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
            raise EzrsError(f"{what}: expected a 3-D tensor {shape} with a contiguous last dimension")
        if t.shape[1] != nsym or t.shape[2] == 0:
            raise EzrsError(f"{what}: {t.shape[1]} symbols per codeword, the plan has {nsym}, and a "
                            "depth of at least 1")

    def _shard_ptrs(self, seq, what, n, optional, shard_len=None):
        return _shard_ptrs(seq, what, n, optional, self.device, self._w, shard_len)

    def _ptr_table(self, t, what, need):
        return _ptr_table(t, what, need, self.device)

    def _align(self, align):
        return _align(align, self._w)


class Recon(_Plan):
    """A reconstruction plan (ezrs_recon_create): one loss pattern shared by every codeword, solved
    once; ``reconstruct`` rebuilds the lost symbols of interleaved frames in place.  The plan keeps
    nothing of the codec it was made from.

    * ``lost``       the lost positions, in the order given (the order of the rebuild rows)
    * ``survivors``  the surviving positions, ascending
    * ``nlost``      len(lost); ``result`` entries are nlost or -1"""

    _destroy = "ezrs_recon_destroy"

    def __init__(self, codec, length, lost):
        self.lost = [int(p) for p in lost]
        self.nlost = len(self.lost)
        self._create("ezrs_recon_create", codec, length, self.lost)
        gone = set(self.lost)
        self.survivors = [p for p in range(self.length + self.nroots) if p not in gone]

    def reconstruct(self, frames, result=None, stream=None):
        """frames: [nframes, length + nroots, depth] device tensor as in Codec.encode_interleaved;
        the lost symbols of every codeword are overwritten, nothing else.  result: an int32 device
        tensor [nframes * depth] (frame-major) that receives nlost, or -1 where the survivors are
        not consistent with any codeword; None: no check.  Returns result."""
        self._sym_rows(frames, "frames", self.length + self.nroots, "[nframes, len + nroots, depth]")
        nframes, _, depth = frames.shape
        if result is not None:
            _dev_rows(result, "result", self.device, 4, ndim=1)
            if result.shape[0] < nframes * depth:
                raise EzrsError("result: fewer entries than codewords")
        _check(lib().ezrs_reconstruct_interleaved(
            self._h, _tp(frames), frames.stride(0), frames.stride(1), depth, nframes, _tp(result),
            _stream_ptr(stream)), "ezrs_reconstruct_interleaved")
        return result

    def reconstruct_ptrs(self, shards, result=None, stream=None):
        """The pointer form (ezrs_reconstruct_ptrs): one stripe, every shard a tensor of its own.
        shards: length + nroots 1-D contiguous device tensors of equal length, by position; the
        survivors are only read, the tensors at the lost positions receive the rebuilt shards, and
        None there (and only there) means that shard is not wanted.  result: as in ``reconstruct``,
        one entry per symbol of a shard.  Returns result."""
        arr, n = self._shard_ptrs(shards, "shards", self.length + self.nroots, set(self.lost))
        if result is not None:
            _dev_rows(result, "result", self.device, 4, ndim=1)
            if result.shape[0] < n:
                raise EzrsError("result: fewer entries than codewords")
        _check(lib().ezrs_reconstruct_ptrs(self._h, arr, n, _tp(result), _stream_ptr(stream)),
               "ezrs_reconstruct_ptrs")
        return result


    def reconstruct_ptrs_batch(self, table, shard_len, align=None, result=None, stream=None):
        """The batched pointer form (ezrs_reconstruct_ptrs_batch): table is an int64 device tensor
        [nstripes, pitch >= length + nroots] of device pointers, entry [s, p] the shard at position
        p of stripe s, shard_len symbols (``ptr_table`` builds one); 0 at a lost position: that
        stripe does not want that shard.  align: what every pointer is a multiple of, 16, 4 or the
        datum size (None); a promise, not checked.  The table is read while the kernels run: keep it
        alive and unchanged until the stream has done the work.  result: an int32 device tensor
        [nstripes * shard_len], stripe-major, or None.  Returns result."""
        nstripes, pitch = self._ptr_table(table, "table", self.length + self.nroots)
        shard_len, align = int(shard_len), self._align(align)
        if shard_len < 0:
            raise EzrsError("shard_len: negative")
        if result is not None:
            _dev_rows(result, "result", self.device, 4, ndim=1)
            if result.shape[0] < nstripes * shard_len:
                raise EzrsError("result: fewer entries than codewords")
        _check(lib().ezrs_reconstruct_ptrs_batch(self._h, _tp(table), pitch, shard_len, nstripes, align,
                                                 _tp(result), _stream_ptr(stream)),
               "ezrs_reconstruct_ptrs_batch")
        return result


PLAN_SKIP = 0xFFFFFFFF                             # EZRS_PLAN_SKIP: in plan_of, leave this stripe alone
SEL_NONE = -1                                      # EZRS_SEL_NONE as int64: in sel, skip this row


class ReconSet(_Plan):
    """A set of reconstruction plans of one codec, length and device (ezrs_recon_set_create), for
    ``reconstruct_ptrs_mixed``: the batched pointer form with a loss pattern per stripe.  The set
    copies the plans' tables; it keeps nothing of the plans or the codec.

    * ``nplans``  the number of plans; an index at or above it (``PLAN_SKIP``) skips a stripe
    * ``nlost``   the plans' nlost, by index: what ``result`` holds for a stripe of that plan, or -1"""

    _destroy = "ezrs_recon_set_destroy"

    def __init__(self, plans):
        plans = list(plans)
        for i, p in enumerate(plans):
            if not isinstance(p, Recon) or not p._h:
                raise EzrsError(f"plans[{i}]: expected a Recon plan")
        self.nplans, self.nlost = len(plans), [p.nlost for p in plans]
        arr = (_vp * max(len(plans), 1))(*[p._h for p in plans])
        h = _vp()
        self._h = None
        _check(lib().ezrs_recon_set_create(C.byref(h), arr, len(plans)), "ezrs_recon_set_create")
        self._h = h
        self.length, self.nroots, self.device, self._w = (plans[0].length, plans[0].nroots, plans[0].device,
                                                          plans[0]._w)

    def reconstruct_ptrs_mixed(self, table, plan_of, shard_len, align=None, result=None, stream=None):
        """ezrs_reconstruct_ptrs_mixed: table, shard_len, align, result and stream as in
        ``Recon.reconstruct_ptrs_batch``; plan_of: an int32 or uint32 device tensor of at least
        nstripes entries, stripe s working under plan plan_of[s] of the set (0 in the table where
        that plan has lost a position: not wanted by that stripe).  A stripe whose index is not
        below ``nplans`` is skipped: nothing of it is read or written, and its result entries stay.
        The table and plan_of are read while the kernels run.  Returns result."""
        import torch
        nstripes, pitch = self._ptr_table(table, "table", self.length + self.nroots)
        shard_len, align = int(shard_len), self._align(align)
        if shard_len < 0:
            raise EzrsError("shard_len: negative")
        _dev_rows(plan_of, "plan_of", self.device, 4, ndim=1)
        if plan_of.dtype not in (torch.int32, torch.uint32):
            raise EzrsError(f"plan_of: expected int32 or uint32 entries, got {plan_of.dtype}")
        if plan_of.shape[0] < nstripes:
            raise EzrsError("plan_of: fewer entries than stripes")
        if result is not None:
            _dev_rows(result, "result", self.device, 4, ndim=1)
            if result.shape[0] < nstripes * shard_len:
                raise EzrsError("result: fewer entries than codewords")
        _check(lib().ezrs_reconstruct_ptrs_mixed(self._h, _tp(plan_of), _tp(table), pitch, shard_len, nstripes,
                                                 align, _tp(result), _stream_ptr(stream)),
               "ezrs_reconstruct_ptrs_mixed")
        return result


class Update(_Plan):
    """A parity-update plan (ezrs_update_create): one set of changed data positions shared by every
    codeword; ``apply`` XORs G[:, changed]·(new ^ old) into the parity of interleaved frames where it
    lies and stores the new data symbols.  The plan keeps nothing of the codec it was made from.

    * ``changed``   the changed data positions, in the order given (the order of ``newsyms``' rows)
    * ``nchanged``  len(changed)"""

    _destroy = "ezrs_update_destroy"

    def __init__(self, codec, length, changed):
        self.changed = [int(p) for p in changed]
        self.nchanged = len(self.changed)
        self._create("ezrs_update_create", codec, length, self.changed)

    def apply(self, frames, newsyms, stream=None):
        """frames: [nframes, length + nroots, depth] device tensor as in Codec.encode_interleaved;
        newsyms: [nframes, nchanged, depth] device tensor, row r the new contents of the symbols at
        changed[r] (only read; it must not overlap the changed and parity symbols of `frames`).  The
        parity of every codeword follows the change and the changed symbols take their new values;
        nothing else is written."""
        self._sym_rows(frames, "frames", self.length + self.nroots, "[nframes, len + nroots, depth]")
        self._sym_rows(newsyms, "newsyms", self.nchanged, "[nframes, nchanged, depth]")
        nframes, _, depth = frames.shape
        if newsyms.shape[0] != nframes or newsyms.shape[2] != depth:
            raise EzrsError(f"newsyms: shape {tuple(newsyms.shape)}, expected "
                            f"({nframes}, {self.nchanged}, {depth})")
        _check(lib().ezrs_update_interleaved(
            self._h, _tp(frames), frames.stride(0), frames.stride(1), depth, nframes, _tp(newsyms),
            newsyms.stride(0), newsyms.stride(1), _stream_ptr(stream)), "ezrs_update_interleaved")

    def apply_ptrs(self, shards, newsyms, stream=None):
        """The pointer form (ezrs_update_ptrs): one stripe, every shard a tensor of its own.
        shards: length + nroots entries by position, of which only the changed and the parity
        positions are used (1-D contiguous device tensors of equal length); every other entry may be
        None: those shards need not be on the device.  newsyms: nchanged such tensors, in the order
        of ``changed``, only read; they must not overlap the changed and parity shards."""
        S = self.length + self.nroots
        used = set(self.changed) | set(range(self.length, S))
        shards = [t if i in used else None for i, t in enumerate(shards)]   # the others are ignored
        arr, n = self._shard_ptrs(shards, "shards", S, set(range(S)) - used)
        new, _ = self._shard_ptrs(newsyms, "newsyms", self.nchanged, (), n)
        _check(lib().ezrs_update_ptrs(self._h, arr, new, n, _stream_ptr(stream)), "ezrs_update_ptrs")


    def apply_ptrs_batch(self, table, new_table, shard_len, align=None, stream=None):
        """The batched pointer form (ezrs_update_ptrs_batch): table as in
        ``Recon.reconstruct_ptrs_batch``, of which only the entries at the changed and the parity
        positions are used; new_table: int64 device tensor [nstripes, pitch >= nchanged], entry
        [s, r] the new symbols of changed[r] of stripe s.  align: the promise for the pointers of
        both tables.  Both tables are read while the kernels run."""
        nstripes, pitch = self._ptr_table(table, "table", self.length + self.nroots)
        nnew, new_pitch = self._ptr_table(new_table, "new_table", self.nchanged)
        if nnew != nstripes:
            raise EzrsError(f"new_table: {nnew} stripes, table has {nstripes}")
        shard_len, align = int(shard_len), self._align(align)
        if shard_len < 0:
            raise EzrsError("shard_len: negative")
        _check(lib().ezrs_update_ptrs_batch(self._h, _tp(table), pitch, _tp(new_table), new_pitch, shard_len,
                                            nstripes, align, _stream_ptr(stream)),
               "ezrs_update_ptrs_batch")


class UpdateSet(_Plan):
    """A set of parity-update plans of one codec, length and device (ezrs_update_set_create), for
    ``apply_ptrs_mixed``: the batched pointer form with a change set per stripe.  The set copies
    the plans' tables; it keeps nothing of the plans or the codec.

    * ``nplans``    the number of plans; an index at or above it (``PLAN_SKIP``) skips a stripe
    * ``nchanged``  the plans' nchanged, by index; new_table needs a pitch of at least the largest"""

    _destroy = "ezrs_update_set_destroy"

    def __init__(self, plans):
        plans = list(plans)
        for i, p in enumerate(plans):
            if not isinstance(p, Update) or not p._h:
                raise EzrsError(f"plans[{i}]: expected an Update plan")
        self.nplans, self.nchanged = len(plans), [p.nchanged for p in plans]
        arr = (_vp * max(len(plans), 1))(*[p._h for p in plans])
        h = _vp()
        self._h = None
        _check(lib().ezrs_update_set_create(C.byref(h), arr, len(plans)), "ezrs_update_set_create")
        self._h = h
        self.length, self.nroots, self.device, self._w = (plans[0].length, plans[0].nroots, plans[0].device,
                                                          plans[0]._w)

    def apply_ptrs_mixed(self, table, new_table, plan_of, shard_len, align=None, stream=None):
        """ezrs_update_ptrs_mixed: table, new_table, shard_len, align and stream as in
        ``Update.apply_ptrs_batch``; plan_of: an int32 or uint32 device tensor of at least nstripes
        entries, stripe s working under plan plan_of[s] of the set.  Of table[s] only the entries at
        that plan's changed positions and at the parity positions are used, of new_table[s] only
        the first nchanged of that plan, in the order of its ``changed``; new_table's pitch is at
        least the largest nchanged of the set.  A stripe whose index is not below ``nplans`` is
        skipped: nothing of it is read or written.  Two stripes of one call must not be the same
        physical stripe.  Both tables and plan_of are read while the kernels run."""
        import torch
        nstripes, pitch = self._ptr_table(table, "table", self.length + self.nroots)
        nnew, new_pitch = self._ptr_table(new_table, "new_table", max(self.nchanged))
        if nnew != nstripes:
            raise EzrsError(f"new_table: {nnew} stripes, table has {nstripes}")
        shard_len, align = int(shard_len), self._align(align)
        if shard_len < 0:
            raise EzrsError("shard_len: negative")
        _dev_rows(plan_of, "plan_of", self.device, 4, ndim=1)
        if plan_of.dtype not in (torch.int32, torch.uint32):
            raise EzrsError(f"plan_of: expected int32 or uint32 entries, got {plan_of.dtype}")
        if plan_of.shape[0] < nstripes:
            raise EzrsError("plan_of: fewer entries than stripes")
        _check(lib().ezrs_update_ptrs_mixed(self._h, _tp(plan_of), _tp(table), pitch, _tp(new_table), new_pitch,
                                            shard_len, nstripes, align, _stream_ptr(stream)),
               "ezrs_update_ptrs_mixed")


def ptr_table(stripes, optional=()):
    """The pointer table of the batched pointer forms from tensors.  stripes: a sequence of
    per-stripe sequences (all of one length) of 1-D contiguous device tensors, all on one device,
    with elements of one size and of one length; None is allowed at the indices in `optional`.
    Returns (table, shard_len, align): the int64 device tensor [nstripes, entries] of their device
    pointers (0 for None), their common length, and the largest of 16 / 4 / the element size that
    every pointer is a multiple of.  The tensors must outlive the use of the table."""
    import torch
    stripes = [list(st) for st in stripes]
    if not stripes or not stripes[0]:
        raise EzrsError("ptr_table: no stripes, or no entries in a stripe")
    optional = set(optional)
    rows, first, bits = [], None, 0
    for s, st in enumerate(stripes):
        if len(st) != len(stripes[0]):
            raise EzrsError(f"ptr_table: stripe {s} has {len(st)} entries, stripe 0 has {len(stripes[0])}")
        row = []
        for i, t in enumerate(st):
            what = f"ptr_table: stripes[{s}][{i}]"
            if t is None:
                if i not in optional:
                    raise EzrsError(f"{what}: None where a buffer is needed")
                row.append(0)
                continue
            if not getattr(t, "is_cuda", False):
                raise EzrsError(f"{what}: expected a GPU tensor")
            if t.dim() != 1 or (t.shape[0] > 1 and t.stride(0) != 1):
                raise EzrsError(f"{what}: expected a 1-D contiguous tensor")
            if first is None:
                first = t
            if t.device != first.device:
                raise EzrsError(f"{what}: tensor on {t.device}, the others on {first.device}")
            if t.element_size() != first.element_size():
                raise EzrsError(f"{what}: {t.element_size()}-byte elements, the others have "
                                f"{first.element_size()}")
            if t.shape[0] != first.shape[0]:
                raise EzrsError(f"{what}: {t.shape[0]} symbols, the other shards have {first.shape[0]}")
            bits |= t.data_ptr()
            row.append(t.data_ptr())
        rows.append(row)
    if first is None:
        raise EzrsError("ptr_table: no buffer at all")
    table = torch.tensor(rows, dtype=torch.int64).to(first.device)
    align = 16 if bits % 16 == 0 else 4 if bits % 4 == 0 else first.element_size()
    return table, first.shape[0], align


def update_bitmatrix(params, length, changed):
    """The matrix of a parity-update plan on the host (ezrs_update_bitmatrix; no device).  params:
    (symbol_bits, poly, fcr, prim, nroots, dual).  Returns cols, a uint16 array
    [nroots, nchanged, symbol_bits]: parity symbol `row` changes by the XOR of cols[row, r, b] over
    the set bits b of new ^ old at changed[r]."""
    mm, poly, fcr, prim, nroots, dual = params
    changed = [int(p) for p in changed]
    cols = np.zeros((nroots, len(changed), mm), np.uint16)
    arr = (C.c_uint32 * max(len(changed), 1))(*changed)
    _check(lib().ezrs_update_bitmatrix(mm, poly, fcr, prim, nroots, int(bool(dual)), length, arr,
                                       len(changed), _np(cols), cols.size),
           "ezrs_update_bitmatrix")
    return cols


def recon_bitmatrix(params, length, lost):
    """The matrix of a reconstruction plan on the host (ezrs_recon_bitmatrix; no device).  params:
    (symbol_bits, poly, fcr, prim, nroots, dual).  Returns (cols, survivors): cols a uint16 array
    [nroots, nsurv, symbol_bits] -- rows 0..len(lost)-1 rebuild `lost` in the order given, the others
    are check rows -- and the surviving positions, ascending."""
    mm, poly, fcr, prim, nroots, dual = params
    lost = [int(p) for p in lost]
    nsurv = max(length + nroots - len(lost), 0)
    cols = np.zeros((nroots, nsurv, mm), np.uint16)
    surv = np.zeros(max(nsurv, 1), np.uint32)
    arr = (C.c_uint32 * max(len(lost), 1))(*lost)
    _check(lib().ezrs_recon_bitmatrix(mm, poly, fcr, prim, nroots, int(bool(dual)), length, arr,
                                      len(lost), _np(cols), cols.size, _np(surv)),
           "ezrs_recon_bitmatrix")
    return cols, surv[:nsurv]


class BCH:
    """A binary BCH codec resident on one HIP device: ezpwd::bch_base(m, t, prim_poly) /
    ezpwd::BCH<N,K,T> (c++/ezpwd/bch:48-463) over include/ezbch.h.

    * ``encode(data, length, ecc)`` -- bch_base::encode(data, len, parity) per row (bch:196-205)
    * ``decode(data, length, ecc)`` -- bch_base::decode(data, len, parity, &position), i.e.
      correct_bch (bch:316-331, bch_base:168-199): int32 result per row, bits fixed in place."""

    def __init__(self, m, t, prim_poly=0, device=0, _h=None):
        h = _vp()
        if _h is None:
            _check(lib().ezbch_create(C.byref(h), m, t, prim_poly, device), "ezbch_create", True)
        else:
            h = _h
        self._h = h
        info = BCHInfo()
        _check(lib().ezbch_get_info(self._h, C.byref(info)), "ezbch_get_info", True)
        self.info = info
        self.m, self.n, self.t, self.ecc_bits, self.ecc_bytes = (info.m, info.n, info.t,
                                                                 info.ecc_bits, info.ecc_bytes)
        self.device = info.device

    @classmethod
    def nkt(cls, n, k, t, device=0):
        h = _vp()
        _check(lib().ezbch_create_nkt(C.byref(h), n, k, t, device), f"ezbch_create_nkt({n},{k},{t})",
               True)
        return cls(0, 0, _h=h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().ezbch_destroy(h)
            except Exception:
                pass
            self._h = None

    def __repr__(self):   # bch_base:204-215
        return f"BCH({self.n},{self.n - self.ecc_bits},{self.t})"

    @property
    def max_len(self):
        return (self.n - self.ecc_bits) // 8

    def encode(self, data, length=None, ecc=None, stream=None):
        """data: [ncw, stride] uint8 device tensor; ecc: [ncw, >=ecc_bytes] tensor, or None: the ECC
        goes to columns length..length+ecc_bytes of each row (ezbch_encode_rows)."""
        ncw = data.shape[0]
        ds = _dev_rows(data, "data", self.device, 1)
        es = _dev_rows(ecc, "ecc", self.device, 1)
        length = data.shape[1] - self.ecc_bytes if length is None else length
        if ecc is None:
            _check(lib().ezbch_encode_rows(self._h, _tp(data), ds, length, ncw, _stream_ptr(stream)),
                   "ezbch_encode_rows", True)
        else:
            _check(lib().ezbch_encode(self._h, _tp(data), ds, length, _tp(ecc), es, ncw,
                                      _stream_ptr(stream)), "ezbch_encode", True)

    def decode(self, data, length=None, ecc=None, result=None, errloc=None, stream=None):
        import torch
        ncw = data.shape[0]
        ds = _dev_rows(data, "data", self.device, 1)
        es = _dev_rows(ecc, "ecc", self.device, 1)
        ls = _dev_rows(errloc, "errloc", self.device, 4)
        length = data.shape[1] - self.ecc_bytes if length is None else length
        if result is None:
            result = torch.empty(ncw, dtype=torch.int32, device=data.device)
        _dev_rows(result, "result", self.device, 4, ndim=1)
        _check(lib().ezbch_decode(self._h, _tp(data), ds, length, _tp(ecc), es, _tp(result),
                                  _tp(errloc), ls, ncw, _stream_ptr(stream)), "ezbch_decode", True)
        return result

    def decode_ecc(self, ecc, length, result=None, errloc=None, stream=None):
        """decode_bch's recv XOR calc form: ecc rows hold the ECC differences; returns the int32
        results (errors found, or a negative errno); nothing is corrected (ezbch_decode_ecc)."""
        import torch
        ncw = ecc.shape[0]
        es = _dev_rows(ecc, "ecc", self.device, 1)
        ls = _dev_rows(errloc, "errloc", self.device, 4)
        if result is None:
            result = torch.empty(ncw, dtype=torch.int32, device=ecc.device)
        _dev_rows(result, "result", self.device, 4, ndim=1)
        _check(lib().ezbch_decode_ecc(self._h, _tp(ecc), es, length, _tp(result), _tp(errloc), ls,
                                      ncw, _stream_ptr(stream)), "ezbch_decode_ecc", True)
        return result

    def decode_syn(self, syn, length, result=None, errloc=None, stream=None):
        """decode_bch's syndrome form: syn rows hold S_1..S_2t (int32/uint32, 2t per row); returns
        the int32 results; nothing is corrected (ezbch_decode_syn)."""
        import torch
        ncw = syn.shape[0]
        ss = _dev_rows(syn, "syn", self.device, 4)
        ls = _dev_rows(errloc, "errloc", self.device, 4)
        if result is None:
            result = torch.empty(ncw, dtype=torch.int32, device=syn.device)
        _dev_rows(result, "result", self.device, 4, ndim=1)
        _check(lib().ezbch_decode_syn(self._h, _tp(syn), ss, length, _tp(result), _tp(errloc), ls,
                                      ncw, _stream_ptr(stream)), "ezbch_decode_syn", True)
        return result

    def encode_host(self, data, length=None, ecc=None, chunk=0):
        ncw = data.shape[0]
        ds = _host_rows(data, "data", 1)
        es = _host_rows(ecc, "ecc", 1)
        length = data.shape[1] - self.ecc_bytes if length is None else length
        if ecc is None:
            _check(lib().ezbch_encode_rows_host(self._h, _np(data), ds, length, ncw, chunk),
                   "ezbch_encode_rows_host", True)
        else:
            _check(lib().ezbch_encode_host(self._h, _np(data), ds, length, _np(ecc), es, ncw, chunk),
                   "ezbch_encode_host", True)

    def decode_host(self, data, length=None, ecc=None, errloc=None, chunk=0):
        ncw = data.shape[0]
        ds = _host_rows(data, "data", 1)
        es = _host_rows(ecc, "ecc", 1)
        ls = _host_rows(errloc, "errloc", 4)
        length = data.shape[1] - self.ecc_bytes if length is None else length
        result = np.zeros(ncw, np.int32)
        _check(lib().ezbch_decode_host(self._h, _np(data), ds, length, _np(ecc), es, _np(result),
                                       _np(errloc), ls, ncw, chunk), "ezbch_decode_host", True)
        return result


def exported_symbols():
    """Function names declared in include/ezrs.h and include/ezbch.h."""
    import re
    names = set()
    for fn in (HEADER, BCH_HEADER):
        txt = open(fn).read()
        names |= set(re.findall(
            r"^\s*(?:int|void|const char \*|size_t)\s*\*?\s*(ez(?:rs|bch)_\w+)\s*\(", txt, re.M))
    return sorted(names)

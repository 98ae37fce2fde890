"""Strided-batch plans (include/fft_wgpu_amd_strided.h): the columns of row-major matrices, transformed in place.

``src`` holds ``batch`` matrices of ``fft_len`` rows x ``howmany`` columns back to back; every column becomes its own DFT
over the rows -- ``numpy.fft.fft(x.reshape(batch, fft_len, howmany), axis=1)`` -- in one launch and one pass over memory.
The classes mirror ``fft_wgpu_amd.Forward / Inverse / Onlyinverse`` (``X(device, queue, src, fft_len, howmany)``,
``X.proc(encoder) -> Buffer``); the result is always ``src`` itself.

The ctypes table of the ``fws_`` functions lives here.  ``libfft_wgpu_amd_strided.so`` is loaded on first use, not when
the package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi, _side
from ._ffi import _I32, _P, _PI32, _PI64, _PP, _PU64, _U32, _U64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_strided.so")
ABI_VERSION = 1   # FWS_ABI_VERSION of the include/fft_wgpu_amd_strided.h this binding was written against

_SIGNATURES = {
    "fws_abi_version": (_I32, []),
    "fws_describe": (_I32, [_U32, _U64, _U64, _PI32, _PI32, _PI32, _PU64]),
    "fws_plan_create": (_I32, [_P, _I32, _U32, _U64, _P, _PP]),
    "fws_plan_exec": (_I32, [_P, _P]),
    "fws_plan_get_i64": (_I32, [_P, ctypes.c_char_p, _PI64]),
    "fws_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_strided.so (once), after the main library, which it links against.  Raises if it was not built or reports
    another ABI version."""
    global _lib
    if _lib is None:
        _lib = _ffi.load(LIB_PATH, "fws", ABI_VERSION, _SIGNATURES, "fft_wgpu_amd_strided.h", "make -C fft_wgpu_amd/strided",
                         needs=_ffi.lib)
    return _lib


def describe(fft_len, howmany, batch=1):
    """The launch geometry a plan of this shape uses -- pure host logic, no GPU needed:
    {"tile_cols", "threads", "lds_bytes", "blocks"}."""
    tile, threads, lds, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fws_describe(fft_len, howmany, batch, ctypes.byref(tile), ctypes.byref(threads), ctypes.byref(lds),
                                  ctypes.byref(blocks)), None, "fws_describe")
    return {"tile_cols": tile.value, "threads": threads.value, "lds_bytes": lds.value, "blocks": blocks.value}


class _Plan(_side.Plan):
    _prefix = "fws"
    _kind = None

    def __init__(self, device, queue, src, fft_len, howmany):
        self.src = src
        self.fft_len = fft_len
        self.howmany = howmany
        self._create(lib(), device, queue, src, device._h, self._kind, fft_len, howmany, src._h)


class Forward(_Plan):
    """Unnormalised forward DFT of every column."""
    _kind = _ffi.FORWARD


class Inverse(_Plan):
    """Inverse DFT of every column with the 1/fft_len scale fused into the last stage."""
    _kind = _ffi.INVERSE_SCALED


class Onlyinverse(_Plan):
    """Inverse DFT of every column, unscaled."""
    _kind = _ffi.INVERSE_UNSCALED

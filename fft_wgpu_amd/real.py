"""Real-input plans (include/fft_wgpu_amd_real.h): rfft and irfft of batched rows, out of place, in one launch.

With ``n = fft_len`` a power of two from 2 to 4096 and ``M = n // 2``: ``Forward`` takes ``src`` -- ``batch`` rows of ``n``
float32 -- to ``dst`` -- ``batch`` rows of ``M + 1`` complex64, ``numpy.fft.rfft(x, axis=-1)``; ``Onlyinverse`` takes
``batch`` rows of ``M + 1`` complex64 to ``batch`` rows of ``n`` float32, ``n * numpy.fft.irfft(X, n, axis=-1)``, and
``Inverse`` is ``numpy.fft.irfft`` itself.  The classes mirror ``fft_wgpu_amd.Forward / Inverse / Onlyinverse``
(``X(device, queue, src, dst, fft_len)``, ``X.proc(encoder) -> Buffer``); the result is always ``dst``, and ``src`` is
never written.

The ctypes table of the ``fwr_`` functions lives here.  ``libfft_wgpu_amd_real.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi, _side
from ._ffi import _I32, _P, _PI32, _PI64, _PP, _PU64, _U32, _U64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_real.so")
ABI_VERSION = 1   # FWR_ABI_VERSION of the include/fft_wgpu_amd_real.h this binding was written against

_SIGNATURES = {
    "fwr_abi_version": (_I32, []),
    "fwr_describe": (_I32, [_U32, _U64, _PI32, _PI32, _PI32, _PU64]),
    "fwr_plan_create": (_I32, [_P, _I32, _U32, _P, _P, _PP]),
    "fwr_plan_exec": (_I32, [_P, _P]),
    "fwr_plan_get_i64": (_I32, [_P, ctypes.c_char_p, _PI64]),
    "fwr_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_real.so (once), after the main library, which it links against.  Raises if it was not built or reports
    another ABI version."""
    global _lib
    if _lib is None:
        _lib = _ffi.load(LIB_PATH, "fwr", ABI_VERSION, _SIGNATURES, "fft_wgpu_amd_real.h", "make -C fft_wgpu_amd/real",
                         needs=_ffi.lib)
    return _lib


def describe(fft_len, batch=1):
    """What a plan of this length over ``batch`` rows launches -- pure host logic, no GPU needed:
    {"threads", "lds_bytes", "rows_per_block", "blocks"}."""
    threads, lds, rows, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fwr_describe(fft_len, batch, ctypes.byref(threads), ctypes.byref(lds), ctypes.byref(rows),
                                  ctypes.byref(blocks)), None, "fwr_describe")
    return {"threads": threads.value, "lds_bytes": lds.value, "rows_per_block": rows.value, "blocks": blocks.value}


class _Plan(_side.Plan):
    _prefix = "fwr"
    _kind = None

    def __init__(self, device, queue, src, dst, fft_len):
        self.src = src
        self.dst = dst
        self.fft_len = fft_len
        self._create(lib(), device, queue, dst, device._h, self._kind, fft_len, src._h, dst._h)


class Forward(_Plan):
    """numpy.fft.rfft of every row: n float32 -> n / 2 + 1 complex64."""
    _kind = _ffi.FORWARD


class Inverse(_Plan):
    """numpy.fft.irfft of every row: n / 2 + 1 complex64 -> n float32."""
    _kind = _ffi.INVERSE_SCALED


class Onlyinverse(_Plan):
    """n * numpy.fft.irfft of every row, unscaled."""
    _kind = _ffi.INVERSE_UNSCALED

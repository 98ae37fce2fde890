"""Fused FFT-convolution plans (include/fft_wgpu_amd_conv.h): ``ifft(fft(x) * H)`` of batched rows in one launch.

With ``n = fft_len`` a power of two from 2 to 4096: ``src`` and ``dst`` hold ``batch`` rows of ``n`` complex64, ``filter``
holds ``F >= 1`` rows of ``n`` complex64, each a filter *spectrum* in natural bin order (what a ``Forward`` plan of length
``n`` writes).  Row ``b`` uses filter row ``b % F``.  ``Convolve`` is
``numpy.fft.ifft(numpy.fft.fft(src[b]) * filter[b % F])`` -- circular convolution; ``OnlyConvolve`` is ``n`` times that
(no scaling); ``conj_filter=True`` multiplies by ``conj(filter)`` instead -- circular cross-correlation.  ``dst`` may be
``src`` (the same Buffer): the in-place form.  ``X(device, queue, src, filter, dst, fft_len, conj_filter=False)``,
``X.proc(encoder) -> dst``; ``filter`` and, out of place, ``src`` are never written.

The ctypes table of the ``fwc_`` functions lives here.  ``libfft_wgpu_amd_conv.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi, _side
from ._ffi import _I32, _P, _PI32, _PI64, _PP, _PU64, _U32, _U64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_conv.so")
ABI_VERSION = 1   # FWC_ABI_VERSION of the include/fft_wgpu_amd_conv.h this binding was written against
CONJ_FILTER = 1   # FWC_CONJ_FILTER

_SIGNATURES = {
    "fwc_abi_version": (_I32, []),
    "fwc_describe": (_I32, [_U32, _U64, _PI32, _PI32, _PI32, _PU64]),
    "fwc_plan_create": (_I32, [_P, _I32, _U32, _U32, _P, _P, _P, _PP]),
    "fwc_plan_exec": (_I32, [_P, _P]),
    "fwc_plan_get_i64": (_I32, [_P, ctypes.c_char_p, _PI64]),
    "fwc_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_conv.so (once), after the main library, which it links against.  Raises if it was not built or reports
    another ABI version."""
    global _lib
    if _lib is None:
        _lib = _ffi.load(LIB_PATH, "fwc", ABI_VERSION, _SIGNATURES, "fft_wgpu_amd_conv.h", "make -C fft_wgpu_amd/conv",
                         needs=_ffi.lib)
    return _lib


def describe(fft_len, batch=1):
    """What a plan of this length over ``batch`` rows launches -- pure host logic, no GPU needed:
    {"threads", "lds_bytes", "rows_per_block", "blocks"}."""
    threads, lds, rows, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fwc_describe(fft_len, batch, ctypes.byref(threads), ctypes.byref(lds), ctypes.byref(rows),
                                  ctypes.byref(blocks)), None, "fwc_describe")
    return {"threads": threads.value, "lds_bytes": lds.value, "rows_per_block": rows.value, "blocks": blocks.value}


class _Plan(_side.Plan):
    _prefix = "fwc"
    _kind = None

    def __init__(self, device, queue, src, filter, dst, fft_len, conj_filter=False):
        self.src = src
        self.filter = filter
        self.dst = dst
        self.fft_len = fft_len
        self.conj_filter = bool(conj_filter)
        self._create(lib(), device, queue, dst, device._h, self._kind, CONJ_FILTER if conj_filter else 0, fft_len, src._h,
                     filter._h, dst._h)


class Convolve(_Plan):
    """numpy.fft.ifft(numpy.fft.fft(x) * H) of every row: circular convolution (correlation with conj_filter)."""
    _kind = _ffi.INVERSE_SCALED


class OnlyConvolve(_Plan):
    """fft_len * numpy.fft.ifft(numpy.fft.fft(x) * H) of every row: the unscaled inverse."""
    _kind = _ffi.INVERSE_UNSCALED

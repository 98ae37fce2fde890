"""2-D plans (include/fft_wgpu_amd_2d.h): batched row-major images, transformed in place.

``src`` holds ``batch`` images of ``rows`` x ``cols`` back to back; a plan computes
``numpy.fft.fft2(x.reshape(batch, rows, cols))`` (``ifft2`` for the inverses) in one launch (rows, cols <= 32) or two, for
every power-of-two width and height from 2 to 4096.  The classes mirror ``fft_wgpu_amd.Forward / Inverse / Onlyinverse``
(``X(device, queue, src, rows, cols)``, ``X.proc(encoder) -> Buffer``); the result is always ``src`` itself.

The ctypes table of the ``fw2_`` functions lives here.  ``libfft_wgpu_amd_2d.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi, _side
from ._ffi import _I32, _P, _PI32, _PI64, _PP, _PU64, _U32, _U64
from . import strided as _strided

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_2d.so")
ABI_VERSION = 1   # FW2_ABI_VERSION of the include/fft_wgpu_amd_2d.h this binding was written against

_SIGNATURES = {
    "fw2_abi_version": (_I32, []),
    "fw2_describe": (_I32, [_U32, _U32, _U64, _PI32, _PI32, _PI32, _PU64]),
    "fw2_plan_create": (_I32, [_P, _I32, _U32, _U32, _P, _PP]),
    "fw2_plan_exec": (_I32, [_P, _P]),
    "fw2_plan_get_i64": (_I32, [_P, ctypes.c_char_p, _PI64]),
    "fw2_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_2d.so (once), after the column plans and the main library, which it links against.  Raises if it
    was not built or reports another ABI version."""
    global _lib
    if _lib is None:
        _lib = _ffi.load(LIB_PATH, "fw2", ABI_VERSION, _SIGNATURES, "fft_wgpu_amd_2d.h", "make -C fft_wgpu_amd/fft2d",
                         needs=_strided.lib)
    return _lib


def describe(rows, cols, batch=1):
    """What a plan of this shape launches -- pure host logic, no GPU needed:
    {"launches", "row_threads", "row_lds_bytes", "row_blocks"}."""
    launches, threads, lds, blocks = _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fw2_describe(rows, cols, batch, ctypes.byref(launches), ctypes.byref(threads), ctypes.byref(lds),
                                  ctypes.byref(blocks)), None, "fw2_describe")
    return {"launches": launches.value, "row_threads": threads.value, "row_lds_bytes": lds.value, "row_blocks": blocks.value}


class _Plan(_side.Plan):
    _prefix = "fw2"
    _kind = None

    def __init__(self, device, queue, src, rows, cols):
        self.src = src
        self.rows = rows
        self.cols = cols
        self._create(lib(), device, queue, src, device._h, self._kind, rows, cols, src._h)


class Forward(_Plan):
    """Unnormalised forward 2-D DFT of every image."""
    _kind = _ffi.FORWARD


class Inverse(_Plan):
    """Inverse 2-D DFT of every image, scaled by 1 / (rows * cols)."""
    _kind = _ffi.INVERSE_SCALED


class Onlyinverse(_Plan):
    """Inverse 2-D DFT of every image, unscaled."""
    _kind = _ffi.INVERSE_UNSCALED

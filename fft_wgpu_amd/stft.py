"""Framed real-input plans (include/fft_wgpu_amd_stft.h): the rfft of overlapping, windowed frames of long real signals,
out of place, in one launch -- the frames of ``torch.stft(..., center=False, onesided=True)`` or ``scipy.signal.stft``.

With ``n = fft_len`` a power of two from 2 to 4096, ``M = n // 2``, ``hop >= 1`` and ``L = signal_len >= n``: ``src`` holds
signals of ``L`` float32 back to back, a signal has ``F = 1 + (L - n) // hop`` frames, and ``dst`` receives one row per frame,
signal-major: ``numpy.fft.rfft(w * sliding_window_view(x, n, axis=-1)[:, ::hop], axis=-1)``.  ``Spectrum`` stores rows of
``M + 1`` complex64, ``Power`` rows of ``M + 1`` float32, ``re**2 + im**2`` of the same bins.  ``window`` is a buffer of ``n``
float32 or ``None`` (rectangular); it is read on every exec.  The classes mirror ``fft_wgpu_amd.real``
(``X(device, queue, src, dst, fft_len, hop, signal_len, window=None)``, ``X.proc(encoder) -> Buffer``); the result is always
``dst``, and ``src`` and ``window`` are never written.

The ctypes table of the ``fwt_`` functions lives here.  ``libfft_wgpu_amd_stft.so`` is loaded on first use, not when the
package is imported, and there is no fallback: a missing library or a failing call raises.
"""
import ctypes
import os

from . import _ffi, _side
from ._ffi import _I32, _P, _PI32, _PI64, _PP, _PU64, _U32, _U64

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfft_wgpu_amd_stft.so")
ABI_VERSION = 1   # FWT_ABI_VERSION of the include/fft_wgpu_amd_stft.h this binding was written against
SPECTRUM, POWER = 0, 1   # FWT_SPECTRUM, FWT_POWER

_SIGNATURES = {
    "fwt_abi_version": (_I32, []),
    "fwt_describe": (_I32, [_U32, _U32, _U64, _U64, _PU64, _PI32, _PI32, _PI32, _PU64]),
    "fwt_plan_create": (_I32, [_P, _I32, _U32, _U32, _U64, _P, _P, _P, _PP]),
    "fwt_plan_exec": (_I32, [_P, _P]),
    "fwt_plan_get_i64": (_I32, [_P, ctypes.c_char_p, _PI64]),
    "fwt_plan_destroy": (_I32, [_P]),
}

_lib = None


def lib():
    """Load libfft_wgpu_amd_stft.so (once), after the main library, which it links against.  Raises if it was not built or reports
    another ABI version."""
    global _lib
    if _lib is None:
        _lib = _ffi.load(LIB_PATH, "fwt", ABI_VERSION, _SIGNATURES, "fft_wgpu_amd_stft.h", "make -C fft_wgpu_amd/stft",
                         needs=_ffi.lib)
    return _lib


def describe(fft_len, hop, signal_len, signals=1):
    """What a plan of this length launches over ``signals`` signals of ``signal_len`` samples at this hop -- pure host logic,
    no GPU needed: {"frames_per_signal", "threads", "lds_bytes", "frames_per_block", "blocks"}."""
    per, threads, lds, rows, blocks = _U64(), _I32(), _I32(), _I32(), _U64()
    _ffi.check(lib().fwt_describe(fft_len, hop, signal_len, signals, ctypes.byref(per), ctypes.byref(threads), ctypes.byref(lds),
                                  ctypes.byref(rows), ctypes.byref(blocks)), None, "fwt_describe")
    return {"frames_per_signal": per.value, "threads": threads.value, "lds_bytes": lds.value, "frames_per_block": rows.value,
            "blocks": blocks.value}


class _Plan(_side.Plan):
    _prefix = "fwt"
    _output = None

    def __init__(self, device, queue, src, dst, fft_len, hop, signal_len, window=None):
        self.src = src
        self.dst = dst
        self.window = window
        self.fft_len = fft_len
        self.hop = hop
        self.signal_len = signal_len
        self._create(lib(), device, queue, dst, device._h, self._output, fft_len, hop, signal_len, src._h,
                     window._h if window is not None else None, dst._h)


class Spectrum(_Plan):
    """numpy.fft.rfft of every windowed frame: n / 2 + 1 complex64 per frame."""
    _output = SPECTRUM


class Power(_Plan):
    """re**2 + im**2 of numpy.fft.rfft of every windowed frame: n / 2 + 1 float32 per frame."""
    _output = POWER
